"""adh_batch_haze_from_u8 and adh_u16_resize_bilinear (csrc/dataset.hip) without a GPU: the source file compiled by the host C++
compiler against tools/host_emu with AddressSanitizer and UndefinedBehaviorSanitizer and run as a stand-alone program
(tools/host_emu/dataset_main.cpp, calls 4 and 5) over the table of tests/_haze_synth_ref64.py.  Both caches are heap blocks of
exactly base + bytes, so a read in front of them or behind them -- the aligned dwords around a quad that starts off phase are the
ones to watch -- is the sanitizer's to report.  Checked: the inputs unchanged, the outputs fully written, the float64 bound with
and without rows, with a depth map and radial, beta = 0 against adh_batch_window_from_u8 (call 3), window geometry against dense
geometry on a dense copy, each sample alone and a second call, the extremes, every refusal, and the 16-bit resize."""
import numpy as np
import pytest
import torch

from tests import _dataset_window_cases as K
from tests import _haze_synth_ref64 as Z
from tests import _hostemu as E

NUM_BLOCKS, WINDOW, RESIZE16, HAZE = 1, 3, 4, 5
CPU_CASES = [(no, c) for no, c in enumerate(Z.CASES) if not c["gpu_only"]]
RANGE = (0.3, 1.0)


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    d = tmp_path_factory.mktemp("haze_synth_emu")
    exe = E.build(d, "dataset", "dataset_main.cpp", sanitize=E.FLOAT_CAST)
    return lambda: E.Script(exe, d)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _i64(s, a):
    return s.vec(torch.from_numpy(np.ascontiguousarray(a, dtype=np.int64)), np.int64)


def _ro(s, arr, off=0):
    """a read-only block of exactly `off` filler bytes and the array's bytes; the entry point gets block + off"""
    a = np.ascontiguousarray(arr).view(np.uint8).reshape(-1)
    k = s.raw(np.concatenate([np.full(off, 0x5C, np.uint8), a]), off)
    s.ro.append(k)
    return k


@pytest.mark.parametrize("radial", [False, True], ids=["depth", "radial"])
@pytest.mark.parametrize("no,case", CPU_CASES, ids=[c["name"] for _, c in CPU_CASES])
def test_haze(emu, no, case, radial):
    clear, depth, geom, dclear, ddepth, fog = Z.build(case)
    (CH, CW), out_off = case["crop"], case["out_off"]
    N, px = len(geom), CH * CW
    nblk = max(1, min(-(-px // 4096), 128))
    s = emu()
    ck = _ro(s, clear, case["base"])
    dk = None if radial else _ro(s, depth, case["dbase"])
    dck = _ro(s, dclear)
    ddk = None if radial else _ro(s, ddepth)
    gk, dgk = _i64(s, geom), _i64(s, Z.dense_geom(N, CH, CW))
    wk = _i64(s, geom[:, :2])
    fk = s.vec(torch.from_numpy(fog))
    f0 = fog.copy()
    f0[:, 0] = 0.0
    f0k = s.vec(torch.from_numpy(f0))
    cb, db = clear.size, 0 if radial else depth.size * 2
    nb = s.call(NUM_BLOCKS, (px,))

    def out():                                                        # `out_off` poison floats in front, checked after the run
        k = s.raw(np.full(out_off + N * 3 * px, E.WPOISON, np.uint32), out_off * 4)
        s.checks.append((k, np.arange(out_off), E.WPOISON, "the floats in front of the output"))
        return k

    def part(n=N):
        return s.out(n * nblk, np.float64)
    runs = []
    for params in [None] + K.param_sets(no + int(radial), N, 1):
        pk = None if params is None else s.vec(torch.from_numpy(params))
        P = (lambda n=N: None) if params is None else part
        got, again, dense, zero, plain = out(), out(), s.out(N * 3 * px), out(), out()
        p0, p1 = P(), P()
        s.call(HAZE, (cb, db, N, CH, CW, nblk), (ck, dk, gk, fk, pk, p0, got), RANGE)
        s.call(HAZE, (cb, db, N, CH, CW, nblk), (ck, dk, gk, fk, pk, P(), again), RANGE)
        s.call(HAZE, (px * 3 * N, 0 if radial else px * 2 * N, N, CH, CW, nblk), (dck, ddk, dgk, fk, pk, p1, dense), RANGE)
        s.call(HAZE, (cb, db, N, CH, CW, nblk), (ck, dk, gk, f0k, pk, P(), zero), RANGE)
        s.call(WINDOW, (cb, N, CH, CW, nblk), (ck, wk, pk, P(), plain))
        alone = []
        for n in range(N if N > 1 else 0):                            # each sample alone
            p1n = None if params is None else s.vec(torch.from_numpy(params[n:n + 1]))
            o1 = s.out(3 * px)
            s.call(HAZE, (cb, db, 1, CH, CW, nblk), (ck, dk, _i64(s, geom[n:n + 1]), s.vec(torch.from_numpy(fog[n:n + 1])), p1n,
                                                     P(1), o1), RANGE)
            alone.append(o1)
        runs.append((params, got, again, dense, zero, plain, alone, p0, p1))
    rcs = s.run()                                                     # also: every input unchanged, the front poison intact
    assert rcs[nb] == nblk and all(r == 0 for k, r in enumerate(rcs) if k != nb), rcs
    for params, got, again, dense, zero, plain, alone, p0, p1 in runs:
        g = s.get(got)[out_off:]
        E.assert_written(g, case["name"])
        g = g.numpy().reshape(N, 3, CH, CW)
        assert np.array_equal(_bits(g), _bits(s.get(again)[out_off:].numpy().reshape(g.shape))), "a second call differs"
        assert np.array_equal(_bits(g), _bits(s.get(dense).numpy().reshape(g.shape))), "differs from dense geometry on a dense copy"
        z = s.get(zero)[out_off:]
        E.assert_written(z, case["name"] + " beta 0")
        assert np.array_equal(_bits(z.numpy()), _bits(s.get(plain)[out_off:].numpy())), "beta = 0 differs from the clear window"
        for n, o1 in enumerate(alone):
            assert np.array_equal(_bits(g[n]), _bits(s.get(o1).numpy().reshape(3, CH, CW))), f"sample {n} alone differs"
        ref = Z.haze_ref(dclear, None if radial else ddepth, fog, RANGE, params)
        err = float(np.abs(g.astype(np.float64) - ref).max())
        bound = Z.HAZE_BOUND if params is None else Z.HAZE_AUG_BOUND
        print(f"{case['name']} radial={radial} rows={params is not None}: max err {err / E.EPS:.3f} * 2^-24, bound {bound / E.EPS:.3f}")
        assert g.min() >= 0.0 and g.max() <= 1.0
        assert err <= bound
        if params is not None:
            assert np.array_equal(s.get(p0, np.float64).numpy().view(np.uint64), s.get(p1, np.float64).numpy().view(np.uint64)), \
                "the partial sums differ from those of the dense copy"


@pytest.mark.parametrize("rows", [False, True], ids=["plain", "rows"])
def test_extremes_stay_in_range(emu, rows):
    """clear 0 and 255 under depth 0 and 65535 with A = 1, beta = 1: inside [0, 1], and within the bound"""
    CH, CW, N = 4, 8, 1
    clear = np.zeros((N, CH, CW, 3), np.uint8)
    clear[:, :, 4:] = 255
    depth = np.zeros((N, CH, CW), np.uint16)
    depth[:, 2:] = 65535
    fog = np.array([[1.0, 1.0]], np.float32)
    params = np.array([[1, 0, 1, 1.1, 1.1]], np.float32) if rows else None
    s = emu()
    o1, o2 = s.out(N * 3 * CH * CW), s.out(N * 3 * CH * CW)
    pk = None if params is None else s.vec(torch.from_numpy(params))
    gk, fk = _i64(s, Z.dense_geom(N, CH, CW)), s.vec(torch.from_numpy(fog))
    ints = (clear.size, depth.size * 2, N, CH, CW, 1)
    s.call(HAZE, ints, (_ro(s, clear), _ro(s, depth), gk, fk, pk, s.out(N, np.float64) if rows else None, o1), RANGE)
    s.call(HAZE, (clear.size, 0, N, CH, CW, 1), (_ro(s, clear), None, gk, fk, pk, s.out(N, np.float64) if rows else None, o2), RANGE)
    assert s.run() == [0, 0]
    for o, d in ((o1, depth), (o2, None)):
        g = s.get(o)
        E.assert_written(g, "extremes")
        g = g.numpy().reshape(N, 3, CH, CW)
        assert g.min() >= 0.0 and g.max() <= 1.0
        assert np.abs(g - Z.haze_ref(clear, d, fog, RANGE, params)).max() <= (Z.HAZE_AUG_BOUND if rows else Z.HAZE_BOUND)


def test_refusals(emu):
    s = emu()
    CH, CW, N = 3, 5, 2
    clear = s.vec(torch.zeros(64, dtype=torch.uint8), np.uint8)
    depth = s.vec(torch.zeros(44, dtype=torch.uint8), np.uint8)
    odd = _ro(s, np.zeros(44, np.uint8), 1)
    geom = _i64(s, [[0, 15, 0, 10], [4, 15, 2, 10]])
    fog = s.vec(torch.tensor([[0.5, 0.8]] * N, dtype=torch.float32))
    par = s.vec(torch.tensor([[0, 0, 0, 1, 1]] * N, dtype=torch.float32))
    partial, out = s.out(N, np.float64), s.out(N * 3 * CH * CW)
    bufs = (clear, depth, geom, fog, par, partial, out)
    bad = []
    for ints in ((64, 44, 0, CH, CW, 1), (64, 44, 65536, CH, CW, 1), (64, 44, -1, CH, CW, 1), (64, 44, N, 0, CW, 1),
                 (64, 44, N, CH, 0, 1), (64, 44, N, -1, CW, 1), (44, 44, N, CH, CW, 1), (-4, 44, N, CH, CW, 1), (64, 29, N, CH, CW, 1),
                 (64, -2, N, CH, CW, 1), (64, 44, N, CH, CW, 2), (64, 44, N, CH, CW, 0),
                 (2 ** 62, 2 ** 62, N, 2 ** 31 - 1, 2 ** 31 - 1, 128)):      # CH * CW * 3 overflows
        bad.append(s.call(HAZE, ints, bufs, RANGE))
    for b in ((None, depth, geom, fog, par, partial, out), (clear, depth, None, fog, par, partial, out),
              (clear, depth, geom, None, par, partial, out), (clear, depth, geom, fog, par, None, out),
              (clear, depth, geom, fog, par, partial, None), (clear, odd, geom, fog, par, partial, out)):
        bad.append(s.call(HAZE, (64, 44, N, CH, CW, 1), b, RANGE))
    # the 16-bit resize: sizes, bytes_per_px, pitch, null pointers, odd addresses
    src, dst = s.vec(torch.zeros(48, dtype=torch.uint8), np.uint8), s.out(4, np.uint16)
    osrc, odst = _ro(s, np.zeros(48, np.uint8), 1), s.raw(np.full(9, 0x5A, np.uint8), 1)
    for ints, b in (((8, 0, 4, 2, 2, 2), (src, dst)), ((8, 4, 0, 2, 2, 2), (src, dst)), ((8, 4, 4, 2, 0, 2), (src, dst)),
                    ((8, 4, 4, 2, 2, 0), (src, dst)), ((8, 4, 4, 3, 2, 2), (src, dst)), ((8, 4, 4, 0, 2, 2), (src, dst)),
                    ((7, 4, 4, 2, 2, 2), (src, dst)), ((3, 4, 4, 1, 2, 2), (src, dst)), ((9, 4, 4, 2, 2, 2), (src, dst)),
                    ((8, 4, 4, 2, 2, 2), (None, dst)), ((8, 4, 4, 2, 2, 2), (src, None)), ((8, 4, 4, 2, 2, 2), (osrc, dst)),
                    ((8, 4, 4, 2, 2, 2), (src, odst))):
        bad.append(s.call(RESIZE16, ints, b))
    rcs = s.run()
    assert [rcs[k] for k in bad] == [E.ADH_E_ARG] * len(bad), rcs
    assert s.unchanged(out) and s.unchanged(partial) and s.unchanged(dst) and s.unchanged(odst)
    s = emu()                                                         # params NULL needs no partial, radial needs no depth
    clear = s.vec(torch.zeros(45, dtype=torch.uint8), np.uint8)
    out = s.out(3 * CH * CW)
    good = s.call(HAZE, (45, 0, 1, CH, CW, 1), (clear, None, _i64(s, [[0, 15, 0, 0]]),
                                                s.vec(torch.tensor([[0.0, 1.0]], dtype=torch.float32)), None, None, out), RANGE)
    assert s.run()[good] == 0 and (s.get(out).numpy() == 0).all()


def _resize16(emu, src, OH, OW, off=0, slack=0):
    """call 4 on a source with `slack` bytes of pitch padding, `off` bytes into its block; returns uint16 [OH, OW]"""
    h, w = src.shape
    bpp = src.dtype.itemsize
    rows = np.full((h, w * bpp + slack), 0xEE, np.uint8)
    rows[:, :w * bpp] = np.ascontiguousarray(src).view(np.uint8).reshape(h, w * bpp)
    flat = rows.reshape(-1)[:rows.size - slack]                       # the block ends with the last row's last level
    s = emu()
    k, dst = _ro(s, flat, off), s.out(OH * OW, np.uint16)
    rc = s.call(RESIZE16, (w * bpp + slack, h, w, bpp, OH, OW), (k, dst))
    assert s.run()[rc] == 0
    return s.get(dst, np.uint16).numpy().reshape(OH, OW)


@pytest.mark.parametrize("size,out", Z.RESIZE16_CASES, ids=[f"{h}x{w}" for (h, w), _ in Z.RESIZE16_CASES])
def test_resize16(emu, size, out):
    rng = np.random.RandomState(size[0] * 100 + size[1])
    src = rng.randint(0, 65536, size=size).astype(np.uint16)
    src.reshape(-1)[:2] = (0, 65535)[:min(2, src.size)]
    Z.check_resize16(_resize16(emu, src, *out, off=2, slack=2), src, *out, what="16-bit")
    src8 = rng.randint(0, 256, size=size).astype(np.uint8)
    Z.check_resize16(_resize16(emu, src8, *out, off=1, slack=1), src8.astype(np.uint16) * 257, *out, what="8-bit")


@pytest.mark.parametrize("size,out", Z.RESIZE16_DYADIC, ids=[f"{h}x{w}" for (h, w), _ in Z.RESIZE16_DYADIC])
def test_resize16_exact(emu, size, out):
    rng = np.random.RandomState(size[0] + size[1])
    src = rng.randint(0, 65536, size=size).astype(np.uint16)
    Z.check_resize16(_resize16(emu, src, *out), src, *out, exact=True, what="dyadic")
    src8 = rng.randint(0, 256, size=size).astype(np.uint8)
    got8 = _resize16(emu, src8, *out, off=3)
    Z.check_resize16(got8, src8.astype(np.uint16) * 257, *out, exact=True, what="dyadic 8-bit")
    if size == out:                                                   # same size: an exact copy, the promotion v * 257
        assert np.array_equal(_resize16(emu, src, *out), src) and np.array_equal(got8, src8.astype(np.uint16) * 257)
