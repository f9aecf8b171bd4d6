"""adh_batch_nhhaze_from_u8 (csrc/dataset.hip) without a GPU: the source file compiled by the host C++ compiler against
tools/host_emu with AddressSanitizer, UndefinedBehaviorSanitizer and float-cast-overflow and run as a stand-alone program
(tools/host_emu/dataset_main.cpp, call 6) over the table of tests/_nhhaze_ref64.py.  Nothing is loaded into Python.  Checked per
case, with a depth map and radial, with and without rows: the float64 bound, a second call, window geometry against dense geometry
on a dense copy, each sample alone, the inputs unchanged and the outputs fully written behind a poisoned front; and bit for bit
  (a) s = 0 with equal channels          == adh_batch_haze_from_u8 (call 5) with (beta, A)
  (b) s = 0, chromatic, no rows: plane c == plane c of adh_batch_haze_from_u8 with (beta_c, A_c)
  (c) a window at (y0, x0) with origin o + (y0, x0) == those pixels of the whole image with origin o (depth map, no rows)
  (d) beta_c = 0                         == adh_batch_window_from_u8 (call 3)
then the extremes and every refusal."""
import numpy as np
import pytest
import torch

from tests import _dataset_window_cases as K
from tests import _haze_synth_ref64 as Z
from tests import _hostemu as E
from tests import _nhhaze_ref64 as NH

NUM_BLOCKS, WINDOW, HAZE, NHHAZE = 1, 3, 5, 6
CPU_CASES = [(no, c) for no, c in enumerate(NH.CASES) if not c["gpu_only"]]
RANGE = (0.3, 1.0)


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    d = tmp_path_factory.mktemp("nhhaze_emu")
    exe = E.build(d, "dataset", "dataset_main.cpp", sanitize=E.FLOAT_CAST)
    return lambda: E.Script(exe, d)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _i64(s, a):
    return s.vec(torch.from_numpy(np.ascontiguousarray(a, dtype=np.int64)), np.int64)


def _f32(s, a):
    return s.vec(torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)))


def _f64(s, a):
    return s.vec(torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)), np.float64)


def _ro(s, arr, off=0):
    """a read-only block of exactly `off` filler bytes and the array's bytes; the entry point gets block + off"""
    a = np.ascontiguousarray(arr).view(np.uint8).reshape(-1)
    k = s.raw(np.concatenate([np.full(off, 0x5C, np.uint8), a]), off)
    s.ro.append(k)
    return k


def _nblk(px):
    return max(1, min(-(-px // 4096), 128))


@pytest.mark.parametrize("radial", [False, True], ids=["depth", "radial"])
@pytest.mark.parametrize("no,case", CPU_CASES, ids=[c["name"] for _, c in CPU_CASES])
def test_nhhaze(emu, no, case, radial):
    clear, depth, geom, dclear, ddepth, fog, fog6, field = NH.build(case)
    (CH, CW), out_off = case["crop"], case["out_off"]
    N, px = len(geom), CH * CW
    nblk = _nblk(px)
    s = emu()
    ck = _ro(s, clear, case["base"])
    dk = None if radial else _ro(s, depth, case["dbase"])
    dck = _ro(s, dclear)
    ddk = None if radial else _ro(s, ddepth)
    gk, dgk, wk = _i64(s, geom), _i64(s, Z.dense_geom(N, CH, CW)), _i64(s, geom[:, :2])
    flat = field.copy()
    flat[:, 4] = 0.0                                                  # s = 0
    zero6 = fog6.copy()
    zero6[:, :3] = 0.0                                                # beta_c = 0
    f6k, qk, q0k, g6k, z6k, f2k = _f32(s, fog6), _f64(s, field), _f64(s, flat), _f32(s, NH.grey(fog)), _f32(s, zero6), _f32(s, fog)
    chan = [_f32(s, fog6[:, [c, 3 + c]]) for c in range(3)]
    cb, db = clear.size, 0 if radial else depth.size * 2
    ints = (cb, db, N, CH, CW, nblk)
    nb = s.call(NUM_BLOCKS, (px,))

    def out():                                                        # `out_off` poison floats in front, checked after the run
        k = s.raw(np.full(out_off + N * 3 * px, E.WPOISON, np.uint32), out_off * 4)
        s.checks.append((k, np.arange(out_off), E.WPOISON, "the floats in front of the output"))
        return k

    runs = []
    for params in [None] + K.param_sets(no + int(radial), N, 1):
        pk = None if params is None else _f32(s, params)
        P = (lambda n=N: None) if params is None else (lambda n=N: s.out(n * nblk, np.float64))
        got, again, dense, a_new, a_old, d_new, d_old = out(), out(), s.out(N * 3 * px), out(), out(), out(), out()
        p0, p1 = P(), P()
        s.call(NHHAZE, ints, (ck, dk, gk, f6k, qk, pk, p0, got), RANGE)
        s.call(NHHAZE, ints, (ck, dk, gk, f6k, qk, pk, P(), again), RANGE)
        s.call(NHHAZE, (px * 3 * N, 0 if radial else px * 2 * N, N, CH, CW, nblk), (dck, ddk, dgk, f6k, qk, pk, p1, dense), RANGE)
        s.call(NHHAZE, ints, (ck, dk, gk, g6k, q0k, pk, P(), a_new), RANGE)                  # (a)
        s.call(HAZE, ints, (ck, dk, gk, f2k, pk, P(), a_old), RANGE)
        s.call(NHHAZE, ints, (ck, dk, gk, z6k, qk, pk, P(), d_new), RANGE)                   # (d)
        s.call(WINDOW, (cb, N, CH, CW, nblk), (ck, wk, pk, P(), d_old))
        b_new, b_old = None, []
        if params is None:                                                                   # (b)
            b_new = out()
            s.call(NHHAZE, ints, (ck, dk, gk, f6k, q0k, None, None, b_new), RANGE)
            for c in range(3):
                b_old.append(out())
                s.call(HAZE, ints, (ck, dk, gk, chan[c], None, None, b_old[-1]), RANGE)
        alone = []
        for n in range(N if N > 1 else 0):                            # each sample alone
            p1n = None if params is None else _f32(s, params[n:n + 1])
            o1 = s.out(3 * px)
            s.call(NHHAZE, (cb, db, 1, CH, CW, nblk), (ck, dk, _i64(s, geom[n:n + 1]), _f32(s, fog6[n:n + 1]),
                                                       _f64(s, field[n:n + 1]), p1n, P(1), o1), RANGE)
            alone.append(o1)
        runs.append((params, got, again, dense, a_new, a_old, d_new, d_old, b_new, b_old, alone, p0, p1))
    rcs = s.run()                                                     # also: every input unchanged, the front poison intact
    assert rcs[nb] == nblk and all(r == 0 for k, r in enumerate(rcs) if k != nb), rcs
    shape = (N, 3, CH, CW)

    def read(k, what):
        t = s.get(k)[out_off:]
        E.assert_written(t, f"{case['name']} {what}")
        return t.numpy().reshape(shape)
    for params, got, again, dense, a_new, a_old, d_new, d_old, b_new, b_old, alone, p0, p1 in runs:
        g = read(got, "out")
        assert np.array_equal(_bits(g), _bits(read(again, "again"))), "a second call differs"
        assert np.array_equal(_bits(g), _bits(s.get(dense).numpy().reshape(shape))), "differs from dense geometry on a dense copy"
        assert np.array_equal(_bits(read(a_new, "a")), _bits(read(a_old, "a old"))), "(a) s = 0, equal channels differs from the uniform entry"
        assert np.array_equal(_bits(read(d_new, "d")), _bits(read(d_old, "d old"))), "(d) beta = 0 differs from the clear window"
        if b_new is not None:
            bn = read(b_new, "b")
            for c in range(3):
                assert np.array_equal(_bits(bn[:, c]), _bits(read(b_old[c], "b old")[:, c])), f"(b) plane {c} differs"
        for n, o1 in enumerate(alone):
            assert np.array_equal(_bits(g[n]), _bits(s.get(o1).numpy().reshape(3, CH, CW))), f"sample {n} alone differs"
        ref = NH.nhhaze_ref(dclear, None if radial else ddepth, fog6, field, RANGE, params)
        err = float(np.abs(g.astype(np.float64) - ref).max())
        bound = NH.NH_BOUND if params is None else NH.NH_AUG_BOUND
        print(f"{case['name']} radial={radial} rows={params is not None}: max err {err / E.EPS:.3f} * 2^-24, bound {bound / E.EPS:.3f}")
        assert g.min() >= 0.0 and g.max() <= 1.0
        assert err <= bound
        if params is not None:
            assert np.array_equal(s.get(p0, np.float64).numpy().view(np.uint64), s.get(p1, np.float64).numpy().view(np.uint64)), \
                "the partial sums differ from those of the dense copy"


@pytest.mark.parametrize("no,case", [(no, c) for no, c in CPU_CASES if c["name"] in ("5x7_bytes", "8x12_phases", "40x130")],
                         ids=["5x7_bytes", "8x12_phases", "40x130"])
def test_crop_sees_the_image_field(emu, no, case):
    """(c): every window of the case against the same pixels of its whole image, whose origin is the row's and the window's that
    plus (y0, x0)"""
    clear, depth, geom, dclear, ddepth, fog, fog6, field = NH.build(case)
    CH, CW = case["crop"]
    s = emu()
    ck, dk = _ro(s, clear, case["base"]), _ro(s, depth, case["dbase"])
    jobs = []
    for n, (k, y0, x0) in enumerate(case["windows"]):
        h, w = case["images"][k]
        whole = field[n:n + 1].copy()                                 # the image's own origin: the table's, some near 2^20
        row = whole.copy()
        row[0, 1:3] += (y0, x0)
        gw = geom[n:n + 1].copy()
        gi = gw - np.array([[(y0 * w + x0) * 3, 0, (y0 * w + x0) * 2, 0]])
        ow, oi = s.out(3 * CH * CW), s.out(3 * h * w)
        f6 = _f32(s, fog6[n:n + 1])
        s.call(NHHAZE, (clear.size, depth.size * 2, 1, CH, CW, _nblk(CH * CW)), (ck, dk, _i64(s, gw), f6, _f64(s, row), None, None, ow), RANGE)
        s.call(NHHAZE, (clear.size, depth.size * 2, 1, h, w, _nblk(h * w)), (ck, dk, _i64(s, gi), f6, _f64(s, whole), None, None, oi), RANGE)
        jobs.append((ow, oi, h, w, y0, x0))
    assert all(r == 0 for r in s.run())
    for ow, oi, h, w, y0, x0 in jobs:
        win, img = s.get(ow).numpy().reshape(3, CH, CW), s.get(oi).numpy().reshape(3, h, w)
        assert np.array_equal(_bits(win), _bits(img[:, y0:y0 + CH, x0:x0 + CW]))


@pytest.mark.parametrize("rows", [False, True], ids=["plain", "rows"])
def test_extremes_stay_in_range(emu, rows):
    """clear 0 and 255 under depth 0 and 65535 with s = 0.99 and beta = 1; A = 0 and A = 1: inside [0, 1] and within the bound"""
    CH, CW, N = 4, 8, 2
    clear = np.zeros((N, CH, CW, 3), np.uint8)
    clear[:, :, 4:] = 255
    depth = np.zeros((N, CH, CW), np.uint16)
    depth[:, 2:] = 65535
    fog6 = np.array([[1, 1, 1, 1, 1, 1], [1, 1, 1, 0, 0, 0]], np.float32)
    field = np.array([[5, 0, 0, 2, 0.99, 0.25], [6, 3, 1, 2, 0.99, 0.25]], np.float64)
    params = np.array([[1, 0, 1, 1.1, 1.1], [0, 1, 0, 0.9, 1.1]], np.float32) if rows else None
    s = emu()
    o1, o2 = s.out(N * 3 * CH * CW), s.out(N * 3 * CH * CW)
    pk = None if params is None else _f32(s, params)
    gk, fk, qk = _i64(s, Z.dense_geom(N, CH, CW)), _f32(s, fog6), _f64(s, field)
    P = lambda: s.out(N, np.float64) if rows else None      # noqa: E731
    s.call(NHHAZE, (clear.size, depth.size * 2, N, CH, CW, 1), (_ro(s, clear), _ro(s, depth), gk, fk, qk, pk, P(), o1), RANGE)
    s.call(NHHAZE, (clear.size, 0, N, CH, CW, 1), (_ro(s, clear), None, gk, fk, qk, pk, P(), o2), RANGE)
    assert s.run() == [0, 0]
    for o, d in ((o1, depth), (o2, None)):
        g = s.get(o)
        E.assert_written(g, "extremes")
        g = g.numpy().reshape(N, 3, CH, CW)
        assert g.min() >= 0.0 and g.max() <= 1.0
        assert np.abs(g - NH.nhhaze_ref(clear, d, fog6, field, RANGE, params)).max() <= (NH.NH_AUG_BOUND if rows else NH.NH_BOUND)


def test_refusals(emu):
    s = emu()
    CH, CW, N = 3, 5, 2
    clear = s.vec(torch.zeros(64, dtype=torch.uint8), np.uint8)
    depth = s.vec(torch.zeros(44, dtype=torch.uint8), np.uint8)
    odd = _ro(s, np.zeros(44, np.uint8), 1)
    geom = _i64(s, [[0, 15, 0, 10], [4, 15, 2, 10]])
    fog = _f32(s, [[0.5, 0.6, 0.7, 0.8, 0.8, 0.9]] * N)
    field = _f64(s, [[1, 0, 0, 2, 0.5, 0.25]] * N)
    par = _f32(s, [[0, 0, 0, 1, 1]] * N)
    partial, out = s.out(N, np.float64), s.out(N * 3 * CH * CW)
    bufs = (clear, depth, geom, fog, field, par, partial, out)
    bad = []
    for ints in ((64, 44, 0, CH, CW, 1), (64, 44, 65536, CH, CW, 1), (64, 44, -1, CH, CW, 1), (64, 44, N, 0, CW, 1),
                 (64, 44, N, CH, 0, 1), (64, 44, N, -1, CW, 1), (44, 44, N, CH, CW, 1), (-4, 44, N, CH, CW, 1), (64, 29, N, CH, CW, 1),
                 (64, -2, N, CH, CW, 1), (64, 44, N, CH, CW, 2), (64, 44, N, CH, CW, 0),
                 (2 ** 62, 2 ** 62, N, 2 ** 31 - 1, 2 ** 31 - 1, 128)):      # CH * CW * 3 overflows
        bad.append(s.call(NHHAZE, ints, bufs, RANGE))
    for k in (0, 2, 3, 4, 6, 7):                                      # clear, geom, fog, field, partial (with params), out
        b = list(bufs)
        b[k] = None
        bad.append(s.call(NHHAZE, (64, 44, N, CH, CW, 1), b, RANGE))
    bad.append(s.call(NHHAZE, (64, 44, N, CH, CW, 1), (clear, odd, geom, fog, field, par, partial, out), RANGE))
    rcs = s.run()
    assert [rcs[k] for k in bad] == [E.ADH_E_ARG] * len(bad), rcs
    assert s.unchanged(out) and s.unchanged(partial)
    s = emu()                                                         # params NULL needs no partial, radial needs no depth
    clear = s.vec(torch.zeros(45, dtype=torch.uint8), np.uint8)
    out = s.out(3 * CH * CW)
    good = s.call(NHHAZE, (45, 0, 1, CH, CW, 1), (clear, None, _i64(s, [[0, 15, 0, 0]]), _f32(s, [[0, 0, 0, 1, 1, 1]]),
                                                  _f64(s, [[1, 0, 0, 1, 0.5, 0.5]]), None, None, out), RANGE)
    assert s.run()[good] == 0 and (s.get(out).numpy() == 0).all()
