"""csrc/train_io.hip without a GPU: the source file, compiled by the host C++ compiler against the stand-in header of tools/host_emu
(its ADH_HOST_EMU_STREAM section: the float64 butterflies of the two-stage sums run on the emulator's __shfl_xor(double)) with
AddressSanitizer and UndefinedBehaviorSanitizer, run as a stand-alone program on heap blocks of exactly their sizes
(tests/_hostemu.py) and held to the float64 restatements and bounds of tests/_ref64.py, the ones tests/test_gpu_train_io.py holds
the library to.  Nothing is loaded into Python.

Two programs are built: "lib" with the grid caps the library has, and "small" with the caps of SMALL_CAPS, under which a few
hundred elements run every grid-stride loop more than once and every partial row over more than one block.  The Adam table, the
chunk list, the float64 partials and the control block are blocks of exactly their bytes; a tensor at float offset 1 of its block
is off 16-byte alignment (the kernels' scalar paths) behind one poison float that is checked afterwards.  Every call is made twice,
on outputs of its own, and the two must agree bit for bit; inputs come back unchanged; no output may still hold its poison."""
import math
import os
import re
import struct

import numpy as np
import pytest
import torch

from tests import _hostemu as E
from tests import _ref64 as R64

EPS, U53 = E.EPS, 2.0 ** -53
ENTRY_POINTS = ["adh_adam_chunk_elems", "adh_adam_multi", "adh_grad_sumsq", "adh_grad_guard_finalize", "adh_adam_multi_guarded",
                "adh_apply_fog", "adh_psnr_num_blocks", "adh_psnr", "adh_ssim_num_blocks", "adh_ssim_gray", "adh_augment_num_blocks",
                "adh_paired_augment"]
(CHUNK_ELEMS, ADAM_MULTI, GRAD_SUMSQ, GUARD_FINALIZE, ADAM_GUARDED, FOG, PSNR_NB, PSNR, SSIM_NB, SSIM, AUG_NB,
 AUGMENT) = range(12)                                                                 # tools/host_emu/train_io_main.cpp
LIB_CAPS = dict(TIO_MAXBLK_PIXELS=2048, PSNR_ELEMS_PER_BLOCK=8192, PSNR_MAXBLK=1024, AUG_ELEMS_PER_BLOCK=4096, AUG_MAXBLK=256)
SMALL_CAPS = dict(TIO_MAXBLK_PIXELS=2, PSNR_ELEMS_PER_BLOCK=512, PSNR_MAXBLK=3, AUG_ELEMS_PER_BLOCK=256, AUG_MAXBLK=2)
CAPS = {"lib": LIB_CAPS, "small": SMALL_CAPS}
BOTH = pytest.mark.parametrize("caps", ["lib", "small"])
CHUNK = 16384
ADH_E_UNSUPPORTED = -3
DPOISON = 0x7FF8DEADBEEF0000        # Script.out's fill of a float64 output


def test_every_entry_point_is_called():
    src = open(os.path.join(E.ROOT, "adam-dehaze_amd", "csrc", "train_io.hip")).read()
    assert re.findall(r'extern "C" int (adh_\w+)', src) == ENTRY_POINTS             # in the driver's order
    me = open(__file__).read()
    names = re.search(r"\(CHUNK_ELEMS,(.*?)\) = range", me, re.S).group(1).replace("\n", " ").split(",")
    for name in ["CHUNK_ELEMS"] + [n.strip() for n in names]:
        assert re.search(r"s\.call\(%s[,)]" % name, me), name


@pytest.fixture(scope="module")
def emus(tmp_path_factory):
    d = tmp_path_factory.mktemp("train_io_emu")
    exe = {"lib": E.build(d, "train_io", "train_io_main.cpp", sanitize=E.FLOAT_CAST, exe="emu_lib"),
           "small": E.build(d, "train_io", "train_io_main.cpp", [f"{k}={v}" for k, v in SMALL_CAPS.items()],
                            sanitize=E.FLOAT_CAST, exe="emu_small")}
    return lambda caps: E.Script(exe[caps], d)


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _rand(*shape, seed=0):
    return torch.rand(shape, dtype=torch.float32, generator=_gen(seed))


def _randn(*shape, seed=0):
    return torch.randn(shape, dtype=torch.float32, generator=_gen(seed))


def _cdiv(a, b):
    return -(-a // b)


def _psnr_nb(c, per):
    return max(1, min(_cdiv(per, c["PSNR_ELEMS_PER_BLOCK"]), c["PSNR_MAXBLK"]))


def _aug_nb(c, HW):
    return max(1, min(_cdiv(HW, c["AUG_ELEMS_PER_BLOCK"]), c["AUG_MAXBLK"]))


def _ssim_nb(Hh, Ww):
    return _cdiv(Hh - 6, 32) * _cdiv(Ww - 6, 32)


def _twice(s, runs):
    for k1, k2 in zip(*runs):
        if k1 is not None:
            assert (s.after[k1] == s.after[k2]).all(), "two identical calls differ"
    return runs[0]


def _getf(s, k, what="output"):
    t = s.get(k)
    E.assert_written(t, what)
    return t


def _getd(s, k, what="partials"):
    t = s.get(k, np.float64)
    assert not (t.view(torch.int64) == DPOISON).any(), f"{what}: elements still hold their poison"
    return t


def _ok(s):
    rcs = s.run()
    assert all(rc == 0 for rc in rcs), rcs


def _same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


@BOTH
def test_block_counts(emus, caps):
    """the block counts the other tests compute from the caps are the program's"""
    s, c = emus(caps), CAPS[caps]
    s.call(CHUNK_ELEMS)
    want = [CHUNK]
    for per in (1, 511, 512, 513, 8192, 8193, 1 << 24):
        s.call(PSNR_NB, [per])
        want.append(_psnr_nb(c, per))
    for HW in (1, 256, 257, 561, 4097, 1 << 22):
        s.call(AUG_NB, [HW])
        want.append(_aug_nb(c, HW))
    for Hh, Ww in ((7, 7), (39, 7), (45, 71), (6, 40), (40, 6)):
        s.call(SSIM_NB, [Hh, Ww])
        want.append(_ssim_nb(Hh, Ww) if min(Hh, Ww) >= 7 else 0)
    assert s.run() == want


# ------------------------------------------------------------------------------------------------ fog
@BOTH
def test_apply_fog(emus, caps):
    """one-pixel rows and columns (the W > 1 ? ... : 0 steps of the grid); 23 x 29 = 667 pixels: three blocks, and two trips under
    the small caps.  clear spans [-0.5, 1.5], so both clamps saturate; every (beta, airlight) pair of the lists runs."""
    s = emus(caps)
    betas, airs = [0.0, 0.15, 0.95, 3.0], [0.0, 0.6, 1.0]
    pairs = [(b, a) for b in betas for a in airs]
    cases = []
    for N, Hh, Ww in ((1, 1, 1), (2, 1, 9), (2, 9, 1), (3, 37, 5), (2, 23, 29)):
        HW = Hh * Ww
        clear = 2.0 * _rand(N, 3, Hh, Ww, seed=HW) - 0.5
        bclear = s.vec(clear)
        for k in range(0, len(pairs), N):
            sel = [pairs[(k + i) % len(pairs)] for i in range(N)]
            beta, air = torch.tensor([p[0] for p in sel]), torch.tensor([p[1] for p in sel])
            bb, ba = s.vec(beta), s.vec(air)
            runs = []
            for _ in range(2):
                out = s.out(N * 3 * HW)
                s.call(FOG, [N, Hh, Ww], [bclear, bb, ba, out])
                runs.append((out,))
            cases.append((clear, beta, air, runs))
    _ok(s)
    saturated = set()
    for clear, beta, air, runs in cases:
        (out,) = _twice(s, runs)
        out = _getf(s, out).view_as(clear)
        h = R64.fog(clear, beta, air)
        # one rounding of the float64 value to fp32 (half an ulp <= EPS |h|), then the clip (1-Lipschitz)
        E.assert_bound(out, h.clamp(0, 1), EPS * h.abs() + R64.FOG_F64_UNITS * U53 * (clear.double().abs() + 1), "fog")
        assert float(out.min()) >= 0.0 and float(out.max()) <= 1.0
        saturated |= {v for v in (0.0, 1.0) if bool((out == v).any())}
    assert saturated == {0.0, 1.0}, "the inputs were meant to saturate both clamps"


# ------------------------------------------------------------------------------------------------ PSNR
PSNR_PER = [1, 3, 4, 5, 147, 8191, 8192, 8193]


def _psnr_bufs(s, t, off):
    """t [N * per] at float offset `off` of a block of exactly off + N * per floats"""
    blk = np.full(off + t.numel(), E.RPOISON, np.uint32)
    blk[off:] = t.numpy().view(np.uint32)
    k = s.raw(blk, 4 * off)
    s.ro.append(k)
    return k


@BOTH
@pytest.mark.parametrize("N", [1, 3])
def test_psnr_vector_and_scalar_paths(emus, caps, N):
    """the same values at a 16-byte aligned base (the vector path when per % 4 == 0) and one float further (the scalar path; with
    N > 1 and per % 4 != 0 the images alternate alignment).  The blocks end with the last image.  mse null: not written."""
    s, c = emus(caps), CAPS[caps]
    cases = []
    for per in PSNR_PER:
        p, t = _rand(N * per, seed=per % 9973), _rand(N * per, seed=per % 9973 + 1)
        nblk = _psnr_nb(c, per)
        res = []
        for off in (0, 1):
            bp, bt = _psnr_bufs(s, p, off), _psnr_bufs(s, t, off)
            runs = []
            for _ in range(2):
                part, mse, psnr, part0, psnr0 = s.out(N * nblk, np.float64), s.out(N), s.out(N), s.out(N * nblk, np.float64), s.out(N)
                s.call(PSNR, [N, per, nblk], [bp, bt, part, mse, psnr], [1.0])
                s.call(PSNR, [N, per, nblk], [bp, bt, part0, None, psnr0], [1.0])
                runs.append((part, mse, psnr, part0, psnr0))
            res.append(runs)
        cases.append((p.view(N, per), t.view(N, per), per, nblk, res))
    _ok(s)
    for p, t, per, nblk, res in cases:
        ref = R64.mse(p, t)
        ref_db = 10.0 * torch.log10(1.0 / ref)
        sums = []
        for runs in res:
            part, mse, psnr, part0, psnr0 = _twice(s, runs)
            # mse: the sum is float64 of exact squares of fp32 differences; (a - b) in fp32 is within EPS relative, its square
            # within 2 EPS; one more rounding for the fp32 store
            E.assert_bound(_getf(s, mse), ref, (3 * EPS + R64.PSNR_F64_UNITS * U53) * ref, f"mse per={per}")
            # PSNR from the float64 mean (2 EPS relative): 10 / ln 10 * 2 EPS dB, then the fp32 store
            E.assert_bound(_getf(s, psnr), ref_db, 10 / math.log(10) * (2 * EPS + R64.PSNR_F64_UNITS * U53) + EPS * ref_db.abs(),
                           f"psnr per={per}")
            assert _same_bits(s.get(psnr), s.get(psnr0)), "psnr must not depend on mse being asked for"
            sums.append(_getd(s, part).view(N, nblk).sum(1))
            _getd(s, part0)
        rel = float(((sums[0] - sums[1]).abs() / sums[1]).max())
        assert rel <= 2.0 ** -50, "vector and scalar paths disagree on the same data"


def test_psnr_identical_inputs(emus):
    s = emus("lib")
    x = _rand(3 * 8193, seed=5)
    bx, by = s.vec(x), s.vec(x.clone())
    part, mse, psnr = s.out(3 * 2, np.float64), s.out(3), s.out(3)
    s.call(PSNR, [3, 8193, 2], [bx, by, part, mse, psnr], [1.0])
    _ok(s)
    mse, psnr = _getf(s, mse), _getf(s, psnr)
    assert (mse == 0).all() and torch.isinf(psnr).all() and (psnr > 0).all()


# ------------------------------------------------------------------------------------------------ SSIM
@pytest.mark.parametrize("kind", ["random", "constant", "two_constants", "negative"])
def test_ssim_gray(emus, kind):
    """39 = 32 + 7: the last tile is one output wide (39, 7), one high (7, 39), both (39, 39); the images are blocks of exactly
    their floats, so a halo read past the last row or column is the sanitizer's to report"""
    s, N = emus("lib"), 2
    cases = []
    for Hh, Ww in ((7, 7), (7, 39), (39, 7), (38, 38), (39, 39), (45, 71)):
        t = _rand(N, 3, Hh, Ww, seed=Hh * Ww)
        if kind == "random":
            p = (t + 0.1 * _randn(N, 3, Hh, Ww, seed=Hh + Ww)).clamp(0, 1)
        elif kind == "constant":
            t = torch.full_like(t, 0.3)
            p = t.clone()
        elif kind == "two_constants":
            t = torch.full_like(t, 0.3)
            p = torch.full_like(t, 0.8)
        else:
            p = 1.0 - t
        nblk = _ssim_nb(Hh, Ww)
        bp, bt = s.vec(p), s.vec(t)
        runs = []
        for _ in range(2):
            part, ssim = s.out(N * nblk, np.float64), s.out(N)
            s.call(SSIM, [N, Hh, Ww, nblk], [bp, bt, part, ssim], [1.0])
            runs.append((part, ssim))
        cases.append((p, t, runs))
    _ok(s)
    for p, t, runs in cases:
        part, ssim = _twice(s, runs)
        _getd(s, part)
        ref = R64.ssim_gray(p, t)
        # the grayscale is the same three fp32 operations on both sides; the window statistics are float64 (see the GPU test)
        E.assert_bound(_getf(s, ssim), ref, EPS * ref.abs() + 1e-10, f"ssim {kind} {tuple(p.shape)}")
        if kind == "constant":
            assert float((s.get(ssim) - 1).abs().max()) <= EPS


# ------------------------------------------------------------------------------------------------ paired augmentation
AUG_HW = [(17, 33), (1, 1), (1, 300), (300, 1)]


def _aug_case(s, c, x, params):
    N, _, Hh, Ww = x.shape
    nblk = _aug_nb(c, Hh * Ww)
    bx, bp = s.vec(x), s.vec(params)
    runs = []
    for _ in range(2):
        part, out = s.out(N * nblk, np.float64), s.out(N * 3 * Hh * Ww)
        s.call(AUGMENT, [N, Hh, Ww, nblk], [bx, bp, part, out])
        runs.append((part, out))
    return runs


@BOTH
def test_paired_augment(emus, caps):
    """all eight (flip_h, flip_v, brightness_first) combinations in every batch; 17 x 33 = 561 pixels: three blocks of the gather
    pass, and under the small caps two trips of both loops and two grayscale partials per image.  Inputs in [-0.3, 1.4]:
    contrast-first takes the grayscale mean of the image as it is, unclamped."""
    s, c = emus(caps), CAPS[caps]
    cases = []
    for Hh, Ww in AUG_HW:
        for b, cc in R64.AUG_BC:
            for lo, hi in ((0.0, 1.0), (-0.3, 1.4)):
                x = lo + (hi - lo) * _rand(8, 3, Hh, Ww, seed=Hh * Ww + 7)
                params = R64.aug_params(b, cc)
                cases.append((x, params, _aug_case(s, c, x, params)))
    _ok(s)
    for x, params, runs in cases:
        part, out = _twice(s, runs)
        _getd(s, part)
        out = _getf(s, out).view_as(x)
        ref, gabs = R64.paired_augment(x, params)
        E.assert_bound(out, ref, R64.aug_bound(x, params, gabs), f"augment {tuple(x.shape)} {params[0, 3:].tolist()}")
        assert float(out.min()) >= 0.0 and float(out.max()) <= 1.0


@BOTH
def test_paired_augment_flips_exact(emus, caps):
    """b = c = 1 on an in-range image: the output is the flipped input bit for bit"""
    s, c = emus(caps), CAPS[caps]
    cases = []
    for Hh, Ww in AUG_HW:
        x = _rand(8, 3, Hh, Ww, seed=Hh + Ww)
        cases.append((x, _aug_case(s, c, x, R64.aug_params(1.0, 1.0))))
    _ok(s)
    for x, runs in cases:
        _, out = _twice(s, runs)
        out = _getf(s, out).view_as(x)
        for n in range(8):
            dims = [d for d, on in ((-1, n & 1), (-2, n & 2)) if on]
            assert _same_bits(out[n], x[n].flip(dims) if dims else x[n]), f"image {n}"


# ------------------------------------------------------------------------------------------------ multi-tensor Adam
class _Adam:
    """p / g / m / v of several tensors, each a block of exactly off + n floats (`off` poison floats in front: off = 1 puts the
    tensor off 16-byte alignment), the chunk list, and the integer part of a driver call"""

    def __init__(self, sizes, repeats, offs, steps, seed, g_special=None):
        self.sizes, self.repeats, self.offs, self.steps = sizes, repeats, offs, steps
        gen = _gen(seed)
        self.t = []
        for i, n in enumerate(sizes):
            d = {"p": torch.randn(n, generator=gen), "g": torch.randn(n, generator=gen) * (1.0 + i % 3),
                 "m": torch.randn(n, generator=gen) * 0.1, "v": (torch.randn(n, generator=gen) * 0.01).abs()}
            if g_special is not None and i == len(sizes) - 1:
                d["g"][n // 2] = g_special
            self.t.append(d)
        ch = [(i, c) for i, n in enumerate(sizes) for c in range(_cdiv(n, CHUNK))]
        self.nchunks, self.chunks = len(ch), torch.tensor(ch, dtype=torch.int32)

    def ints(self):
        out = []
        for n, st, r, o in zip(self.sizes, self.steps, self.repeats, self.offs):
            out += [n, st, r, *o]
        return out

    def bufs(self, s, fresh):
        """the buffer list of one call: g is shared by the calls of a script (read only), p / m / v are `fresh`'s"""
        out = []
        for i, o in enumerate(self.offs):
            for q, off in zip("pgmv", o):
                if q == "g":
                    if "g" not in fresh[i]:
                        fresh[i]["g"] = self._block(s, self.t[i]["g"], off, ro=True)
                    out.append(fresh[i]["g"])
                else:
                    fresh[i][q + "k"] = self._block(s, self.t[i][q], off, ro=False)
                    out.append(fresh[i][q + "k"])
        return out

    @staticmethod
    def _block(s, t, off, ro):
        blk = np.full(off + t.numel(), E.RPOISON if ro else E.WPOISON, np.uint32)
        blk[off:] = t.numpy().view(np.uint32)
        k = s.raw(blk)                      # the driver adds the float offset when it builds the table
        if ro:
            s.ro.append(k)
        elif off:
            s.checks.append((k, np.arange(off), E.WPOISON, "the float in front of a tensor"))
        return k

    @staticmethod
    def read(s, k, off):
        return torch.from_numpy(s.after[k].view(np.float32)[off:].copy())


def _f32(v):
    return float(np.float32(v))


def _check_adam(s, st, fresh, dup_mode, wd, gscale, csu, what, steps_back=0):
    """p, m, v of one call against one float64 step from the initial state"""
    for i, (n, r, o) in enumerate(zip(st.sizes, st.repeats, st.offs)):
        d = st.t[i]
        refs, bounds = R64.adam(d["p"], d["g"], d["m"], d["v"], st.steps[i] + (csu - steps_back) * r, r, dup_mode, wd=wd, gscale=gscale,
                                pow_units=R64.ADAM_POW_UNITS, **R64.ADAM_KW)
        for q, off, ref, e in zip("pmv", (o[0], o[2], o[3]), refs, bounds):
            E.assert_bound(st.read(s, fresh[i][q + "k"], off), ref, e, f"{what}: tensor {i} (n={n}, repeats={r}, offsets={o}) {q}")


ADAM_SETS = [
    # sizes, repeats (4 is the last slot of the bias-correction arrays), float offsets of p g m v, steps at upload
    ([1, 5, CHUNK, CHUNK + 1], [1, 2, 3, 4], [(0, 0, 0, 0), (1, 1, 1, 1), (0, 0, 0, 0), (1, 1, 1, 1)], [0, 3, 0, 100000]),
    ([5, 40000, CHUNK + 1, 1], [4, 1, 2, 3], [(0, 0, 0, 0), (1, 1, 1, 1), (0, 1, 0, 0), (1, 1, 1, 1)], [7, 0, 1, 0]),
    ([CHUNK, 40000, 5], [2, 4, 1], [(1, 1, 1, 1), (0, 0, 0, 0), (0, 0, 0, 1)], [0, 2, 0]),
]


@pytest.mark.parametrize("dup_mode", [0, 1])
@pytest.mark.parametrize("k", range(len(ADAM_SETS)))
def test_adam_multi(emus, k, dup_mode):
    """tensors of 1 .. 40000 floats (one chunk, exactly one, one float more, two and a half) at offsets 0 (16 bytes per lane) and 1
    (single floats; one tensor has only g, or only v, off alignment), with a resident table: calls_since_upload 0 and 3"""
    s = emus("lib")
    sizes, repeats, offs, steps = ADAM_SETS[k]
    st = _Adam(sizes, repeats, offs, steps, seed=10 * k + dup_mode)
    bch = s.vec(st.chunks, np.int32)
    kw = R64.ADAM_KW
    cases, shared = [], [{} for _ in sizes]
    for wd, gscale, csu in ((0.0, 1.0, 0), (_f32(1e-2), 0.125, 3)):
        runs = []
        for _ in range(2):
            fresh = [dict(sh) for sh in shared]                     # g is shared by the calls; p, m and v are this call's own
            bufs = st.bufs(s, fresh)
            for sh, f in zip(shared, fresh):
                sh["g"] = f["g"]
            s.call(ADAM_MULTI, [len(sizes), st.nchunks, dup_mode, 4, csu, *st.ints()], [bch, *bufs],
                   [kw["lr"], kw["beta1"], kw["beta2"], kw["eps"], wd, gscale])
            runs.append(fresh)
        cases.append((wd, gscale, csu, runs))
    _ok(s)
    for wd, gscale, csu, runs in cases:
        for f1, f2 in zip(*runs):
            for q in "pmv":
                assert (s.after[f1[q + "k"]] == s.after[f2[q + "k"]]).all(), "two identical calls differ"
        _check_adam(s, st, runs[0], dup_mode, wd, gscale, csu, f"adam_multi csu={csu}")


def _ctrl(s, skipped, total):
    """an adh_grad_ctrl block of exactly its 32 bytes: the counters set, everything else poison"""
    return s.raw(np.frombuffer(struct.pack("<QIIiiiI", DPOISON, E.WPOISON, E.WPOISON, -77, skipped, total, 0x5A5A5A5A), np.uint8))


def _read_ctrl(s, k):
    sumsq, norm, gs, finite, skipped, total, reserved = struct.unpack("<dffiiiI", s.after[k].tobytes())
    assert reserved == 0x5A5A5A5A, "the reserved word was written"
    return dict(sumsq=sumsq, norm=norm, gscale_eff=gs, finite=finite, skipped=skipped, total=total)


GUARD_CASES = [
    # what, max_norm, skip_nonfinite, the special gradient value
    ("finite, measure only", 0.0, 1, None),
    ("clip engaged", 2.5, 1, None),
    ("non-finite, skipped", 2.5, 1, float("inf")),
    ("non-finite, not skipped", 2.5, 0, float("nan")),
]


@pytest.mark.parametrize("what,max_norm,skip,special", GUARD_CASES, ids=[c[0] for c in GUARD_CASES])
def test_grad_guard_chain(emus, what, max_norm, skip, special):
    """adh_grad_sumsq -> adh_grad_guard_finalize -> adh_adam_multi_guarded on one table.  The control block enters with skipped = 2
    and skipped_total = 5; calls_since_upload = 3, so a step that is taken advances from step + (3 - 2) * repeats."""
    s = emus("lib")
    sizes, repeats, offs, steps = ADAM_SETS[1]
    st = _Adam(sizes, repeats, offs, steps, seed=77, g_special=special)
    bch = s.vec(st.chunks, np.int32)
    kw, gscale, wd, csu = R64.ADAM_KW, 0.5, _f32(1e-2), 3
    shared, runs = [{} for _ in sizes], []
    for _ in range(2):
        fresh = [dict(sh) for sh in shared]
        bufs = st.bufs(s, fresh)
        for sh, f in zip(shared, fresh):
            sh["g"] = f["g"]
        part, ctrl = s.out(st.nchunks, np.float64), _ctrl(s, 2, 5)
        s.call(GRAD_SUMSQ, [len(sizes), st.nchunks, *st.ints()], [bch, part, *bufs], [gscale])
        s.call(GUARD_FINALIZE, [st.nchunks, skip], [part, ctrl], [gscale, max_norm])
        s.call(ADAM_GUARDED, [len(sizes), st.nchunks, 0, 4, csu, *st.ints()], [bch, ctrl, *bufs],
               [kw["lr"], kw["beta1"], kw["beta2"], kw["eps"], wd])
        runs.append((fresh, part, ctrl))
    _ok(s)
    (f1, p1, c1), (f2, p2, c2) = runs
    assert (s.after[p1] == s.after[p2]).all() and (s.after[c1] == s.after[c2]).all()
    for a, b in zip(f1, f2):
        for q in "pmv":
            assert (s.after[a[q + "k"]] == s.after[b[q + "k"]]).all(), "two identical calls differ"
    part, ctrl = s.get(p1, np.float64), _read_ctrl(s, c1)
    want = torch.stack([((st.t[i]["g"][c * CHUNK:(c + 1) * CHUNK].double() * gscale) ** 2).sum() for i, c in st.chunks.tolist()])
    if special is None:
        # a chunk's sum: float64 products of exact factors and at most 16384 / 256 serial additions per lane plus the trees
        assert float(((part - want).abs() / want).max()) <= 128 * U53
        sumsq = float(want.sum())
        assert abs(ctrl["sumsq"] - sumsq) <= (128 + st.nchunks) * U53 * sumsq
        assert abs(ctrl["norm"] - math.sqrt(sumsq)) <= EPS * math.sqrt(sumsq)
        coef = min(1.0, max_norm / (math.sqrt(sumsq) + 1e-6)) if max_norm > 0 else 1.0
        assert (coef < 1.0) == (what == "clip engaged")
        assert abs(ctrl["gscale_eff"] - gscale * coef) <= EPS * gscale * coef + 256 * U53
        assert (ctrl["finite"], ctrl["skipped"], ctrl["total"]) == (1, 2, 5)
        _check_adam(s, st, f1, 0, wd, ctrl["gscale_eff"], csu, what, steps_back=2)
    elif skip:
        assert not math.isfinite(ctrl["sumsq"])
        assert (ctrl["finite"], ctrl["skipped"], ctrl["total"]) == (0, 3, 6), "both skipped counters advance by one"
        for i, o in enumerate(st.offs):
            for q, off in zip("pmv", (o[0], o[2], o[3])):
                assert s.unchanged(f1[i][q + "k"]), f"a skipped step changed {q} of tensor {i}"
    else:
        assert math.isnan(ctrl["sumsq"])
        assert (ctrl["finite"], ctrl["skipped"], ctrl["total"]) == (1, 2, 5) and ctrl["gscale_eff"] == gscale
        # the unguarded behaviour: every tensor but the one that holds the NaN is updated as usual
        st.sizes, st.repeats, st.offs, st.steps = (v[:-1] for v in (st.sizes, st.repeats, st.offs, st.steps))
        _check_adam(s, st, f1, 0, wd, gscale, csu, what, steps_back=2)
        last = len(sizes) - 1
        assert torch.isnan(st.read(s, f1[last]["pk"], offs[last][0])[sizes[last] // 2]), "the NaN gradient reaches its parameter"


def test_grad_guard_finalize_alone(emus):
    """thread t adds its run of ceil(nchunks / 256) consecutive partials: counts on both sides of one and two runs per thread"""
    s = emus("lib")
    cases = []
    for nchunks in (1, 255, 256, 257, 1000):
        part = _rand(nchunks, seed=nchunks).double() * 3 + 0.5
        bp = s.vec(part, np.float64)
        runs = []
        for _ in range(2):
            ctrl = _ctrl(s, 0, 0)
            s.call(GUARD_FINALIZE, [nchunks, 1], [bp, ctrl], [0.25, 3.0])
            runs.append((ctrl,))
        cases.append((part, runs))
    _ok(s)
    for part, runs in cases:
        (ctrl,) = _twice(s, runs)
        ctrl, sumsq = _read_ctrl(s, ctrl), float(part.sum())
        assert abs(ctrl["sumsq"] - sumsq) <= (len(part) + 2) * U53 * sumsq
        assert abs(ctrl["norm"] - math.sqrt(sumsq)) <= EPS * math.sqrt(sumsq)
        coef = min(1.0, 3.0 / (math.sqrt(sumsq) + 1e-6))
        assert abs(ctrl["gscale_eff"] - 0.25 * coef) <= EPS * 0.25 * coef + 256 * U53
        assert (ctrl["finite"], ctrl["skipped"], ctrl["total"]) == (1, 0, 0)


# ------------------------------------------------------------------------------------------------ argument rejections
def test_argument_rejections_write_nothing(emus):
    """every bad call returns ADH_E_ARG (an image smaller than the SSIM window: ADH_E_UNSUPPORTED) before anything is launched:
    every output keeps its poison, and p, m and v keep their values"""
    s = emus("lib")
    x = s.vec(_rand(2 * 3 * 8 * 8))
    one = s.vec(torch.ones(2))
    params = s.vec(R64.aug_params(1.0, 1.0))
    out, part = s.out(2 * 3 * 8 * 8), s.out(8, np.float64)
    bad, unsupported = [], []
    for N, Hh, Ww in ((0, 4, 4), (65536, 4, 4), (1, 0, 4), (1, 4, 0)):
        bad.append(s.call(FOG, [N, Hh, Ww], [x, one, one, out]))
    bad.append(s.call(FOG, [1, 4, 4], [x, None, one, out]))
    for N, nblk in ((2, 2), (2, 0), (0, 1), (65536, 1)):
        bad.append(s.call(PSNR, [N, 96, nblk], [x, x, part, out, out], [1.0]))
    bad.append(s.call(PSNR, [2, 0, 1], [x, x, part, out, out], [1.0]))
    bad.append(s.call(PSNR, [2, 96, 1], [x, x, part, out, None], [1.0]))
    for Hh, Ww in ((6, 16), (16, 6)):
        unsupported.append(s.call(SSIM, [1, Hh, Ww, 1], [x, x, part, out], [1.0]))
    bad.append(s.call(SSIM, [1, 8, 8, 2], [x, x, part, out], [1.0]))                     # nblk is 1
    bad.append(s.call(SSIM, [0, 8, 8, 1], [x, x, part, out], [1.0]))
    bad.append(s.call(AUGMENT, [2, 8, 8, 1], [x, params, part, x]))                      # in place
    bad.append(s.call(AUGMENT, [2, 8, 8, 2], [x, params, part, out]))                    # nblk is 1
    bad.append(s.call(AUGMENT, [0, 8, 8, 1], [x, params, part, out]))
    bad.append(s.call(AUGMENT, [2, 0, 8, 1], [x, params, part, out]))
    st = _Adam([5, 9], [1, 2], [(0, 0, 0, 0), (1, 1, 1, 1)], [0, 0], seed=4)
    bch = s.vec(st.chunks, np.int32)
    fresh = [{}, {}]
    bufs = st.bufs(s, fresh)
    kw = [R64.ADAM_KW[k] for k in ("lr", "beta1", "beta2", "eps")]
    ctrl = _ctrl(s, 0, 0)
    ctrl_off = s.raw(np.full(36, 0x5A, np.uint8), 4)                                      # a control block off 8-byte alignment
    for nt, nchunks, dup_mode, max_rep, csu in ((2, 2, 0, 0, 0), (2, 2, 0, 5, 0), (2, 2, 2, 4, 0), (2, 2, -1, 4, 0), (2, 2, 0, 4, -1),
                                                (2, 0, 0, 4, 0), (-1, 2, 0, 4, 0)):
        bad.append(s.call(ADAM_MULTI, [nt, nchunks, dup_mode, max_rep, csu, *st.ints()], [bch, *bufs], [*kw, 0.0, 1.0]))
        bad.append(s.call(ADAM_GUARDED, [nt, nchunks, dup_mode, max_rep, csu, *st.ints()], [bch, ctrl, *bufs], [*kw, 0.0]))
    bad.append(s.call(ADAM_GUARDED, [2, 2, 0, 4, 0, *st.ints()], [bch, ctrl_off, *bufs], [*kw, 0.0]))
    bad.append(s.call(ADAM_GUARDED, [2, 2, 0, 4, 0, *st.ints()], [bch, None, *bufs], [*kw, 0.0]))
    bad.append(s.call(ADAM_MULTI, [2, 2, 0, 4, 0, *st.ints()], [None, *bufs], [*kw, 0.0, 1.0]))
    bad.append(s.call(GRAD_SUMSQ, [2, 0, *st.ints()], [bch, part, *bufs], [1.0]))
    bad.append(s.call(GRAD_SUMSQ, [-1, 2, *st.ints()], [bch, part, *bufs], [1.0]))
    bad.append(s.call(GRAD_SUMSQ, [2, 2, *st.ints()], [bch, None, *bufs], [1.0]))
    for nchunks, skip, c in ((0, 1, ctrl), (2, 2, ctrl), (2, -1, ctrl), (2, 1, ctrl_off), (2, 1, None)):
        bad.append(s.call(GUARD_FINALIZE, [nchunks, skip], [part, c], [1.0, 1.0]))
    rcs = s.run()
    assert [rcs[k] for k in bad] == [E.ADH_E_ARG] * len(bad), [(k, rcs[k]) for k in bad if rcs[k] != E.ADH_E_ARG]
    assert [rcs[k] for k in unsupported] == [ADH_E_UNSUPPORTED] * 2
    for k in [out, part, ctrl, ctrl_off] + [f[q + "k"] for f in fresh for q in "pmv"]:
        assert s.unchanged(k), "a rejected call wrote to an output"
