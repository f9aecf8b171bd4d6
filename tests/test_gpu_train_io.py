"""The kernels of csrc/train_io.hip through the C ABI, each entry point against a float64 restatement of the same operation
(tests/_ref64.py), at the sizes the wrappers' tests never reach: the grid-stride loops past their block caps (fog and
augmentation beyond 2048 x 256 pixels, the PSNR partials beyond 1024 x 8192 elements), one-pixel rows and columns, SSIM
tiles one pixel wide, PSNR's scalar path on the same data as its vector path, out-of-range augmentation input, and Adam
with a table that stays resident for 50 launches.

Every output and every caller-owned partial buffer is prefilled with NaN and sits inside a NaN guard band that must still
be NaN afterwards.  Every entry point runs twice and must reproduce itself bit for bit.  Tolerances are in units of
EPS = 2^-24 relative to the sum of |terms| added; each comment names the fp32 operations that make up the bound."""
import math

import numpy as np
import pytest
import torch

from adam_dehaze_amd import _hip as H
from tests import _ref64 as R64
from tests._util import DEV, EPS, _assert_bound, _nan, _pad_untouched, _padded, _same_bits, _twice

pytestmark = pytest.mark.gpu
U53 = 2.0 ** -53


def _gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def _rand(*shape, seed=0):
    return torch.rand(shape, device=DEV, dtype=torch.float32, generator=_gen(seed))


def _randn(*shape, seed=0):
    return torch.randn(shape, device=DEV, dtype=torch.float32, generator=_gen(seed))


def _rejected(name, *args):
    with pytest.raises(RuntimeError):
        H.call(name, *args)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ fog
FOG_SHAPES = [(1, 1, 1), (2, 1, 9), (2, 9, 1), (3, 37, 5), (2, 512, 1024), (1, 1024, 2048), (1, 725, 1447)]
FOG_F64_UNITS = R64.FOG_F64_UNITS     # (the bounds shared with tests/test_train_io_hostemu_cpu.py are in tests/_ref64.py)

@pytest.mark.parametrize("N,Hh,Ww", FOG_SHAPES)
def test_apply_fog(N, Hh, Ww):
    """(2, 512, 1024) is exactly the 2048-block cap, (1, 1024, 2048) and (1, 725, 1447) are past it (the latter with a
    ragged last block).  clear spans [-0.5, 1.5], so both clamps saturate; every (beta, airlight) pair of the lists runs."""
    betas, airs = [0.0, 0.15, 0.95, 3.0], [0.0, 0.6, 1.0]
    HW = Hh * Ww
    clear = 2.0 * _rand(N, 3, Hh, Ww, seed=HW) - 0.5
    pairs = [(b, a) for b in betas for a in airs]
    if HW > 100000:
        pairs = [(3.0, 0.0), (0.95, 1.0)] if N > 1 else [(0.95, 0.6)]      # full size: one launch, not the sweep
    saturated = set()
    for k in range(0, len(pairs), N):
        sel = [pairs[(k + i) % len(pairs)] for i in range(N)]
        beta = torch.tensor([s[0] for s in sel], device=DEV, dtype=torch.float32)
        air = torch.tensor([s[1] for s in sel], device=DEV, dtype=torch.float32)

        def run():
            whole, out = _padded(N * 3 * HW)
            H.call("adh_apply_fog", clear.data_ptr(), beta.data_ptr(), air.data_ptr(), N, Hh, Ww, out.data_ptr())
            torch.cuda.synchronize()
            assert _pad_untouched(whole, N * 3 * HW)
            return (out.view(N, 3, Hh, Ww),)
        out, = _twice(run)
        h = R64.fog(clear, beta, air)
        # one rounding of the float64 value to fp32 (half an ulp <= EPS |h|), then the clip (1-Lipschitz)
        bound = EPS * h.abs() + FOG_F64_UNITS * U53 * (clear.double().abs() + 1)
        _assert_bound(out, h.clamp(0, 1), bound, f"fog {sel}")
        assert float(out.min()) >= 0.0 and float(out.max()) <= 1.0
        saturated |= {v for v in (0.0, 1.0) if bool((out == v).any())}
    if HW > 1000:
        assert saturated == {0.0, 1.0}, "the inputs were meant to saturate both clamps"


def test_apply_fog_rejects():
    x = _rand(1, 3, 4, 4)
    b = torch.ones(1, device=DEV)
    out = _nan(1, 3, 4, 4)
    _rejected("adh_apply_fog", x.data_ptr(), b.data_ptr(), b.data_ptr(), 0, 4, 4, out.data_ptr())
    _rejected("adh_apply_fog", x.data_ptr(), b.data_ptr(), b.data_ptr(), 65536, 4, 4, out.data_ptr())
    _rejected("adh_apply_fog", x.data_ptr(), b.data_ptr(), b.data_ptr(), 1, 0, 4, out.data_ptr())
    assert torch.isnan(out).all()


# ------------------------------------------------------------------------------------------------ PSNR
PSNR_PER = [1, 3, 4, 5, 147, 8191, 8192, 8193, 1024 * 8192 - 4, 1024 * 8192 + 4, 3 * 2048 * 2048]
PSNR_F64_UNITS = R64.PSNR_F64_UNITS

def _run_psnr(pred, target, N, per, want_mse=True):
    nblk = H.value("adh_psnr_num_blocks", per)

    def run():
        wpart, part = _padded(N * nblk, dtype=torch.float64)
        wm, mse = _padded(N)
        wp, psnr = _padded(N)
        H.call("adh_psnr", pred.data_ptr(), target.data_ptr(), N, per, 1.0, part.data_ptr(), nblk,
               mse.data_ptr() if want_mse else None, psnr.data_ptr())
        torch.cuda.synchronize()
        assert _pad_untouched(wpart, N * nblk) and _pad_untouched(wm, N) and _pad_untouched(wp, N)
        return mse, psnr, part.view(N, nblk)
    return _twice(run)


@pytest.mark.parametrize("N", [1, 3])
@pytest.mark.parametrize("per", PSNR_PER)
def test_psnr_vector_and_scalar_paths(per, N):
    """The same values at a 16-byte aligned base (vector path when per % 4 == 0) and one float further (scalar path; with
    N > 1 and per % 4 != 0 the images alternate alignment).  8 M elements is the 1024-block cap; 3 x 2048 x 2048 is 1.5
    trips of the grid-stride loop."""
    if per > (1 << 24) and N > 1:
        N = 2
    base_p, base_t = _rand(N * per + 4, seed=per % 9973), _rand(N * per + 4, seed=per % 9973 + 1)
    res = []
    for off in (0, 1):
        p, t = base_p[off:off + N * per], base_t[off:off + N * per]
        if off:
            p.copy_(base_p[:N * per].clone())
            t.copy_(base_t[:N * per].clone())
        res.append(_run_psnr(p, t, N, per))
    p, t = base_p[1:1 + N * per].view(N, per), base_t[1:1 + N * per].view(N, per)
    ref = R64.mse(p, t)
    for mse, psnr, part in res:
        assert not torch.isnan(part).any(), "a partial was not written"
        # mse: the sum is float64 of exact squares of fp32 differences; (a - b) in fp32 is within EPS relative, its square
        # within 2 EPS; one more rounding for the fp32 store
        _assert_bound(mse, ref, (3 * EPS + PSNR_F64_UNITS * U53) * ref, f"mse per={per}")
        ref_db = 10.0 * torch.log10(1.0 / ref)
        # PSNR from the float64 mean (2 EPS relative): 10 / ln 10 * 2 EPS dB, then the fp32 store
        _assert_bound(psnr, ref_db, 10 / math.log(10) * (2 * EPS + PSNR_F64_UNITS * U53) + EPS * ref_db.abs(), f"psnr per={per}")
    s0, s1 = res[0][2].sum(1), res[1][2].sum(1)
    rel = float(((s0 - s1).abs() / s1).max())
    print(f"[measure] psnr vector vs scalar float64 sums: rel diff {rel / U53:.2f} units of 2^-53")
    assert rel <= 2.0 ** -50, "vector and scalar paths disagree on the same data"


def test_psnr_identical_inputs_and_null_mse():
    x = _rand(3 * 8193, seed=5)
    mse, psnr, _ = _run_psnr(x, x.clone(), 3, 8193)
    assert (mse == 0).all() and torch.isinf(psnr).all() and (psnr > 0).all()
    y = _rand(3 * 8193, seed=6)
    mse2, psnr2, _ = _run_psnr(x, y, 3, 8193, want_mse=False)
    assert torch.isnan(mse2).all(), "mse == NULL must not be written"
    _, psnr3, _ = _run_psnr(x, y, 3, 8193)
    assert _same_bits(psnr2, psnr3)


def test_psnr_rejects():
    x, y = _rand(4096, seed=1), _rand(4096, seed=2)
    part, mse, psnr = _nan(8, dtype=torch.float64), _nan(4), _nan(4)
    ok = H.value("adh_psnr_num_blocks", 1024)
    for N, nblk in ((4, ok + 1), (4, 0), (0, ok), (65536, ok)):
        _rejected("adh_psnr", x.data_ptr(), y.data_ptr(), N, 1024, 1.0, part.data_ptr(), nblk, mse.data_ptr(), psnr.data_ptr())
    assert torch.isnan(part).all() and torch.isnan(mse).all() and torch.isnan(psnr).all()
    assert H.value("adh_psnr_num_blocks", 1) == 1 and H.value("adh_psnr_num_blocks", 8193) == 2
    assert H.value("adh_psnr_num_blocks", 3 * 2048 * 2048) == 1024


# ------------------------------------------------------------------------------------------------ SSIM
SSIM_HW = [(7, 7), (7, 39), (39, 7), (38, 38), (39, 39), (71, 40), (45, 131), (512, 1024)]


@pytest.mark.parametrize("kind", ["random", "constant", "two_constants", "negative"])
@pytest.mark.parametrize("Hh,Ww", SSIM_HW)
def test_ssim_gray(Hh, Ww, kind):
    """39 = 32 + 7: the last tile is one output wide (39, 7), one high (7, 39), both (39, 39); (71, 40) has three tile
    rows with a one-column and a one-row last tile together."""
    N = 2
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
    nblk = H.value("adh_ssim_num_blocks", Hh, Ww)
    assert nblk == -(-(Hh - 6) // 32) * -(-(Ww - 6) // 32)

    def run():
        wpart, part = _padded(N * nblk, dtype=torch.float64)
        ws, ssim = _padded(N)
        H.call("adh_ssim_gray", p.data_ptr(), t.data_ptr(), N, Hh, Ww, 1.0, part.data_ptr(), nblk, ssim.data_ptr())
        torch.cuda.synchronize()
        assert _pad_untouched(wpart, N * nblk) and _pad_untouched(ws, N)
        return ssim, part
    ssim, part = _twice(run)
    assert not torch.isnan(part).any()
    ref = R64.ssim_gray(p, t)
    # the grayscale is the same three fp32 operations on both sides; the window statistics are float64: each of the five
    # 49-term sums is within 49 * 2^-53 of its |terms| <= 49, the variances cancel, so they carry ~1e-14 absolute and S
    # (denominators >= C2 = 9e-4) ~1.2e-11; 1e-10 with margin for the order of the sums.  Then one fp32 store.
    _assert_bound(ssim, ref, EPS * ref.abs() + 1e-10, f"ssim {kind}")
    if kind == "constant":
        assert float((ssim - 1).abs().max()) <= EPS


def test_ssim_small_images_unsupported():
    x = _rand(1, 3, 6, 40)
    part, ssim = _nan(4, dtype=torch.float64), _nan(1)
    assert H.value("adh_ssim_num_blocks", 6, 40) == 0 and H.value("adh_ssim_num_blocks", 40, 6) == 0
    for Hh, Ww in ((6, 40), (40, 6)):
        with pytest.raises(RuntimeError, match="UNSUPPORTED"):
            H.call("adh_ssim_gray", x.data_ptr(), x.data_ptr(), 1, Hh, Ww, 1.0, part.data_ptr(), 1, ssim.data_ptr())
    _rejected("adh_ssim_gray", x.data_ptr(), x.data_ptr(), 1, 40, 40, 1.0, part.data_ptr(), 1, ssim.data_ptr())   # nblk is 4
    torch.cuda.synchronize()
    assert torch.isnan(part).all() and torch.isnan(ssim).all()


# ------------------------------------------------------------------------------------------------ paired augmentation
AUG_HW = [(17, 33), (1, 1), (1, 300), (300, 1), (512, 1024), (1024, 2048)]
AUG_BC = R64.AUG_BC


def _aug_params(b, c):
    return R64.aug_params(b, c).to(DEV)


def _run_aug(x, params, Hh, Ww):
    N = x.shape[0]
    nblk = H.value("adh_augment_num_blocks", Hh * Ww)

    def run():
        wpart, part = _padded(N * nblk, dtype=torch.float64)
        whole, out = _padded(N * 3 * Hh * Ww)
        H.call("adh_paired_augment", x.data_ptr(), params.data_ptr(), N, Hh, Ww, part.data_ptr(), nblk, out.data_ptr())
        torch.cuda.synchronize()
        assert _pad_untouched(wpart, N * nblk) and _pad_untouched(whole, N * 3 * Hh * Ww)
        assert not torch.isnan(part).any()
        return (out.view(N, 3, Hh, Ww),)
    return _twice(run)[0]


# every (b, c) pair and both input ranges at the small shapes; the two full-size shapes get one case per range, not the sweep
AUG_CASES = [(h, w, b, c, lo, hi) for (h, w) in AUG_HW[:4] for (b, c) in AUG_BC for (lo, hi) in ((0.0, 1.0), (-0.3, 1.4))] + \
    [(h, w, b, c, lo, hi) for (h, w) in AUG_HW[4:] for (b, c, lo, hi) in ((0.9, 1.1, 0.0, 1.0), (1.05, 0.9, -0.3, 1.4))]


@pytest.mark.parametrize("Hh,Ww,b,c,lo,hi", AUG_CASES)
def test_paired_augment(Hh, Ww, b, c, lo, hi):
    """All eight (flip_h, flip_v, brightness_first) combinations in one batch.  (1024, 2048) is past both caps (2048 blocks
    of the gather pass, 256 x 4096 pixels of the grayscale partials).  Inputs in [-0.3, 1.4]: a network output is not
    confined to [0, 1], and contrast-first takes the grayscale mean of the image as it is, unclamped (torchvision)."""
    x = lo + (hi - lo) * _rand(8, 3, Hh, Ww, seed=Hh * Ww + 7)
    params = _aug_params(b, c)
    out = _run_aug(x, params, Hh, Ww)
    ref, gabs = R64.paired_augment(x, params)
    _assert_bound(out, ref, R64.aug_bound(x, params, gabs), f"augment b={b} c={c} range=[{lo}, {hi}]")
    assert float(out.min()) >= 0.0 and float(out.max()) <= 1.0


@pytest.mark.parametrize("Hh,Ww", AUG_HW)
def test_paired_augment_flips_exact(Hh, Ww):
    """b = c = 1 on an in-range image: 1 * x, 1 * x + 0 * mean and the clamps change nothing, so the output is the
    flipped input bit for bit."""
    x = _rand(8, 3, Hh, Ww, seed=Hh + Ww)
    params = _aug_params(1.0, 1.0)
    out = _run_aug(x, params, Hh, Ww)
    for n in range(8):
        dims = [d for d, on in ((-1, n & 1), (-2, n & 2)) if on]
        assert _same_bits(out[n], x[n].flip(dims) if dims else x[n]), f"image {n}"


def test_paired_augment_rejects():
    x = _rand(2, 3, 8, 8)
    params = _aug_params(1.0, 1.0)
    part, out = _nan(2, dtype=torch.float64), _nan(2, 3, 8, 8)
    _rejected("adh_paired_augment", x.data_ptr(), params.data_ptr(), 2, 8, 8, part.data_ptr(), 1, x.data_ptr())       # in place
    _rejected("adh_paired_augment", x.data_ptr(), params.data_ptr(), 2, 8, 8, part.data_ptr(), 2, out.data_ptr())     # nblk
    _rejected("adh_paired_augment", x.data_ptr(), params.data_ptr(), 0, 8, 8, part.data_ptr(), 1, out.data_ptr())
    assert torch.isnan(part).all() and torch.isnan(out).all()
    assert H.value("adh_augment_num_blocks", 1) == 1 and H.value("adh_augment_num_blocks", 1024 * 2048) == 256


# ------------------------------------------------------------------------------------------------ multi-tensor Adam
ADAM_POW_UNITS, ADAM_KW = R64.ADAM_POW_UNITS, R64.ADAM_KW

class _AdamState:
    """p / g / m / v of several tensors carved out of four NaN arenas with 16-float gaps (the last tensor starts one float
    off 16-byte alignment), the device table and chunk list of adh_adam_multi."""

    def __init__(self, sizes, repeats, seed, zero_mv=False):
        self.sizes, self.repeats = sizes, repeats
        self.chunk = H.value("adh_adam_chunk_elems")
        offs, o = [], 16
        for i, n in enumerate(sizes):
            o = (o + 3) // 4 * 4 + (1 if i == len(sizes) - 1 else 0)
            offs.append(o)
            o += n + 16
        self.offs, self.total = offs, o
        self.arena = {k: _nan(o) for k in "pgmv"}
        self.owned = torch.zeros(o, dtype=torch.bool, device=DEV)
        for off, n in zip(offs, sizes):
            self.owned[off:off + n] = True
        g = _gen(seed)
        for k, scale in (("p", 1.0), ("m", 0.1), ("v", 0.01)):
            for off, n in zip(offs, sizes):
                r = torch.randn(n, device=DEV, generator=g) * scale
                self.arena[k][off:off + n] = 0.0 if (zero_mv and k != "p") else (r.abs() if k == "v" else r)
        self.init = {k: self.arena[k].clone() for k in "pmv"}
        ch = [(i, c) for i, n in enumerate(sizes) for c in range(-(-n // self.chunk))]
        self.nchunks = len(ch)
        self.chunks = torch.tensor(ch, dtype=torch.int32, device=DEV).contiguous()
        self.table = None

    def view(self, k, i):
        return self.arena[k][self.offs[i]:self.offs[i] + self.sizes[i]]

    def reset(self):
        for k in "pmv":
            self.arena[k].copy_(self.init[k])

    def upload(self, steps):
        tab = (H.AdamTensor * len(self.sizes))()
        for i, n in enumerate(self.sizes):
            tab[i].p, tab[i].g, tab[i].m, tab[i].v = (self.view(k, i).data_ptr() for k in "pgmv")
            tab[i].n, tab[i].step, tab[i].repeats = n, steps[i], self.repeats[i]
        self.table = torch.frombuffer(bytearray(bytes(tab)), dtype=torch.uint8).to(DEV)
        torch.cuda.synchronize()

    def launch(self, dup_mode, wd, gscale, csu, max_repeats=4, **kw):
        kw = {**ADAM_KW, **kw}
        H.call("adh_adam_multi", self.table.data_ptr(), self.chunks.data_ptr(), self.nchunks, kw["lr"], kw["beta1"], kw["beta2"],
               kw["eps"], wd, gscale, dup_mode, max_repeats, csu)

    def set_grads(self, k, zero):
        g = _gen(7000 + k)
        for off, n in zip(self.offs, self.sizes):
            self.arena["g"][off:off + n] = 0.0 if zero else torch.randn(n, device=DEV, generator=g) * (1.0 + (k % 3))

    def guards_ok(self):
        return all(bool(torch.isnan(self.arena[k][~self.owned]).all()) for k in "pmv")


def _adam_sizes():
    ch = H.value("adh_adam_chunk_elems")
    return [1, 3, 4, 5, ch - 1, ch, ch + 1, 2 * ch + 7, 1000]


ADAM_CASES = [(0.0, 1.0, False, 0, r) for r in range(4)] + [(1e-2, 0.125, False, 0, r) for r in range(4)] + \
    [(1e-2, 1.0, True, 0, 0), (0.0, 1.0, True, 0, 1), (1e-2, 1.0, False, 100000, 2), (0.0, 0.125, False, 1, 3)]


@pytest.mark.parametrize("dup_mode", [0, 1])
@pytest.mark.parametrize("wd,gscale,gzero,start,rot", ADAM_CASES)
def test_adam_multi_resident_table(wd, gscale, gzero, start, rot, dup_mode):
    """50 launches with the table uploaded ONCE (calls_since_upload 0..49) against 50 launches that re-upload the table
    with the advanced step counts: bit-equal after every launch.  Each launch is compared with one float64 step taken
    from the state the kernel started that launch with (so the bounds are those of one step: _ref64.adam derives them
    operation by operation), and p_final - p0 with the sum of those float64 updates under the sum of the bounds.
    Tensor i takes repeats 1 + (i + rot) % 4; sizes straddle the 16384-float chunk, the last tensor is unaligned (scalar
    path)."""
    sizes = _adam_sizes()
    repeats = [1 + (i + rot) % 4 for i in range(len(sizes))]
    wd32 = float(np.float32(wd))
    st = _AdamState(sizes, repeats, seed=rot + 10 * dup_mode, zero_mv=gzero and wd == 0.0)
    steps0 = [start] * len(sizes)
    K = 50
    # run A: resident table
    st.upload(steps0)
    hist = []
    for k in range(K):
        st.set_grads(k, gzero)
        st.launch(dup_mode, wd32, gscale, k)
        hist.append({q: st.arena[q].clone() for q in "pmv"})
    torch.cuda.synchronize()
    assert st.guards_ok(), "adam wrote outside its tensors"
    # run B: table uploaded again before every launch
    st.reset()
    for k in range(K):
        st.set_grads(k, gzero)
        st.upload([s + k * r for s, r in zip(steps0, repeats)])
        st.launch(dup_mode, wd32, gscale, 0)
        for q in "pmv":
            assert _same_bits(st.arena[q][st.owned], hist[k][q][st.owned]), f"launch {k}: resident and re-uploaded tables differ in {q}"
    # float64, one launch at a time
    worst = {"p": 0.0, "m": 0.0, "v": 0.0}
    sls = [slice(o, o + n) for o, n in zip(st.offs, sizes)]
    acc_ref = [torch.zeros(n, dtype=torch.float64, device=DEV) for n in sizes]
    acc_bound = [torch.zeros(n, dtype=torch.float64, device=DEV) for n in sizes]
    for k in range(K):
        st.set_grads(k, gzero)
        before = st.init if k == 0 else hist[k - 1]
        for i, (n, r, sl) in enumerate(zip(sizes, repeats, sls)):
            (p, m, v), (ep, em, ev) = R64.adam(before["p"][sl], st.arena["g"][sl], before["m"][sl], before["v"][sl], steps0[i] + k * r,
                                               r, dup_mode, wd=wd32, gscale=gscale, pow_units=ADAM_POW_UNITS, **ADAM_KW)
            for q, ref, e in (("p", p, ep), ("m", m, em), ("v", v, ev)):
                got = hist[k][q][sl]
                assert not torch.isnan(got).any()
                err = (got.double() - ref).abs()
                if float(err.max()) > 0:
                    worst[q] = max(worst[q], float((err / e.clamp_min(1e-300)).max()))
                over = float((err - e).max())
                assert over <= 0, f"tensor {i} (n={n}, repeats={r}) launch {k}: {q} is {over:.3e} over its bound"
            acc_ref[i] += p - before["p"][sl].double()
            acc_bound[i] += ep
    for i, sl in enumerate(sls):
        moved = hist[-1]["p"][sl].double() - st.init["p"][sl].double()
        assert float(((moved - acc_ref[i]).abs() - acc_bound[i]).max()) <= 0, f"tensor {i}: accumulated update"
        if gzero and wd == 0.0:
            assert _same_bits(hist[-1]["p"][sl], st.init["p"][sl]), "g = 0, m = v = 0, wd = 0: 0 / eps moves nothing"
    print(f"[bound] adam worst |err| / bound: {worst}")


def test_adam_bias_correction_powf():
    """One-element tensors with m = v = 0, g = 1, eps = 0, lr = 1 at start steps 0..127 and a few large ones: the update is
    (1 - beta1) / bc1 * bc2 / sqrt(1 - beta2), six fp32 roundings besides the two powf.  What exceeds those six EPS is
    powf's error amplified by beta^t / (1 - beta^t): printed in EPS units of beta^t, bounded by ADAM_POW_UNITS."""
    steps = list(range(128)) + [1000, 10000, 100000]
    n = len(steps)
    st = _AdamState([1] * n, [1] * n, seed=3)
    for k in "pmv":
        st.arena[k][st.owned] = 0.0
    st.arena["g"][st.owned] = 1.0
    st.upload(steps)
    st.launch(0, 0.0, 1.0, 0, lr=1.0, eps=0.0)
    torch.cuda.synchronize()
    got = -st.arena["p"][st.owned].double().cpu()
    b1, b2 = ADAM_KW["beta1"], ADAM_KW["beta2"]
    t = torch.tensor(steps, dtype=torch.float64) + 1
    ref = (1 - b1) / (1 - b1 ** t) * torch.sqrt(1 - b2 ** t) / math.sqrt(1 - b2)
    rel = (got - ref).abs() / ref
    amp = b1 ** t / (1 - b1 ** t) + 0.5 * b2 ** t / (1 - b2 ** t)
    need = ((rel - 8 * EPS) / (amp * EPS)).clamp_min(0)
    print(f"[measure] adam powf: worst rel err {float(rel.max()) / EPS:.1f} EPS at t={int(t[rel.argmax()])}; powf units needed "
          f"beyond 8 EPS of plain roundings: {float(need.max()):.2f}; rel / (amp EPS) max {float((rel / (amp * EPS))[:128].max()):.2f}")
    assert float((rel - (8 + ADAM_POW_UNITS * amp) * EPS).max()) <= 0
    assert st.guards_ok()


def test_adam_multi_rejects():
    st = _AdamState([5, 9], [1, 2], seed=4)
    st.set_grads(0, False)
    st.upload([0, 0])
    before = {k: st.arena[k].clone() for k in "pmv"}
    for dup_mode, max_rep, csu in ((0, 0, 0), (0, 5, 0), (2, 4, 0), (-1, 4, 0), (0, 4, -1)):
        with pytest.raises(RuntimeError):
            st.launch(dup_mode, 0.0, 1.0, csu, max_repeats=max_rep)
    with pytest.raises(RuntimeError):
        H.call("adh_adam_multi", st.table.data_ptr(), st.chunks.data_ptr(), 0, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1.0, 0, 4, 0)
    torch.cuda.synchronize()
    for k in "pmv":
        assert _same_bits(st.arena[k][st.owned], before[k][st.owned])
