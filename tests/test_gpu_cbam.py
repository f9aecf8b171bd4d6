"""The AttentionBlock kernels of csrc/cbam.hip through the C ABI, each entry point against a float64 torch restatement of
the same operation (base_model.py:43-78), at the edges the 16 / 32 / 96-channel fixtures never reach: the product widths
192 and 384, images smaller than the 7 x 7 window, exact ties in both arg-maxes (the first index must win, like
torch.max / adaptive_max_pool2d on the CPU), 256-pixel blocks that straddle images, and the grid-stride loops past their
caps.

Every output buffer is prefilled with NaN (index buffers with -7): a kernel must write every element it owns, and
everything outside the channel slice it owns must still be NaN afterwards.  Every entry point runs twice and must
reproduce itself bit for bit.  Tolerances are in units of EPS = 2^-24, the fp32 unit roundoff, relative to the sum of
|terms| the kernel adds; the float64 restatements and their bounds are tests/_cbam_ref64.py's, which the host-emulation run of
the same source (tests/test_cbam_hostemu_cpu.py) shares."""
import pytest
import torch

from adam_dehaze_amd import _hip as H
from adam_dehaze_amd.engine import Act, Engine
from tests import _cbam_ref64 as R
from tests._cbam_ref64 import APPLY_HW, EPS, POOL_PPB
from tests.test_gpu_fullsize import _cbam_ref64

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")


def _nan(*shape):
    return torch.full(shape, NAN, device=DEV, dtype=torch.float32)


def _idx(*shape):
    return torch.full(shape, -7, device=DEV, dtype=torch.int32)


def _gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def _randn(*shape, seed=0):
    return torch.randn(shape, device=DEV, dtype=torch.float32, generator=_gen(seed))


def _rand(*shape, seed=0):
    return torch.rand(shape, device=DEV, dtype=torch.float32, generator=_gen(seed))


def _ints(shape, lo, hi, seed):
    return torch.randint(lo, hi + 1, shape, device=DEV, generator=_gen(seed)).float()


def _same_bits(u, v):
    if u.is_floating_point():
        u, v = u.view(torch.int32), v.view(torch.int32)
    return torch.equal(u, v)


def _twice(fn):
    a = fn()
    b = fn()
    torch.cuda.synchronize()
    for i, (u, v) in enumerate(zip(a, b)):
        assert _same_bits(u, v), f"output {i} differs between two identical runs"
    return a


_assert_bound = R.assert_bound


# ------------------------------------------------------------------------------------------------ channel pooling
POOL_C = [4, 16, 96, 192, 384, 1024]
POOL_HW = [1, 7, 511, 512, 513, 128 * 256, 256 * 512]


def _run_pool(xb, x_cs, N, HW, C):
    nblk = H.value("adh_cbam_pool_num_blocks", HW)

    def run():
        part, pidx = _nan(N, nblk, 2, C), _idx(N, nblk, C)
        pooled, amax = _nan(N, 2, C), _idx(N, C)
        H.call("adh_cbam_pool", xb.data_ptr(), x_cs, N, HW, C, part.data_ptr(), pidx.data_ptr(), nblk, pooled.data_ptr(),
               amax.data_ptr())
        return pooled, amax
    return _twice(run)


@pytest.mark.parametrize("HW", POOL_HW)
@pytest.mark.parametrize("C", POOL_C)
def test_cbam_pool_ties_first_index(C, HW):
    """Values from {0, 1, 2}: ties everywhere, within a thread's pixels, across the rows of a block and across blocks.
    Channel 1 is constant, channel 2 all negative; channel 3 holds 0 / 1 with its maximum 2 first in block 1 and again in
    blocks 8 and 9 (8 is in block 0's stream of the final reduction, so only the index tie-break picks block 1).  The sums
    are of small integers and halves: exact in fp32, so the mean is the float64 mean rounded once."""
    N = 3 if C * HW <= (1 << 22) else 1
    x_cs = C + 4
    xb = _ints((N, HW, x_cs), 0, 2, seed=C + HW)
    xb[..., 1] = 1.5
    xb[..., 2] = -_ints((N, HW), 1, 3, seed=C + HW + 1)
    if HW > 10 * POOL_PPB:
        xb[..., 3] = xb[..., 3].clamp_max(1.0)
        for p in (POOL_PPB + 100, 8 * POOL_PPB + 5, 9 * POOL_PPB + 3):
            xb[:, p, 3] = 2.0
    x = xb[..., :C].double()
    pooled, amax = _run_pool(xb, x_cs, N, HW, C)
    mean, mx, first = R.pool64(x)
    assert torch.equal(pooled[:, 0].double(), mean), "mean"
    assert torch.equal(pooled[:, 1].double(), mx), "max"
    assert torch.equal(amax.long(), first), "arg-max must be the first index in scan order"
    if HW > 10 * POOL_PPB:
        assert (amax[:, 3] == POOL_PPB + 100).all()


# ------------------------------------------------------------------------------------------------ MLP
@pytest.mark.parametrize("C", [16, 96, 192, 384, 1024])
def test_cbam_mlp(C):
    Ch, N = C // 16, 3
    pooled = _randn(N, 2, C, seed=C)
    w1 = _randn(Ch, C, seed=C + 1) / C ** 0.5
    w1[0] = 0.0                                 # hidden unit 0: pre-activation exactly 0 for every image
    w2 = _randn(C, Ch, seed=C + 2) / Ch ** 0.5

    def run():
        ca, hidden = _nan(N, C), _nan(N, 2, Ch)
        H.call("adh_cbam_mlp", pooled.data_ptr(), w1.data_ptr(), w2.data_ptr(), N, C, Ch, ca.data_ptr(), hidden.data_ptr())
        return ca, hidden

    ca, hidden = _twice(run)
    h, e_h, ca_ref, e_ca = R.mlp64(pooled, w1, w2)
    _assert_bound(hidden, h, e_h, "hidden")
    assert (hidden[:, :, 0] == 0).all()
    _assert_bound(ca, ca_ref, e_ca, "ca")


# ------------------------------------------------------------------------------------------------ spatial statistics
SS_CASES = [(4, 7), (4, 513), (4, 256 * 300), (16, 513), (96, 7), (96, 256 * 300), (192, 513), (384, 513), (1024, 2000)]


@pytest.mark.parametrize("C,HW", SS_CASES)
def test_cbam_spatial_stats_ties_first_index(C, HW):
    """x from {0, 1, 2} and ca from powers of two: x * ca is exact, ties in the channel max are everywhere, every 5th pixel
    is all zero.  C = 4 leaves 7 of the 8 lanes of a pixel idle; HW = 76 800 > 2048 blocks x 32 pixels runs the loop."""
    N = 2
    x_cs = C + 8
    xb = _ints((N, HW, x_cs), 0, 2, seed=C + HW)
    xb[:, ::5, :] = 0.0
    ca = torch.pow(2.0, _ints((N, C), -3, 1, seed=C + HW + 1))

    def run():
        smap, cidx = _nan(N, HW, 2), _idx(N, HW)
        H.call("adh_cbam_spatial_stats", xb.data_ptr(), x_cs, ca.data_ptr(), N, HW, C, smap.data_ptr(), cidx.data_ptr())
        return smap, cidx

    smap, cidx = _twice(run)
    mean, e_mean, mx, first = R.spatial_stats64(xb[..., :C], ca)
    _assert_bound(smap[..., 0], mean, e_mean, "channel mean")
    assert torch.equal(smap[..., 1].double(), mx), "channel max"
    assert torch.equal(cidx.long(), first), "channel arg-max must be the first index"


# ------------------------------------------------------------------------------------------------ spatial attention + apply
def _check_apply(N, Hh, Ww, C, x_cs, out_cs, seed):
    HW = Hh * Ww
    xb = _randn(N, Hh, Ww, x_cs, seed=seed)
    ca = _rand(N, C, seed=seed + 1)
    smap = _randn(N, HW, 2, seed=seed + 2)
    wsp = _randn(98, seed=seed + 3) / 98 ** 0.5

    def run():
        sa, ob = _nan(N, HW), _nan(N, Hh, Ww, out_cs)
        H.call("adh_cbam_apply", xb.data_ptr(), x_cs, ca.data_ptr(), smap.data_ptr(), wsp.data_ptr(), N, Hh, Ww, C,
               sa.data_ptr(), ob.data_ptr(), out_cs)
        return sa, ob

    sa, ob = _twice(run)
    sa_ref, e_sa = R.sa64(smap, wsp, N, Hh, Ww)
    _assert_bound(sa.view(N, Hh, Ww), sa_ref, e_sa, "sa")
    # out = (x * ca) * sa, two roundings in that order: equal to the same two fp32 products
    assert torch.equal(ob[..., :C], R.scale_f32(xb[..., :C], ca, sa, N, Hh, Ww)), "out = x * ca * sa"
    assert torch.isnan(ob[..., C:]).all(), "written outside its channel slice"


@pytest.mark.parametrize("hw", APPLY_HW, ids=lambda s: "%dx%d" % s)
def test_cbam_apply_small_images_and_tile_edges(hw):
    # the 7 x 7 window larger than the image, and both edges of the 32 x 8 tiles
    Hh, Ww = hw
    _check_apply(2, Hh, Ww, 16, x_cs=20, out_cs=24, seed=Hh * 41 + Ww)


def test_cbam_apply_product_widths():
    _check_apply(2, 37, 53, 192, x_cs=196, out_cs=200, seed=5)
    _check_apply(1, 33, 40, 384, x_cs=384, out_cs=392, seed=6)


def test_cbam_apply_past_the_grid_cap():
    """C = 1024, HW = 512 x 1040: 136M quads per image, past CBAM_SCALE_MAXBLK x 256 threads x 8 = 2^27, so the scale pass
    takes a second trip (2.2 GB per tensor).  The output is compared in chunks with the same two fp32 products."""
    N, Hh, Ww, C = 1, 512, 1040, 1024
    HW = Hh * Ww
    x = _randn(N, Hh, Ww, C, seed=7)
    ca = _rand(N, C, seed=8)
    smap = _randn(N, HW, 2, seed=9)
    wsp = _randn(98, seed=10) / 98 ** 0.5
    sa, out = _nan(N, HW), _nan(N, Hh, Ww, C)
    for run in range(2):
        out.fill_(NAN)
        H.call("adh_cbam_apply", x.data_ptr(), C, ca.data_ptr(), smap.data_ptr(), wsp.data_ptr(), N, Hh, Ww, C, sa.data_ptr(),
               out.data_ptr(), C)
        torch.cuda.synchronize()
        for y0 in range(0, Hh, 64):
            want = x[:, y0:y0 + 64] * ca.view(N, 1, 1, C) * sa.view(N, Hh, Ww, 1)[:, y0:y0 + 64]
            assert torch.equal(out[:, y0:y0 + 64], want), f"run {run}, rows {y0}.."
            del want
    sa_ref, e_sa = R.sa64(smap, wsp, N, Hh, Ww)
    _assert_bound(sa.view(N, Hh, Ww), sa_ref, e_sa, "sa")
    del x, out, sa, smap
    torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------ backward, pass by pass
class _Fwd:
    """The forward kernels on quantized input (ties in both arg-maxes) and everything the backward passes read."""

    def __init__(self, N, Hh, Ww, C, seed, x_cs=None):
        self.N, self.Hh, self.Ww, self.C, self.HW = N, Hh, Ww, C, Hh * Ww
        self.Ch = max(1, C // 16)
        self.x_cs = x_cs or C
        HW = self.HW
        self.xb = _ints((N, HW, self.x_cs), 0, 2, seed=seed)
        self.g = _randn(N, HW, C + 4, seed=seed + 1)
        self.w1 = _randn(self.Ch, C, seed=seed + 2) / C ** 0.5
        self.w1[0] = 0.0                           # a hidden unit with pre-activation exactly 0
        self.w2 = _randn(C, self.Ch, seed=seed + 3) / self.Ch ** 0.5
        self.wsp = _randn(98, seed=seed + 4) / 98 ** 0.5
        self.nblk = H.value("adh_cbam_pool_num_blocks", HW)
        part, pidx = _nan(N, self.nblk, 2, C), _idx(N, self.nblk, C)
        self.pooled, self.amax = _nan(N, 2, C), _idx(N, C)
        H.call("adh_cbam_pool", self.xb.data_ptr(), self.x_cs, N, HW, C, part.data_ptr(), pidx.data_ptr(), self.nblk,
               self.pooled.data_ptr(), self.amax.data_ptr())
        self.ca, self.hidden = _nan(N, C), _nan(N, 2, self.Ch)
        H.call("adh_cbam_mlp", self.pooled.data_ptr(), self.w1.data_ptr(), self.w2.data_ptr(), N, C, self.Ch,
               self.ca.data_ptr(), self.hidden.data_ptr())
        self.smap, self.cidx = _nan(N, HW, 2), _idx(N, HW)
        H.call("adh_cbam_spatial_stats", self.xb.data_ptr(), self.x_cs, self.ca.data_ptr(), N, HW, C, self.smap.data_ptr(),
               self.cidx.data_ptr())
        self.sa, out = _nan(N, HW), _nan(N, HW, C)
        H.call("adh_cbam_apply", self.xb.data_ptr(), self.x_cs, self.ca.data_ptr(), self.smap.data_ptr(), self.wsp.data_ptr(),
               N, Hh, Ww, C, self.sa.data_ptr(), out.data_ptr(), C)
        torch.cuda.synchronize()

    @property
    def x(self):
        return self.xb[..., :self.C]

    @property
    def gv(self):
        return self.g[..., :self.C]


BWD_SHAPES = [(3, 37, 53, 96), (2, 1, 5, 16), (3, 4, 2, 32), (1, 7, 7, 192), (2, 16, 40, 384), (1, 64, 80, 1024)]
_ids = lambda s: "%dx%dx%dx%d" % s


@pytest.mark.parametrize("shape", BWD_SHAPES + [(2, 256, 300, 16)], ids=_ids)
def test_cbam_bwd_a(shape):
    # 256 x 300 = 76 800 pixels per image: past CBAM_ROW_MAXBLK x 32, so the per-pixel loop takes a second trip
    f = _Fwd(*shape, seed=sum(shape), x_cs=shape[3] + 8)
    N, HW, C = f.N, f.HW, f.C

    def run():
        out = _nan(N, HW)
        H.call("adh_cbam_bwd_a", f.g.data_ptr(), C + 4, f.xb.data_ptr(), f.x_cs, f.ca.data_ptr(), f.sa.data_ptr(), N, HW, C,
               out.data_ptr())
        return (out,)

    (gsa,) = _twice(run)
    ref, e = R.bwd_a64(f.gv, f.x, f.ca, f.sa)
    _assert_bound(gsa, ref, e, "gsa_pre")


BWD_B_SHAPES = [(3, 37, 53), (2, 1, 5), (3, 4, 2), (1, 7, 7), (2, 40, 33), (1, 1, 1)]


@pytest.mark.parametrize("shape", BWD_B_SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_cbam_bwd_b_transposed_conv_and_weight_gradient(shape):
    """gsmap = conv7x7^T(gsa_pre) and d-wsp, against float64 autograd of F.conv2d(smap, wsp, padding=3); N x HW is not a
    multiple of the 256-pixel blocks, which straddle images."""
    N, Hh, Ww = shape
    HW = Hh * Ww
    gsa = _randn(N, HW, seed=HW)
    smap = _randn(N, HW, 2, seed=HW + 1)
    wsp = _randn(98, seed=HW + 2) / 98 ** 0.5
    nb = H.value("adh_cbam_bwd_b_num_blocks", N, Hh, Ww)
    dw0 = _randn(98, seed=HW + 3)

    def run():
        gsmap, part, dw, dwa = _nan(N, HW, 2), _nan(nb, 98), _nan(98), dw0.clone()
        H.call("adh_cbam_bwd_b", gsa.data_ptr(), smap.data_ptr(), wsp.data_ptr(), N, Hh, Ww, gsmap.data_ptr(), part.data_ptr(),
               nb, dw.data_ptr(), 0)
        H.call("adh_cbam_bwd_b", gsa.data_ptr(), smap.data_ptr(), wsp.data_ptr(), N, Hh, Ww, gsmap.data_ptr(), part.data_ptr(),
               nb, dwa.data_ptr(), 1)
        return gsmap, dw, dwa

    gsmap, dw, dwa = _twice(run)
    gs_ref, e_gs, dw_ref, e_dw = R.bwd_b64(gsa, smap, wsp, N, Hh, Ww)
    _assert_bound(gsmap.view(N, Hh, Ww, 2), gs_ref, e_gs, "gsmap")
    _assert_bound(dw, dw_ref, e_dw, "d-wsp")
    assert torch.equal(dwa, dw0 + dw), "accumulate=1 adds the fp32 result"


@pytest.mark.parametrize("shape", BWD_SHAPES, ids=_ids)
def test_cbam_bwd_c(shape):
    f = _Fwd(*shape, seed=sum(shape) + 1, x_cs=shape[3] + 8)
    N, HW, C, nblk = f.N, f.HW, f.C, f.nblk
    gsmap = _randn(N, HW, 2, seed=3)

    def run():
        part = _nan(N, nblk, C)
        H.call("adh_cbam_bwd_c", f.g.data_ptr(), C + 4, f.xb.data_ptr(), f.x_cs, f.sa.data_ptr(), gsmap.data_ptr(),
               f.cidx.data_ptr(), N, HW, C, part.data_ptr(), nblk)
        return (part,)

    (part,) = _twice(run)
    ref, e = R.bwd_c64(f.gv, f.x, f.sa, gsmap, f.cidx)
    _assert_bound(part.double().sum(1), ref, e, "gca")


@pytest.mark.parametrize("N", [1, 5])
@pytest.mark.parametrize("C", [16, 96, 192, 384, 1024])
def test_cbam_bwd_d_mlp_gradients(N, C):
    """gpool, d-W1, d-W2 against float64 autograd of the MLP with the forward's hidden ReLU decisions (a unit whose
    pre-activation is exactly 0 passes no gradient, like torch's ReLU)."""
    f = _Fwd(N, 9, 11, C, seed=C + N)
    Ch, nblk = f.Ch, 3
    gcap = _randn(N, nblk, C, seed=C)
    dw10, dw20 = _randn(Ch, C, seed=1), _randn(C, Ch, seed=2)
    assert (f.hidden[:, :, 0] == 0).all()

    def run(acc):
        gpool = _nan(N, 2, C)
        dw1, dw2 = (dw10.clone(), dw20.clone()) if acc else (_nan(Ch, C), _nan(C, Ch))
        scratch = _nan(H.value("adh_cbam_bwd_d_scratch_floats", N, C, Ch))
        H.call("adh_cbam_bwd_d", gcap.data_ptr(), nblk, f.ca.data_ptr(), f.pooled.data_ptr(), f.hidden.data_ptr(),
               f.w1.data_ptr(), f.w2.data_ptr(), N, C, Ch, gpool.data_ptr(), dw1.data_ptr(), dw2.data_ptr(), acc,
               scratch.data_ptr())
        return gpool, dw1, dw2

    gpool, dw1, dw2 = _twice(lambda: run(0))
    _, dw1a, dw2a = run(1)
    assert torch.equal(dw1a, dw10 + dw1) and torch.equal(dw2a, dw20 + dw2), "accumulate=1"

    (gp, g1, g2), (tp, t1, t2), k = R.bwd_d64(gcap, f.ca, f.pooled, f.hidden, f.w1, f.w2)
    _assert_bound(gpool, gp, k * tp, "gpool")
    _assert_bound(dw1, g1, k * t1, "d-W1")
    _assert_bound(dw2, g2, k * t2, "d-W2")


@pytest.mark.parametrize("shape", BWD_SHAPES, ids=_ids)
def test_cbam_bwd_e_gradient_lands_on_the_first_index(shape):
    """gx = (g sa + gmean / C + gmax [c == cidx]) ca + gavg / HW + gpmax [p == amax_idx] on quantized input: the max-pool
    gradient must land exactly on amax_idx and the channel-max gradient exactly on cidx (both first-index ties)."""
    f = _Fwd(*shape, seed=sum(shape) + 2)
    N, HW, C = f.N, f.HW, f.C
    gsmap = _randn(N, HW, 2, seed=4) * 8
    gpool = _randn(N, 2, C, seed=5) * 8 * HW ** 0.5
    gx_cs = C + 12

    def run():
        gx = _nan(N, HW, gx_cs)
        H.call("adh_cbam_bwd_e", f.g.data_ptr(), C + 4, f.xb.data_ptr(), f.x_cs, f.ca.data_ptr(), f.sa.data_ptr(),
               gsmap.data_ptr(), f.cidx.data_ptr(), gpool.data_ptr(), f.amax.data_ptr(), N, HW, C, gx.data_ptr(), gx_cs)
        return (gx,)

    (gx,) = _twice(run)
    want, e = R.bwd_e64(f.gv, f.ca, f.sa, gsmap, f.cidx, gpool, f.amax)
    _assert_bound(gx[..., :C], want, e, "gx")
    assert torch.isnan(gx[..., C:]).all(), "written outside its channel slice"


# ------------------------------------------------------------------------------------------------ engine level
@pytest.mark.parametrize("C,Hh,Ww", [(192, 256, 512), (384, 128, 256)])
def test_engine_attention_product_widths_vs_float64(C, Hh, Ww):
    """Engine.attention forward and backward at the product widths and sizes (N = 2) against float64 autograd of
    _cbam_ref64.  x = k / 8 + 1e-3 u keeps the top-2 values of the pooling max well apart; the channel max of x * ca can
    still come within fp32 rounding of a tie, so pixels whose float64 top-2 gap is below 1e-5 of the max are left out of
    the input-gradient check (their gradient goes to a different channel in fp32)."""
    N, Ch = 2, C // 16
    x = _ints((N, Hh, Ww, C), -16, 16, seed=C) / 8 + 1e-3 * _rand(N, Hh, Ww, C, seed=C + 1)
    # one clear maximum per (image, channel): with HW = 131 072 the pooling max of k / 8 + 1e-3 u would tie in fp32, and
    # amax's backward splits a tie where the kernels (like torch.max) route the gradient to the first index
    ch = torch.arange(C, device=DEV)
    x.view(N, Hh * Ww, C)[:, (ch * 7919) % (Hh * Ww), ch] = 2.25 + 1e-3 * _rand(N, C, seed=C + 6)
    w1 = (_randn(Ch, C, 1, 1, seed=C + 2) / C ** 0.5).requires_grad_(True)
    w2 = (_randn(C, Ch, 1, 1, seed=C + 3) / Ch ** 0.5).requires_grad_(True)
    wsp = (_randn(1, 2, 7, 7, seed=C + 4) / 98 ** 0.5).requires_grad_(True)
    g = _randn(N, Hh, Ww, C, seed=C + 5)
    eng = Engine(torch.device(DEV), record=True)
    xa = Act(x.clone())
    o = eng.attention(xa, w1, w2, wsp)
    out = o.t.clone()
    o.grad = g
    eng.backward()
    torch.cuda.synchronize()

    x64 = x.double().requires_grad_(True)
    a1, a2, a3 = (t.detach().double().requires_grad_(True) for t in (w1, w2, wsp))
    ref = _cbam_ref64(x64, a1, a2, a3)
    assert float((out.double() - ref.detach()).abs().max()) <= 2e-5 * float(ref.detach().abs().max()), "forward"
    (ref * g.double()).sum().backward()
    with torch.no_grad():
        avg, mx = x64.mean((1, 2)), x64.amax((1, 2))
        fc = lambda v: torch.relu(v @ a1.flatten(1).t()) @ a2.flatten(1).t()
        xc = x64 * torch.sigmoid(fc(avg) + fc(mx))[:, None, None, :]
        top2 = xc.topk(2, dim=3).values
        clear = (top2[..., 0] - top2[..., 1]) > 1e-5 * top2[..., 0].abs().clamp_min(1e-3)
    err = (xa.grad.double() - x64.grad).abs()[clear]
    assert float(err.max()) <= 5e-5 * float(x64.grad.abs().max()), "input gradient"
    for p, want in ((w1, a1.grad), (w2, a2.grad), (wsp, a3.grad)):
        got = eng.param_grads[id(p)].double()
        assert float((got - want).abs().max()) <= 1e-4 * float(want.abs().max()), "weight gradient"


def test_cbam_bwd_e_past_the_grid_cap():
    """C = 1024, HW = 512 x 1040: 136M quads per image, past CBAM_SCALE_MAXBLK x 256 threads x 8 = 2^27, so the grid of
    adh_cbam_bwd_e is capped and each thread walks its pixels in more trips (2.2 GB per tensor).  Random ca, sa, gsmap,
    indices and gpool; the result is checked in row chunks after each of the two runs."""
    N, Hh, Ww, C = 1, 512, 1040, 1024
    HW = Hh * Ww
    g = _randn(N, HW, C, seed=21)
    ca, sa = _rand(N, C, seed=22), _rand(N, HW, seed=23)
    gsmap = _randn(N, HW, 2, seed=24)
    cidx = torch.randint(0, C, (N, HW), device=DEV, generator=_gen(25), dtype=torch.int32)
    amax = torch.randint(0, HW, (N, C), device=DEV, generator=_gen(26), dtype=torch.int32)
    gpool = _randn(N, 2, C, seed=27) * 64
    gx = torch.empty(N, HW, C, device=DEV)
    a = ca.double()[:, None, :]
    gavg, gmax = gpool[:, 0].double()[:, None, :], gpool[:, 1].double()[:, None, :]
    R = 16 * Ww
    for run in range(2):
        gx.fill_(NAN)
        H.call("adh_cbam_bwd_e", g.data_ptr(), C, g.data_ptr(), C, ca.data_ptr(), sa.data_ptr(), gsmap.data_ptr(),
               cidx.data_ptr(), gpool.data_ptr(), amax.data_ptr(), N, HW, C, gx.data_ptr(), C)
        torch.cuda.synchronize()
        for p0 in range(0, HW, R):
            p1 = min(HW, p0 + R)
            pos = torch.arange(p0, p1, device=DEV).view(1, -1, 1)
            onehot_c = torch.arange(C, device=DEV).view(1, 1, C) == cidx[:, p0:p1, None].long()
            onehot_p = pos == amax.long()[:, None, :]
            gv = g[:, p0:p1].double() * sa[:, p0:p1, None].double()
            gm, gxs = gsmap[:, p0:p1, 0:1].double(), gsmap[:, p0:p1, 1:2].double()
            want = (gv + gm / C + gxs * onehot_c) * a + gavg / HW + gmax * onehot_p
            terms = (gv.abs() + gm.abs() / C + gxs.abs() * onehot_c) * a + gavg.abs() / HW + gmax.abs() * onehot_p
            # as test_cbam_bwd_e_gradient_lands_on_the_first_index: 8 EPS of the terms
            _assert_bound(gx[:, p0:p1], want, 8 * EPS * terms, f"run {run}, pixels [{p0}, {p1})")
            del want, terms, gv, onehot_c, onehot_p
    del g, gx
    torch.cuda.empty_cache()
