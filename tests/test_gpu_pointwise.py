"""The glue kernels of csrc/pointwise.hip (pooling, resize, branch-head blends, image layout, routing, losses, gradient
helpers) through the C ABI, each against a float64 torch restatement of the same operation, at the edges the whole-branch
fixtures never reach: grid-stride loops past their block caps, the n % 4 tail of the loss reductions, MaxPool ties,
padded / overlapping windows, channel-slice inputs and outputs, clamp bounds hit exactly.

Every output and gradient buffer is prefilled with NaN: a kernel must write every element it owns, and everything outside
the channel slice it owns must still be NaN afterwards.  Every deterministic kernel runs twice and must reproduce itself
bit for bit.  Tolerances are relative to the float64 reference's largest magnitude unless a comment says otherwise, and
each comment says what in the kernel's fp32 arithmetic bounds it (EPS = 2^-24, the fp32 unit roundoff).  The restatements, case
builders and bounds this file shares with tests/test_pointwise_hostemu_cpu.py (the same source under the host sanitizers) are in
tests/_pointwise_ref64.py: they build CPU tensors, which are moved to the device here."""
import pytest
import torch
import torch.nn.functional as F

from adam_dehaze_amd import _hip as H
from adam_dehaze_amd.engine import Act, Engine
from tests import _pointwise_ref64 as P

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS = 2.0 ** -24


def _nan(*shape):
    return torch.full(shape, float("nan"), device=DEV, dtype=torch.float32)


def _gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def _rand(*shape, seed=0):
    return torch.rand(shape, device=DEV, dtype=torch.float32, generator=_gen(seed))


def _randn(*shape, seed=0):
    return torch.randn(shape, device=DEV, dtype=torch.float32, generator=_gen(seed))


def _rel(a, ref):
    """max|a - ref| / max|ref| (a's NaNs count as infinitely wrong)."""
    d = (a.double() - ref).abs()
    if torch.isnan(d).any():
        return float("inf")
    return float(d.max() / ref.abs().max().clamp_min(1e-300))


def _twice(fn):
    """Run `fn` (which returns a tuple of fresh tensors) twice; the runs must agree bit for bit (NaN where NaN)."""
    a = fn()
    b = fn()
    torch.cuda.synchronize()
    for i, (u, v) in enumerate(zip(a, b)):
        if u.is_floating_point():
            u, v = u.view(torch.int32), v.view(torch.int32)      # bit patterns: NaN == NaN, -0 != +0
        assert torch.equal(u, v), f"output {i} differs between two identical runs"
    return a


def _nchw64(t_nhwc):
    return t_nhwc.permute(0, 3, 1, 2).double().contiguous()


# ------------------------------------------------------------------------------------------------ MaxPool
MP_CFG = P.MP_CFG
MP_SHAPES = [(2, 7, 9, 16), (3, 33, 47, 64), (1, 5, 130, 96)]


def _rejected(name, *args):
    with pytest.raises(RuntimeError):
        H.call(name, *args)
    torch.cuda.synchronize()


def _check_maxpool(N, Hh, Ww, C, k, s, p, x_cs, g_cs, gx_cs, seed):
    xb, gb = (t.to(DEV) for t in P.maxpool_inputs(N, Hh, Ww, k, s, p, x_cs, g_cs, seed))      # ties everywhere, exact sums
    OH, OW = gb.shape[1], gb.shape[2]

    def run():
        out, idx = _nan(N, OH, OW, C), torch.full((N, OH, OW, C), -7, device=DEV, dtype=torch.int32)
        H.call("adh_maxpool", xb.data_ptr(), x_cs, N, Hh, Ww, C, k, s, p, out.data_ptr(), C, idx.data_ptr())
        gx = _nan(N, Hh, Ww, gx_cs)
        H.call("adh_maxpool_bwd", gb.data_ptr(), g_cs, idx.data_ptr(), N, OH, OW, C, k, s, p, Hh, Ww, gx.data_ptr(), gx_cs)
        return out, idx, gx

    out, idx, gx = _twice(run)
    y, ind, gref = P.maxpool_ref(xb[..., :C], gb[..., :C], k, s, p)
    assert torch.equal(_nchw64(out), y), "pooled values"
    assert torch.equal(idx.permute(0, 3, 1, 2).long(), ind), "arg-max indices (ties must go to the first in scan order)"
    assert torch.equal(_nchw64(gx[..., :C]), gref), "input gradient"
    assert torch.isnan(gx[..., C:]).all(), "gradient written outside its channel slice"


@pytest.mark.parametrize("shape", MP_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("cfg", MP_CFG, ids=lambda c: "k%ds%dp%d" % c)
def test_maxpool_ties_and_gradient_vs_float64(shape, cfg):
    N, Hh, Ww, C = shape
    _check_maxpool(N, Hh, Ww, C, *cfg, x_cs=C, g_cs=C, gx_cs=C, seed=sum(shape) + 10 * cfg[0])


def test_maxpool_channel_slices():
    # input read from a channel slice (x_cs = C + 8), gradient read from and written into wider buffers
    _check_maxpool(2, 33, 47, 16, 3, 2, 1, x_cs=24, g_cs=20, gx_cs=28, seed=5)


def test_maxpool_grid_stride_loop():
    # OH*OW*C/4 = 1.2M > 4096 blocks * 256 threads (forward), H*W*C = 19.2M (backward): both loops run several times
    _check_maxpool(1, 600, 1000, 32, 2, 2, 0, x_cs=32, g_cs=32, gx_cs=32, seed=6)


# ------------------------------------------------------------------------------------------------ bilinear resize
BL_CASES = P.BL_CASES


@pytest.mark.parametrize("case", BL_CASES, ids=lambda c: "%dx%dx%dx%d-%dx%d-a%d-xcs%d-ocs%d" % c)
def test_bilinear_fwd_bwd_vs_float64(case):
    N, Hh, Ww, C, OH, OW, align, x_cs, out_cs = case
    off = 4 if out_cs > C else 0
    xb, g = (t.to(DEV) for t in P.bilinear_inputs(N, Hh, Ww, C, OH, OW, x_cs))

    def run():
        ob = _nan(N, OH, OW, out_cs)
        H.call("adh_bilinear", xb.data_ptr(), x_cs, N, Hh, Ww, C, OH, OW, align, ob.data_ptr() + 4 * off, out_cs)
        gx = _nan(N, Hh, Ww, C)              # no zero-fill: the backward must write every element itself
        H.call("adh_bilinear_bwd", g.data_ptr(), C, N, Hh, Ww, C, OH, OW, align, gx.data_ptr(), C)
        return ob, gx

    ob, gx = _twice(run)
    y, gref = P.bilinear_ref(xb[..., :C], g, OH, OW, align)
    # both sides use ATen's source-coordinate formula; the kernel evaluates it in fp32 like ATen's fp32 path.  An error ds
    # in a coordinate moves an output by at most ds * (neighbour difference <= max|x| for x in [0, 1)) and a weight by ds.
    # backward: up to (2 * ratio + 1)^2 fp32 products summed per input element, in two levels (row sums, then rows)
    b_f, b_b, ds = P.bilinear_bounds(Hh, Ww, OH, OW, align)
    assert (b_f, b_b) == (4 * ds + 8 * EPS, 8 * ds + 64 * EPS)
    e_f = _rel(ob[..., off:off + C], y)
    assert e_f <= b_f, f"forward: {e_f:.3e} (source-coordinate error {ds:.3e})"
    e_b = _rel(gx, gref)
    assert e_b <= b_b, f"backward: {e_b:.3e} (source-coordinate error {ds:.3e})"
    if out_cs > C:
        assert torch.isnan(ob[..., :off]).all() and torch.isnan(ob[..., off + C:]).all(), "written outside its slice"


# ------------------------------------------------------------------------------------------------ average pooling
@pytest.mark.parametrize("shape", [(2, 9, 13, 16, 24, 16), (1, 33, 47, 64, 72, 80)], ids=["9x13", "33x47"])
def test_avgpool_k2_floor_slices(shape):
    N, Hh, Ww, C, x_cs, out_cs = shape
    xb = _rand(N, Hh, Ww, x_cs, seed=Hh)

    def run():
        ob = _nan(N, Hh // 2, Ww // 2, out_cs)
        H.call("adh_avgpool", xb.data_ptr(), x_cs, N, Hh, Ww, C, 2, ob.data_ptr(), out_cs)
        return (ob,)

    (ob,) = _twice(run)
    ref = F.avg_pool2d(_nchw64(xb[..., :C]), 2).permute(0, 2, 3, 1)
    # four fp32 adds and a multiply by the exact 1/4: <= 4 EPS of the window sum (x >= 0)
    assert _rel(ob[..., :C], ref) <= 4 * EPS
    assert torch.isnan(ob[..., C:]).all()


# ------------------------------------------------------------------------------------------------ global average pool
@pytest.mark.parametrize("C", [64, 1024, 1280, 2048])
@pytest.mark.parametrize("hw", [(1, 1), (7, 7), (23, 29), (31, 50)], ids=lambda s: "%dx%d" % s)
def test_global_avgpool_engine_fwd_bwd(C, hw):
    Hh, Ww = hw
    N = 2
    xb = _rand(N, Hh, Ww, C + 8, seed=C + Hh)       # a channel slice of a wider buffer (x.cs = C + 8)
    g = _randn(N, 1, 1, C, seed=C - Hh)

    def run():
        eng = Engine(torch.device(DEV), record=True)
        x = Act(xb[..., :C], C)
        o = eng.global_avgpool(x)
        o.grad = g
        eng.backward()
        return o.t.clone(), x.grad.clone()

    out, gx = _twice(run)
    ref = _nchw64(xb[..., :C]).mean(dim=(2, 3)).view(N, 1, 1, C)
    # 512-pixel fp32 partial sums per block, then the block partials: a random walk of ~sqrt(512 + blocks) roundings
    assert _rel(out, ref) <= 64 * EPS
    # backward = g * fp32(1 / HW): two roundings of each element
    gref = (g.double() / (Hh * Ww)).expand(N, Hh, Ww, C)
    assert float(((gx.double() - gref).abs() - 3 * EPS * gref.abs()).max()) <= 0


def test_global_avgpool_bwd_channel_slice():
    N, HW, C, gx_cs = 3, 667, 1280, 1292
    g = _randn(N, C, seed=1)

    def run():
        gx = _nan(N, HW, gx_cs)
        H.call("adh_global_avgpool_bwd", g.data_ptr(), N, HW, C, gx.data_ptr(), gx_cs)
        return (gx,)

    (gx,) = _twice(run)
    gref = (g.double() / HW)[:, None, :].expand(N, HW, C)
    assert float(((gx[..., :C].double() - gref).abs() - 3 * EPS * gref.abs()).max()) <= 0
    assert torch.isnan(gx[..., C:]).all()


# ------------------------------------------------------------------------------------------------ branch-head blends
_blend_ref = P.blend_ref


def _blend_inputs(mode, N, Hh, Ww, r_cs, gd_cs, seed):
    return tuple(t.to(DEV) for t in P.blend_inputs(mode, N, Hh, Ww, r_cs, gd_cs, seed))


def _check_head_blend(mode, N, Hh, Ww, r_cs, gd_cs, seed):
    x, rb, gdb = _blend_inputs(mode, N, Hh, Ww, r_cs, gd_cs, seed)
    alpha = torch.tensor([P.BLEND_ALPHA], device=DEV)
    g = _randn(N, 3, Hh, Ww, seed=seed + 3)
    nb = H.value("adh_head_blend_bwd_num_blocks", N, Hh, Ww)
    gated = mode in (2, 4)

    def run():
        out = _nan(N, 3, Hh, Ww)
        H.call("adh_head_blend", mode, x.data_ptr(), rb.data_ptr(), r_cs, gdb.data_ptr() if gated else None,
               gd_cs if gated else 0, alpha.data_ptr() if mode == 0 else None, N, Hh, Ww, out.data_ptr())
        g_r, g_gd, gap, ga = _nan(N, Hh, Ww, r_cs), _nan(N, Hh, Ww, gd_cs), _nan(nb), _nan(1)
        H.call("adh_head_blend_bwd", mode, g.data_ptr(), x.data_ptr(), rb.data_ptr(), r_cs,
               gdb.data_ptr() if gated else None, gd_cs if gated else 0, alpha.data_ptr() if mode == 0 else None,
               N, Hh, Ww, g_r.data_ptr(), g_gd.data_ptr() if gated else None, gap.data_ptr() if mode == 0 else None, nb)
        if mode == 0:
            H.call("adh_sum_partials", gap.data_ptr(), nb, 1.0, ga.data_ptr())
        return out, g_r, g_gd, ga

    out, g_r, g_gd, ga = _twice(run)
    y, gr_ref, ggd_ref, ga_ref, terms = P.blend_ref_grads(mode, x, rb, gdb, g)
    b_f, b_g, b_a = P.blend_bounds()
    assert (b_f, b_g, b_a) == (16 * EPS, 32 * EPS, 64 * EPS)
    # forward: expf / tanhf are faithful to a few ulp, then two or three fp32 operations on values of size <= 2
    assert float((out.double() - y).abs().max()) <= b_f, "forward"
    # gradients: products of a few faithfully rounded factors (the gate gradient adds three of them)
    assert _rel(g_r[..., :3], gr_ref) <= b_g, "g_r"
    assert torch.equal(g_r[..., 3:], torch.zeros_like(g_r[..., 3:])), "padding channels of g_r must be exactly 0"
    if gated:
        assert _rel(g_gd[..., :1], ggd_ref) <= b_g, "g_gd"
        assert torch.equal(g_gd[..., 1:], torch.zeros_like(g_gd[..., 1:])), "padding channels of g_gd must be exactly 0"
    else:
        assert torch.isnan(g_gd).all()
    if mode == 0:
        # fp32 sums per thread, wave and block, then fp64 over the block partials: relative to the sum of |terms|
        assert abs(float(ga) - ga_ref) <= b_a * terms, "alpha gradient"


@pytest.mark.parametrize("mode", [0, 1, 2, 3, 4])
def test_head_blend_all_modes(mode):
    _check_head_blend(mode, 2, 37, 53, 4, 4, seed=11 + mode)


def test_head_blend_wide_strides():
    # r_cs = 16, gd_cs = 8 on correctly sized gradient buffers: every channel past 3 (r) and past 0 (gd) is exactly 0
    for mode in (2, 4):
        _check_head_blend(mode, 2, 19, 23, 16, 8, seed=31 + mode)


@pytest.mark.parametrize("mode", [0, 2])
def test_head_blend_grid_stride_loop(mode):
    # 3 x 769 x 1031 = 2.38M pixels: past both the forward's 8192 and the backward's 4096 blocks of 256
    _check_head_blend(mode, 3, 769, 1031, 4, 4, seed=41 + mode)


def test_engine_head_blend_channel_slice_inputs():
    """Engine.head_blend with r and gd read from channel slices of wider buffers: the gradient buffers must be sized by the
    pixel strides the kernel writes (r.cs, gd.cs floats per pixel), not by the slices' channel counts."""
    N, Hh, Ww, mode = 2, 21, 27, 2
    x, rb, gdb = _blend_inputs(mode, N, Hh, Ww, 16, 8, seed=51)
    g = _randn(N, 3, Hh, Ww, seed=52)
    eng = Engine(torch.device(DEV), record=True)
    r, gd = Act(rb[..., :4], 3), Act(gdb[..., :4], 1)
    assert r.cs == 16 and gd.cs == 8
    out, holder = eng.head_blend(mode, x, r, gd, None)
    holder["g"] = g
    eng.backward()
    torch.cuda.synchronize()
    r64 = rb[..., :3].permute(0, 3, 1, 2).double().requires_grad_(True)
    gd64 = gdb[..., :1].permute(0, 3, 1, 2).double().requires_grad_(True)
    y = _blend_ref(mode, x.double(), r64, gd64, None)
    y.backward(g.double())
    assert float((out.double() - y.detach()).abs().max()) <= 16 * EPS
    assert _rel(r.grad[..., :3], r64.grad.permute(0, 2, 3, 1)) <= 32 * EPS
    assert _rel(gd.grad[..., :1], gd64.grad.permute(0, 2, 3, 1)) <= 32 * EPS


# ------------------------------------------------------------------------------------------------ image layout
def test_image_to_nhwc8_exact():
    N, Hh, Ww = 2, 1031, 1031            # 2.13M pixels: past the 8192-block cap
    img = _rand(N, 3, Hh, Ww, seed=61)

    def run():
        out = _nan(N, Hh, Ww, 8)
        H.call("adh_image_to_nhwc8", img.data_ptr(), N, Hh, Ww, out.data_ptr())
        return (out,)

    (out,) = _twice(run)
    assert torch.equal(out[..., :3], img.permute(0, 2, 3, 1))
    assert torch.equal(out[..., 3:], torch.zeros_like(out[..., 3:]))


def test_image_normalize_fwd_bwd():
    N, Hh, Ww = 2, 1031, 1031
    img = _rand(N, 3, Hh, Ww, seed=62)
    mean, std = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
    inv = [1.0 / s for s in std]
    g = _randn(N, Hh, Ww, 8, seed=63)

    def run():
        out = _nan(N, Hh, Ww, 8)
        H.call("adh_image_normalize_to_nhwc8", img.data_ptr(), N, Hh, Ww, *mean, *inv, out.data_ptr())
        gi = _nan(N, 3, Hh, Ww)
        H.call("adh_image_normalize_bwd", g.data_ptr(), 8, N, Hh, Ww, *inv, gi.data_ptr())
        return out, gi

    out, gi = _twice(run)
    m64 = torch.tensor(mean, device=DEV, dtype=torch.float64).view(1, 3, 1, 1)
    s64 = torch.tensor(std, device=DEV, dtype=torch.float64).view(1, 3, 1, 1)
    x64 = img.double().requires_grad_(True)
    y = (x64 - m64) / s64
    y.backward(g[..., :3].permute(0, 3, 1, 2).double())
    # (x - m) * fp32(1/s): the subtraction's rounding is relative to |x - m| (<= 1), the rest to the result
    ref = y.detach().permute(0, 2, 3, 1)
    assert float(((out[..., :3].double() - ref).abs() - 3 * EPS * (ref.abs() + 1 / 0.224)).max()) <= 0
    assert torch.equal(out[..., 3:], torch.zeros_like(out[..., 3:]))
    # g * fp32(1/s): two roundings
    assert float(((gi.double() - x64.grad).abs() - 3 * EPS * x64.grad.abs()).max()) <= 0


# ------------------------------------------------------------------------------------------------ routing
def _logits(N, seed):
    lg = _randn(N, 3, seed=seed) * 4
    lg[::7] = torch.tensor([80.0, -80.0, 3.0], device=DEV)
    lg[3::7] = torch.tensor([-80.0, -80.0, 80.0], device=DEV)
    return lg


def test_softmax3_fwd_bwd():
    N, nblk, T = 300, 3, 0.7
    lg = _logits(N, 71)
    gwp = _randn(N, nblk, 3, seed=72)

    def run():
        w, gl = _nan(N, 3), _nan(N, 3)
        H.call("adh_softmax3", lg.data_ptr(), T, N, w.data_ptr())
        H.call("adh_softmax3_bwd", w.data_ptr(), gwp.data_ptr(), nblk, T, N, gl.data_ptr())
        return w, gl

    w, gl = _twice(run)
    l64 = lg.double().requires_grad_(True)
    w64 = torch.softmax(l64 / T, dim=1)
    G = gwp.double().sum(1)
    w64.backward(G)
    # expf and one division per weight (weights <= 1)
    assert float((w.double() - w64.detach()).abs().max()) <= 8 * EPS
    # w * (g - dot) / T: a few roundings of terms bounded by max|G| / T
    assert float((gl.double() - l64.grad).abs().max()) <= 32 * EPS * float(G.abs().max()) / T


@pytest.mark.parametrize("null", [None, 0, 1, 2])
def test_soft_blend_fwd_bwd(null):
    N, per, nblk = 3, 3 * 44 * 53, 4      # per = 6996: a multiple of 4, not of 1024; 4 blocks of 256 lanes loop twice
    w = torch.softmax(_randn(N, 3, seed=81), dim=1).contiguous()
    o = [_rand(N, per, seed=82 + i) for i in range(3)]
    g = _randn(N, per, seed=85)

    def run():
        out = _nan(N, per)
        H.call("adh_soft_blend", w.data_ptr(), o[0].data_ptr(), o[1].data_ptr(), o[2].data_ptr(), N, per, out.data_ptr())
        gs = [None if i == null else _nan(N, per) for i in range(3)]
        gwp = _nan(N, nblk, 3)
        H.call("adh_soft_blend_bwd", w.data_ptr(), g.data_ptr(), o[0].data_ptr(), o[1].data_ptr(), o[2].data_ptr(), N, per,
               H.ptr(gs[0]), H.ptr(gs[1]), H.ptr(gs[2]), gwp.data_ptr(), nblk)
        return (out, gwp) + tuple(x for x in gs if x is not None)

    res = _twice(run)
    out, gwp, gs = res[0], res[1], list(res[2:])
    w64 = w.double().requires_grad_(True)
    o64 = [t.double() for t in o]
    y = sum(w64[:, i:i + 1] * o64[i] for i in range(3))
    y.backward(g.double())
    # three products and two adds of terms in [0, 1]
    assert float((out.double() - y.detach()).abs().max()) <= 8 * EPS
    for i in range(3):
        if i == null:
            continue
        ref = g.double() * w.double()[:, i:i + 1]
        assert float(((gs.pop(0).double() - ref).abs() - EPS * ref.abs()).max()) <= 0, f"g{i}: one rounded product"
    # weight gradients: fp32 per-lane sums, wave and block trees; relative to the sum of |terms|
    terms = torch.stack([(g.double() * o64[i]).abs().sum(1) for i in range(3)], 1)
    assert float(((gwp.double().sum(1) - w64.grad).abs() - 64 * EPS * terms).max()) <= 0


def test_argmax3_first_index_on_ties():
    N = 300
    lg = torch.randint(0, 2, (N, 3), device=DEV, generator=_gen(91)).float()    # ties in most rows
    lg[0] = torch.tensor([1.0, 1.0, 1.0], device=DEV)
    lg[1] = torch.tensor([-1.0, 2.0, 2.0], device=DEV)

    def run():
        idx = torch.full((N,), -5, device=DEV, dtype=torch.int64)
        H.call("adh_argmax3", lg.data_ptr(), N, idx.data_ptr())
        return (idx,)

    (idx,) = _twice(run)
    ref = torch.tensor([max(range(3), key=lambda j, row=row: (row[j], -j)) for row in lg.cpu().tolist()])
    assert torch.equal(idx.cpu(), ref)
    assert torch.equal(idx, torch.argmax(lg.double(), dim=1))


@pytest.mark.parametrize("N", [1, 37, 300])
def test_route_compact_stable(N):
    idx = torch.randint(0, 3, (N,), device=DEV, generator=_gen(N), dtype=torch.int64)

    def run():
        sel = torch.full((3 * N,), -1, device=DEV, dtype=torch.int32)
        cnt = torch.full((3,), -1, device=DEV, dtype=torch.int32)
        H.call("adh_route_compact", idx.data_ptr(), N, sel.data_ptr(), cnt.data_ptr())
        return sel, cnt

    sel, cnt = _twice(run)
    for c in range(3):
        want = (idx == c).nonzero().flatten().to(torch.int32)
        k = int(cnt[c])
        assert k == want.numel()
        assert torch.equal(sel[c * N:c * N + k], want), "members of a class must keep their batch order"
        assert (sel[c * N + k:(c + 1) * N] == -1).all()


def test_gather_scatter_images_round_trip():
    N, per = 5, 3 * 512 * 700          # per / 4 = 268800 > 1024 blocks * 256 lanes: the per-image loop runs twice
    src = _randn(N, per, seed=95)
    sel = torch.tensor([4, 0, 2], device=DEV, dtype=torch.int32)

    def run():
        dst = _nan(3, per)
        H.call("adh_gather_images", src.data_ptr(), sel.data_ptr(), 3, per, dst.data_ptr())
        back = _nan(N, per)
        H.call("adh_scatter_images", dst.data_ptr(), sel.data_ptr(), 3, per, back.data_ptr())
        return dst, back

    dst, back = _twice(run)
    assert torch.equal(dst, src[sel.long()])
    assert torch.equal(back[sel.long()], src[sel.long()])
    assert torch.isnan(back[[1, 3]]).all()


# ------------------------------------------------------------------------------------------------ losses
LOSS_N = P.LOSS_N


@pytest.mark.parametrize("sq", [0, 1], ids=["l1", "mse"])
@pytest.mark.parametrize("n", LOSS_N)
def test_diff_partial_sum_vs_float64(n, sq):
    a, b = _randn(n, seed=n), _randn(n, seed=n + 1)
    nblk = H.value("adh_reduce_num_blocks", n)

    def run():
        part, out = _nan(nblk), _nan(1)
        H.call("adh_mse_partial" if sq else "adh_l1_partial", a.data_ptr(), b.data_ptr(), n, part.data_ptr())
        H.call("adh_sum_partials", part.data_ptr(), nblk, 1.0 / n, out.data_ptr())
        return part, out

    _, out = _twice(run)
    d = a.double() - b.double()
    ref = float((d * d).mean() if sq else d.abs().mean())
    # all terms are >= 0: fp32 per-lane sums of 4-element pairs, wave and block trees (< 32 roundings deep in all), fp64 over
    # the blocks; 1e-6 relative bounds it with room to spare
    assert abs(float(out) - ref) <= 1e-6 * ref


def test_l1_bwd_sign_zero_and_mse_bwd():
    n = 4096 * 2048 + 5                  # past the 8192-block cap of the elementwise kernels
    a = _randn(n, seed=101)
    b = _randn(n, seed=102)
    b[::3] = a[::3]                      # a == b: torch's sign(0) = 0
    up = torch.tensor([0.75], device=DEV)
    a64, b64 = a.double(), b.double()
    for upstream in (None, up):
        u = 1.0 if upstream is None else 0.75

        def run():
            gl, gm = _nan(n), _nan(n)
            H.call("adh_l1_bwd", a.data_ptr(), b.data_ptr(), n, 1.0 / n, H.ptr(upstream), gl.data_ptr())
            H.call("adh_mse_bwd", a.data_ptr(), b.data_ptr(), n, 1.0 / n, H.ptr(upstream), gm.data_ptr())
            return gl, gm

        gl, gm = _twice(run)
        x = a64.clone().requires_grad_(True)
        ((x - b64).abs().mean() * u).backward()
        assert torch.equal(gl[::3], torch.zeros_like(gl[::3]))
        # +-fp32(fp32(1/n) * upstream): two roundings
        assert float(((gl.double() - x.grad).abs() - 3 * EPS * x.grad.abs()).max()) <= 0
        x = a64.clone().requires_grad_(True)
        (((x - b64) ** 2).mean() * u).backward()
        # 2 * fp32(a - b) * fp32(fp32(1/n) * upstream): four roundings
        assert float(((gm.double() - x.grad).abs() - 5 * EPS * x.grad.abs()).max()) <= 0


@pytest.mark.parametrize("N", [1, 7, 300])
def test_cross_entropy3_vs_float64(N):
    lg = _randn(N, 3, seed=N + 200) * 3
    lg[::2] *= 300                       # logits of order +-1e3 in every other row
    lab = torch.randint(0, 3, (N,), device=DEV, generator=_gen(N + 201), dtype=torch.int64)

    def run():
        loss, dl = _nan(1), _nan(N, 3)
        H.call("adh_cross_entropy3", lg.data_ptr(), lab.data_ptr(), N, loss.data_ptr(), dl.data_ptr())
        return loss, dl

    loss, dl = _twice(run)
    l64 = lg.double().requires_grad_(True)
    ref = F.cross_entropy(l64, lab)
    ref.backward()
    # per row, log(sum) + max - logit in fp32: a few roundings of terms as large as |max| + |logit|
    scale = float((lg.double().abs().max(1).values * 2 + 2).mean())
    assert abs(float(loss) - float(ref.detach())) <= 8 * EPS * scale
    # softmax / N - onehot / N: expf, a sum, two products, a division and a subtraction of terms <= 1 / N
    assert float((dl.double() - l64.grad).abs().max()) <= 16 * EPS / N


# ------------------------------------------------------------------------------------------------ gradient helpers
@pytest.mark.parametrize("P", [3 * 37 * 53, 800003])
def test_axpby_strided(P):
    C, dst_cs, src_cs = 12, 20, 16       # 800003 x 3 quads > 8192 blocks * 256: the loop runs twice
    src = _randn(P, src_cs, seed=P)
    d0 = _randn(P, dst_cs, seed=P + 1)

    def run():
        dst = _nan(P, dst_cs)            # a = 0 must not read dst: NaN * 0 would poison the result
        H.call("adh_axpby_strided", dst.data_ptr(), dst_cs, src.data_ptr(), src_cs, P, C, 0.0, 1.5)
        acc = d0.clone()
        acc[:, C:] = float("nan")
        H.call("adh_axpby_strided", acc.data_ptr(), dst_cs, src.data_ptr(), src_cs, P, C, 0.5, -2.0)
        return dst, acc

    dst, acc = _twice(run)
    assert torch.equal(dst[:, :C], src[:, :C] * 1.5), "a = 0: one exactly scaled product"
    assert torch.isnan(dst[:, C:]).all()
    ref = d0[:, :C].double() * 0.5 - 2.0 * src[:, :C].double()
    # d * 0.5 and s * -2 are exact; one rounding of the sum
    assert float(((acc[:, :C].double() - ref).abs() - EPS * ref.abs()).max()) <= 0
    assert torch.isnan(acc[:, C:]).all()


@pytest.mark.parametrize("n", [5, 255 * 8193, 2 * 256 * 8192 + 13])
def test_add_inplace_and_mul_exact(n):
    a, b = _randn(n, seed=n), _randn(n, seed=n + 1)

    def run():
        s = a.clone()
        H.call("adh_add_inplace", s.data_ptr(), b.data_ptr(), n)
        m = _nan(n)
        H.call("adh_mul", m.data_ptr(), a.data_ptr(), b.data_ptr(), n)
        return s, m

    s, m = _twice(run)
    # one correctly rounded operation each: equal to the float64 result rounded to fp32
    assert torch.equal(s, (a.double() + b.double()).float())
    assert torch.equal(m, (a.double() * b.double()).float())


# ------------------------------------------------------------------------------------------------ generic transposes
@pytest.mark.parametrize("HW", P.LAYOUT_HW)
@pytest.mark.parametrize("C", P.LAYOUT_C)
def test_nchw_nhwc_transposes_exact(C, HW):
    """32 x 32 tiles through LDS: channel and pixel counts on both sides of a tile edge, dense (cs = C) and into / out of a
    channel slice (cs = C + 5: the stores are scalar, so any stride is legal).  A bit-exact copy; the slack stays NaN."""
    N = 2
    src = P.randn(N, C, HW, 1, seed=C * 100 + HW).to(DEV)
    for cs in (C, C + 5):
        def run():
            nhwc = _nan(N, HW, 1, cs)
            H.call("adh_nchw_to_nhwc", src.data_ptr(), N, C, HW, 1, nhwc.data_ptr(), cs)
            back = _nan(N, C, 1, HW)                               # the same plane as 1 x HW: only H * W enters
            H.call("adh_nhwc_to_nchw", nhwc.data_ptr(), cs, N, C, 1, HW, back.data_ptr())
            return nhwc, back

        nhwc, back = _twice(run)
        assert torch.equal(nhwc[..., :C].view(torch.int32), src.permute(0, 2, 3, 1).contiguous().view(torch.int32))
        assert torch.isnan(nhwc[..., C:]).all(), "written outside its channel slice"
        assert torch.equal(back.view(N, C, HW).view(torch.int32), src.view(N, C, HW).view(torch.int32))


# ------------------------------------------------------------------------------------------------ single-tensor Adam
@pytest.mark.parametrize("step", [0, 7])
@pytest.mark.parametrize("repeats", [1, 2, 3])
@pytest.mark.parametrize("n", P.ADAM_STEP_N)
def test_adam_step_vs_float64(n, repeats, step):
    """adh_adam_step (in the C ABI, unused by the package) against the float64 Adam of tests/_ref64.py with its powf allowance;
    p, m and v sit in NaN guard bands, 257 and 1500 elements take more than one block."""
    kw = dict(lr=1e-3, beta1=float(torch.tensor(0.9)), beta2=float(torch.tensor(0.999)), eps=float(torch.tensor(1e-8)),
              wd=float(torch.tensor(1e-2)))
    p0, g, m0, v0 = P.adam_step_case(n, seed=n + 10 * repeats + step)
    gd = g.to(DEV)

    def run():
        bufs = []
        for t in (p0, m0, v0):
            whole = _nan(n + 32)
            whole[16:16 + n] = t.to(DEV)
            bufs.append(whole)
        p, m, v = (b[16:16 + n] for b in bufs)
        H.call("adh_adam_step", p.data_ptr(), gd.data_ptr(), m.data_ptr(), v.data_ptr(), n, step, kw["lr"], kw["beta1"],
               kw["beta2"], kw["eps"], kw["wd"], repeats)
        return tuple(bufs)

    bufs = _twice(run)
    (p, m, v), (ep, em, ev) = P.adam_step_ref(p0, g, m0, v0, step, repeats, **kw)
    for what, whole, ref, e in (("p", bufs[0], p, ep), ("m", bufs[1], m, em), ("v", bufs[2], v, ev)):
        got = whole[16:16 + n].cpu()
        assert not torch.isnan(got).any(), what
        over = float(((got.double() - ref).abs() - e).max())
        assert over <= 0, f"{what} is {over:.3e} over its bound"
        assert torch.isnan(whole[:16]).all() and torch.isnan(whole[16 + n:]).all(), f"{what}: written outside the tensor"


# ------------------------------------------------------------------------------------------------ argument rejections
def test_pool_and_resize_reject_bad_strides():
    """the buffer contract of include/adam_dehaze_hip.h: four channels per lane need cs % 4 == 0 and cs >= C; N, H, W >= 1.
    Every bad call raises and leaves its outputs NaN."""
    N, Hh, Ww, C = 2, 6, 8, 8
    x = _rand(N, Hh, Ww, 16, seed=1)
    out, idx = _nan(N, Hh, Ww, 16), torch.full((N, Hh, Ww, C), -7, device=DEV, dtype=torch.int32)
    for x_cs, out_cs, n, h, w in ((10, 8, N, Hh, Ww), (8, 10, N, Hh, Ww), (4, 8, N, Hh, Ww), (8, 4, N, Hh, Ww), (8, 8, 0, Hh, Ww),
                                  (8, 8, N, 0, Ww), (8, 8, N, Hh, 0), (8, 8, 65536, Hh, Ww)):
        _rejected("adh_maxpool", x.data_ptr(), x_cs, n, h, w, C, 2, 2, 0, out.data_ptr(), out_cs, idx.data_ptr())
        if h and w:
            _rejected("adh_avgpool", x.data_ptr(), x_cs, n, h, w, C, 2, out.data_ptr(), out_cs)
        _rejected("adh_bilinear", x.data_ptr(), x_cs, n, h, w, C, 3, 5, 0, out.data_ptr(), out_cs)
    # a base one float off 16-byte alignment
    _rejected("adh_maxpool", x.data_ptr() + 4, 8, N, Hh, Ww, C, 2, 2, 0, out.data_ptr(), 8, idx.data_ptr())
    _rejected("adh_avgpool", x.data_ptr(), 8, N, Hh, Ww, C, 2, out.data_ptr() + 4, 8)
    _rejected("adh_bilinear", x.data_ptr() + 8, 8, N, Hh, Ww, C, 3, 5, 1, out.data_ptr(), 8)
    assert torch.isnan(out).all() and (idx == -7).all()


def test_backward_entry_points_reject_bad_arguments():
    N, Hh, Ww, C = 2, 6, 8, 4
    g = _rand(N, 3, 4, 8, seed=2)
    idx = torch.zeros((N, 3, 4, C), device=DEV, dtype=torch.int32)
    gx = _nan(N, Hh, Ww, 8)
    ok = dict(g_cs=8, N=N, OH=3, OW=4, C=C, k=2, s=2, p=0, H=Hh, W=Ww, gx_cs=8)
    for bad in (dict(g_cs=3), dict(gx_cs=3), dict(N=0), dict(OH=0), dict(OW=5), dict(OH=4), dict(C=0), dict(H=0), dict(W=0),
                dict(p=-1), dict(p=2), dict(k=0), dict(s=0)):
        a = {**ok, **bad}
        _rejected("adh_maxpool_bwd", g.data_ptr(), a["g_cs"], idx.data_ptr(), a["N"], a["OH"], a["OW"], a["C"], a["k"], a["s"],
                  a["p"], a["H"], a["W"], gx.data_ptr(), a["gx_cs"])
    for g_cs, gx_cs, n in ((3, 8, N), (8, 3, N), (8, 8, 0)):
        _rejected("adh_bilinear_bwd", g.data_ptr(), g_cs, n, Hh, Ww, C, 3, 4, 0, gx.data_ptr(), gx_cs)
    gv = _rand(N, C, seed=3)
    for n, hw, c, gx_cs in ((N, 48, C, 3), (0, 48, C, 8), (N, 0, C, 8), (N, 48, 0, 8)):
        _rejected("adh_global_avgpool_bwd", gv.data_ptr(), n, hw, c, gx.data_ptr(), gx_cs)
    gi = _nan(N, 3, Hh, Ww)
    for g_cs, n, h, w in ((2, N, Hh, Ww), (8, 0, Hh, Ww), (8, N, 0, Ww), (8, N, Hh, 0)):
        _rejected("adh_image_normalize_bwd", gx.data_ptr(), g_cs, n, h, w, 1.0, 1.0, 1.0, gi.data_ptr())
    assert torch.isnan(gx).all() and torch.isnan(gi).all()


def test_head_blend_and_layout_reject_bad_sizes():
    N, Hh, Ww = 2, 5, 7
    x, rb, gdb = _blend_inputs(2, N, Hh, Ww, 4, 4, seed=4)
    alpha = torch.tensor([P.BLEND_ALPHA], device=DEV)
    out, g_r, g_gd, gap = _nan(N, 3, Hh, Ww), _nan(N, Hh, Ww, 4), _nan(N, Hh, Ww, 4), _nan(4)
    for n, h, w in ((0, Hh, Ww), (N, 0, Ww), (N, Hh, 0)):
        for mode in (0, 2):
            _rejected("adh_head_blend", mode, x.data_ptr(), rb.data_ptr(), 4, gdb.data_ptr(), 4, alpha.data_ptr(), n, h, w,
                      out.data_ptr())
            _rejected("adh_head_blend_bwd", mode, x.data_ptr(), x.data_ptr(), rb.data_ptr(), 4, gdb.data_ptr(), 4, alpha.data_ptr(),
                      n, h, w, g_r.data_ptr(), g_gd.data_ptr(), gap.data_ptr(), H.value("adh_head_blend_bwd_num_blocks", n, h, w))
        _rejected("adh_image_to_nhwc8", x.data_ptr(), n, h, w, g_r.data_ptr())
        _rejected("adh_nchw_to_nhwc", x.data_ptr(), n, 3, h, w, g_r.data_ptr(), 4)
        _rejected("adh_nhwc_to_nchw", rb.data_ptr(), 4, n, 3, h, w, out.data_ptr())
    _rejected("adh_head_blend", 2, x.data_ptr(), rb.data_ptr(), 2, gdb.data_ptr(), 4, alpha.data_ptr(), N, Hh, Ww, out.data_ptr())
    _rejected("adh_head_blend", 2, x.data_ptr(), rb.data_ptr(), 4, gdb.data_ptr(), 0, alpha.data_ptr(), N, Hh, Ww, out.data_ptr())
    _rejected("adh_nchw_to_nhwc", x.data_ptr(), N, 3, Hh, Ww, g_r.data_ptr(), 2)
    _rejected("adh_image_to_nhwc8", x.data_ptr(), N, Hh, Ww, g_r.data_ptr() + 4)                      # 16-byte stores
    assert all(torch.isnan(t).all() for t in (out, g_r, g_gd, gap))


def test_vector_paths_reject_unaligned_bases():
    """what moves 16 bytes per lane needs 16-byte aligned bases; the single-float paths (per % 4 != 0) take any"""
    N, per = 2, 16
    buf = _rand(4 * N * per + 8, seed=5)
    w = torch.softmax(_randn(N, 3, seed=6), dim=1).contiguous()
    o = [buf[i * N * per:(i + 1) * N * per] for i in range(3)]
    out, gwp, part = _nan(N * per + 4), _nan(N, 1, 3), _nan(4)
    sel = torch.tensor([1, 0], device=DEV, dtype=torch.int32)
    _rejected("adh_soft_blend", w.data_ptr(), o[0].data_ptr() + 4, o[1].data_ptr(), o[2].data_ptr(), N, per, out.data_ptr())
    _rejected("adh_soft_blend", w.data_ptr(), o[0].data_ptr(), o[1].data_ptr(), o[2].data_ptr(), N, per, out.data_ptr() + 4)
    _rejected("adh_soft_blend_bwd", w.data_ptr(), o[0].data_ptr(), o[0].data_ptr(), o[1].data_ptr(), o[2].data_ptr(), N, per,
              out.data_ptr() + 4, None, None, gwp.data_ptr(), 1)
    _rejected("adh_gather_images", o[0].data_ptr() + 4, sel.data_ptr(), N, per, out.data_ptr())
    _rejected("adh_scatter_images", o[0].data_ptr(), sel.data_ptr(), N, per, out.data_ptr() + 4)
    _rejected("adh_l1_partial", o[0].data_ptr() + 4, o[1].data_ptr(), per, part.data_ptr())
    _rejected("adh_mse_partial", o[0].data_ptr(), o[1].data_ptr() + 4, per, part.data_ptr())
    _rejected("adh_axpby_strided", out.data_ptr() + 4, 8, o[0].data_ptr(), 8, 2, 8, 0.0, 1.0)
    _rejected("adh_axpby_strided", out.data_ptr(), 4, o[0].data_ptr(), 8, 2, 8, 0.0, 1.0)                # dst_cs < C
    assert all(torch.isnan(t).all() for t in (out, gwp, part))
    # the scalar path at the same unaligned base is legal
    H.call("adh_soft_blend", w.data_ptr(), o[0].data_ptr() + 4, o[1].data_ptr(), o[2].data_ptr(), N, per - 1, out.data_ptr() + 4)
    torch.cuda.synchronize()
    assert not torch.isnan(out[1:1 + N * (per - 1)]).any() and torch.isnan(out[0])
