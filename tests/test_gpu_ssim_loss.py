"""csrc/ssim_loss.hip through the C ABI against float64 (tests/_ssim_ref64.py), then the layers above it: the autograd
function, SSIMLoss, DehazingLoss(lambda_ssim), a branch trained through it, and the training step.

Conventions of tests/test_gpu_train_io.py: every output is prefilled with NaN and sits inside a NaN guard band that must
still be NaN afterwards; every entry point runs twice and must reproduce itself bit for bit."""
import warnings

import pytest
import torch

import adam_dehaze_amd as A
from adam_dehaze_amd import _hip as H
from adam_dehaze_amd import loss as L
from adam_dehaze_amd.metrics import ssim_batch
from oracle import ref_cpu as R
from tests import _ssim_ref64 as S64
from tests._util import DEV, EPS, _assert_bound, _pad_untouched, _padded, _same_bits, _twice, kink_audit, kink_matched, kink_recording, oracle_with_masks

pytestmark = pytest.mark.gpu
U53 = 2.0 ** -53

# The kernel's tile (csrc/ssim_loss.hip): SSIML_T x SSIML_T output pixels per workgroup, tiles laid over the H x W pixels.
# 32 and 64 fill the last tile exactly; 33 and 65 leave a last tile one pixel high / wide, each direction with the other full.
SSIML_T = 32
TILE_EDGE_HW = [(SSIML_T, SSIML_T + 1), (SSIML_T + 1, SSIML_T), (2 * SSIML_T, 2 * SSIML_T + 1), (2 * SSIML_T + 1, 2 * SSIML_T)]
SIZES = [(7, 7), (8, 9), (13, 13), (14, 20), (7, 39), (39, 7), (38, 38), (39, 39), (45, 131)] + TILE_EDGE_HW
KINDS = ["random", "noise", "identical", "const_pred", "two_constants", "wide_range"]

# Float64 part of the kernel, in units u = 2^-53 of the sum of |terms| that tests/_ssim_ref64.py::closed_form returns.
# M = 1.5 bounds |gray| over the input kinds below, C1 = 1e-4, C2 = 9e-4 (data_range 1).
#   a window mean: 48 additions, the product under it, 1/49 rounded and applied: 51 u of the mean of absolute values
#   A1 = 2 mx my + C1: 51 + 51 + 1 for the product, 1 for the sum: 104 u of its absolute terms;  A2 = 2 cn (mxy - mx my) + C2:
#     51 for mxy, 103 for mx my, the difference, cn (rounded) and the sum: 107 u of its absolute terms
#   B1 = mx^2 + my^2 + C1: d(mx^2) <= 102 u mean|x| |mx|, and |mx| mean|x| / (mx^2 + C1) <= M / (2 sqrt C1) = 75: 7650 u for
#     x, as much for y, the sums:  k1 = 15400 u of B1 itself
#   B2 = vx + vy + C2: each variance cancels, d(vx) <= cn (51 mxx + 102 mean|x| |mx| + mx^2 + 2) u <= 164 M^2 u, and B2 >= C2:
#     k2 = 2 * 164 * 2.25 / 9e-4 = 820000 u of B2 itself -- the conditioning of SSIM's variance denominator, which the
#     float64 statistics are there to pay for
#   the worst term, cn mx S / B2 = cn mx A1 A2 / (B1 B2^2) (b has the same denominators): 51 + 104 + 107 + k1 + 2 k2, the three
#     reciprocals and six products: <= 280 more: 1,655,700 u
#   the three additions inside a, the 48 additions of each box sum, 2 x sb and y sc, two additions, the coefficient
#     g / (3 * 49 * OH * OW) and its product: <= 60 u
# 1,655,760 u for the kernel.  The reference is the same function evaluated in float64 by other means (window means by
# avg_pool2d, the gradient by autograd through the same denominators), so it is granted as much: 3.4e6 <= 2^22.
# An fp32 accumulation anywhere behind the grayscale costs >= 2^-24 of the terms = 2^7 of this bound.
SSIM_BWD_F64_UNITS = 2.0 ** 22


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _inputs(kind, N, Hh, Ww):
    """(pred, target) fp32 on the CPU."""
    gen = _gen(Hh * 1000 + Ww * 7 + N)
    t = torch.rand(N, 3, Hh, Ww, generator=gen)
    if kind == "random":
        p = torch.rand(N, 3, Hh, Ww, generator=gen)
    elif kind == "noise":                                   # the cancellation regime: 2 x sum b against y sum c
        p = t + 0.002 * torch.randn(N, 3, Hh, Ww, generator=gen)
    elif kind == "identical":
        p = t.clone()
    elif kind == "const_pred":
        p = torch.full_like(t, 0.4)
    elif kind == "two_constants":
        t = torch.full_like(t, 0.3)
        p = torch.full_like(t, 0.8)
    else:                                                   # LightweightDehazeModel's output is not clamped
        p = 2.0 * torch.rand(N, 3, Hh, Ww, generator=gen) - 0.5
        t = 2.0 * torch.rand(N, 3, Hh, Ww, generator=gen) - 0.5
    return p, t


def _upstream(N):
    """g_ssim as the kernel reads it (fp32): mixed signs, and for N = 3 one exact zero (image 1)."""
    return torch.tensor([0.7, 0.0, -1.3] if N > 1 else [-1.3], dtype=torch.float32)[:N]


def _launch(p, t, g, data_range=1.0):
    """adh_ssim_gray_bwd on device tensors, twice, into NaN-filled guarded buffers; returns the gradient [N,3,H,W]."""
    N, _, Hh, Ww = p.shape
    n = p.numel()

    def run():
        whole, out = _padded(n)
        H.call("adh_ssim_gray_bwd", p.data_ptr(), t.data_ptr(), N, Hh, Ww, data_range, g.data_ptr(), out.data_ptr())
        torch.cuda.synchronize()
        assert _pad_untouched(whole, n)
        return (out,)
    (out,) = _twice(run)
    return out.view(N, 3, Hh, Ww)


def _check_kernel(kind, N, Hh, Ww):
    p, t = _inputs(kind, N, Hh, Ww)
    gl = _upstream(N)
    (val, ref), terms = S64.ssim_and_grad(p, t, gl.double())
    got = _launch(p.to(DEV), t.to(DEV), gl.to(DEV))
    assert _same_bits(got[:, 0], got[:, 1]) and _same_bits(got[:, 0], got[:, 2])       # one value per pixel, three stores
    bound = EPS * ref.abs() + SSIM_BWD_F64_UNITS * U53 * terms.expand_as(ref)
    _assert_bound(got.cpu(), ref, bound, f"ssim bwd {kind} N={N} {Hh}x{Ww}")
    for n, gv in enumerate(gl.tolist()):
        if gv == 0.0:
            assert bool((got[n] == 0).all()) and not bool(torch.signbit(got[n]).any()), "g_ssim = 0: exact +0.0 expected"
    return got, ref


@pytest.mark.parametrize("N", [1, 3])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("Hh,Ww", SIZES)
def test_ssim_bwd_kernel_vs_float64(Hh, Ww, kind, N):
    """Bound per element: EPS |ref| (the one fp32 rounding, at the store) + SSIM_BWD_F64_UNITS * 2^-53 * sum|terms|."""
    _check_kernel(kind, N, Hh, Ww)


def test_ssim_bwd_kernel_full_size():
    """one launch at 1 x 512 x 1024 (16 x 32 tiles), in the cancellation regime."""
    got, ref = _check_kernel("noise", 1, 512, 1024)
    assert float(ref.abs().max()) > 0


def test_ssim_bwd_rejections_leave_the_output_untouched():
    N, Hh, Ww = 2, 9, 12
    p, t = (x.to(DEV) for x in _inputs("random", N, Hh, Ww))
    g = torch.tensor([0.5, -0.5], device=DEV)
    whole, out = _padded(p.numel())
    p0, t0 = p.clone(), t.clone()

    def rejected(match, *args):
        with pytest.raises(RuntimeError, match=match):
            H.call("adh_ssim_gray_bwd", *args)
        torch.cuda.synchronize()

    for hh, ww in ((6, 12), (9, 6), (6, 6)):
        rejected("UNSUPPORTED", p.data_ptr(), t.data_ptr(), N, hh, ww, 1.0, g.data_ptr(), out.data_ptr())
    rejected("ADH_E_ARG", None, t.data_ptr(), N, Hh, Ww, 1.0, g.data_ptr(), out.data_ptr())
    rejected("ADH_E_ARG", p.data_ptr(), None, N, Hh, Ww, 1.0, g.data_ptr(), out.data_ptr())
    rejected("ADH_E_ARG", p.data_ptr(), t.data_ptr(), N, Hh, Ww, 1.0, None, out.data_ptr())
    rejected("ADH_E_ARG", p.data_ptr(), t.data_ptr(), N, Hh, Ww, 1.0, g.data_ptr(), None)
    rejected("ADH_E_ARG", p.data_ptr(), t.data_ptr(), 0, Hh, Ww, 1.0, g.data_ptr(), out.data_ptr())
    rejected("ADH_E_ARG", p.data_ptr(), t.data_ptr(), 65536, Hh, Ww, 1.0, g.data_ptr(), out.data_ptr())
    # the gradient may not be (or overlap) an image it is computed from
    rejected("ADH_E_ARG", p.data_ptr(), t.data_ptr(), N, Hh, Ww, 1.0, g.data_ptr(), p.data_ptr())
    rejected("ADH_E_ARG", p.data_ptr(), t.data_ptr(), N, Hh, Ww, 1.0, g.data_ptr(), t.data_ptr())
    rejected("ADH_E_ARG", p.data_ptr(), t.data_ptr(), 1, Hh, Ww, 1.0, g.data_ptr(), p[1].data_ptr() - 4 * Ww)
    assert bool(torch.isnan(whole).all())
    assert _same_bits(p, p0) and _same_bits(t, t0)


# ------------------------------------------------------------------------------------------------ autograd
def test_ssim_per_image_autograd():
    N, Hh, Ww = 3, 21, 45
    p, t = _inputs("noise", N, Hh, Ww)
    w = _upstream(N)
    (val, ref), terms = S64.ssim_and_grad(p, t, w.double())
    pd, td = p.to(DEV).requires_grad_(True), t.to(DEV).requires_grad_(True)
    out = L.ssim_per_image(pd, td)
    assert out.shape == (N,) and out.requires_grad
    assert _same_bits(out.detach(), ssim_batch(pd.detach(), td.detach()))
    (out * w.to(DEV)).sum().backward()
    assert td.grad is None
    _assert_bound(pd.grad.cpu(), ref, EPS * ref.abs() + SSIM_BWD_F64_UNITS * U53 * terms.expand_as(ref), "ssim_per_image grad")
    assert bool((pd.grad[1] == 0).all())
    # the batch's input checks are ssim_batch's
    with pytest.raises(ValueError, match="win_size exceeds image extent"):
        L.ssim_per_image(pd[:, :, :6], td[:, :, :6])
    with pytest.raises(RuntimeError):
        L.ssim_per_image(pd, td[:2])


def test_ssim_per_image_without_grad_launches_no_backward(monkeypatch):
    calls = []
    real = H.call

    def spy(name, *a, **k):
        calls.append(name)
        return real(name, *a, **k)
    monkeypatch.setattr(H, "call", spy)
    p, t = (x.to(DEV) for x in _inputs("random", 2, 16, 16))
    out = L.ssim_per_image(p, t.requires_grad_(True))
    assert not out.requires_grad and out.grad_fn is None
    with torch.no_grad():
        out2 = L.SSIMLoss()(p.clone().requires_grad_(True), t)
    assert not out2.requires_grad
    # a graph in which only something else needs the gradient: the SSIM backward is never reached
    s = torch.ones((), device=DEV, requires_grad=True)
    (L.ssim_per_image(p, t).sum() * s).backward()
    torch.cuda.synchronize()
    assert "adh_ssim_gray" in calls and "adh_ssim_gray_bwd" not in calls
    pg = p.clone().requires_grad_(True)
    L.SSIMLoss()(pg, t).backward()
    assert calls.count("adh_ssim_gray_bwd") == 1 and pg.grad is not None


# ------------------------------------------------------------------------------------------------ DehazingLoss
def test_dehazing_loss_with_ssim_term():
    N, Hh, Ww = 2, 24, 40
    p, t = _inputs("random", N, Hh, Ww)
    pd, td = p.to(DEV).requires_grad_(True), t.to(DEV)
    crit = L.DehazingLoss(content=False, perceptual=False, lambda_ssim=0.5).to(DEV)
    total, comps = crit(pd, td)
    assert set(comps) == {"l1", "content", "perceptual", "ssim", "total"}
    sb = ssim_batch(pd.detach(), td).double()
    l1 = float(comps["l1"].detach().double())
    mean = float(sb.mean())
    expect = l1 + 0.5 * (1.0 - mean)
    # fp32: the batch mean (an addition and a division), 1 - mean, the product with 0.5 is exact, one addition to l1
    assert abs(float(total.detach().double()) - expect) <= 4 * EPS * (abs(l1) + 1.0 + abs(mean))
    assert abs(float(comps["ssim"].detach().double()) - (1.0 - mean)) <= 3 * EPS * (1.0 + abs(mean))
    total.backward()
    # float64 reference of the sum: sign(p - t) / numel  -  0.5 / N * d ssim[n] / d pred
    (val, gs), terms = S64.ssim_and_grad(p, t, [-0.5 / N] * N)
    gl1 = torch.sign(p.double() - t.double()) / p.numel()
    ref = gl1 + gs
    # L1 backward: 1 / numel rounded to fp32 and one product; SSIM backward: its own bound, with the fp32 upstream
    # -0.5 / N exact; autograd's accumulation of the two: one fp32 addition
    bound = EPS * (2 * gl1.abs() + gs.abs() + ref.abs()) + SSIM_BWD_F64_UNITS * U53 * terms.expand_as(ref)
    _assert_bound(pd.grad.cpu(), ref, bound, "DehazingLoss(lambda_ssim=0.5) grad")

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        plain = L.DehazingLoss(content=False, perceptual=False).to(DEV)
        zero = L.DehazingLoss(content=False, perceptual=False, lambda_ssim=0).to(DEV)
    ta, ca = plain(pd.detach(), td)
    tb, cb = zero(pd.detach(), td)
    assert _same_bits(ta, tb) and set(ca) == set(cb) == {"l1", "content", "perceptual", "total"}


# ------------------------------------------------------------------------------------------------ composition
def test_branch_trained_through_ssim_loss_vs_float64_oracle():
    """LightweightDehazeModel(base_channels=8, n_blocks=1), train mode, SSIMLoss alone on 2 x 3 x 24 x 40: every parameter
    gradient against the oracle branch followed by tests/_ssim_ref64.py, both in float64, with the ReLU masks the kernels
    used replayed in the oracle.  Gate and tolerance are those tests/test_gpu_parity.py::test_branches_vs_reference_fixtures
    applies to light_b8: err_gpu <= 3 * err_ref + 3e-4 of the tensor's scale, err_ref the distance of the fp32 CPU oracle from
    its float64 twin (both free-running); a tensor whose true gradient is 0 (scale < 1e-6) must stay below 1e-6."""
    torch.manual_seed(7)
    m = A.LightweightDehazeModel(base_channels=8, n_blocks=1)
    sd_cpu = {k: v.clone() for k, v in m.state_dict().items()}
    hazy, clear, _ = R.synthetic_batch(2, 24, 40, seed=11)

    def oracle(dtype):
        sd = {k: (v.clone().to(dtype) if v.is_floating_point() else v.clone()) for k, v in sd_cpu.items()}
        for k, v in sd.items():
            if v.is_floating_point() and "running" not in k:
                v.requires_grad_(True)
        out = R.lightweight_forward(hazy.to(dtype), sd, training=True)
        loss = 1.0 - S64.ssim_of_images(out, clear.to(dtype)).mean()
        loss.backward()
        return float(loss.detach()), {k: v.grad for k, v in sd.items() if v.is_floating_point() and "running" not in k}

    with kink_recording() as rec32:
        _, g32_free = oracle(torch.float32)
    with kink_recording() as rec64:
        _, g64_free = oracle(torch.float64)
    m = m.to(DEV).train()
    with kink_matched(m) as km:
        out = m(hazy.to(DEV))
        loss = L.SSIMLoss()(out, clear.to(DEV))
        loss.backward()
    torch.cuda.synchronize()
    # the masks about to be replayed against the ones float64 chose on its own (tests/_util.py kink_audit)
    audit = kink_audit("ssim branch light_b8", rec64, family="branches", masks=km.masks(), post=km.post(), rec32=rec32)
    loss64, g64 = oracle_with_masks(lambda: oracle(torch.float64), km.masks(), audit=audit)
    assert abs(float(loss.detach()) - loss64) < 1e-3                  # BASELINE.json north_star: losses within 1e-3 fp32
    bad, seen = [], 0
    for name, p in m.named_parameters():
        ref = g64[name]
        g = (p.grad.cpu() if p.grad is not None else torch.zeros_like(ref)).double()
        scale = max(float(ref.abs().max()), 1e-8)
        if scale < 1e-6:
            assert float(g.abs().max()) < 1e-6, name
            continue
        err_ref = float((g32_free[name].double() - g64_free[name]).abs().max()) / scale
        err_gpu = float((g - ref).abs().max()) / scale
        print(f"[ssim branch] {name:40s} scale {scale:.2e} err_ref {err_ref:.2e} err_gpu {err_gpu:.2e}")
        seen += 1
        if not err_gpu <= 3.0 * err_ref + 3e-4:
            bad.append((name, err_gpu, err_ref))
    assert seen >= 4 and not bad, bad[:8]


def test_training_step_with_ssim_term():
    from adam_dehaze_amd.optim import Adam
    from adam_dehaze_amd.train import dehazing_train_step
    torch.manual_seed(3)
    m = A.LightweightDehazeModel(base_channels=8, n_blocks=1).to(DEV).train()
    crit = L.DehazingLoss(content=False, perceptual=False, lambda_ssim=0.4).to(DEV)     # L1 + SSIM: no extractor needed
    opt = Adam(m.parameters(), lr=1e-3, weight_decay=1e-4)
    hazy, clear, labels = R.synthetic_batch(2, 24, 40, seed=5)
    batch = {"hazy": hazy, "clear": clear, "intensity": labels}
    before = [p.detach().clone() for p in m.parameters()]
    for _ in range(2):
        st = dehazing_train_step(m, crit, opt, batch, None, torch.device(DEV))
        assert set(st) == {"loss", "l1", "ssim"}
        vals = {k: float(v) for k, v in st.items()}
        assert all(v == v and abs(v) != float("inf") for v in vals.values()), vals
        assert 0.0 <= vals["ssim"] <= 2.0
        assert abs(vals["loss"] - (vals["l1"] + 0.4 * vals["ssim"])) < 1e-5
    assert any(not torch.equal(a, p.detach()) for a, p in zip(before, m.parameters()))
    assert all(bool(torch.isfinite(p).all()) for p in m.parameters())
