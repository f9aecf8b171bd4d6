"""csrc/msssim.hip through the C ABI against float64 (tests/_msssim_ref64.py), then the layers above it: metrics.ssim_gaussian_batch
and ms_ssim_batch, loss.ms_ssim_per_image, MSSSIMLoss, DehazingLoss(lambda_msssim), the two training steps and the demo scores.

Every comparison is against the float64 reference on the same fp32 inputs, with the bounds of tests/_msssim_cases.py: the
operation count of tests/_msssim_ref64.py (FWD_UNITS = 2^21, BWD_UNITS = 2^22 units of 2^-53 of the |terms|) plus 2^-24 |ref| for
the one fp32 store.  Outputs of the C ABI are prefilled with NaN inside NaN guard bands; every entry point runs twice and must
reproduce itself bit for bit.  The worst |err| / bound of each case is printed before it is asserted."""
import json
import math
import os
import warnings

import numpy as np
import pytest
import torch

import adam_dehaze_amd as A
from adam_dehaze_amd import _hip as H
from adam_dehaze_amd import image_io as IO
from adam_dehaze_amd import loss as L
from adam_dehaze_amd import metrics as M
from adam_dehaze_amd import train as T
from tests import _msssim_cases as K
from tests import _msssim_ref64 as R64
from tests._util import DEV, EPS, _pad_untouched, _padded, _same_bits, _twice

pytestmark = pytest.mark.gpu
F64 = torch.float64
W3 = (0.3, 0.3, 0.4)


# ------------------------------------------------------------------------------------------------ one level, C ABI
def _level_fwd(x, y, data_range, pool=True):
    N, _, Hh, Ww = x.shape
    ntiles = H.value("adh_msssim_num_tiles", Hh, Ww)
    PH, PW = Hh // 2, Ww // 2

    def run():
        bufs = [_padded(n, dtype=F64) for n in (N * 3, N * 3, N * 3 * PH * PW, N * 3 * PH * PW)]
        partial = torch.full((N * 3 * ntiles * 2,), float("nan"), device=DEV, dtype=F64)
        H.call("adh_msssim_level_fwd", x.data_ptr(), y.data_ptr(), int(x.dtype == F64), N, Hh, Ww, float(data_range),
               partial.data_ptr(), ntiles, bufs[0][1].data_ptr(), bufs[1][1].data_ptr(),
               bufs[2][1].data_ptr() if pool else None, bufs[3][1].data_ptr() if pool else None)
        torch.cuda.synchronize()
        for (whole, own), n in zip(bufs, (N * 3, N * 3, N * 3 * PH * PW, N * 3 * PH * PW)):
            assert _pad_untouched(whole, n)
        assert not bool(torch.isnan(partial).any())
        return tuple(own for _, own in bufs)
    S, CS, qx, qy = _twice(run)
    return S.view(N, 3).cpu(), CS.view(N, 3).cpu(), qx.view(N, 3, PH, PW), qy.view(N, 3, PH, PW)


def _level_bwd(x, y, ca, cb, data_range, g_coarse=None, out_f64=False):
    N, _, Hh, Ww = x.shape
    n = x.numel()

    def run():
        whole, out = _padded(n, dtype=F64 if out_f64 else torch.float32)
        H.call("adh_msssim_level_bwd", x.data_ptr(), y.data_ptr(), int(x.dtype == F64), N, Hh, Ww, float(data_range),
               ca.data_ptr(), cb.data_ptr(), H.ptr(g_coarse), out.data_ptr(), int(out_f64))
        torch.cuda.synchronize()
        assert _pad_untouched(whole, n)
        return (out,)
    (out,) = _twice(run)
    assert not bool(torch.isnan(out).any()), "an element was not written"
    return out.view(N, 3, Hh, Ww)


@pytest.mark.parametrize("data_range", [1.0, 255.0])
@pytest.mark.parametrize("N", [1, 3])
@pytest.mark.parametrize("Hh,Ww", K.ISSUE_SHAPES + K.TILE_EDGE_SHAPES)
def test_one_level_forward_and_backward_vs_float64(Hh, Ww, N, data_range):
    worst = {"ssim": 0.0, "cs": 0.0, "pool": 0.0, "grad": 0.0}
    for kind in K.KINDS:
        x, y = K.inputs(kind, N, Hh, Ww, data_range)
        xd, yd = x.to(DEV), y.to(DEV)
        S, CS, qx, qy = _level_fwd(xd, yd, data_range)
        (rS, rCS), (bS, bCS) = K.fwd_reference(x, y, data_range)
        worst["ssim"] = max(worst["ssim"], K.worst(S, rS, bS))
        worst["cs"] = max(worst["cs"], K.worst(CS, rCS, bCS))
        for q, src in ((qx, x), (qy, y)):
            ref, bound = K.pool_reference(src)
            worst["pool"] = max(worst["pool"], K.worst(q.cpu(), ref, bound))
        S1, CS1, _, _ = _level_fwd(xd[:1].contiguous(), yd[:1].contiguous(), data_range, pool=False)
        assert _same_bits(S1, S[:1]) and _same_bits(CS1, CS[:1]), "image 0 alone differs from image 0 in the batch"
        if kind == "identical":
            assert bool((S.float() == 1.0).all()) and bool((CS.float() == 1.0).all())
        for a, b in K.COEFS:
            ca, cb = K.coef_planes(N, a, b)
            g = _level_bwd(xd, yd, ca.to(DEV), cb.to(DEV), data_range)
            ref, bound = K.bwd_reference(x, y, ca, cb, data_range)
            worst["grad"] = max(worst["grad"], K.worst(g.cpu(), ref, bound))
            z = g[N - 1, 1]
            assert bool((z == 0).all()) and not bool(torch.signbit(z).any()), "a = b = 0: exact +0.0 expected"
    print(f"[msssim level] {N}x3x{Hh}x{Ww} R={data_range}: worst |err| / bound " + " ".join(f"{k} {v:.3g}" for k, v in worst.items()))
    assert max(worst.values()) <= 1.0, worst


def test_float64_level_with_the_pool_adjoint():
    """a pooled level as the pyramid runs it: float64 in, float64 gradient out, then level 0 folding it in; 27 x 47 -> 13 x 23"""
    x, y = K.inputs("noise", 2, 27, 47)
    xd, yd = x.to(DEV), y.to(DEV)
    _, _, x1, y1 = _level_fwd(xd, yd, 1.0)
    rx1, ry1 = R64.pool(x.double()), R64.pool(y.double())
    S1, _, _, _ = _level_fwd(x1, y1, 1.0, pool=False)
    (rS1, _), (bS1, _) = K.fwd_reference(rx1, ry1, 1.0)
    a1, zero = torch.tensor([[0.6, -0.2, 0.0], [0.1, 0.2, 0.3]], dtype=F64), torch.zeros(2, 3, dtype=F64)
    b0 = torch.tensor([[0.5, 0.0, 0.0], [0.0, -0.4, 0.2]], dtype=F64)
    g1 = _level_bwd(x1, y1, a1.to(DEV), zero.to(DEV), 1.0, out_f64=True)
    ref1, bound1 = K.bwd_reference(rx1, ry1, a1, zero, 1.0, fp32_out=False)
    g0 = _level_bwd(xd, yd, zero.to(DEV), b0.to(DEV), 1.0, g_coarse=g1)
    ref0, bound0 = K.bwd_reference(x, y, zero, b0, 1.0, g_coarse=ref1)
    carried = R64.level_closed_form(x, y, zero, zero, 1.0, bound1)[0]        # what level 1 was granted, at a quarter
    ratios = (K.worst(S1, rS1, bS1), K.worst(g1.cpu(), ref1, bound1), K.worst(g0.cpu(), ref0, bound0 + carried))
    print("[msssim level] float64 level and pool adjoint: worst |err| / bound", ratios)
    assert max(ratios) <= 1.0
    assert bool((g0[0, 2] == 0).all()) and bool((g0[0, 1, 26] == 0).all()) and bool((g0[0, 1, :, 46] == 0).all())


def test_c_abi_refusals_leave_the_outputs_untouched():
    N, Hh, Ww = 2, 12, 13
    x, y = (v.to(DEV) for v in K.inputs("noise", N, Hh, Ww))
    x0, y0 = x.clone(), y.clone()
    ntiles = H.value("adh_msssim_num_tiles", Hh, Ww)
    partial = torch.full((N * 3 * ntiles * 2,), float("nan"), device=DEV, dtype=F64)
    S, CS = (torch.full((N * 3,), float("nan"), device=DEV, dtype=F64) for _ in range(2))
    qx, qy = (torch.full((N * 3 * 36,), float("nan"), device=DEV, dtype=F64) for _ in range(2))
    ca = cb = torch.ones(N * 3, device=DEV, dtype=F64)
    g = torch.full((x.numel(),), float("nan"), device=DEV)

    def rejected(match, name, *args):
        with pytest.raises(RuntimeError, match=match):
            H.call(name, *args)
        torch.cuda.synchronize()
    P = lambda t: t.data_ptr()
    fwd = [P(x), P(y), 0, N, Hh, Ww, 1.0, P(partial), ntiles, P(S), P(CS), P(qx), P(qy)]
    for k in (0, 1, 7, 9, 10, 12):                       # a null pointer; only one of the pool pair
        rejected("ADH_E_ARG", "adh_msssim_level_fwd", *[None if i == k else v for i, v in enumerate(fwd)])
    for k, v in ((3, 0), (3, 65536), (2, 2), (8, ntiles + 1), (6, 0.0), (12, P(qx)), (11, P(x))):
        rejected("ADH_E_ARG", "adh_msssim_level_fwd", *[v if i == k else w for i, w in enumerate(fwd)])
    bwd = [P(x), P(y), 0, N, Hh, Ww, 1.0, P(ca), P(cb), None, P(g), 0]
    for k in (0, 1, 7, 8, 10):
        rejected("ADH_E_ARG", "adh_msssim_level_bwd", *[None if i == k else v for i, v in enumerate(bwd)])
    # the gradient may not be (or overlap) an image it is computed from
    for k, v in ((3, 0), (3, 65536), (11, 2), (10, P(x)), (10, P(y)), (10, P(x) + 4 * Ww)):
        rejected("ADH_E_ARG", "adh_msssim_level_bwd", *[v if i == k else w for i, w in enumerate(bwd)])
    for hh, ww in ((10, Ww), (Hh, 10)):
        rejected("UNSUPPORTED", "adh_msssim_level_fwd", *[{4: hh, 5: ww}.get(i, v) for i, v in enumerate(fwd)])
        rejected("UNSUPPORTED", "adh_msssim_level_bwd", *[{4: hh, 5: ww}.get(i, v) for i, v in enumerate(bwd)])
        with pytest.raises(RuntimeError, match="UNSUPPORTED"):
            H.value("adh_msssim_num_tiles", hh, ww)
    for t in (partial, S, CS, qx, qy, g):
        assert bool(torch.isnan(t).all())
    assert _same_bits(x, x0) and _same_bits(y, y0)


# ------------------------------------------------------------------------------------------------ the pyramid, public API
_PYRAMID_REF = {}


def _pyramid_ref(Hh, Ww, weights, kind="noise"):
    """the float64 reference of one pyramid case, computed once and shared"""
    key = (Hh, Ww, weights, kind)
    if key not in _PYRAMID_REF:
        p, t = K.inputs(kind, 2, Hh, Ww)
        g_up = torch.tensor([0.7, -1.3])
        w = R64.MS_SSIM_WEIGHTS if weights is None else weights
        val, grad = R64.ms_ssim_autograd(p, t, g_up.double(), 1.0, w)
        vbound, gbound, V = R64.pyramid_bounds(p, t, g_up.double(), 1.0, w)
        _PYRAMID_REF[key] = (p, t, g_up, val, grad, vbound, gbound, V)
    return _PYRAMID_REF[key]


PYRAMIDS = [(176, 176, None), (177, 191, None), (176, 353, None), (44, 47, W3), (45, 50, W3)]


@pytest.mark.parametrize("Hh,Ww,weights", PYRAMIDS)
def test_ms_ssim_value_and_gradient_vs_float64(Hh, Ww, weights):
    p, t, g_up, val, grad, vbound, gbound, V = _pyramid_ref(Hh, Ww, weights)
    assert bool((V > 0.9).all())                                             # no factor near the clamp
    kw = {} if weights is None else {"weights": weights}
    pd, td = p.to(DEV).requires_grad_(True), t.to(DEV).requires_grad_(True)

    def run():
        pd.grad = None
        out = L.ms_ssim_per_image(pd, td, **kw)
        (out * g_up.to(DEV)).sum().backward()
        return out.detach(), pd.grad
    out, g = _twice(run)                                                     # two runs are bit-equal
    assert out.shape == (2,) and out.dtype == torch.float32 and td.grad is None
    assert _same_bits(out, M.ms_ssim_batch(pd.detach(), td.detach(), **kw))
    rv = K.worst(out.cpu(), val, EPS * val.abs() + vbound)
    rg = K.worst(g.cpu(), grad, EPS * grad.abs() + gbound)
    sg = M.ssim_gaussian_batch(pd.detach(), td.detach())
    rs_ref = R64.ssim_gaussian(p, t)
    rs = K.worst(sg.cpu(), rs_ref, EPS * rs_ref.abs() + R64.FWD_UNITS * K.U53 * R64.level_terms(p, t)[0].mean(1))
    print(f"[ms-ssim] 2x3x{Hh}x{Ww} L={len(weights or R64.MS_SSIM_WEIGHTS)}: worst |err| / bound value {rv:.3g} gradient {rg:.3g} "
          f"ssim_gaussian {rs:.3g}; ms_ssim {out.tolist()}")
    assert max(rv, rg, rs) <= 1.0
    # image i alone is image i of the batch, bit for bit: value and gradient
    for i in (0, 1):
        pi = p[i:i + 1].to(DEV).requires_grad_(True)
        oi = L.ms_ssim_per_image(pi, t[i:i + 1].to(DEV), **kw)
        (oi * g_up[i:i + 1].to(DEV)).sum().backward()
        assert _same_bits(oi.detach(), out[i:i + 1]) and _same_bits(pi.grad, g[i:i + 1])
        assert _same_bits(M.ssim_gaussian_batch(pi.detach(), t[i:i + 1].to(DEV)), sg[i:i + 1])


def test_identical_images_score_exactly_one_and_negated_ones_exactly_zero():
    t = K.inputs("negated", 2, 176, 176)[1].to(DEV)
    assert M.ssim_gaussian_batch(t, t).tolist() == [1.0, 1.0] and M.ms_ssim_batch(t, t).tolist() == [1.0, 1.0]
    p = (1.0 - t).requires_grad_(True)
    out = L.ms_ssim_per_image(p, t)
    out.sum().backward()
    assert out.tolist() == [0.0, 0.0]
    assert bool((p.grad == 0).all()) and not bool(torch.signbit(p.grad).any()), "a clamped plane: exact +0.0 expected"
    assert float(L.MSSSIMLoss()(p.detach(), t)) == 1.0 and float(L.MSSSIMLoss()(t, t)) == 0.0
    # one plane clamped, the others not: that plane's gradient alone is zero
    q = t.clone()
    q[:, 0] = 1.0 - t[:, 0]
    q.requires_grad_(True)
    L.ms_ssim_per_image(q, t).sum().backward()
    assert bool((q.grad[:, 0] == 0).all())
    assert float(q.grad[:, 1:].abs().max()) < 1e-10                                  # the others are identical: at their maximum


def test_data_range_255_scores_the_scaled_images_alike():
    p, t, _, val, _, vbound, _, _ = _pyramid_ref(44, 47, W3)
    a = M.ms_ssim_batch((p * 255).to(DEV), (t * 255).to(DEV), data_range=255.0, weights=W3)
    ref = R64.ms_ssim(p * 255, t * 255, 255.0, W3)
    assert K.worst(a.cpu(), ref, EPS * ref.abs() + 2 * vbound) <= 1.0


def test_python_refusals():
    p, t = (v.to(DEV) for v in K.inputs("noise", 2, 175, 300))
    with pytest.raises(ValueError, match="at least 176x176"):
        M.ms_ssim_batch(p, t)
    with pytest.raises(ValueError, match="at least 176x176"):
        L.ms_ssim_per_image(p, t)
    assert M.ms_ssim_batch(p, t, weights=(0.5, 0.5)).shape == (2,)
    with pytest.raises(ValueError, match="at least 44x44"):
        M.ms_ssim_batch(p[:, :, :43], t[:, :, :43], weights=W3)
    with pytest.raises(ValueError, match="at least 11x11"):
        M.ssim_gaussian_batch(p[:, :, :, :10], t[:, :, :, :10])
    with pytest.raises(ValueError, match="1 to 5 positive"):
        M.ms_ssim_batch(p, t, weights=(0.5, 0.0))
    with pytest.raises(ValueError, match="data_range"):
        M.ssim_gaussian_batch(p, t, data_range=0.0)
    for fn in (M.ssim_gaussian_batch, M.ms_ssim_batch, L.ms_ssim_per_image):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            fn(p.cpu(), t.cpu())
        with pytest.raises(RuntimeError, match="expected two"):
            fn(p, t[:1])
        with pytest.raises(RuntimeError, match="expected two"):
            fn(p[:, :2], t[:, :2])
        with pytest.raises(RuntimeError, match="float32"):
            fn(p.double(), t.double())


def test_metric_switches_add_the_two_keys_only_when_set():
    p, t = (v.to(DEV) for v in K.inputs("noise", 2, 176, 180))
    assert set(M.calculate_image_metrics(p, t)) == {"psnr", "ssim"}
    m = M.calculate_image_metrics(p, t, ms_ssim=True)
    assert list(m) == ["psnr", "ssim", "ssim_gaussian", "ms_ssim"]
    assert _same_bits(m["ms_ssim"], M.ms_ssim_batch(p, t)) and _same_bits(m["ssim_gaussian"], M.ssim_gaussian_batch(p, t))
    q = M.ImageQualityMetrics(device=DEV, use_lpips=False, use_ms_ssim=True)
    q.add_batch(p, t, ["low_intensity", "high_intensity"])
    avg = q.compute_averages()
    assert set(avg["low_intensity"]) == {"psnr", "ssim", "ssim_gaussian", "ms_ssim", "samples"}
    assert avg["high_intensity"]["ms_ssim"] == float(m["ms_ssim"][1].double())
    plain = M.ImageQualityMetrics(device=DEV, use_lpips=False)
    plain.add_batch(p, t)
    assert set(plain.compute_averages()["all"]) == {"psnr", "ssim", "samples"}


def test_without_grad_nothing_is_kept_and_no_backward_is_launched(monkeypatch):
    calls = []
    real = H.call
    monkeypatch.setattr(H, "call", lambda name, *a, **k: (calls.append(name), real(name, *a, **k))[1])
    p, t = (v.to(DEV) for v in K.inputs("noise", 1, 44, 44))
    out = L.ms_ssim_per_image(p, t.requires_grad_(True), weights=W3)
    assert not out.requires_grad
    with torch.no_grad():
        assert not L.MSSSIMLoss(weights=W3)(p.clone().requires_grad_(True), t).requires_grad
    assert calls.count("adh_msssim_level_fwd") == 6 and "adh_msssim_level_bwd" not in calls
    pg = p.clone().requires_grad_(True)
    L.MSSSIMLoss(weights=W3)(pg, t).backward()
    assert calls.count("adh_msssim_level_bwd") == 3 and pg.grad is not None


# ------------------------------------------------------------------------------------------------ loss plumbing
def test_dehazing_loss_with_the_ms_ssim_term():
    p, t, _, val, _, vbound, _, _ = _pyramid_ref(44, 47, W3)
    N = 2
    pd, td = p.to(DEV).requires_grad_(True), t.to(DEV)
    crit = L.DehazingLoss(content=False, perceptual=False, lambda_msssim=0.2, msssim_weights=W3).to(DEV)
    total, comps = crit(pd, td)
    assert list(comps) == ["l1", "content", "perceptual", "ms_ssim", "total"]
    l1 = float((p.double() - t.double()).abs().mean())
    mean = float(val.mean())
    vb = float((EPS * val.abs() + vbound).mean())
    # fp32: the batch mean (an addition and a division), 1 - mean; then the product with 0.2 and one addition to l1; the L1
    # kernel's own reduction is granted 8 EPS
    assert abs(float(comps["ms_ssim"].detach().double()) - (1.0 - mean)) <= 3 * EPS * (1.0 + mean) + vb
    assert abs(float(total.detach().double()) - (l1 + 0.2 * (1.0 - mean))) <= 8 * EPS * l1 + 6 * EPS * (1.0 + mean) + 0.2 * vb
    total.backward()
    _, gs = R64.ms_ssim_autograd(p, t, torch.full((N,), -0.2 / N, dtype=F64), 1.0, W3)
    gbound = R64.pyramid_bounds(p, t, torch.full((N,), -0.2 / N, dtype=F64), 1.0, W3)[1]
    gl1 = torch.sign(p.double() - t.double()) / p.numel()
    ref = gl1 + gs
    # L1 backward: 1 / numel rounded to fp32 and one product; the upstream -0.2 / N reaches the kernel as fp32 (two roundings
    # on the way: 0.2 and the division); autograd's accumulation of the two terms: one fp32 addition
    bound = EPS * (2 * gl1.abs() + 4 * gs.abs() + ref.abs()) + gbound
    r = K.worst(pd.grad.cpu(), ref, bound)
    print(f"[ms-ssim] DehazingLoss(lambda_msssim=0.2) gradient: worst |err| / bound {r:.3g}")
    assert r <= 1.0
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        plain = L.DehazingLoss(content=False, perceptual=False).to(DEV)
        zero = L.DehazingLoss(content=False, perceptual=False, lambda_msssim=0, msssim_weights=W3).to(DEV)
    ta, ca = plain(pd.detach(), td)
    tz, cz = zero(pd.detach(), td)
    assert _same_bits(ta, tz) and list(ca) == list(cz) == ["l1", "content", "perceptual", "total"]


def _drive(loss_cfg):
    """one joint_train_step and one dehazing_train_step at 48 x 48 under the launch recorder"""
    from adam_dehaze_amd.optim import Adam
    from tests._joint_step_trace import StepTrace, train_mode
    from tests.test_gpu_train import _cfg
    cfg = _cfg()
    if loss_cfg is not None:
        cfg["loss"] = loss_cfg
    torch.manual_seed(2)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        system = T.build_joint_system(cfg)
        crit = L.get_dehazing_loss(cfg).to(DEV)
    train_mode(system)
    batch = next(T.synthetic_loader(4, (48, 48), 1, seed=5, device=DEV))
    m = A.LightweightDehazeModel(base_channels=8, n_blocks=1).to(DEV).train()
    opt = Adam(m.parameters(), lr=1e-3, weight_decay=1e-4)
    params = {"joint": [q for g in system["optimizer"].param_groups for q in g["params"]], "branch": list(m.parameters())}
    before = {k: [q.detach().clone() for q in v] for k, v in params.items()}
    with pytest.MonkeyPatch.context() as mp:
        trace = StepTrace(H.call)
        mp.setattr(H, "call", trace.call)
        stats = [T.joint_train_step(system, batch), T.dehazing_train_step(m, crit, opt, batch, None, torch.device(DEV))]
    torch.cuda.synchronize()
    moved = {k: [not torch.equal(b, q.detach()) for b, q in zip(before[k], v)] for k, v in params.items()}
    after = {k: [q.detach().clone() for q in v] for k, v in params.items()}
    return stats, [r[0] for r in trace.records], moved, after


def test_training_steps_carry_the_ms_ssim_term_and_every_parameter_moves():
    stats, names, moved, _ = _drive({"lambda_msssim": 0.2, "msssim_weights": list(W3)})
    assert set(stats[0]) == {"loss", "dehazing", "classification", "ms_ssim"} and set(stats[1]) == {"loss", "l1", "ms_ssim"}
    for st in stats:
        vals = {k: float(v) for k, v in st.items()}
        assert all(math.isfinite(v) for v in vals.values()), vals
        assert 0.0 <= vals["ms_ssim"] <= 1.0
    assert names.count("adh_msssim_level_fwd") == 6 and names.count("adh_msssim_level_bwd") == 6
    for k, flags in moved.items():
        assert flags and all(flags), (k, [i for i, f in enumerate(flags) if not f])


def test_training_steps_with_lambda_zero_are_the_steps_without_the_key():
    s0, n0, _, a0 = _drive({"lambda_msssim": 0.0, "msssim_weights": list(W3)})
    s1, n1, _, a1 = _drive(None)
    assert n0 == n1 and not [n for n in n0 if n.startswith("adh_msssim")]
    assert set(s0[0]) == {"loss", "dehazing", "classification"} and set(s0[1]) == {"loss", "l1"}
    for u, v in zip(s0, s1):
        assert all(_same_bits(u[k], v[k]) for k in u)
    for k in a0:
        assert all(_same_bits(u, v) for u, v in zip(a0[k], a1[k]))


# ------------------------------------------------------------------------------------------------ demo
BASE_KEYS = {"file", "height", "width", "routing", "weights", "intensity"}


@pytest.fixture(scope="module")
def demo(tmp_path_factory):
    """two 176 x 192 pairs and one 40 x 56 pair through run_demo, with and without the switch"""
    Image = pytest.importorskip("PIL.Image")
    from tests.test_gpu_demo_scores import _cfg
    hazy, clear = tmp_path_factory.mktemp("hazy"), tmp_path_factory.mktemp("clear")
    g = np.random.default_rng(5)
    for name, (h, w) in (("a.png", (176, 192)), ("b.png", (176, 192)), ("s.png", (40, 56))):
        gt = g.integers(0, 256, (h, w, 3), dtype=np.uint8)
        hz = np.clip(gt.astype(np.int32) // 2 + 100 + g.integers(-8, 9, gt.shape), 0, 255).astype(np.uint8)
        Image.fromarray(gt).save(clear / name)
        Image.fromarray(hz).save(hazy / name)
    torch.manual_seed(11)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        system = T._joint_system_for_evaluation(_cfg())[0]
    runs = {}
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(T, "_joint_system_for_evaluation", lambda config: (system, None))
        for key, kw in (("on", {"ms_ssim": True}), ("off", {})):
            out = tmp_path_factory.mktemp("demo_" + key)
            runs[key] = (out, T.run_demo(_cfg(), str(hazy), str(out), False, target=str(clear), **kw))
    return hazy, clear, runs


def test_demo_records_and_means(demo):
    hazy, clear, runs = demo
    out, results = runs["on"]
    planes = lambda path: IO.u8_to_image(IO.load_image(str(path)).to(DEV))
    for r in results:
        name = os.path.basename(r["file"])
        assert set(r) == BASE_KEYS | {"target", "scored"} | set(IO.SCORE_KEYS) | set(IO.MS_SSIM_SCORE_KEYS)
        tgt = planes(clear / name)
        for prefix, img in (("", planes(out / name)), ("hazy_", planes(hazy / name))):
            assert r[prefix + "ssim_gaussian"] == float(M.ssim_gaussian_batch(img, tgt).double()[0])
            if name == "s.png":
                assert r[prefix + "ms_ssim"] is None
            else:
                assert r[prefix + "ms_ssim"] == float(M.ms_ssim_batch(img, tgt).double()[0])
    assert json.load(open(out / "demo_results.json")) == results
    scores = json.load(open(out / "demo_scores.json"))
    for side, prefix in (("dehazed", ""), ("hazy", "hazy_")):
        al = scores[side]["all"]
        assert set(al) == {"psnr", "ssim", "ciede2000", "samples", "ssim_gaussian", "ms_ssim", "ms_ssim_too_small"}
        assert al["samples"] == 3 and al["ms_ssim_too_small"] == 1
        big = [r for r in results if r["height"] == 176]
        assert abs(al["ms_ssim"] - sum(r[prefix + "ms_ssim"] for r in big) / 2) <= 1e-12
        assert abs(al["ssim_gaussian"] - sum(r[prefix + "ssim_gaussian"] for r in results) / 3) <= 1e-12
    assert 0.0 < scores["hazy"]["all"]["ms_ssim"] < 1.0


def test_demo_without_the_switch_keeps_todays_keys(demo):
    _, _, runs = demo
    out, results = runs["off"]
    assert all(set(r) == BASE_KEYS | {"target", "scored"} | set(IO.SCORE_KEYS) for r in results)
    scores = json.load(open(out / "demo_scores.json"))
    assert all(set(e) == {"psnr", "ssim", "ciede2000", "samples"} for side in scores.values() for e in side.values())
    on = {os.path.basename(r["file"]): r for r in runs["on"][1]}
    for r in results:                                        # and today's numbers
        assert all(r[k] == on[os.path.basename(r["file"])][k] for k in IO.SCORE_KEYS)
