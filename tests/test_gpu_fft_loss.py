"""csrc/fft_loss.hip on the GPU against float64 (tests/_fft_ref64.py), then the layers above it: frequency_l1's autograd
function, FrequencyLoss, DehazingLoss(lambda_fft) and the training steps.

Tolerance.  Not chosen: measured.  torch's own float32 fft2 + autograd against the float64 reference on the CPU, at every
shape of the gate with the recorded seeds (python -m tests._fft_ref64), loss relative error / gradient max-abs error over the
gradient's RMS:

    (N, H, W)        backward             ortho
    (1, 8, 8)        6.41e-08  1.72e-07   6.41e-08  1.72e-07
    (2, 8, 32)       5.87e-08  2.42e-07   5.87e-08  2.42e-07
    (3, 64, 16)      7.77e-08  4.03e-07   7.77e-08  4.03e-07
    (2, 32, 64)      1.06e-07  3.64e-07   6.43e-08  4.19e-07
    (5, 16, 16)      1.62e-08  4.84e-07   1.62e-08  4.65e-07
    (1, 8, 4096)     3.08e-08  4.71e-07   1.51e-08  5.39e-07
    (1, 4096, 8)     2.37e-08  5.84e-07   4.00e-08  6.23e-07
    (1, 256, 256)    3.99e-08  5.67e-07   3.99e-08  5.67e-07

The gate is 8 x the largest per quantity (the factor allows for a different but equally valid butterfly order and twiddle
rounding): 8 x 1.06e-7 on the loss, 8 x 6.23e-7 of the gradient's RMS on every gradient element.  No bin is excluded; before
anything is compared the float64 spectrum must keep every component (but the four self-conjugate imaginary parts, exactly 0
by definition) at least 1e-5 x RMS(D) away from the kink of |.|, so that no fp32 rounding can flip a sign -- the seeds
recorded in tests/_fft_ref64.py were searched for that on the CPU."""
import math
import warnings

import pytest
import torch

import adam_dehaze_amd as A
from adam_dehaze_amd import _hip as H
from adam_dehaze_amd import loss as L
from tests import _fft_ref64 as F64
from tests._util import DEV, EPS, _assert_bound, _pad_untouched, _padded, _same_bits, _twice

pytestmark = pytest.mark.gpu

FFT_LOSS_RTOL = 8 * 1.06e-7         # |loss - ref| / ref
FFT_GRAD_TOL = 8 * 6.23e-7          # max |grad - ref| / RMS(ref)

SHAPES = list(F64.SEEDS)            # (1,8,8) (2,8,32) (3,64,16) (2,32,64) (5,16,16) (1,8,4096) (1,4096,8) (1,256,256)
_REF = {}


def _reference(shape, norm):
    """(pred, target, loss, grad) of a gate shape: float64 on the CPU, computed once, kink guard included"""
    key = (shape, norm)
    if key not in _REF:
        p, t = F64.inputs(*shape)
        assert F64.min_kink_distance(p, t) >= F64.KINK_MIN, "the reference itself sits on the kink: pick another seed"
        _REF[key] = (p, t) + F64.loss_and_grad(p, t, norm)
    return _REF[key]


def _launch(p, t, norm, want_grad=True):
    """adh_fft_l1 on device tensors, twice, every output NaN-filled inside a NaN guard band; (loss [1], grad or None)"""
    N, _, Hh, Ww = p.shape
    n = p.numel()
    nws = H.value("adh_fft_l1_workspace_bytes", N, Hh, Ww) // 4
    nparts = H.value("adh_fft_l1_num_partials", N, Hh, Ww)
    assert nws == n and nparts >= 3 * N                 # the half spectrum takes the bytes of one image

    def run():
        wws, ws = _padded(nws)
        wpa, part = _padded(nparts, dtype=torch.float64)
        wlo, loss = _padded(1)
        wgr, grad = _padded(n) if want_grad else (None, None)
        H.call("adh_fft_l1", p.data_ptr(), t.data_ptr(), N, Hh, Ww, int(norm == "ortho"), ws.data_ptr(), part.data_ptr(),
               loss.data_ptr(), H.ptr(grad))
        torch.cuda.synchronize()
        assert _pad_untouched(wws, nws) and _pad_untouched(wpa, nparts) and _pad_untouched(wlo, 1)
        assert not want_grad or _pad_untouched(wgr, n)
        return (loss, grad) if want_grad else (loss,)
    out = _twice(run)
    return out[0], (out[1].view(N, 3, Hh, Ww) if want_grad else None)


def _compare(what, loss, grad, ref_loss, ref_grad):
    rel = abs(float(loss) - float(ref_loss)) / float(ref_loss)
    rms = math.sqrt(float((ref_grad * ref_grad).mean()))
    print(f"[fft] {what}: loss rel err {rel:.2e} (gate {FFT_LOSS_RTOL:.2e})")
    _assert_bound(grad.cpu(), ref_grad, FFT_GRAD_TOL * rms, f"{what} grad")
    assert rel <= FFT_LOSS_RTOL, (what, rel)


# ------------------------------------------------------------------------------------------------ the kernels
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_fft_l1_kernel_vs_float64(shape):
    p, t, ref_loss, ref_grad = _reference(shape, "backward")
    loss, grad = _launch(p.to(DEV), t.to(DEV), "backward")
    _compare(f"{shape} backward", loss, grad, ref_loss, ref_grad)


@pytest.mark.parametrize("shape", [(3, 64, 16), (2, 32, 64)], ids=lambda s: "x".join(map(str, s)))
def test_fft_l1_kernel_ortho_vs_float64(shape):
    p, t, ref_loss, ref_grad = _reference(shape, "ortho")
    loss, grad = _launch(p.to(DEV), t.to(DEV), "ortho")
    _compare(f"{shape} ortho", loss, grad, ref_loss, ref_grad)


def test_fft_l1_value_only_launch_matches_and_writes_no_gradient():
    shape = (2, 32, 64)
    p, t, ref_loss, _ = _reference(shape, "backward")
    pd, td = p.to(DEV), t.to(DEV)
    loss, grad = _launch(pd, td, "backward")
    only, none = _launch(pd, td, "backward", want_grad=False)
    assert none is None and _same_bits(only, loss)


def test_fft_l1_identical_images_are_exactly_zero():
    p, _ = F64.inputs(2, 32, 64)
    pd = p.to(DEV)
    for other in (pd, pd.clone()):
        loss, grad = _launch(pd, other, "backward")
        assert float(loss) == 0.0 and bool((grad == 0).all())


@pytest.mark.parametrize("norm", F64.NORMS)
def test_fft_l1_known_answer_single_cosine(norm):
    """d = cos(2 pi (u0 y / H + v0 x / W)) with phases that are multiples of a quarter turn (exact in fp32): L = 0.5, or
    0.5 / sqrt(H W) under "ortho", within the measured bound"""
    for (N, Hh, Ww, u0, v0) in [(1, 8, 8, 2, 2), (2, 16, 32, 4, 8)]:
        p, t = F64.cosine_pair(N, Hh, Ww, u0, v0, torch.float32)
        loss, _ = _launch(p.to(DEV), t.to(DEV), norm)
        expect = 0.5 / math.sqrt(Hh * Ww) if norm == "ortho" else 0.5
        assert abs(float(loss) - expect) <= FFT_LOSS_RTOL * expect, (Hh, Ww, float(loss))


def test_fft_l1_rejections_leave_the_outputs_untouched():
    N, Hh, Ww = 1, 8, 8
    p, t = (x.to(DEV) for x in F64.inputs(N, Hh, Ww))
    whole, out = _padded(1024)
    ws, part, loss, grad = out[:256], out[256:512].view(torch.float64), out[512:513], out[768:768 + p.numel()]

    def rejected(match, *args):
        with pytest.raises(RuntimeError, match=match):
            H.call("adh_fft_l1", *args)
        torch.cuda.synchronize()

    ok = (p.data_ptr(), t.data_ptr(), N, Hh, Ww, 0, ws.data_ptr(), part.data_ptr(), loss.data_ptr(), grad.data_ptr())
    for hh, ww in ((30, 46), (4, 8), (8, 4), (8192, 8), (8, 8192), (12, 8)):
        rejected("UNSUPPORTED", *ok[:3], hh, ww, *ok[5:])
        for q in ("adh_fft_l1_workspace_bytes", "adh_fft_l1_num_partials"):
            with pytest.raises(RuntimeError, match="UNSUPPORTED"):
                H.value(q, N, hh, ww)
    rejected("UNSUPPORTED", *ok[:2], 21846, *ok[3:])                   # 3 N > 65535
    for i in (0, 1, 6, 7, 8):
        rejected("ADH_E_ARG", *ok[:i], None, *ok[i + 1:])
    rejected("ADH_E_ARG", *ok[:2], 0, *ok[3:])
    rejected("ADH_E_ARG", *ok[:5], 2, *ok[6:])
    rejected("ADH_E_ARG", *ok[:6], ws.data_ptr() + 4, *ok[7:])
    assert bool(torch.isnan(whole).all())


# ------------------------------------------------------------------------------------------------ autograd
def test_frequency_l1_autograd_and_noncontiguous_pred():
    shape = (2, 32, 64)
    p, t, ref_loss, ref_grad = _reference(shape, "backward")
    wide = torch.zeros(2, 3, 32, 128, device=DEV)
    wide[..., ::2] = p.to(DEV)
    wide.requires_grad_(True)
    pd, td = wide[..., ::2], t.to(DEV).requires_grad_(True)
    assert not pd.is_contiguous()
    out = L.frequency_l1(pd, td)
    assert out.shape == () and out.requires_grad
    (out * 3.0).backward()
    assert td.grad is None
    assert bool((wide.grad[..., 1::2] == 0).all())
    _compare("frequency_l1 non-contiguous, upstream 3", out.detach(), wide.grad[..., ::2] / 3.0, ref_loss, ref_grad)
    again = L.FrequencyLoss()(p.to(DEV).requires_grad_(True), t.to(DEV))
    assert _same_bits(again.detach(), out.detach())


def test_frequency_l1_without_grad_passes_no_gradient_buffer(monkeypatch):
    calls = []
    real = H.call

    def spy(name, *a, **k):
        calls.append((name, a))
        return real(name, *a, **k)
    monkeypatch.setattr(H, "call", spy)
    shape = (2, 32, 64)
    p, t, ref_loss, _ = _reference(shape, "backward")
    pd, td = p.to(DEV), t.to(DEV)
    with torch.no_grad():
        v0 = L.frequency_l1(pd.clone().requires_grad_(True), td)
    v1 = L.frequency_l1(pd, td)                                      # nothing requires a gradient
    assert not v0.requires_grad and not v1.requires_grad and _same_bits(v0, v1)
    assert abs(float(v0) - float(ref_loss)) <= FFT_LOSS_RTOL * float(ref_loss)
    assert [c[0] for c in calls] == ["adh_fft_l1", "adh_fft_l1"] and all(c[1][-1] is None for c in calls)
    v2 = L.frequency_l1(pd.clone().requires_grad_(True), td)
    assert calls[-1][1][-1] is not None and _same_bits(v2.detach(), v0)
    pg = pd.clone().requires_grad_(True)
    n = len(calls)
    L.frequency_l1(pg, pg).backward()                                # pred is target
    assert len(calls) == n + 1 and bool((pg.grad == 0).all())        # the backward launches nothing


# ------------------------------------------------------------------------------------------------ DehazingLoss
def test_dehazing_loss_with_fft_term():
    shape = (2, 32, 64)
    p, t, ref_loss, ref_grad = _reference(shape, "backward")
    pd, td = p.to(DEV).requires_grad_(True), t.to(DEV)
    crit = L.DehazingLoss(content=False, perceptual=False, lambda_fft=0.1).to(DEV)
    total, comps = crit(pd, td)
    assert list(comps) == ["l1", "content", "perceptual", "fft", "total"]
    l1, fft = float(comps["l1"].detach().double()), float(comps["fft"].detach().double())
    assert abs(fft - float(ref_loss)) <= FFT_LOSS_RTOL * float(ref_loss)
    # fp32: the product with 0.1 (rounded itself) and one addition
    assert abs(float(total.detach().double()) - (l1 + 0.1 * fft)) <= 4 * EPS * (abs(l1) + 0.1 * abs(fft))
    total.backward()
    gl1 = torch.sign(p.double() - t.double()) / p.numel()
    ref = gl1 + 0.1 * ref_grad
    # L1 backward: 1 / numel rounded to fp32 and one product; the frequency term: its own bound, times fp32(0.1); autograd's sum
    rms = math.sqrt(float((ref_grad * ref_grad).mean()))
    bound = EPS * (2 * gl1.abs() + 0.2 * ref_grad.abs() + ref.abs()) + 0.1 * FFT_GRAD_TOL * rms
    _assert_bound(pd.grad.cpu(), ref, bound, "DehazingLoss(lambda_fft=0.1) grad")

    both = L.DehazingLoss(content=False, perceptual=False, lambda_ssim=0.5, lambda_fft=0.1, fft_norm="ortho").to(DEV)
    tb, cb = both(pd.detach(), td)
    assert list(cb) == ["l1", "content", "perceptual", "ssim", "fft", "total"]
    assert abs(float(cb["fft"]) * math.sqrt(32 * 64) - fft) <= 4 * EPS * fft
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        plain = L.DehazingLoss(content=False, perceptual=False).to(DEV)
        zero = L.DehazingLoss(content=False, perceptual=False, lambda_fft=0).to(DEV)
    ta, ca = plain(pd.detach(), td)
    tz, cz = zero(pd.detach(), td)
    assert _same_bits(ta, tz) and list(ca) == list(cz) == ["l1", "content", "perceptual", "total"]


# ------------------------------------------------------------------------------------------------ the drivers
def _drive(with_fft):
    """two joint_train_steps and one dehazing_train_step at 32 x 64 under the launch recorder; (stats..., entry points)"""
    from adam_dehaze_amd import train as T
    from adam_dehaze_amd.optim import Adam
    from tests._joint_step_trace import StepTrace, train_mode
    from tests.test_gpu_train import _cfg
    cfg = _cfg()
    if with_fft:
        cfg["loss"] = {"lambda_fft": 0.1}
    torch.manual_seed(2)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        system = T.build_joint_system(cfg)
        crit = L.get_dehazing_loss(cfg).to(DEV)
    train_mode(system)
    batch = next(T.synthetic_loader(4, (32, 64), 1, seed=5, device=DEV))
    m = A.LightweightDehazeModel(base_channels=8, n_blocks=1).to(DEV).train()
    opt = Adam(m.parameters(), lr=1e-3, weight_decay=1e-4)
    queries = []
    with pytest.MonkeyPatch.context() as mp:
        trace = StepTrace(H.call)
        real_value = H.value
        mp.setattr(H, "call", trace.call)
        mp.setattr(H, "value", lambda name, *a: (queries.append(name), real_value(name, *a))[1])
        stats = [T.joint_train_step(system, batch), T.joint_train_step(system, batch),
                 T.dehazing_train_step(m, crit, opt, batch, None, torch.device(DEV))]
    torch.cuda.synchronize()
    return stats, [r[0] for r in trace.records] + queries


def test_training_steps_carry_the_fft_term():
    stats, names = _drive(True)
    for st in stats:
        assert "fft" in st and "ssim" not in st
        vals = {k: float(v) for k, v in st.items()}
        assert all(math.isfinite(v) for v in vals.values()), vals
        assert vals["fft"] > 0
    assert names.count("adh_fft_l1") == 3


def test_training_steps_without_the_key_launch_nothing_for_it():
    stats, names = _drive(False)
    assert set(stats[0]) == set(stats[1]) == {"loss", "dehazing", "classification"} and set(stats[2]) == {"loss", "l1"}
    assert not [n for n in names if n.startswith("adh_fft_")]
    assert all(math.isfinite(float(v)) for st in stats for v in st.values())
