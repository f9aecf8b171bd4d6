"""CPU checks of the SSIM loss term: the float64 reference the GPU tests lean on (tests/_ssim_ref64.py) against
_ref64.ssim_gray, a central difference and the closed form of DESIGN 4.20, and the host-side plumbing of `lambda_ssim`."""
import warnings

import pytest
import torch

from tests import _ref64 as R64
from tests import _ssim_ref64 as S64

U53 = 2.0 ** -53


def _pair(N, Hh, Ww, kind, seed):
    gen = torch.Generator().manual_seed(seed)
    t = torch.rand(N, 3, Hh, Ww, generator=gen)
    if kind == "random":
        p = torch.rand(N, 3, Hh, Ww, generator=gen)
    elif kind == "close":
        p = t + 0.002 * torch.randn(N, 3, Hh, Ww, generator=gen)
    elif kind == "equal":
        p = t.clone()
    else:
        p = torch.full_like(t, 0.4)
    return p, t


@pytest.mark.parametrize("kind", ["random", "close", "equal", "constant"])
@pytest.mark.parametrize("Hh,Ww", [(7, 7), (8, 9), (13, 13), (39, 7), (45, 131)])
def test_reference_value_is_ref64_ssim_gray(Hh, Ww, kind):
    p, t = _pair(2, Hh, Ww, kind, Hh * Ww)
    (val, grad), terms = S64.ssim_and_grad(p, t, [0.7, -1.3])
    ref = R64.ssim_gray(p, t)
    # the same expressions on the same fp32 grayscale: float64 rounding only (the statistics cancel against C2 = 9e-4)
    assert float((val - ref).abs().max()) <= 1e-12
    assert grad.shape == p.shape and terms.shape == (2, 1, Hh, Ww)
    assert bool((terms > 0).all())


def test_reference_gradient_is_the_central_difference():
    """9 x 10, every element of one image: (f(p + h e) - f(p - h e)) / 2h in float64, h = 1e-5 (truncation ~h^2 f''', rounding
    ~1e-16 / h).  The difference quotient sees the float64 grayscale, the reference the fp32 one: the inputs are float32
    values whose channel sums are exact in fp32 up to the division by 3, which moves the gradient by ~1e-7 relative."""
    gen = torch.Generator().manual_seed(5)
    t = torch.rand(1, 3, 9, 10, generator=gen)
    p = (t + 0.1 * torch.randn(1, 3, 9, 10, generator=gen)).clamp(0, 1)
    (val, grad), _ = S64.ssim_and_grad(p, t, [1.0])
    p64, h = p.double(), 1e-5
    fd = torch.zeros_like(p64)
    flat = fd.view(-1)
    for i in range(p64.numel()):
        e = torch.zeros_like(p64).view(-1)
        e[i] = h
        e = e.view_as(p64)
        up = S64.ssim_of_images(p64 + e, t.double())
        dn = S64.ssim_of_images(p64 - e, t.double())
        flat[i] = float(up - dn) / (2 * h)
    scale = float(grad.abs().max())
    assert scale > 1e-4
    assert float((fd - grad).abs().max()) <= 2e-6 * scale


@pytest.mark.parametrize("kind", ["random", "close", "equal", "constant"])
@pytest.mark.parametrize("Hh,Ww", [(7, 7), (8, 8), (13, 13), (7, 39), (39, 7), (38, 38), (39, 39), (45, 131)])
def test_reference_gradient_is_the_closed_form(Hh, Ww, kind):
    p, t = _pair(2, Hh, Ww, kind, Hh + 7 * Ww)
    g = [0.7, -1.3]
    (val, grad), terms = S64.ssim_and_grad(p, t, g)
    cf, terms2 = S64.closed_form(p, t, g)
    assert torch.equal(terms, terms2)
    # two float64 evaluations of one function: apart by a few thousand roundings of the terms at worst (the window
    # variances cancel against C2; tests/test_gpu_ssim_loss.py counts them)
    assert float(((cf - grad).abs() / terms).max()) <= 2.0 ** 21 * U53


def test_lambda_ssim_is_stored_and_off_by_default():
    from adam_dehaze_amd.loss import DehazingLoss, SSIMLoss
    d = DehazingLoss(content=False, perceptual=False)
    assert d.lambda_ssim == 0.0 and d.ssim_loss is None
    d = DehazingLoss(content=False, perceptual=False, lambda_ssim=0)
    assert d.lambda_ssim == 0.0 and d.ssim_loss is None
    d = DehazingLoss(content=False, perceptual=False, lambda_ssim=0.3)
    assert d.lambda_ssim == 0.3 and isinstance(d.ssim_loss, SSIMLoss)
    assert not list(d.parameters()) and not d.state_dict()
    with pytest.raises(ValueError):
        DehazingLoss(content=False, perceptual=False, lambda_ssim=-0.1)


def test_lambda_ssim_zero_keeps_the_four_keys(monkeypatch):
    """forward with the launches replaced by host arithmetic: only the dict's keys and the composition are looked at."""
    import adam_dehaze_amd.loss as L
    monkeypatch.setattr(L, "l1_loss", lambda a, b: (a - b).abs().mean())
    monkeypatch.setattr(L, "ssim_per_image", lambda a, b, r=1.0: torch.full((a.shape[0],), 0.25))
    p, t = torch.rand(2, 3, 8, 8), torch.rand(2, 3, 8, 8)
    total, comps = L.DehazingLoss(content=False, perceptual=False, lambda_ssim=0)(p, t)
    assert set(comps) == {"l1", "content", "perceptual", "total"}
    total3, comps3 = L.DehazingLoss(content=False, perceptual=False, lambda_ssim=0.3)(p, t)
    assert set(comps3) == {"l1", "content", "perceptual", "ssim", "total"}
    assert float(comps3["ssim"]) == 0.75
    assert abs(float(total3) - (float(total) + 0.3 * 0.75)) < 1e-6
    assert comps3["total"] is total3


def test_factories_read_the_config_key():
    from adam_dehaze_amd.loss import get_dehazing_loss, get_joint_loss
    from training.loss import SSIMLoss, ssim_per_image      # noqa: F401  (re-exported like their neighbours)
    jt = {"lambda_dehazing": 1.0, "lambda_classification": 0.2, "lambda_detection": 0.5}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        assert get_dehazing_loss({}).lambda_ssim == 0.0
        assert get_dehazing_loss({"loss": {}}).lambda_ssim == 0.0
        assert get_dehazing_loss({"loss": {"lambda_ssim": 0.2}}).lambda_ssim == 0.2
        j = get_joint_loss({"joint_training": jt})
        assert j.dehazing_loss.lambda_ssim == 0.0 and j.dehazing_loss.ssim_loss is None
        j = get_joint_loss({"joint_training": jt, "loss": {"lambda_ssim": 0.4}})
        assert j.dehazing_loss.lambda_ssim == 0.4 and j.dehazing_loss.ssim_loss is not None
