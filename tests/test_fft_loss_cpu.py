"""CPU checks of the frequency-domain L1 loss term: the float64 reference the GPU tests lean on
(tests/_fft_ref64.py) against an explicit DFT-matrix product and a known answer, the seeds' distance from the kink, and the
host-side plumbing of `lambda_fft` / `fft_norm` and of the size check."""
import math
import warnings

import pytest
import torch

from tests import _fft_ref64 as F64


@pytest.mark.parametrize("norm", F64.NORMS)
@pytest.mark.parametrize("Hh,Ww", [(8, 8), (8, 16)])
def test_reference_is_the_brute_force_dft(Hh, Ww, norm):
    p, t = F64.inputs(2, Hh, Ww, seed=3)
    val, grad = F64.loss_and_grad(p, t, norm)
    bval, bgrad = F64.brute_force(p, t, norm)
    # two float64 evaluations of one function, <= 16 terms per sum: a few hundred roundings of O(1) terms at worst
    assert abs(float(val) - float(bval)) <= 1e-13 * float(bval)
    assert float((grad - bgrad).abs().max()) <= 1e-13 * float(bgrad.abs().max())
    assert float(grad.abs().max()) > 0


def test_reference_self_conjugate_bins_are_exactly_real():
    for shape in [(1, 8, 8), (2, 8, 32), (3, 64, 16), (2, 32, 64)]:
        p, t = F64.inputs(*shape)
        re, im = F64.spectrum(p, t)
        Hh, Ww = shape[1:]
        for u in (0, Hh // 2):
            for v in (0, Ww // 2):
                assert bool((im[..., u, v] == 0).all())


@pytest.mark.parametrize("norm", F64.NORMS)
@pytest.mark.parametrize("Hh,Ww,u0,v0", [(8, 8, 1, 2), (16, 32, 3, 5), (64, 16, 0, 3), (8, 32, 2, 0)])
def test_known_answer_single_cosine(Hh, Ww, u0, v0, norm):
    """d = cos(2 pi (u0 y / H + v0 x / W)) has D = H W / 2 at (u0, v0) and at (H - u0, W - v0), both real, and 0 elsewhere:
    L = (2 * H W / 2) / (2 H W) = 0.5 under "backward" and 0.5 / sqrt(H W) under "ortho" (one image-channel or many alike)."""
    p, t = F64.cosine_pair(2, Hh, Ww, u0, v0)
    expect = 0.5 / math.sqrt(Hh * Ww) if norm == "ortho" else 0.5
    assert abs(float(F64.loss_of(p, t, norm)) - expect) <= 1e-12 * expect       # float64 samples: ~1e-16 each, H W bins


def test_recorded_seeds_keep_the_spectrum_off_the_kink():
    for shape in F64.SEEDS:
        p, t = F64.inputs(*shape)
        assert F64.min_kink_distance(p, t) >= F64.KINK_MIN, shape


def test_lambda_fft_is_stored_and_off_by_default():
    from adam_dehaze_amd.loss import DehazingLoss, FrequencyLoss
    d = DehazingLoss(content=False, perceptual=False)
    assert d.lambda_fft == 0.0 and d.fft_loss is None
    d = DehazingLoss(content=False, perceptual=False, lambda_fft=0)
    assert d.lambda_fft == 0.0 and d.fft_loss is None
    d = DehazingLoss(content=False, perceptual=False, lambda_fft=0.1, fft_norm="ortho")
    assert d.lambda_fft == 0.1 and isinstance(d.fft_loss, FrequencyLoss) and d.fft_loss.norm == "ortho"
    assert not list(d.parameters()) and not d.state_dict()
    with pytest.raises(ValueError):
        DehazingLoss(content=False, perceptual=False, lambda_fft=-0.1)
    with pytest.raises(ValueError):
        DehazingLoss(content=False, perceptual=False, lambda_fft=0.1, fft_norm="forward")
    with pytest.raises(ValueError):
        FrequencyLoss("none")


def test_lambda_fft_zero_keeps_todays_keys(monkeypatch):
    """forward with the launches replaced by host arithmetic: only the dict's keys and the composition are looked at."""
    import adam_dehaze_amd.loss as L
    monkeypatch.setattr(L, "l1_loss", lambda a, b: (a - b).abs().mean())
    monkeypatch.setattr(L, "ssim_per_image", lambda a, b, r=1.0: torch.full((a.shape[0],), 0.25))
    monkeypatch.setattr(L, "frequency_l1", lambda a, b, norm="backward": torch.tensor(2.0 if norm == "backward" else 0.5))
    p, t = torch.rand(2, 3, 8, 8), torch.rand(2, 3, 8, 8)
    total, comps = L.DehazingLoss(content=False, perceptual=False)(p, t)
    assert list(comps) == ["l1", "content", "perceptual", "total"]
    total0, comps0 = L.DehazingLoss(content=False, perceptual=False, lambda_fft=0)(p, t)
    assert list(comps0) == ["l1", "content", "perceptual", "total"] and torch.equal(total0, total)
    total1, comps1 = L.DehazingLoss(content=False, perceptual=False, lambda_fft=0.1)(p, t)
    assert list(comps1) == ["l1", "content", "perceptual", "fft", "total"]
    assert float(comps1["fft"]) == 2.0 and comps1["total"] is total1
    assert abs(float(total1) - (float(total) + 0.1 * 2.0)) < 1e-6
    total2, comps2 = L.DehazingLoss(content=False, perceptual=False, lambda_ssim=0.3, lambda_fft=0.1, fft_norm="ortho")(p, t)
    assert list(comps2) == ["l1", "content", "perceptual", "ssim", "fft", "total"]
    assert abs(float(total2) - (float(total) + 0.3 * 0.75 + 0.1 * 0.5)) < 1e-6


def test_factories_read_the_config_keys():
    from adam_dehaze_amd.loss import _lambda_fft, get_dehazing_loss, get_joint_loss
    from training.loss import FrequencyLoss, frequency_l1      # noqa: F401  (re-exported like their neighbours)
    jt = {"lambda_dehazing": 1.0, "lambda_classification": 0.2, "lambda_detection": 0.5}
    assert _lambda_fft(None) == _lambda_fft({}) == _lambda_fft({"loss": None}) == {"lambda_fft": 0.0, "fft_norm": "backward"}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for cfg in ({}, {"loss": {}}, {"loss": {"lambda_ssim": 0.2}}, {"loss": {"lambda_fft": 0}}):
            d = get_dehazing_loss(cfg)
            assert d.lambda_fft == 0.0 and d.fft_loss is None
        d = get_dehazing_loss({"loss": {"lambda_fft": 0.1}})
        assert d.lambda_fft == 0.1 and d.fft_norm == "backward" and d.fft_loss.norm == "backward" and d.ssim_loss is None
        d = get_dehazing_loss({"loss": {"lambda_fft": 0.2, "fft_norm": "ortho", "lambda_ssim": 0.3}})
        assert d.lambda_fft == 0.2 and d.fft_loss.norm == "ortho" and d.lambda_ssim == 0.3
        j = get_joint_loss({"joint_training": jt})
        assert j.dehazing_loss.lambda_fft == 0.0 and j.dehazing_loss.fft_loss is None
        j = get_joint_loss({"joint_training": jt, "loss": {"lambda_fft": 0.4, "fft_norm": "ortho"}})
        assert j.dehazing_loss.lambda_fft == 0.4 and j.dehazing_loss.fft_loss.norm == "ortho"
        with pytest.raises(ValueError):
            get_dehazing_loss({"loss": {"lambda_fft": -1}})
        with pytest.raises(ValueError):
            get_joint_loss({"joint_training": jt, "loss": {"lambda_fft": 0.1, "fft_norm": "bad"}})


@pytest.mark.parametrize("Hh,Ww", [(30, 46), (32, 46), (30, 64), (4, 8), (8, 4), (8192, 8), (8, 8192)])
def test_unsupported_sizes_raise_before_any_launch(monkeypatch, Hh, Ww):
    """not a power of two, too small and too large, each way: a ValueError that says "power of two", raised on CPU tensors and
    with every route into the device library closed"""
    import adam_dehaze_amd.loss as L

    def closed(*a, **k):
        raise AssertionError("the device library was touched")
    for name in ("load", "call", "value"):
        monkeypatch.setattr(L.H, name, closed)
    p = torch.zeros(1, 3, Hh, Ww)
    with pytest.raises(ValueError, match="power of two"):
        L.frequency_l1(p, p)
    with pytest.raises(ValueError, match="power of two"):
        L.FrequencyLoss()(p, p)
    with pytest.raises(ValueError, match="fft_norm"):
        L.frequency_l1(torch.zeros(1, 3, 8, 8), torch.zeros(1, 3, 8, 8), norm="forward")
    with pytest.raises(ValueError, match=r"\[N,3,H,W\]"):
        L.frequency_l1(torch.zeros(1, 1, 8, 8), torch.zeros(1, 1, 8, 8))
