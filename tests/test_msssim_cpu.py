"""The float64 reference of the Gaussian-window SSIM and MS-SSIM against itself (closed form, autograd, central difference, known
values), and the host side of the feature: weights and config parsing, DehazingLoss with the term off, main.py's refusal,
summarize_scores with null entries.  No GPU and no library call."""
import os
import sys

import pytest
import torch
import yaml

from adam_dehaze_amd import image_io as IO
from adam_dehaze_amd import loss as L
from adam_dehaze_amd import metrics as M
from adam_dehaze_amd import train as T
from tests import _msssim_cases as K
from tests import _msssim_ref64 as R64

CONFIG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "config", "config.yaml")

# --------------------------------------------------------------------------------------------------------------- the reference
def test_window_is_wangs():
    g = R64.window()
    assert g.dtype == torch.float64 and g.numel() == 11 and abs(float(g.sum()) - 1.0) < 1e-15
    assert torch.equal(g, g.flip(0)) and abs(float(g[5] / g[4]) - 2.718281828459045 ** (1 / 4.5)) < 1e-14
    assert M.MS_SSIM_WEIGHTS == R64.MS_SSIM_WEIGHTS and M.ms_ssim_min_side() == R64.min_side(5) == 176


@pytest.mark.parametrize("a,b", K.COEFS)
def test_closed_form_level_gradient_is_autograds(a, b):
    x, y = K.inputs("noise", 1, 23, 29)
    ca, cb = K.coef_planes(1, a, b)
    grad, terms = R64.level_closed_form(x, y, ca, cb)
    auto = R64.level_autograd(x, y, ca, cb)
    assert float((grad - auto).abs().max()) <= 1e-15 and float(grad.abs().max()) > 1e-4
    assert bool((terms >= grad.abs() * (1 - 1e-12)).all())                   # the terms bound the value they bound the error of
    assert bool((grad[0, 1] == 0).all())                                     # plane (0, 1) has a = b = 0


def test_closed_form_level_gradient_against_a_central_difference():
    x, y = K.inputs("outside", 1, 14, 17)
    ca, cb = K.coef_planes(1, 0.3, -0.7)
    grad, _ = R64.level_closed_form(x, y, ca, cb)
    f = lambda z: float(((R64.level_stats(z, y)[0] * ca) + (R64.level_stats(z, y)[1] * cb)).sum())
    h = 1e-6
    for c, i, j in ((0, 0, 0), (0, 7, 9), (2, 13, 16), (2, 5, 0)):
        d = torch.zeros_like(x, dtype=torch.float64)
        d[0, c, i, j] = h
        fd = (f(x.double() + d) - f(x.double() - d)) / (2 * h)
        assert abs(fd - float(grad[0, c, i, j])) <= 1e-8 * max(1.0, abs(fd)), (c, i, j, fd, float(grad[0, c, i, j]))


def test_pyramid_chain_is_autograds_with_odd_sides_and_a_quarter_per_pixel():
    x, y = K.inputs("noise", 2, 45, 50)
    w = (0.2, 0.3, 0.5)
    g_up = torch.tensor([0.7, -1.3], dtype=torch.float64)
    val, grad, terms = R64.ms_ssim_closed_form(x, y, g_up, 1.0, w)
    aval, auto = R64.ms_ssim_autograd(x, y, g_up, 1.0, w)
    assert torch.equal(val, aval) and float((grad - auto).abs().max()) <= 1e-15 and float(grad.abs().max()) > 1e-5
    assert bool((val > 0.9).all()) and bool((terms > 0).all())


def test_known_values():
    t = torch.rand(1, 3, 176, 176, generator=torch.Generator().manual_seed(1))
    assert float(R64.ssim_gaussian(t, t)) == 1.0 and float(R64.ms_ssim(t, t)) == 1.0
    # pred = 1 - target: the structure is negated, CS < 0 at levels 0..3, so the product is exactly 0 with gradient exactly 0
    V, _ = R64.pyramid_values((1 - t).double(), t.double())
    assert bool((V[:4] < 0).all())
    val, grad, _ = R64.ms_ssim_closed_form(1 - t, t, [1.0])
    aval, auto = R64.ms_ssim_autograd(1 - t, t, [1.0])
    assert float(val) == 0.0 and float(aval) == 0.0 and bool((grad == 0).all()) and bool((auto == 0).all())
    # a little noise keeps every factor near 1
    p = t + 0.02 * torch.randn(t.shape, generator=torch.Generator().manual_seed(2))
    V, _ = R64.pyramid_values(p.double(), t.double())
    assert bool((V > 0.99).all()) and 0.99 < float(R64.ms_ssim(p, t)) < 1.0
    # independent noise: a factor clamps -- not an input to compare gradients on
    q = torch.rand(t.shape, generator=torch.Generator().manual_seed(3))
    V, _ = R64.pyramid_values(q.double(), t.double())
    assert bool((V <= 0).any())


def test_user_weights_are_used_as_given():
    x, y = K.inputs("noise", 1, 44, 47)
    V, _ = R64.pyramid_values(x.double(), y.double(), 1.0, 3)
    want = (V[0] ** 2.0 * V[1] ** 0.5 * V[2] ** 3.0).mean(1)
    assert float((R64.ms_ssim(x, y, 1.0, (2.0, 0.5, 3.0)) - want).abs().max()) < 1e-15    # not renormalised
    assert float((R64.ms_ssim(x, y, 1.0, (1.0,)) - R64.ssim_gaussian(x, y)).abs().max()) < 1e-15


# --------------------------------------------------------------------------------------------------------------- host logic
def test_weights_are_checked():
    assert M.check_ms_ssim_weights([0.5, 0.5]) == (0.5, 0.5)
    for bad in ((), (0.1,) * 6, (0.5, 0.0), (0.5, -1.0), (float("inf"),), 0.5):
        with pytest.raises(ValueError, match="1 to 5 positive"):
            M.check_ms_ssim_weights(bad)
    assert [M.ms_ssim_min_side(k) for k in (1, 2, 3, 5)] == [11, 22, 44, 176]


def test_config_parsing_and_the_term_off_constructs_nothing():
    assert L._lambda_msssim(None) == {} and L._lambda_msssim({"loss": {"lambda_msssim": 0.0, "msssim_weights": [1, 1]}}) == {}
    assert L._lambda_msssim({"loss": {"lambda_msssim": 0.2}}) == {"lambda_msssim": 0.2, "msssim_weights": None}
    assert L._lambda_msssim({"loss": {"lambda_msssim": 0.2, "msssim_weights": [0.3, 0.3, 0.4]}}) == \
        {"lambda_msssim": 0.2, "msssim_weights": (0.3, 0.3, 0.4)}
    off = L.DehazingLoss(content=False, perceptual=False)
    assert off.msssim_loss is None and off.lambda_msssim == 0.0 and not list(off.children())
    on = L.DehazingLoss(content=False, perceptual=False, lambda_msssim=0.2, msssim_weights=(0.3, 0.3, 0.4))
    assert isinstance(on.msssim_loss, L.MSSSIMLoss) and on.msssim_loss.weights == (0.3, 0.3, 0.4)
    assert L.MSSSIMLoss().weights == M.MS_SSIM_WEIGHTS
    with pytest.raises(ValueError, match="lambda_msssim"):
        L.DehazingLoss(content=False, perceptual=False, lambda_msssim=-1.0)
    with pytest.raises(ValueError, match="1 to 5 positive"):
        L.DehazingLoss(content=False, perceptual=False, lambda_msssim=0.1, msssim_weights=(1, 2, 3, 4, 5, 6))
    assert T._OPT_IN_TERMS["ms_ssim"] == "1 - MS-SSIM"
    assert T._ms_ssim_switch({}) == {} and T._ms_ssim_switch({"evaluation": {"ms_ssim": False}}) == {}
    assert T._ms_ssim_switch({"evaluation": {"ms_ssim": True}}) == {"use_ms_ssim": True}


def test_shipped_config_leaves_everything_off():
    with open(CONFIG) as f:
        config = yaml.safe_load(f)
    assert L._lambda_msssim(config) == {} and T._ms_ssim_switch(config) == {}
    assert not (config.get("demo") or {}).get("ms_ssim")


def test_main_refuses_ms_ssim_without_target(monkeypatch):
    import main as Mn
    monkeypatch.setattr(T, "run_demo", lambda *a, **k: pytest.fail("must not run"))
    monkeypatch.setattr(T, "build_joint_system", lambda *a, **k: pytest.fail("must not build"))
    for argv in (["--mode", "demo", "--input", "hazy", "--ms-ssim"], ["--mode", "demo", "--ms-ssim"], ["--ms-ssim"]):
        monkeypatch.setattr(sys, "argv", ["main.py", "--device", "cpu"] + argv)
        with pytest.raises(SystemExit) as ei:
            Mn.main()
        assert "--ms-ssim needs" in str(ei.value)
    calls = []
    monkeypatch.setattr(T, "run_demo", lambda *a, **k: calls.append((a[1:], k)))
    monkeypatch.setattr(sys, "argv", ["main.py", "--config", CONFIG, "--mode", "demo", "--input", "hazy", "--target", "clear", "--ms-ssim",
                                     "--device", "cpu"])
    Mn.main()
    assert calls == [(("hazy", "demo", False), {"target": "clear", "ms_ssim": True})]


def test_run_demo_refuses_the_config_switch_without_target_before_building(tmp_path, monkeypatch):
    (tmp_path / "hazy").mkdir()
    IO.save_image(str(tmp_path / "hazy" / "a.png"), torch.zeros(8, 8, 3, dtype=torch.uint8))
    monkeypatch.setattr(T, "_joint_system_for_evaluation", lambda *a, **k: pytest.fail("must not build"))
    with pytest.raises(SystemExit, match="needs --target"):
        T.run_demo({"demo": {"ms_ssim": True}}, str(tmp_path / "hazy"), str(tmp_path / "out"))
    with pytest.raises(ValueError, match="needs `targets`"):
        IO.dehaze_files({}, [], str(tmp_path / "out"), ms_ssim=True)


def _record(name, intensity, base, extra=None):
    r = {"file": name, "intensity": intensity, "scored": True, **dict(zip(IO.SCORE_KEYS, base))}
    if extra is not None:
        r.update(zip(IO.MS_SSIM_SCORE_KEYS, extra))
    return r


def test_summary_with_null_entries():
    base = (20.0, 0.5, 4.0, 10.0, 0.25, 9.0)
    recs = [_record("a", "low", base, (0.5, 0.75, 0.25, 0.5)), _record("b", "low", base, (0.75, None, 0.5, None)),
            _record("c", "high", base, (None, None, None, None)), {"file": "d", "intensity": "low", "scored": False}]
    s = IO.summarize_scores(recs)
    low, high, al = s["dehazed"]["low_intensity"], s["dehazed"]["high_intensity"], s["dehazed"]["all"]
    assert low["ssim_gaussian"] == 0.625 and low["ms_ssim"] == 0.75 and low["ms_ssim_too_small"] == 1
    assert "ssim_gaussian_too_small" not in low and low["samples"] == 2
    assert high["ssim_gaussian"] is None and high["ms_ssim"] is None
    assert high["ssim_gaussian_too_small"] == 1 and high["ms_ssim_too_small"] == 1
    assert al["ssim_gaussian"] == 0.625 and al["ms_ssim"] == 0.75 and al["ms_ssim_too_small"] == 2 and al["samples"] == 3
    assert s["hazy"]["low_intensity"]["ssim_gaussian"] == 0.375 and s["hazy"]["low_intensity"]["ms_ssim"] == 0.5
    # records scored without the switch keep today's entries
    plain = IO.summarize_scores([_record("a", "low", base)])
    assert set(plain["dehazed"]["all"]) == {"psnr", "ssim", "ciede2000", "samples"}
    assert IO.SCORE_KEYS == ("psnr", "ssim", "ciede2000", "hazy_psnr", "hazy_ssim", "hazy_ciede2000")
