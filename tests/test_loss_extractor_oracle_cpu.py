"""CPU side of the loss-extractor gate (tests/test_gpu_loss_extractors.py): the generalised VGG / LPIPS oracles reproduce
their earlier form bit for bit at default arguments, run in float64 as well as fp32, replay forced ReLU masks and max-pool
choices, and give the fp32-against-float64 distance the GPU gate is measured in.  The last test walks ContentLoss._features
over an engine that only records its calls: a tap ON a conv index is followed by that conv's ReLU as a pass of its own."""
import warnings

import pytest
import torch
import torch.nn.functional as F

from oracle import ref_cpu as R
from tests import _loss_extractor as LX
from tests._thirdparty_init import lpips_alex_sd, vgg16_sd, vgg19_sd


def _images(shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(shape, generator=g), torch.rand(shape, generator=g)


# ------------------------------------------------------------------------------------------------ the earlier form
def _old_vgg16_prefix(x, sd, last_idx, prefix="model."):
    idx = 0
    for v in R.VGG16_CFG:
        if idx > last_idx:
            break
        if v == "M":
            x = F.max_pool2d(x, 2, 2)
            idx += 1
        else:
            x = F.conv2d(x, sd[f"{prefix}{idx}.weight"], sd[f"{prefix}{idx}.bias"], padding=1)
            idx += 1
            if idx > last_idx:
                break
            x = F.relu(x)
            idx += 1
    return x


def _old_content_loss(pred, target, sd):
    mean = torch.tensor(R.IMAGENET_MEAN).view(1, 3, 1, 1)
    std = torch.tensor(R.IMAGENET_STD).view(1, 3, 1, 1)
    a = (pred - mean) / std
    b = (target - mean) / std
    loss = 0.0
    for idx in (9, 16, 23):
        loss = loss + F.mse_loss(_old_vgg16_prefix(a, sd, idx), _old_vgg16_prefix(b, sd, idx))
    return loss / 3


def _old_lpips_alex(x, t, sd, prefix="loss_fn."):
    def taps(h):
        out, idx = [], 0
        for v in R.ALEX_CFG:
            if v == "M":
                h = F.max_pool2d(h, 3, 2)
                idx += 1
            else:
                _, k, s, p = v
                name = prefix + "net." + R.ALEX_SLICE_OF[idx]
                h = F.relu(F.conv2d(h, sd[name + ".weight"], sd[name + ".bias"], stride=s, padding=p))
                idx += 2
                out.append(h)
        return out
    shift = torch.tensor(R.LPIPS_SHIFT).view(1, 3, 1, 1)
    scale = torch.tensor(R.LPIPS_SCALE).view(1, 3, 1, 1)
    total = None
    for k, (a, b) in enumerate(zip(taps((x - shift) / scale), taps((t - shift) / scale))):
        na = a / (torch.sqrt(torch.sum(a * a, dim=1, keepdim=True)) + 1e-10)
        nb = b / (torch.sqrt(torch.sum(b * b, dim=1, keepdim=True)) + 1e-10)
        v = F.conv2d((na - nb) ** 2, sd[f"{prefix}lin{k}.model.1.weight"]).mean(dim=(2, 3), keepdim=True)
        total = v if total is None else total + v
    return total


def test_default_arguments_reproduce_the_earlier_oracle_bit_for_bit():
    sd = vgg16_sd(2)
    pred, target = _images((2, 3, 37, 51), 2)
    for last in range(31):
        assert torch.equal(R.vgg16_prefix(pred, sd, last), _old_vgg16_prefix(pred, sd, last)), last
    p_new, p_old = pred.clone().requires_grad_(True), pred.clone().requires_grad_(True)
    new, old = R.content_loss(p_new, target, sd), _old_content_loss(p_old, target, sd)
    new.backward()
    old.backward()
    assert torch.equal(new, old) and torch.equal(p_new.grad, p_old.grad)
    lsd = lpips_alex_sd(5)
    pred, target = _images((2, 3, 67, 99), 4)
    p_new, p_old = pred.clone().requires_grad_(True), pred.clone().requires_grad_(True)
    new, old = R.perceptual_loss(p_new, target, lsd), _old_lpips_alex(2 * p_old - 1, 2 * target - 1, lsd)
    new.mean().backward()
    old.mean().backward()
    assert torch.equal(new, old) and torch.equal(p_new.grad, p_old.grad)


def test_vgg19_state_dict_and_prefix():
    sd = vgg19_sd(1)
    convs = [k for k in sd if k.endswith(".weight")]
    assert len(convs) == 16 and sd["model.16.weight"].shape == (256, 256, 3, 3) and sd["model.34.weight"].shape == (512, 512, 3, 3)
    assert all(torch.equal(sd[k], vgg19_sd(1)[k]) for k in sd) and not torch.equal(sd["model.0.weight"], vgg19_sd(2)["model.0.weight"])
    x, _ = _images((1, 3, 32, 32), 0)
    # index 16 of vgg19.features is a conv: the prefix ends on its output, before the relu
    y16 = R.vgg16_prefix(x, sd, 16, cfg=R.VGG19_CFG)
    assert y16.shape == (1, 256, 8, 8) and bool((y16 < 0).any())
    assert torch.equal(R.vgg16_prefix(x, sd, 17, cfg=R.VGG19_CFG), F.relu(y16))
    assert R.vgg16_prefix(x, sd, 36, cfg=R.VGG19_CFG).shape == (1, 512, 1, 1)


def test_oracles_follow_the_input_dtype():
    pred, target = _images((1, 3, 33, 35), 3)
    for dt in (torch.float32, torch.float64):
        v = R.content_loss(pred.to(dt), target.to(dt), LX.cast_sd(vgg19_sd(0), dt), taps=(2, 9), cfg=R.VGG19_CFG)
        p = R.perceptual_loss(pred.to(dt), target.to(dt), LX.cast_sd(lpips_alex_sd(0), dt))
        assert v.dtype == dt and p.dtype == dt and p.shape == (1, 1, 1, 1)


CASES = [("vgg16", ("relu1_1", "relu2_2"), (2, 3, 37, 51)), ("vgg16", ("relu3_1", "relu3_3", "relu4_2"), (1, 3, 33, 32)),
         ("vgg19", LX.DEFAULT_NAMES, (2, 3, 37, 51)), ("lpips", None, (1, 3, 31, 31)), ("lpips", None, (2, 3, 35, 47))]


def _loss_and_grad(model, names, sd, pred, target, dt):
    p = pred.detach().to(dt).clone().requires_grad_(True)
    if model == "lpips":
        v = R.perceptual_loss(p, target.to(dt), LX.cast_sd(sd, dt))
        (v.view(-1) * torch.linspace(0.4, 1.7, v.shape[0], dtype=dt)).sum().backward()
    else:
        v = R.content_loss(p, target.to(dt), LX.cast_sd(sd, dt), taps=tuple(LX.taps_of(names)), cfg=LX.CFGS[model])
        (0.37 * v).backward()
    return v.detach(), p.grad


@pytest.mark.parametrize("model,names,shape", CASES, ids=lambda v: "-".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_forced_kinks_replay_and_fp32_distance(model, names, shape):
    """A float64 pass forced to its own kinks reproduces itself exactly (the mask and the gather select what relu and max
    selected), and the fp32 pass forced to the same kinks stays within fp32 rounding of it: err_ref, the unit of the GPU
    gate.  Free-running, a flipped kink moves the gradient by far more: 1e-4 of the scale separates the two."""
    sd = {"vgg16": vgg16_sd, "vgg19": vgg19_sd, "lpips": lpips_alex_sd}[model](7)
    pred, target = _images(shape, 11)
    (v64, g64), masks, pools = LX.record_kinks(lambda: _loss_and_grad(model, names, sd, pred, target, torch.float64))
    assert masks and pools and any(k.startswith(R.TARGET_KINKS) for k in masks)
    v64f, g64f = LX.run_forced(lambda: _loss_and_grad(model, names, sd, pred, target, torch.float64), masks, pools)
    assert torch.equal(v64f, v64) and torch.equal(g64f, g64)
    v32, g32 = LX.run_forced(lambda: _loss_and_grad(model, names, sd, pred, target, torch.float32), masks, pools)
    assert v32.dtype == torch.float32 and g32.dtype == torch.float32
    for what, a, ref in (("value", v32, v64), ("gradient", g32, g64)):
        err_ref, scale = LX.err_over_scale(a, ref)
        print(f"{model} {names} {shape} {what}: scale {scale:.3e} err_ref {err_ref:.2e}")
        assert scale > 1e-12 and 0 < err_ref < 1e-4, (what, scale, err_ref)
    # forcing is not a no-op: other masks give another function
    flipped = {k: ~m for k, m in masks.items()}
    v_other, _ = LX.run_forced(lambda: _loss_and_grad(model, names, sd, pred, target, torch.float64), flipped, pools)
    assert not torch.equal(v_other, v64)


class _Walk:
    """An engine that records the ops ContentLoss._features asks for."""
    record = False

    def __init__(self):
        self.ops = []

    def image_normalize_to_nhwc8(self, img, mean, std, holder):
        return "x"

    def conv(self, h, w, b, bn, *, k, stride, pad, relu):
        self.ops.append(("conv+relu" if relu else "conv", len(self.ops)))
        return self.ops[-1]

    def activation(self, h, act, capture=None):
        from adam_dehaze_amd import _hip as H
        assert act == H.ACT_RELU and capture is not None
        self.ops.append(("relu", len(self.ops)))
        return self.ops[-1]

    def maxpool(self, h, k):
        assert k == 2
        self.ops.append(("pool", len(self.ops)))
        return self.ops[-1]


def _walk(model, names):
    from adam_dehaze_amd.loss import ContentLoss
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        c = ContentLoss(model, list(names) if names else None)
    eng = _Walk()
    feats = c._features(eng, None, c.tap_indices, {})
    return [op[0] for op in eng.ops], [f[1] for f in feats]


def test_features_walk_runs_the_relu_behind_a_tapped_conv():
    # default VGG16: every conv fused with its relu, taps on the three pools -- what it launched before
    ops, taps = _walk("vgg16", None)
    assert ops == ["conv+relu"] * 2 + ["pool"] + ["conv+relu"] * 2 + ["pool"] + ["conv+relu"] * 3 + ["pool"] + ["conv+relu"] * 3 + ["pool"]
    assert taps == [5, 9, 13]
    # VGG19: index 16 is the fourth conv of block 3: tapped raw, then its relu, then the pool
    ops, taps = _walk("vgg19", None)
    # (and 23 is the third conv of block 4: the last tap, raw, nothing behind it)
    assert ops[6:] == ["conv+relu"] * 3 + ["conv", "relu", "pool"] + ["conv+relu"] * 2 + ["conv"]
    assert taps == [5, 9, 14]
    # relu1_1 -> 2 is conv 2: tapped raw, relu 3 on its own, pool 4, ...; relu2_2 -> 9 is the pool
    ops, taps = _walk("vgg16", ("relu1_1", "relu2_2"))
    assert ops == ["conv+relu", "conv", "relu", "pool", "conv+relu", "conv+relu", "pool"] and taps == [1, 6]
    # a tap on the last conv: nothing runs behind it
    ops, taps = _walk("vgg16", ("relu3_1", "relu3_3", "relu4_2"))
    assert ops[6:] == ["conv+relu", "conv", "relu", "conv+relu", "pool", "conv+relu", "conv+relu", "conv"] and taps == [7, 10, 13]
