"""Float64 torch restatement of torchvision's MobileNetV2 / V3-large / V3-small feature extractors plus this repository's
classifier head (classifier.{1,4}), and seeded state_dicts with torchvision's key names.  Test helper only: the
architectures are restated here independently of adam-dehaze_amd/classifier.py."""
import math

import torch
import torch.nn.functional as F

V2_SETTING = ((1, 16, 1, 1), (6, 24, 2, 2), (6, 32, 3, 2), (6, 64, 4, 2), (6, 96, 3, 1), (6, 160, 3, 2), (6, 320, 1, 1))
# (in, k, exp, out, SE, act, stride)
V3_LARGE = ((16, 3, 16, 16, 0, "RE", 1), (16, 3, 64, 24, 0, "RE", 2), (24, 3, 72, 24, 0, "RE", 1), (24, 5, 72, 40, 1, "RE", 2),
            (40, 5, 120, 40, 1, "RE", 1), (40, 5, 120, 40, 1, "RE", 1), (40, 3, 240, 80, 0, "HS", 2), (80, 3, 200, 80, 0, "HS", 1),
            (80, 3, 184, 80, 0, "HS", 1), (80, 3, 184, 80, 0, "HS", 1), (80, 3, 480, 112, 1, "HS", 1),
            (112, 3, 672, 112, 1, "HS", 1), (112, 5, 672, 160, 1, "HS", 2), (160, 5, 960, 160, 1, "HS", 1),
            (160, 5, 960, 160, 1, "HS", 1))
V3_SMALL = ((16, 3, 16, 16, 1, "RE", 2), (16, 3, 72, 24, 0, "RE", 2), (24, 3, 88, 24, 0, "RE", 1), (24, 5, 96, 40, 1, "HS", 2),
            (40, 5, 240, 40, 1, "HS", 1), (40, 5, 240, 40, 1, "HS", 1), (40, 5, 120, 48, 1, "HS", 1), (48, 5, 144, 48, 1, "HS", 1),
            (48, 5, 288, 96, 1, "HS", 2), (96, 5, 576, 96, 1, "HS", 1), (96, 5, 576, 96, 1, "HS", 1))
FEATURE_DIM = {"mobilenet_v2": 1280, "mobilenet_v3_large": 960, "mobilenet_v3_small": 576}


def make_divisible(v, d=8):
    nv = max(d, int(v + d / 2) // d * d)
    return nv + d if nv < 0.9 * v else nv


def _v3_setting(name):
    return V3_LARGE if name == "mobilenet_v3_large" else V3_SMALL


# ---------------------------------------------------------------------------------------------------------------- layout
def layers(name):
    """[(key prefix, kind, dict)] in network order: kind 'cna' (conv + bn), 'conv' (bare conv), 'bn', 'se'."""
    out = []
    f = "backbone.features."
    if name == "mobilenet_v2":
        out.append((f + "0", "cna", dict(cin=3, cout=32, k=3, groups=1)))
        cin, i = 32, 1
        for t, c, n, _s in V2_SETTING:
            for _ in range(n):
                hid = cin * t
                j = 0
                if t != 1:
                    out.append((f"{f}{i}.conv.0", "cna", dict(cin=cin, cout=hid, k=1, groups=1)))
                    j = 1
                out.append((f"{f}{i}.conv.{j}", "cna", dict(cin=hid, cout=hid, k=3, groups=hid)))
                out.append((f"{f}{i}.conv.{j + 1}", "conv", dict(cin=hid, cout=c, k=1, groups=1)))
                out.append((f"{f}{i}.conv.{j + 2}", "bn", dict(c=c)))
                cin, i = c, i + 1
        out.append((f"{f}{i}", "cna", dict(cin=cin, cout=1280, k=1, groups=1)))
        return out
    setting = _v3_setting(name)
    out.append((f + "0", "cna", dict(cin=3, cout=16, k=3, groups=1)))
    for i, (cin, k, exp, cout, se, _a, _s) in enumerate(setting, start=1):
        j = 0
        if exp != cin:
            out.append((f"{f}{i}.block.{j}", "cna", dict(cin=cin, cout=exp, k=1, groups=1)))
            j += 1
        out.append((f"{f}{i}.block.{j}", "cna", dict(cin=exp, cout=exp, k=k, groups=exp)))
        j += 1
        if se:
            out.append((f"{f}{i}.block.{j}", "se", dict(c=exp, sq=make_divisible(exp // 4))))
            j += 1
        out.append((f"{f}{i}.block.{j}", "cna", dict(cin=exp, cout=cout, k=1, groups=1)))
    last = setting[-1][3]
    out.append((f"{f}{len(setting) + 1}", "cna", dict(cin=last, cout=6 * last, k=1, groups=1)))
    return out


def state_dict(name, seed=0):
    """Seeded random state_dict with torchvision's key names (BN running statistics away from 0 / 1 so that eval mode
    differs from train mode) and the classifier head."""
    g = torch.Generator().manual_seed(seed)
    sd = {}

    def conv(p, cin, cout, k, groups, bias=False):
        fan_in = cin // groups * k * k
        sd[p + ".weight"] = torch.randn(cout, cin // groups, k, k, generator=g) * math.sqrt(2.0 / fan_in)
        if bias:
            sd[p + ".bias"] = 0.05 * torch.randn(cout, generator=g)

    def bn(p, c):
        sd[p + ".weight"] = 0.8 + 0.4 * torch.rand(c, generator=g)
        sd[p + ".bias"] = 0.05 * torch.randn(c, generator=g)
        sd[p + ".running_mean"] = 0.05 * torch.randn(c, generator=g)
        sd[p + ".running_var"] = 0.8 + 0.4 * torch.rand(c, generator=g)
        sd[p + ".num_batches_tracked"] = torch.tensor(0, dtype=torch.int64)

    for p, kind, a in layers(name):
        if kind == "cna":
            conv(p + ".0", a["cin"], a["cout"], a["k"], a["groups"])
            bn(p + ".1", a["cout"])
        elif kind == "conv":
            conv(p, a["cin"], a["cout"], a["k"], a["groups"])
        elif kind == "bn":
            bn(p, a["c"])
        else:
            conv(p + ".fc1", a["c"], a["sq"], 1, 1, bias=True)
            conv(p + ".fc2", a["sq"], a["c"], 1, 1, bias=True)
            sd[p + ".fc2.bias"] += 0.5      # keep the gate mostly inside Hardsigmoid's linear range
    fd = FEATURE_DIM[name]
    sd["classifier.1.weight"] = torch.randn(256, fd, generator=g) / math.sqrt(fd)
    sd["classifier.1.bias"] = 0.05 * torch.randn(256, generator=g)
    sd["classifier.4.weight"] = torch.randn(3, 256, generator=g) / 16.0
    sd["classifier.4.bias"] = 0.05 * torch.randn(3, generator=g)
    return sd


# ---------------------------------------------------------------------------------------------------------------- forward
# test hook of the kink audit (tests/_util.py: kink_recording): RECORD(conv weight key, pre-activation) at every ReLU / ReLU6
RECORD = None


def _act(x, a):
    return {"RE": F.relu, "RE6": F.relu6, "HS": F.hardswish, None: lambda v: v}[a](x)


def features(x, sd, name, training, masks=None):
    """Backbone features [N, feature_dim] (train-mode BN updates the running statistics in sd, as nn.BatchNorm2d does).
    masks: {conv weight key: bool [N, C, H, W]} -- the ReLU / ReLU6 derivative masks another implementation used, replayed
    as this graph's derivative at those layers (values unchanged), so both differentiate the same piece of the network; the
    ReLU between a squeeze-excite block's two 1x1 convolutions goes under its fc1.weight key."""
    v3 = name != "mobilenet_v2"
    eps, mom = (1e-3, 0.01) if v3 else (1e-5, 0.1)

    def bn(h, p):
        return F.batch_norm(h, sd[p + ".running_mean"], sd[p + ".running_var"], sd[p + ".weight"], sd[p + ".bias"],
                            training=training, momentum=mom, eps=eps)

    def cna(h, p, k, s, groups, a):
        h = F.conv2d(h, sd[p + ".0.weight"], None, s, (k - 1) // 2, 1, groups)
        if training:
            sd[p + ".1.num_batches_tracked"] += 1
        z = bn(h, p + ".1")
        if RECORD is not None and a in ("RE", "RE6"):
            RECORD(p + ".0.weight", z)
        m = masks.get(p + ".0.weight") if masks is not None else None
        if m is not None and a in ("RE", "RE6"):
            return _act(z, a).detach() + (z - z.detach()) * m.to(z.dtype)
        return _act(z, a)

    f = "backbone.features."
    if not v3:
        h = cna(x, f + "0", 3, 2, 1, "RE6")
        cin, i = 32, 1
        for t, c, n, s0 in V2_SETTING:
            for r in range(n):
                s = s0 if r == 0 else 1
                hid = cin * t
                q = f"{f}{i}.conv."
                o, j = h, 0
                if t != 1:
                    o = cna(o, q + "0", 1, 1, 1, "RE6")
                    j = 1
                o = cna(o, q + str(j), 3, s, hid, "RE6")
                o = bn(F.conv2d(o, sd[q + str(j + 1) + ".weight"]), q + str(j + 2))
                if training:
                    sd[q + str(j + 2) + ".num_batches_tracked"] += 1
                h = o + h if (s == 1 and cin == c) else o
                cin, i = c, i + 1
        h = cna(h, f"{f}{i}", 1, 1, 1, "RE6")
    else:
        setting = _v3_setting(name)
        h = cna(x, f + "0", 3, 2, 1, "HS")
        for i, (cin, k, exp, cout, se, a, s) in enumerate(setting, start=1):
            q = f"{f}{i}.block."
            o, j = h, 0
            if exp != cin:
                o = cna(o, q + "0", 1, 1, 1, a)
                j = 1
            o = cna(o, q + str(j), k, s, exp, a)
            j += 1
            if se:
                p = q + str(j)
                sc = F.adaptive_avg_pool2d(o, 1)
                z = F.conv2d(sc, sd[p + ".fc1.weight"], sd[p + ".fc1.bias"])
                if RECORD is not None:
                    RECORD(p + ".fc1.weight", z)
                m = masks.get(p + ".fc1.weight") if masks is not None else None
                sc = F.relu(z) if m is None else F.relu(z).detach() + (z - z.detach()) * m.to(z.dtype)
                sc = F.hardsigmoid(F.conv2d(sc, sd[p + ".fc2.weight"], sd[p + ".fc2.bias"]))
                o = o * sc
                j += 1
            o = cna(o, q + str(j), 1, 1, 1, None)
            h = o + h if (s == 1 and cin == cout) else o
        h = cna(h, f"{f}{len(setting) + 1}", 1, 1, 1, "HS")
    return torch.flatten(F.adaptive_avg_pool2d(h, 1), 1)


def classifier_forward(x, sd, name, training=False, masks=None, act_masks=None):
    """(logits, features) of FogIntensityClassifier(name): features -> [dropout mask 0] -> Linear -> ReLU -> [mask 1] ->
    Linear.  masks: (m0 [N, fd], m1 [N, 256]) pre-scaled dropout masks, or None (eval)."""
    f = features(x, sd, name, training, act_masks)
    h = f if masks is None else f * masks[0]
    h = F.relu(F.linear(h, sd["classifier.1.weight"], sd["classifier.1.bias"]))
    if masks is not None:
        h = h * masks[1]
    return F.linear(h, sd["classifier.4.weight"], sd["classifier.4.bias"]), f
