"""Inputs shared by tests/test_gpu_ciede2000.py and tests/test_ciede2000_hostemu_cpu.py: CPU float32 [N,3,H,W] pairs.  The bound
both files hold the kernel to is TOL, derived and not tuned: dE00 stays below 128, where half an fp32 unit in the last place
is 3.8e-6; the float64 work in front of the store adds about 1e-12."""
import math

import numpy as np
import torch

from tests import _ref64_ciede as R

TOL = 5e-6
# N, H, W: one pixel; H * W = 63 (no multiple of 4); whole quads; 1395 pixels per image, so the images of the batch alternate
# alignment
SHAPES = [(1, 1, 1), (1, 7, 9), (2, 16, 20), (3, 31, 45)]


def ragged_shape(num_blocks):
    """(N, H, W) whose image takes at least three workgroups with a ragged last one; `num_blocks`: pixels -> workgroups"""
    H = 33
    W = next(w for w in range(1, 1 << 16) if num_blocks(H * w) >= 3 and (H * w) % 4)
    per = next(p for p in range(1, 1 << 20) if num_blocks(p + 1) == 2)           # pixels per workgroup
    assert (H * W) % per != 0 and num_blocks(H * W) == 3
    return 2, H, W


def rgb_pair(N, H, W, seed):
    """two 8-bit-derived sRGB batches, the second a disturbed copy of the first on half of its pixels"""
    g = torch.Generator().manual_seed(seed)
    a = torch.randint(0, 256, (N, 3, H, W), generator=g)
    b = torch.randint(0, 256, (N, 3, H, W), generator=g)
    near = (a + torch.randint(-12, 13, (N, 3, H, W), generator=g)).clamp(0, 255)
    pick = torch.rand(N, 1, H, W, generator=g) < 0.5
    b = torch.where(pick, near, b)
    return a.float() / 255, b.float() / 255


def sharma_image():
    """the fourteen published pairs as one lab_input image of 2 x 7, and the table's values [2, 7]"""
    a = torch.tensor([p[0] for p in R.SHARMA_PAIRS], dtype=torch.float32).t().reshape(1, 3, 2, 7).contiguous()
    b = torch.tensor([p[1] for p in R.SHARMA_PAIRS], dtype=torch.float32).t().reshape(1, 3, 2, 7).contiguous()
    return a, b, np.array([p[2] for p in R.SHARMA_PAIRS]).reshape(2, 7)


def knife_edge_image():
    a = torch.tensor([p[0] for p in R.KNIFE_EDGE_PAIRS], dtype=torch.float32).t().reshape(1, 3, 1, 2).contiguous()
    b = torch.tensor([p[1] for p in R.KNIFE_EDGE_PAIRS], dtype=torch.float32).t().reshape(1, 3, 1, 2).contiguous()
    return a, b


def _polar(L, C, deg):
    return (L, C * math.cos(math.radians(deg)), C * math.sin(math.radians(deg)))


def crafted_lab():
    """[1,3,1,K] pairs on the branches of the formula, with the name of each column"""
    cols = [("both grey", (50, 0, 0), (60, 0, 0)),
            ("first grey", (50, 0, 0), (50, 10, 5)),
            ("second grey", (50, 10, 5), (52, 0, 0)),
            ("equal", (40, 10, -20), (40, 10, -20)),
            ("equal greys", (70, 0, 0), (70, 0, 0)),
            ("hues 179.9 apart", _polar(50, 10, 0), _polar(50, 10, 179.9)),
            ("hues 180.1 apart", _polar(50, 10, 0), _polar(50, 10, 180.1)),
            ("hues -179.9 apart", _polar(50, 10, 200), _polar(55, 30, 20.1)),
            ("hues -180.1 apart", _polar(50, 10, 200), _polar(55, 30, 19.9)),
            ("hue sum just below 360", _polar(50, 20, 10), _polar(50, 20, 349.9)),
            ("hue sum just above 360", _polar(50, 20, 10), _polar(50, 20, 350.1)),
            ("hue sum far below 360", _polar(50, 20, 5), _polar(60, 25, 200)),
            ("hue sum far above 360", _polar(50, 20, 300), _polar(60, 25, 100)),
            ("blue region (rotation term)", _polar(50, 60, 275), _polar(52, 50, 280)),
            ("large chroma", (30, 120, -110), (90, -100, 90)),
            ("black against white", (0, 0, 0), (100, 0, 0))]
    a = torch.tensor([c[1] for c in cols], dtype=torch.float32).t().reshape(1, 3, 1, len(cols)).contiguous()
    b = torch.tensor([c[2] for c in cols], dtype=torch.float32).t().reshape(1, 3, 1, len(cols)).contiguous()
    return a, b, [c[0] for c in cols]


def crafted_rgb():
    """[1,3,1,K] sRGB pairs: the clamp and NaN rule, black / white, and the float32 neighbours of both piecewise thresholds"""
    f32 = np.float32
    nan, inf = float("nan"), float("inf")
    knee = f32(R.SRGB_KNEE)
    k_lo, k_hi = float(np.nextafter(knee, f32(0))), float(np.nextafter(knee, f32(1)))
    # the grey whose Y is (6/29)^3
    v = f32(1.055 * R.LAB_KNEE ** (1 / 2.4) - 0.055)
    v_lo, v_hi = float(np.nextafter(v, f32(0))), float(np.nextafter(v, f32(1)))
    cols = [("black against white", (0, 0, 0), (1, 1, 1)),
            ("white against black", (1, 1, 1), (0, 0, 0)),
            ("equal", (0.3, 0.6, 0.9), (0.3, 0.6, 0.9)),
            ("below 0 and above 1", (-0.5, 1.5, 0.25), (0.1, 0.9, 2.0)),
            ("infinities and -0", (-inf, inf, -0.0), (0.5, 0.5, 0.5)),
            ("NaN", (nan, 0.5, 0.25), (0.5, nan, nan)),
            ("all NaN against black", (nan, nan, nan), (0, 0, 0)),
            ("sRGB knee, below", (k_lo, k_lo, k_lo), (0.2, 0.1, 0.05)),
            ("sRGB knee", (float(knee),) * 3, (0.2, 0.1, 0.05)),
            ("sRGB knee, above", (k_hi, k_hi, k_hi), (0.2, 0.1, 0.05)),
            ("Lab knee, below", (v_lo, v_lo, v_lo), (0.0, 0.2, 0.0)),
            ("Lab knee", (float(v),) * 3, (0.0, 0.2, 0.0)),
            ("Lab knee, above", (v_hi, v_hi, v_hi), (0.0, 0.2, 0.0)),
            ("saturated primaries", (1, 0, 0), (0, 0, 1))]
    a = torch.tensor([c[1] for c in cols], dtype=torch.float32).t().reshape(1, 3, 1, len(cols)).contiguous()
    b = torch.tensor([c[2] for c in cols], dtype=torch.float32).t().reshape(1, 3, 1, len(cols)).contiguous()
    return a, b, [c[0] for c in cols]


def reference(a, b, lab_input=False):
    """(map [N,H,W], mean [N]) in float64 from CPU tensors"""
    return R.ciede2000(a.numpy(), b.numpy(), lab_input)
