"""csrc/lpips.hip without a GPU: the source file, compiled by the host C++ compiler against the stand-in header of tools/host_emu
(its ADH_HOST_EMU_STREAM section: the 8-lane sums and the block's wave_sum run on the emulator's __shfl_xor) with
AddressSanitizer and UndefinedBehaviorSanitizer, run as a stand-alone program on heap blocks of exactly their sizes
(tests/_hostemu.py) and held to the float64 restatements and bounds of tests/_ref64.py, the ones tests/test_gpu_lpips.py holds
the library to.  A second program is built with LP_PPB = 32, so that the forward's partial blocks end inside a few dozen
pixels.  Every call is made twice, on outputs of its own, and the two must agree bit for bit; inputs come back unchanged."""
import os
import re
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest
import torch

from tests import _hostemu as E
from tests import _ref64 as R64

ENTRY_POINTS = ["adh_lpips_s2d", "adh_lpips_s2d_bwd", "adh_lpips_layer_num_blocks", "adh_lpips_layer", "adh_lpips_layer_bwd",
                "adh_rows_sum"]                                                  # the driver's call numbers
S2D, S2D_BWD, LAYER_NBLK, LAYER, LAYER_BWD, ROWS_SUM = range(6)
SMALL = {"LP_PPB": 32}
EPS = E.EPS
# lpips' ScalingLayer: ((2 x - 1) - shift) / scale = x a + b
_SHIFT, _SCALE = (-0.030, -0.088, -0.188), (0.458, 0.448, 0.450)
A3 = [float(np.float32(2.0 / s)) for s in _SCALE]
B3 = [float(np.float32((-1.0 - sh) / s)) for sh, s in zip(_SHIFT, _SCALE)]


def test_every_entry_point_is_called():
    src = open(os.path.join(E.ROOT, "adam-dehaze_amd", "csrc", "lpips.hip")).read()
    assert sorted(re.findall(r'extern "C" int (adh_\w+)', src)) == sorted(ENTRY_POINTS)
    me = open(__file__).read()
    for name in ("S2D", "S2D_BWD", "LAYER_NBLK", "LAYER", "LAYER_BWD", "ROWS_SUM"):
        assert re.search(r"s\.call\(%s," % name, me), name


@pytest.fixture(scope="module")
def emus(tmp_path_factory):
    d = tmp_path_factory.mktemp("lpips_emu")
    dirs = {False: d / "default", True: d / "small"}
    for sub in dirs.values():
        sub.mkdir()
    with ThreadPoolExecutor(2) as pool:
        exe = dict(zip((False, True), pool.map(lambda small: E.build(
            dirs[small], "lpips", "lpips_main.cpp", [f"{k}={v}" for k, v in SMALL.items()] if small else (), sanitize=E.FLOAT_CAST),
            (False, True))))
    return lambda small=False: E.Script(exe[small], d)


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _twice(s, runs):
    for k1, k2 in zip(*runs):
        assert (s.after[k1] == s.after[k2]).all(), "two identical calls differ"
    return runs[0]


def _getf(s, k, what):
    t = s.get(k)
    E.assert_written(t, what)
    return t


# ------------------------------------------------------------------------------------------------ space-to-depth
def _s2d_dims(Hh, Ww):
    return (Hh + 4 - 11) // 4 + 1 + 2, (Ww + 4 - 11) // 4 + 1 + 2          # the wrapper's OH + 2, OW + 2


@pytest.mark.parametrize("Hh,Ww", [(11, 11), (13, 15), (21, 27), (33, 19)])
def test_lpips_s2d_forward_backward(emus, Hh, Ww):
    """odd image sizes that are no multiple of the 4-pixel cells: the last cells are partly outside the image; and a grid one
    cell row and column short, whose uncovered pixels get a gradient of exactly 0"""
    s = emus()
    N = 2
    OHp, OWp = _s2d_dims(Hh, Ww)
    x = torch.rand(N, 3, Hh, Ww, generator=_gen(Hh * Ww))
    g = torch.randn(N, OHp, OWp, 48, generator=_gen(Hh + Ww))
    gs = g[:, :OHp - 1, :OWp - 1].contiguous()
    bx, bg, bgs = s.vec(x), s.vec(g), s.vec(gs)
    n_out = N * OHp * OWp * 48
    runs = []
    for _ in range(2):
        out, gx, gxs = s.out(n_out), s.out(N * 3 * Hh * Ww), s.out(N * 3 * Hh * Ww)
        s.call(S2D, [N, Hh, Ww, OHp, OWp], [bx, out], A3 + B3)
        s.call(S2D_BWD, [N, Hh, Ww, OHp, OWp], [bg, gx], A3)
        s.call(S2D_BWD, [N, Hh, Ww, OHp - 1, OWp - 1], [bgs, gxs], A3)
        runs.append((out, gx, gxs))
    assert s.run() == [0] * 6
    out, gx, gxs = _twice(s, runs)
    out = _getf(s, out, "s2d").view(N, OHp, OWp, 48)
    ref, mag = R64.lpips_s2d(x, A3, B3, OHp, OWp)
    # one multiply-add per element: two roundings (one if contracted to FMA), each at most EPS of |x a| + |b|; the host does
    # not contract: the product's rounding and the sum's, 2 EPS of the terms at the most
    E.assert_bound(out, ref, 2 * EPS * mag, "s2d forward")
    assert (out[mag == 0] == 0).all(), "cells and taps outside the image are exactly 0"
    assert bool((mag == 0).any())
    gref = R64.lpips_s2d_bwd(g, A3, Hh, Ww)
    E.assert_bound(_getf(s, gx, "s2d backward").view(N, 3, Hh, Ww), gref, EPS * gref.abs(), "s2d backward")            # one product
    gref = R64.lpips_s2d_bwd(gs, A3, Hh, Ww)
    gxs = _getf(s, gxs, "s2d backward, short grid").view(N, 3, Hh, Ww)
    E.assert_bound(gxs, gref, EPS * gref.abs(), "s2d backward, short grid")
    hh, ww = min(Hh, 4 * (OHp - 1) - 2), min(Ww, 4 * (OWp - 1) - 2)
    assert hh < Hh or ww < Ww
    assert (gxs[:, :, hh:] == 0).all() and (gxs[:, :, :, ww:] == 0).all()


# ------------------------------------------------------------------------------------------------ per-tap distance
LAYER_CASES = [(small, C_, HW) for small, ppb in ((True, 32), (False, 1024)) for C_ in (8, 64, 72) for HW in (1, ppb - 1, ppb + 1)] + \
    [(True, 4, 67)]


@pytest.mark.parametrize("small,C_,HW", LAYER_CASES)
def test_lpips_layer_forward_backward_and_rows_sum(emus, small, C_, HW):
    """C = 8: two of a pixel's eight lanes hold a quad; 64: two quads each; 72: lanes 0 and 1 a third; 4: one lane.  HW on both
    sides of a block of LP_PPB pixels; the backward walks 32 pixels a block.  Post-ReLU-like features with all-zero pixels, equal
    pixels and a dominant channel (tests/_ref64.py, lpips_features)."""
    s = emus(small)
    ppb = SMALL["LP_PPB"] if small else 1024
    N = 2
    seed = C_ + HW
    fa, fb, w, fam = R64.lpips_features(N, HW, C_, lambda k, *shape: torch.randn(shape, generator=_gen(seed + k)),
                                        lambda k, *shape: torch.rand(shape, generator=_gen(seed + k)))
    g_val = torch.tensor([0.7, -1.3])
    nblk = -(-HW // ppb)
    scale = float(np.float32(1.0 / HW))
    prev = torch.randn(N, generator=_gen(9))
    bfa, bfb, bw, bgv = s.vec(fa), s.vec(fb), s.vec(w), s.vec(g_val)
    c_n = s.call(LAYER_NBLK, [HW])
    runs = []
    for _ in range(2):
        part, gfa, o0, o1 = s.out(N * nblk), s.out(N * HW * C_), s.out(N), s.out(N, init=prev)
        s.call(LAYER, [N, HW, C_, nblk], [bfa, bfb, bw, part])
        s.call(LAYER_BWD, [N, HW, C_], [bfa, bfb, bw, bgv, gfa])
        s.call(ROWS_SUM, [N, nblk, 0], [part, o0], [scale])
        s.call(ROWS_SUM, [N, nblk, 1], [part, o1], [scale])
        runs.append((part, gfa, o0, o1))
    rcs = s.run()
    assert rcs[c_n] == nblk and rcs[c_n + 1:] == [0] * 8, rcs
    part, gfa, o0, o1 = _twice(s, runs)
    part = _getf(s, part, "partials").view(N, nblk)
    dpix, blk_ref, blk_bound = R64.lpips_layer_blocks(fa, fb, w, ppb)
    E.assert_bound(part, blk_ref, blk_bound, f"layer partials C={C_} HW={HW}")
    # rows_sum: float64 sum of the fp32 partials times the fp32 scale, rounded once; accumulate adds one fp32 sum
    v = part.double().sum(1) * scale
    o0 = _getf(s, o0, "rows_sum")
    E.assert_bound(o0, v, EPS * v.abs() * (1 + 1e-6), "rows_sum")
    E.assert_bound(s.get(o1), prev.double() + v, EPS * (v.abs() + (prev.double() + v).abs()) * (1 + 1e-6), "rows_sum accumulate")
    E.assert_bound(o0, dpix.mean(1), blk_bound.sum(1) / HW + 2 * EPS * dpix.mean(1), "layer mean")
    gfa = _getf(s, gfa, "layer backward").view(N, HW, C_)
    ref = R64.lpips_layer_grad(fa, fb, w, g_val)
    E.assert_bound(gfa, ref, R64.lpips_layer_grad_bound(fa, fb, w, g_val, ref), f"layer backward C={C_} HW={HW}")
    assert (gfa[fam == 4] == 0).all(), "fa == fb: the gradient is exactly 0"
    assert (gfa[fam == 3] == 0).all(), "fa and fb all zero at a pixel: gradient 0"
    if bool((fam == 1).any()):
        assert torch.isfinite(gfa[fam == 1]).all() and bool((gfa[fam == 1] != 0).any()), "zero pixel of fa: delta / 1e-10, finite"


def test_lpips_layer_identical_inputs_exactly_zero(emus):
    """LPIPS(x, x) = 0: both unit vectors are the same fp32 numbers, every partial and every gradient element exactly 0"""
    s = emus(True)
    N, HW, C_ = 2, 33, 72
    fa, _, w, _ = R64.lpips_features(N, HW, C_, lambda k, *shape: torch.randn(shape, generator=_gen(k)),
                                     lambda k, *shape: torch.rand(shape, generator=_gen(k)))
    bfa, bfb, bw, bgv = s.vec(fa), s.vec(fa.clone()), s.vec(w), s.vec(torch.tensor([0.7, -1.3]))
    part, gfa = s.out(N * 2), s.out(N * HW * C_)
    s.call(LAYER, [N, HW, C_, 2], [bfa, bfb, bw, part])
    s.call(LAYER_BWD, [N, HW, C_], [bfa, bfb, bw, bgv, gfa])
    assert s.run() == [0, 0]
    assert (s.get(part) == 0).all() and (s.get(gfa) == 0).all()


def test_argument_rejections_write_nothing(emus):
    s = emus()
    bv = s.vec(torch.rand(3 * 16 * 16))
    of = s.out(1200)
    bad = [s.call(S2D, [1, Hh, Ww, OHp, OWp], [bv, of], A3 + B3)
           for Hh, Ww, OHp, OWp in ((10, 16, 5, 5), (16, 10, 5, 5), (16, 16, 2, 5), (16, 16, 5, 2))]
    bad += [s.call(S2D, [0, 16, 16, 5, 5], [bv, of], A3 + B3), s.call(S2D, [1, 16, 16, 5, 5], [bv, None], A3 + B3),
            s.call(S2D_BWD, [0, 16, 16, 5, 5], [bv, of], A3), s.call(S2D_BWD, [1, 16, 16, 5, 5], [None, of], A3)]
    bad += [s.call(LAYER, [N, HW, C_, nblk], [bv, bv, bv, of]) for N, HW, C_, nblk in ((1, 8, 6, 1), (1, 8, 0, 1), (1, 8, 8, 2),
                                                                                      (0, 8, 8, 1), (1, 0, 8, 0))]
    bad += [s.call(LAYER_BWD, [N, HW, C_], [bv, bv, bv, bv, of]) for N, HW, C_ in ((1, 8, 6), (0, 8, 8), (1, 0, 8))]
    bad += [s.call(ROWS_SUM, [0, 1, 0], [bv, of], [1.0]), s.call(ROWS_SUM, [1, 0, 0], [bv, of], [1.0]),
            s.call(ROWS_SUM, [1, 1, 0], [bv, None], [1.0])]
    rcs = s.run()
    assert [rcs[i] for i in bad] == [E.ADH_E_ARG] * len(bad), rcs
    assert s.unchanged(of), "a rejected call wrote to an output"
