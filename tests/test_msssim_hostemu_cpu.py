"""csrc/msssim.hip without a GPU: the source file, compiled by the host C++ compiler against tools/host_emu with
AddressSanitizer and UndefinedBehaviorSanitizer, run as a stand-alone program (tools/host_emu/msssim_main.cpp) on heap blocks of
exactly the addressed bytes behind poison, and held to the float64 reference of tests/_msssim_ref64.py with the bounds of the
GPU test (tests/_msssim_cases.py).  A read or a write outside a block -- global or LDS, the LDS arrays being statics of exactly
their size -- is the sanitizer's to report.  The build caps grid.y at 2, so the three planes of one image already walk the plane
loop that on the device starts at 65,535.  Nothing is loaded into Python."""
import numpy as np
import pytest
import torch

from tests import _hostemu as E
from tests import _msssim_cases as K
from tests import _msssim_ref64 as R64

FWD, BWD, NUM_TILES = 0, 1, 2
ADH_E_UNSUPPORTED = -3


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    d = tmp_path_factory.mktemp("msssim_emu")
    exe = E.build(d, "msssim", "msssim_main.cpp", defines=("MSS_MAX_GRID_Y=2",))
    return lambda: E.Script(exe, d)


def _tiles(emu, H, W):
    s = emu()
    s.call(NUM_TILES, (H, W))
    return s.run()[0]


def _f64(s, k, shape):
    t = s.get(k, np.float64)
    assert not torch.isnan(t).any(), "a float64 output element still holds its poison"
    return t.view(*shape)


def _forward(emu, x, y, data_range, pool=True):
    """adh_msssim_level_fwd on exactly sized blocks -> SSIM, CS [N,3], pooled x, pooled y (float64)"""
    N, _, H, W = x.shape
    f64 = x.dtype == torch.float64
    ntiles = _tiles(emu, H, W)
    s = emu()
    dt = np.float64 if f64 else np.float32
    px, py = s.vec(x.reshape(-1), dt), s.vec(y.reshape(-1), dt)
    partial, ssim, cs = s.out(N * 3 * ntiles * 2, np.float64), s.out(N * 3, np.float64), s.out(N * 3, np.float64)
    PH, PW = H // 2, W // 2
    qx = s.out(N * 3 * PH * PW, np.float64) if pool else None
    qy = s.out(N * 3 * PH * PW, np.float64) if pool else None
    s.call(FWD, (int(f64), N, H, W, ntiles), (px, py, partial, ssim, cs, qx, qy), (data_range,))
    assert s.run() == [0]
    out = [_f64(s, ssim, (N, 3)), _f64(s, cs, (N, 3))]
    _f64(s, partial, (-1,))                                  # every partial of every plane was written
    if pool:
        out += [_f64(s, qx, (N, 3, PH, PW)), _f64(s, qy, (N, 3, PH, PW))]
    return out


def _backward(emu, x, y, ca, cb, data_range, g_coarse=None, out_f64=False):
    N, _, H, W = x.shape
    f64 = x.dtype == torch.float64
    s = emu()
    dt = np.float64 if f64 else np.float32
    px, py = s.vec(x.reshape(-1), dt), s.vec(y.reshape(-1), dt)
    ka, kb = s.vec(ca.reshape(-1), np.float64), s.vec(cb.reshape(-1), np.float64)
    kg = None if g_coarse is None else s.vec(g_coarse.reshape(-1), np.float64)
    out = s.out(N * 3 * H * W, np.float64 if out_f64 else np.float32)
    s.call(BWD, (int(f64), N, H, W, int(out_f64)), (px, py, ka, kb, kg, out), (data_range,))
    assert s.run() == [0]
    if out_f64:
        return _f64(s, out, (N, 3, H, W))
    got = s.get(out)
    E.assert_written(got, "gradient")
    return got.view(N, 3, H, W)


def _check_level(emu, kind, H, W, coef, data_range=1.0, N=1):
    x, y = K.inputs(kind, N, H, W, data_range)
    S, CS, qx, qy = _forward(emu, x, y, data_range)
    (rS, rCS), (bS, bCS) = K.fwd_reference(x, y, data_range)
    ratios = [K.worst(S, rS, bS), K.worst(CS, rCS, bCS)]
    for q, src in ((qx, x), (qy, y)):
        ref, bound = K.pool_reference(src)
        ratios.append(K.worst(q, ref, bound))
    ca, cb = K.coef_planes(N, *coef)
    g = _backward(emu, x, y, ca, cb, data_range)
    ref, bound = K.bwd_reference(x, y, ca, cb, data_range)
    ratios.append(K.worst(g, ref, bound))
    assert bool((g[N - 1, 1] == 0).all()) and not bool(torch.signbit(g[N - 1, 1]).any()), "a = b = 0: exact +0.0 expected"
    if kind == "identical":
        assert bool((S.float() == 1.0).all()) and bool((CS.float() == 1.0).all())      # what the public fp32 numbers round to
    print(f"{kind} {N}x3x{H}x{W} R={data_range} coef={coef}: worst |err| / bound: SSIM {ratios[0]:.3g} CS {ratios[1]:.3g} "
          f"pool {max(ratios[2:4]):.3g} gradient {ratios[4]:.3g}")
    assert max(ratios) <= 1.0, ratios


@pytest.mark.parametrize("H,W", [(11, 11), (11, 40), (12, 27)] + K.TILE_EDGE_SHAPES)
def test_one_level_vs_float64(emu, H, W):
    k = (H * 3 + W) % 3
    _check_level(emu, ("noise", "outside", "constant")[k], H, W, K.COEFS[(H + W) % 3])


def test_one_level_identical_and_data_range_255(emu):
    _check_level(emu, "identical", 13, 23, K.COEFS[2])
    _check_level(emu, "noise", 12, 27, K.COEFS[2], data_range=255.0, N=2)


def test_two_level_pyramid_with_odd_sides_at_both_levels(emu):
    """27 x 47 -> 13 x 23: the forward of level 0 pools, level 1 reads float64; the backward of level 1 writes float64, that of
    level 0 folds it in through the pool adjoint (row 26 and column 46 get none) and stores fp32"""
    N, H, W = 1, 27, 47
    x, y = K.inputs("noise", N, H, W)
    S0, CS0, x1, y1 = _forward(emu, x, y, 1.0)
    assert tuple(x1.shape) == (N, 3, 13, 23)
    rx1, ry1 = R64.pool(x.double()), R64.pool(y.double())
    S1, CS1 = _forward(emu, x1, y1, 1.0, pool=False)
    (rS1, _), (bS1, _) = K.fwd_reference(rx1, ry1, 1.0)
    (_, rCS0), (_, bCS0) = K.fwd_reference(x, y, 1.0)
    assert K.worst(S1, rS1, bS1) <= 1.0 and K.worst(CS0, rCS0, bCS0) <= 1.0
    a1, zero = torch.tensor([[0.6, -0.2, 0.0]], dtype=torch.float64), torch.zeros(1, 3, dtype=torch.float64)
    b0 = torch.tensor([[0.5, 0.0, 0.0]], dtype=torch.float64)
    g1 = _backward(emu, x1, y1, a1, zero, 1.0, out_f64=True)
    ref1, bound1 = K.bwd_reference(rx1, ry1, a1, zero, 1.0, fp32_out=False)
    assert K.worst(g1, ref1, bound1) <= 1.0
    g0 = _backward(emu, x, y, zero, b0, 1.0, g_coarse=g1)
    ref0, bound0 = K.bwd_reference(x, y, zero, b0, 1.0, g_coarse=ref1)
    # what level 1 was granted comes through the adjoint at a quarter
    carried = R64.level_closed_form(x, y, zero, zero, 1.0, bound1)[0]
    assert K.worst(g0, ref0, bound0 + carried) <= 1.0
    assert bool((g0[:, 1:, 26] == 0).all()) and bool((g0[:, 1:, :, 46] == 0).all())      # no coefficient, no coarse pixel
    assert bool((g0[0, 2] == 0).all())                                                     # nothing at either level
    assert bool((g0[0, 1, :26, :46] == (0.25 * g1[0, 1]).repeat_interleave(2, 0).repeat_interleave(2, 1).float()).all())


def test_refusals(emu):
    N, H, W = 1, 12, 13
    x, y = K.inputs("noise", N, H, W)
    ntiles = _tiles(emu, H, W)
    s = emu()
    px, py = s.vec(x.reshape(-1)), s.vec(y.reshape(-1))
    partial, ssim, cs = s.out(N * 3 * ntiles * 2, np.float64), s.out(N * 3, np.float64), s.out(N * 3, np.float64)
    qx, qy = s.out(N * 3 * 36, np.float64), s.out(N * 3 * 36, np.float64)
    ca, cb = s.vec(torch.ones(3, dtype=torch.float64), np.float64), s.vec(torch.ones(3, dtype=torch.float64), np.float64)
    g = s.out(N * 3 * H * W)
    fwd_ok = (px, py, partial, ssim, cs, qx, qy)
    bad, unsupported = [], []
    for k in range(5):
        bad.append(s.call(FWD, (0, N, H, W, ntiles), tuple(None if i == k else b for i, b in enumerate(fwd_ok)), (1.0,)))
    bad.append(s.call(FWD, (0, N, H, W, ntiles), (px, py, partial, ssim, cs, qx, None), (1.0,)))
    bad.append(s.call(FWD, (0, N, H, W, ntiles), (px, py, partial, ssim, cs, qx, qx), (1.0,)))
    for ints in ((0, 0, H, W, ntiles), (0, 65536, H, W, ntiles), (2, N, H, W, ntiles), (0, N, H, W, ntiles + 1)):
        bad.append(s.call(FWD, ints, fwd_ok, (1.0,)))
    bad.append(s.call(FWD, (0, N, H, W, ntiles), fwd_ok, (0.0,)))
    for h, w in ((10, W), (H, 10)):
        unsupported.append(s.call(FWD, (0, N, h, w, ntiles), fwd_ok, (1.0,)))
        unsupported.append(s.call(BWD, (0, N, h, w, 0), (px, py, ca, cb, None, g), (1.0,)))
        unsupported.append(s.call(NUM_TILES, (h, w)))
    bwd_ok = (px, py, ca, cb, None, g)
    for k in (0, 1, 2, 3, 5):
        bad.append(s.call(BWD, (0, N, H, W, 0), tuple(None if i == k else b for i, b in enumerate(bwd_ok)), (1.0,)))
    for ints in ((0, 0, H, W, 0), (0, 65536, H, W, 0), (0, N, H, W, 2), (-1, N, H, W, 0)):
        bad.append(s.call(BWD, ints, bwd_ok, (1.0,)))
    bad.append(s.call(BWD, (0, N, H, W, 0), (px, py, ca, cb, None, px), (1.0,)))         # the gradient over an input
    bad.append(s.call(BWD, (0, N, H, W, 0), (px, py, ca, cb, None, py), (1.0,)))
    rcs = s.run()                                            # Script.run also checks that the inputs are unchanged
    assert [rcs[k] for k in bad] == [E.ADH_E_ARG] * len(bad), rcs
    assert [rcs[k] for k in unsupported] == [ADH_E_UNSUPPORTED] * len(unsupported), rcs
    assert all(s.unchanged(k) for k in (partial, ssim, cs, qx, qy, g))
