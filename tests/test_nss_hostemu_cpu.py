"""csrc/nss.hip without a GPU: the source file, compiled by the host C++ compiler against tools/host_emu with AddressSanitizer and
UndefinedBehaviorSanitizer, run as a stand-alone program (tools/host_emu/nss_main.cpp) on heap blocks of exactly the addressed
bytes behind poison, and held to the float64 reference of tests/_nss_ref64.py with the bounds of the GPU test
(tests/_nss_cases.py).  A read or a write outside a block -- global or LDS, the LDS arrays being statics of exactly their size --
is the sanitizer's to report.  The build caps the grid at 2, so a batch of three images, or a plane of more than two regions,
already walks the region loop that on the device starts at 65,535; and it sets the second stage's last level to 2 partials and its
chunks to 2, so a region of 4 tiles already adds its partials in levels, as on the device one of more than 160 does.  Nothing is
loaded into Python."""
import numpy as np
import pytest
import torch

from tests import _hostemu as E
from tests import _nss_cases as K
from tests import _nss_ref64 as R

HALVE, MOMENTS = 0, 1


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    d = tmp_path_factory.mktemp("nss_emu")
    exe = E.build(d, "nss", "nss_main.cpp", defines=("NSS_MAX_GRID=2", "NSS_LAST=2", "NSS_CHUNK=2"))
    return lambda: E.Script(exe, d)


def _f64(s, k, shape):
    t = s.get(k, np.float64)
    assert not torch.isnan(t).any(), "a float64 output element still holds its poison"
    return t.view(*shape)


def _src(s, src):
    return s.vec(src.reshape(-1), np.float32 if src.dtype == torch.float32 else np.float64)


def _moments(emu, src, Hc, Wc, rh, rw):
    """adh_nss_moments on exactly sized blocks; src fp32 [N,3,H,W] or float64 [N,H,W]"""
    rgb = int(src.dtype == torch.float32)
    N, Hh, Ww = src.shape[0], src.shape[-2], src.shape[-1]
    nt, nreg = K.tiles(rh, rw), N * (Hc // rh) * (Wc // rw)
    s = emu()
    partial, out = s.out(nreg * nt * 24, np.float64), s.out(nreg * 24, np.float64)
    s.call(MOMENTS, (rgb, N, Hh, Ww, Hc, Wc, rh, rw, nt), (_src(s, src), partial, out))
    assert s.run() == [0]
    _f64(s, partial, (-1,))                                  # every partial of every tile was written
    return _f64(s, out, (N, Hc // rh, Wc // rw, 24))


def _halve(emu, src, Hc, Wc):
    rgb = int(src.dtype == torch.float32)
    N, Hh, Ww = src.shape[0], src.shape[-2], src.shape[-1]
    OH, OW = (Hc + 1) // 2, (Wc + 1) // 2
    s = emu()
    dst = s.out(N * OH * OW, np.float64)
    s.call(HALVE, (rgb, N, Hh, Ww, Hc, Wc), (_src(s, src), dst))
    assert s.run() == [0]
    return _f64(s, dst, (N, OH, OW))


@pytest.mark.parametrize("shape", K.MOMENT_SHAPES + [K.MANY_TILES_EMU], ids=lambda s: "x".join(map(str, s)))
def test_moments_vs_float64(emu, shape):
    H, W, Hc, Wc, rh, rw = shape
    kind = K.KINDS[(K.MOMENT_SHAPES + [K.MANY_TILES_EMU]).index(shape) % 4]
    N = 3 if H * W <= 400 else 1                             # three images over a grid of two: the loop runs
    x, _, _ = K.moment_reference(kind, N, H, W, Hc, Wc, rh, rw)
    ratio = K.check_moments(_moments(emu, x, Hc, Wc, rh, rw), kind, N, H, W, Hc, Wc, rh, rw)
    print(f"{kind} {N}x3x{H}x{W} crop {Hc}x{Wc} regions {rh}x{rw}: worst |err| / bound {ratio:.3g}")
    assert ratio <= 1.0


def test_flat_half_gives_exact_zero_products_and_equal_counts(emu):
    H, W = 12, 40
    x, ref, _ = K.moment_reference("halfflat", 1, H, W, H, W, H, W)
    got = _moments(emu, x, H, W, H, W)
    assert K.check_moments(got, "halfflat", 1, H, W, H, W, H, W) <= 1.0
    n = H * W
    for k in range(4):
        assert float(got[0, 0, 0, 3 + 5 * k] + got[0, 0, 0, 5 + 5 * k]) < n      # the flat half's products are in neither set
        assert bool((got[..., 3 + 5 * k] == ref[..., 3 + 5 * k]).all()) and bool((got[..., 5 + 5 * k] == ref[..., 5 + 5 * k]).all())


@pytest.mark.parametrize("H,W", K.HALVE_SIDES)
def test_halve_vs_float64(emu, H, W):
    x, Y, ref, bound = K.halve_reference("u8noise", 3, H, W, H, W)
    assert K.worst(_halve(emu, x, H, W), ref, bound) <= 1.0                         # grey formed on the fly
    assert K.worst(_halve(emu, Y, H, W), ref, bound) <= 1.0                         # a float64 plane


def test_second_scale_and_crop(emu):
    """the halved crop of a 23 x 45 plane, then moments of that float64 plane in 5 x 10 regions"""
    H, W, Hc, Wc = 23, 45, 20, 40
    x, Y, ref, bound = K.halve_reference("ramp", 1, H, W, Hc, Wc)
    y2 = _halve(emu, x, Hc, Wc)
    assert tuple(y2.shape) == (1, 10, 20) and K.worst(y2, ref, bound) <= 1.0
    got = _moments(emu, y2, 10, 20, 5, 10)
    flat = R.flat_windows(ref)
    mb, taus, ps = R.moment_bounds(ref, 5, 10, flat, dY=bound)
    for tau, p in zip(taus, ps):
        assert bool((p.abs()[p != 0] > tau[p != 0]).all()), "a bad case"
    assert K.worst(got, R.moments(ref, 5, 10), mb) <= 1.0


def test_refusals(emu):
    N, H, W = 1, 12, 16
    x = K.inputs("uniform", N, H, W)
    s = emu()
    px = s.vec(x.reshape(-1))
    partial, out, dst = s.out(24, np.float64), s.out(24, np.float64), s.out(6 * 8, np.float64)
    ok_m, ok_h = (1, N, H, W, H, W, H, W, 1), (1, N, H, W, H, W)
    bad = []
    for k in range(3):
        bad.append(s.call(MOMENTS, ok_m, tuple(None if i == k else b for i, b in enumerate((px, partial, out)))))
    for k in range(2):
        bad.append(s.call(HALVE, ok_h, tuple(None if i == k else b for i, b in enumerate((px, dst)))))
    for ints in ((2, N, H, W, H, W, H, W, 1), (-1, N, H, W, H, W, H, W, 1), (1, 0, H, W, H, W, H, W, 1),
                 (1, N, H, W, H + 1, W, H + 1, W, 1), (1, N, H, W, H, W + 1, H, W + 1, 1), (1, N, H, W, H, W, 5, W, 1),
                 (1, N, H, W, H, W, H, 5, 1), (1, N, H, W, H, W, H, W, 2), (1, N, H, W, H, W, 0, W, 1),
                 (1, N, H, W, 0, W, H, W, 1), (1, N, 0, W, H, W, H, W, 1)):
        bad.append(s.call(MOMENTS, ints, (px, partial, out)))
    for ints in ((2, N, H, W, H, W), (1, 0, H, W, H, W), (1, N, H, W, H + 1, W), (1, N, H, W, H, W + 1), (1, N, H, W, 0, W)):
        bad.append(s.call(HALVE, ints, (px, dst)))
    bad.append(s.call(MOMENTS, ok_m, (px, partial, px)))     # outputs over the input or each other
    bad.append(s.call(MOMENTS, ok_m, (px, px, out)))
    bad.append(s.call(MOMENTS, ok_m, (px, out, out)))
    bad.append(s.call(HALVE, ok_h, (px, px)))
    rcs = s.run()                                            # Script.run also checks that the inputs are unchanged
    assert [rcs[k] for k in bad] == [E.ADH_E_ARG] * len(bad), rcs
    assert all(s.unchanged(k) for k in (partial, out, dst))
