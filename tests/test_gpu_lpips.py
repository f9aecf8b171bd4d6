"""The LPIPS kernels of csrc/lpips.hip through the C ABI, each entry point against a float64 restatement (tests/_ref64.py):
the scaling + space-to-depth input stage and its adjoint, the per-tap distance with its gradient, and the row sum.  The
loss tests see them only end to end on one 67 x 99 image; here they run at image sizes past the 4096-block caps, at
channel counts below the 8 lanes of a pixel group and with a ragged last trip, at the 1024-pixel block edges, and on
post-ReLU features with all-zero pixels, where the gradient of the unit normalisation needs a stated convention.

Every output is prefilled with NaN inside a NaN guard band that must stay untouched; every entry point runs twice and
must reproduce itself bit for bit.  Tolerances are in EPS = 2^-24 relative to the sum of |terms| added; the comments name
the fp32 operations behind each count."""
import ctypes as C

import numpy as np
import pytest
import torch

from adam_dehaze_amd import _hip as H
from tests import _ref64 as R64
from tests._util import DEV, EPS, _assert_bound, _nan, _pad_untouched, _padded, _twice

pytestmark = pytest.mark.gpu
LP_PPB = 1024           # pixels per block of the forward partials (lpips.hip)

# lpips' ScalingLayer: ((2 x - 1) - shift) / scale = x a + b
_SHIFT, _SCALE = (-0.030, -0.088, -0.188), (0.458, 0.448, 0.450)
A3 = [float(np.float32(2.0 / s)) for s in _SCALE]
B3 = [float(np.float32((-1.0 - sh) / s)) for sh, s in zip(_SHIFT, _SCALE)]


def _gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def _rand(*shape, seed=0):
    return torch.rand(shape, device=DEV, dtype=torch.float32, generator=_gen(seed))


def _randn(*shape, seed=0):
    return torch.randn(shape, device=DEV, dtype=torch.float32, generator=_gen(seed))


def _rejected(name, *args):
    with pytest.raises(RuntimeError):
        H.call(name, *args)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ space-to-depth
S2D_HW = [(11, 11), (12, 15), (67, 99), (64, 64), (224, 224), (512, 1024), (1024, 2048)]


def _s2d_dims(Hh, Ww):
    return (Hh + 4 - 11) // 4 + 1 + 2, (Ww + 4 - 11) // 4 + 1 + 2          # the wrapper's OH + 2, OW + 2


@pytest.mark.parametrize("Hh,Ww", S2D_HW)
def test_lpips_s2d_forward_backward_adjoint(Hh, Ww):
    """(512, 1024) is 131 x 259 cells x 16 = 0.54 M threads' worth against a cap of 1 M; (1024, 2048) is past it (2.1 M), and
    its backward (2 M pixels) as well."""
    N = 2 if Hh * Ww <= 512 * 1024 else 1
    OHp, OWp = _s2d_dims(Hh, Ww)
    a3, b3 = (C.c_float * 3)(*A3), (C.c_float * 3)(*B3)
    x = _rand(N, 3, Hh, Ww, seed=Hh * Ww)
    n_out = N * OHp * OWp * 48

    def fwd(img):
        def run():
            whole, out = _padded(n_out)
            H.call("adh_lpips_s2d", img.data_ptr(), N, Hh, Ww, a3, b3, OHp, OWp, out.data_ptr())
            torch.cuda.synchronize()
            assert _pad_untouched(whole, n_out)
            return (out.view(N, OHp, OWp, 48),)
        return _twice(run)[0]
    out = fwd(x)
    ref, mag = R64.lpips_s2d(x, A3, B3, OHp, OWp)
    # one multiply-add per element: two roundings (one if contracted to FMA), each at most EPS of |x a| + |b|
    _assert_bound(out, ref, 1.5 * EPS * mag, "s2d forward")
    assert (out[mag == 0] == 0).all(), "cells and taps outside the image are exactly 0"
    assert bool((mag == 0).any()) and bool((mag[:, 1:-2, 1:-2] > 0).all())

    g = _randn(N, OHp, OWp, 48, seed=Hh + Ww)

    def run_bwd():
        whole, gx = _padded(N * 3 * Hh * Ww)
        H.call("adh_lpips_s2d_bwd", g.data_ptr(), N, Hh, Ww, a3, OHp, OWp, gx.data_ptr())
        torch.cuda.synchronize()
        assert _pad_untouched(whole, N * 3 * Hh * Ww)
        return (gx.view(N, 3, Hh, Ww),)
    gx, = _twice(run_bwd)
    gref = R64.lpips_s2d_bwd(g, A3, Hh, Ww)
    _assert_bound(gx, gref, EPS * gref.abs(), "s2d backward")            # one product
    # adjoint identity on the kernels' own outputs: <s2d(x) - s2d(0), g> == <x, s2d_bwd(g)>
    out0 = fwd(torch.zeros_like(x))
    lhs = ((out.double() - out0.double()) * g.double()).sum()
    rhs = (x.double() * gx.double()).sum()
    # the forward elements carry 1.5 EPS (|x a| + |b|) each (twice: out and out0), the backward ones EPS |g a|
    slack = (g.double().abs() * (1.5 * EPS * (mag + R64.lpips_s2d(torch.zeros_like(x), A3, B3, OHp, OWp)[1]))).sum() + \
        (x.double().abs() * EPS * gref.abs()).sum()
    assert abs(float(lhs - rhs)) <= float(slack) * (1 + 1e-6), f"adjoint identity off by {abs(float(lhs - rhs)):.3e} (slack {float(slack):.3e})"


@pytest.mark.parametrize("Hh,Ww", [(11, 11), (12, 15), (67, 99)])
def test_lpips_s2d_bwd_uncovered_pixels(Hh, Ww):
    """With one cell row and column fewer than the image needs, the pixels beyond the last cell are covered by no cell:
    their gradient is exactly 0."""
    N = 2
    OHp, OWp = _s2d_dims(Hh, Ww)
    OHp, OWp = OHp - 1, OWp - 1
    a3 = (C.c_float * 3)(*A3)
    g = _randn(N, OHp, OWp, 48, seed=3)
    gx = _nan(N, 3, Hh, Ww)
    H.call("adh_lpips_s2d_bwd", g.data_ptr(), N, Hh, Ww, a3, OHp, OWp, gx.data_ptr())
    torch.cuda.synchronize()
    gref = R64.lpips_s2d_bwd(g, A3, Hh, Ww)
    _assert_bound(gx, gref, EPS * gref.abs(), "s2d backward, short grid")
    hh, ww = min(Hh, 4 * OHp - 2), min(Ww, 4 * OWp - 2)
    assert hh < Hh or ww < Ww
    assert (gx[:, :, hh:] == 0).all() and (gx[:, :, :, ww:] == 0).all()


def test_lpips_s2d_rejects():
    x, out = _rand(1, 3, 16, 16), _nan(1, 5, 5, 48)
    a3, b3 = (C.c_float * 3)(*A3), (C.c_float * 3)(*B3)
    for Hh, Ww, OHp, OWp, N in ((10, 16, 5, 5, 1), (16, 10, 5, 5, 1), (16, 16, 2, 5, 1), (16, 16, 5, 2, 1), (16, 16, 5, 5, 0)):
        _rejected("adh_lpips_s2d", x.data_ptr(), N, Hh, Ww, a3, b3, OHp, OWp, out.data_ptr())
    _rejected("adh_lpips_s2d_bwd", out.data_ptr(), 0, 16, 16, a3, 5, 5, x.data_ptr())
    assert torch.isnan(out).all()


# ------------------------------------------------------------------------------------------------ per-tap distance
LAYER_C = [4, 8, 28, 32, 64, 192, 256, 384]
LAYER_HW_SMALL = [1, 31, 32, 33, 1023, 1024, 1025]
# every C at every block-edge size with N = 1 and 3; past the backward's 2048 x 32-pixel cap one case per size and a few C
LAYER_CASES = [(c, hw, n) for c in LAYER_C for hw in LAYER_HW_SMALL for n in (1, 3)] + \
    [(4, 65536, 3), (192, 65536, 1), (28, 65537, 1), (64, 65537, 3), (8, 255 * 511, 3), (256, 255 * 511, 1)]


def _features(N, HW, C_, seed):
    """post-ReLU-like features: |randn| with ~30 % zeros; by pixel index (p + n) % 7: 1 -> fa all zero, 2 -> fb all zero,
    3 -> both all zero, 4 -> fa == fb, 5 -> one channel of fa dominant by 1e4."""
    return R64.lpips_features(N, HW, C_, lambda k, *shape: _randn(*shape, seed=seed + k),
                              lambda k, *shape: _rand(*shape, seed=seed + k))


@pytest.mark.parametrize("C_,HW,N", LAYER_CASES)
def test_lpips_layer_forward_and_rows_sum(C_, HW, N):
    fa, fb, w, fam = _features(N, HW, C_, seed=C_ + HW)
    nblk = H.value("adh_lpips_layer_num_blocks", HW)
    assert nblk == -(-HW // LP_PPB)

    def run():
        wp, part = _padded(N * nblk)
        H.call("adh_lpips_layer", fa.data_ptr(), fb.data_ptr(), w.data_ptr(), N, HW, C_, part.data_ptr(), nblk)
        torch.cuda.synchronize()
        assert _pad_untouched(wp, N * nblk)
        return (part.view(N, nblk),)
    part, = _twice(run)
    dpix, blk_ref, blk_bound = R64.lpips_layer_blocks(fa, fb, w, LP_PPB)
    _assert_bound(part, blk_ref, blk_bound, f"layer partials C={C_} HW={HW}")
    # rows_sum: float64 sum of the fp32 partials times the fp32 scale, rounded once; accumulate adds one fp32 sum
    scale = float(np.float32(1.0 / HW))
    prev = _randn(N, seed=9)

    def run_sum():
        w0, o0 = _padded(N)
        w1, o1 = _padded(N)
        o1.copy_(prev)
        H.call("adh_rows_sum", part.data_ptr(), N, nblk, scale, o0.data_ptr(), 0)
        H.call("adh_rows_sum", part.data_ptr(), N, nblk, scale, o1.data_ptr(), 1)
        torch.cuda.synchronize()
        assert _pad_untouched(w0, N) and _pad_untouched(w1, N)
        return o0, o1
    o0, o1 = _twice(run_sum)
    v = part.double().sum(1) * scale
    _assert_bound(o0, v, EPS * v.abs() * (1 + 1e-6), "rows_sum")
    _assert_bound(o1, prev.double() + v, EPS * (v.abs() + (prev.double() + v).abs()) * (1 + 1e-6), "rows_sum accumulate")
    # and end to end against the float64 mean
    _assert_bound(o0, dpix.mean(1), blk_bound.sum(1) / HW + 2 * EPS * dpix.mean(1), "layer mean")


@pytest.mark.parametrize("C_,HW,N", LAYER_CASES)
def test_lpips_layer_backward(C_, HW, N):
    """Against the closed-form float64 gradient with the kernel's convention at an all-zero pixel of fa (the second term of
    the normalisation's gradient is dropped: grad = delta / 1e-10; torch autograd returns NaN there).  fa == fb gives a
    gradient of exactly 0."""
    fa, fb, w, fam = _features(N, HW, C_, seed=C_ + HW)
    g_val = torch.tensor([0.7, -1.3, 2.0][:N], device=DEV)

    def run():
        whole, gfa = _padded(N * HW * C_)
        H.call("adh_lpips_layer_bwd", fa.data_ptr(), fb.data_ptr(), w.data_ptr(), g_val.data_ptr(), N, HW, C_, gfa.data_ptr())
        torch.cuda.synchronize()
        assert _pad_untouched(whole, N * HW * C_)
        return (gfa.view(N, HW, C_),)
    gfa, = _twice(run)
    ref = R64.lpips_layer_grad(fa, fb, w, g_val)
    bound = R64.lpips_layer_grad_bound(fa, fb, w, g_val, ref)
    _assert_bound(gfa, ref, bound, f"layer backward C={C_} HW={HW}")
    same = (fam == 4)
    assert (gfa[same] == 0).all(), "fa == fb: the gradient is exactly 0"
    both = (fam == 3)
    assert (gfa[both] == 0).all(), "fa and fb all zero at a pixel: gradient 0"
    only_a = (fam == 1)
    if bool(only_a.any()):
        assert torch.isfinite(gfa[only_a]).all() and bool((gfa[only_a] != 0).any()), "zero pixel of fa: delta / 1e-10, finite"


@pytest.mark.parametrize("C_", [4, 28, 64, 384])
def test_lpips_layer_identical_inputs_exactly_zero(C_):
    """LPIPS(x, x) = 0: with fa == fb both unit vectors are the same fp32 numbers, so every partial and every gradient
    element is exactly 0 (not the rounding error of one product, which an fma-contracted a * ia - b * ib leaves)."""
    N, HW = 2, 1025
    fa, _, w, _ = _features(N, HW, C_, seed=C_)
    fb = fa.clone()
    nblk = H.value("adh_lpips_layer_num_blocks", HW)
    part, gfa = _nan(N, nblk), _nan(N, HW, C_)
    g_val = torch.tensor([0.7, -1.3], device=DEV)
    H.call("adh_lpips_layer", fa.data_ptr(), fb.data_ptr(), w.data_ptr(), N, HW, C_, part.data_ptr(), nblk)
    H.call("adh_lpips_layer_bwd", fa.data_ptr(), fb.data_ptr(), w.data_ptr(), g_val.data_ptr(), N, HW, C_, gfa.data_ptr())
    torch.cuda.synchronize()
    assert (part == 0).all(), f"partials of identical inputs: max {float(part.abs().max()):.3e}"
    assert (gfa == 0).all(), f"gradient of identical inputs: max {float(gfa.abs().max()):.3e}"


def test_lpips_layer_rejects():
    fa, w, g = _rand(1, 8, 8), _rand(8), torch.ones(1, device=DEV)
    part, gfa, out = _nan(4), _nan(1, 8, 8), _nan(1)
    for N, HW, C_, nblk in ((1, 8, 6, 1), (1, 8, 0, 1), (1, 8, 8, 2), (0, 8, 8, 1), (1, 0, 8, 0)):
        _rejected("adh_lpips_layer", fa.data_ptr(), fa.data_ptr(), w.data_ptr(), N, HW, C_, part.data_ptr(), nblk)
    for N, HW, C_ in ((1, 8, 6), (0, 8, 8), (1, 0, 8)):
        _rejected("adh_lpips_layer_bwd", fa.data_ptr(), fa.data_ptr(), w.data_ptr(), g.data_ptr(), N, HW, C_, gfa.data_ptr())
    for N, nblk in ((0, 1), (1, 0)):
        _rejected("adh_rows_sum", part.data_ptr(), N, nblk, 1.0, out.data_ptr(), 0)
    assert torch.isnan(part).all() and torch.isnan(gfa).all() and torch.isnan(out).all()
