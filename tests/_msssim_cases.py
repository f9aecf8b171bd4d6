"""Shapes, inputs and bounds shared by tests/test_msssim_hostemu_cpu.py and tests/test_gpu_msssim.py (csrc/msssim.hip against
tests/_msssim_ref64.py).  CPU only; nothing here touches the library."""
import torch

from tests import _msssim_ref64 as R64

EPS = 2.0 ** -24
U53 = R64.U53

# csrc/msssim.hip: the forward tiles the (H-10) x (W-10) window positions 16 x 32 and stages 26 x 42 pixels per tile; the
# backward tiles the H x W pixels 12 x 22 and stages 32 x 42 pixels per tile
MSF_TH, MSF_TW, MSB_TH, MSB_TW, HALO = 16, 32, 12, 22, 10
ISSUE_SHAPES = [(11, 11), (11, 40), (12, 27), (37, 53), (64, 64)]
# one pixel under, at and over: a forward tile plus its halo (26 x 42: the last window of the first tile); a backward tile
# (12 x 22; 11 is the smallest side there is); a backward tile plus its halo on both sides (32 x 42)
TILE_EDGE_SHAPES = [(MSF_TH + HALO + d, MSF_TW + HALO + d) for d in (-1, 0, 1)] + \
                   [(MSB_TH + d, MSB_TW + d) for d in (-1, 0, 1)] + \
                   [(MSB_TH + 2 * HALO + d, MSB_TW + 2 * HALO + d) for d in (-1, 0, 1)]
KINDS = ["identical", "constant", "noise", "outside"]
COEFS = [(1.0, 0.0), (0.0, 1.0), (0.3, -0.7)]


def inputs(kind, N, H, W, data_range=1.0, seed=0):
    """(pred, target) fp32 [N,3,H,W] on the CPU, |value| <= 1.1 data_range (the M of the error budget in _msssim_ref64)"""
    gen = torch.Generator().manual_seed(H * 1000 + W * 7 + N + seed)
    t = torch.rand(N, 3, H, W, generator=gen)
    if kind == "identical":
        p = t.clone()
    elif kind == "constant":                                 # zero variance: D2 is C2 and a cancellation residue
        t = torch.rand(N, 3, 1, 1, generator=gen).expand(N, 3, H, W).contiguous()
        p = torch.rand(N, 3, 1, 1, generator=gen).expand(N, 3, H, W).contiguous()
    elif kind == "noise":                                    # the regime training lives in: the gradient terms cancel
        p = (t + 0.02 * torch.randn(N, 3, H, W, generator=gen)).clamp(-0.1, 1.1)
    elif kind == "outside":                                  # LightweightDehazeModel's output is not clamped
        p = 1.2 * torch.rand(N, 3, H, W, generator=gen) - 0.1
        t = 1.2 * torch.rand(N, 3, H, W, generator=gen) - 0.1
    elif kind == "negated":                                  # CS < 0 at the fine levels: MS-SSIM clamps to exactly 0
        p = 1.0 - t
    else:
        raise ValueError(kind)
    return (p * data_range).float().contiguous(), (t * data_range).float().contiguous()


def coef_planes(N, a, b):
    """[N,3] float64 coefficient arrays: (a, b) on every plane but plane (N-1, 1), which gets (0, 0)"""
    ca, cb = torch.full((N, 3), a, dtype=torch.float64), torch.full((N, 3), b, dtype=torch.float64)
    ca[N - 1, 1] = 0.0
    cb[N - 1, 1] = 0.0
    return ca, cb


def fwd_reference(x, y, data_range):
    """((SSIM, CS) [N,3] float64, their bounds): FWD_UNITS 2^-53 of the terms; the kernel stores float64, so no fp32 rounding"""
    S, CS = R64.level_stats(x, y, data_range)
    TS, TCS = R64.level_terms(x, y, data_range)
    return (S, CS), (R64.FWD_UNITS * U53 * TS, R64.FWD_UNITS * U53 * TCS)


def pool_reference(x):
    """(avg_pool2d in float64, its bound): the sum of four values and the product with 0.25, exact for fp32 inputs of similar
    magnitude and within 2 roundings of the absolute values otherwise"""
    return R64.pool(x.double()), 2 * U53 * R64.pool(x.double().abs())


def bwd_reference(x, y, ca, cb, data_range, g_coarse=None, fp32_out=True):
    """(gradient [N,3,H,W] float64, its bound): EPS |ref| for the one fp32 store (none for a float64 gradient) +
    BWD_UNITS 2^-53 of the terms"""
    ref, terms = R64.level_closed_form(x, y, ca, cb, data_range, g_coarse)
    return ref, (EPS * ref.abs() if fp32_out else 0.0) + R64.BWD_UNITS * U53 * terms


def worst(got, ref, bound):
    """max |err| / bound, counting 0 / 0 as 0 and err > 0 = bound as inf; NaN in `got` is inf"""
    err = (got.double() - ref).abs()
    err = torch.where(torch.isnan(err), torch.full_like(err, float("inf")), err)
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound)
    return float(ratio.max()) if ratio.numel() else 0.0
