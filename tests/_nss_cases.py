"""What tests/test_gpu_nss.py and tests/test_nss_hostemu_cpu.py share: the fixed-seed inputs, the shapes at the edges of the
kernel's tile, and the comparison of a kernel's moments and halved planes with the float64 reference of tests/_nss_ref64.py under
its counted bounds.  CPU only; references are cached per case and never modified."""
import functools

import torch

from tests import _nss_ref64 as R

TH, TW = 16, 32                       # csrc/nss.hip's tile; the staged block adds a ring of 4 (3 window + 1 neighbour)
KINDS = ("uniform", "u8noise", "ramp", "halfflat")

# (H, W, Hc, Wc, rh, rw): planes smaller than the window in one or both directions; one under, at and over the tile sides and
# tile + ring; regions equal to the plane, 1 x 1, 8 x 8 on 16 x 24, a region side that is no multiple of the tile side; a crop
# smaller than the plane
MOMENT_SHAPES = [
    (1, 1, 1, 1, 1, 1), (1, 9, 1, 9, 1, 9), (7, 9, 7, 9, 7, 9), (7, 9, 7, 9, 1, 1),
    (15, 31, 15, 31, 15, 31), (16, 32, 16, 32, 16, 32), (17, 33, 17, 33, 17, 33),
    (23, 39, 23, 39, 23, 39), (24, 40, 24, 40, 24, 40), (25, 41, 25, 41, 25, 41),
    (16, 24, 16, 24, 8, 8), (40, 52, 40, 52, 20, 26), (23, 45, 20, 40, 10, 40),
]
# regions of many tiles, where the second stage adds the partials in levels: 12 tiles under the host emulation (built with a last
# level of 2 and chunks of 2: three levels), 13 x 13 = 169 > 160 tiles on the device (one level of chunks of 64)
MANY_TILES_EMU = (40, 100, 40, 100, 40, 100)
MANY_TILES_GPU = (208, 416, 208, 416, 208, 416)
HALVE_SIDES = [(1, 1), (2, 7), (7, 2), (8, 9), (9, 8), (11, 13)]


# a hand-written libsvm model of two support vectors (tests/test_nss_cpu.py checks its closed form)
SVR_MODEL = """svm_type epsilon_svr
kernel_type rbf
gamma 0.05
nr_class 2
total_sv 2
rho -1.5
SV
0.75 1:1 2:-1 36:0.5
-0.25 1:0.5 3:2
"""


def tiles(rh, rw):
    return -(-rh // TH) * -(-rw // TW)


def inputs(kind, N, H, W, seed=0):
    """fp32 [N,3,H,W] in [0,1]"""
    g = torch.Generator().manual_seed(1000 * seed + 7 * H + W + KINDS.index(kind))
    if kind == "uniform":
        return torch.rand((N, 3, H, W), generator=g)
    u8 = torch.randint(0, 256, (N, 3, H, W), generator=g).float() / 255.0
    if kind == "u8noise":
        return u8
    if kind == "ramp":
        ramp = (torch.arange(H).view(1, 1, H, 1) * 0.5 + torch.arange(W).view(1, 1, 1, W) * 0.25) / max(H + W, 1)
        return (ramp + 0.25 * torch.rand((N, 3, H, W), generator=g)).clamp(0, 1).float()
    x = u8.clone()                    # halfflat: the left half one saturated 8-bit colour, the right half 8-bit noise
    x[:, :, :, : (W + 1) // 2] = 1.0
    return x


def worst(got, ref, bound):
    """max |err| / bound over the elements with a non-zero bound; elements with bound 0 must be equal"""
    assert not torch.isnan(got).any(), "NaN: an element was not written"
    err = (got.double() - ref).abs()
    exact = bound == 0
    assert bool((err[exact] == 0).all()), f"exact elements differ by up to {float(err[exact].max()):.3e}"
    return float((err[~exact] / bound[~exact]).max()) if bool((~exact).any()) else 0.0


@functools.lru_cache(maxsize=None)
def moment_reference(kind, N, H, W, Hc, Wc, rh, rw, seed=0):
    """(x, reference moments, bound) of the first scale; asserts on the reference alone that no non-zero product lies within
    the counted bound tau of 0, which is what makes demanding equal counts fair"""
    x = inputs(kind, N, H, W, seed)
    Y = R.grey(x, Hc, Wc)
    flat = R.flat_windows(x, Hc, Wc)
    bound, taus, ps = R.moment_bounds(Y, rh, rw, flat)
    for tau, p in zip(taus, ps):
        nz = p != 0
        assert bool((p.abs()[nz] > tau[nz]).all()), "a bad case: a non-zero product of the reference lies within tau of 0"
        assert bool((tau[~nz] == 0).all()), "a bad case: a zero product of the reference that is not exactly zero everywhere"
    return x, R.moments(Y, rh, rw), bound


def check_moments(got, kind, N, H, W, Hc, Wc, rh, rw, seed=0):
    """got [N,Hc/rh,Wc/rw,24] float64 -> the largest |err| / bound of the sums; the counts must be equal"""
    _, ref, bound = moment_reference(kind, N, H, W, Hc, Wc, rh, rw, seed)
    assert tuple(got.shape) == tuple(ref.shape)
    assert bool((got[..., 23] == 0).all())
    return worst(got, ref, bound)


@functools.lru_cache(maxsize=None)
def halve_reference(kind, N, H, W, Hc, Wc, seed=0):
    x = inputs(kind, N, H, W, seed)
    Y = R.grey(x, Hc, Wc)
    return x, Y, R.halve(Y), R.halve_bound(Y)


def check_features(got, kernel_moments, ref_moments, bound, n):
    """got [...,18] features from the kernel's moments (any leading shape, CPU float64), against the reference fit
      - of the kernel's own moments: every alpha exactly equal, the other features to 1e-12 relative (the lgamma of two
        libraries under the mean's factor, a dozen roundings)
      - of the reference's moments: the variances within the moment bound divided by their count; an alpha equal, or one grid
        step (0.001) off only where the reference's ratio lies within its first-order moment bound of a decision point (the
        fit of ratio - delta and of ratio + delta differ), which at most one feature per case may do; a mean, where its alpha is
        equal, within factor (d sr + d sl) + 1e-12 |mean|.
    Returns the number of alphas that sit on a decision point."""
    own = R.fit_features(kernel_moments, n)
    assert bool((torch.isnan(got) == torch.isnan(own)).all())
    ok = ~torch.isnan(own)
    for c in R.ALPHA_COLUMNS:
        assert bool((got[..., c][ok[..., c]] == own[..., c][ok[..., c]]).all()), "alpha differs on the kernel's own moments"
    assert float(((got - own).abs()[ok] / own.abs()[ok].clamp_min(1e-300)).max()) <= 1e-12
    ref, m, b = R.fit_features(ref_moments, n), ref_moments, bound
    assert bool((torch.isnan(got) == torch.isnan(ref)).all())
    rel = lambda i: b[..., i] / m[..., i]
    assert bool(((got[..., 1] - ref[..., 1]).abs() <= b[..., 1] / n).all())
    on_edge = 0

    def alphas(col, ratio, delta, fit):
        nonlocal on_edge
        diff = (got[..., col] != ref[..., col]) & ~torch.isnan(ref[..., col])
        if bool(diff.any()):
            assert bool(((got[..., col] - ref[..., col]).abs()[diff] <= 0.001 + 1e-12).all()), "alpha more than one grid step off"
            assert bool((fit(ratio - delta)[diff] != fit(ratio + delta)[diff]).all()), "alpha differs away from a decision point"
            on_edge += int(diff.sum())
        return ~diff
    rho = R.ggd_ratio(m, n)
    alphas(0, rho, 2 * rho * (rel(1) + 2 * rel(0)), R.ggd_alpha)
    for k in range(4):
        c, s = 2 + 4 * k, 3 + 5 * k
        Rr, sl, sr = R.aggd_ratio(m, n, k)
        # R = rhat f(gh): rhat carries 2 rel(sum|p|) + rel(S- + S+), gh = sl / sr half of rel(S-) + rel(S+), and |gh f' / f| <= 4
        d_rhat = 2 * rel(s + 4) + (b[..., s + 1] + b[..., s + 3]) / (m[..., s + 1] + m[..., s + 3])
        same = alphas(c, Rr, 2 * Rr * (d_rhat + 4 * 0.5 * (rel(s + 1) + rel(s + 3))), R.aggd_alpha)
        for col, i, cnt in ((c + 2, s + 1, s), (c + 3, s + 3, s + 2)):
            fin = ~torch.isnan(ref[..., col])
            assert bool(((got[..., col] - ref[..., col]).abs()[fin] <= (b[..., i] / m[..., cnt])[fin]).all())
        dsl, dsr = b[..., s + 1] / m[..., s] / (2 * sl), b[..., s + 3] / m[..., s + 2] / (2 * sr)
        chk = same & ~torch.isnan(ref[..., c + 1])
        mb = R.mean_factor(ref[..., c]) * (dsl + dsr) + 1e-12 * ref[..., c + 1].abs()
        assert bool(((got[..., c + 1] - ref[..., c + 1]).abs()[chk] <= mb[chk]).all())
    assert on_edge <= 1, f"{on_edge} alphas of one case sit on a decision point: choose another seed"
    return on_edge
