"""Float64 reference of the natural-scene statistics behind NIQE and BRISQUE (csrc/nss.hip, adam-dehaze_amd/nss.py):
the definitions restated with torch on the CPU, the brute-force feature fit, the NIQE distance written out, and the count of
roundings the bounds of the tests are stated in.  Every function takes and returns float64 (fp32 inputs are converted exactly).

Grey plane.  Input fp32 [N,3,H,W], nominally in [0,1]; Y = 255 (0.299 R + 0.587 G + 0.114 B) in float64 over the top-left
Hc x Wc crop.
Local statistics, centred on the pixel, so that an exactly flat window gives exact zeros in any summation order:
  g[i] = exp(-(i-3)^2 / (2 sigma^2)), sigma = 7/6, i = 0..6, normalised to sum 1 in float64; w = g (x) g; window positions outside
  the cropped plane take the nearest in-plane pixel (replicate).  For pixel p with window pixels q
    d = sum w_q (Y_q - Y_p),  v = sum w_q (Y_q - Y_p)^2 - d^2,  s = sqrt|v|,  M_p = -d / (s + 1)
  which equals the releases' (Y - w*Y) / (sqrt|w*Y^2 - (w*Y)^2| + 1) up to sum w = 1 (direct_mscn below; the direct form cancels
  against Y^2 ~ 6e4 and leaves order-dependent residue on flat windows).
Second scale.  The grey plane halved by the antialiased bicubic (a = -0.5), the releases' imresize(., 0.5): output size
  ceil(Hc/2) x ceil(Wc/2), output j reads inputs 2j-3 .. 2j+4 with indices clamped to the plane, weights
  [-3, -9, 29, 111, 111, 29, -9, -3] / 256, along W, then along H.
Regions.  An rh x rw block of the cropped plane (Hc % rh == 0, Wc % rw == 0).  M comes from the plane-level statistics, so
  windows cross region borders; neighbour products wrap within the region as circshift does: for direction k the product at
  (i, j) is M(i, j) M((i+di) mod rh, (j+dj) mod rw), (di, dj) = (0,1), (1,0), (1,1), (1,-1).
Per region, 24 values: [0] sum|M|, [1] sum M^2, [2] sum s; for direction k at 3 + 5k: n- (count of products < 0), the sum of
  their p^2, n+ (count > 0), the sum of their p^2, sum|p| over all; [23] = 0.  A product equal to 0 is in neither set.
Features, 18 per scale, from the moments with n = rh rw.  T is the grid gamma = 0.2, 0.201, ..., 10 (9801 points) and
  r(gamma) = Gamma(2/gamma)^2 / (Gamma(1/gamma) Gamma(3/gamma)) through lgamma, strictly increasing.
  GGD: rho = (sum M^2 / n) / (sum|M| / n)^2; alpha = the grid point minimising |rho - 1 / r(gamma)|, lowest index on ties;
    features alpha, sum M^2 / n.
  AGGD per direction: sl = sqrt(S- / n-), sr = sqrt(S+ / n+), gh = sl / sr, rh = (sum|p| / n)^2 / ((S- + S+) / n),
    R = rh (gh^3 + 1)(gh + 1) / (gh^2 + 1)^2; alpha = the grid point minimising (r(gamma) - R)^2, lowest index on ties;
    mean = (sr - sl) Gamma(2/alpha) / sqrt(Gamma(1/alpha) Gamma(3/alpha)); features alpha, mean, sl^2, sr^2.
  With n- = 0, n+ = 0 or sum|M| = 0 the arithmetic gives NaN and the feature is NaN: the defined result.
BRISQUE features [N,36]: region = the whole plane, no crop; scale 1, then scale 2.
NIQE: crop to 96 floor(H/96) x 96 floor(W/96); P patches of 96 x 96; scale 2 = the halved cropped plane with 48 x 48 regions;
  patch vector = 18 + 18 features, patch sharpness = sum s / 96^2 at scale 1.  Model: over a set of images the patches with
  sharpness > t (that image's maximum), t = 0.75, rows with a non-finite entry dropped; mu their mean, cov their covariance
  (N-1).  Score: all the image's patches with finite rows give mu_d, cov_d; sqrt(delta^T pinv((cov + cov_d) / 2) delta),
  delta = mu - mu_d; None when a side is under 96 px or fewer than two finite rows remain."""
import math

import numpy as np
import torch
import torch.nn.functional as F

U53 = 2.0 ** -53
WIN = 7
SIGMA = 7.0 / 6.0
HALVE_TAPS = (-3.0, -9.0, 29.0, 111.0, 111.0, 29.0, -9.0, -3.0)
DIRECTIONS = ((0, 1), (1, 0), (1, 1), (1, -1))
PATCH = 96

# ---- the error budget, in units u = 2^-53.  A = max|Y| over the plane bounds every pixel.
#   the grey expression: three products, two sums and the scaling by 255, six roundings -> |dY| <= GREY_UNITS u A (the fp32 -> float64
#     conversion is exact); a pooled plane's pixel carries its own bound instead
#   t = Y_q - Y_p: both pixels' dY and the subtraction's rounding -> dt <= (2 GREY_UNITS + 1) u A =: E_t.  On a window whose 49
#     inputs are identical every implementation forms 49 identical doubles: t = 0 exactly, and d = v = s = M = 0 with no error at all.
#   a 49-term sum: the weights (exp, a 7-term sum, a division, the outer product: <= 8 u relative, in the kernel and here) and the
#     sum itself (49 fused or unfused multiply-adds, 50 roundings with the product under v) -> SUM_UNITS = 2 * 8 + 50 + 49 = 115 u of the
#     sum of absolute terms, the reference's own 49-term sum included
#     dd <= E_t + SUM_UNITS u sum w|t|;  dv' <= 2 E_t sum w|t| + E_t^2 + SUM_UNITS u sum w t^2;  dv <= dv' + 2|d| dd + dd^2 + 2 u (v' + d^2)
#   one sqrt: |sqrt a - sqrt b| <= min(|a - b| / sqrt a, sqrt|a - b|) -> ds <= min(dv / s, sqrt dv) + 2 u s
#   one division: dM <= dd / (s + 1) + |d| ds / (s + 1)^2 + 4 u |M|
#   a product p = M M': tau = |M| dM' + |M'| dM + dM dM' + 2 u |p|
#   a sum of n terms in any order (the tile tree, the slices, this file's own sum): n u of the sum of absolute terms, twice, plus
#     one fp64 store: (2 n + 2) u
GREY_UNITS = 6.0
SUM_UNITS = 115.0


def gauss():
    i = torch.arange(WIN, dtype=torch.float64)
    g = torch.exp(-((i - WIN // 2) ** 2) / (2.0 * SIGMA ** 2))
    return g / g.sum()


def window():
    g = gauss()
    return g[:, None] * g[None, :]


def grey(x, Hc=None, Wc=None):
    """fp32 (or float64) [N,3,H,W] -> float64 [N,Hc,Wc]"""
    x = x.double()
    Hc, Wc = Hc or x.shape[2], Wc or x.shape[3]
    x = x[:, :, :Hc, :Wc]
    return 255.0 * (0.299 * x[:, 0] + 0.587 * x[:, 1] + 0.114 * x[:, 2])


def _windows(Y):
    """[N,H,W] -> [N,49,H,W]: the 7x7 window of every pixel, replicate padding"""
    N, H, W = Y.shape
    P = F.pad(Y.unsqueeze(1), (3, 3, 3, 3), mode="replicate")
    return F.unfold(P, WIN).view(N, WIN * WIN, H, W)


def local_stats(Y):
    """(d, v, s, M), each [N,H,W], centred form"""
    t = _windows(Y) - Y.unsqueeze(1)
    w = window().reshape(1, -1, 1, 1)
    d = (w * t).sum(1)
    v = (w * t * t).sum(1) - d * d
    s = v.abs().sqrt()
    return d, v, s, -d / (s + 1.0)


def direct_mscn(Y):
    """the releases' form: (Y - mu) / (sqrt|w*Y^2 - mu^2| + 1)"""
    q = _windows(Y)
    w = window().reshape(1, -1, 1, 1)
    mu = (w * q).sum(1)
    return (Y - mu) / (((w * q * q).sum(1) - mu * mu).abs().sqrt() + 1.0)


def halve_axis(Y, dim):
    n = Y.shape[dim]
    out = (n + 1) // 2
    j = torch.arange(out)
    acc = torch.zeros_like(Y.index_select(dim, j))
    for k, t in enumerate(HALVE_TAPS):
        acc = acc + (t / 256.0) * Y.index_select(dim, (2 * j - 3 + k).clamp(0, n - 1))
    return acc


def halve(Y):
    """[N,H,W] -> [N,ceil(H/2),ceil(W/2)]: along W, then along H"""
    return halve_axis(halve_axis(Y, 2), 1)


def halve_bound(Y):
    """|error| bound of a halved plane [N,OH,OW]: 8 + 8 multiply-adds of each pass and one store, of the absolute terms, plus the
    grey expression's GREY_UNITS u A on every tap of a plane formed on the fly (sum of |weights| = 304/256 per pass)"""
    A = float(Y.abs().max()) if Y.numel() else 0.0
    absw = sum(abs(t) for t in HALVE_TAPS) / 256.0
    mag = Y.abs()
    for dim in (2, 1):
        n = mag.shape[dim]
        j = torch.arange((n + 1) // 2)
        acc = torch.zeros_like(mag.index_select(dim, j))
        for k, t in enumerate(HALVE_TAPS):
            acc = acc + (abs(t) / 256.0) * mag.index_select(dim, (2 * j - 3 + k).clamp(0, n - 1))
        mag = acc
    return (2 * (16 + 1) + 2) * U53 * mag + 2 * GREY_UNITS * U53 * A * absw * absw


def _regions(Z, rh, rw):
    """[N,H,W] -> [N,H/rh,W/rw,rh,rw]"""
    N, H, W = Z.shape
    return Z.view(N, H // rh, rh, W // rw, rw).permute(0, 1, 3, 2, 4)


def products(M, rh, rw):
    """[4][N,ry,rx,rh,rw]: the four torus-neighbour products inside every region"""
    R = _regions(M, rh, rw)
    return [R * torch.roll(R, shifts=(-di, -dj), dims=(3, 4)) for di, dj in DIRECTIONS]


def moments(Y, rh, rw):
    """[N,H/rh,W/rw,24]"""
    _, _, s, M = local_stats(Y)
    Rm, Rs = _regions(M, rh, rw), _regions(s, rh, rw)
    out = [Rm.abs().sum((3, 4)), (Rm * Rm).sum((3, 4)), Rs.sum((3, 4))]
    for p in products(M, rh, rw):
        neg, pos = p < 0, p > 0
        out += [neg.double().sum((3, 4)), (p * p * neg).sum((3, 4)), pos.double().sum((3, 4)), (p * p * pos).sum((3, 4)),
                p.abs().sum((3, 4))]
    out.append(torch.zeros_like(out[0]))
    return torch.stack(out, -1)


def flat_windows(x_or_Y, Hc=None, Wc=None):
    """[N,H,W] bool: every pixel of the 7x7 window (replicate) has the centre's input values, so every implementation computes
    exact zeros there.  x_or_Y: the fp32 [N,3,H,W] input of a plane formed on the fly, or a float64 [N,H,W] plane."""
    Z = x_or_Y.double()
    if Z.dim() == 3:
        Z = Z.unsqueeze(1)
    Z = Z[:, :, :Hc or Z.shape[2], :Wc or Z.shape[3]]
    P = F.pad(Z, (3, 3, 3, 3), mode="replicate")
    hi, lo = F.max_pool2d(P, WIN, 1), -F.max_pool2d(-P, WIN, 1)
    return (hi == lo).all(1)


def pixel_bounds(Y, flat, dY=None):
    """(ds, dM) [N,H,W]: the per-pixel error bounds of the budget above; exactly 0 on flat windows.  dY: the bound on a pixel's
    own error where the plane is not the grey expression of exact inputs (a halved plane: halve_bound)."""
    A = float(Y.abs().max())
    Et = (2 * GREY_UNITS + 1) * U53 * A if dY is None else 2 * float(dY.max()) + U53 * A
    t = _windows(Y) - Y.unsqueeze(1)
    w = window().reshape(1, -1, 1, 1)
    d = (w * t).sum(1)
    D1, V1 = (w * t.abs()).sum(1), (w * t * t).sum(1)
    v = V1 - d * d
    s = v.abs().sqrt()
    M = -d / (s + 1.0)
    dd = Et + SUM_UNITS * U53 * D1
    dv = 2 * Et * D1 + Et * Et + SUM_UNITS * U53 * V1 + 2 * d.abs() * dd + dd * dd + 2 * U53 * (V1 + d * d)
    ds = torch.minimum(dv / s.clamp_min(1e-300), dv.sqrt()) + 2 * U53 * s
    dM = dd / (s + 1.0) + d.abs() * ds / (s + 1.0) ** 2 + 4 * U53 * M.abs()
    zero = torch.zeros_like(ds)
    return torch.where(flat, zero, ds), torch.where(flat, zero, dM)


def moment_bounds(Y, rh, rw, flat, dY=None):
    """(bound [N,ry,rx,24] on the sums -- 0 for the counts, which must be equal --, tau [4][N,ry,rx,rh,rw] on the products, the
    products themselves): the test asserts on the reference that no non-zero product lies within tau of 0"""
    _, _, s, M = local_stats(Y)
    ds, dM = pixel_bounds(Y, flat, dY)
    n = rh * rw
    su = (2 * n + 2) * U53
    Rm, Rs, Rdm, Rds = (_regions(z, rh, rw) for z in (M, s, dM, ds))
    out = [Rdm.sum((3, 4)) + su * Rm.abs().sum((3, 4)),
           (2 * Rm.abs() * Rdm + Rdm * Rdm + 2 * U53 * Rm * Rm).sum((3, 4)) + su * (Rm * Rm).sum((3, 4)),
           Rds.sum((3, 4)) + su * Rs.sum((3, 4))]
    taus, ps = [], products(M, rh, rw)
    for (di, dj), p in zip(DIRECTIONS, ps):
        Rn, Rdn = torch.roll(Rm, (-di, -dj), (3, 4)), torch.roll(Rdm, (-di, -dj), (3, 4))
        tau = Rm.abs() * Rdn + Rn.abs() * Rdm + Rdm * Rdn + 2 * U53 * p.abs()
        taus.append(tau)
        dp2 = 2 * p.abs() * tau + tau * tau + 2 * U53 * p * p
        neg, pos = p < 0, p > 0
        z = torch.zeros_like(out[0])
        out += [z, (dp2 * neg).sum((3, 4)) + su * (p * p * neg).sum((3, 4)), z,
                (dp2 * pos).sum((3, 4)) + su * (p * p * pos).sum((3, 4)), tau.sum((3, 4)) + su * p.abs().sum((3, 4))]
    out.append(torch.zeros_like(out[0]))
    return torch.stack(out, -1), taus, ps


# ---------------------------------------------------------------------------------------------------------------- features
def gamma_grid():
    return torch.arange(200, 10001, dtype=torch.float64) / 1000.0


def r_table():
    g = gamma_grid()
    return torch.exp(2 * torch.lgamma(2 / g) - torch.lgamma(1 / g) - torch.lgamma(3 / g))


def mean_factor(alpha):
    return torch.exp(torch.lgamma(2 / alpha) - 0.5 * (torch.lgamma(1 / alpha) + torch.lgamma(3 / alpha)))


def ggd_ratio(mom, n):
    return (mom[..., 1] / n) / (mom[..., 0] / n) ** 2


def aggd_ratio(mom, n, k):
    b = 3 + 5 * k
    sl, sr = (mom[..., b + 1] / mom[..., b]).sqrt(), (mom[..., b + 3] / mom[..., b + 2]).sqrt()
    gh = sl / sr
    rhat = (mom[..., b + 4] / n) ** 2 / ((mom[..., b + 1] + mom[..., b + 3]) / n)
    return rhat * (gh ** 3 + 1) * (gh + 1) / (gh ** 2 + 1) ** 2, sl, sr


def _argmin_first(cost):
    """index of the first minimum along the last dimension; rows with a NaN give -1"""
    idx = torch.argmin(torch.where(torch.isnan(cost), torch.full_like(cost, float("inf")), cost), -1)
    first = (cost == cost.gather(-1, idx.unsqueeze(-1))).double().argmax(-1)      # argmax returns the first maximum
    return torch.where(torch.isnan(cost).any(-1), torch.full_like(first, -1), first)


def _pick(idx):
    nan = torch.full(idx.shape, float("nan"), dtype=torch.float64)
    return torch.where(idx >= 0, gamma_grid()[idx.clamp_min(0)], nan)


def ggd_alpha(rho):
    """the grid point minimising |rho - 1 / r(gamma)|, lowest index on ties, by brute force; NaN for NaN"""
    return _pick(_argmin_first((rho.unsqueeze(-1) - 1.0 / r_table()).abs()))


def aggd_alpha(R):
    """the grid point minimising (r(gamma) - R)^2, lowest index on ties, by brute force; NaN for NaN"""
    return _pick(_argmin_first((r_table() - R.unsqueeze(-1)) ** 2))


def fit_features(mom, n):
    """[...,24] -> [...,18] by a brute-force argmin over the whole grid"""
    feats = [ggd_alpha(ggd_ratio(mom, n)), mom[..., 1] / n]
    for k in range(4):
        R, sl, sr = aggd_ratio(mom, n, k)
        alpha = aggd_alpha(R)
        feats += [alpha, (sr - sl) * mean_factor(alpha), sl * sl, sr * sr]
    return torch.stack(feats, -1)


ALPHA_COLUMNS = (0, 2, 6, 10, 14)


def brisque_features(x):
    """fp32 [N,3,H,W] -> [N,36]"""
    N, _, H, W = x.shape
    Y = grey(x)
    Y2 = halve(Y)
    f1 = fit_features(moments(Y, H, W), H * W).view(N, 18)
    f2 = fit_features(moments(Y2, Y2.shape[1], Y2.shape[2]), Y2.shape[1] * Y2.shape[2]).view(N, 18)
    return torch.cat([f1, f2], 1)


def niqe_patch_features(x):
    """fp32 [N,3,H,W] -> ([N,P,36], sharpness [N,P]); needs both sides >= 96"""
    N, _, H, W = x.shape
    Hc, Wc = PATCH * (H // PATCH), PATCH * (W // PATCH)
    Y = grey(x, Hc, Wc)
    m1 = moments(Y, PATCH, PATCH)
    m2 = moments(halve(Y), PATCH // 2, PATCH // 2)
    f = torch.cat([fit_features(m1, PATCH * PATCH), fit_features(m2, PATCH * PATCH // 4)], -1)
    return f.view(N, -1, 36), (m1[..., 2] / (PATCH * PATCH)).view(N, -1)


def niqe_distance(mu, cov, feats):
    """the score of one image from its [P,36] patch features, written out with numpy; None with fewer than two finite rows"""
    f = np.asarray(feats, dtype=np.float64)
    f = f[np.isfinite(f).all(1)]
    if f.shape[0] < 2:
        return None
    mu_d = f.mean(0)
    c = f - mu_d
    cov_d = c.T @ c / (f.shape[0] - 1)
    delta = np.asarray(mu, dtype=np.float64) - mu_d
    return float(math.sqrt(max(float(delta @ np.linalg.pinv((np.asarray(cov, dtype=np.float64) + cov_d) / 2.0) @ delta), 0.0)))


def niqe_model(feature_sets, sharpness_sets, t=0.75):
    """(mu, cov, rows kept) over per-image ([P,36], [P]) pairs"""
    rows = []
    for f, sh in zip(feature_sets, sharpness_sets):
        f, sh = np.asarray(f, dtype=np.float64), np.asarray(sh, dtype=np.float64)
        keep = f[sh > t * sh.max()]
        rows.append(keep[np.isfinite(keep).all(1)])
    rows = np.concatenate(rows)
    mu = rows.mean(0)
    c = rows - mu
    return mu, c.T @ c / (rows.shape[0] - 1), rows.shape[0]
