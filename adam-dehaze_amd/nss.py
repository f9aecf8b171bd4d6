"""No-reference image quality on the natural-scene-statistics kernels of csrc/nss.hip: the 36 BRISQUE features
(Mittal, Moorthy, Bovik 2012), the per-patch features of NIQE (Mittal, Soundararajan, Bovik 2013), a NIQE model fitted from the
user's own clean images, the NIQE distance, and the BRISQUE score through a libsvm epsilon-SVR model file the user supplies (none
is shipped).  Not in the reference, which scores against ground truth only.

The kernels return 24 float64 sums per region (`nss_moments`); `fit_features` turns them into the 18 features of a scale with a
few float64 torch operations on the device (a `searchsorted` on the table r(gamma) plus a two-neighbour compare), as the MS-SSIM
combining step does.  Nothing is read back before the features exist; NIQE then reads `[n,P,36]` back once per chunk and
finishes with `numpy.linalg.pinv` on the host.  No CPU fallback and no gradient."""
from __future__ import annotations

import math
import os
import warnings
from typing import Dict, Iterable, List, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from . import _hip as H

PATCH = 96                                   # NIQE's patch side; 48 at the second scale
TILE_H, TILE_W = 16, 32                      # csrc/nss.hip: the tile a workgroup owns (include/adam_dehaze_hip.h names them)
MODEL_VERSION = 1

GAMMA_GRID = torch.arange(200, 10001, dtype=torch.float64) / 1000.0      # 0.2, 0.201, ..., 10: 9801 points


def _lgamma_table(fn) -> torch.Tensor:
    return torch.tensor([fn(g) for g in GAMMA_GRID.tolist()], dtype=torch.float64)


# r(gamma) = Gamma(2/gamma)^2 / (Gamma(1/gamma) Gamma(3/gamma)), strictly increasing; and the factor of the AGGD mean,
# Gamma(2/gamma) / sqrt(Gamma(1/gamma) Gamma(3/gamma)); both through lgamma in float64, once, on the host
GAMMA_TABLE = _lgamma_table(lambda g: math.exp(2.0 * math.lgamma(2.0 / g) - math.lgamma(1.0 / g) - math.lgamma(3.0 / g)))
MEAN_FACTOR_TABLE = _lgamma_table(lambda g: math.exp(math.lgamma(2.0 / g) - 0.5 * (math.lgamma(1.0 / g) + math.lgamma(3.0 / g))))
_tables: Dict[str, Tuple[torch.Tensor, ...]] = {}


def _device_tables(device) -> Tuple[torch.Tensor, ...]:
    key = str(device)
    if key not in _tables:
        # 1 / r is decreasing: flipped it is a sorted table too
        _tables[key] = tuple(t.to(device) for t in (GAMMA_GRID, GAMMA_TABLE, (1.0 / GAMMA_TABLE).flip(0), MEAN_FACTOR_TABLE))
    return _tables[key]


def _nearest(table: torch.Tensor, x: torch.Tensor, squared: bool, prefer_upper: bool) -> torch.Tensor:
    """index into the increasing `table` of the entry nearest to x (|.| or (.)^2 as the definition writes the cost); of two
    equally near neighbours the upper one with `prefer_upper`, else the lower.  NaN gives an arbitrary index: callers mask."""
    K = table.numel()
    hi = torch.searchsorted(table, x.contiguous()).clamp(1, K - 1)
    lo = hi - 1
    a, b = table[lo] - x, table[hi] - x
    ca, cb = (a * a, b * b) if squared else (a.abs(), b.abs())
    return torch.where(cb <= ca, hi, lo) if prefer_upper else torch.where(ca <= cb, lo, hi)


def fit_features(moments: torch.Tensor, n: int) -> torch.Tensor:
    """[...,24] float64 region sums of `nss_moments` (any device) -> [...,18] features of one scale, n = rh * rw pixels per
    region: the GGD shape and variance of the MSCN coefficients, then for each of the four neighbour directions the AGGD shape,
    mean, left and right variance.  Empty sets (n- = 0, n+ = 0, sum|M| = 0) give NaN: the defined result."""
    if moments.dtype != torch.float64 or moments.shape[-1] != 24:
        raise ValueError(f"fit_features takes float64 [...,24] moments, got {moments.dtype} {tuple(moments.shape)}")
    grid, r, inv_flipped, mean_factor = _device_tables(moments.device)
    K = grid.numel()
    nan = torch.full_like(moments[..., 0], float("nan"))
    n = float(n)
    rho = (moments[..., 1] / n) / (moments[..., 0] / n) ** 2
    # lowest index on ties = the upper neighbour of the flipped table
    idx = K - 1 - _nearest(inv_flipped, rho, squared=False, prefer_upper=True)
    feats = [torch.where(torch.isnan(rho), nan, grid[idx]), moments[..., 1] / n]
    d = moments[..., 3:23].reshape(*moments.shape[:-1], 4, 5)      # the four directions at once: n-, S-, n+, S+, sum|p|
    sl, sr = (d[..., 1] / d[..., 0]).sqrt(), (d[..., 3] / d[..., 2]).sqrt()
    gh = sl / sr
    rhat = (d[..., 4] / n) ** 2 / ((d[..., 1] + d[..., 3]) / n)
    R = rhat * (gh ** 3 + 1) * (gh + 1) / (gh ** 2 + 1) ** 2
    idx = _nearest(r, R, squared=True, prefer_upper=False)
    bad = torch.isnan(R)
    nan4 = nan.unsqueeze(-1).expand_as(R)
    aggd = torch.stack([torch.where(bad, nan4, grid[idx]), torch.where(bad, nan4, (sr - sl) * mean_factor[idx]), sl * sl, sr * sr], -1)
    return torch.cat([torch.stack(feats, -1), aggd.flatten(-2)], -1)


# ---------------------------------------------------------------------------------------------------------------- kernels
def _check_batch(x: torch.Tensor, what: str) -> torch.Tensor:
    H.require_cuda(x, what)
    if x.dim() != 4 or x.shape[1] != 3:
        raise RuntimeError(f"expected an [N,3,H,W] batch, got {tuple(x.shape)}")
    return x.contiguous()


def _plane(src: torch.Tensor) -> Tuple[int, int, int, int]:
    """(src_rgb, N, H, W) of an fp32 [N,3,H,W] batch or a float64 [N,H,W] grey plane on the device"""
    if not src.is_cuda or not src.is_contiguous():
        raise RuntimeError("the natural-scene-statistics kernels take dense device tensors (no CPU fallback)")
    if src.dtype == torch.float32 and src.dim() == 4 and src.shape[1] == 3:
        return 1, src.shape[0], src.shape[2], src.shape[3]
    if src.dtype == torch.float64 and src.dim() == 3:
        return 0, src.shape[0], src.shape[1], src.shape[2]
    raise RuntimeError(f"expected fp32 [N,3,H,W] or float64 [N,H,W], got {src.dtype} {tuple(src.shape)}")


def nss_halve(src: torch.Tensor, Hc: Optional[int] = None, Wc: Optional[int] = None) -> torch.Tensor:
    """The second scale: the top-left Hc x Wc crop of the grey plane halved by the antialiased bicubic -> float64
    [N, ceil(Hc/2), ceil(Wc/2)] (adh_nss_halve)."""
    rgb, N, Hh, Ww = _plane(src)
    Hc, Wc = Hc or Hh, Wc or Ww
    dst = torch.empty((N, (Hc + 1) // 2, (Wc + 1) // 2), device=src.device, dtype=torch.float64)
    H.call("adh_nss_halve", src.data_ptr(), rgb, N, Hh, Ww, Hc, Wc, dst.data_ptr())
    return dst


def nss_moments(src: torch.Tensor, rh: int, rw: int, Hc: Optional[int] = None, Wc: Optional[int] = None) -> torch.Tensor:
    """The 24 sums of every rh x rw region of the top-left Hc x Wc crop -> float64 [N, Hc/rh, Wc/rw, 24] (adh_nss_moments)."""
    rgb, N, Hh, Ww = _plane(src)
    Hc, Wc = Hc or Hh, Wc or Ww
    if rh < 1 or rw < 1 or Hc % rh or Wc % rw:
        raise ValueError(f"{rh}x{rw} regions do not tile a {Hc}x{Wc} plane")
    ntiles = -(-rh // TILE_H) * -(-rw // TILE_W)
    ry, rx = Hc // rh, Wc // rw
    partial = torch.empty(N * ry * rx * ntiles * 24, device=src.device, dtype=torch.float64)
    out = torch.empty((N, ry, rx, 24), device=src.device, dtype=torch.float64)
    H.call("adh_nss_moments", src.data_ptr(), rgb, N, Hh, Ww, Hc, Wc, rh, rw, partial.data_ptr(), ntiles, out.data_ptr())
    return out


def brisque_features(x: torch.Tensor) -> torch.Tensor:
    """fp32 [N,3,H,W] in [0,1] -> the 36 BRISQUE features [N,36] (float64, on the device): the 18 of `fit_features` over the
    whole grey plane, then over the halved plane."""
    x = _check_batch(x, "images")
    N, _, Hh, Ww = x.shape
    y2 = nss_halve(x)
    f1 = fit_features(nss_moments(x, Hh, Ww), Hh * Ww)
    f2 = fit_features(nss_moments(y2, y2.shape[1], y2.shape[2]), y2.shape[1] * y2.shape[2])
    return torch.cat([f1.view(N, 18), f2.view(N, 18)], 1)


def niqe_patch_features(x: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """fp32 [N,3,H,W] in [0,1], both sides at least 96 -> ([N,P,36] patch features, [N,P] patch sharpness), float64 on the device:
    the top-left 96 floor(H/96) x 96 floor(W/96) crop in 96 x 96 patches, their 18 features, the 18 of the matching 48 x 48
    regions of the halved crop, and the mean local deviation s of the patch at the first scale."""
    x = _check_batch(x, "images")
    N, _, Hh, Ww = x.shape
    if Hh < PATCH or Ww < PATCH:
        raise ValueError(f"NIQE needs images of at least {PATCH}x{PATCH}, got {Hh}x{Ww}")
    Hc, Wc = PATCH * (Hh // PATCH), PATCH * (Ww // PATCH)
    m1 = nss_moments(x, PATCH, PATCH, Hc, Wc)
    m2 = nss_moments(nss_halve(x, Hc, Wc), PATCH // 2, PATCH // 2)
    f = torch.cat([fit_features(m1, PATCH * PATCH), fit_features(m2, PATCH * PATCH // 4)], -1)
    return f.view(N, -1, 36), (m1[..., 2] / float(PATCH * PATCH)).view(N, -1)


# ---------------------------------------------------------------------------------------------------------------- NIQE
def niqe_distance(mu, cov, feats) -> Optional[float]:
    """The NIQE score of one image from its [P,36] patch features: rows with a non-finite entry are dropped; mu_d and cov_d
    (N-1) of the rest; sqrt(delta^T pinv((cov + cov_d) / 2) delta), delta = mu - mu_d, in float64 on the host.  None with fewer
    than two finite rows."""
    f = np.asarray(feats, dtype=np.float64)
    f = f[np.isfinite(f).all(1)]
    if f.shape[0] < 2:
        return None
    mu_d = f.mean(0)
    c = f - mu_d
    cov_d = c.T @ c / (f.shape[0] - 1)
    delta = np.asarray(mu, dtype=np.float64) - mu_d
    q = float(delta @ np.linalg.pinv((np.asarray(cov, dtype=np.float64) + cov_d) / 2.0) @ delta)
    return math.sqrt(max(q, 0.0))


class NiqeModel:
    """NIQE's "pristine model": the mean `mu` [36] and covariance `cov` [36,36] of the features of sharp patches of clean
    images, and `meta` (patch_size, images, patches, sharpness_threshold, version)."""

    def __init__(self, mu, cov, meta: Optional[Dict] = None):
        self.mu = np.asarray(mu, dtype=np.float64)
        self.cov = np.asarray(cov, dtype=np.float64)
        if self.mu.shape != (36,) or self.cov.shape != (36, 36):
            raise ValueError(f"a NIQE model holds mu [36] and cov [36,36], got {self.mu.shape} and {self.cov.shape}")
        self.meta = dict(meta or {})

    @classmethod
    def fit(cls, batches_or_paths: Iterable[Union[torch.Tensor, str]], sharpness_threshold: float = 0.75,
            batch_size: int = 4, device="cuda") -> "NiqeModel":
        """From fp32 [N,3,H,W] device batches, or from image file paths (grouped by size through image_io.plan_chunks, `batch_size`
        at a time; files under 96 px on a side are skipped with a warning).  Of every image the patches whose sharpness exceeds
        `sharpness_threshold` times that image's maximum are kept, rows with a non-finite entry dropped."""
        items = list(batches_or_paths)
        if items and all(isinstance(i, (str, os.PathLike)) for i in items):
            batches = _file_batches([str(i) for i in items], batch_size, device)
        else:
            batches = iter(items)
        rows, images = [], 0
        for x in batches:
            f, sh = niqe_patch_features(x)
            host = torch.cat([f, sh.unsqueeze(-1)], -1).cpu().numpy()           # one read-back per chunk
            for img in host:
                feats, sharp = img[:, :36], img[:, 36]
                keep = feats[sharp > sharpness_threshold * sharp.max()]
                rows.append(keep[np.isfinite(keep).all(1)])
                images += 1
        rows = np.concatenate(rows) if rows else np.zeros((0, 36))
        if rows.shape[0] < 2:
            raise ValueError(f"a NIQE model needs at least two sharp {PATCH}x{PATCH} patches with finite features, got "
                             f"{rows.shape[0]} from {images} image(s)")
        mu = rows.mean(0)
        c = rows - mu
        return cls(mu, c.T @ c / (rows.shape[0] - 1),
                   {"patch_size": PATCH, "images": images, "patches": int(rows.shape[0]),
                    "sharpness_threshold": float(sharpness_threshold), "version": MODEL_VERSION})

    def save(self, path: str) -> None:
        m = self.meta
        with open(path, "wb") as f:                        # a file object: numpy appends no extension
            np.savez(f, mu=self.mu, cov=self.cov, patch_size=np.int64(m.get("patch_size", PATCH)),
                     images=np.int64(m.get("images", 0)), patches=np.int64(m.get("patches", 0)),
                     sharpness_threshold=np.float64(m.get("sharpness_threshold", 0.75)),
                     version=np.int64(m.get("version", MODEL_VERSION)))

    @classmethod
    def load(cls, path: str) -> "NiqeModel":
        with np.load(path, allow_pickle=False) as z:
            missing = sorted({"mu", "cov", "patch_size", "version"} - set(z.files))
            if missing:
                raise ValueError(f"{path}: not a NIQE model file (no {', '.join(missing)})")
            meta = {k: (float(z[k]) if k == "sharpness_threshold" else int(z[k])) for k in z.files if k not in ("mu", "cov")}
            if meta["version"] != MODEL_VERSION or meta["patch_size"] != PATCH:
                raise ValueError(f"{path}: NIQE model version {meta['version']} with patch size {meta['patch_size']}; this build "
                                 f"reads version {MODEL_VERSION} with patch size {PATCH}")
            return cls(z["mu"], z["cov"], meta)


def _file_batches(paths: Sequence[str], batch_size: int, device):
    from . import image_io as IO
    sizes = {}
    for p in paths:
        hw = IO.image_size(p)
        if min(hw) < PATCH:
            warnings.warn(f"{p}: {hw[0]}x{hw[1]} is smaller than {PATCH} pixels on a side; skipped")
            continue
        sizes[p] = hw
    for chunk in IO.plan_chunks(sizes, batch_size):
        yield IO.u8_to_image(IO._stack([IO.load_image(p) for p in chunk]).to(device))


def niqe_batch(x: torch.Tensor, model: NiqeModel) -> List[Optional[float]]:
    """NIQE of every image of an fp32 [N,3,H,W] batch against `model` (lower is better): a list of floats, None for images
    under 96 px on a side or with fewer than two patches of finite features.  One read-back."""
    x = _check_batch(x, "images")
    if x.shape[2] < PATCH or x.shape[3] < PATCH:
        return [None] * x.shape[0]
    feats = niqe_patch_features(x)[0].cpu().numpy()
    return [niqe_distance(model.mu, model.cov, f) for f in feats]


# ---------------------------------------------------------------------------------------------------------------- BRISQUE
class SvrModel:
    """A libsvm epsilon-SVR model with an RBF kernel, as the BRISQUE release ships its `allmodel`, and optionally the svm-scale
    range file (`allrange`) its features are scaled with.  score = sum_i coef_i exp(-gamma |x' - sv_i|^2) - rho."""

    def __init__(self, gamma: float, rho: float, coef, sv, lower: float = -1.0, upper: float = 1.0, ranges=None):
        self.gamma, self.rho = float(gamma), float(rho)
        self.coef = np.asarray(coef, dtype=np.float64)
        self.sv = np.asarray(sv, dtype=np.float64)
        if self.sv.ndim != 2 or self.sv.shape != (self.coef.shape[0], 36):
            raise ValueError(f"support vectors must be [{self.coef.shape[0]},36], got {self.sv.shape}")
        self.lower, self.upper = float(lower), float(upper)
        self.ranges = None if ranges is None else np.asarray(ranges, dtype=np.float64)      # [36,2] min, max; NaN = unscaled

    @classmethod
    def load(cls, model_path: str, range_path: Optional[str] = None) -> "SvrModel":
        head: Dict[str, str] = {}
        coef, rows = [], []
        with open(model_path) as f:
            lines = [ln.strip() for ln in f if ln.strip()]
        at = 0
        while at < len(lines) and lines[at] != "SV":
            k, _, v = lines[at].partition(" ")
            head[k] = v.strip()
            at += 1
        if at == len(lines):
            raise ValueError(f"{model_path}: not a libsvm model file (no SV section)")
        if head.get("svm_type") != "epsilon_svr" or head.get("kernel_type") != "rbf":
            raise ValueError(f"{model_path}: BRISQUE needs an epsilon_svr model with an rbf kernel, found svm_type "
                             f"{head.get('svm_type')!r} with kernel_type {head.get('kernel_type')!r}")
        for key in ("gamma", "rho"):
            if key not in head:
                raise ValueError(f"{model_path}: no {key} in the model's header")
        for ln in lines[at + 1:]:
            parts = ln.split()
            coef.append(float(parts[0]))
            row = np.zeros(36)
            for item in parts[1:]:
                i, _, v = item.partition(":")
                if not 1 <= int(i) <= 36:
                    raise ValueError(f"{model_path}: feature index {i} outside 1..36")
                row[int(i) - 1] = float(v)
            rows.append(row)
        if "total_sv" in head and int(head["total_sv"]) != len(rows):
            raise ValueError(f"{model_path}: total_sv {head['total_sv']} but {len(rows)} support vectors")
        lower, upper, ranges = -1.0, 1.0, None
        if range_path is not None:
            with open(range_path) as f:
                rl = [ln.strip() for ln in f if ln.strip()]
            if not rl or rl[0] != "x":
                raise ValueError(f"{range_path}: an svm-scale range file of the features starts with a line 'x', found "
                                 f"{rl[0] if rl else 'nothing'!r}")
            lower, upper = (float(v) for v in rl[1].split())
            ranges = np.full((36, 2), np.nan)
            for ln in rl[2:]:
                i, lo, hi = ln.split()
                if not 1 <= int(i) <= 36:
                    raise ValueError(f"{range_path}: feature index {i} outside 1..36")
                ranges[int(i) - 1] = (float(lo), float(hi))
        return cls(float(head["gamma"]), float(head["rho"].split()[0]), coef, np.stack(rows) if rows else np.zeros((0, 36)),
                   lower, upper, ranges)

    def scale(self, feats: torch.Tensor) -> torch.Tensor:
        """svm-scale: lower + (upper - lower) (x - min) / (max - min) per listed feature with max > min; others unchanged"""
        if self.ranges is None:
            return feats
        lo = torch.as_tensor(self.ranges[:, 0], device=feats.device)
        hi = torch.as_tensor(self.ranges[:, 1], device=feats.device)
        ok = hi > lo                                             # NaN compares false
        scaled = self.lower + (self.upper - self.lower) * (feats - lo) / (hi - lo)
        return torch.where(ok, scaled, feats)

    def predict(self, feats: torch.Tensor) -> torch.Tensor:
        """[N,36] float64 (any device) -> [N] float64"""
        x = self.scale(feats.double())
        sv = torch.as_tensor(self.sv, device=x.device)
        coef = torch.as_tensor(self.coef, device=x.device)
        d2 = ((x.unsqueeze(1) - sv.unsqueeze(0)) ** 2).sum(-1)
        return (coef * torch.exp(-self.gamma * d2)).sum(-1) - self.rho


def brisque_batch(x: torch.Tensor, svr: SvrModel) -> List[Optional[float]]:
    """BRISQUE of every image of an fp32 [N,3,H,W] batch through `svr` (lower is better): a list of floats, None where a feature
    is not finite (a constant image).  One read-back."""
    vals = svr.predict(brisque_features(x)).cpu().tolist()
    return [v if math.isfinite(v) else None for v in vals]
