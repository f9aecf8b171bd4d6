"""Evaluation harness on device: per-image PSNR / SSIM / LPIPS for NCHW batches without per-image D2H copies.

Mirrors /root/reference evaluation/metrics.py:13-124 (`calculate_image_metrics`, `ImageQualityMetrics` with the same
method names and results-JSON schema) and the validation loops of training/train_joint.py:187-229 and
training/train_dehazing.py:110-166.  The reference copies every image to the host and calls skimage
(`peak_signal_noise_ratio(target, pred, data_range=1.0)`; `structural_similarity` on the channel-mean grayscale with
its defaults) -- here both are HIP reduction kernels over the whole batch (csrc/train_io.hip), LPIPS goes through the
LPIPS-alex kernels of the perceptual loss, and values stay on the device until `compute_averages()` reads them once.
"""
from __future__ import annotations

import json
import os
from collections import defaultdict
from typing import Dict, List, Optional, Sequence

import torch

from . import _hip as H
from .detection_metrics import DetectionMetrics   # noqa: F401  (evaluation/metrics.py:126-270)
from .nss import brisque_batch, niqe_batch         # noqa: F401  (the no-reference scores)

CATEGORY_BY_LABEL = {0: "low_intensity", 1: "medium_intensity", 2: "high_intensity"}   # evaluate.py:160-166


def _check_pair(pred: torch.Tensor, target: torch.Tensor):
    H.require_cuda(pred, "predicted images")
    H.require_cuda(target, "target images")
    if pred.dim() != 4 or pred.shape[1] != 3 or pred.shape != target.shape:
        raise RuntimeError(f"expected two [N,3,H,W] batches, got {tuple(pred.shape)} and {tuple(target.shape)}")
    return pred.contiguous(), target.contiguous()


def psnr_batch(pred: torch.Tensor, target: torch.Tensor, data_range: float = 1.0) -> torch.Tensor:
    """Per-image PSNR [N] (device tensor): 10 log10(R^2 / mean((t-p)^2)), mean in float64 (metrics.py:27)."""
    pred, target = _check_pair(pred, target)
    N = pred.shape[0]
    per = pred[0].numel()
    nblk = H.value("adh_psnr_num_blocks", per)
    partial = torch.empty(N * nblk, device=pred.device, dtype=torch.float64)
    out = torch.empty(N, device=pred.device, dtype=torch.float32)
    H.call("adh_psnr", pred.data_ptr(), target.data_ptr(), N, per, float(data_range), partial.data_ptr(), nblk, None,
           out.data_ptr())
    return out


def ssim_batch(pred: torch.Tensor, target: torch.Tensor, data_range: float = 1.0) -> torch.Tensor:
    """Per-image SSIM [N] of the channel-mean grayscale images with skimage's defaults (metrics.py:29-32)."""
    pred, target = _check_pair(pred, target)
    N, _, Hh, Ww = pred.shape
    if Hh < 7 or Ww < 7:
        raise ValueError("win_size exceeds image extent (images must be at least 7x7)")   # skimage's message
    nblk = H.value("adh_ssim_num_blocks", Hh, Ww)
    partial = torch.empty(N * nblk, device=pred.device, dtype=torch.float64)
    out = torch.empty(N, device=pred.device, dtype=torch.float32)
    H.call("adh_ssim_gray", pred.data_ptr(), target.data_ptr(), N, Hh, Ww, float(data_range), partial.data_ptr(), nblk,
           out.data_ptr())
    return out


def ciede2000_batch(pred: torch.Tensor, target: torch.Tensor, lab_input: bool = False, return_map: bool = False):
    """Per-image mean CIEDE2000 colour difference [N] (device tensor) between two sRGB [0,1] batches -- or, with `lab_input`,
    two batches whose planes are L, a, b -- on the float64 kernel of csrc/ciede2000.hip.  With `return_map` also
    the per-pixel dE00 [N,H,W].  Not in the reference, which has no colour metric; no gradient."""
    pred, target = _check_pair(pred, target)
    N, _, Hh, Ww = pred.shape
    nblk = H.value("adh_ciede2000_num_blocks", Hh * Ww)
    partial = torch.empty(N * nblk, device=pred.device, dtype=torch.float64)
    out = torch.empty(N, device=pred.device, dtype=torch.float32)
    dmap = torch.empty((N, Hh, Ww), device=pred.device, dtype=torch.float32) if return_map else None
    H.call("adh_ciede2000", pred.data_ptr(), target.data_ptr(), N, Hh, Ww, 1 if lab_input else 0, partial.data_ptr(), nblk,
           H.ptr(dmap), out.data_ptr())
    return (out, dmap) if return_map else out


MS_SSIM_WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)      # Wang, Simoncelli, Bovik 2003
SSIM_GAUSSIAN_WIN = 11


def ms_ssim_min_side(levels: int = len(MS_SSIM_WEIGHTS)) -> int:
    """the smallest H and W an L-level MS-SSIM takes: the coarsest level must still hold one 11x11 window"""
    return SSIM_GAUSSIAN_WIN * 2 ** (levels - 1)


def check_ms_ssim_weights(weights) -> tuple:
    """1 to 5 positive numbers, used as given (not renormalised)"""
    try:
        w = tuple(float(v) for v in weights)
    except TypeError:
        raise ValueError(f"MS-SSIM weights must be a sequence of 1 to 5 positive numbers, got {weights!r}") from None
    if not 1 <= len(w) <= 5 or not all(v > 0 and v < float("inf") for v in w):
        raise ValueError(f"MS-SSIM weights must be 1 to 5 positive numbers, got {weights!r}")
    return w


def _check_data_range(data_range) -> float:
    if not float(data_range) > 0:
        raise ValueError(f"data_range must be > 0, got {data_range!r}")
    return float(data_range)


def msssim_level_forward(x: torch.Tensor, y: torch.Tensor, data_range: float, want_pool: bool):
    """One level of csrc/msssim.hip on [N,3,H,W] float32 (level 0) or float64 (a pooled level) batches: (SSIM [N,3], CS [N,3],
    pooled x or None, pooled y or None), the statistics and the pooled pair float64 on the device."""
    N, _, Hh, Ww = x.shape
    f64 = x.dtype == torch.float64
    ntiles = H.value("adh_msssim_num_tiles", Hh, Ww)
    dev = x.device
    partial = torch.empty(N * 3 * ntiles * 2, device=dev, dtype=torch.float64)
    ssim = torch.empty((N, 3), device=dev, dtype=torch.float64)
    cs = torch.empty((N, 3), device=dev, dtype=torch.float64)
    px = torch.empty((N, 3, Hh // 2, Ww // 2), device=dev, dtype=torch.float64) if want_pool else None
    py = torch.empty_like(px) if want_pool else None
    H.call("adh_msssim_level_fwd", x.data_ptr(), y.data_ptr(), int(f64), N, Hh, Ww, float(data_range), partial.data_ptr(), ntiles,
           ssim.data_ptr(), cs.data_ptr(), H.ptr(px), H.ptr(py))
    return ssim, cs, px, py


def ssim_gaussian_batch(pred: torch.Tensor, target: torch.Tensor, data_range: float = 1.0) -> torch.Tensor:
    """Per-image SSIM [N] as the dehazing literature reports it (Wang et al. 2004): 11x11 Gaussian window with sigma 1.5,
    "valid" filtering, population covariances, per colour channel, then the mean over the three channels.  Not the
    reference's number: that is ssim_batch.  float64 statistics, one rounding to float32 at the end; no gradient."""
    pred, target = _check_pair(pred, target)
    data_range = _check_data_range(data_range)
    if pred.shape[2] < SSIM_GAUSSIAN_WIN or pred.shape[3] < SSIM_GAUSSIAN_WIN:
        raise ValueError(f"ssim_gaussian needs images of at least {SSIM_GAUSSIAN_WIN}x{SSIM_GAUSSIAN_WIN}, got "
                         f"{pred.shape[2]}x{pred.shape[3]}")
    ssim, _, _, _ = msssim_level_forward(pred, target, data_range, False)
    return ssim.mean(1).to(torch.float32)


def ms_ssim_pyramid(pred: torch.Tensor, target: torch.Tensor, data_range: float, weights: tuple, keep_levels: bool):
    """The forward of ms_ssim_batch: (ms_ssim [N] float32, V [L,N,3] float64, beta [L,1,1] float64, the level images or None).
    V_s is CS of level s for s < L-1 and SSIM of the last level.  Everything stays on the device."""
    pred, target = _check_pair(pred, target)
    data_range = _check_data_range(data_range)
    L = len(weights)
    if min(pred.shape[2], pred.shape[3]) < ms_ssim_min_side(L):
        raise ValueError(f"ms_ssim with {L} level{'s' if L > 1 else ''} needs images of at least {ms_ssim_min_side(L)}x"
                         f"{ms_ssim_min_side(L)} (11 * 2^(levels-1) on the shorter side), got {pred.shape[2]}x{pred.shape[3]}; "
                         "pass fewer weights for smaller images")
    x, y = pred, target
    V, levels = [], []
    for s in range(L):
        levels.append((x, y))
        ssim, cs, px, py = msssim_level_forward(x, y, data_range, s < L - 1)
        V.append(cs if s < L - 1 else ssim)
        x, y = px, py
    V = torch.stack(V)
    beta = torch.tensor(weights, dtype=torch.float64, device=pred.device).view(L, 1, 1)
    pos = (V > 0).all(0)
    M = torch.where(pos, V.clamp_min(0).pow(beta).prod(0), torch.zeros_like(V[0]))
    return M.mean(1).to(torch.float32), V, beta, (levels if keep_levels else None)


def ms_ssim_batch(pred: torch.Tensor, target: torch.Tensor, data_range: float = 1.0, weights=MS_SSIM_WEIGHTS) -> torch.Tensor:
    """Per-image MS-SSIM [N] (Wang, Simoncelli, Bovik 2003) on the Gaussian-window statistics of ssim_gaussian_batch: per colour
    plane prod_s max(V_s, 0)^weights[s] over a pyramid of 2x2 means, V_s the contrast-structure mean of level s and the full SSIM
    of the last, then the mean over the planes.  `weights`: 1 to 5 positive numbers, used as given; L of them need
    min(H, W) >= 11 * 2^(L-1) (176 for the default five).  No gradient: loss.ms_ssim_per_image has one."""
    return ms_ssim_pyramid(pred, target, data_range, check_ms_ssim_weights(weights), False)[0]


def calculate_image_metrics(pred: torch.Tensor, target: torch.Tensor, ciede2000: bool = False,
                            ms_ssim: bool = False) -> Dict[str, torch.Tensor]:
    """metrics.py:13-36 for a batch (or one [3,H,W] image): {'psnr': [N], 'ssim': [N]} device tensors; with `ciede2000` also
    that key; with `ms_ssim` also 'ssim_gaussian' and 'ms_ssim' (DESIGN 4.28)."""
    if pred.dim() == 3:
        pred, target = pred.unsqueeze(0), target.unsqueeze(0)
    m = {"psnr": psnr_batch(pred, target), "ssim": ssim_batch(pred, target)}
    if ciede2000:
        m["ciede2000"] = ciede2000_batch(pred, target)
    if ms_ssim:
        m["ssim_gaussian"] = ssim_gaussian_batch(pred, target)
        m["ms_ssim"] = ms_ssim_batch(pred, target)
    return m


class ImageQualityMetrics:
    """metrics.py:38-124: accumulate per-image metrics per category, average, print, save as JSON
    ({category: {psnr, ssim, lpips, samples}}).  `use_ciede2000` adds the key `ciede2000` to every chunk, and so to `results`,
    the averages, the printed lines and the saved JSON; off by default, which leaves the reference's key sets.  `use_ms_ssim`
    adds `ssim_gaussian` and `ms_ssim` the same way."""

    def __init__(self, device="cuda", lpips_fn=None, use_lpips: bool = True, use_ciede2000: bool = False,
                 use_ms_ssim: bool = False):
        self.device = torch.device(device)
        self.use_ciede2000 = bool(use_ciede2000)
        self.use_ms_ssim = bool(use_ms_ssim)
        self.lpips_fn = lpips_fn
        if lpips_fn is None and use_lpips:
            from .loss import PerceptualLoss
            self.lpips_fn = PerceptualLoss().to(self.device)
        self._chunks: Dict[str, List[Dict[str, torch.Tensor]]] = defaultdict(list)

    @property
    def results(self) -> Dict[str, List[Dict[str, float]]]:
        """The reference's `results` attribute: {category: [per-sample metric dicts]} (one host read-back)."""
        out: Dict[str, List[Dict[str, float]]] = defaultdict(list)
        for cat, chunks in self._chunks.items():
            for ch in chunks:
                host = {k: v.detach().cpu().tolist() for k, v in ch.items()}
                n = len(next(iter(host.values())))
                for i in range(n):
                    out[cat].append({k: host[k][i] for k in host})
        return out

    def add_batch(self, pred: torch.Tensor, target: torch.Tensor, categories: Optional[Sequence[str]] = None):
        """Whole [N,3,H,W] batches at once; `categories`: one name per image (or None -> 'all').  No host sync."""
        with torch.no_grad():
            m = calculate_image_metrics(pred, target, ciede2000=self.use_ciede2000, ms_ssim=self.use_ms_ssim)
            if self.lpips_fn is not None:
                # loss.PerceptualLoss maps [0,1] -> [-1,1] itself, i.e. it IS lpips.LPIPS(net='alex')(2p-1, 2t-1) of
                # metrics.py:69-75
                m["lpips"] = self.lpips_fn(pred.contiguous(), target.contiguous()).reshape(-1)
        if categories is None:
            self._chunks["all"].append(m)
            return
        cats = list(categories)
        for cat in sorted(set(cats)):
            sel = torch.tensor([i for i, c in enumerate(cats) if c == cat], device=pred.device)
            self._chunks[cat].append({k: v.index_select(0, sel) for k, v in m.items()})

    def add_sample(self, pred: torch.Tensor, target: torch.Tensor, category=None):
        """metrics.py:47-84 signature: one [3,H,W] pair."""
        self.add_batch(pred.unsqueeze(0), target.unsqueeze(0), None if not category else [category])

    def compute_averages(self):
        avg = {}
        for cat, chunks in self._chunks.items():
            if not chunks:
                continue
            avg[cat] = {}
            for name in chunks[0]:
                allv = torch.cat([c[name].double() for c in chunks])
                avg[cat][name] = float(allv.mean())
            avg[cat]["samples"] = int(sum(len(next(iter(c.values()))) for c in chunks))
        return avg

    def print_results(self):
        avg = self.compute_averages()
        print("Image Quality Evaluation Results:")
        for cat, ms in sorted(avg.items()):
            print(f"\n{cat.upper()} ({ms['samples']} samples):")
            for k, v in ms.items():
                if k != "samples":
                    print(f"  {k.upper()}: {v:.4f}")
        return avg

    def save_results(self, output_path):
        d = os.path.dirname(output_path)
        if d:
            os.makedirs(d, exist_ok=True)
        with open(output_path, "w") as f:
            json.dump(self.compute_averages(), f, indent=2)
        print(f"Results saved to {output_path}")
