"""Time the kernels of csrc/msssim.hip at 8 x 3 x 512 x 1024 and 1 x 3 x 2160 x 3840, forward and backward:

  * `ssim_gaussian`       metrics.ssim_gaussian_batch: one level forward (no pooled output)
  * `ms_ssim`             metrics.ms_ssim_batch: the five-level forward with the small torch operations that combine the levels
  * `ms_ssim_fwd_bwd`     loss.ms_ssim_per_image and its backward: forward, coefficients, five level backwards

and, in the same run, alternated with them:

  (a) `torch_f64` / `torch_f64_fwd_bwd`: the same formulas as float64 torch expressions on the device (the separable filter as 11
      weighted shifted slices per pass, avg_pool2d, autograd for the gradient), which is what a user without the kernels would
      write;
  (b) the time the algorithmic bytes would take at the 6.29 TB/s streaming rate: the fp32 images, the float64 pooled levels
      written and read again, the gradients written and the coarser gradients read.

Every variant walks the same ring of input pairs, sized past the 256 MiB Infinity Cache.  Device events around back-to-back calls,
warm-up first, median of `--rounds` alternated samples.  Kernel and chain are compared once per shape.

    python tools/bench_msssim.py [--rounds 5] [--out profiles/bench_msssim.json]

Prints one JSON object (and writes it to --out when given)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from adam_dehaze_amd import loss as L  # noqa: E402
from adam_dehaze_amd import metrics as M  # noqa: E402

HBM_BPS = 6.29e12
RING_BYTES = 768 << 20
MAX_SETS = 64
SHAPES = [(8, 512, 1024), (1, 2160, 3840)]
SAMPLE_SECONDS = 0.05
LEVELS = len(M.MS_SSIM_WEIGHTS)
_COARSE = sum(0.25 ** s for s in range(1, LEVELS))          # pixels of the pooled levels per level-0 pixel
BYTES_PER_PIXEL = {
    "ssim_gaussian": 24.0,                                   # six fp32 planes read
    # the fp32 pair read; the float64 pooled pairs written, and read again by their own level
    "ms_ssim": 24.0 + 2 * 48.0 * _COARSE,
    # backward alone: every level's pair read, its gradient written (fp32 at level 0, float64 below), the coarser gradient read
    "ms_ssim_bwd": 24.0 + 12.0 + 48.0 * _COARSE + 24.0 * _COARSE + 24.0 * _COARSE,
}
BYTES_PER_PIXEL["ms_ssim_fwd_bwd"] = BYTES_PER_PIXEL["ms_ssim"] + BYTES_PER_PIXEL["ms_ssim_bwd"]


def _window(dev):
    i = torch.arange(11, dtype=torch.float64, device=dev)
    g = torch.exp(-((i - 5) ** 2) / 4.5)
    return (g / g.sum()).tolist()


def _filt(z, g):
    OW, OH = z.shape[-1] - 10, z.shape[-2] - 10
    r = sum(g[k] * z[..., k:k + OW] for k in range(11))
    return sum(g[k] * r[..., k:k + OH, :] for k in range(11))


def torch_chain(pred, target, g, weights=M.MS_SSIM_WEIGHTS):
    """ms_ssim [N] in float64 from whole-tensor torch operations; differentiable in pred"""
    x, y = pred.double(), target.double()
    C1, C2 = 0.01 ** 2, 0.03 ** 2
    M_ = None
    for s, beta in enumerate(weights):
        mx, my = _filt(x, g), _filt(y, g)
        D2 = (_filt(x * x, g) - mx * mx) + (_filt(y * y, g) - my * my) + C2
        cs = (2 * (_filt(x * y, g) - mx * my) + C2) / D2
        v = cs if s < len(weights) - 1 else cs * (2 * mx * my + C1) / (mx * mx + my * my + C1)
        v = v.flatten(2).mean(2).clamp_min(1e-300) ** beta
        M_ = v if M_ is None else M_ * v
        if s < len(weights) - 1:
            x, y = F.avg_pool2d(x, 2), F.avg_pool2d(y, 2)
    return M_.mean(1)


def _time_us(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(n):
        fn(i)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / n


def _measure(N, H, W, rounds, dev):
    pair_bytes = 24 * N * H * W
    nsets = max(2, min(MAX_SETS, -(-RING_BYTES // pair_bytes)))
    gen = torch.Generator(device=dev).manual_seed(0)
    pred, target = [], []
    for _ in range(nsets):                                   # a dehazed image is a disturbed copy of its ground truth
        t = torch.rand(N, 3, H, W, device=dev, generator=gen)
        target.append(t)
        pred.append((t + 0.05 * torch.randn(N, 3, H, W, device=dev, generator=gen)).clamp(0, 1))
    g = _window(dev)
    up = torch.full((N,), -1.0 / N, device=dev)

    def kernel_fwd_bwd(i):
        p = pred[i % nsets].requires_grad_(True)
        (L.ms_ssim_per_image(p, target[i % nsets]) * up).sum().backward()
        grad, p.grad = p.grad, None
        p.requires_grad_(False)
        return grad

    def chain_fwd_bwd(i):
        p = pred[i % nsets].requires_grad_(True)
        (torch_chain(p, target[i % nsets], g) * up.double()).sum().backward()
        grad, p.grad = p.grad, None
        p.requires_grad_(False)
        return grad

    def chain_fwd(i):
        with torch.no_grad():
            return torch_chain(pred[i % nsets], target[i % nsets], g)
    fns = {"ssim_gaussian": lambda i: M.ssim_gaussian_batch(pred[i % nsets], target[i % nsets]),
           "ms_ssim": lambda i: M.ms_ssim_batch(pred[i % nsets], target[i % nsets]),
           "ms_ssim_fwd_bwd": kernel_fwd_bwd, "torch_f64": chain_fwd, "torch_f64_fwd_bwd": chain_fwd_bwd}
    vk, vt = M.ms_ssim_batch(pred[0], target[0]).double(), chain_fwd(0)
    gk, gt = kernel_fwd_bwd(0).double(), chain_fwd_bwd(0).double()
    agree = {"max_abs_value_difference": float((vk - vt).abs().max()), "mean_ms_ssim": float(vt.mean()),
             "max_abs_gradient_difference": float((gk - gt).abs().max()), "max_abs_gradient": float(gt.abs().max())}
    del gk, gt
    calls = {}
    for k, fn in fns.items():
        _time_us(fn, 2)
        calls[k] = max(3, min(400, int(SAMPLE_SECONDS * 1e6 / _time_us(fn, 3))))
    us = {k: [] for k in fns}
    for _ in range(rounds):                                  # alternate, so drift of the shared host hits all alike
        for k, fn in fns.items():
            us[k].append(_time_us(fn, calls[k]))
    med = {k: statistics.median(v) for k, v in us.items()}
    px = N * H * W
    res = {"N": N, "H": H, "W": W, "input_pairs_in_ring": nsets, "calls_per_sample": calls, "kernel_against_chain": agree}
    for k in fns:
        res[k] = {"us": {"median": round(med[k], 2), "min": round(min(us[k]), 2), "max": round(max(us[k]), 2)},
                  "ns_per_pixel": round(med[k] * 1e3 / px, 4)}
    res["ms_ssim_bwd_by_difference_us"] = round(med["ms_ssim_fwd_bwd"] - med["ms_ssim"], 2)
    floors = {k: v * px / HBM_BPS * 1e6 for k, v in BYTES_PER_PIXEL.items()}
    res["streaming_floor_us"] = {k: round(v, 2) for k, v in floors.items()}
    res["ratios"] = {"ssim_gaussian_over_floor": round(med["ssim_gaussian"] / floors["ssim_gaussian"], 2),
                     "ms_ssim_over_floor": round(med["ms_ssim"] / floors["ms_ssim"], 2),
                     "ms_ssim_fwd_bwd_over_floor": round(med["ms_ssim_fwd_bwd"] / floors["ms_ssim_fwd_bwd"], 2),
                     "torch_f64_over_ms_ssim": round(med["torch_f64"] / med["ms_ssim"], 2),
                     "torch_f64_fwd_bwd_over_ms_ssim_fwd_bwd": round(med["torch_f64_fwd_bwd"] / med["ms_ssim_fwd_bwd"], 2)}
    # float64 fused multiply-adds of one level per pixel and plane (the two 11-tap passes over five moments forward; those over
    # the tile's halo, and the two transposed passes over three maps, backward), all levels: x (1 + _COARSE)
    res["float64_fma_per_pixel"] = {"forward": round(3 * (1 + _COARSE) * 55 * (26 * 32 + 16 * 32) / (16 * 32), 1),
                                    "backward": round(3 * (1 + _COARSE) * (55 * (32 * 32 + 22 * 32) + 33 * (22 * 22 + 12 * 22)) / (12 * 22), 1)}
    res["float64_tflops"] = {"ms_ssim": round(2 * res["float64_fma_per_pixel"]["forward"] * px / (med["ms_ssim"] * 1e-6) / 1e12, 2),
                             "ms_ssim_bwd_by_difference": round(2 * res["float64_fma_per_pixel"]["backward"] * px
                                                                / (max(res["ms_ssim_bwd_by_difference_us"], 1e-3) * 1e-6) / 1e12, 2)}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5, help="samples per variant, alternated")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_msssim.py needs the GPU: there is no CPU timing to report")
    dev = "cuda:0"
    res = {"hbm_bytes_per_s": HBM_BPS, "samples": a.rounds, "bytes_per_pixel": {k: round(v, 2) for k, v in BYTES_PER_PIXEL.items()},
           "shapes": [_measure(N, H, W, a.rounds, dev) for N, H, W in SHAPES]}
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
