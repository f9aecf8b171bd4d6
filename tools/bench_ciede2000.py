"""Time the kernel of csrc/ciede2000.hip (metrics.ciede2000_batch, sRGB input) at 1 x 512 x 1024, 8 x 512 x 1024 and
1 x 2160 x 3840 and, in the same run, alternated with it:

  * the same formula as a float64 torch expression chain on the device (`torch_chain` below: rgb2lab and dE00 as whole-tensor
    operations, the per-image mean at the end), which is what a user without the kernel would write,
  * with the per-pixel map as well as the mean (28 bytes per pixel instead of 24).

Two bounds are reported beside the times: the time the 24 bytes per pixel of the six input planes would take at the 6.29 TB/s
streaming rate, and the torch chain.  Every variant walks the same ring of input pairs, sized past the 256 MiB Infinity Cache, so
a small shape does not time the cache.  Device events around back-to-back calls, warm-up first, median of `--rounds` alternated
samples.  At each shape kernel and chain are compared once (largest difference of the maps and of the means).

    python tools/bench_ciede2000.py [--rounds 5] [--out profiles/bench_ciede2000.json]

Prints one JSON object (and writes it to --out when given)."""
import argparse
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from adam_dehaze_amd import metrics as M  # noqa: E402

HBM_BPS = 6.29e12
RING_BYTES = 768 << 20          # input pairs are added until they hold this much (at most MAX_SETS)
MAX_SETS = 64
SHAPES = [(1, 512, 1024), (8, 512, 1024), (1, 2160, 3840)]
BYTES_PER_PIXEL = 24            # six fp32 planes read; the mean is N floats
SAMPLE_SECONDS = 0.05           # device time one sample aims at


def _rgb2lab(x):
    """[N,3,H,W] sRGB, any float dtype -> L, a, b as three float64 [N,H,W]"""
    x = x.double()
    c = torch.where(x > 0, x.clamp(max=1.0), torch.zeros_like(x))
    lin = torch.where(c <= 0.04045, c / 12.92, ((c + 0.055) / 1.055) ** 2.4)
    r, g, b = lin[:, 0], lin[:, 1], lin[:, 2]
    xyz = ((0.412453 * r + 0.357580 * g + 0.180423 * b) / 0.95047, 0.212671 * r + 0.715160 * g + 0.072169 * b,
           (0.019334 * r + 0.119193 * g + 0.950227 * b) / 1.08883)
    d = 6.0 / 29.0
    fx, fy, fz = (torch.where(t > d ** 3, t.pow(1.0 / 3.0), t / (3 * d * d) + 4.0 / 29.0) for t in xyz)
    return 116 * fy - 16, 500 * (fx - fy), 200 * (fy - fz)


def _hue(b, ap):
    h = torch.rad2deg(torch.atan2(b, ap))
    h = torch.where(h < 0, h + 360, h)
    return torch.where((ap == 0) & (b == 0), torch.zeros_like(h), h)


def torch_chain(pred, target):
    """(mean [N], map [N,H,W]) in float64: the definition at the head of csrc/ciede2000.hip as torch expressions"""
    L1, a1, b1 = _rgb2lab(pred)
    L2, a2, b2 = _rgb2lab(target)
    Cm = (torch.hypot(a1, b1) + torch.hypot(a2, b2)) / 2
    Cm7 = Cm ** 7
    G = 0.5 * (1 - torch.sqrt(Cm7 / (Cm7 + 25.0 ** 7)))
    ap1, ap2 = (1 + G) * a1, (1 + G) * a2
    Cp1, Cp2 = torch.hypot(ap1, b1), torch.hypot(ap2, b2)
    h1, h2 = _hue(b1, ap1), _hue(b2, ap2)
    CC = Cp1 * Cp2
    grey = CC == 0
    hd, hs = h2 - h1, h1 + h2
    dh = torch.where(grey, torch.zeros_like(hd), torch.where(hd > 180, hd - 360, torch.where(hd < -180, hd + 360, hd)))
    dH = 2 * torch.sqrt(CC) * torch.sin(torch.deg2rad(dh / 2))
    Lm, Cpm = (L1 + L2) / 2, (Cp1 + Cp2) / 2
    hm = torch.where(grey, hs, torch.where((h1 - h2).abs() <= 180, hs / 2, torch.where(hs < 360, (hs + 360) / 2, (hs - 360) / 2)))
    T = (1 - 0.17 * torch.cos(torch.deg2rad(hm - 30)) + 0.24 * torch.cos(torch.deg2rad(2 * hm))
         + 0.32 * torch.cos(torch.deg2rad(3 * hm + 6)) - 0.20 * torch.cos(torch.deg2rad(4 * hm - 63)))
    l50 = (Lm - 50) ** 2
    SL = 1 + 0.015 * l50 / torch.sqrt(20 + l50)
    SC = 1 + 0.045 * Cpm
    SH = 1 + 0.015 * Cpm * T
    Cpm7 = Cpm ** 7
    RT = -torch.sin(torch.deg2rad(60 * torch.exp(-(((hm - 275) / 25) ** 2)))) * 2 * torch.sqrt(Cpm7 / (Cpm7 + 25.0 ** 7))
    tL, tC, tH = (L2 - L1) / SL, (Cp2 - Cp1) / SC, dH / SH
    de = torch.sqrt((tL * tL + tC * tC + tH * tH + RT * tC * tH).clamp(min=0))
    return de.flatten(1).mean(1), de


def _time_us(fn, n):
    """mean microseconds per call of fn(i) over n back-to-back calls between two device events"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(n):
        fn(i)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / n


def _measure(N, H, W, rounds, dev):
    nbytes = BYTES_PER_PIXEL * N * H * W
    nsets = max(2, min(MAX_SETS, -(-RING_BYTES // nbytes)))
    gen = torch.Generator(device=dev).manual_seed(0)
    # 8-bit-derived pixels, as image files give them; the second image a disturbed copy of the first, as a dehazed file is of its
    # ground truth
    pred, target = [], []
    for _ in range(nsets):
        a = torch.randint(0, 256, (N, 3, H, W), device=dev, generator=gen)
        b = (a + torch.randint(-40, 41, (N, 3, H, W), device=dev, generator=gen)).clamp(0, 255)
        pred.append(a.float() / 255)
        target.append(b.float() / 255)
    fns = {"ciede2000": lambda i: M.ciede2000_batch(pred[i % nsets], target[i % nsets]),
           "ciede2000_with_map": lambda i: M.ciede2000_batch(pred[i % nsets], target[i % nsets], return_map=True),
           "torch_chain_f64": lambda i: torch_chain(pred[i % nsets], target[i % nsets])}
    mean_k, map_k = M.ciede2000_batch(pred[0], target[0], return_map=True)
    mean_t, map_t = torch_chain(pred[0], target[0])
    agree = {"max_abs_map_difference": float((map_k.double() - map_t).abs().max()),
             "max_abs_mean_difference": float((mean_k.double() - mean_t).abs().max()), "mean_dE00": float(mean_t.mean())}
    del map_k, map_t
    calls = {}
    for k, fn in fns.items():                            # warm every variant at this shape, then size its sample
        _time_us(fn, 2)
        calls[k] = max(3, min(400, int(SAMPLE_SECONDS * 1e6 / _time_us(fn, 3))))
    us = {k: [] for k in fns}
    for _ in range(rounds):                              # alternate, so drift of the shared host hits all alike
        for k, fn in fns.items():
            us[k].append(_time_us(fn, calls[k]))
    med = {k: statistics.median(v) for k, v in us.items()}
    floor_us = nbytes / HBM_BPS * 1e6
    res = {"N": N, "H": H, "W": W, "bytes_per_call": nbytes, "input_pairs_in_ring": nsets, "calls_per_sample": calls,
           "streaming_floor_us": round(floor_us, 2), "kernel_against_chain": agree}
    for k in fns:
        res[k] = {"us": {"median": round(med[k], 2), "min": round(min(us[k]), 2), "max": round(max(us[k]), 2)},
                  "ns_per_pixel": round(med[k] * 1e3 / (N * H * W), 4)}
    res["ratios"] = {"ciede2000_over_streaming_floor": round(med["ciede2000"] / floor_us, 2),
                     "torch_chain_f64_over_ciede2000": round(med["torch_chain_f64"] / med["ciede2000"], 2),
                     "with_map_over_without": round(med["ciede2000_with_map"] / med["ciede2000"], 3)}
    # which bound the kernel sits nearer to, on a logarithmic scale
    res["nearer_bound"] = "streaming_floor" if math.log(med["ciede2000"] / floor_us) < math.log(
        max(med["torch_chain_f64"] / med["ciede2000"], 1e-9)) else "torch_chain_f64"
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5, help="samples per variant, alternated")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_ciede2000.py needs the GPU: there is no CPU timing to report")
    dev = "cuda:0"
    res = {"hbm_bytes_per_s": HBM_BPS, "samples": a.rounds, "bytes_per_pixel": BYTES_PER_PIXEL,
           "shapes": [_measure(N, H, W, a.rounds, dev) for N, H, W in SHAPES]}
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
