"""Time the natural-scene-statistics kernels of csrc/nss.hip at 8 x 3 x 512 x 1024 and 1 x 3 x 2160 x 3840:

  * `brisque_features`      nss.brisque_features: moments of the whole plane, the halving, moments of the halved plane, the fit
  * `niqe_patch_features`   nss.niqe_patch_features: the same over 96 x 96 patches of the crop (48 x 48 at the second scale)
  * `moments_rgb`, `halve`, `moments_f64`   the three launches of `brisque_features` on their own

and, in the same run, alternated with them:

  (a) `torch_f64_brisque` / `torch_f64_niqe`: the same formulas as float64 torch expressions on the device (the window as 49
      weighted shifted slices of the replicate-padded plane, the halving as eight gathered slices per pass, the neighbour
      products with torch.roll inside the regions), which is what a user without the kernels would write; the fit is shared;
  (b) the time the algorithmic bytes would take at the 6.29 TB/s streaming rate: the fp32 planes read once, the float64 halved
      plane written and read again (16 bytes per pixel).

Every variant walks the same ring of inputs, sized past the 256 MiB Infinity Cache.  Device events around back-to-back calls,
warm-up first, median of `--rounds` alternated samples.  Kernel and chain are compared once per shape.

    python tools/bench_nss.py [--rounds 5] [--out profiles/bench_nss.json]

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

from adam_dehaze_amd import nss as NSS  # noqa: E402

HBM_BPS = 6.29e12
RING_BYTES = 768 << 20
MAX_SETS = 64
SHAPES = [(8, 512, 1024), (1, 2160, 3840)]
SAMPLE_SECONDS = 0.05
BYTES_PER_PIXEL = 12.0 + 2.0 + 2.0
TAPS = [v / 256.0 for v in (-3.0, -9.0, 29.0, 111.0, 111.0, 29.0, -9.0, -3.0)]
DIRECTIONS = ((0, 1), (1, 0), (1, 1), (1, -1))


def _window():
    i = torch.arange(7, dtype=torch.float64)
    g = torch.exp(-((i - 3) ** 2) / (2.0 * (7.0 / 6.0) ** 2))
    g = g / g.sum()
    return (g[:, None] * g[None, :]).tolist()


def _moments_chain(Y, rh, rw, w):
    """[N,H,W] float64 -> [N,H/rh,W/rw,24] from whole-tensor operations"""
    N, H, W = Y.shape
    P = F.pad(Y.unsqueeze(1), (3, 3, 3, 3), mode="replicate")[:, 0]
    d, v = torch.zeros_like(Y), torch.zeros_like(Y)
    for a in range(7):
        for b in range(7):
            t = P[:, a:a + H, b:b + W] - Y
            d = d + w[a][b] * t
            v = v + w[a][b] * t * t
    s = (v - d * d).abs().sqrt()
    M = -d / (s + 1.0)
    reg = lambda z: z.view(N, H // rh, rh, W // rw, rw).permute(0, 1, 3, 2, 4)
    Rm = reg(M)
    out = [Rm.abs().sum((3, 4)), (Rm * Rm).sum((3, 4)), reg(s).sum((3, 4))]
    for di, dj in DIRECTIONS:
        p = Rm * torch.roll(Rm, (-di, -dj), (3, 4))
        neg, pos = p < 0, p > 0
        out += [neg.double().sum((3, 4)), (p * p * neg).sum((3, 4)), pos.double().sum((3, 4)), (p * p * pos).sum((3, 4)),
                p.abs().sum((3, 4))]
    out.append(torch.zeros_like(out[0]))
    return torch.stack(out, -1)


def _halve_chain(Y):
    for dim in (2, 1):
        n = Y.shape[dim]
        j = torch.arange((n + 1) // 2, device=Y.device)
        acc = None
        for k, t in enumerate(TAPS):
            term = t * Y.index_select(dim, (2 * j - 3 + k).clamp(0, n - 1))
            acc = term if acc is None else acc + term
        Y = acc
    return Y


def _grey(x, Hc, Wc):
    x = x[:, :, :Hc, :Wc].double()
    return 255.0 * (0.299 * x[:, 0] + 0.587 * x[:, 1] + 0.114 * x[:, 2])


def chain_brisque(x, w):
    N, _, H, W = x.shape
    Y = _grey(x, H, W)
    Y2 = _halve_chain(Y)
    f1 = NSS.fit_features(_moments_chain(Y, H, W, w), H * W)
    f2 = NSS.fit_features(_moments_chain(Y2, Y2.shape[1], Y2.shape[2], w), Y2.shape[1] * Y2.shape[2])
    return torch.cat([f1.view(N, 18), f2.view(N, 18)], 1)


def chain_niqe(x, w):
    N, _, H, W = x.shape
    Y = _grey(x, 96 * (H // 96), 96 * (W // 96))
    f1 = NSS.fit_features(_moments_chain(Y, 96, 96, w), 96 * 96)
    f2 = NSS.fit_features(_moments_chain(_halve_chain(Y), 48, 48, w), 48 * 48)
    return torch.cat([f1, f2], -1).view(N, -1, 36)


def _time_us(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(n):
        fn(i)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / n


def _measure(N, H, W, rounds, dev):
    nsets = max(2, min(MAX_SETS, -(-RING_BYTES // (12 * N * H * W))))
    gen = torch.Generator(device=dev).manual_seed(0)
    # 8-bit images with smooth structure under the noise, as decoded photographs are
    xs = [(torch.rand(N, 3, H, W, device=dev, generator=gen) * 255).round() / 255 for _ in range(nsets)]
    w = _window()
    halved = NSS.nss_halve(xs[0])
    fns = {"brisque_features": lambda i: NSS.brisque_features(xs[i % nsets]),
           "niqe_patch_features": lambda i: NSS.niqe_patch_features(xs[i % nsets]),
           "moments_rgb": lambda i: NSS.nss_moments(xs[i % nsets], H, W),
           "halve": lambda i: NSS.nss_halve(xs[i % nsets]),
           "moments_f64": lambda i: NSS.nss_moments(halved, halved.shape[1], halved.shape[2]),
           "torch_f64_brisque": lambda i: chain_brisque(xs[i % nsets], w),
           "torch_f64_niqe": lambda i: chain_niqe(xs[i % nsets], w)}
    with torch.no_grad():
        fb, cb = fns["brisque_features"](0), fns["torch_f64_brisque"](0)
        fn_, cn = fns["niqe_patch_features"](0)[0], fns["torch_f64_niqe"](0)
        agree = {"brisque_max_abs_feature_difference": float((fb - cb).abs().max()),
                 "niqe_max_abs_feature_difference": float((fn_ - cn).abs().max())}
        calls = {}
        for k, fn in fns.items():
            _time_us(fn, 2)
            calls[k] = max(3, min(400, int(SAMPLE_SECONDS * 1e6 / _time_us(fn, 3))))
        us = {k: [] for k in fns}
        for _ in range(rounds):                              # alternate, so drift of the shared host hits all alike
            for k, fn in fns.items():
                us[k].append(_time_us(fn, calls[k]))
    med = {k: statistics.median(v) for k, v in us.items()}
    px = N * H * W
    res = {"N": N, "H": H, "W": W, "inputs_in_ring": nsets, "calls_per_sample": calls, "kernel_against_chain": agree}
    for k in fns:
        res[k] = {"us": {"median": round(med[k], 2), "min": round(min(us[k]), 2), "max": round(max(us[k]), 2)},
                  "ns_per_pixel": round(med[k] * 1e3 / px, 4)}
    floor = BYTES_PER_PIXEL * px / HBM_BPS * 1e6
    res["streaming_floor_us"] = round(floor, 2)
    res["ratios"] = {"brisque_over_floor": round(med["brisque_features"] / floor, 2),
                     "niqe_over_floor": round(med["niqe_patch_features"] / floor, 2),
                     "torch_f64_over_brisque": round(med["torch_f64_brisque"] / med["brisque_features"], 2),
                     "torch_f64_over_niqe": round(med["torch_f64_niqe"] / med["niqe_patch_features"], 2)}
    # per pixel of the first scale: 49 taps of a subtraction and two fused multiply-adds with a product under the second
    res["float64_tflops_moments_rgb"] = round(49 * 5 * px / (med["moments_rgb"] * 1e-6) / 1e12, 2)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5, help="samples per variant, alternated")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_nss.py needs the GPU: there is no CPU timing to report")
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
