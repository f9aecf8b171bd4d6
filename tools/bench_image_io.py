"""Time the two kernels of csrc/image_io.hip (image_io.u8_to_image / image_to_u8, RGB) at 512 x 1024 and 2160 x 3840, N = 1 and 8,
and in the same run, alternated with them:

  * a device-to-device copy that moves the same number of bytes (half of them read, half written),
  * the torch expression chain each kernel replaces:  t.permute(0, 3, 1, 2).contiguous().float().div(255)  on the way in and
    x.clamp(0, 1).mul(255).round().to(torch.uint8).permute(0, 2, 3, 1).contiguous()  on the way out.

A call moves 15 bytes per pixel (3 as bytes, 12 as floats); GB/s is that count over the measured time, for the chains too (what
they achieve of the job, not what their passes move).  Every variant walks the same ring of buffer sets, sized past the 256 MiB
Infinity Cache, so a small shape does not time the cache.  Device events around back-to-back calls, warm-up first.  At each shape
the outputs of kernel and chain are compared once and the number of differing elements is reported (torch divides by a scalar
on the device as a product with its reciprocal, so some of the 256 values can differ in the last bit on the way in).

    python tools/bench_image_io.py [--rounds 5] [--out profiles/bench_image_io.json]

Prints one JSON object (and writes it to --out when given)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from adam_dehaze_amd import image_io as IO  # noqa: E402

HBM_BPS = 6.29e12
RING_BYTES = 768 << 20          # buffer sets are added until they hold this much (at most MAX_SETS)
MAX_SETS = 64
SHAPES = [(1, 512, 1024), (8, 512, 1024), (1, 2160, 3840), (8, 2160, 3840)]
BYTES_PER_PIXEL = 15


def _time_us(fn, n):
    """mean microseconds per call of fn(i) over n back-to-back calls between two device events"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(n):
        fn(i)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / n


def chain_in(t):
    return t.permute(0, 3, 1, 2).contiguous().float().div(255)


def chain_out(x):
    return x.clamp(0, 1).mul(255).round().to(torch.uint8).permute(0, 2, 3, 1).contiguous()


def _measure(N, H, W, rounds, dev):
    nbytes = BYTES_PER_PIXEL * N * H * W
    nsets = max(1, min(MAX_SETS, -(-RING_BYTES // nbytes)))
    gen = torch.Generator(device=dev).manual_seed(0)
    u8 = [torch.randint(0, 256, (N, H, W, 3), dtype=torch.uint8, device=dev, generator=gen) for _ in range(nsets)]
    f32 = [torch.rand((N, 3, H, W), device=dev, generator=gen) * 1.2 - 0.1 for _ in range(nsets)]
    out8 = [torch.empty_like(t) for t in u8]
    half = [(torch.empty(nbytes // 2, dtype=torch.uint8, device=dev), torch.empty(nbytes // 2, dtype=torch.uint8, device=dev))
            for _ in range(nsets)]
    fns = {"u8_to_image": lambda i: IO.u8_to_image(u8[i % nsets]),
           "torch_chain_in": lambda i: chain_in(u8[i % nsets]),
           "image_to_u8": lambda i: IO.image_to_u8(f32[i % nsets], out=out8[i % nsets]),
           "torch_chain_out": lambda i: chain_out(f32[i % nsets]),
           "d2d_copy": lambda i: half[i % nsets][1].copy_(half[i % nsets][0])}
    differ = {"in": int((IO.u8_to_image(u8[0]).view(torch.int32) != chain_in(u8[0]).view(torch.int32)).sum()),
              "out": int((IO.image_to_u8(f32[0]) != chain_out(f32[0])).sum())}
    calls = max(20, min(2000, int(0.02 / (nbytes / HBM_BPS))))
    for fn in fns.values():                              # warm every variant at this shape: code objects, allocator
        _time_us(fn, max(3, nsets))
    us = {k: [] for k in fns}
    for _ in range(rounds):                              # alternate, so drift of the shared host hits all alike
        for k, fn in fns.items():
            us[k].append(_time_us(fn, calls))
    med = {k: statistics.median(v) for k, v in us.items()}
    res = {"N": N, "H": H, "W": W, "bytes_per_call": nbytes, "buffer_sets": nsets, "calls_per_sample": calls,
           "streaming_floor_us": round(nbytes / HBM_BPS * 1e6, 2), "elements_differing_from_chain": differ}
    for k in fns:
        res[k] = {"us": {"median": round(med[k], 2), "min": round(min(us[k]), 2), "max": round(max(us[k]), 2)},
                  "GBps": round(nbytes / med[k] * 1e-3, 1), "fraction_of_streaming_rate": round(nbytes / (med[k] * 1e-6) / HBM_BPS, 4)}
    res["ratios"] = {"u8_to_image_over_d2d_copy": round(med["u8_to_image"] / med["d2d_copy"], 3),
                     "image_to_u8_over_d2d_copy": round(med["image_to_u8"] / med["d2d_copy"], 3),
                     "torch_chain_in_over_u8_to_image": round(med["torch_chain_in"] / med["u8_to_image"], 3),
                     "torch_chain_out_over_image_to_u8": round(med["torch_chain_out"] / med["image_to_u8"], 3)}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5, help="samples per variant, alternated")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_image_io.py needs the GPU: there is no CPU timing to report")
    dev = "cuda:0"
    res = {"hbm_bytes_per_s": HBM_BPS, "samples": a.rounds, "bytes_per_pixel": BYTES_PER_PIXEL, "channels": 3,
           "shapes": [_measure(N, H, W, a.rounds, dev) for N, H, W in SHAPES]}
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
