"""Time one training step's input from the device-resident 8-bit cache (data.batch_from_cache on csrc/dataset.hip: both roles,
hazy and clear, augmented with one parameter row per sample) at 16 x 256 x 256 and 8 x 512 x 1024, and in the same run,
alternated with it, the composition of the code that existed before it:

    paired_augment([u8_to_image(hazy[idx]), u8_to_image(clear[idx])], params)

(torch's index gather of the bytes, csrc/image_io.hip, csrc/train_io.hip).  Both draw a fresh random index per call from a seeded
cache of random bytes sized past the 256 MiB Infinity Cache, so a small shape does not time the cache; the index upload is part of
both.  Device events around back-to-back calls, every variant warmed up first, each timed window about `--window` seconds long.

Bytes: the new path moves 18 bytes per pixel and role (3 read by the grey-mean pass, 3 read and 12 written by the gather pass);
GB/s and the share of the chip's streaming rate are that count over the measured time, for the composition too (what it achieves
of the job; its own passes move 57 bytes per pixel and role).

    python tools/bench_dataset.py [--rounds 5] [--window 0.5] [--out profiles/bench_dataset.json]

Prints one JSON object (and writes it to --out when given)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from adam_dehaze_amd import data as D  # noqa: E402
from adam_dehaze_amd import image_io as IO  # noqa: E402

HBM_BPS = 6.29e12
CACHE_BYTES = 384 << 20         # per role
SHAPES = [(16, 256, 256), (8, 512, 1024)]
BYTES_PER_PIXEL = 18            # per role
ROLES = 2


def _time_us(fn, n):
    """mean microseconds per call of fn(i) over n back-to-back calls between two device events"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(n):
        fn(i)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / n


def _measure(N, H, W, rounds, window, dev):
    M = max(2 * N, CACHE_BYTES // (H * W * 3))
    gen = torch.Generator(device=dev).manual_seed(0)
    hazy = torch.randint(0, 256, (M, H, W, 3), dtype=torch.uint8, device=dev, generator=gen)
    clear = torch.randint(0, 256, (M, H, W, 3), dtype=torch.uint8, device=dev, generator=gen)
    rng = np.random.RandomState(0)
    indices = [torch.from_numpy(rng.randint(0, M, size=N).astype(np.int64)) for _ in range(64)]
    params = [D.draw_augment_params(N, rng) for _ in range(64)]

    def cache_path(i):
        return D.batch_from_cache((hazy, clear), indices[i % 64], params[i % 64])

    def composition(i):
        idx, p = indices[i % 64].to(dev), params[i % 64]
        return D.paired_augment([IO.u8_to_image(hazy[idx]), IO.u8_to_image(clear[idx])], p)[0]
    fns = {"batch_from_cache": cache_path, "composition": composition}
    a, b = cache_path(0), composition(0)
    max_diff = max(float((x - y).abs().max()) for x, y in zip(a, b))
    nbytes = ROLES * BYTES_PER_PIXEL * N * H * W
    calls = {}
    for k, fn in fns.items():                            # warm every variant at this shape, and size its window
        _time_us(fn, 20)
        calls[k] = max(50, int(window / (_time_us(fn, 50) * 1e-6)))
    us = {k: [] for k in fns}
    for _ in range(rounds):                              # alternate, so drift of the shared host hits both alike
        for k, fn in fns.items():
            us[k].append(_time_us(fn, calls[k]))
    med = {k: statistics.median(v) for k, v in us.items()}
    res = {"N": N, "H": H, "W": W, "cache_images_per_role": M, "bytes_per_step_input": nbytes, "calls_per_sample": calls,
           "streaming_floor_us": round(nbytes / HBM_BPS * 1e6, 2), "max_abs_difference_from_composition": max_diff}
    for k in fns:
        res[k] = {"us": {"median": round(med[k], 2), "min": round(min(us[k]), 2), "max": round(max(us[k]), 2)},
                  "GBps": round(nbytes / med[k] * 1e-3, 1), "fraction_of_streaming_rate": round(nbytes / (med[k] * 1e-6) / HBM_BPS, 4)}
    res["composition_over_batch_from_cache"] = round(med["composition"] / med["batch_from_cache"], 3)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5, help="samples per variant, alternated")
    ap.add_argument("--window", type=float, default=0.5, help="seconds of back-to-back calls per sample")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_dataset.py needs the GPU: there is no CPU timing to report")
    dev = "cuda:0"
    res = {"hbm_bytes_per_s": HBM_BPS, "samples": a.rounds, "window_s": a.window, "bytes_per_pixel_and_role": BYTES_PER_PIXEL,
           "roles": ROLES, "shapes": [_measure(N, H, W, a.rounds, a.window, dev) for N, H, W in SHAPES]}
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
