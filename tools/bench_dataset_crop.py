"""Time one training step's input as random crops of native-size images (data.batch_from_windows on csrc/dataset.hip's
adh_batch_window_from_u8: both roles, hazy and clear, augmented with one parameter row per sample) at 16 x 256 x 256 windows out
of 512 x 1024 images and 8 x 512 x 1024 out of 1024 x 2048, separately for origins with x0 % 4 == 0 and for arbitrary origins,
and in the same run, alternated with it:

    (a) data.batch_from_cache on a dense [M,CH,CW,3] cache at the window's shape: the same output from pre-cropped images,
        which does less addressing work and reads every quad as three aligned dwords;
    (b) what one would write without the kernel, per role:
        paired_augment(u8_to_image(torch.stack([view[y0:y0 + CH, x0:x0 + CW] for each sample])))
        (one slice copy per sample inside the stack, csrc/image_io.hip, csrc/train_io.hip), at the arbitrary origins.

Every variant draws fresh random images and origins per call from seeded caches of random bytes of 384 MiB per role, past the
256 MiB Infinity Cache; the windows / index / origins are drawn before the clock starts, their upload is part of every variant.
Device events around back-to-back calls, every variant warmed up first, each timed window about `--window` seconds long.

Bytes: the new path moves 18 bytes per pixel and role as (a) does (3 read by the grey-mean pass, 3 read and 12 written by the
gather pass; the dwords around an unaligned quad add at most 4 bytes per 12 to what a lane asks for, on lines its neighbours ask
for anyway); GB/s is that count over the measured time.

    python tools/bench_dataset_crop.py [--rounds 5] [--window 0.5] [--out profiles/bench_dataset_crop.json]

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
from tools.bench_dataset import BYTES_PER_PIXEL, CACHE_BYTES, HBM_BPS, ROLES, _time_us  # noqa: E402

SHAPES = [(16, (256, 256), (512, 1024)), (8, (512, 1024), (1024, 2048))]      # N, window, image
SETS = 64


def _measure(N, crop, image, rounds, window, dev):
    (CH, CW), (Hi, Wi) = crop, image
    L = max(2 * N, CACHE_BYTES // (Hi * Wi * 3))                      # images per role; Hi * Wi * 3 is a multiple of 4
    M = (L * Hi * Wi) // (CH * CW)                                    # the same bytes read as a dense cache of windows
    gen = torch.Generator(device=dev).manual_seed(0)
    hazy = torch.randint(0, 256, (L * Hi * Wi * 3,), dtype=torch.uint8, device=dev, generator=gen)
    clear = torch.randint(0, 256, (L * Hi * Wi * 3,), dtype=torch.uint8, device=dev, generator=gen)
    dense = [c[:M * CH * CW * 3].view(M, CH, CW, 3) for c in (hazy, clear)]
    views = [[c[k * Hi * Wi * 3:(k + 1) * Hi * Wi * 3].view(Hi, Wi, 3) for k in range(L)] for c in (hazy, clear)]
    rng = np.random.RandomState(0)
    sizes = np.tile(np.array([[Hi, Wi]], np.int64), (N, 1))
    picks = [rng.randint(0, L, size=N) for _ in range(SETS)]
    origins = [D.draw_crop_origins(sizes, crop, rng) for _ in range(SETS)]
    aligned = [o // np.array([1, 4]) * np.array([1, 4]) for o in origins]
    win = {"windows_aligned_x0": [D.crop_windows(p * (Hi * Wi * 3), sizes, o) for p, o in zip(picks, aligned)],
           "windows_any_x0": [D.crop_windows(p * (Hi * Wi * 3), sizes, o) for p, o in zip(picks, origins)]}
    indices = [torch.from_numpy(rng.randint(0, M, size=N).astype(np.int64)) for _ in range(SETS)]
    params = [D.draw_augment_params(N, rng) for _ in range(SETS)]

    def windows(kind):
        return lambda i: D.batch_from_windows((hazy, clear), win[kind][i % SETS], crop, params[i % SETS])

    def dense_cache(i):
        return D.batch_from_cache(dense, indices[i % SETS], params[i % SETS])

    def slices(i):
        where = list(zip(picks[i % SETS].tolist(), origins[i % SETS].tolist()))
        roles = [IO.u8_to_image(torch.stack([v[k][y0:y0 + CH, x0:x0 + CW] for k, (y0, x0) in where])) for v in views]
        return D.paired_augment(roles, params[i % SETS])[0]
    fns = {"windows_aligned_x0": windows("windows_aligned_x0"), "windows_any_x0": windows("windows_any_x0"),
           "dense_cache": dense_cache, "slices": slices}
    max_diff = max(float((x - y).abs().max()) for x, y in zip(fns["windows_any_x0"](0), slices(0)))
    nbytes = ROLES * BYTES_PER_PIXEL * N * CH * CW
    calls = {}
    for k, fn in fns.items():                            # warm every variant at this shape, and size its window
        _time_us(fn, 20)
        calls[k] = max(50, int(window / (_time_us(fn, 50) * 1e-6)))
    us = {k: [] for k in fns}
    for _ in range(rounds):                              # alternate, so drift of the shared host hits all alike
        for k, fn in fns.items():
            us[k].append(_time_us(fn, calls[k]))
    med = {k: statistics.median(v) for k, v in us.items()}
    res = {"N": N, "window": [CH, CW], "image": [Hi, Wi], "images_per_role": L, "bytes_per_step_input": nbytes,
           "calls_per_sample": calls, "streaming_floor_us": round(nbytes / HBM_BPS * 1e6, 2),
           "max_abs_difference_from_slices": max_diff}
    for k in fns:
        res[k] = {"us": {"median": round(med[k], 2), "min": round(min(us[k]), 2), "max": round(max(us[k]), 2)},
                  "GBps": round(nbytes / med[k] * 1e-3, 1), "fraction_of_streaming_rate": round(nbytes / (med[k] * 1e-6) / HBM_BPS, 4)}
    for k in ("windows_aligned_x0", "windows_any_x0"):
        res[k]["over_dense_cache"] = round(med[k] / med["dense_cache"], 3)
        res[k]["slices_over_it"] = round(med["slices"] / med[k], 3)
        res[k]["beats_slices_beyond_the_spread"] = max(us[k]) < min(us["slices"])
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5, help="samples per variant, alternated")
    ap.add_argument("--window", type=float, default=0.5, help="seconds of back-to-back calls per sample")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_dataset_crop.py needs the GPU: there is no CPU timing to report")
    dev = "cuda:0"
    res = {"hbm_bytes_per_s": HBM_BPS, "samples": a.rounds, "window_s": a.window, "bytes_per_pixel_and_role": BYTES_PER_PIXEL,
           "roles": ROLES, "shapes": [_measure(N, crop, image, a.rounds, a.window, dev) for N, crop, image in SHAPES]}
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
