"""Time one training step's input when the hazy role is synthesized from clear pixels and depth maps (data.batch_haze_from_windows
on csrc/dataset.hip's adh_batch_haze_from_u8, plus data.batch_from_windows for the clear role; both augmented with one parameter
row per sample, uploads included) at 16 x 256 x 256 windows out of 512 x 1024 images and 8 x 512 x 1024 out of 1024 x 2048, and in
the same run, alternated with it:

    (a) stored pairs: data.batch_from_windows((hazy, clear)) at the same windows, what a step's input costs when the hazy files
        exist, and its hazy half alone next to the synthesized role alone;
    (b) the composition one would write without the kernel: batch_from_windows(clear) without rows, the depth windows stacked by
        torch slices, the scattering model as float32 torch expressions (no float64), then data.paired_augment on both roles.

Every variant draws fresh random images and origins per call from seeded caches of random bytes of 384 MiB per role, past the
256 MiB Infinity Cache; the windows, rows and (beta, A) are drawn before the clock starts, their upload is part of every variant.
Device events around back-to-back calls, every variant warmed up first, each timed window about `--window` seconds long, the
variants alternated so that drift of a shared host hits all alike; median, minimum and maximum over `--rounds` windows.

    python tools/bench_haze_synth.py [--rounds 5] [--window 0.5] [--out profiles/bench_haze_synth.json]

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
from tools.bench_dataset import CACHE_BYTES, _time_us  # noqa: E402

SHAPES = [(16, (256, 256), (512, 1024)), (8, (512, 1024), (1024, 2048))]      # N, window, image
SETS = 64
RANGE = (0.3, 1.0)


def _measure(N, crop, image, rounds, window, dev):
    (CH, CW), (Hi, Wi) = crop, image
    L = max(2 * N, CACHE_BYTES // (Hi * Wi * 3))                      # images per role; Hi * Wi is a multiple of 4
    gen = torch.Generator(device=dev).manual_seed(0)
    hazy = torch.randint(0, 256, (L * Hi * Wi * 3,), dtype=torch.uint8, device=dev, generator=gen)
    clear = torch.randint(0, 256, (L * Hi * Wi * 3,), dtype=torch.uint8, device=dev, generator=gen)
    depth = torch.randint(-32768, 32768, (L * Hi * Wi,), dtype=torch.int16, device=dev, generator=gen).view(torch.uint16)
    dviews = [depth.view(torch.int16)[k * Hi * Wi:(k + 1) * Hi * Wi].view(Hi, Wi) for k in range(L)]
    rng = np.random.RandomState(0)
    sizes = np.tile(np.array([[Hi, Wi]], np.int64), (N, 1))
    picks = [rng.randint(0, L, size=N) for _ in range(SETS)]
    origins = [D.draw_crop_origins(sizes, crop, rng) for _ in range(SETS)]
    wins = [D.crop_windows(p * (Hi * Wi * 3), sizes, o) for p, o in zip(picks, origins)]
    geoms = [torch.cat([w, torch.stack([w[:, 0] // 3 * 2, w[:, 1] // 3 * 2], 1)], 1).contiguous() for w in wins]
    params = [D.draw_augment_params(N, rng) for _ in range(SETS)]
    fogs = [D.draw_haze_params(N, rng)[1] for _ in range(SETS)]

    def synthesized(i, d=depth):
        k = i % SETS
        return [D.batch_haze_from_windows(clear, d, geoms[k], fogs[k], crop, params[k], RANGE),
                D.batch_from_windows(clear, wins[k], crop, params[k])]

    def role(i):
        k = i % SETS
        return D.batch_haze_from_windows(clear, depth, geoms[k], fogs[k], crop, params[k], RANGE)

    def stored_pair(i):
        return D.batch_from_windows((hazy, clear), wins[i % SETS], crop, params[i % SETS])

    def stored_role(i):
        return D.batch_from_windows(hazy, wins[i % SETS], crop, params[i % SETS])

    def composition(i):
        k = i % SETS
        J = D.batch_from_windows(clear, wins[k], crop)
        lev = torch.stack([dviews[p][y0:y0 + CH, x0:x0 + CW] for p, (y0, x0) in zip(picks[k].tolist(), origins[k].tolist())]).float()
        lev = torch.where(lev < 0, lev + 65536.0, lev)               # the int16 view of the uint16 levels
        fog = fogs[k].to(dev)
        t = torch.exp(-fog[:, 0].view(N, 1, 1, 1) * (RANGE[0] + (RANGE[1] - RANGE[0]) * (lev / 65535.0)).unsqueeze(1))
        hz = (J * t + fog[:, 1].view(N, 1, 1, 1) * (1 - t)).clamp_(0, 1)
        return D.paired_augment([hz, J], params[k])[0]
    fns = {"synthesized": synthesized, "synthesized_radial": lambda i: synthesized(i, None), "stored_pair": stored_pair,
           "composition": composition, "synthesized_role": role, "stored_role": stored_role}
    max_diff = max(float((x - y).abs().max()) for x, y in zip(synthesized(0), composition(0)))
    calls = {}
    for k, fn in fns.items():                            # warm every variant at this shape, and size its window
        _time_us(fn, 20)
        calls[k] = max(50, int(window / (_time_us(fn, 50) * 1e-6)))
    us = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            us[k].append(_time_us(fn, calls[k]))
    med = {k: statistics.median(v) for k, v in us.items()}
    res = {"N": N, "window": [CH, CW], "image": [Hi, Wi], "images_per_role": L, "calls_per_sample": calls,
           "max_abs_difference_from_composition": max_diff}
    for k in fns:
        res[k] = {"us": {"median": round(med[k], 2), "min": round(min(us[k]), 2), "max": round(max(us[k]), 2)}}
    for k in ("synthesized", "synthesized_radial"):
        res[k]["over_stored_pair"] = round(med[k] / med["stored_pair"], 3)
        res[k]["composition_over_it"] = round(med["composition"] / med[k], 3)
        res[k]["beats_composition_beyond_the_spread"] = max(us[k]) < min(us["composition"])
    res["synthesized_role"]["over_stored_role"] = round(med["synthesized_role"] / med["stored_role"], 3)
    res["synthesized_role"]["ns_per_pixel"] = round(med["synthesized_role"] * 1e3 / (N * CH * CW), 4)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5, help="samples per variant, alternated")
    ap.add_argument("--window", type=float, default=0.5, help="seconds of back-to-back calls per sample")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_haze_synth.py needs the GPU: there is no CPU timing to report")
    dev = "cuda:0"
    res = {"samples": a.rounds, "window_s": a.window, "depth_range": list(RANGE),
           "shapes": [_measure(N, crop, image, a.rounds, a.window, dev) for N, crop, image in SHAPES]}
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
