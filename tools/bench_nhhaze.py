"""Time the hazy role of a training step under patchy, wavelength-dependent haze (data.batch_nhhaze_from_windows on csrc/dataset.hip's
adh_batch_nhhaze_from_u8; one parameter row per sample, uploads included) at the two shapes of tools/bench_haze_synth.py, 16 x 256 x
256 windows out of 512 x 1024 images and 8 x 512 x 1024 out of 1024 x 2048, and in the same run, alternated with it:

    (i)   uniform:      data.batch_haze_from_windows (adh_batch_haze_from_u8) from the same build;
    (ii)  patchy_k1, patchy_k3 (one and three octaves, grey), chromatic (no field: s = 0, one octave), both (three octaves);
    (iii) composition:  the same formulas in torch: the float64 field by integer and float expressions on the device (the hash in
          int64 with 32-bit masks), the model in float64, then data.paired_augment.

The method is bench_haze_synth.py's: fresh random images, origins, rows and haze per call from seeded caches of random bytes past
the Infinity Cache, drawn before the clock starts (their upload is part of every variant); device events around back-to-back
calls, every variant warmed up first, each timed window about `--window` seconds long, the variants alternated; median, minimum
and maximum over `--rounds` windows.

    python tools/bench_nhhaze.py [--rounds 5] [--window 0.5] [--label TEXT] [--out profiles/bench_nhhaze.json]

Prints one JSON object (and writes it to --out when given).  `--label` is copied into it (which build of the library ran)."""
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
from tools.bench_haze_synth import RANGE, SETS, SHAPES  # noqa: E402

M32 = 0xFFFFFFFF


def torch_hash(ix, iy, k, seed):
    """the lattice hash on int64 tensors of values below 2^31 (products wrap modulo 2^64: the low 32 bits are those of uint32)"""
    h = ((ix * 0x9E3779B1) & M32) ^ ((iy * 0x85EBCA77) & M32) ^ ((k * 0xC2B2AE3D) & M32) ^ seed
    h = h ^ (h >> 16)
    h = (h * 0x7FEB352D) & M32
    h = h ^ (h >> 15)
    h = (h * 0x846CA68B) & M32
    return h ^ (h >> 16)


def torch_field(field, CH, CW, K):
    """float64 [N, CH, CW] on the device of `field` (float64 [N, 6], every row with K octaves)"""
    dev = field.device
    seed = field[:, 0].to(torch.int64).view(-1, 1, 1)
    y = (torch.arange(CH, device=dev).view(1, CH, 1) + field[:, 1].to(torch.int64).view(-1, 1, 1)).double()
    x = (torch.arange(CW, device=dev).view(1, 1, CW) + field[:, 2].to(torch.int64).view(-1, 1, 1)).double()
    f0 = field[:, 5].view(-1, 1, 1)
    acc, norm = 0.0, 0.0
    for k in range(K):
        fk = f0 * 2.0 ** k
        py, px = y * fk, x * fk
        fy, fx = torch.floor(py), torch.floor(px)
        uy, ux = py - fy, px - fx
        wy, wx = uy * uy * (3.0 - 2.0 * uy), ux * ux * (3.0 - 2.0 * ux)
        iy, ix = fy.to(torch.int64), fx.to(torch.int64)
        v00, v01 = torch_hash(ix, iy, k, seed).double() / 4294967296.0, torch_hash(ix + 1, iy, k, seed).double() / 4294967296.0
        v10, v11 = torch_hash(ix, iy + 1, k, seed).double() / 4294967296.0, torch_hash(ix + 1, iy + 1, k, seed).double() / 4294967296.0
        top, bot = v00 + wx * (v01 - v00), v10 + wx * (v11 - v10)
        acc = acc + 2.0 ** -k * (top + wy * (bot - top))
        norm += 2.0 ** -k
    return acc / norm


def _measure(N, crop, image, rounds, window, dev):
    (CH, CW), (Hi, Wi) = crop, image
    L = max(2 * N, CACHE_BYTES // (Hi * Wi * 3))                      # images; Hi * Wi is a multiple of 4
    gen = torch.Generator(device=dev).manual_seed(0)
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
    k1, k3 = D._nh_settings("nonuniform", {"octaves": 1}), D._nh_settings("nonuniform", {})
    ch = D._nh_settings("chromatic", {})
    modes = {"patchy_k1": (k1, None), "patchy_k3": (k3, None), "chromatic": (None, ch), "both": (k3, ch)}
    drawn = {m: [D.draw_nh_params(N, rng, nu, c, sizes, o, f) for o, f in zip(origins, fogs)] for m, (nu, c) in modes.items()}

    def uniform(i):
        k = i % SETS
        return D.batch_haze_from_windows(clear, depth, geoms[k], fogs[k], crop, params[k], RANGE)

    def kernel(mode):
        def run(i):
            k = i % SETS
            fog6, field = drawn[mode][k]
            return D.batch_nhhaze_from_windows(clear, depth, geoms[k], fog6, field, crop, params[k], RANGE)
        return run

    def composition(i, mode="both"):
        k = i % SETS
        fog6, field = drawn[mode][k]
        fog6, field = fog6.to(dev).double(), field.to(dev)
        J = D.batch_from_windows(clear, wins[k], crop)
        lev = torch.stack([dviews[p][y0:y0 + CH, x0:x0 + CW] for p, (y0, x0) in zip(picks[k].tolist(), origins[k].tolist())]).double()
        lev = torch.where(lev < 0, lev + 65536.0, lev)               # the int16 view of the uint16 levels
        d = (RANGE[0] + (RANGE[1] - RANGE[0]) * (lev / 65535.0)).unsqueeze(1)
        m = 1.0 + field[:, 4].view(N, 1, 1) * (2.0 * torch_field(field, CH, CW, int(field[0, 3])) - 1.0)
        t = torch.exp(-((fog6[:, :3].view(N, 3, 1, 1) * m.unsqueeze(1)) * d))
        hz = (J.double() * t + fog6[:, 3:].view(N, 3, 1, 1) * (1.0 - t)).clamp_(0, 1).float()
        return D.paired_augment([hz], params[k])[0]
    fns = {"uniform": uniform, **{m: kernel(m) for m in modes}, "composition": composition}
    max_diff = {m: float((kernel(m)(0) - composition(0, m)[0]).abs().max()) for m in modes}
    calls = {}
    for k, fn in fns.items():                            # warm every variant at this shape, and size its window
        _time_us(fn, 20)
        calls[k] = max(20, int(window / (_time_us(fn, 20) * 1e-6)))
    us = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            us[k].append(_time_us(fn, calls[k]))
    med = {k: statistics.median(v) for k, v in us.items()}
    px = N * CH * CW
    res = {"N": N, "window": [CH, CW], "image": [Hi, Wi], "images": L, "calls_per_sample": calls,
           "max_abs_difference_from_composition": max_diff}
    for k in fns:
        res[k] = {"us": {"median": round(med[k], 2), "min": round(min(us[k]), 2), "max": round(max(us[k]), 2)},
                  "ns_per_pixel": round(med[k] * 1e3 / px, 4)}
    for m in modes:
        res[m]["over_uniform"] = round(med[m] / med["uniform"], 3)
        res[m]["added_ns_per_pixel_and_pass"] = round((med[m] - med["uniform"]) * 1e3 / px / 2, 4)   # mean pass + gather pass
        res[m]["composition_over_it"] = round(med["composition"] / med[m], 3)
        res[m]["beats_composition_beyond_the_spread"] = max(us[m]) < min(us["composition"])
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5, help="samples per variant, alternated")
    ap.add_argument("--window", type=float, default=0.5, help="seconds of back-to-back calls per sample")
    ap.add_argument("--label", default=None, help="copied into the result: which build of the library ran")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_nhhaze.py needs the GPU: there is no CPU timing to report")
    dev = "cuda:0"
    res = {"label": a.label, "samples": a.rounds, "window_s": a.window, "depth_range": list(RANGE),
           "composition_is": "both (three octaves, chromatic)",
           "shapes": [_measure(N, crop, image, a.rounds, a.window, dev) for N, crop, image in SHAPES]}
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
