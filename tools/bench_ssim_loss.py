"""Time the SSIM loss term at 8 x 3 x 512 x 1024: the forward (adh_ssim_gray) and backward (adh_ssim_gray_bwd) launches
against the rate the MI355X streams their algorithmic bytes at, and the Complex branch's training step with L1 alone
against L1 + lambda_ssim * (1 - SSIM), alternated in one process.  Device events, warm-up, repeated launches.

    python tools/bench_ssim_loss.py [--launches 200] [--steps 6] [--rounds 4] [--out profiles/bench_ssim_loss.json]

Prints one JSON object (and writes it to --out when given)."""
import argparse
import json
import os
import statistics
import sys
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import adam_dehaze_amd as A  # noqa: E402
from adam_dehaze_amd import _hip as H  # noqa: E402
from adam_dehaze_amd import loss as L  # noqa: E402
from adam_dehaze_amd.optim import Adam  # noqa: E402
from adam_dehaze_amd.train import dehazing_train_step  # noqa: E402

HBM_BPS = 6.3e12
FWD_BYTES_PER_PIXEL = 24      # two 3-channel fp32 images read
BWD_BYTES_PER_PIXEL = 36      # two images read, one gradient image written


def _time(fn, warmup, n):
    """mean milliseconds per call of fn over n back-to-back calls between two device events."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--height", type=int, default=512)
    ap.add_argument("--width", type=int, default=1024)
    ap.add_argument("--base-channels", type=int, default=96)
    ap.add_argument("--lambda-ssim", type=float, default=0.2)
    ap.add_argument("--skip-step", action="store_true", help="kernels only")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_ssim_loss.py needs the GPU: there is no CPU timing to report")
    dev = "cuda:0"
    N, Hh, Ww = a.batch, a.height, a.width
    gen = torch.Generator(device=dev).manual_seed(0)
    target = torch.rand(N, 3, Hh, Ww, device=dev, generator=gen)
    pred = (target + 0.05 * torch.randn(N, 3, Hh, Ww, device=dev, generator=gen)).clamp(0, 1)
    pixels = N * Hh * Ww
    res = {"shape": [N, 3, Hh, Ww], "hbm_bytes_per_s": HBM_BPS, "launches_per_sample": a.launches, "samples": a.repeats}

    nblk = H.value("adh_ssim_num_blocks", Hh, Ww)
    partial = torch.empty(N * nblk, device=dev, dtype=torch.float64)
    ssim = torch.empty(N, device=dev)
    g = torch.full((N,), -0.2 / N, device=dev)
    gp = torch.empty_like(pred)

    def fwd():
        H.call("adh_ssim_gray", pred.data_ptr(), target.data_ptr(), N, Hh, Ww, 1.0, partial.data_ptr(), nblk, ssim.data_ptr())

    def bwd():
        H.call("adh_ssim_gray_bwd", pred.data_ptr(), target.data_ptr(), N, Hh, Ww, 1.0, g.data_ptr(), gp.data_ptr())

    for name, fn, bpp in (("adh_ssim_gray", fwd, FWD_BYTES_PER_PIXEL), ("adh_ssim_gray_bwd", bwd, BWD_BYTES_PER_PIXEL)):
        us = [_time(fn, a.warmup, a.launches) * 1e3 for _ in range(a.repeats)]
        med = statistics.median(us)
        res[name] = {"us_per_launch_median": round(med, 2), "us_per_launch_min": round(min(us), 2),
                     "us_per_launch_max": round(max(us), 2), "algorithmic_bytes": bpp * pixels,
                     "streaming_floor_us": round(bpp * pixels / HBM_BPS * 1e6, 2),
                     "fraction_of_streaming_rate": round(bpp * pixels / (med * 1e-6) / HBM_BPS, 4)}

    if not a.skip_step:
        torch.manual_seed(0)
        model = A.HighIntensityDehazeModel(base_channels=a.base_channels).to(dev).train()
        opt = Adam(model.parameters(), lr=1e-4, weight_decay=1e-4)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            crits = {"l1": L.DehazingLoss(content=False, perceptual=False).to(dev),
                     "l1_ssim": L.DehazingLoss(content=False, perceptual=False, lambda_ssim=a.lambda_ssim).to(dev)}
        batch = {"hazy": pred, "clear": target, "intensity": torch.zeros(N, dtype=torch.int64, device=dev)}
        ms = {k: [] for k in crits}
        for k, c in crits.items():                       # warm every shape both variants use
            _time(lambda: dehazing_train_step(model, c, opt, batch, None, torch.device(dev)), 0, a.warmup)
        for _ in range(a.rounds):                        # alternate, so drift of the shared host hits both alike
            for k, c in crits.items():
                ms[k].append(_time(lambda: dehazing_train_step(model, c, opt, batch, None, torch.device(dev)), 0, a.steps))
        res["dehazing_train_step_complex"] = {
            "base_channels": a.base_channels, "lambda_ssim": a.lambda_ssim, "steps_per_sample": a.steps, "samples": a.rounds,
            **{k + "_ms": {"median": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3)}
               for k, v in ms.items()},
            "added_ms_median": round(statistics.median(ms["l1_ssim"]) - statistics.median(ms["l1"]), 3)}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
