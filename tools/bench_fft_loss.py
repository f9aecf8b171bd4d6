"""Time the frequency-domain L1 loss term (csrc/fft_loss.hip): adh_fft_l1 with and without the gradient at
8 x 3 x 512 x 1024 and 16 x 3 x 256 x 256 against the bytes its passes must move at the rate the MI355X streams, and the
Complex branch's training step with L1 alone against L1 + lambda_fft * frequency_l1, alternated in one process.  Device
events; warm-up, then 20 timed repetitions of a run of back-to-back launches.

    python tools/bench_fft_loss.py [--launches 20] [--repeats 20] [--steps 6] [--rounds 4] [--out profiles/bench_fft_loss.json]

Prints one JSON object (and writes it to --out when given).  --skip-step times the kernels only (the form to run under a
kernel trace, which gives the split between the passes)."""
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

HBM_BPS = 6.29e12
# bytes per image element (N * 3 * H * W of them) that the pass structure must move; the half spectrum of an image takes the
# bytes of the image (H * W/2 complex)
#   rows forward: pred and target read (8), half spectrum written (4)
#   columns:      half spectrum read (4); with the gradient, written back (4)
#   rows adjoint: half spectrum read (4), gradient written (4)
FWD_ONLY_BYTES = 8 + 4 + 4
FWD_BWD_BYTES = 8 + 4 + 4 + 4 + 4 + 4
SHAPES = [(8, 512, 1024), (16, 256, 256)]


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
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--base-channels", type=int, default=96)
    ap.add_argument("--lambda-fft", type=float, default=0.1)
    ap.add_argument("--skip-step", action="store_true", help="kernels only")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_fft_loss.py needs the GPU: there is no CPU timing to report")
    dev = "cuda:0"
    res = {"hbm_bytes_per_s": HBM_BPS, "launches_per_sample": a.launches, "samples": a.repeats, "shapes": {}}
    for N, Hh, Ww in SHAPES:
        gen = torch.Generator(device=dev).manual_seed(0)
        target = torch.rand(N, 3, Hh, Ww, device=dev, generator=gen)
        pred = (target + 0.05 * torch.randn(N, 3, Hh, Ww, device=dev, generator=gen)).clamp(0, 1)
        ws = torch.empty(H.value("adh_fft_l1_workspace_bytes", N, Hh, Ww) // 4, device=dev)
        part = torch.empty(H.value("adh_fft_l1_num_partials", N, Hh, Ww), device=dev, dtype=torch.float64)
        loss, grad = torch.empty((), device=dev), torch.empty_like(pred)

        def run(g):
            H.call("adh_fft_l1", pred.data_ptr(), target.data_ptr(), N, Hh, Ww, 0, ws.data_ptr(), part.data_ptr(), loss.data_ptr(), g)

        entry = {}
        for name, g, bpe in (("forward_backward", grad.data_ptr(), FWD_BWD_BYTES), ("forward_only", None, FWD_ONLY_BYTES)):
            us = [_time(lambda: run(g), a.warmup, a.launches) * 1e3 for _ in range(a.repeats)]
            med, nbytes = statistics.median(us), bpe * pred.numel()
            entry[name] = {"us_per_call_median": round(med, 2), "us_per_call_min": round(min(us), 2),
                           "us_per_call_max": round(max(us), 2), "algorithmic_bytes": nbytes,
                           "streaming_floor_us": round(nbytes / HBM_BPS * 1e6, 2),
                           "fraction_of_streaming_rate": round(nbytes / (med * 1e-6) / HBM_BPS, 4)}
        entry["loss"] = float(loss)
        res["shapes"][f"{N}x3x{Hh}x{Ww}"] = entry

    if not a.skip_step:
        N, Hh, Ww = SHAPES[0]
        gen = torch.Generator(device=dev).manual_seed(0)
        target = torch.rand(N, 3, Hh, Ww, device=dev, generator=gen)
        hazy = (target + 0.05 * torch.randn(N, 3, Hh, Ww, device=dev, generator=gen)).clamp(0, 1)
        torch.manual_seed(0)
        model = A.HighIntensityDehazeModel(base_channels=a.base_channels).to(dev).train()
        opt = Adam(model.parameters(), lr=1e-4, weight_decay=1e-4)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            crits = {"l1": L.DehazingLoss(content=False, perceptual=False).to(dev),
                     "l1_fft": L.DehazingLoss(content=False, perceptual=False, lambda_fft=a.lambda_fft).to(dev)}
        batch = {"hazy": hazy, "clear": target, "intensity": torch.zeros(N, dtype=torch.int64, device=dev)}
        ms = {k: [] for k in crits}
        for k, c in crits.items():                       # warm every shape both variants use
            _time(lambda: dehazing_train_step(model, c, opt, batch, None, torch.device(dev)), 0, 3)
        for _ in range(a.rounds):                        # alternate, so drift of the shared host hits both alike
            for k, c in crits.items():
                ms[k].append(_time(lambda: dehazing_train_step(model, c, opt, batch, None, torch.device(dev)), 0, a.steps))
        med = {k: statistics.median(v) for k, v in ms.items()}
        res["dehazing_train_step_complex"] = {
            "shape": [N, 3, Hh, Ww], "base_channels": a.base_channels, "lambda_fft": a.lambda_fft, "steps_per_sample": a.steps,
            "samples": a.rounds,
            **{k + "_ms": {"median": round(med[k], 3), "min": round(min(v), 3), "max": round(max(v), 3)} for k, v in ms.items()},
            "added_ms_median": round(med["l1_fft"] - med["l1"], 3),
            "added_share_of_step": round((med["l1_fft"] - med["l1"]) / med["l1"], 5)}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
