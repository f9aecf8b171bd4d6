"""Time the MobileNet HDEN backbones at 8 x 3 x 512 x 1024 next to resnet18: eval forward and train forward + backward
(dropout on, cross-entropy), device events, 5 warm-ups, >= 20 timed steps; then the depthwise launches of one train step
with their algorithmic bytes (read x once, write y once) and bytes/s against the ~6.3 TB/s the MI355X streams.

    python tools/bench_mobilenet.py [--steps 20] [--batch 8] [--out profiles/bench_mobilenet.json]

Prints one JSON object (and writes it to --out when given)."""
import argparse
import json
import os
import sys
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from adam_dehaze_amd import _hip as H  # noqa: E402
from adam_dehaze_amd import classifier as CL  # noqa: E402
from adam_dehaze_amd import loss as L  # noqa: E402

HBM_BPS = 6.3e12
NAMES = ("resnet18", "mobilenet_v2", "mobilenet_v3_large", "mobilenet_v3_small")
DW_CALLS = ("adh_dwconv_fwd", "adh_dwconv_dgrad", "adh_dwconv_wgrad")


def _time(fn, warmup, steps):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--height", type=int, default=512)
    ap.add_argument("--width", type=int, default=1024)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = "cuda:0"
    torch.manual_seed(0)
    x = torch.rand(a.batch, 3, a.height, a.width, device=dev)
    labels = torch.arange(a.batch, device=dev) % 3
    res = {"shape": [a.batch, 3, a.height, a.width], "steps": a.steps, "warmup": a.warmup, "hbm_bytes_per_s": HBM_BPS,
           "models": {}}
    for name in NAMES:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            m = CL.FogIntensityClassifier(name, 3, pretrained=False).to(dev)
        m.eval()

        def fwd():
            with torch.no_grad():
                m(x)
        eval_ms = _time(fwd, a.warmup, a.steps)
        m.train()

        def step():
            for p in m.parameters():
                p.grad = None
            logits, _ = m(x)
            L.cross_entropy3(logits, labels).backward()
        train_ms = _time(step, a.warmup, a.steps)
        entry = {"eval_forward_ms": round(eval_ms, 3), "train_step_ms": round(train_ms, 3),
                 "images_per_s_train": round(a.batch / train_ms * 1e3, 2)}
        if name != "resnet18":
            # per-launch bytes/s of the depthwise kernels in one train step
            timer = H.KernelTimer(DW_CALLS)
            H.TIMER = timer
            try:
                step()
            finally:
                H.TIMER = None
            torch.cuda.synchronize()
            launches = []
            for call, e0, e1, work, _ in timer.records:
                sec = e0.elapsed_time(e1) * 1e-3
                launches.append({"call": call, "bytes": work, "us": round(sec * 1e6, 1),
                                 "frac_hbm": round(work / sec / HBM_BPS, 3) if sec > 0 else None})
            entry["depthwise_launches"] = launches
            top = sorted((ln for ln in launches if ln["call"] != "adh_dwconv_wgrad"), key=lambda ln: -ln["bytes"])[:6]
            entry["largest_fwd_dgrad_frac_hbm"] = [(ln["call"], ln["bytes"], ln["frac_hbm"]) for ln in top]
        res["models"][name] = entry
        del m
        torch.cuda.empty_cache()
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
