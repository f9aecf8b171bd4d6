"""Time the DenseNet121 HDEN train step (forward + cross-entropy + backward + Adam) at 16 x 3 x 256 x 256 (the reference's
classifier setting) and 8 x 3 x 512 x 1024 (the config-2 frame), with its eval forward and the resnet18 train step beside it:
device events, warm-ups, >= 20 timed steps.  Then one train step under a kernel timer: library launches per step, and each
DenseNet pass's algorithmic bytes and bytes/s against the ~6.3 TB/s the MI355X streams.

    python tools/bench_densenet.py [--steps 20] [--warmup 3] [--out profiles/bench_densenet.json]

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
from adam_dehaze_amd.optim import Adam  # noqa: E402

HBM_BPS = 6.3e12
SHAPES = ((16, 256, 256), (8, 512, 1024))
# the streaming passes of the pre-activation BatchNorms (bn_apply / bn_bwd_reduce also serve the other layers)
PASSES = ("adh_bn_slice_stats", "adh_bn_apply", "adh_bn_bwd_reduce", "adh_bn_preact_bwd_accum", "adh_avgpool2_bwd")


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


def _model(name, dev):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return CL.FogIntensityClassifier(name, 3, pretrained=False).to(dev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = "cuda:0"
    torch.manual_seed(0)
    res = {"steps": a.steps, "warmup": a.warmup, "hbm_bytes_per_s": HBM_BPS, "shapes": {}}
    for N, Hh, Ww in SHAPES:
        x = torch.rand(N, 3, Hh, Ww, device=dev)
        labels = torch.arange(N, device=dev) % 3
        entry = {}
        for name in ("densenet121", "resnet18"):
            m = _model(name, dev)
            opt = Adam(list(m.parameters()), lr=1e-4, weight_decay=1e-4)

            def step():
                opt.zero_grad()
                logits, _ = m(x)
                L.cross_entropy3(logits, labels).backward()
                opt.step()
            m.train()
            e = {"train_step_ms": round(_time(step, a.warmup, a.steps), 3)}
            e["images_per_s_train"] = round(N / e["train_step_ms"] * 1e3, 2)
            if name == "densenet121":
                timer = H.KernelTimer(set(H._SIGNATURES))
                H.TIMER = timer
                try:
                    step()
                finally:
                    H.TIMER = None
                agg = timer.summary()
                e["launches_per_step"] = sum(v["launches"] for v in agg.values())
                e["kernel_seconds_per_step"] = round(sum(v["seconds"] for v in agg.values()), 6)
                e["passes"] = {k: {"launches": agg[k]["launches"], "bytes": agg[k]["work"], "ms": round(agg[k]["seconds"] * 1e3, 3),
                                   "frac_hbm": round(agg[k]["work"] / agg[k]["seconds"] / HBM_BPS, 3) if agg[k]["seconds"] > 0
                                   else None} for k in PASSES if k in agg}
                m.eval()

                def fwd():
                    with torch.no_grad():
                        m(x)
                e["eval_forward_ms"] = round(_time(fwd, a.warmup, a.steps), 3)
            entry[name] = e
            del m, opt
            torch.cuda.empty_cache()
        res["shapes"][f"{N}x3x{Hh}x{Ww}"] = entry
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
