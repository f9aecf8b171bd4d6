"""Time the optimiser step of the joint model's parameter list (config/config.yaml: classifier + three branches, the branch
parameters listed twice) three ways, alternated in one process: the plain `adh_adam_multi` launch, the guarded step that only
measures (max_grad_norm = inf, skip_nonfinite on) and the guarded step that clips (max_grad_norm = half the gradient norm).
Then the two added launches alone against the rate the MI355X streams their algorithmic bytes at.  Device events, warm-up,
repeated launches; the gradients are fixed random tensors, so no forward or backward runs.

    python tools/bench_grad_clip.py [--steps 50] [--rounds 5] [--out profiles/bench_grad_clip.json]

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

from adam_dehaze_amd import _hip as H  # noqa: E402
from adam_dehaze_amd import train as T  # noqa: E402
from adam_dehaze_amd.optim import Adam  # noqa: E402

HBM_BPS = 6.3e12
ADAM_BYTES_PER_PARAM = 28      # p, m, v read and written, g read
SUMSQ_BYTES_PER_PARAM = 4      # g read once more


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


def _stats(v, digits=4):
    return {"median": round(statistics.median(v), digits), "min": round(min(v), digits), "max": round(max(v), digits)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50, help="optimiser steps per sample")
    ap.add_argument("--rounds", type=int, default=5, help="samples per variant, alternated")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--launches", type=int, default=200, help="launches per sample of the kernels timed alone")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_grad_clip.py needs the GPU: there is no CPU timing to report")
    import yaml
    dev = "cuda:0"
    cfg = yaml.safe_load(open(os.path.join(ROOT, "config", "config.yaml")))
    cfg["device"] = dev
    cfg["classifier"]["pretrained"] = False
    for k in ("classifier", "dehazing"):
        cfg[k]["checkpoint_dir"] = "/nonexistent"
    torch.manual_seed(0)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        listed = list(T.build_joint_system(cfg)["optimizer"]._listed)      # the reference's list, duplicates included
    gen = torch.Generator(device=dev).manual_seed(0)
    unique = list({id(p): p for p in listed}.values())
    for p in unique:
        p.grad = torch.randn(p.shape, device=dev, generator=gen) * 1e-3
    nparam = sum(p.numel() for p in unique)
    norm = float(torch.sqrt(sum(p.grad.double().pow(2).sum() for p in unique)))
    kw = dict(lr=cfg["joint_training"]["learning_rate"], weight_decay=1e-4)
    opts = {"unguarded": Adam(listed, **kw),
            "guarded_measure_only": Adam(listed, max_grad_norm=float("inf"), skip_nonfinite=True, **kw),
            "guarded_clipping": Adam(listed, max_grad_norm=0.5 * norm, skip_nonfinite=True, **kw)}
    for opt in opts.values():                            # warm every variant: table upload, code objects
        _time(opt.step, 0, a.warmup)
    ms = {k: [] for k in opts}
    for _ in range(a.rounds):                            # alternate, so drift of the shared host hits all alike
        for k, opt in opts.items():
            ms[k].append(_time(opt.step, 0, a.steps))
    clip = opts["guarded_clipping"]
    assert clip.skipped_steps() == 0 and abs(float(clip.last_grad_norm) - norm) <= 1e-5 * norm
    base = statistics.median(ms["unguarded"])
    res = {"tensors": len(unique), "listed": len(listed), "parameters": nparam, "chunks": clip._nchunks, "grad_norm": norm,
           "hbm_bytes_per_s": HBM_BPS, "steps_per_sample": a.steps, "samples": a.rounds,
           "optimiser_step_ms": {k: _stats(v) for k, v in ms.items()},
           "added_ms_median": {k: round(statistics.median(v) - base, 4) for k, v in ms.items() if k != "unguarded"},
           "adam_streaming_floor_ms": round(ADAM_BYTES_PER_PARAM * nparam / HBM_BPS * 1e3, 4)}

    def sumsq():
        H.call("adh_grad_sumsq", clip._table_dev.data_ptr(), clip._chunks_dev.data_ptr(), clip._nchunks, 1.0,
               clip._partials.data_ptr())

    def finalize():
        H.call("adh_grad_guard_finalize", clip._partials.data_ptr(), clip._nchunks, 1.0, 0.5 * norm, 1, clip._ctrl.data_ptr())

    for name, fn, nbytes in (("adh_grad_sumsq", sumsq, SUMSQ_BYTES_PER_PARAM * nparam),
                             ("adh_grad_guard_finalize", finalize, 8 * clip._nchunks)):
        us = [_time(fn, a.warmup, a.launches) * 1e3 for _ in range(a.rounds)]
        med = statistics.median(us)
        res[name] = {"us_per_launch": _stats(us, 2), "algorithmic_bytes": nbytes,
                     "streaming_floor_us": round(nbytes / HBM_BPS * 1e6, 2),
                     "fraction_of_streaming_rate": round(nbytes / (med * 1e-6) / HBM_BPS, 4)}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
