"""Time the weight EMA (ema.WeightEMA: `update()` = adh_ema_begin + adh_ema_multi, `applied()` = two adh_ema_swap) for two
parameter sets of config/config.yaml: the Complex (high-intensity) branch alone and the joint system (classifier + three
branches, every parameter once).  Next to each: the bytes the launches move (12 B per parameter for an update, 16 B per parameter
per swap), the time those bytes take at the streaming rate DESIGN uses, and the plain `adh_adam_multi` launch over the same set
(28 B per parameter) measured in the same run, alternated with the EMA samples.  Device events, warm-up, repeated launches; the
gradients are fixed random tensors, so no forward or backward runs.

    python tools/bench_ema.py [--launches 200] [--rounds 5] [--out profiles/bench_ema.json]

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

from adam_dehaze_amd import train as T  # noqa: E402
from adam_dehaze_amd.ema import WeightEMA  # noqa: E402
from adam_dehaze_amd.optim import Adam  # noqa: E402

HBM_BPS = 6.29e12
UPDATE_BYTES_PER_PARAM = 12    # p and ema read, ema written
SWAP_BYTES_PER_PARAM = 16      # p and ema read and written
ADAM_BYTES_PER_PARAM = 28      # p, m, v read and written, g read


def _time_us(fn, warmup, n):
    """mean microseconds per call of fn over n back-to-back calls between two device events."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / n


def _stats(v, digits=2):
    return {"median": round(statistics.median(v), digits), "min": round(min(v), digits), "max": round(max(v), digits)}


def _measure(params, a, dev):
    gen = torch.Generator(device=dev).manual_seed(0)
    for p in params:
        p.grad = torch.randn(p.shape, device=dev, generator=gen) * 1e-3
    nparam = sum(p.numel() for p in params)
    opt = Adam(params, lr=1e-4, weight_decay=1e-4)
    ema = WeightEMA(params, decay=0.999)

    def update():
        ema.update(opt)

    def round_trip():
        with ema.applied():
            pass

    fns = {"adam_multi": opt.step, "ema_update": update, "ema_applied_round_trip": round_trip}
    for fn in fns.values():                              # warm every variant: table upload, code objects
        _time_us(fn, 0, a.warmup)
    us = {k: [] for k in fns}
    for _ in range(a.rounds):                            # alternate, so drift of the shared host hits all alike
        for k, fn in fns.items():
            us[k].append(_time_us(fn, 0, a.launches))
    assert ema.updates() == a.warmup + a.rounds * a.launches and ema.uploads == 1
    nbytes = {"adam_multi": ADAM_BYTES_PER_PARAM * nparam, "ema_update": UPDATE_BYTES_PER_PARAM * nparam,
              "ema_applied_round_trip": 2 * SWAP_BYTES_PER_PARAM * nparam}
    out = {"tensors": len(params), "parameters": nparam, "chunks": ema._nchunks}
    for k in fns:
        med = statistics.median(us[k])
        out[k] = {"us_per_call": _stats(us[k]), "launches_per_call": {"adam_multi": 1}.get(k, 2), "algorithmic_bytes": nbytes[k],
                  "streaming_floor_us": round(nbytes[k] / HBM_BPS * 1e6, 2),
                  "fraction_of_streaming_rate": round(nbytes[k] / (med * 1e-6) / HBM_BPS, 4)}
    out["ema_update_over_adam_multi"] = round(statistics.median(us["ema_update"]) / statistics.median(us["adam_multi"]), 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=200, help="calls per sample")
    ap.add_argument("--rounds", type=int, default=5, help="samples per variant, alternated")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_ema.py needs the GPU: there is no CPU timing to report")
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
        system = T.build_joint_system(cfg)
    res = {"hbm_bytes_per_s": HBM_BPS, "launches_per_sample": a.launches, "samples": a.rounds,
           "bytes_per_parameter": {"ema_update": UPDATE_BYTES_PER_PARAM, "ema_swap": SWAP_BYTES_PER_PARAM,
                                   "adam_multi": ADAM_BYTES_PER_PARAM},
           "complex_branch": _measure(list(system["models"]["high"].parameters()), a, dev),
           "joint_system": _measure(list(system["router"].parameters()), a, dev)}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
