"""Time adh_d4_apply (csrc/d4.hip, d4.d4_apply) for each of the eight ops, plain and accumulating, at 8 x 3 x 512 x 1024 and
1 x 3 x 2160 x 3840, and in the same run, alternated with them:

  * a device-to-device copy that moves the same number of bytes (8 per element plain: one read, one write; 12 accumulating),
  * the torch chain the launch replaces: flip / transpose(-1, -2) / contiguous() for the plain form, and
    acc.add_(that).mul_(scale) for the accumulating one (the last launch of a self-ensemble).

GB/s is bytes the job has to move over the measured time, for the chains too (what they achieve of the job, not what their passes
move).  Every variant walks the same ring of buffer sets, sized past the 256 MiB Infinity Cache.  Device events around
back-to-back calls, warm-up first, samples alternated.  At each shape kernel and chain are compared once, bit for bit.

Then one end-to-end `d8` demo chunk (image_io._dehaze_on_device, the routed system at the widths of config/config.yaml with
random weights) against eight plain router passes of the same chunk, and the 15 D4 launches of that chunk on their own: the share
of the ensemble's time the transforms take.

    python tools/bench_d4.py [--rounds 5] [--out profiles/bench_d4.json] [--skip-demo]

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

from adam_dehaze_amd import d4 as D  # noqa: E402
from adam_dehaze_amd import image_io as IO  # noqa: E402

HBM_BPS = 6.29e12
RING_BYTES = 768 << 20          # buffer sets are added until they hold this much
SHAPES = [(8, 3, 512, 1024), (1, 3, 2160, 3840)]
SCALE = 0.125
DEMO_CHUNK = (2, 512, 1024)


def _time_us(fn, n):
    """mean microseconds per call of fn(i) over n back-to-back calls between two device events"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(n):
        fn(i)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / n


def chain(x, op):
    t = x.transpose(-1, -2) if op[0] else x
    dims = [d for d, bit in ((-1, 1), (-2, 2)) if op[1] & bit]
    return (t.flip(dims) if dims else t).contiguous() if (dims or op[0]) else t.clone()


def chain_acc(x, op, acc):
    t = x.transpose(-1, -2) if op[0] else x
    dims = [d for d, bit in ((-1, 1), (-2, 2)) if op[1] & bit]
    return acc.add_(t.flip(dims) if dims else t).mul_(SCALE)


def _stats(us, nbytes):
    med = statistics.median(us)
    return {"us": {"median": round(med, 2), "min": round(min(us), 2), "max": round(max(us), 2)},
            "GBps": round(nbytes / med * 1e-3, 1), "fraction_of_streaming_rate": round(nbytes / (med * 1e-6) / HBM_BPS, 4)}


def _measure(N, C, H, W, rounds, dev):
    n = N * C * H * W
    nsets = max(2, -(-RING_BYTES // (8 * n)))
    gen = torch.Generator(device=dev).manual_seed(0)
    src = [torch.rand((N, C, H, W), device=dev, generator=gen) for _ in range(nsets)]
    dst = {0: [torch.rand((N, C, H, W), device=dev, generator=gen) for _ in range(nsets)]}
    dst[1] = [d.view(N, C, W, H) for d in dst[0]]
    long_ = [(torch.empty(n + n // 2, device=dev), torch.empty(n + n // 2, device=dev)) for _ in range(nsets)]   # 12 bytes / element
    fns, nbytes, same = {}, {}, {}
    for op in D.D4_OPS:
        name = f"t{op[0]}f{op[1]}"
        fns[name] = lambda i, op=op: D.d4_apply(src[i % nsets], op, out=dst[op[0]][i % nsets])
        fns[name + "_torch"] = lambda i, op=op: chain(src[i % nsets], op)
        fns[name + "_acc"] = lambda i, op=op: D.d4_apply(src[i % nsets], op, out=dst[op[0]][i % nsets], accumulate=True, scale=SCALE)
        fns[name + "_acc_torch"] = lambda i, op=op: chain_acc(src[i % nsets], op, dst[op[0]][i % nsets])
        nbytes.update({name: 8 * n, name + "_torch": 8 * n, name + "_acc": 12 * n, name + "_acc_torch": 12 * n})
        a = D.d4_apply(src[0], op)
        old = dst[op[0]][1].clone()
        b = D.d4_apply(src[0], op, out=old.clone(), accumulate=True, scale=SCALE)
        same[name] = bool(torch.equal(a.view(torch.int32), chain(src[0], op).view(torch.int32))
                          and torch.equal(b.view(torch.int32), chain_acc(src[0], op, old.clone()).view(torch.int32)))
    fns["d2d_copy_8B"] = lambda i: dst[0][i % nsets].copy_(src[i % nsets])
    fns["d2d_copy_12B"] = lambda i: long_[i % nsets][1].copy_(long_[i % nsets][0])
    nbytes.update({"d2d_copy_8B": 8 * n, "d2d_copy_12B": 12 * n})
    calls = max(20, min(300, int(0.02 / (8 * n / HBM_BPS))))
    for fn in fns.values():                              # warm every variant at this shape: code objects, allocator
        _time_us(fn, max(3, nsets))
    us = {k: [] for k in fns}
    for _ in range(rounds):                              # alternate, so drift of the shared host hits all alike
        for k, fn in fns.items():
            us[k].append(_time_us(fn, calls))
    res = {"N": N, "C": C, "H": H, "W": W, "elements": n, "buffer_sets": nsets, "calls_per_sample": calls,
           "bit_equal_to_torch_chain": same, "variants": {k: _stats(us[k], nbytes[k]) for k in fns}}
    med = {k: statistics.median(v) for k, v in us.items()}
    res["ratios"] = {}
    for op in D.D4_OPS:
        name = f"t{op[0]}f{op[1]}"
        res["ratios"][name] = {"over_d2d_copy": round(med[name] / med["d2d_copy_8B"], 3),
                               "torch_over_kernel": round(med[name + "_torch"] / med[name], 3),
                               "acc_over_d2d_copy": round(med[name + "_acc"] / med["d2d_copy_12B"], 3),
                               "acc_torch_over_kernel": round(med[name + "_acc_torch"] / med[name + "_acc"], 3)}
    return res


def _demo(rounds, dev):
    import yaml
    from adam_dehaze_amd import train as T
    with open(os.path.join(ROOT, "config", "config.yaml")) as f:
        config = yaml.safe_load(f)
    config["device"] = dev
    config["classifier"]["pretrained"] = False
    for key in ("classifier", "dehazing", "joint_training"):
        config[key]["checkpoint_dir"] = "/nonexistent"
    torch.manual_seed(0)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        system = T._joint_system_for_evaluation(config)[0]
    N, H, W = DEMO_CHUNK
    u8 = torch.randint(0, 256, (N, H, W, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(1))
    x = IO.u8_to_image(u8.to(dev))
    y = torch.rand_like(x)
    acc = torch.empty_like(x)

    def plain8(i):
        with torch.no_grad():
            for _ in range(8):
                system["router"](x)

    def transforms(i):                                   # the 15 launches self_ensemble('d8') adds to the eight passes
        D.d4_apply(y, (0, 0), out=acc)
        for k, op in enumerate(D.D4_OPS[1:], 1):
            v = D.d4_apply(x, op)
            D.d4_apply(torch.empty_like(v) if op[0] else y, D.d4_inverse(op), out=acc, accumulate=True,
                       scale=SCALE if k == 7 else 1.0)

    fns = {"d8_chunk": lambda i: IO._dehaze_on_device(system, u8, False, self_ensemble="d8"),
           "plain_chunk": lambda i: IO._dehaze_on_device(system, u8, False),
           "eight_router_passes": plain8, "d4_launches_of_one_chunk": transforms}
    for fn in fns.values():
        _time_us(fn, 2)
    us = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            us[k].append(_time_us(fn, 3))
    med = {k: statistics.median(v) for k, v in us.items()}
    return {"chunk": {"N": N, "H": H, "W": W}, "routing": config["routing"]["type"],
            "us": {k: {"median": round(med[k], 1), "min": round(min(v), 1), "max": round(max(v), 1)} for k, v in us.items()},
            "d8_chunk_over_eight_router_passes": round(med["d8_chunk"] / med["eight_router_passes"], 4),
            "d4_share_of_d8_chunk": round(med["d4_launches_of_one_chunk"] / med["d8_chunk"], 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5, help="samples per variant, alternated")
    ap.add_argument("--out", default=None)
    ap.add_argument("--skip-demo", action="store_true", help="leave out the end-to-end d8 chunk")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_d4.py needs the GPU: there is no CPU timing to report")
    dev = "cuda:0"
    res = {"hbm_bytes_per_s": HBM_BPS, "samples": a.rounds, "accumulate_scale": SCALE,
           "shapes": [_measure(*s, a.rounds, dev) for s in SHAPES]}
    if not a.skip_demo:
        res["demo_d8"] = _demo(a.rounds, dev)
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
