#!/usr/bin/env python3
"""Bit-for-bit A/B of the weight-gradient reduce stage between two builds of libadamdehaze_hip.so.

    python tools/wgrad_reduce_ab.py                    digests of the library ADH_LIB_PATH names (default: the tree's own)
    python tools/wgrad_reduce_ab.py --ab OTHER.so      the same in two fresh child processes, OTHER.so and the tree's own,
                                                       and a line-by-line comparison (exit status 1 when a line differs)

A digest line is `<case> <SHA-256 of the result's bytes>`.  Cases: every reduce entry point called directly on seeded slabs
(the cases of tests/_wgrad_reduce_ref.py, accumulate 0 and 1, one and several splits), and Engine._wgrad on one shape per
weight-gradient family from seeded inputs (F(4x4,3x3), F(2x2,3x3), F(3x3,2x2) per class / merged classes / four-class form,
row-split, general, few-channel, 7x7 stem on both of its paths)."""
import argparse
import ctypes as C
import hashlib
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def digests():
    import numpy as np
    import torch
    import adam_dehaze_amd.engine as E
    from adam_dehaze_amd import _hip as H
    from adam_dehaze_amd.engine import Act, Engine
    from tests import _wgrad_reduce_ref as R
    dev = torch.device("cuda:0")

    def sha(t):
        torch.cuda.synchronize()
        return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()

    def entry(name, cs, nsplit, acc, desc=None):
        slab = torch.from_numpy(cs.slab(7, nsplit)).to(dev)
        dst = torch.from_numpy(R.rng_dst(7, cs.ndst, 1)).to(dev)      # seeded: skipped elements hash the same
        L = H.WLayout(*cs.L)
        pre = (nsplit,) if desc is None else (nsplit, C.byref(desc))
        H.call(cs.entry, slab.data_ptr(), *pre, R.KP, R.NCP, C.byref(L), dst.data_ptr(), acc)
        print(f"{name}/K{cs.L.K}/nsplit{nsplit}/acc{acc} {sha(dst)}", flush=True)

    def desc32(KH, in_s, out_s, dstep):
        d = H.ConvDesc()
        d.N, d.Cin, d.in_cstride, d.Cout, d.out_cstride, d.NcP = 1, 32, 32, 32, 32, 32
        d.VH = d.VW = 4
        d.IH = d.IW = 4 * in_s
        d.OH = d.OW = 4 * out_s
        d.in_sy = d.in_sx = in_s
        d.out_sy = d.out_sx = out_s
        d.KH = d.KW = KH
        d.dy0 = d.dx0 = -1 if dstep > 0 else 0
        d.dstep_y = d.dstep_x = dstep
        return d

    os.environ["ADH_WINO32_WGRAD"] = "2"        # the four-class form is taken only when asked
    for acc in (0, 1):
        for K, Nc in R.SIZES:
            for ns in (1, 7):
                entry("reduce", R.case("adh_wgrad_reduce", K, Nc, 3, reverse=True), ns, acc)
                entry("reduce16", R.case("adh_wgrad_reduce", K, Nc, 4), ns, acc)
            for ns in (1, 130):
                entry("small", R.case("adh_wgrad_reduce_small", K, Nc, 3, reverse=True), ns, acc)
            for ns in (1, 2, 37):
                entry("wino", R.case("adh_wgrad_reduce_wino", K, Nc, 3, reverse=True), ns, acc)
                entry("wino43", R.case("adh_wgrad_reduce_wino43", K, Nc, 3), ns, acc)
                entry("wino32conv", R.case("adh_wgrad_reduce_wino32", K, Nc, 4, classes=R.CONV_K4S2_CLASSES), ns, acc,
                      desc32(4, 2, 1, 1))
                entry("wino32convT", R.case("adh_wgrad_reduce_wino32", K, Nc, 2, reverse=True, classes=R.CONVT_CLASS), ns, acc,
                      desc32(2, 1, 2, -1))
        for ns in (1, 2, 3):
            slab = torch.from_numpy(R.rng_slab(9, ns, 14, 32, R.NCP)).to(dev)
            dst = torch.from_numpy(R.rng_dst(9, 5 * 3 * 49, 1)).to(dev)
            H.call("adh_wgrad_reduce_packed", slab.data_ptr(), ns, R.NCP, 3, 7, 7, 5, dst.data_ptr(), acc)
            print(f"packed/nsplit{ns}/acc{acc} {sha(dst)}", flush=True)
    del os.environ["ADH_WINO32_WGRAD"]

    def randn(*shape, seed):
        return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)).to(dev)

    def family(name, kind, k, stride, pad, Ci, Co, Hh, Ww, N=1, xalloc=None, xC=None, nsplit=None):
        """Engine._wgrad of one layer: x [N, Hh, Ww, Ci], dL/dy on the layer's output grid"""
        if nsplit is not None:
            os.environ["ADH_NSPLIT"] = str(nsplit)
        try:
            eng = Engine(dev, record=False)
            w = torch.zeros((Co, Ci, k, k) if kind == "conv" else (Ci, Co, k, k), device=dev, requires_grad=True)
            x = torch.zeros(N, Hh, Ww, xalloc or Ci, device=dev)
            x[..., :Ci] = randn(N, Hh, Ww, Ci, seed=1)
            oh, ow = ((Hh + 2 * pad - k) // stride + 1, (Ww + 2 * pad - k) // stride + 1) if kind == "conv" else (2 * Hh, 2 * Ww)
            g = randn(N, oh, ow, (Co + 3) // 4 * 4, seed=2)
            g[..., Co:] = 0
            plans = eng._launch_plan(kind, k, stride, pad, w, "fwd")
            dw = eng._wgrad(plans, Act(x, xC or Ci), g, Co, w)
            print(f"engine/{name} {sha(dw)}", flush=True)
        finally:
            os.environ.pop("ADH_NSPLIT", None)

    family("f43", "conv", 3, 1, 1, 32, 96, 16, 32, N=2)
    family("f43/nsplit5", "conv", 3, 1, 1, 32, 96, 16, 32, N=2, nsplit=5)
    family("f23", "conv", 3, 1, 1, 32, 64, 8, 32, N=2)
    family("f23/nsplit3", "conv", 3, 1, 1, 32, 64, 8, 32, N=2, nsplit=3)
    family("f32-classes", "convT", 4, 2, 1, 32, 32, 9, 50)
    family("f32-merged", "convT", 4, 2, 1, 64, 96, 12, 48)
    family("f32-merged/nsplit3", "convT", 4, 2, 1, 64, 96, 12, 48, nsplit=3)
    family("f32-conv-v2", "conv", 4, 2, 1, 192, 96, 24, 100)
    family("rows", "conv", 4, 2, 1, 32, 64, 16, 128)
    family("rows/nsplit3", "conv", 4, 2, 1, 32, 64, 16, 128, nsplit=3)
    family("general", "conv", 3, 1, 1, 32, 32, 7, 9, N=2)
    family("small", "conv", 3, 1, 1, 3, 16, 12, 70, xalloc=8)
    family("fewout", "conv", 3, 1, 1, 48, 3, 12, 70)
    family("stem", "conv", 7, 1, 3, 3, 64, 12, 70, xalloc=8, xC=8)
    E.USE_SMALL_WGRAD = False
    family("stem-packed", "conv", 7, 1, 3, 3, 64, 12, 70, xalloc=8, xC=8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ab", metavar="OTHER.so", help="compare the tree's library with this build of it")
    a = ap.parse_args()
    if not a.ab:
        return digests()
    out = []
    for tag, lib in (("other", os.path.abspath(a.ab)), ("this", None)):
        env = dict(os.environ)
        env.pop("ADH_LIB_PATH", None)
        if lib:
            env["ADH_LIB_PATH"] = lib
        r = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, capture_output=True, text=True, timeout=240)
        if r.returncode:
            print(f"{tag}: child failed with status {r.returncode}\n{r.stdout[-3000:]}\n{r.stderr[-3000:]}")
            return 2
        out.append(r.stdout.splitlines())
    other, this = out
    print(f"# {len(other)} digests of OTHER.so, {len(this)} of this tree's library")
    bad = len(other) != len(this)
    for x, y in zip(other, this):
        if x == y:
            print(y)
        else:
            bad = True
            print(f"DIFFERENT other: {x}\nDIFFERENT this:  {y}")
    print("# RESULT:", "DIFFERENT" if bad else f"all {len(this)} digests equal, line for line")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
