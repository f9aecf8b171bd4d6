"""csrc/conv_wgrad_reduce.hip without a GPU: the source file, compiled by the host C++ compiler against the stand-in header of
tools/host_emu (its ADH_HOST_EMU section) with AddressSanitizer and UndefinedBehaviorSanitizer, run as a stand-alone program
on heap buffers of exactly their sizes and held to the float64 reference and the bound of tests/_wgrad_reduce_ref.py -- the
ones tests/test_gpu_wgrad_reduce.py holds the library to.  It runs the index decode, the split sums, the inverse transforms
and the layout scatter (negative tap strides included) of the very source the GPU runs under the sanitizers.  The class taps
of the wino32 form, which conv_wgrad32.hip derives from a descriptor, are given by the case.  The one-wave-per-element kernel
(adh_wgrad_reduce_small: csrc/wave.h's wave_sum on the emulator's __shfl_xor) runs in a second program of the same source, on
the streaming runtime (tools/host_emu/stream_rt.cpp, wgrad_reduce_small_main.cpp; tests/_hostemu.py)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import _hostemu as E
from tests import _wgrad_reduce_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_ID = {"adh_wgrad_reduce": 0, "adh_wgrad_reduce_packed": 2, "adh_wgrad_reduce_wino": 3, "adh_wgrad_reduce_wino32": 4,
            "adh_wgrad_reduce_wino43": 5}
ADH_E_ARG = -1


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler found"
    d = tmp_path_factory.mktemp("wgrad_reduce_emu")
    shutil.copy(os.path.join(ROOT, "adam-dehaze_amd", "csrc", "conv_wgrad_reduce.hip"), d / "conv_wgrad_reduce.cpp")
    for fn in ("common.h", "wgrad_reduce_main.cpp"):       # the copy's #include "common.h" finds the stand-in next to it
        shutil.copy(os.path.join(ROOT, "tools", "host_emu", fn), d / fn)
    exe = d / "wgrad_reduce_emu"
    subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-DADH_HOST_EMU", "-I", os.path.join(ROOT, "include"),
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wno-unknown-pragmas", "-pthread",
                    str(d / "conv_wgrad_reduce.cpp"), str(d / "wgrad_reduce_main.cpp"), "-o", str(exe)], check=True, cwd=d)

    def run(entry, slab, dst0, nsplit, L=None, accumulate=0, packed=(0, 0, 0, 0), classes=(), ncp=R.NCP, null_slab=False):
        h = np.zeros(40, np.int32)
        h[0:4] = ENTRY_ID[entry], nsplit, R.KP, ncp
        if L is not None:
            h[4:13] = L
        h[13:16] = accumulate, dst0.size, slab.size
        h[16:20] = packed
        h[20] = len(classes)
        for c, cl in enumerate(classes):
            h[21 + c], h[25 + c], h[29 + c], h[33 + c] = cl
        h[37] = int(null_slab)
        with open(d / "in.bin", "wb") as f:
            f.write(h.tobytes() + np.ascontiguousarray(slab, np.float32).tobytes() + dst0.tobytes())
        r = subprocess.run([str(exe), str(d / "in.bin"), str(d / "out.bin")], capture_output=True, text=True)
        assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
        out = np.fromfile(d / "out.bin", dtype=np.int32)
        return int(out[0]), out[1:].view(np.float32).copy()
    return run


def _run_case(emu, cs, nsplit, accumulate, seed):
    slab = cs.slab(seed, nsplit)
    dst0 = R.rng_dst(seed, cs.ndst, accumulate)
    rc, got = emu(cs.entry, slab, dst0, nsplit, cs.L, accumulate, classes=cs.classes)
    assert rc == 0
    ref, bound, written = R.reference(slab, cs.M, cs.c, cs.L, cs.taps, dst0, accumulate)
    R.check(got, dst0, ref, bound, written, f"{cs.entry} K={cs.L.K} Nc={cs.L.Nc} taps={cs.L.KHt} nsplit={nsplit} acc={accumulate}")


@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("K,Nc", R.SIZES)
def test_direct_reduce_reversed_taps(emu, K, Nc, accumulate):
    for KH, nsplit in ((1, 1), (2, 5), (3, 1), (4, 5)):
        _run_case(emu, R.case("adh_wgrad_reduce", K, Nc, KH, reverse=True), nsplit, accumulate, seed=10 + KH)


@pytest.fixture(scope="module")
def small_emu(tmp_path_factory):
    d = tmp_path_factory.mktemp("wgrad_reduce_small_emu")
    exe = E.build(d, "conv_wgrad_reduce", "wgrad_reduce_small_main.cpp")
    return lambda: E.Script(exe, d)


def _small_call(s, slab, dst0, nslabs, L, accumulate, null_slab=False):
    dst = s.out(dst0.size, init=dst0)
    s.call(0, [nslabs, slab.shape[-2], slab.shape[-1], accumulate] + list(L), [None if null_slab else s.vec(slab), dst])
    return dst


@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("nslabs", [1, 63, 64, 65, 200])
def test_wave_reduce(small_emu, nslabs, accumulate):
    """adh_wgrad_reduce_small, one wave per element: fewer slabs than lanes, one short of a wave, exactly one, one more, three
    trips and a partial fourth.  3 x 3 taps with K = 3, Nc = 16 (432 elements: 108 workgroups of four waves, reversed taps) and
    7 x 7 taps with K = 3, Nc = 5 (735 elements: the last workgroup has one idle wave).  The bound is the tap-domain one of the
    sibling kernels, (nslabs + c) EPS of the sum of |terms|, with c = 6 for the six additions of the 64-lane tree.  The slabs
    are padded to KP = 4 rows and NcP = 20 / 8 columns (random in the padding too), not to the 32 x 32 of the other cases: 200
    of those would be 40 MB a case.  Each case runs twice and must give the same bits."""
    s = small_emu()
    todo = []
    for cs, seed, ncp in ((R.case("adh_wgrad_reduce_small", 3, 16, 3, reverse=True), 60 + nslabs, 20),
                          (R.case("adh_wgrad_reduce_small", 3, 5, 7), 61 + nslabs, 8)):
        slab, dst0 = R.rng_slab(seed, nslabs, 1, cs.M.shape[1], 4, ncp), R.rng_dst(seed, cs.ndst, accumulate)
        todo.append((cs, slab, dst0, [_small_call(s, slab, dst0, nslabs, cs.L, accumulate) for _ in range(2)]))
    rcs = s.run()
    assert rcs == [0] * 4, rcs
    for cs, slab, dst0, (d1, d2) in todo:
        assert (s.after[d1] == s.after[d2]).all(), "two identical calls differ"
        ref, bound, written = R.reference(slab, cs.M, cs.c + 6, cs.L, cs.taps, dst0, accumulate)
        R.check(s.get(d1).numpy(), dst0, ref, bound, written, f"small taps={cs.L.KHt} nslabs={nslabs} acc={accumulate}")


def test_wave_reduce_rejections_leave_dst_unwritten(small_emu):
    s = small_emu()
    cs = R.case("adh_wgrad_reduce_small", 3, 16, 3)
    slab, nan = cs.slab(50, 1), R.rng_dst(0, cs.ndst, 0)
    bad = [_small_call(s, slab, nan, 1, cs.L, 0, null_slab=True), _small_call(s, slab, nan, 0, cs.L, 0)]
    assert s.run() == [ADH_E_ARG] * 2
    for dst in bad:
        assert s.unchanged(dst)


@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("nsplit", [1, 5])
@pytest.mark.parametrize("entry", ["adh_wgrad_reduce_wino", "adh_wgrad_reduce_wino43"])
def test_winograd_reduce(emu, entry, nsplit, accumulate):
    for (K, Nc), reverse in zip(R.SIZES, (True, False)):
        _run_case(emu, R.case(entry, K, Nc, 3, reverse=reverse), nsplit, accumulate, seed=20 + nsplit)


@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("nsplit", [1, 5])
def test_wino32_class_forms(emu, nsplit, accumulate):
    """the four kernel-parity classes of Conv2d k4 s2 on a 4x4 layout; one transposed 2x2 class, taps walked backwards, on a
    layout whose tap strides are negative too"""
    _run_case(emu, R.case("adh_wgrad_reduce_wino32", 5, 7, 4, classes=R.CONV_K4S2_CLASSES), nsplit, accumulate, seed=31)
    _run_case(emu, R.case("adh_wgrad_reduce_wino32", 32, 32, 4, classes=R.CONV_K4S2_CLASSES), nsplit, accumulate, seed=32)
    _run_case(emu, R.case("adh_wgrad_reduce_wino32", 5, 7, 2, reverse=True, classes=R.CONVT_CLASS), nsplit, accumulate, seed=33)


@pytest.mark.parametrize("accumulate", [0, 1])
def test_packed_reduce(emu, accumulate):
    Cin, KH, KW, Cout = 3, 7, 7, 5
    for nsplit in (1, 2, 3, 5):
        slab = R.rng_slab(40 + nsplit, nsplit, KH * ((KW + 3) // 4), 32, R.NCP)
        dst0 = R.rng_dst(40, Cout * Cin * KH * KW, accumulate)
        rc, got = emu("adh_wgrad_reduce_packed", slab, dst0, nsplit, None, accumulate, packed=(Cin, KH, KW, Cout))
        assert rc == 0
        ref, bound = R.packed_reference(slab, Cin, KH, KW, Cout, dst0, accumulate)
        R.check(got, dst0, ref, bound, np.ones(dst0.shape, bool), f"packed nsplit={nsplit} acc={accumulate}")


def test_rejections_leave_dst_unwritten(emu):
    cs = R.case("adh_wgrad_reduce_wino", 5, 7, 3)
    two = R.case("adh_wgrad_reduce_wino", 5, 7, 2)
    slab = cs.slab(50, 1)
    nan = R.rng_dst(0, cs.ndst, 0)
    bad = []
    for entry in ("adh_wgrad_reduce", "adh_wgrad_reduce_wino", "adh_wgrad_reduce_wino43", "adh_wgrad_reduce_wino32"):
        cl = R.CONVT_CLASS if entry.endswith("32") else ()
        bad.append((entry, dict(nsplit=1, L=cs.L, null_slab=True, classes=cl)))
        bad.append((entry, dict(nsplit=0, L=cs.L, classes=cl)))
    for entry in ("adh_wgrad_reduce_wino", "adh_wgrad_reduce_wino43"):
        bad.append((entry, dict(nsplit=1, L=two.L)))                       # a 2x2 layout passed to a 3x3 reduce
        bad.append((entry, dict(nsplit=1, L=cs.L, ncp=30)))                # NcP % 4 != 0
    bad.append(("adh_wgrad_reduce_wino32", dict(nsplit=1, L=two.L, ncp=30, classes=R.CONVT_CLASS)))
    bad.append(("adh_wgrad_reduce_packed", dict(nsplit=1, packed=(9, 7, 7, 5))))   # Cin = 9
    bad.append(("adh_wgrad_reduce_packed", dict(nsplit=0, packed=(3, 7, 7, 5))))
    bad.append(("adh_wgrad_reduce_packed", dict(nsplit=1, packed=(3, 7, 7, 5), null_slab=True)))
    for entry, kw in bad:
        rc, got = emu(entry, slab, nan, **kw)
        assert rc == ADH_E_ARG, (entry, kw, rc)
        assert np.isnan(got).all(), (entry, kw)
