"""csrc/fft_loss.hip without a GPU: the kernels' source file, compiled by the host C++ compiler against the stand-in header of
tools/host_emu (its ADH_HOST_EMU and ADH_HOST_EMU_DYN_LDS sections: one OS thread per GPU thread, a barrier for
__syncthreads, every launch's dynamic LDS a heap block of exactly its size) with AddressSanitizer and
UndefinedBehaviorSanitizer, run as a stand-alone program on heap buffers of exactly their sizes, and held to the float64
reference with the bounds of tests/test_gpu_fft_loss.py.  It checks the butterfly, bit-reversal, slot-packing, swizzle and tile
index arithmetic of the very source the GPU runs, LDS indices included; the GPU tests check the rest.  (sincospif is the
float64 functions rounded once here, the device's own there.)"""
import math
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from tests import _fft_ref64 as F64
from tests.test_gpu_fft_loss import FFT_GRAD_TOL, FFT_LOSS_RTOL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler found"
    d = tmp_path_factory.mktemp("fft_emu")
    shutil.copy(os.path.join(ROOT, "adam-dehaze_amd", "csrc", "fft_loss.hip"), d / "fft_loss.cpp")
    for fn in ("common.h", "fft_loss_main.cpp"):          # the copy's #include "common.h" finds the stand-in next to it
        shutil.copy(os.path.join(ROOT, "tools", "host_emu", fn), d / fn)
    exe = d / "fft_loss_emu"
    subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-DADH_HOST_EMU", "-DADH_HOST_EMU_DYN_LDS", "-I", os.path.join(ROOT, "include"),
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wno-unknown-pragmas", "-pthread",
                    str(d / "fft_loss.cpp"), str(d / "fft_loss_main.cpp"), "-o", str(exe)], check=True, cwd=d)

    def run(p, t, norm, want_grad=True):
        N, _, Hh, Ww = p.shape
        with open(d / "in.bin", "wb") as f:
            for x in (p, t):
                f.write(x.contiguous().numpy().tobytes())
        r = subprocess.run([str(exe), str(N), str(Hh), str(Ww), str(int(norm == "ortho")), str(int(want_grad)), str(d / "in.bin"),
                            str(d / "out.bin")], capture_output=True, text=True)
        assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
        out = np.fromfile(d / "out.bin", dtype=np.float32)
        assert out.size == 1 + (p.numel() if want_grad else 0)
        return float(out[0]), (torch.from_numpy(out[1:].copy()).view(N, 3, Hh, Ww) if want_grad else None)
    return run


def _check(emu, shape, norm):
    p, t = F64.inputs(*shape)
    assert F64.min_kink_distance(p, t) >= F64.KINK_MIN
    val, ref = F64.loss_and_grad(p, t, norm)
    got_val, got = emu(p, t, norm)
    assert not torch.isnan(got).any(), "an element was not written"
    rel = abs(got_val - float(val)) / float(val)
    err = float((got.double() - ref).abs().max()) / math.sqrt(float((ref * ref).mean()))
    print(f"[fft emu] {shape} {norm}: loss rel {rel:.2e} (gate {FFT_LOSS_RTOL:.2e}), grad {err:.2e} (gate {FFT_GRAD_TOL:.2e})")
    assert rel <= FFT_LOSS_RTOL and err <= FFT_GRAD_TOL
    return got_val


# 8 x 8: one column tile of the 4 slots there are, three stages each way (a radix-4 unit and the left-over radix-2 stage);
# 8 x 32: five stages across, and 16 slots = two column tiles of 8, the smallest image with more than one; 64 x 16: six stages
# down (three radix-4 units), one tile of 8; 16 x 16 with N = 5: 15 image-channels, four stages both ways
@pytest.mark.parametrize("shape", [(1, 8, 8), (2, 8, 32), (3, 64, 16), (5, 16, 16)])
def test_kernel_source_on_host_threads_vs_float64(emu, shape):
    _check(emu, shape, "backward")


def test_ortho_and_value_only_on_host_threads(emu):
    shape = (2, 8, 32)
    p, t = F64.inputs(*shape)
    v_b = _check(emu, shape, "backward")
    v_o = _check(emu, shape, "ortho")
    assert abs(v_o * math.sqrt(8 * 32) - v_b) <= 2.0 ** -22 * v_b       # one scale apart: two fp32 roundings
    v_only, none = emu(p, t, "backward", want_grad=False)               # no gradient buffer exists: a store would be a fault
    assert none is None and v_only == v_b
    same, g = emu(p, p, "backward")
    assert same == 0.0 and bool((g == 0).all())
