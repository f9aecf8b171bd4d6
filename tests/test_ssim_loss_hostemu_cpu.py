"""csrc/ssim_loss.hip without a GPU: the kernel's source file, compiled by the host C++ compiler against the stand-in
header of tools/host_emu (one OS thread per GPU thread, a barrier for __syncthreads) with AddressSanitizer and
UndefinedBehaviorSanitizer, run as a stand-alone program on heap buffers of exactly their sizes, and held to the float64
reference with the bound of tests/test_gpu_ssim_loss.py.  It checks the tile / halo / window index arithmetic and the
float64 arithmetic of the very source the GPU runs; the GPU tests check the rest."""
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from tests import _ssim_ref64 as S64
from tests.test_gpu_ssim_loss import SSIM_BWD_F64_UNITS, SSIML_T, U53, _inputs, _upstream
from tests._util import EPS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler found"
    d = tmp_path_factory.mktemp("ssim_emu")
    shutil.copy(os.path.join(ROOT, "adam-dehaze_amd", "csrc", "ssim_loss.hip"), d / "ssim_loss.cpp")
    for fn in ("common.h", "ssim_bwd_main.cpp"):          # the copy's #include "common.h" finds the stand-in next to it
        shutil.copy(os.path.join(ROOT, "tools", "host_emu", fn), d / fn)
    exe = d / "ssim_bwd_emu"
    subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-Wno-unknown-pragmas", "-pthread", str(d / "ssim_loss.cpp"), str(d / "ssim_bwd_main.cpp"), "-o", str(exe)],
                   check=True, cwd=d)

    def run(p, t, g):
        N, _, Hh, Ww = p.shape
        with open(d / "in.bin", "wb") as f:
            for x in (p, t, g):
                f.write(x.contiguous().numpy().tobytes())
        r = subprocess.run([str(exe), str(N), str(Hh), str(Ww), str(d / "in.bin"), str(d / "out.bin")], capture_output=True,
                           text=True)
        assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
        return torch.from_numpy(np.fromfile(d / "out.bin", dtype=np.float32).copy()).view(N, 3, Hh, Ww)
    return run


# one window; a partial tile; exactly one tile and one pixel more, each way; a 2 x 5 grid of tiles with ragged edges
@pytest.mark.parametrize("Hh,Ww", [(7, 7), (13, 14), (SSIML_T, SSIML_T + 1), (SSIML_T + 1, SSIML_T), (45, 131)])
@pytest.mark.parametrize("kind", ["noise", "wide_range", "two_constants"])
def test_kernel_source_on_host_threads_vs_float64(emu, Hh, Ww, kind):
    N = 3
    p, t = _inputs(kind, N, Hh, Ww)
    g = _upstream(N)
    (val, ref), terms = S64.ssim_and_grad(p, t, g.double())
    got = emu(p, t, g)
    assert not torch.isnan(got).any(), "an element was not written"
    assert torch.equal(got[:, 0], got[:, 1]) and torch.equal(got[:, 0], got[:, 2])
    assert bool((got[1] == 0).all())                       # g_ssim[1] = 0
    bound = EPS * ref.abs() + SSIM_BWD_F64_UNITS * U53 * terms.expand_as(ref)
    err = (got.double() - ref).abs()
    assert bool((err <= bound).all()), float((err / bound).max())
    if kind != "two_constants":
        assert float(got.abs().max()) > 0
