"""csrc/ema.hip without a GPU: the source file, compiled by the host C++ compiler against the stand-in header of tools/host_emu
(its ADH_HOST_EMU section) with AddressSanitizer and UndefinedBehaviorSanitizer, run as a stand-alone program on heap blocks of
exactly their sizes and held to the float64 reference and the bound of tests/_ema_ref64.py -- the ones tests/test_gpu_ema.py
holds the library to.  It runs the chunk, quad and tail index arithmetic, the alignment test and the control-block logic of the
very source the GPU runs under the sanitizers.  (The host compiler does not contract a * b + c, so the blend is three roundings
here: the bound's own count.)"""
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from tests import _ema_ref64 as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ADH_E_ARG = -1
POISON = 0x7FC0DEAD


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler found"
    d = tmp_path_factory.mktemp("ema_emu")
    shutil.copy(os.path.join(ROOT, "adam-dehaze_amd", "csrc", "ema.hip"), d / "ema.cpp")
    for fn in ("common.h", "ema_main.cpp"):                # the copy's #include "common.h" finds the stand-in next to it
        shutil.copy(os.path.join(ROOT, "tools", "host_emu", fn), d / fn)
    exe = d / "ema_emu"
    subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-DADH_HOST_EMU", "-I", os.path.join(ROOT, "include"),
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wno-unknown-pragmas", "-pthread",
                    str(d / "ema.cpp"), str(d / "ema_main.cpp"), "-o", str(exe)], check=True, cwd=d)

    def run(mode, data, decay=0.9, warmup=0, finite=1, updates0=0, steps=1, nrc=1):
        h = np.array([len(data), mode, finite, warmup, updates0, steps, 0, 0], np.int32)
        desc = np.array([(n, po, eo) for n, po, eo, _ in R.TENSORS[:len(data)]], np.int32)
        with open(d / "in.bin", "wb") as f:
            f.write(h.tobytes() + np.float64(decay).tobytes() + desc.tobytes())
            for p, e in data:
                f.write(p.numpy().tobytes() + e.numpy().tobytes())
        r = subprocess.run([str(exe), str(d / "in.bin"), str(d / "out.bin")], capture_output=True, text=True)
        assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
        out = np.fromfile(d / "out.bin", dtype=np.int32)
        rcs, ctrl, rest = out[:nrc], out[nrc:nrc + 4], out[nrc + 4:]
        got, at = [], 0
        for n, po, eo, _ in R.TENSORS[:len(data)]:
            blocks = []
            for off in (po, eo):
                blk = rest[at:at + off + n]
                assert (blk[:off].view(np.uint32) == POISON).all(), "the floats in front of an offset tensor were written"
                blocks.append(torch.from_numpy(blk[off:].view(np.float32).copy()))
                at += off + n
            got.append(tuple(blocks))
        assert at == rest.size
        return [int(x) for x in rcs], (int(ctrl[0]), int(ctrl[1]), ctrl[2:3].view(np.float32)[0]), got
    return run


def _bits(t):
    return t.view(torch.int32)


@pytest.mark.parametrize("warmup,decay,updates0,steps", [(0, 0.9, 0, 1), (1, 0.999, 0, 1), (1, 0.5, 20, 1), (0, 0.9, 3, 5)])
def test_update_vs_float64(emu, warmup, decay, updates0, steps):
    data = R.inputs(1)
    rcs, (updates, active, w), got = emu(0, data, decay=decay, warmup=warmup, updates0=updates0, steps=steps)
    assert rcs == [0]
    u = updates0
    trajs = [R.Trajectory(e) for _, e in data]
    for _ in range(steps):
        u, act, w_ref = R.begin(u, decay, bool(warmup))
        assert act == 1
        for t, (p, _) in zip(trajs, data):
            t.step(p, w_ref)
    assert (updates, active) == (u, 1)
    assert np.float32(w).view(np.uint32) == w_ref.view(np.uint32), (w, w_ref)
    for i, (t, (p, e), (gp, ge)) in enumerate(zip(trajs, data, got)):
        assert torch.equal(_bits(gp), _bits(p)), f"tensor {i}: p was written"
        err = (ge.double() - t.ema).abs()
        assert bool((err <= t.bound()).all()), (i, float((err / t.bound().clamp_min(1e-300)).max()))
        assert not torch.equal(ge, e), f"tensor {i}: the shadow did not move"


def test_skipped_update_touches_nothing(emu):
    data = R.inputs(2)
    rcs, (updates, active, w), got = emu(1, data, finite=0, updates0=7, warmup=1)
    assert rcs == [0] and (updates, active) == (7, 0) and R.begin(7, 0.9, True, guard_finite=0)[:2] == (7, 0)
    for (p, e), (gp, ge) in zip(data, got):
        assert torch.equal(_bits(gp), _bits(p)) and torch.equal(_bits(ge), _bits(e))
    # a guard block that says "finite" is the same as none
    _, c1, g1 = emu(1, data, finite=1, updates0=7, warmup=1)
    _, c0, g0 = emu(0, data, updates0=7, warmup=1)
    assert c1[:2] == c0[:2] == (8, 1) and np.float32(c1[2]).view(np.uint32) == np.float32(c0[2]).view(np.uint32)
    for (_, a), (_, b) in zip(g1, g0):
        assert torch.equal(_bits(a), _bits(b))


def test_swap_is_bit_exact(emu):
    data = R.inputs(3)
    data[3][0][5] = float("nan")                           # payloads travel too
    data[6][1][R.CHUNK + 3] = float("-inf")
    rcs, _, got = emu(2, data)
    assert rcs == [0]
    for (p, e), (gp, ge) in zip(data, got):
        assert torch.equal(_bits(gp), _bits(e)) and torch.equal(_bits(ge), _bits(p))


def test_argument_rejections(emu):
    data = R.inputs(4)[:2]
    rcs, ctrl, got = emu(3, data, nrc=17)
    assert rcs[-1] == -100 and rcs[:-1] == [ADH_E_ARG] * 16, rcs
    assert ctrl[:2] == (0, 0)
    for (p, e), (gp, ge) in zip(data, got):
        assert torch.equal(_bits(gp), _bits(p)) and torch.equal(_bits(ge), _bits(e))
