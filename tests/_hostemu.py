"""Shared by the tests/test_*_hostemu_cpu.py that run on tools/host_emu/stream_rt.cpp (bn_act, depthwise, densenet, image_io, d4,
ciede2000, cbam, lpips, detect, pointwise, train_io, and the shuffle's self-test): builds a copy of one csrc/*.hip file with the host C++
compiler against tools/host_emu (common.h's ADH_HOST_EMU_STREAM section, stream_rt.cpp, the file's driver) under
AddressSanitizer and UndefinedBehaviorSanitizer, and runs scripts (tools/host_emu/stream_rt.h) through the resulting stand-alone
program.  Nothing is loaded into Python.

A Script lays every tensor out as the drivers' buffer rules ask: a heap block of exactly the bytes the contract gives it.  A
channel slice (cs > C) starts `off` floats into its block behind poison floats, and the block ends at the last used channel of the
last pixel; the slack between the pixels is NaN for tensors the kernel reads and the bit pattern WPOISON for tensors it writes.
Script.run checks afterwards that every poison float is still there, bit for bit."""
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ADH_E_ARG = -1
EPS = 2.0 ** -24
RPOISON = 0x7FC0DEAD        # in front of a tensor that is read
WPOISON = 0x7FC0BEEF        # slack and unwritten elements of a tensor that is written (a NaN: it fails every bound)
TIMEOUT = 120


FLOAT_CAST = "address,undefined,float-cast-overflow"     # -fsanitize=undefined leaves a float -> int conversion out of range to g++


def build(tmp, hip, driver, defines=(), exe="emu", sanitize="address,undefined"):
    """compile csrc/<hip>.hip + tools/host_emu/<driver> + stream_rt.cpp in the directory `tmp`; returns the program's path.
    hip = None: the driver brings its own kernel (tools/host_emu/shuffle_main.cpp)."""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler found"
    srcs = [driver, "stream_rt.cpp"]
    if hip is not None:
        shutil.copy(os.path.join(ROOT, "adam-dehaze_amd", "csrc", hip + ".hip"), tmp / (hip + ".cpp"))
        srcs.insert(0, hip + ".cpp")
    for fn in ("bn_stream.h", "wave.h"):                                  # compiled as they ship
        shutil.copy(os.path.join(ROOT, "adam-dehaze_amd", "csrc", fn), tmp / fn)
    for fn in ("common.h", "stream_rt.h", "stream_rt.cpp", driver):      # the copy's #include "common.h" finds the stand-in
        shutil.copy(os.path.join(ROOT, "tools", "host_emu", fn), tmp / fn)
    out = tmp / exe
    subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-DADH_HOST_EMU", "-DADH_HOST_EMU_STREAM", *["-D" + d for d in defines],
                    "-I", os.path.join(ROOT, "include"), "-fsanitize=" + sanitize, "-fno-sanitize-recover=all",
                    "-Wno-unknown-pragmas", "-pthread", *[str(tmp / f) for f in srcs], "-o", str(out)], check=True, cwd=tmp)
    return out


def _f32(t):
    return np.ascontiguousarray(torch.as_tensor(t).detach().to(torch.float32).numpy())


class Script:
    def __init__(self, exe, workdir):
        self.exe, self.dir = exe, workdir
        self.bufs = []          # (uint8 block, off bytes)
        self.checks = []        # (buffer, uint32 index array, pattern, what)
        self.outs = {}          # channel-slice buffer -> the float index of every element of its [P, C] slice
        self.calls = []
        self.ro = []            # buffers the kernels only read: unchanged after the run

    # ------------------------------------------------------------------ buffers
    def raw(self, arr, off_bytes=0):
        a = np.ascontiguousarray(arr)
        self.bufs.append((a.view(np.uint8).reshape(-1).copy(), off_bytes))
        return len(self.bufs) - 1

    def vec(self, t, dtype=np.float32):
        """a dense tensor the kernel reads: exactly its bytes"""
        self.ro.append(self.raw(np.ascontiguousarray(torch.as_tensor(t).detach().numpy().astype(dtype))))
        return self.ro[-1]

    def _slice(self, P, C, cs, off, values, slack_bits, front_bits):
        n = off + P * cs - (cs - C)
        blk = np.full(n, slack_bits, np.uint32)
        blk[:off] = front_bits
        idx = off + (np.arange(P)[:, None] * cs + np.arange(C)[None, :]).reshape(-1)
        if values is not None:
            blk[idx] = _f32(values).reshape(-1).view(np.uint32)
        k = self.raw(blk, off * 4)
        mask = np.ones(n, bool)
        mask[idx] = False
        self.outs[k] = idx
        return k, np.nonzero(mask)[0]

    def sin(self, t, cs=None, off=0):
        """[P, C] read by the kernel at channel stride cs: NaN slack, RPOISON in front"""
        P, C = t.shape
        k, slack = self._slice(P, C, cs or C, off, t, 0x7FC00000, RPOISON)
        self.ro.append(k)
        return k

    def sout(self, P, C, cs=None, off=0, init=None):
        """[P, C] written by the kernel at channel stride cs: WPOISON everywhere (or `init` in the slice: accumulate forms);
        front and slack are checked after the run"""
        k, slack = self._slice(P, C, cs or C, off, init, WPOISON, WPOISON)
        self.checks.append((k, slack, WPOISON, "the slack around a written channel slice"))
        return k

    def out(self, n, dtype=np.float32, init=None):
        """a dense output of n elements, every element poison (every byte 0x5A for the integer types: 0x5A5A5A5A as int32)
        unless `init` is given"""
        if init is not None:
            return self.raw(np.ascontiguousarray(torch.as_tensor(init).detach().numpy().astype(dtype)))
        if dtype == np.float32:
            return self.raw(np.full(n, WPOISON, np.uint32))
        if dtype == np.float64:
            return self.raw(np.full(n, 0x7FF8DEADBEEF0000, np.uint64))
        return self.raw(np.full(n * np.dtype(dtype).itemsize, 0x5A, np.uint8).view(dtype))

    # ------------------------------------------------------------------ calls
    def call(self, fn, ints=(), bufs=(), doubles=()):
        self.calls.append((fn, [int(v) for v in ints], [float(v) for v in doubles], [-1 if b is None else int(b) for b in bufs]))
        return len(self.calls) - 1

    def run(self):
        """returns the return values; the blocks are read back with get / get_slice"""
        with open(self.dir / "in.bin", "wb") as f:
            f.write(np.int64(len(self.bufs)).tobytes())
            for blk, off in self.bufs:
                f.write(np.array([blk.size, off], np.int64).tobytes() + blk.tobytes())
            f.write(np.int64(len(self.calls)).tobytes())
            for fn, i, d, b in self.calls:
                f.write(np.array([fn, len(i)] + i + [len(d)], np.int64).tobytes() + np.array(d, np.float64).tobytes()
                        + np.array([len(b)] + b, np.int64).tobytes())
        try:
            r = subprocess.run([str(self.exe), str(self.dir / "in.bin"), str(self.dir / "out.bin")], capture_output=True,
                               text=True, timeout=TIMEOUT)
        except subprocess.TimeoutExpired as e:
            pytest.fail(f"the emulated program did not finish in {TIMEOUT} s: most likely a lane waits in __shfl_xor for a "
                        f"partner that has left the kernel.  stderr: {(e.stderr or b'')[-4000:]!r}")
        assert r.returncode == 0, f"exit {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-6000:]}"
        raw = np.fromfile(self.dir / "out.bin", dtype=np.uint8)
        n = 8 * len(self.calls)
        rcs = [int(v) for v in raw[:n].view(np.int64)]
        self.after, at = [], n
        for blk, _ in self.bufs:
            self.after.append(raw[at:at + blk.size].copy())
            at += blk.size
        assert at == raw.size
        for k, idx, pattern, what in self.checks:
            assert (self.after[k].view(np.uint32)[idx] == pattern).all(), f"buffer {k}: {what} was written"
        for k in self.ro:
            assert self.unchanged(k), f"buffer {k}: an input was written"
        return rcs

    def get(self, k, dtype=np.float32):
        return torch.from_numpy(self.after[k].view(dtype).copy())

    def get_slice(self, k, P, C, written=True):
        """the [P, C] slice of an sout buffer; `written`: no element may still hold its poison"""
        bits = self.after[k].view(np.uint32)[self.outs[k]]
        if written:
            assert not (bits == WPOISON).any(), f"buffer {k}: {(bits == WPOISON).sum()} output elements still hold their poison"
        return torch.from_numpy(bits.view(np.float32).reshape(P, C).copy())

    def unchanged(self, k):
        return bool((self.after[k] == self.bufs[k][0]).all())


def assert_written(t, what):
    """a dense float32 output read back with Script.get: no element still holds its poison"""
    assert not (t.view(torch.int32) == WPOISON).any(), f"{what}: output elements still hold their poison"


def assert_bound(got, ref64, bound, what):
    """|got - ref64| <= bound element-wise; NaN (an unwritten element) fails"""
    assert not torch.isnan(got).any(), f"{what}: NaN (an element was not written)"
    ref64 = torch.as_tensor(ref64, dtype=torch.float64)
    bound = torch.as_tensor(bound, dtype=torch.float64)
    err = (got.double() - ref64).abs()
    d = err - bound
    worst = float((err / bound.clamp_min(1e-300)).max()) if err.numel() else 0.0
    assert float(d.max()) <= 0, f"{what}: exceeds its bound by {float(d.max()):.3e} (|err| / bound = {worst:.3f})"
