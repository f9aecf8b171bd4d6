"""The emulator's own cross-lane shuffle (tools/host_emu/common.h, __shfl_xor) and csrc/wave.h on top of it, before any kernel
relies on them: tools/host_emu/shuffle_main.cpp runs 64-lane butterflies (wave_sum, wave_max, an XOR of bit patterns), an
8-lane butterfly and the fixed-partner exchange with mask 1 (int, and floats that carry NaN payloads and the sign of zero), and
the float64 butterflies of csrc/train_io.hip's sums (a double travels as two 32-bit exchanges: a sum of integers near 2^32 that
are exact in float64 only, an XOR of 64-bit patterns carried as doubles, one lane of each wave holding a signalling NaN with a
payload and one -0.0), interleaved, inside a loop whose trip count differs between the four waves of a workgroup, followed by 8-lane butterflies that
only some 8-lane groups make.  Every lane checks every result of every trip against a serial restatement and counts what
differs; the count must be 0 for every lane, and the last trip's results are checked again here.  The sums are of small
integers, exact in fp32 in any order.

What the two-slot mailbox this scheme replaced gave for the same program (its int shuffle carrying the floats by bit-cast; 8
CPUs, one OS thread per lane): it counted a lane's shuffles whoever the partner, so in a butterfly a lane could post shuffle
n + 2 into the slot its partner of step n had not read yet, and two lanes that had shuffled different numbers of times with
third lanes no longer met at all.
  * With NWG = 4 as here the program did not finish (stopped by the timeout): lanes t and t ^ 32 sit in 8-lane groups that
    make different numbers of closing butterflies, enter the second workgroup with different counts, and the one ahead waits
    for a count its partner never reaches.
  * With one workgroup a launch (NWG = 1, ITERS = 150, two launches, four runs): 1 058 371 of the 2 216 704 lane results were
    wrong, and all 2048 lanes had wrong results.
Here every one of them must be right.  (150 to 159 trips a wave in each of four workgroups, twice: a second or two on 8 CPUs.)"""
import numpy as np
import pytest
import torch

from tests import _hostemu as E

NWG, ITERS = 4, 150


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    d = tmp_path_factory.mktemp("shuffle_emu")
    exe = E.build(d, None, "shuffle_main.cpp")
    return lambda: E.Script(exe, d)


def _case(s, seed):
    x = torch.randint(-40, 41, (NWG * 256,), generator=torch.Generator().manual_seed(seed)).float()
    b = {"in": s.vec(x), "bad": s.out(NWG * 256, np.int32), "s64": s.out(NWG * 256), "s8": s.out(NWG * 256),
         "bits": s.out(NWG * 256, np.uint32), "sd": s.out(NWG * 256, np.float64), "bd": s.out(NWG * 256, np.uint64)}
    s.call(0, [NWG, ITERS], [b["in"], b["bad"], b["s64"], b["s8"], b["bits"], b["sd"], b["bd"]])
    return x, b


def _pattern(t, it):
    return (np.uint64(0x9E3779B9) * (t + 1) & 0xFFFFFFFF) ^ (np.uint64(0x85EBCA6B) * np.uint64(it + 1) & 0xFFFFFFFF)


def _dbl_bits(t, it):
    """shuffle_main.cpp's dbl_bits"""
    t, it = t.astype(np.uint64), it.astype(np.uint64)
    out = (_pattern(t, it) << np.uint64(32)) | _pattern(t + np.uint64(7), it + np.uint64(3))
    nan = np.uint64(0x7FF4DEAD00000001) | ((_pattern(t, it) << np.uint64(8)) & np.uint64(0x0000FFFFFFFFFF00))
    out = np.where(t % 64 == 5, nan, out)
    return np.where(t % 64 == 9, np.uint64(0x8000000000000000), out)


def test_every_lane_result_is_exact(emu):
    s = emu()
    cases = [_case(s, seed) for seed in (1, 2)]                       # two launches: the channels are cleared in between
    rcs = s.run()
    assert rcs == [0, 0]
    t = np.arange(NWG * 256)
    last = ITERS + 3 * ((t % 256) >> 6) - 1                           # the last trip of each lane's wave
    for x, b in cases:
        bad = s.get(b["bad"], np.int32).numpy()
        assert (bad == 0).all(), f"{(bad != 0).sum()} lanes saw {bad.sum()} wrong shuffle results"
        xn = x.numpy().astype(np.float64)
        want64 = np.repeat((xn + (last & 7)).reshape(-1, 64).sum(1), 64)
        want8 = np.repeat((xn + (last & 3)).reshape(-1, 8).sum(1), 8)
        assert np.array_equal(s.get(b["s64"]).numpy().astype(np.float64), want64), "wave_sum"
        assert np.array_equal(s.get(b["s8"]).numpy().astype(np.float64), want8), "8-lane butterfly"
        pat = _pattern((t % 256).astype(np.uint64), last.astype(np.uint64)).reshape(-1, 64)
        wantx = np.repeat(np.bitwise_xor.reduce(pat, axis=1), 64).astype(np.uint32)
        assert np.array_equal(s.after[b["bits"]].view(np.uint32), wantx), "XOR butterfly of bit patterns"
        term = np.where(t % 64 == 9, -0.0, xn * 4294967311.0 + (last & 7))            # exact: |x| <= 40, so below 2^38
        wantd = np.repeat(term.reshape(-1, 64).sum(1), 64)
        assert np.array_equal(s.after[b["sd"]].view(np.uint64), wantd.view(np.uint64)), "float64 butterfly: the exact sum, bit for bit"
        patd = _dbl_bits(t % 256, last).reshape(-1, 64)
        assert ((patd[:, 5] >> np.uint64(51)) == 0xFFE).all() and (patd[:, 9] == np.uint64(1 << 63)).all()      # sNaN, -0.0
        wantxd = np.repeat(np.bitwise_xor.reduce(patd, axis=1), 64)
        assert np.array_equal(s.after[b["bd"]].view(np.uint64), wantxd), "XOR butterfly of 64-bit patterns carried as doubles"
