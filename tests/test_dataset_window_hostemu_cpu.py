"""adh_batch_window_from_u8 (csrc/dataset.hip) without a GPU: the source file compiled by the host C++ compiler against
tools/host_emu with AddressSanitizer and UndefinedBehaviorSanitizer and run as a stand-alone program (tools/host_emu/dataset_main.cpp,
call 3) over the table of tests/_dataset_window_cases.py.  The cache is a heap block of exactly base + cache_bytes bytes, so a
read in front of it or behind it -- the aligned dwords around a quad that starts off phase are the ones to watch -- is the
sanitizer's to report.  Checked: the inputs unchanged, the outputs fully written, the bit contract against adh_batch_from_u8
(call 2) on a dense copy of each window, sample n alone and a second call, the float64 bound of tests/_dataset_ref64.py, and every
refusal."""
import numpy as np
import pytest
import torch

from tests import _dataset_ref64 as R
from tests import _dataset_window_cases as K
from tests import _hostemu as E

NUM_BLOCKS, BATCH, WINDOW = 1, 2, 3
CPU_CASES = [(no, c) for no, c in enumerate(K.CASES) if not c["gpu_only"]]


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    d = tmp_path_factory.mktemp("dataset_window_emu")
    exe = E.build(d, "dataset", "dataset_main.cpp", sanitize=E.FLOAT_CAST)
    return lambda: E.Script(exe, d)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _i64(s, a):
    return s.vec(torch.from_numpy(np.ascontiguousarray(a, dtype=np.int64)), np.int64)


@pytest.mark.parametrize("no,case", CPU_CASES, ids=[c["name"] for _, c in CPU_CASES])
def test_windows(emu, no, case):
    flat, windows, dense = K.build(case)
    (CH, CW), base, out_off = case["crop"], case["base"], case["out_off"]
    N, px = len(windows), CH * CW
    nblk = max(1, min(-(-px // 4096), 128))       # 40 x 130: two blocks, whose lanes stride up to three times
    s = emu()
    ck = s.raw(np.concatenate([np.full(base, 0x5C, np.uint8), flat]), base)      # ends with the cache's last byte
    s.ro.append(ck)
    dk = s.vec(torch.from_numpy(dense), np.uint8)
    wk, ik = _i64(s, windows), _i64(s, np.arange(N))
    nb = s.call(NUM_BLOCKS, (px,))

    def out():                                                        # `out_off` poison floats in front, checked after the run
        k = s.raw(np.full(out_off + N * 3 * px, E.WPOISON, np.uint32), out_off * 4)
        s.checks.append((k, np.arange(out_off), E.WPOISON, "the floats in front of the output"))
        return k
    runs = []
    for params in [None] + K.param_sets(no, N, 2):
        pk = None if params is None else s.vec(torch.from_numpy(params))
        got, want, again = out(), s.out(N * 3 * px), out()
        part = [None if params is None else s.out(N * nblk, np.float64) for _ in range(3)]
        s.call(WINDOW, (flat.size, N, CH, CW, nblk), (ck, wk, pk, part[0], got))
        s.call(BATCH, (px * 3, N, CH, CW, N, nblk), (dk, ik, pk, part[1], want))
        s.call(WINDOW, (flat.size, N, CH, CW, nblk), (ck, wk, pk, part[2], again))
        alone = []
        for n in range(N if N > 1 else 0):                            # each sample alone
            p1 = None if params is None else s.vec(torch.from_numpy(params[n:n + 1]))
            o1 = s.out(3 * px)
            s.call(WINDOW, (flat.size, 1, CH, CW, nblk), (ck, _i64(s, windows[n:n + 1]), p1,
                                                          None if params is None else s.out(nblk, np.float64), o1))
            alone.append(o1)
        runs.append((params, got, want, again, alone, part))
    rcs = s.run()                                                     # also: every input unchanged, the front poison intact
    assert rcs[nb] == nblk and all(r == 0 for k, r in enumerate(rcs) if k != nb), rcs
    for params, got, want, again, alone, part in runs:
        g = s.get(got)[out_off:]
        E.assert_written(g, case["name"])
        g = g.numpy().reshape(N, 3, CH, CW)
        assert np.array_equal(_bits(g), _bits(s.get(want).numpy().reshape(N, 3, CH, CW))), "differs from the dense copy"
        assert np.array_equal(_bits(g), _bits(s.get(again)[out_off:].numpy().reshape(N, 3, CH, CW))), "a second call differs"
        for n, o1 in enumerate(alone):
            assert np.array_equal(_bits(g[n]), _bits(s.get(o1).numpy().reshape(3, CH, CW))), f"sample {n} alone differs"
        if params is None:
            assert np.array_equal(_bits(g), _bits((dense.astype(np.float32) / np.float32(255)).transpose(0, 3, 1, 2)))
        else:
            assert np.array_equal(s.get(part[0], np.float64).numpy().view(np.uint64),
                                  s.get(part[1], np.float64).numpy().view(np.uint64)), "the partial sums differ"
            ref = R.batch_ref(dense, np.arange(N), params)
            assert np.abs(g.astype(np.float64) - ref).max() <= R.BATCH_BOUND


def test_refusals(emu):
    s = emu()
    CH, CW, N = 3, 5, 2
    cache = s.vec(torch.zeros(64, dtype=torch.uint8), np.uint8)
    win = _i64(s, [[0, 15], [4, 15]])
    par = s.vec(torch.tensor([[0, 0, 0, 1, 1]] * N, dtype=torch.float32))
    partial, out = s.out(N, np.float64), s.out(N * 3 * CH * CW)
    bad = []
    for ints in ((64, 0, CH, CW, 1), (64, 65536, CH, CW, 1), (64, -1, CH, CW, 1), (64, N, 0, CW, 1), (64, N, CH, 0, 1),
                 (64, N, -1, CW, 1), (44, N, CH, CW, 1), (-4, N, CH, CW, 1), (64, N, CH, CW, 2), (64, N, CH, CW, 0),
                 (2 ** 62, N, 2 ** 31 - 1, 2 ** 31 - 1, 128)):         # CH * CW * 3 overflows
        bad.append(s.call(WINDOW, ints, (cache, win, par, partial, out)))
    for bufs in ((None, win, par, partial, out), (cache, None, par, partial, out), (cache, win, par, None, out),
                 (cache, win, par, partial, None)):
        bad.append(s.call(WINDOW, (64, N, CH, CW, 1), bufs))
    rcs = s.run()
    assert [rcs[k] for k in bad] == [E.ADH_E_ARG] * len(bad), rcs
    assert s.unchanged(out) and s.unchanged(partial)
    s = emu()                                                         # params NULL needs no partial; 45 bytes hold one 3 x 5 window
    cache = s.vec(torch.zeros(45, dtype=torch.uint8), np.uint8)
    out = s.out(3 * CH * CW)
    good = s.call(WINDOW, (45, 1, CH, CW, 1), (cache, _i64(s, [[0, 15]]), None, None, out))
    assert s.run()[good] == 0 and (s.get(out).numpy() == 0).all()
