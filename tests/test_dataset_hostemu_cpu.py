"""csrc/dataset.hip without a GPU: the source file, compiled by the host C++ compiler against tools/host_emu with AddressSanitizer
and UndefinedBehaviorSanitizer, run as a stand-alone program (tools/host_emu/dataset_main.cpp) on heap blocks of exactly the
addressed bytes, and compared with the float64 references of tests/_dataset_ref64.py.  A read or write outside a block is the
sanitizer's to report; the pitch slack of a source holds a poison byte nothing may depend on, and every input is checked
unchanged after the run (tests/_hostemu.py)."""
import numpy as np
import pytest
import torch

from tests import _dataset_ref64 as R
from tests import _hostemu as E

RESIZE, NUM_BLOCKS, BATCH = 0, 1, 2
POISON = 0xA5


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    d = tmp_path_factory.mktemp("dataset_emu")
    exe = E.build(d, "dataset", "dataset_main.cpp", sanitize=E.FLOAT_CAST)
    return lambda: E.Script(exe, d)


def _source(s, u8, pitch_slack, off):
    """a block of exactly off + (h - 1) * row_pitch + w * C bytes: it ends with the last pixel of the last row"""
    h, w, C = u8.shape
    rp = w * C + pitch_slack
    blk = np.full(off + (h - 1) * rp + w * C, POISON, np.uint8)
    for y in range(h):
        blk[off + y * rp: off + y * rp + w * C] = u8[y].reshape(-1)
    k = s.raw(blk, off)
    s.ro.append(k)
    return k, rp


@pytest.mark.parametrize("C", [1, 3, 4])
def test_resize(emu, C):
    s, cases = emu(), []
    shapes = R.RESIZE_CASES + R.RESIZE_DYADIC[:1] + [((1, 9), (4, 7)), ((7, 5), (7, 5))]       # + a 1 x N image, same size
    for k, ((h, w), (OH, OW)) in enumerate(shapes):
        u8 = np.random.RandomState(100 * k + C).randint(0, 256, size=(h, w, C)).astype(np.uint8)
        src, rp = _source(s, u8, pitch_slack=(0, 5, 3)[k % 3], off=(1, 0, 3, 2)[k % 4])         # odd bases, W * C no multiple of 4
        dst = s.out(OH * OW * 3, np.uint8)
        s.call(RESIZE, (rp, h, w, C, OH, OW), (src, dst))
        cases.append((u8, OH, OW, dst, ((h, w), (OH, OW)) in R.RESIZE_DYADIC or (h, w) == (OH, OW)))
    assert s.run() == [0] * len(cases)
    for u8, OH, OW, dst, exact in cases:
        R.check_resize(s.get(dst, np.uint8).numpy(), u8, OH, OW, exact=exact, what=f"C={C}")


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


PARAMS = [[0, 0, 0, 1.0, 1.0], [1, 0, 1, 0.9, 1.1], [0, 1, 0, 1.1, 0.9], [1, 1, 1, 1.1, 1.1]]


@pytest.mark.parametrize("HW", [(1, 1), (1, 7), (3, 5), (5, 8), (9, 12), (65, 64)])
def test_batch(emu, HW):
    Hh, Ww = HW
    M, pitch = 3, Hh * Ww * 3 + (0 if Ww % 2 else 4)
    cache = R.all_values_cache(M, Hh, Ww, seed=Hh * 31 + Ww)
    for off in (0, 1):                                                # a 4-byte aligned cache and an odd base
        s = emu()
        blk = np.full(off + (M - 1) * pitch + Hh * Ww * 3, POISON, np.uint8)      # ends with the last image's last byte
        for m in range(M):
            blk[off + m * pitch: off + m * pitch + Hh * Ww * 3] = cache[m].reshape(-1)
        ck = s.raw(blk, off)
        s.ro.append(ck)
        nb = s.call(NUM_BLOCKS, (Hh * Ww,))
        index = [2, 0, 2, 1]
        ik = s.vec(torch.tensor(index, dtype=torch.int64), np.int64)
        pk = s.vec(torch.tensor(PARAMS, dtype=torch.float32))
        nblk = max(1, min(-(-Hh * Ww // 4096), 128))
        outs = []
        for params in (None, pk):
            out, partial = s.out(4 * 3 * Hh * Ww), s.out(4 * nblk, np.float64)
            s.call(BATCH, (pitch, M, Hh, Ww, 4, nblk), (ck, ik, params, None if params is None else partial, out))
            outs.append(out)
        one = s.out(3 * Hh * Ww)                                      # sample 1 of the batch, alone
        p1 = s.vec(torch.tensor(PARAMS[1:2], dtype=torch.float32))
        s.call(BATCH, (pitch, M, Hh, Ww, 1, nblk), (ck, s.vec(torch.tensor([0], dtype=torch.int64), np.int64), p1,
                                                    s.out(nblk, np.float64), one))
        rcs = s.run()
        assert rcs[nb] == nblk and [r for k, r in enumerate(rcs) if k != nb] == [0, 0, 0], rcs
        plain = s.get(outs[0]).numpy().reshape(4, 3, Hh, Ww)
        E.assert_written(s.get(outs[0]), "plain")
        assert np.array_equal(_bits(plain), _bits((cache[index].astype(np.float32) / np.float32(255)).transpose(0, 3, 1, 2)))
        aug = s.get(outs[1])
        E.assert_written(aug, "augmented")
        aug = aug.numpy().reshape(4, 3, Hh, Ww)
        assert np.array_equal(_bits(aug[0]), _bits(plain[0]))        # b = c = 1, no flip: the bytes' own values
        ref = R.batch_ref(cache, index, np.array(PARAMS, np.float32))
        assert np.abs(aug.astype(np.float64) - ref).max() <= R.BATCH_BOUND
        assert np.array_equal(_bits(s.get(one).numpy().reshape(3, Hh, Ww)), _bits(aug[1]))     # alone = in the batch


def test_refusals(emu):
    s = emu()
    Hh, Ww, M, N = 3, 5, 2, 2
    u8 = np.zeros((Hh, Ww, 4), np.uint8)
    src, dst = s.vec(torch.from_numpy(u8), np.uint8), s.out(4 * 4 * 3, np.uint8)
    cache = s.vec(torch.zeros(M * Hh * Ww * 3, dtype=torch.uint8), np.uint8)
    idx = s.vec(torch.tensor([0, 1], dtype=torch.int64), np.int64)
    par = s.vec(torch.tensor([[0, 0, 0, 1, 1]] * N, dtype=torch.float32))
    partial, out = s.out(N, np.float64), s.out(N * 3 * Hh * Ww)
    bad = []
    for ints in ((20, 0, Ww, 4, 4, 4), (20, Hh, 0, 4, 4, 4), (20, Hh, Ww, 4, 0, 4), (20, Hh, Ww, 4, 4, 0), (20, Hh, Ww, 4, -1, 4),
                 (20, Hh, Ww, 2, 4, 4), (20, Hh, Ww, 0, 4, 4), (20, Hh, Ww, 5, 4, 4), (19, Hh, Ww, 4, 4, 4), (14, Hh, Ww, 3, 4, 4)):
        bad.append(s.call(RESIZE, ints, (src, dst)))
    bad.append(s.call(RESIZE, (20, Hh, Ww, 4, 4, 4), (None, dst)))
    bad.append(s.call(RESIZE, (20, Hh, Ww, 4, 4, 4), (src, None)))
    ip = Hh * Ww * 3
    for ints in ((ip, M, Hh, Ww, 0, 1), (ip, M, Hh, Ww, 65536, 1), (ip, M, 0, Ww, N, 1), (ip, M, Hh, 0, N, 1), (ip, 0, Hh, Ww, N, 1),
                 (ip - 1, M, Hh, Ww, N, 1), (ip, M, Hh, Ww, N, 2), (ip, M, Hh, Ww, N, 0)):
        bad.append(s.call(BATCH, ints, (cache, idx, par, partial, out)))
    for bufs in ((None, idx, par, partial, out), (cache, None, par, partial, out), (cache, idx, par, None, out),
                 (cache, idx, par, partial, None)):
        bad.append(s.call(BATCH, (ip, M, Hh, Ww, N, 1), bufs))
    good = s.call(BATCH, (ip, M, Hh, Ww, N, 1), (cache, idx, None, None, out))       # params NULL needs no partial
    rcs = s.run()
    assert [rcs[k] for k in bad] == [E.ADH_E_ARG] * len(bad), rcs
    assert rcs[good] == 0
    assert s.unchanged(dst) and s.unchanged(partial)
    assert (s.get(out).numpy() == 0).all()
