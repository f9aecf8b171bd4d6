"""csrc/d4.hip without a GPU: the source file, compiled by the host C++ compiler against tools/host_emu with AddressSanitizer and
UndefinedBehaviorSanitizer, run as a stand-alone program (tools/host_emu/d4_main.cpp) on heap blocks of exactly the addressed
bytes and compared bit for bit (as int32) with the torch CPU reference of tests/_d4_cases.py.  A read or a write outside a
block, or outside the LDS tile, is the sanitizer's to report."""
import numpy as np
import pytest
import torch

from tests import _d4_cases as K
from tests import _hostemu as E

APPLY, APPLY_SHIFTED = 0, 1


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    d = tmp_path_factory.mktemp("d4_emu")
    exe = E.build(d, "d4", "d4_main.cpp")
    return lambda: E.Script(exe, d)


def _call(s, src, N, C, H, W, op, dst, flip_ops=None, accumulate=0, scale=1.0):
    return s.call(APPLY, (N, C, H, W, op[0], op[1], accumulate), (src, flip_ops, dst), (scale,))


@pytest.mark.parametrize("N,C", K.NC)
def test_bit_equality_sweep(emu, N, C):
    s, cases = emu(), []
    for H, W in K.HW:
        x = K.distinct(N, C, H, W)
        src = s.vec(x.reshape(-1))
        for op in K.OPS:
            dst = s.out(x.numel())
            _call(s, src, N, C, H, W, op, dst)
            cases.append(((H, W, op), dst, K.ref(x, *op)))
    assert s.run() == [0] * len(cases)
    for what, dst, want in cases:
        assert torch.equal(K.bits(s.get(dst)), K.bits(want.reshape(-1))), what


@pytest.mark.parametrize("H,W", [(5, 7), (8, 12), (33, 70)])
def test_per_image_flip_codes_are_masked(emu, H, W):
    N, C = 6, 2
    codes = torch.tensor([7, -1, 0, 2, 0x7FFFFFFD, -2147483648 + 2], dtype=torch.int64)     # & 3: 3 3 0 2 1 2
    assert [int(c) & 3 for c in codes] == [3, 3, 0, 2, 1, 2]
    x = K.distinct(N, C, H, W)
    s = emu()
    src, ops = s.vec(x.reshape(-1)), s.vec(codes, np.int32)
    a, b = s.out(x.numel()), s.out(x.numel())
    _call(s, src, N, C, H, W, (0, 1), a, flip_ops=ops)          # the `flips` argument is not looked at with flip_ops
    _call(s, src, N, C, H, W, (1, 0), b, flip_ops=ops)
    assert s.run() == [0, 0]
    assert torch.equal(K.bits(s.get(a)), K.bits(K.ref_per_image(x, 0, codes).reshape(-1)))
    assert torch.equal(K.bits(s.get(b)), K.bits(K.ref_per_image(x, 1, codes).reshape(-1)))


@pytest.mark.parametrize("scale", [0.125, 0.25, 1.0])
def test_accumulate_and_scale(emu, scale):
    s, cases = emu(), []
    for k, (H, W) in enumerate([(5, 7), (8, 12), (65, 66)]):
        x = K.random((2, 3, H, W), 10 + k)
        src = s.vec(x.reshape(-1))
        for op in K.OPS:
            old = K.random(K.out_shape(2, 3, H, W, op[0]), 20 + k)
            dst = s.out(x.numel(), init=old.reshape(-1))
            _call(s, src, 2, 3, H, W, op, dst, accumulate=1, scale=scale)
            cases.append(((H, W, op, "accumulate"), dst, (old + K.ref(x, *op)) * scale))
            if scale != 1.0:
                dst = s.out(x.numel())
                _call(s, src, 2, 3, H, W, op, dst, accumulate=0, scale=scale)
                cases.append(((H, W, op, "scale alone"), dst, K.ref(x, *op) * scale))
    assert s.run() == [0] * len(cases)
    for what, dst, want in cases:
        assert torch.equal(K.bits(s.get(dst)), K.bits(want.reshape(-1))), what


@pytest.mark.parametrize("src_off,dst_off", [(1, 0), (0, 1), (1, 1)])
def test_bases_off_by_one_float_take_the_single_float_path(emu, src_off, dst_off):
    """W % 4 == 0 and 16-byte blocks: only the offset base keeps the launch from the 16-byte accesses"""
    N, C, H, W = 2, 3, 6, 16
    x, old = K.random((N, C, H, W), 3), K.random((N, C, H, W), 4)
    s, cases = emu(), []
    for op in K.OPS:
        for acc in (0, 1):
            blk = np.full(x.numel() + src_off, E.RPOISON, np.uint32)
            blk[src_off:] = x.reshape(-1).numpy().view(np.uint32)
            src = s.raw(blk, 4 * src_off)
            s.ro.append(src)
            blk = np.full(x.numel() + dst_off, E.WPOISON, np.uint32)
            blk[dst_off:] = old.reshape(-1).numpy().view(np.uint32)
            dst = s.raw(blk, 4 * dst_off)
            s.checks.append((dst, np.arange(dst_off), E.WPOISON, "the float in front of an offset output"))
            _call(s, src, N, C, H, W, op, dst, accumulate=acc, scale=0.25 if acc else 1.0)
            o = old.reshape(K.out_shape(N, C, H, W, op[0]))
            cases.append(((op, acc), dst, (o + K.ref(x, *op)) * 0.25 if acc else K.ref(x, *op)))
    assert s.run() == [0] * len(cases)
    for what, dst, want in cases:
        assert torch.equal(K.bits(s.get(dst)[dst_off:]), K.bits(want.reshape(-1))), what


def test_copy_form_keeps_nan_payloads_and_negative_zero(emu):
    N, C, H, W = 1, 2, 8, 8
    # quiet and signalling NaNs of both signs with payloads, and -0; every element another payload but the zeros
    pattern = np.array([0x7FC0BEEF, 0x7F800001, 0x80000000, 0xFFC12345, 0xFF8ABCDE], np.uint32)
    w = np.tile(pattern, 26)[:N * C * H * W]
    w = np.where(w == 0x80000000, w, w + 16 * np.arange(w.size, dtype=np.uint32))
    words = torch.from_numpy(w.view(np.int32).copy())
    x = words.view(torch.float32)
    assert int(torch.isnan(x).sum()) == int((w != 0x80000000).sum()) > 100 and len(set(w.tolist())) == int((w != 0x80000000).sum()) + 1
    s, cases = emu(), []
    src = s.raw(words.numpy())
    s.ro.append(src)
    for op in K.OPS:
        dst = s.out(x.numel())
        _call(s, src, N, C, H, W, op, dst)
        cases.append((op, dst, K.ref(words.reshape(N, C, H, W), *op)))
    assert s.run() == [0] * len(cases)
    for what, dst, want in cases:
        assert torch.equal(s.get(dst, np.int32), want.reshape(-1)), what


def test_refusals_leave_the_output_alone(emu):
    N, C, H, W = 2, 3, 4, 8
    n = N * C * H * W
    x = K.random((N, C, H, W), 1)
    s = emu()
    src = s.vec(x.reshape(-1))
    dst = s.raw(np.full(n, 0x5A, np.uint8).repeat(4))
    both = s.raw(np.full(8 * n, 0x5A, np.uint8))                       # 2 n floats: src and dst ranges inside one block
    bad = [s.call(APPLY, (N, C, H, W, 0, 0, 0), (None, None, dst), (1.0,)),
           s.call(APPLY, (N, C, H, W, 0, 0, 0), (src, None, None), (1.0,))]
    for shape in ((0, C, H, W), (N, 0, H, W), (N, C, 0, W), (N, C, H, 0), (-1, C, H, W), (N, -1, H, W), (N, C, -4, W), (N, C, H, -8)):
        for t in (0, 1):
            bad.append(s.call(APPLY, (*shape, t, 0, 0), (src, None, dst), (1.0,)))
    for t in (-1, 2, 3):
        bad.append(s.call(APPLY, (N, C, H, W, t, 0, 0), (src, None, dst), (1.0,)))
    for f in (-1, 4, 7):
        for t in (0, 1):
            bad.append(s.call(APPLY, (N, C, H, W, t, f, 0), (src, None, dst), (1.0,)))
    for t in (0, 1):
        for acc in (0, 1):
            bad.append(s.call(APPLY, (N, C, H, W, t, 0, acc), (both, None, both), (1.0,)))       # in place
    rcs = s.run()
    assert [rcs[k] for k in bad] == [E.ADH_E_ARG] * len(bad), rcs
    assert s.unchanged(dst) and s.unchanged(both)
    assert (s.after[dst] == 0x5A).all()


@pytest.mark.parametrize("shift", [1, 5, 31, -1, -5, -31])
def test_partly_overlapping_ranges_are_refused(emu, shift):
    """src and dst ranges of 32 floats inside one block, dst `shift` floats behind src (in front of it where negative): they
    share at least one float"""
    N, C, H, W = 1, 1, 4, 8
    s = emu()
    blk = s.raw(np.full(4 * (N * C * H * W + abs(shift)), 0x5A, np.uint8))
    bad = [s.call(APPLY_SHIFTED, (N, C, H, W, t, 0, acc, shift), (blk,), (1.0,)) for t in (0, 1) for acc in (0, 1)]
    rcs = s.run()
    assert [rcs[k] for k in bad] == [E.ADH_E_ARG] * len(bad), rcs
    assert s.unchanged(blk)


def test_adjacent_ranges_are_taken(emu):
    """dst starts at the float behind src's last: no overlap"""
    N, C, H, W = 1, 2, 4, 8
    n = N * C * H * W
    x = K.distinct(N, C, H, W)
    for shift in (n, -n):
        s = emu()
        both = np.full(2 * n, E.WPOISON, np.uint32)
        both[(0 if shift > 0 else n):][:n] = x.reshape(-1).numpy().view(np.uint32)
        blk = s.raw(both)
        s.call(APPLY_SHIFTED, (N, C, H, W, 1, 3, 0, shift), (blk,), (1.0,))
        assert s.run() == [0]
        got = s.get(blk)
        src, dst = (got[:n], got[n:]) if shift > 0 else (got[n:], got[:n])
        assert torch.equal(K.bits(src), K.bits(x.reshape(-1))) and torch.equal(K.bits(dst), K.bits(K.ref(x, 1, 3).reshape(-1)))
