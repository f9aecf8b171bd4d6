"""adh_d4_apply (csrc/d4.hip) on the MI355X: the bit-equality sweep of tests/test_d4_hostemu_cpu.py through the C ABI, the grid
loops, a full-size batch, and d4.self_ensemble against the same composition written in torch ops.  Everything is compared as
int32 with the torch CPU reference of tests/_d4_cases.py: the kernel moves values, or adds and scales them with one rounding each."""
import pytest
import torch

from adam_dehaze_amd import _hip as H
from adam_dehaze_amd import d4 as D
from tests import _d4_cases as K

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _raw(src, N, C, h, w, op, dst, flip_ops=None, accumulate=0, scale=1.0):
    return H.load().adh_d4_apply(H.stream_ptr(), src.data_ptr(), N, C, h, w, op[0], op[1], H.ptr(flip_ops), dst.data_ptr(),
                                 accumulate, scale)


def _filled(shape):
    return torch.full(shape, K.FILL, dtype=torch.int32, device=DEV).view(torch.float32)


@pytest.mark.parametrize("N,C", K.NC)
def test_bit_equality_sweep(N, C):
    for h, w in K.HW:
        x = K.distinct(N, C, h, w)
        xd = x.to(DEV)
        for op in K.OPS:
            dst = _filled(K.out_shape(N, C, h, w, op[0]))
            assert _raw(xd, N, C, h, w, op, dst) == 0
            assert torch.equal(K.bits(dst.cpu()), K.bits(K.ref(x, *op))), (h, w, op)


def test_accumulate_scale_per_image_codes_and_offset_bases():
    N, C = 3, 2
    codes = torch.tensor([7, -1, 2], dtype=torch.int32)
    for k, (h, w) in enumerate([(5, 7), (8, 12), (65, 66), (6, 16)]):
        x = K.random((N, C, h, w), 30 + k)
        n = x.numel()
        for off in (0, 1):                               # a base one float off its 16-byte alignment: single floats
            xd = torch.empty(n + off, device=DEV)[off:].view(N, C, h, w).copy_(x)
            for op in K.OPS:
                old = K.random(K.out_shape(N, C, h, w, op[0]), 40 + k)
                for scale in (0.125, 0.25):
                    dst = torch.empty(n + off, device=DEV)[off:].view(old.shape).copy_(old)
                    assert _raw(xd, N, C, h, w, op, dst, accumulate=1, scale=scale) == 0
                    assert torch.equal(K.bits(dst.cpu()), K.bits((old + K.ref(x, *op)) * scale)), (h, w, op, scale, off)
                dst = _filled(old.shape)
                assert _raw(xd, N, C, h, w, (op[0], 0), dst, flip_ops=codes.to(DEV)) == 0
                assert torch.equal(K.bits(dst.cpu()), K.bits(K.ref_per_image(x, op[0], codes))), (h, w, op, off)


def test_nan_payloads_and_negative_zero_survive_the_copy():
    words = torch.tensor([0x7FC0BEEF, 0x7F800001, -0x80000000, -0x3EDCBB, -0x754322], dtype=torch.int32).repeat(16)[:64]
    x = words.view(torch.float32).reshape(1, 1, 8, 8)
    for op in K.OPS:
        dst = _filled((1, 1, 8, 8))
        assert _raw(x.to(DEV), 1, 1, 8, 8, op, dst) == 0
        assert torch.equal(K.bits(dst.cpu()), K.ref(words.reshape(1, 1, 8, 8), *op)), op


def test_refusals():
    x, dst = torch.rand(2, 3, 4, 8, device=DEV), _filled((2, 3, 4, 8))
    before = dst.clone()
    lib, s = H.load(), H.stream_ptr()
    bad = [lib.adh_d4_apply(s, None, 2, 3, 4, 8, 0, 0, None, dst.data_ptr(), 0, 1.0),
           lib.adh_d4_apply(s, x.data_ptr(), 2, 3, 4, 8, 0, 0, None, None, 0, 1.0)]
    for shape in ((0, 3, 4, 8), (2, 0, 4, 8), (2, 3, 0, 8), (2, 3, 4, 0), (-2, 3, 4, 8)):
        bad.append(lib.adh_d4_apply(s, x.data_ptr(), *shape, 1, 0, None, dst.data_ptr(), 0, 1.0))
    bad += [_raw(x, 2, 3, 4, 8, (t, 0), dst) for t in (-1, 2)] + [_raw(x, 2, 3, 4, 8, (0, f), dst) for f in (-1, 4)]
    bad += [_raw(x, 2, 3, 4, 8, (t, 0), x) for t in (0, 1)]                              # in place
    both = torch.rand(2 * x.numel() - 1, device=DEV)
    bad.append(_raw(both[:x.numel()], 2, 3, 4, 8, (1, 0), both[x.numel() - 1:]))         # one float shared
    assert bad == [-1] * len(bad)
    torch.cuda.synchronize()
    assert torch.equal(K.bits(dst), K.bits(before))
    with pytest.raises(RuntimeError, match="ADH_E_ARG"):
        D.d4_apply(x, (0, 1), out=x)


@pytest.mark.parametrize("op", [(0, 3), (1, 1)])
def test_more_planes_than_a_grid_dimension_holds(op):
    N, C, h, w = 35000, 2, 2, 3                          # 70,000 planes: grid z is 65,535 and loops
    x = K.distinct(N, C, h, w)
    codes = (torch.arange(N, dtype=torch.int32) * 7 + 1)
    dst = _filled(K.out_shape(N, C, h, w, op[0]))
    assert _raw(x.to(DEV), N, C, h, w, op, dst) == 0
    assert torch.equal(K.bits(dst.cpu()), K.bits(K.ref(x, *op)))
    dst = _filled(K.out_shape(N, C, h, w, op[0]))
    assert _raw(x.to(DEV), N, C, h, w, op, dst, flip_ops=codes.to(DEV)) == 0
    want = torch.empty(K.out_shape(N, C, h, w, op[0]))
    for f in range(4):
        sel = (codes & 3) == f
        want[sel] = K.ref(x[sel], op[0], f)
    assert torch.equal(K.bits(dst.cpu()), K.bits(want))


@pytest.mark.parametrize("h,w,op", [(4 * 65535 + 5, 3, (0, 2)),          # the streaming kernel walks 4 rows per workgroup
                                    (2, 64 * 65535 + 70, (1, 2)),        # the transposing kernel one 64-row tile of dst
                                    (2, 64 * 65535 + 70, (1, 1))])
def test_more_rows_than_grid_y_holds(h, w, op):
    x = K.distinct(1, 1, h, w)                           # under 2^24 elements: every value exact
    dst = _filled(K.out_shape(1, 1, h, w, op[0]))
    assert _raw(x.to(DEV), 1, 1, h, w, op, dst) == 0
    assert torch.equal(K.bits(dst.cpu()), K.bits(K.ref(x, *op))), op


def test_full_size_batch_all_ops():
    N, C, h, w = 2, 3, 512, 1024
    x = K.random((N, C, h, w), 7)
    xd = x.to(DEV)
    for op in K.OPS:
        got = D.d4_apply(xd, op)
        assert tuple(got.shape) == K.out_shape(N, C, h, w, op[0])
        assert torch.equal(K.bits(got.cpu()), K.bits(K.ref(x, *op))), op
        back = D.d4_apply(got, D.d4_inverse(op))
        assert torch.equal(K.bits(back.cpu()), K.bits(x)), op


@pytest.mark.parametrize("mode", ["flip", "d8"])
@pytest.mark.parametrize("h,w", [(31, 45), (32, 48)])
def test_self_ensemble_is_the_torch_composition(mode, h, w):
    """a cheap `fn` that no symmetry commutes with: a product with a fixed random plane of the variant's own shape"""
    x = K.random((2, 3, h, w), 5)
    planes = {(h, w): K.random((1, 1, h, w), 8), (w, h): K.random((1, 1, w, h), 9)}
    calls = []

    def fn(b):
        calls.append(tuple(b.shape))
        return b * planes[tuple(b.shape[2:])].to(b.device), {"call": len(calls)}

    got, aux = D.self_ensemble(fn, x.to(DEV), mode)
    ops = K.OPS[:4] if mode == "flip" else K.OPS
    assert aux == {"call": 1} and len(calls) == len(ops)
    acc = None
    for op in ops:
        v = K.ref(x, *op)
        y = K.ref(v * planes[tuple(v.shape[2:])], *D.d4_inverse(op))
        acc = y if acc is None else acc + y
    want = acc * (1.0 / len(ops))
    assert torch.equal(K.bits(got.cpu()), K.bits(want))
    plain = x * planes[(h, w)]
    assert not torch.equal(want, plain), "the ensemble of this fn must differ from its single pass"
