"""csrc/image_io.hip without a GPU: the source file, compiled by the host C++ compiler against tools/host_emu with
AddressSanitizer and UndefinedBehaviorSanitizer, run as a stand-alone program (tools/host_emu/image_io_main.cpp) on heap blocks of
exactly the addressed bytes and compared bit for bit with the torch CPU expressions of tests/_image_io_cases.py.  A read or a
write outside the addressed rectangle's block is the sanitizer's to report; a write inside the block but outside a row's W * C
run shows as a byte that no longer holds its fill."""
import numpy as np
import pytest
import torch

from tests import _hostemu as E
from tests import _image_io_cases as K

TO_IMAGE, TO_U8 = 0, 1


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    d = tmp_path_factory.mktemp("image_io_emu")
    exe = E.build(d, "image_io", "image_io_main.cpp")
    return lambda: E.Script(exe, d)


def _bits(t):
    return t.contiguous().view(torch.int32)


def test_all_256_values_and_back(emu):
    s = emu()
    u8 = torch.arange(256, dtype=torch.uint8).view(1, 16, 16, 1)
    src, img, back = s.vec(u8, np.uint8), s.out(3 * 256), s.out(3 * 256, np.uint8)
    s.call(TO_IMAGE, (16, 256, 1, 16, 16, 1), (src, img))
    s.call(TO_U8, (1, 16, 16, 48, 768, 3), (img, back))
    assert s.run() == [0, 0]
    got = s.get(img).view(1, 3, 16, 16)
    want = torch.arange(256).float() / 255
    for c in range(3):
        assert torch.equal(_bits(got[0, c].reshape(-1)), _bits(want)), f"plane {c}"
    assert torch.equal(s.get(back, np.uint8).view(256, 3), torch.arange(256, dtype=torch.uint8)[:, None].expand(256, 3))


@pytest.mark.parametrize("W", [130, 132])
@pytest.mark.parametrize("C", [3, 4])
def test_quantiser_edges(emu, W, C):
    x = K.edge_image(W)
    H = x.shape[2]
    s = emu()
    src, dst = s.vec(x.reshape(-1)), s.out(H * W * C, np.uint8)
    s.call(TO_U8, (1, H, W, W * C, H * W * C, C), (src, dst))
    assert s.run() == [0]
    got, want = s.get(dst, np.uint8).view(1, H, W, C), K.ref_to_u8(x, C)
    bad = (got != want).nonzero()
    assert bad.numel() == 0, (bad[:5].tolist(), [float(x[0, c, y, xx]) for _, y, xx, c in bad[:5].tolist() if c < 3])
    n = K.edge_values().numel()
    flat = got[..., :3].permute(0, 3, 1, 2).reshape(-1)[:n]
    assert flat[-8:].tolist() == [0, 0, 255, 255, 0, 255, 0, 255]      # 0, -0.0, 1, nextafter(1, 2), -1e-7, inf, -inf, 1e30


@pytest.mark.parametrize("W", [5, 8])
def test_nan_writes_zero(emu, W):
    x = torch.rand(2, 3, 3, W)
    x[0, 0, 0, 0] = x[0, 1, 1, W - 1] = x[1, 2, 2, 3] = x[1, 0, 1, 4] = float("nan")
    x[1, 1, 0, 1] = torch.tensor([0x7F800001], dtype=torch.int32).view(torch.float32)[0]     # a signalling NaN
    s = emu()
    src, dst = s.vec(x.reshape(-1)), s.out(2 * 3 * W * 3, np.uint8)
    s.call(TO_U8, (2, 3, W, W * 3, 3 * W * 3, 3), (src, dst))
    assert s.run() == [0]
    got = s.get(dst, np.uint8).view(2, 3, W, 3).permute(0, 3, 1, 2)
    nan = torch.isnan(x)
    assert nan.sum() == 5 and (got[nan] == 0).all()
    assert torch.equal(got[~nan], K.ref_to_u8(torch.nan_to_num(x)).permute(0, 3, 1, 2)[~nan])


def test_geometry_u8_to_image(emu):
    g = torch.Generator().manual_seed(5)
    s, cases = emu(), []
    for N, H, W, C, rp, ip, off in K.geometry((1, 3, 4)):
        size, idx = K.layout(N, H, W, C, rp, ip, off)
        u8 = torch.randint(0, 256, (N, H, W, C), dtype=torch.uint8, generator=g)
        blk = np.full(size, 0xA5, np.uint8)
        blk[idx] = u8.numpy()
        src, dst = s.raw(blk, off), s.out(N * 3 * H * W)
        s.ro.append(src)
        s.call(TO_IMAGE, (rp, ip, N, H, W, C), (src, dst))
        cases.append(((N, H, W, C, rp, ip, off), dst, K.ref_to_image(u8)))
    assert s.run() == [0] * len(cases)
    for what, dst, want in cases:
        assert torch.equal(_bits(s.get(dst)), _bits(want.reshape(-1))), what


def test_geometry_image_to_u8(emu):
    g = torch.Generator().manual_seed(6)
    s, cases = emu(), []
    for N, H, W, C, rp, ip, off in K.geometry((3, 4)):
        size, idx = K.layout(N, H, W, C, rp, ip, off)
        x = torch.rand(N, 3, H, W, generator=g) * 1.2 - 0.1
        src, dst = s.vec(x.reshape(-1)), s.raw(np.full(size, K.FILL, np.uint8), off)
        s.call(TO_U8, (N, H, W, rp, ip, C), (src, dst))
        cases.append(((N, H, W, C, rp, ip, off), dst, idx, K.ref_to_u8(x, C)))
    assert s.run() == [0] * len(cases)
    for what, dst, idx, want in cases:
        after = s.after[dst]
        assert (after[idx] == want.numpy()).all(), what
        if want.shape[-1] == 4:
            assert (after[idx][..., 3] == 255).all(), what
        outside = np.ones(after.size, bool)
        outside[idx.reshape(-1)] = False
        assert (after[outside] == K.FILL).all(), (what, "a byte outside the rows' W * C runs was written")


def test_grey_is_replicated_and_alpha_ignored(emu):
    s = emu()
    grey = torch.tensor([[[[7], [200], [31]]]], dtype=torch.uint8)
    rgba = torch.tensor([[[[1, 2, 3, 9], [4, 5, 6, 99], [250, 251, 252, 0]]]], dtype=torch.uint8)
    a, b = s.out(9), s.out(9)
    s.call(TO_IMAGE, (3, 3, 1, 1, 3, 1), (s.vec(grey, np.uint8), a))
    s.call(TO_IMAGE, (12, 12, 1, 1, 3, 4), (s.vec(rgba, np.uint8), b))
    assert s.run() == [0, 0]
    ga, gb = s.get(a).view(3, 3), s.get(b).view(3, 3)
    assert torch.equal(ga[0], ga[1]) and torch.equal(ga[0], ga[2]) and torch.equal(ga[0], torch.tensor([7., 200., 31.]) / 255)
    assert torch.equal(gb, rgba[0, 0, :, :3].t().float() / 255)


def test_refusals(emu):
    s = emu()
    N, H, W = 2, 3, 5
    u8 = torch.randint(0, 256, (N, H, W, 4), dtype=torch.uint8)
    x = torch.rand(N, 3, H, W)
    src8, srcf = s.vec(u8, np.uint8), s.vec(x.reshape(-1))
    dstf, dst8 = s.out(N * 3 * H * W), s.out(N * H * W * 4, np.uint8)
    bad = []
    for C in (3, 4):
        rp, ip = W * C, H * W * C
        for n, h, w in ((0, H, W), (N, 0, W), (N, H, 0), (-1, H, W), (N, -2, W), (N, H, -3)):
            bad.append(s.call(TO_IMAGE, (rp, ip, n, h, w, C), (src8, dstf)))
            bad.append(s.call(TO_U8, (n, h, w, rp, ip, C), (srcf, dst8)))
        bad.append(s.call(TO_IMAGE, (rp - 1, ip, N, H, W, C), (src8, dstf)))
        bad.append(s.call(TO_U8, (N, H, W, rp - 1, ip, C), (srcf, dst8)))
        bad.append(s.call(TO_IMAGE, (rp, ip - 1, N, H, W, C), (src8, dstf)))
        bad.append(s.call(TO_U8, (N, H, W, rp, ip - 1, C), (srcf, dst8)))
        bad.append(s.call(TO_IMAGE, (rp, ip, N, H, W, C), (None, dstf)))
        bad.append(s.call(TO_IMAGE, (rp, ip, N, H, W, C), (src8, None)))
        bad.append(s.call(TO_U8, (N, H, W, rp, ip, C), (None, dst8)))
        bad.append(s.call(TO_U8, (N, H, W, rp, ip, C), (srcf, None)))
    for C in (0, 2, 5, -1):
        bad.append(s.call(TO_IMAGE, (W * 4, H * W * 4, N, H, W, C), (src8, dstf)))
    for C in (0, 1, 2, 5, -1):
        bad.append(s.call(TO_U8, (N, H, W, W * 4, H * W * 4, C), (srcf, dst8)))
    rcs = s.run()
    assert [rcs[k] for k in bad] == [E.ADH_E_ARG] * len(bad), rcs
    assert s.unchanged(dstf) and s.unchanged(dst8)


def test_image_pitch_is_not_looked_at_for_one_image(emu):
    s = emu()
    u8 = torch.randint(0, 256, (1, 2, 4, 3), dtype=torch.uint8)
    dstf = s.out(24)
    s.call(TO_IMAGE, (12, 0, 1, 2, 4, 3), (s.vec(u8, np.uint8), dstf))
    assert s.run() == [0]
    assert torch.equal(_bits(s.get(dstf)), _bits(K.ref_to_image(u8).reshape(-1)))
