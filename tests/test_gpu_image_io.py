"""csrc/image_io.hip on the GPU through image_io.u8_to_image / image_to_u8: the exhaustive, quantiser-edge and geometry cases of
tests/test_image_io_hostemu_cpu.py, bit for bit against the torch CPU expressions of tests/_image_io_cases.py.  Pitched and offset
cases are views into a larger device tensor filled with 0x5A, which must still hold it everywhere outside the rows' W * C runs."""
import numpy as np
import pytest
import torch

from adam_dehaze_amd import image_io as IO
from tests import _image_io_cases as K

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _bits(t):
    return t.contiguous().view(torch.int32)


def _view(N, H, W, C, rp, ip, off):
    """(a 0x5A-filled device buffer with 64 spare bytes behind the addressed ones, the [N,H,W,C] view into it, the buffer index
    of every byte of the view)"""
    size, idx = K.layout(N, H, W, C, rp, ip, off)
    buf = torch.full((size + 64,), K.FILL, dtype=torch.uint8, device=DEV)
    return buf, torch.as_strided(buf, (N, H, W, C), (ip, rp, C, 1), off), idx


def test_all_256_values_and_back():
    u8 = torch.arange(256, dtype=torch.uint8).view(1, 16, 16, 1)
    img = IO.u8_to_image(u8.to(DEV))
    assert tuple(img.shape) == (1, 3, 16, 16) and img.dtype == torch.float32
    want = torch.arange(256).float() / 255
    for c in range(3):
        assert torch.equal(_bits(img[0, c].cpu().reshape(-1)), _bits(want)), f"plane {c}"
    back = IO.image_to_u8(img).cpu()
    assert torch.equal(back.view(256, 3), torch.arange(256, dtype=torch.uint8)[:, None].expand(256, 3))
    # [H,W,C] is one image
    assert torch.equal(_bits(IO.u8_to_image(u8[0].to(DEV)).cpu()), _bits(img.cpu()))


@pytest.mark.parametrize("W", [130, 132])
@pytest.mark.parametrize("C", [3, 4])
def test_quantiser_edges(W, C):
    x = K.edge_image(W)
    got, want = IO.image_to_u8(x.to(DEV), channels=C).cpu(), K.ref_to_u8(x, C)
    bad = (got != want).nonzero()
    assert bad.numel() == 0, bad[:5].tolist()
    flat = got[..., :3].permute(0, 3, 1, 2).reshape(-1)[:K.edge_values().numel()]
    assert flat[-8:].tolist() == [0, 0, 255, 255, 0, 255, 0, 255]      # 0, -0.0, 1, nextafter(1, 2), -1e-7, inf, -inf, 1e30


@pytest.mark.parametrize("W", [5, 8])
def test_nan_writes_zero(W):
    torch.manual_seed(2)
    x = torch.rand(2, 3, 3, W)
    x[0, 0, 0, 0] = x[0, 1, 1, W - 1] = x[1, 2, 2, 3] = x[1, 0, 1, 4] = float("nan")
    x[1, 1, 0, 1] = torch.tensor([0x7F800001], dtype=torch.int32).view(torch.float32)[0]     # a signalling NaN
    got = IO.image_to_u8(x.to(DEV)).cpu().permute(0, 3, 1, 2)
    nan = torch.isnan(x)
    assert nan.sum() == 5 and (got[nan] == 0).all()
    assert torch.equal(got[~nan], K.ref_to_u8(torch.nan_to_num(x)).permute(0, 3, 1, 2)[~nan])


def test_geometry_u8_to_image():
    g = torch.Generator().manual_seed(5)
    for N, H, W, C, rp, ip, off in K.geometry((1, 3, 4)):
        u8 = torch.randint(0, 256, (N, H, W, C), dtype=torch.uint8, generator=g)
        buf, view, _ = _view(N, H, W, C, rp, ip, off)
        view.copy_(u8.to(DEV))
        before = buf.clone()
        got = IO.u8_to_image(view)
        assert torch.equal(_bits(got.cpu()), _bits(K.ref_to_image(u8))), (N, H, W, C, rp, ip, off)
        assert torch.equal(buf, before), (N, H, W, C, rp, ip, off)


def test_geometry_image_to_u8():
    g = torch.Generator().manual_seed(6)
    for N, H, W, C, rp, ip, off in K.geometry((3, 4)):
        what = (N, H, W, C, rp, ip, off)
        x = torch.rand(N, 3, H, W, generator=g) * 1.2 - 0.1
        buf, view, idx = _view(N, H, W, C, rp, ip, off)
        assert IO.image_to_u8(x.to(DEV), out=view) is view
        after, want = buf.cpu().numpy(), K.ref_to_u8(x, C).numpy()
        assert (after[idx] == want).all(), what
        if C == 4:
            assert (after[idx][..., 3] == 255).all(), what
        outside = np.ones(after.size, bool)
        outside[idx.reshape(-1)] = False
        assert (after[outside] == K.FILL).all(), (what, "a byte outside the rows' W * C runs was written")


def test_two_images_side_by_side_in_one_panel():
    g = torch.Generator().manual_seed(7)
    a, b = torch.rand(1, 3, 5, 7, generator=g), torch.rand(1, 3, 5, 7, generator=g)
    panel = torch.full((5, 14, 3), K.FILL, dtype=torch.uint8, device=DEV)
    IO.image_to_u8(a.to(DEV), out=panel[:, :7])
    IO.image_to_u8(b.to(DEV), out=panel[:, 7:])
    dense = [IO.image_to_u8(t.to(DEV))[0] for t in (a, b)]
    assert torch.equal(panel, torch.cat(dense, dim=1))
    assert torch.equal(panel.cpu(), torch.cat([K.ref_to_u8(a)[0], K.ref_to_u8(b)[0]], dim=1))
    # and a crop is read in place
    crop = panel[1:4, 3:12]
    assert torch.equal(_bits(IO.u8_to_image(crop).cpu()), _bits(K.ref_to_image(crop.cpu().unsqueeze(0))))


def test_what_the_module_refuses():
    u8 = torch.zeros((2, 4, 6, 3), dtype=torch.uint8, device=DEV)
    with pytest.raises(ValueError, match="dense"):
        IO.u8_to_image(u8[:, :, ::2])
    with pytest.raises(ValueError, match="dense"):
        IO.u8_to_image(u8[..., :2])
    with pytest.raises(RuntimeError, match="ADH_E_ARG"):
        IO.u8_to_image(torch.zeros((1, 4, 6, 2), dtype=torch.uint8, device=DEV))
    with pytest.raises(RuntimeError, match="ADH_E_ARG"):
        IO.image_to_u8(torch.zeros((1, 3, 4, 6), device=DEV), channels=1)
    with pytest.raises(RuntimeError, match="uint8"):
        IO.u8_to_image(torch.zeros((1, 4, 6, 3), dtype=torch.uint8))
    with pytest.raises(ValueError, match="does not match"):
        IO.image_to_u8(torch.zeros((1, 3, 4, 6), device=DEV), out=u8[:1, :, :5])
