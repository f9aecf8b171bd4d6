"""Shared by tests/test_image_io_hostemu_cpu.py and tests/test_gpu_image_io.py: the torch CPU expressions csrc/image_io.hip must
match bit for bit, the quantiser's edge inputs, and the pitched / offset layouts of the geometry cases."""
import itertools

import numpy as np
import torch

FILL = 0x5A                                  # every byte of an 8-bit output block before the call
SHAPES = [(1, 1, 1), (1, 1, 3), (1, 2, 4), (2, 3, 5), (1, 5, 16), (2, 7, 17), (1, 3, 67),
          (1, 2, 260)]                       # the last one: a second workgroup in x (a workgroup covers 256 pixels of a row)
ROW_PADS = (0, 1, 5)                         # row_pitch = W * C + pad
OFFSETS = (0, 1, 3)                          # bytes in front of the first pixel
IMAGE_PADS = (0, 8, 7)                       # image_pitch = H * row_pitch + pad: exact; padded, dwords still possible; padded, odd


def geometry(channels):
    """(N, H, W, C, row_pitch, image_pitch, off) of every geometry case"""
    for (N, H, W), C, rpad, off, ipad in itertools.product(SHAPES, channels, ROW_PADS, OFFSETS, IMAGE_PADS):
        rp = W * C + rpad
        yield N, H, W, C, rp, H * rp + ipad, off


def layout(N, H, W, C, rp, ip, off):
    """(bytes of the block: `off` in front, then exactly the addressed bytes; the block index of byte (n, y, x, c))"""
    n, y, x, c = np.ix_(np.arange(N), np.arange(H), np.arange(W), np.arange(C))
    return off + (N - 1) * ip + (H - 1) * rp + W * C, off + n * ip + y * rp + x * C + c


def ref_to_image(u8):
    """[N,H,W,C] uint8 -> [N,3,H,W] float32: float(v) / 255.0f, grey replicated, alpha ignored"""
    x = u8.to(torch.float32) / 255
    x = x.expand(-1, -1, -1, 3) if x.shape[-1] == 1 else x[..., :3]
    return x.permute(0, 3, 1, 2).contiguous()


def ref_to_u8(x, channels=3):
    """[N,3,H,W] float32 (no NaN) -> [N,H,W,C] uint8, alpha 255"""
    q = (x.clamp(0, 1) * 255).round().to(torch.uint8).permute(0, 2, 3, 1)
    if channels == 4:
        q = torch.cat([q, torch.full_like(q[..., :1], 255)], dim=-1)
    return q.contiguous()


def edge_values():
    """fp32((k + 0.5) / 255) and its two neighbours for k = 0..254, then the special inputs"""
    h = ((np.arange(255, dtype=np.float64) + 0.5) / 255).astype(np.float32)
    v = np.concatenate([np.nextafter(h, np.float32(-1)), h, np.nextafter(h, np.float32(2)),
                        np.array([0.0, -0.0, 1.0, np.nextafter(np.float32(1), np.float32(2)), -1e-7, np.inf, -np.inf, 1e30],
                                 np.float32)])
    assert v.dtype == np.float32
    return torch.from_numpy(v)


def edge_image(W):
    """the edge values as a [1,3,H,W] tensor (padded with 0.25): W % 4 picks the planar access width"""
    v = edge_values()
    H = -(-v.numel() // (3 * W))
    x = torch.full((3 * H * W,), 0.25)
    x[:v.numel()] = v
    return x.view(1, 3, H, W)
