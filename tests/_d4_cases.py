"""Shared by tests/test_d4_hostemu_cpu.py and tests/test_gpu_d4.py (not a test file): the torch CPU reference of adh_d4_apply
(csrc/d4.hip), the shape list of the bit-equality sweep and the fill helpers."""
import torch

OPS = [(0, 0), (0, 1), (0, 2), (0, 3), (1, 0), (1, 1), (1, 2), (1, 3)]          # (transpose, flips)
# 33 / 64 / 65 / 129 straddle the transposing kernel's 64 x 64 tile (63 comes with the 31- and 129-wide cases' remainders; the
# 4-wide quads of the streaming kernel are straddled by 1, 3, 5, 7, 45, 67)
HW = [(1, 1), (1, 7), (7, 1), (3, 5), (4, 4), (16, 20), (31, 45), (32, 48), (33, 64), (64, 33), (65, 130), (129, 67), (63, 63)]
NC = [(1, 3), (2, 3), (3, 1)]
FILL = 0x5A5A5A5A        # the int32 pattern of an output nothing has written (0x5A bytes)


def ref(src, transpose, flips):
    """the element definition: transpose, then mirror along x if bit 0 of `flips` is set, along y if bit 1 is"""
    t = src.transpose(-1, -2) if transpose else src
    dims = [d for d, bit in ((-1, 1), (-2, 2)) if flips & bit]
    return (t.flip(dims) if dims else t).contiguous()


def ref_per_image(src, transpose, codes):
    """`ref` with one flip code per image, masked as the kernel masks it"""
    return torch.stack([ref(src[n], transpose, int(c) & 3) for n, c in enumerate(codes)])


def out_shape(N, C, H, W, transpose):
    return (N, C, W, H) if transpose else (N, C, H, W)


def distinct(N, C, H, W):
    """every element another value, exactly representable: a wrong index shows as a wrong number"""
    return torch.arange(N * C * H * W, dtype=torch.float32).reshape(N, C, H, W) - 7.0


def random(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed))


def bits(t):
    return t.contiguous().view(torch.int32)
