"""The cases of adh_batch_window_from_u8 for the host-emulated run (tests/test_dataset_window_hostemu_cpu.py) and the GPU
(tests/test_gpu_dataset_crop.py): flat caches built from three or four images of unequal size -- random bytes that hold all 256
values, the all-0 and the all-255 image of tests/_dataset_ref64.all_values_cache -- and windows into them.

The shapes are the smallest that reach each way the kernel can go: CW 1 and 3 (no whole quad), 4, 5 and 8 (whole quads, with and
without a partial one at the right edge), 67, 260 (a second block column: a block covers 256 output columns); CH 1, 2, 5 and 9
(the row loop past its four rows per block); origins at 0 and at the maximum of each axis, x0 % 4 in {0, 1, 2, 3}; image widths
with W * 3 % 4 in {0, 1, 2, 3}, so the phase of a quad's address changes from row to row; a window that is a whole image, the one
that starts at byte 0 and the one that ends with the cache's last byte; one window twice in a batch; N = 1 and 3; 40 x 130 (5,200
pixels: two blocks of the mean pass, and quads that straddle rows because 130 % 4 != 0); on the GPU alone 512 x 516 (65 blocks of
the mean pass, so the lane + 64 term of the wave sum runs).  pack 4 lays the images out as data.FolderDataset does (every slot
and the total rounded up to 4: the dword path); pack 1 packs them tight behind `base` odd bytes and the output `out_off` floats
off 16-byte alignment (the byte and single-float paths)."""
import itertools

import numpy as np

from tests import _dataset_ref64 as R

RAND, ZERO, FULL = 0, 1, 2      # which image of all_values_cache(3, h, w, seed) an image of the case is

# the 72 parameter rows {flip_h, flip_v, brightness_first, b, c}
ROWS = [[fh, fv, bf, b, c] for fh, fv, bf, b, c in itertools.product((0, 1), (0, 1), (0, 1), (0.9, 1.0, 1.1), (0.9, 1.0, 1.1))]


def _case(name, images, crop, windows, pack=4, base=0, out_off=0, gpu_only=False):
    """images: [((h, w), kind)]; windows: [(image, y0, x0)]"""
    return dict(name=name, images=images, crop=crop, windows=windows, pack=pack, base=base, out_off=out_off, gpu_only=gpu_only)


CASES = [
    _case("cw1_ch5", [((7, 9), RAND), ((5, 6), RAND), ((3, 3), ZERO), ((5, 4), FULL)], (5, 1), [(0, 0, 0), (0, 2, 8), (1, 0, 5)]),
    _case("cw3_ch2_whole_image", [((6, 10), RAND), ((9, 7), RAND), ((2, 3), ZERO), ((4, 5), FULL)], (2, 3),
          [(0, 4, 7), (1, 7, 1), (2, 0, 0)]),
    _case("cw4_ch9_phases", [((9, 11), RAND), ((12, 13), RAND), ((9, 4), ZERO), ((10, 6), FULL)], (9, 4),
          [(0, 0, 1), (1, 3, 2), (1, 1, 7)]),
    _case("cw4_ch9_zero_and_full", [((9, 11), RAND), ((12, 13), RAND), ((9, 4), ZERO), ((10, 6), FULL)], (9, 4),
          [(2, 0, 0), (3, 1, 2), (0, 0, 4)]),
    _case("cw5_ch1_n1", [((3, 9), RAND), ((2, 6), ZERO), ((1, 5), FULL)], (1, 5), [(0, 2, 4)]),
    _case("cw8_ch5_first_and_last_byte", [((5, 8), RAND), ((6, 10), RAND), ((7, 9), ZERO), ((8, 8), FULL)], (5, 8),
          [(0, 0, 0), (3, 3, 0), (1, 1, 2)]),
    _case("cw8_ch5_out_off", [((5, 8), RAND), ((6, 10), RAND), ((7, 9), ZERO), ((8, 8), FULL)], (5, 8),
          [(1, 0, 1), (0, 0, 0), (1, 1, 2)], out_off=1),
    _case("cw67_ch2", [((3, 70), RAND), ((2, 67), ZERO), ((4, 69), FULL), ((5, 68), RAND)], (2, 67),
          [(0, 1, 3), (3, 3, 1), (2, 2, 2)]),
    _case("cw260_ch2_twice", [((3, 263), RAND), ((2, 261), ZERO), ((2, 260), FULL)], (2, 260), [(0, 1, 3), (0, 1, 3), (2, 0, 0)]),
    _case("40x130", [((41, 133), RAND), ((43, 130), RAND), ((40, 130), ZERO), ((40, 131), FULL)], (40, 130),
          [(0, 1, 3), (1, 3, 0), (3, 0, 1)]),
    _case("tight_odd_base_n1_last_byte", [((6, 7), RAND), ((3, 6), ZERO), ((4, 5), FULL)], (2, 5), [(2, 2, 0)], pack=1, base=1,
          out_off=1),
    _case("tight_odd_base", [((6, 7), RAND), ((5, 9), RAND), ((3, 6), ZERO), ((4, 5), FULL)], (2, 5),
          [(0, 0, 0), (3, 2, 0), (1, 3, 4)], pack=1, base=1, out_off=1),
    _case("tight_cw8", [((5, 9), RAND), ((7, 11), RAND), ((5, 8), ZERO), ((6, 10), FULL)], (5, 8), [(0, 0, 1), (1, 2, 3), (3, 1, 2)],
          pack=1, base=3),
    _case("512x516", [((513, 519), RAND), ((2, 2), ZERO), ((512, 516), FULL)], (512, 516), [(0, 1, 3)], gpu_only=True),
]


def build(case):
    """-> flat uint8 cache (without the `base` bytes in front), int64 windows [N, 2] relative to its first byte, and the dense
    uint8 [N, CH, CW, 3] copy of the windows' bytes"""
    seed = sum(ord(ch) for ch in case["name"])
    pack, (CH, CW) = case["pack"], case["crop"]
    imgs, offsets, at = [], [], 0
    for k, ((h, w), kind) in enumerate(case["images"]):
        imgs.append(R.all_values_cache(3, h, w, seed + k)[kind])
        offsets.append(at)
        at += -(-h * w * 3 // pack) * pack
    flat = np.full(at, 0xA5, np.uint8)                                # the padding between slots is a byte nothing may depend on
    for img, o in zip(imgs, offsets):
        flat[o:o + img.size] = img.reshape(-1)
    windows, dense = [], []
    for k, y0, x0 in case["windows"]:
        h, w = imgs[k].shape[:2]
        assert 0 <= y0 <= h - CH and 0 <= x0 <= w - CW, case["name"]
        windows.append([offsets[k] + (y0 * w + x0) * 3, w * 3])
        dense.append(imgs[k][y0:y0 + CH, x0:x0 + CW])
    return flat, np.array(windows, np.int64), np.ascontiguousarray(np.stack(dense))


def param_sets(case_no, N, count):
    """`count` float32 [N, 5] blocks of ROWS; consecutive samples are 7 rows apart (7 and 72 are coprime), so 72 / N blocks hold
    every row once and a few blocks per case still cover, over the table, every flip pair, both jitter orders and every b, c"""
    return [np.array([ROWS[((case_no * 6 + k * N + j) * 7) % len(ROWS)] for j in range(N)], np.float32) for k in range(count)]


def window_mask(flat_size, windows, crop):
    """bool [flat_size]: the bytes that belong to a window"""
    CH, CW = crop
    m = np.zeros(flat_size, bool)
    for off, pitch in np.asarray(windows).tolist():
        for y in range(CH):
            m[off + y * pitch: off + y * pitch + CW * 3] = True
    return m
