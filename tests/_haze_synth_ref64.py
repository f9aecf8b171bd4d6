"""float64 reference of adh_batch_haze_from_u8 and adh_u16_resize_bilinear (csrc/dataset.hip) for tests/test_haze_synth_cpu.py
(which checks it against plain torch / numpy expressions), the host-emulated run and tests/test_gpu_haze_synth.py, plus the
case table the last two share and the fixture tree of clear files and depth maps.

The batch: v / 255, depth scaling or the radial map of the reference's `apply_random_fog` over the window, the scattering model
I = J t + A (1 - t), t = exp(-beta d), the clamp, then the flips and the ColorJitter of tests/_dataset_ref64.batch_ref."""
import os

import numpy as np

from tests import _dataset_ref64 as R
from tests import _pointwise_ref64 as P

EPS = 2.0 ** -24
U53 = 2.0 ** -53

# Double arithmetic of the model, kernel against numpy, for |beta| <= 4, |d| <= 2, A <= 1: at most 20 roundings per side (radial:
# two coordinates from an index and a step that is itself rounded, two differences, two squares, a sum, sqrt, * 0.7, + 0.3; or
# u / 65535, * span, + near; then * -beta, 1 - t, A *, J * t, the sum), each at a magnitude < 4 and so <= 2^-51 = 4 units of
# 2^-53, and passed on with a gain <= max(beta, 1) <= 4; exp itself within one ulp of a value <= 1 on either side (2 units
# each).  20 * 4 * 4 + 2, per side, twice: 644, stated as 1024 units of 2^-53 (1.1e-13, a millionth of the fp32 terms).
HAZE_F64_UNITS = 1024
# Without rows, fp32: the rounding of J = v / 255 (<= 2^-25 below 1, counted as 2^-24 like BATCH_BOUND does, scaled by t <= 1) and
# the cast of h <= 1 to float: 2.
HAZE_BOUND = 2 * EPS + HAZE_F64_UNITS * U53
# With rows: BATCH_BOUND's eight (v / 255, b * v, c * v, 1 - c, (1 - c) * mean, the sum, the mean and the grey values under it)
# plus the cast of h: 9.  The transform's gain on its input is b * c <= 1.21, applied to the float64 term.
HAZE_AUG_BOUND = 9 * EPS + 2 * HAZE_F64_UNITS * U53


def radial_depth(CH, CW):
    """float64 [CH, CW]: 0.3 + 0.7 * sqrt((x - 0.5)^2 + (y - 0.2)^2) on linspace(0, 1, CW) x linspace(0, 1, CH) (helpers.py:241-247)"""
    x, y = np.meshgrid(np.linspace(0, 1, CW), np.linspace(0, 1, CH))
    return 0.3 + 0.7 * np.sqrt((x - 0.5) ** 2 + (y - 0.2) ** 2)


def augment_ref(x, row):
    """x float64 [3, H, W], row {flip_h, flip_v, brightness_first, b, c} -> the flips and the jitter of R.batch_ref"""
    fh, fv, bfirst, b, c = [float(v) for v in np.asarray(row, dtype=np.float32).astype(np.float64)]
    if fh:
        x = x[:, :, ::-1]
    if fv:
        x = x[:, ::-1, :]

    def brightness(t):
        return np.clip(b * t, 0.0, 1.0)

    def contrast(t):
        mean = (R.GRAY[0] * t[0] + R.GRAY[1] * t[1] + R.GRAY[2] * t[2]).mean()
        return np.clip(c * t + (1.0 - c) * mean, 0.0, 1.0)
    return contrast(brightness(x)) if bfirst else brightness(contrast(x))


def haze_ref(clear, depth, fog, depth_range=(0.3, 1.0), params=None):
    """clear uint8 [N, CH, CW, 3] (the windows' bytes), depth uint16 [N, CH, CW] or None (radial), fog [N, 2] {beta, A} (their
    float32 values), params [N, 5] or None -> float64 [N, 3, CH, CW] = augment(fog(window))"""
    clear = np.asarray(clear)
    N, CH, CW, _ = clear.shape
    fog = np.asarray(fog, dtype=np.float32).astype(np.float64).reshape(N, 2)
    near, far = float(depth_range[0]), float(depth_range[1])
    out = []
    for n in range(N):
        J = clear[n].astype(np.float64).transpose(2, 0, 1) / 255.0
        d = radial_depth(CH, CW) if depth is None else near + (far - near) * (np.asarray(depth[n]).astype(np.float64) / 65535.0)
        t = np.exp(-fog[n, 0] * d)
        x = np.clip(J * t[None] + fog[n, 1] * (1.0 - t[None]), 0.0, 1.0)
        if params is not None:
            x = augment_ref(x, params[n])
        out.append(np.ascontiguousarray(x))
    return np.stack(out)


# ------------------------------------------------------------------------------------------------ 16-bit resize
# (h, w) -> (OH, OW), and the ratios at which every coordinate and weight is exact in fp32
RESIZE16_CASES = [((40, 56), (32, 32)), ((17, 67), (32, 32)), ((5, 3), (32, 32)), ((1, 1), (8, 8))]
RESIZE16_DYADIC = [((64, 64), (32, 32)), ((40, 40), (32, 32)), ((32, 24), (32, 24))]


def resize16_values(u16, OH, OW):
    """float64 [OH, OW]: R.resize_values on one channel of 16-bit levels"""
    x = np.asarray(u16).astype(np.float64)
    y0, y1, ly = R._axis(x.shape[0], OH)
    x0, x1, lx = R._axis(x.shape[1], OW)
    ly, lx = ly[:, None], lx[None, :]
    top = x[y0][:, x0] * (1 - lx) + x[y0][:, x1] * lx
    bot = x[y1][:, x0] * (1 - lx) + x[y1][:, x1] * lx
    return top * (1 - ly) + bot * ly


def resize16_delta(h, w, OH, OW):
    """R.resize_delta's count with 65535 levels in place of 255: how far the kernel's fp32 value may lie from the float64 one"""
    ds = P.src_err(h, OH, 0) + P.src_err(w, OW, 0)
    return 2 * 65535 * ds + 8 * 65535 * EPS


def check_resize16(got, u16, OH, OW, exact=False, what=""):
    """|got - value64| <= 0.5 + resize16_delta (delta exceeds one level at 16 bits, so a byte-equality rule with near-ties cannot
    work); exact: got == rint(value64) everywhere.  Returns the largest error."""
    h, w = np.asarray(u16).shape
    val = resize16_values(u16, OH, OW)
    got = np.asarray(got).astype(np.float64).reshape(val.shape)
    err = float(np.abs(got - val).max())
    bound = 0.0 if exact else 0.5 + resize16_delta(h, w, OH, OW)
    print(f"resize16 {what} {h}x{w}->{OH}x{OW}: max |got - value64| {err:.4f}, bound {bound:.4f}")
    if exact:
        assert np.array_equal(got, np.clip(np.rint(val), 0, 65535)), what
    else:
        assert err <= bound, (what, err, bound)
    return err


# ------------------------------------------------------------------------------------------------ cases
def _case(name, images, crop, windows, pack=4, base=0, dbase=0, out_off=0, gpu_only=False):
    """images: [(h, w)]; windows: [(image, y0, x0)]; pack 4 rounds every slot of both caches up to 4 bytes (data.HazeSynthDataset's
    layout: the dword paths), pack 1 packs tight; `base` / `dbase` bytes (dbase even) stand in front of the clear / depth cache,
    `out_off` floats in front of the output"""
    return dict(name=name, images=images, crop=crop, windows=windows, pack=pack, base=base, dbase=dbase, out_off=out_off,
                gpu_only=gpu_only)


# The smallest shapes that reach each way the kernels can go: 5 x 7 from caches that start on an odd byte / 2 mod 4 (every access
# byte by byte, level by level) behind an output off 16-byte alignment; 8 x 12 with x0 = 0, 1, 2, 3 (clear phases 0, 3, 2, 1, depth
# phases 0 and 2), the last window ending on the last byte of both caches, out aligned and not; 1 x 9 and 9 x 1 (the radial map's
# one-pixel axes); 40 x 130 (two blocks of the mean pass, quads that straddle rows, a partial quad at the right edge); caches that
# start on a multiple of 4 and end off one (65 pixels: 195 and 130 bytes); on the GPU alone 512 x 516 (65 mean blocks).
CASES = [
    _case("5x7_bytes", [(7, 9), (6, 11), (5, 7)], (5, 7), [(0, 1, 1), (1, 0, 3), (2, 0, 0)], pack=1, base=1, dbase=2, out_off=1),
    _case("8x12_phases", [(9, 16), (8, 15), (10, 12), (8, 12)], (8, 12), [(0, 0, 0), (0, 1, 1), (1, 0, 2), (1, 0, 3), (3, 0, 0)]),
    _case("8x12_out_off", [(9, 16), (8, 15), (8, 12)], (8, 12), [(0, 1, 3), (1, 0, 1), (2, 0, 0)], out_off=1),
    _case("1x9", [(3, 12), (1, 9)], (1, 9), [(0, 2, 3), (0, 0, 1), (1, 0, 0)]),
    _case("9x1", [(12, 3), (9, 1)], (9, 1), [(0, 2, 1), (1, 0, 0)]),
    _case("40x130", [(41, 133), (40, 130)], (40, 130), [(0, 1, 3), (0, 0, 2), (1, 0, 0)]),
    _case("tight_end_off_4", [(5, 9), (4, 5)], (3, 5), [(0, 1, 2), (1, 1, 0)], pack=1),
    _case("tight_base_3_cw8", [(5, 9), (6, 10)], (5, 8), [(0, 0, 1), (1, 1, 2)], pack=1, base=3, dbase=2),
    _case("512x516", [(513, 519), (2, 2)], (512, 516), [(0, 1, 3)], gpu_only=True),
]


def build(case):
    """-> clear uint8 flat cache, depth uint16 flat cache (both without the bytes in front), geom int64 [N, 4] relative to their
    first bytes, the dense uint8 [N, CH, CW, 3] and uint16 [N, CH, CW] copies of the windows, and fog float32 [N, 2]"""
    seed = sum(ord(ch) for ch in case["name"])
    rng = np.random.RandomState(seed)
    pack, (CH, CW) = case["pack"], case["crop"]
    imgs, deps, coff, doff, cat, dat = [], [], [], [], 0, 0
    for k, (h, w) in enumerate(case["images"]):
        imgs.append(R.all_values_cache(3, h, w, seed + k)[0])
        d = rng.randint(0, 65536, size=(h, w)).astype(np.uint16)
        d.reshape(-1)[rng.permutation(d.size)[:2]] = (0, 65535)[:min(2, d.size)]
        deps.append(d)
        coff.append(cat)
        doff.append(dat)
        cat += -(-h * w * 3 // pack) * pack
        dat += -(-h * w * 2 // pack) * pack
    clear = np.full(cat, 0xA5, np.uint8)                              # the padding between slots is a byte nothing may depend on
    depth = np.full(dat // 2, 0xA5A5, np.uint16)
    for img, d, co, do in zip(imgs, deps, coff, doff):
        clear[co:co + img.size] = img.reshape(-1)
        depth[do // 2:do // 2 + d.size] = d.reshape(-1)
    geom, dc, dd = [], [], []
    for k, y0, x0 in case["windows"]:
        h, w = deps[k].shape
        assert 0 <= y0 <= h - CH and 0 <= x0 <= w - CW, case["name"]
        geom.append([coff[k] + (y0 * w + x0) * 3, w * 3, doff[k] + (y0 * w + x0) * 2, w * 2])
        dc.append(imgs[k][y0:y0 + CH, x0:x0 + CW])
        dd.append(deps[k][y0:y0 + CH, x0:x0 + CW])
    N = len(geom)
    fog = np.stack([rng.uniform(0.1, 1.0, N), rng.uniform(0.5, 1.0, N)], axis=1).astype(np.float32)
    return clear, depth, np.array(geom, np.int64), np.ascontiguousarray(np.stack(dc)), np.ascontiguousarray(np.stack(dd)), fog


def dense_geom(N, CH, CW):
    """int64 [N, 4]: the geometry that serves a dense [N, CH, CW, 3] / [N, CH, CW] pair of caches"""
    i = np.arange(N, dtype=np.int64)
    return np.stack([i * CH * CW * 3, np.full(N, CW * 3), i * CH * CW * 2, np.full(N, CW * 2)], axis=1).astype(np.int64)


# ------------------------------------------------------------------------------------------------ fixture tree
def write_tree(root, splits=(("train", 6), ("val", 4)), seed=0, depth=True):
    """<root>/<split>/clear/<name> with mixed 32x32 and 40x56 files (.png and .jpg) and, with `depth`, <root>/<split>/depth/<stem>.png:
    16-bit grey, but 8-bit grey for the first file of every split.  Returns {split: [name]} in index order."""
    from PIL import Image
    rng = np.random.RandomState(seed)
    listing = {}
    for split, n in splits:
        names = sorted(f"im{k}" + (".jpg" if k % 3 == 2 else ".png") for k in range(n))
        os.makedirs(os.path.join(root, split, "clear"), exist_ok=True)
        if depth:
            os.makedirs(os.path.join(root, split, "depth"), exist_ok=True)
        for k, name in enumerate(names):
            h, w = (40, 56) if k % 2 == 0 else (32, 32)
            Image.fromarray(rng.randint(0, 256, size=(h, w, 3)).astype(np.uint8)).save(os.path.join(root, split, "clear", name))
            if depth:
                stem = os.path.splitext(name)[0] + ".png"
                if k == 0:
                    Image.fromarray(rng.randint(0, 256, size=(h, w)).astype(np.uint8)).save(os.path.join(root, split, "depth", stem))
                else:
                    Image.fromarray(rng.randint(0, 65536, size=(h, w)).astype(np.uint16)).save(os.path.join(root, split, "depth", stem))
        listing[split] = names
    return listing
