"""float64 references of csrc/dataset.hip for tests/test_dataset_cpu.py (which checks them against torch), the host-emulated run
and tests/test_gpu_dataset.py: the bilinear resize of 8-bit images (numpy) and the batch assembly (v / 255, flips, torchvision's
float ColorJitter in both orders), plus the near-tie rule the byte comparison of the resize uses and the fixtures' files."""
import os

import numpy as np

from tests import _pointwise_ref64 as P

EPS = 2.0 ** -24
GRAY = (0.2989, 0.587, 0.114)

# (h, w) -> (OH, OW): general ratios, an upscale, a one-pixel source
RESIZE_CASES = [((40, 56), (32, 32)), ((17, 67), (32, 32)), ((5, 3), (32, 32)), ((33, 47), (16, 24)), ((1, 1), (8, 8))]
# dyadic ratios: every coordinate and weight is exact in fp32, so the bytes are equal with no exception
RESIZE_DYADIC = [((64, 64), (32, 32)), ((128, 64), (32, 32)), ((40, 40), (32, 32))]
NEAR_TIE_SHARE = 0.05


def rgb3(u8):
    """[h, w, C] (C = 1, 3, 4) -> [h, w, 3]: grey replicated, alpha dropped"""
    u8 = np.asarray(u8)
    return np.repeat(u8, 3, axis=2) if u8.shape[2] == 1 else u8[:, :, :3]


def _axis(n_in, n_out):
    s = np.maximum((np.arange(n_out, dtype=np.float64) + 0.5) * (n_in / n_out) - 0.5, 0.0)
    i0 = np.minimum(np.floor(s).astype(np.int64), n_in - 1)
    i1 = np.minimum(i0 + 1, n_in - 1)
    return i0, i1, s - i0


def resize_values(u8, OH, OW):
    """the interpolated values before rounding, float64 [OH, OW, 3]: source coordinate max((d + 0.5) * in / out - 0.5, 0), the
    upper neighbour clamped to the last row / column, no antialiasing"""
    x = rgb3(u8).astype(np.float64)
    y0, y1, ly = _axis(x.shape[0], OH)
    x0, x1, lx = _axis(x.shape[1], OW)
    ly, lx = ly[:, None, None], lx[None, :, None]
    top = x[y0][:, x0] * (1 - lx) + x[y0][:, x1] * lx
    bot = x[y1][:, x0] * (1 - lx) + x[y1][:, x1] * lx
    return top * (1 - ly) + bot * ly


def resize_bytes(values):
    """rint (halves to even), clamped to 0..255"""
    return np.clip(np.rint(values), 0, 255).astype(np.uint8)


def resize_delta(h, w, OH, OW):
    """How far the kernel's fp32 value may lie from the float64 one, in grey levels.  The coordinate of each axis is off by at
    most src_err (tests/_pointwise_ref64.py: the kernel evaluates adh_bilinear's fp32 formula), which moves that axis's weight
    by as much and the value by at most that times the neighbour difference <= 255; a coordinate that crosses an integer
    swaps the pair of neighbours continuously, so the same bound holds: 255 * ds, counted twice (255 * 2) for the weight and
    its complement 1 - l, each rounded from the same coordinate.  Value roundings, each <= 255 * 2^-24: 1 - lx, 1 - ly (2), per
    row two products and a sum (3, the rows in parallel), the product with the row weight (1), the final sum (1), the
    conversion of the coordinate difference l = src - i0 (1): 8."""
    ds = P.src_err(h, OH, 0) + P.src_err(w, OW, 0)
    return 2 * 255 * ds + 8 * 255 * EPS


def check_resize(got, u8, OH, OW, exact=False, what=""):
    """bytes equal everywhere, except +-1 where the float64 value lies within resize_delta of a half-integer; the share of
    such pixels is at most NEAR_TIE_SHARE.  exact: no exception at all.  Returns the share."""
    h, w = u8.shape[:2]
    val = resize_values(u8, OH, OW)
    ref = resize_bytes(val).astype(np.int64)
    got = np.asarray(got).astype(np.int64).reshape(ref.shape)
    near = np.zeros(val.shape, bool) if exact else np.abs(val - (np.floor(val) + 0.5)) <= resize_delta(h, w, OH, OW)
    diff = np.abs(got - ref)
    share = float(near.mean())
    print(f"resize {what} {h}x{w}->{OH}x{OW}: near-tie share {share:.4f}, differing bytes {int((diff > 0).sum())}, "
          f"max |diff| {int(diff.max())}")
    assert share <= NEAR_TIE_SHARE, (what, share)
    assert (diff[~near] == 0).all(), (what, "bytes differ outside near-ties", int((diff[~near] > 0).sum()))
    assert (diff[near] <= 1).all(), (what, "a near-tie is off by more than one grey level")
    return share


def batch_ref(cache, index, params=None):
    """cache uint8 [M, H, W, 3], index ints, params [N, 5] rows {flip_h, flip_v, brightness_first, b, c} (their float32
    values) or None -> float64 [N, 3, H, W]: v / 255, RandomHorizontalFlip, RandomVerticalFlip, then torchvision's ColorJitter
    for float images: brightness clamp(b * x, 0, 1), contrast clamp(c * x + (1 - c) * mean(grey(x)), 0, 1) with the mean
    over the whole image the contrast step sees, in the order brightness_first says."""
    cache = np.asarray(cache)
    out = []
    for n, i in enumerate(np.asarray(index).tolist()):
        x = cache[i].astype(np.float64).transpose(2, 0, 1) / 255.0
        if params is not None:
            fh, fv, bfirst, b, c = [float(v) for v in np.asarray(params, dtype=np.float32)[n].astype(np.float64)]
            if fh:
                x = x[:, :, ::-1]
            if fv:
                x = x[:, ::-1, :]

            def brightness(t):
                return np.clip(b * t, 0.0, 1.0)

            def contrast(t):
                mean = (GRAY[0] * t[0] + GRAY[1] * t[1] + GRAY[2] * t[2]).mean()
                return np.clip(c * t + (1.0 - c) * mean, 0.0, 1.0)
            x = contrast(brightness(x)) if bfirst else brightness(contrast(x))
        out.append(np.ascontiguousarray(x))
    return np.stack(out)


# fp32 roundings of the jittered value at magnitudes <= 1.21 (half an ulp <= 2^-24 there): v / 255, b * v, c * v, 1 - c,
# (1 - c) * mean, the sum, the rounding of the mean itself and of the grey values under it (both scaled by |1 - c| <= 0.1): 8
BATCH_BOUND = 8 * EPS


def all_values_cache(M, Hh, Ww, seed):
    """uint8 [M, H, W, 3] holding all 256 byte values where H * W * 3 * (M - 2) allows, image M-2 all 0 and M-1 all 255"""
    rng = np.random.RandomState(seed)
    c = rng.randint(0, 256, size=(M, Hh, Ww, 3)).astype(np.uint8)
    flat = c[:M - 2].reshape(-1)
    n = min(256, flat.size)
    flat[rng.permutation(flat.size)[:n]] = np.arange(n, dtype=np.uint8)
    c[M - 2], c[M - 1] = 0, 255
    return c


# ------------------------------------------------------------------------------------------------ fixture trees
def write_tree(root, splits=(("train", 4), ("val", 2), ("test", 2)), seed=0, sub_split=True):
    """<root>/<split>/{low,medium,high}/{hazy,clear}/<name> (or <root>/{low,...} for one split when not sub_split) with n files
    per level: mixed 40x56 and 32x32, .png and .jpg, one grey and one RGBA file per split.  Returns {split: [(level, name)]}
    in index order."""
    from PIL import Image
    rng = np.random.RandomState(seed)
    listing = {}
    for split, n in splits:
        base = os.path.join(root, split) if sub_split else root
        listing[split] = []
        for li, level in enumerate(("low", "medium", "high")):
            names = sorted(f"im{li}{k}" + (".jpg" if (k + li) % 3 == 2 else ".png") for k in range(n))
            for k, name in enumerate(names):
                h, w = (40, 56) if (k + li) % 2 == 0 else (32, 32)
                for role in ("hazy", "clear"):
                    d = os.path.join(base, level, role)
                    os.makedirs(d, exist_ok=True)
                    a = rng.randint(0, 256, size=(h, w, 3)).astype(np.uint8)
                    if name.endswith(".png") and li == 0 and k == 0 and role == "hazy":
                        im = Image.fromarray(a[:, :, 0])                             # grey
                    elif name.endswith(".png") and li == 1 and k == 0 and role == "hazy":
                        im = Image.fromarray(np.concatenate([a, a[:, :, :1]], axis=2))   # RGBA
                    else:
                        im = Image.fromarray(a)
                    im.save(os.path.join(d, name))
                listing[split].append((level, name))
    return listing
