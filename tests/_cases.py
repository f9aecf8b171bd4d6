"""Input families shared by tests/test_ref64_cpu.py and the kernel-level GPU tests: built on the CPU from fixed seeds, so
that the properties the GPU tests rely on (exact decisions, margins to decision boundaries) can be asserted without a GPU."""
import torch

from tests import _ref64 as R64

EPS = 2.0 ** -24
BOXPOST_NC = [2, 5, 64, 65, 91, 129]


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def int_boxes(M, seed, ngroups=1, zero_area=False, span=200, max_side=60):
    """M boxes on integer coordinates below 2^11: every area, intersection and union is exact in fp32 (products below
    2^24) with or without FMA contraction, and the one division is correctly rounded in fp32 and fp64 alike, so
    `IoU > thr` is the same decision on both sides.  Every 11th box repeats its predecessor; with zero_area every 7th
    box has zero width, height or both (IoU with another zero-area box: 0 / 0)."""
    g = _gen(seed)
    xy = torch.randint(0, span, (M, 2), generator=g)
    wh = torch.randint(1, max_side + 1, (M, 2), generator=g)
    if zero_area:
        k = torch.arange(0, M, 7)
        wh[k, 0] = torch.where(k % 3 != 1, 0, wh[k, 0])
        wh[k, 1] = torch.where(k % 3 != 0, 0, wh[k, 1])
    b = torch.cat([xy, xy + wh], 1)
    d = torch.arange(11, max(M, 11), 11)
    b[d] = b[d - 1]
    groups = torch.randint(0, ngroups, (M,), generator=g, dtype=torch.int32)
    groups[d] = groups[d - 1]
    return b.float(), groups


def nms_hand_cases():
    """name -> (boxes, groups, thr, expected keep)."""
    f = lambda rows: torch.tensor(rows, dtype=torch.float32)
    z = lambda n: torch.zeros(n, dtype=torch.int32)
    return {
        "iou exactly thr is kept (> not >=)": (f([[0, 0, 10, 10], [0, 0, 10, 5]]), z(2), 0.5, [1, 1]),
        "iou 2/3": (f([[0, 0, 10, 10], [0, 0, 10, 15]]), z(2), 0.5, [1, 0]),
        "chain: B suppressed, so C (overlapping only B) stays": (f([[0, 0, 10, 10], [0, 3, 10, 13], [0, 6, 10, 16]]), z(3), 0.5, [1, 0, 1]),
        "identical boxes: one survivor per group": (f([[2, 3, 9, 8]] * 5), torch.tensor([0, 0, 1, 1, 1], dtype=torch.int32), 0.5,
                                                    [1, 0, 1, 0, 0]),
        "zero-area boxes are kept (0 / 0 > thr is False)": (f([[0, 0, 10, 10], [5, 5, 5, 5], [5, 5, 5, 5], [3, 0, 3, 10], [0, 0, 10, 10]]),
                                                            z(5), 0.5, [1, 1, 1, 1, 0]),
    }


FPN_IMG_HW = (512.0, 768.0)


def fpn_shapes(nlevels, img_hw=FPN_IMG_HW):
    """[(H, W, scale)] of the pyramid levels 1/4 .. 1/32 of an image."""
    return [(int(img_hw[0]) >> (2 + l), int(img_hw[1]) >> (2 + l), 0.25 / (1 << l)) for l in range(nlevels)]


def roi_sample_margin(rois, shapes):
    """float64 distance of each RoI's 14 + 14 sample coordinates to the discontinuities of RoIAlign's sampling (a sample
    at y < -1 or y > H contributes 0, one just inside contributes the border row): [R] minimum over the samples."""
    lvl, _ = R64.fpn_level(rois, len(shapes))
    r = rois.double()
    Hs, Ws, sc = [torch.tensor([s[k] for s in shapes], dtype=torch.float64)[lvl] for k in range(3)]
    k = torch.arange(14, dtype=torch.float64)
    frac = (k // 2 + ((k % 2) + 0.5) / 2) / 7
    out = torch.full((rois.shape[0],), float("inf"), dtype=torch.float64)
    for lo, hi, size in ((r[:, 1], r[:, 3], Ws), (r[:, 2], r[:, 4], Hs)):
        c = (lo * sc)[:, None] + frac[None] * (hi * sc - lo * sc).clamp(min=1.0)[:, None]
        out = torch.minimum(out, torch.minimum((c + 1).abs(), (c - size[:, None]).abs()).amin(1))
    return out


def random_rois(R, nlevels, seed, img_hw=FPN_IMG_HW, n_images=2):
    """[R, 5] random RoIs (image, x1, y1, x2, y2) whose pyramid-level decision floor(4 + log2(sqrt(area) / 224) + 1e-6)
    stands at least 512 EPS (64 EPS relative to an argument below 8) from an integer in float64, and whose samples stand
    at least 1e-3 pixels from the inside / outside decision of the sampling; others are drawn again from the same
    generator.  Returns (rois, number still too close after 8 rounds)."""
    g = _gen(1000 + seed)
    Hh, Ww = img_hw
    shapes = fpn_shapes(nlevels, img_hw)

    def draw(n):
        c = torch.rand(n, 2, generator=g) * torch.tensor([Ww, Hh])
        wh = torch.exp(torch.rand(n, 2, generator=g) * 6.5 + 0.5)                   # sides 1.6 .. 1100
        img = torch.randint(0, n_images, (n, 1), generator=g).float()
        return torch.cat([img, c - wh / 2, c + wh / 2], 1)

    def bad_of(r):
        return (R64.fpn_level(r, nlevels)[1] <= 512 * EPS) | (roi_sample_margin(r, shapes) <= 1e-3)
    rois = draw(R)
    for _ in range(8):
        bad = bad_of(rois)
        if not bad.any():
            break
        rois[bad] = draw(int(bad.sum()))
    return rois, int(bad_of(rois).sum())


BOXPOST_IMG_HW = [[480.0, 640.0], [333.0, 500.5]]
BOXPOST_MIN_SIZE = 1e-2


def boxpost_inputs(R, NC, seed, thresh=0.05):
    """Inputs of the box head's post-processing, (logits [R, NC], deltas [R, NC, 4], props [R, 4], img [R], thresh, left).
    Rows cycle through four logit families: random; one dominant class (scores near 1 and near 1e-30); all equal (score
    1 / NC); random shifted by +-80.  Deltas: random, every 5th row at the log(1000 / 16) clamp, every 7th row pushed out
    of the image (boxes clip to zero width).  Both decisions of `valid` are kept away from their boundaries in float64:
    |score - thresh| > 64 EPS thresh and |side - min_size| > 64 EPS x 1024; rows that come closer are drawn again.
    `left` is the number of rows still too close after 8 rounds."""
    g = _gen(2000 + seed)
    thresh = min(thresh, 0.5 / NC) if NC > 8 else thresh
    hw = torch.tensor(BOXPOST_IMG_HW)
    img = (torch.arange(R) % 3 == 1).to(torch.int32)

    def draw(rows):
        n = rows.numel()
        fam = rows % 4
        l = 3 * torch.randn(n, NC, generator=g)
        dom = torch.zeros(n, NC)
        dom[torch.arange(n), (rows * 7 + 1) % NC] = 70.0
        l = torch.where((fam == 1)[:, None], dom, l)
        l = torch.where((fam == 2)[:, None], torch.full_like(l, 1.25), l)
        l = torch.where((fam == 3)[:, None], l + torch.where(rows % 8 == 3, 80.0, -80.0)[:, None], l)
        d = torch.randn(n, NC, 4, generator=g) * torch.tensor([2.0, 2.0, 1.5, 1.5])
        d[rows % 5 == 0, :, 2:] = 30.0
        d[rows % 7 == 3, :, 0] = 4000.0
        c = torch.rand(n, 2, generator=g) * hw[img[rows].long()].flip(-1)
        wh = 8 + 200 * torch.rand(n, 2, generator=g)
        return l, d, torch.cat([c - wh / 2, c + wh / 2], 1)

    def bad_rows(l, d, p):
        b, sc, _, _, _ = R64.box_postprocess(l, d, p, hw, img, thresh, BOXPOST_MIN_SIZE)
        side = torch.stack([b[..., 2] - b[..., 0], b[..., 3] - b[..., 1]], -1)
        return (((sc - thresh).abs() / thresh) <= 64 * EPS).any(1) | ((side - BOXPOST_MIN_SIZE).abs() <= 65536 * EPS).flatten(1).any(1)
    rows = torch.arange(R)
    logits, deltas, props = draw(rows)
    for _ in range(8):
        bad = bad_rows(logits, deltas, props)
        if not bad.any():
            break
        logits[bad], deltas[bad], props[bad] = draw(rows[bad])
    return logits, deltas, props, img, thresh, int(bad_rows(logits, deltas, props).sum())
