"""csrc/detect.hip without a GPU: the source file, compiled by the host C++ compiler against the stand-in header of tools/host_emu
(its ADH_HOST_EMU_STREAM section: the box head's 64-lane butterflies run on the emulator's __shfl_xor, the removed set of the NMS
scan is a heap block of exactly `words` uint64) with AddressSanitizer and UndefinedBehaviorSanitizer, run as a stand-alone
program on heap blocks of exactly their sizes (tests/_hostemu.py) and held to the float64 restatements and bounds of
tests/_ref64.py and the cases of tests/_cases.py, the ones tests/test_gpu_detect_kernels.py holds the library to.  Decisions (NMS
keep, valid, pyramid level) are exact.  Every call is made twice, on outputs of its own, and the two must agree bit for bit;
inputs come back unchanged."""
import os
import re

import numpy as np
import pytest
import torch

from tests import _cases as K
from tests import _hostemu as E
from tests import _ref64 as R64

ENTRY_POINTS = ["adh_upsample_nearest_add", "adh_rpn_decode", "adh_nms_words", "adh_nms_sorted", "adh_roi_align_fpn",
                "adh_box_postprocess"]                                           # the driver's call numbers
UPSAMPLE, RPN, NMS_WORDS, NMS, ROI_ALIGN, BOXPOST = range(6)
EPS = E.EPS
IPOISON = 0x5A5A5A5A     # Script.out's fill of an int32 output


def test_every_entry_point_is_called():
    src = open(os.path.join(E.ROOT, "adam-dehaze_amd", "csrc", "detect.hip")).read()
    assert sorted(re.findall(r'extern "C" int (adh_\w+)', src)) == sorted(ENTRY_POINTS)
    me = open(__file__).read()
    for name in ("UPSAMPLE", "RPN", "NMS_WORDS", "NMS", "ROI_ALIGN", "BOXPOST"):
        assert re.search(r"s\.call\(%s," % name, me), name


@pytest.fixture(scope="module")
def emus(tmp_path_factory):
    d = tmp_path_factory.mktemp("detect_emu")
    exe = E.build(d, "detect", "detect_main.cpp", sanitize=E.FLOAT_CAST)
    return lambda: E.Script(exe, d)


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _randn(*shape, seed=0):
    return torch.randn(shape, generator=_gen(seed))


def _twice(s, runs):
    for k1, k2 in zip(*runs):
        assert (s.after[k1] == s.after[k2]).all(), "two identical calls differ"
    return runs[0]


def _getf(s, k, what):
    t = s.get(k)
    E.assert_written(t, what)
    return t


def _geti(s, k):
    t = s.get(k, np.int32)
    assert not (t == IPOISON).any(), "an integer output was not written"
    return t


# ------------------------------------------------------------------------------------------------ FPN top-down add
@pytest.mark.parametrize("C_,pad_t,pad_l", [(8, 8, 4), (4, 4, 12)])
@pytest.mark.parametrize("top_hw,lat_hw", [((5, 7), (10, 14)), ((5, 7), (9, 13)), ((1, 1), (3, 5)), ((7, 5), (7, 5))])
def test_upsample_nearest_add(emus, top_hw, lat_hw, C_, pad_t, pad_l):
    """integer and non-integer scales; both tensors are channel slices (stride > C) whose padding holds NaN / poison: none may
    leak into the sum, and the lateral's padding must stay.  One fp32 add per element: the float64 sum rounded once."""
    s = emus()
    (th, tw), (Hh, Ww), N = top_hw, lat_hw, 2
    top, lat0 = _randn(N, th, tw, C_, seed=th * tw), _randn(N, Hh, Ww, C_, seed=Hh * Ww + 1)
    btop = s.sin(top.view(-1, C_), C_ + pad_t, 4)
    runs = []
    for _ in range(2):
        lat = s.sout(N * Hh * Ww, C_, C_ + pad_l, 8, init=lat0.view(-1, C_))
        s.call(UPSAMPLE, [C_ + pad_t, th, tw, C_ + pad_l, N, Hh, Ww, C_], [btop, lat])
        runs.append((lat,))
    assert s.run() == [0, 0]
    (lat,) = _twice(s, runs)
    ref = R64.upsample_nearest_add(top, lat0)
    assert torch.equal(s.get_slice(lat, N * Hh * Ww, C_).view(N, Hh, Ww, C_), ref.float()), "one fp32 add"


# ------------------------------------------------------------------------------------------------ RPN decode
def _base_anchors(A, seed):
    wh = torch.randint(8, 300, (A, 2), generator=_gen(seed)).float()
    return (torch.cat([-wh, wh], 1) / 2).round().contiguous()


@pytest.mark.parametrize("N,Hh,Ww,A,cpad,rpad,sh,sw", [(2, 5, 7, 1, 0, 0, 4, 4), (2, 5, 7, 3, 5, 4, 8, 16), (1, 9, 4, 15, 1, 4, 8, 16),
                                                       (2, 1, 1, 15, 0, 0, 64, 64), (1, 13, 21, 3, 1, 0, 4, 4)])
def test_rpn_decode(emus, N, Hh, Ww, A, cpad, rpad, sh, sw):
    """strides greater than A and 4 A; 13 x 21 x 3 = 819 anchors: four blocks, the last one partly idle.  Of every 8 positions
    one has zero deltas (the clipped anchor, exactly), one sits at the log(1000 / 16) clamp, two are pushed out of the image."""
    s = emus()
    ccs, rcs = A + cpad, 4 * A + rpad
    base = _base_anchors(A, A + sh)
    cls = _randn(N, Hh, Ww, A, seed=1)
    d = 0.5 * _randn(N, Hh * Ww, A, 4, seed=2)
    pos = torch.arange(Hh * Ww)
    d[:, pos % 8 == 1] = 0.0
    d[:, pos % 8 == 2, :, 2:] = 6.0
    d[:, pos % 8 == 3, :, :2] = 4000.0
    d[:, pos % 8 == 4, :, :2] = -4000.0
    img_h, img_w = Hh * sh - 2.5, Ww * sw * 0.75
    tot = Hh * Ww * A
    bcls, breg, bbase = s.sin(cls.view(-1, A), ccs, 3), s.sin(d.view(N * Hh * Ww, 4 * A), rcs, 5), s.vec(base)
    runs = []
    for _ in range(2):
        boxes, logits = s.out(N * tot * 4), s.out(N * tot)
        s.call(RPN, [ccs, rcs, N, Hh, Ww, A, sh, sw], [bcls, breg, bbase, boxes, logits], [img_h, img_w])
        runs.append((boxes, logits))
    assert s.run() == [0, 0]
    boxes, logits = _twice(s, runs)
    boxes = _getf(s, boxes, "boxes").view(N, tot, 4)
    assert torch.equal(s.get(logits).view(torch.int32), cls.reshape(-1).view(torch.int32)), "logits are copied"
    anchors = R64.rpn_anchors(Hh, Ww, base, sh, sw)                      # [tot, 4]
    ref, mag, pwh = R64.decode_clip(d.view(N, tot, 4), anchors[None], (1.0, 1.0, 1.0, 1.0), img_h, img_w)
    _, bound = R64.rpn_decode_bounds(mag, pwh)
    E.assert_bound(boxes, ref, bound, "rpn boxes")
    zero = (pos % 8 == 1).repeat_interleave(A)
    clipped = torch.stack([anchors[:, 0].clamp(0, img_w), anchors[:, 1].clamp(0, img_h), anchors[:, 2].clamp(0, img_w),
                           anchors[:, 3].clamp(0, img_h)], -1).float()
    assert torch.equal(boxes[:, zero], clipped[zero][None].expand(N, -1, -1)), "zero deltas: the clipped anchor, exactly"
    out = (pos % 8 == 3).repeat_interleave(A)
    assert (boxes[:, out][..., 0] == np.float32(img_w)).all() and (boxes[:, out][..., 2] == np.float32(img_w)).all()
    assert (boxes[:, (pos % 8 == 4).repeat_interleave(A)] == 0).all()


# ------------------------------------------------------------------------------------------------ NMS
def _nms_calls(s, boxes, groups, thr):
    M = boxes.shape[0]
    words = (M + 63) // 64
    bb, bg = s.vec(boxes), s.vec(groups, np.int32)
    c_n = s.call(NMS_WORDS, [M])
    runs = []
    for _ in range(2):
        mask, keep = s.out(M * words, np.uint64), s.out(M, np.int32)
        s.call(NMS, [M], [bb, bg, mask, keep], [thr])
        runs.append((keep, mask))
    return c_n, words, runs


def _nms_keep(s, rcs, c_n, words, runs):
    assert rcs[c_n:c_n + 3] == [words, 0, 0], rcs
    keep, _ = _twice(s, runs)
    keep = _geti(s, keep).numpy()
    assert ((keep == 0) | (keep == 1)).all(), "every keep entry must become 0 or 1"
    return keep


@pytest.mark.parametrize("M", [1, 63, 64, 65, 130])
def test_nms_sorted_integer_boxes(emus, M):
    """one word short of full, full, one box into a second word, a third word with two boxes; one and two groups; every 11th
    box a copy of its predecessor; with and without zero-area boxes (0 / 0 = NaN > thr is False).  Integer coordinates: keep is
    exact.  The mask workspace is exactly M x words uint64 and the removed set exactly `words`."""
    s = emus()
    todo = []
    for ngroups in (1, 2):
        for zero_area in (False, True):
            boxes, groups = K.int_boxes(M, seed=M + ngroups, ngroups=ngroups, zero_area=zero_area)
            for thr in (0.5, 0.7):
                todo.append((boxes, groups, thr) + _nms_calls(s, boxes, groups, thr))
    rcs = s.run()
    for boxes, groups, thr, c_n, words, runs in todo:
        keep = _nms_keep(s, rcs, c_n, words, runs)
        ref = R64.nms_sorted(boxes.numpy(), groups.numpy(), thr)
        assert np.array_equal(keep, ref), f"thr={thr}: {int((keep != ref).sum())} of {M} decisions differ"
        if M >= 128:
            assert 0 < ref.sum() < M


def test_nms_sorted_hand_cases(emus):
    s = emus()
    todo = [(name, expect) + _nms_calls(s, boxes, groups, thr) for name, (boxes, groups, thr, expect) in K.nms_hand_cases().items()]
    rcs = s.run()
    for name, expect, c_n, words, runs in todo:
        assert _nms_keep(s, rcs, c_n, words, runs).tolist() == expect, name


# ------------------------------------------------------------------------------------------------ RoIAlign over the pyramid
def _hand_rois():
    rows = [[0, 100.0, 80.0, 100.0 + d, 80.0 + d] for d in (56.0, 112.0, 224.0, 448.0, 896.0)]      # the level boundaries
    rows += [[1, 3000.0, 3000.0, 3100.0, 3100.0], [0, -900.0, -900.0, -700.0, -800.0],                # fully outside: exactly 0
             [1, -40.0, -30.0, 60.0, 90.0], [0, 700.0, 450.0, 800.0, 540.0],                         # crossing two borders each
             [1, 200.0, 200.0, 201.0, 200.5], [0, 300.25, 100.5, 300.75, 140.0],                     # under one pixel: max(., 1)
             [1, 50.0, 60.0, 50.0, 60.0], [0, 10.0, 20.0, 10.0, 300.0],                              # zero area: level 0
             [0, 0.0, 0.0, 120.0, 90.0], [1, 648.0, 402.0, 768.0, 512.0],                            # touching two borders each
             [0, 300.0, -20.0, 420.0, 70.0], [1, -25.0, 200.0, 80.0, 330.0],                         # crossing the top; the left
             [0, 350.0, 430.0, 460.0, 530.0], [1, 690.0, 150.0, 790.0, 260.0]]                       # the bottom; the right
    return torch.tensor(rows)


@pytest.mark.parametrize("nlevels,C_,pad", [(4, 8, 4), (2, 4, 8), (1, 12, 4), (3, 4, 4)])
def test_roi_align_fpn(emus, nlevels, C_, pad):
    """a 512 x 768 image's pyramid at cs > C; RoIs on the level boundaries, outside the image, touching and crossing each of its
    four borders, under one pixel and of zero size, and random ones that stand a checked margin from every decision
    (tests/_cases.py).  Every level ends at the last used channel of its last pixel.  The program is built with
    -fsanitize=float-cast-overflow on top (g++'s `undefined` leaves it out): the two RoIs of zero size, whose level argument is
    log2f(0) = -inf, found the kernel converting -inf to int before it clamped the level; it now clamps in float first."""
    s = emus()
    N, cs = 2, C_ + pad
    shapes = K.fpn_shapes(nlevels)
    feats = [_randn(N, Hh, Ww, C_, seed=10 * l + C_) for l, (Hh, Ww, _) in enumerate(shapes)]
    rand_rois, left = K.random_rois(24, nlevels, seed=nlevels)
    assert left == 0, "the margin rule left RoIs out"
    rois = torch.cat([_hand_rois(), rand_rois])
    margin = K.roi_sample_margin(rois[13:19], shapes)
    assert float(margin.min()) >= 1e-3, "a hand-made border RoI has a sample too close to the inside / outside decision"
    R = rois.shape[0]
    bf = [s.sin(f.view(-1, C_), cs, 4 * (l + 1)) for l, f in enumerate(feats)]
    brois = s.vec(rois)
    ints = [nlevels, R, C_] + [v for Hh, Ww, _ in shapes for v in (Hh, Ww, cs)]
    runs = []
    for _ in range(2):
        out = s.out(R * C_ * 49)
        s.call(ROI_ALIGN, ints, [brois, out] + bf, [sc for _, _, sc in shapes])
        runs.append((out,))
    assert s.run() == [0, 0]
    (out,) = _twice(s, runs)
    out = _getf(s, out, "roi_align").view(R, C_ * 49)
    lvl, _ = R64.fpn_level(rois, nlevels)
    assert lvl[:5].tolist() == [min(l, nlevels - 1) for l in (0, 1, 2, 3, 3)] and lvl[11:13].tolist() == [0, 0]
    ref = torch.zeros(R, C_, 7, 7, dtype=torch.float64)
    bound = torch.zeros_like(ref)
    for l, (Hh, Ww, sc) in enumerate(shapes):
        idx = torch.where(lvl == l)[0]
        if idx.numel() == 0:
            continue
        v, mag = R64.roi_align(feats[l], rois[idx], sc)
        ref[idx] = v
        bound[idx] = R64.roi_align_bound(rois[idx], mag, sc, feats[l].abs().max().double())
    E.assert_bound(out, ref.flatten(1), bound.flatten(1), f"roi_align nlevels={nlevels} C={C_}")
    assert (out[5:7] == 0).all(), "RoIs fully outside the feature map pool to exactly 0"
    assert float(out[7:9].abs().max()) > 0 and float(out[13:19].abs().max()) > 0


# ------------------------------------------------------------------------------------------------ box head post-processing
@pytest.mark.parametrize("R", [1, 3, 140])
@pytest.mark.parametrize("NC", K.BOXPOST_NC)
def test_box_postprocess(emus, NC, R):
    """tests/_cases.py's rows (four logit families, clamped and pushed-out deltas, both `valid` decisions a margin from their
    boundaries) at strides NC + 3 and 4 NC + 5; R = 140 holds every combination of the families' periods 4, 5 and 7.  NC = 65
    and 129 put one class into a second / third trip of the 64-lane class loop; NC = 2 leaves 63 lanes idle."""
    s = emus()
    logits, deltas, props, img, thresh, left = K.boxpost_inputs(R, NC, seed=NC)
    assert left == 0, "the margin rule left rows out"
    hw = torch.tensor(K.BOXPOST_IMG_HW)
    n = R * (NC - 1)
    bufs = [s.sin(logits, NC + 3, 2), s.sin(deltas.view(R, 4 * NC), 4 * NC + 5, 3), s.vec(props), s.vec(hw), s.vec(img, np.int32)]
    runs = []
    for _ in range(2):
        boxes, scores, valid = s.out(n * 4), s.out(n), s.out(n, np.int32)
        s.call(BOXPOST, [NC + 3, 4 * NC + 5, R, NC], bufs + [boxes, scores, valid], [thresh, K.BOXPOST_MIN_SIZE])
        runs.append((boxes, scores, valid))
    assert s.run() == [0, 0]
    boxes, scores, valid = _twice(s, runs)
    boxes, scores = _getf(s, boxes, "boxes").view(R, NC - 1, 4), _getf(s, scores, "scores").view(R, NC - 1)
    valid = _geti(s, valid).view(R, NC - 1)
    rb, rs, rv, mag, pwh = R64.box_postprocess(logits, deltas, props, hw, img, thresh, K.BOXPOST_MIN_SIZE)
    _, e_s, _, e_b = R64.box_postprocess_bounds(logits, rs, mag, pwh)
    E.assert_bound(scores, rs, e_s, f"scores NC={NC}")
    E.assert_bound(boxes, rb, e_b, f"boxes NC={NC}")
    assert ((valid == 0) | (valid == 1)).all()
    assert torch.equal(valid.bool(), rv), f"{int((valid.bool() != rv).sum())} valid flags differ"
    eq = torch.arange(R) % 4 == 2
    if NC in (2, 64) and bool(eq.any()):
        assert (scores[eq] == 1.0 / NC).all(), "equal logits, NC a power of two: exactly 1 / NC"
    if R >= 8:
        assert not valid[torch.arange(R) % 7 == 3].any(), "boxes clipped to zero width are not valid"
        assert bool(valid.any())


# ------------------------------------------------------------------------------------------------ rejections
def test_argument_rejections_write_nothing(emus):
    s = emus()
    bv, bi = s.vec(torch.rand(256)), s.vec(torch.zeros(64), np.int32)
    of, oi, om = s.out(256), s.out(64, np.int32), s.out(64, np.uint64)
    lat = s.sout(16, 8)
    up = lambda C_=4, tcs=8, lcs=8, th=2: s.call(UPSAMPLE, [tcs, th, 2, lcs, 1, 4, 4, C_], [bv, lat])
    rpn = lambda A=3, ccs=3, rcs=12, N=1: s.call(RPN, [ccs, rcs, N, 2, 2, A, 4, 4], [bv, bv, bv, of, of], [8.0, 8.0])
    roi = lambda ints, b=(bv, of, bv, bv): s.call(ROI_ALIGN, ints, list(b), [0.25, 0.125])
    post = lambda R=2, NC=5, lcs=5, dcs=20: s.call(BOXPOST, [lcs, dcs, R, NC], [bv, bv, bv, bv, bi, of, of, oi], [0.05, 1e-2])
    bad = [up(C_=6), up(tcs=6), up(lcs=7), up(C_=0), up(th=0),
           rpn(ccs=2), rpn(rcs=11), rpn(A=0), rpn(N=0),
           s.call(NMS, [0], [bv, bi, om, oi], [0.5]), s.call(NMS, [16385], [bv, bi, om, oi], [0.5]), s.call(NMS, [-1], [bv, bi, om, oi], [0.5]),
           s.call(NMS, [8], [bv, bi, None, oi], [0.5]),
           roi([2, 3, 6, 4, 4, 8, 2, 2, 8]), roi([2, 0, 8, 4, 4, 8, 2, 2, 8]), roi([5, 3, 8, 4, 4, 8, 2, 2, 8]), roi([0, 3, 8, 4, 4, 8, 2, 2, 8]),
           roi([2, 3, 8, 4, 4, 8, 2, 2, 4]), roi([2, 3, 8, 4, 4, 8, 2, 2, 10]), roi([2, 3, 8, 4, 4, 8, 0, 2, 8]), roi([-1, 3, 8]),
           roi([2, 3, 8, 4, 4, 8, 2, 2, 8], (bv, of, bv)),
           post(R=0), post(NC=1), post(lcs=4), post(dcs=19)]
    rcs = s.run()
    assert [rcs[i] for i in bad] == [E.ADH_E_ARG] * len(bad), rcs
    for b in (of, oi, om, lat):
        assert s.unchanged(b), "a rejected call wrote to an output"
