"""The detector-stage kernels of csrc/detect.hip through the C ABI, each entry point against a float64 restatement of the
torchvision operation it implements (tests/_ref64.py): FPN nearest-upsample-add, RPN anchor decode, grouped NMS,
multi-level RoIAlign and the box head's post-processing.  The detector tests see these only behind the convolutions, on
96 x 128 inputs and with the network's tolerances; here they run alone, past their grid caps, at the 64-box word
boundaries of the NMS mask, at the pyramid-level boundaries and with more classes than one wave has lanes.

Outputs are prefilled with NaN (int outputs and workspaces with -7) inside guard bands that must stay untouched; every
entry point runs twice and must reproduce itself bit for bit.  Decisions (NMS keep, valid, pyramid level) are compared
exactly, on inputs whose decision is exact in fp32 (integer boxes) or stands a checked margin from its boundary
(tests/_cases.py, asserted without a GPU in tests/test_ref64_cpu.py).  Value tolerances are in EPS = 2^-24 relative to the
sum of |terms| added, each with the fp32 operations it counts."""
import ctypes as C

import numpy as np
import pytest
import torch

from adam_dehaze_amd import _hip as H
from tests import _cases as K
from tests import _ref64 as R64
from tests._util import DEV, EPS, _assert_bound, _idx, _nan, _pad_untouched, _padded, _same_bits, _twice

pytestmark = pytest.mark.gpu
# (the bounds, and EXP_UNITS for expf, are tests/_ref64.py's: the host-emulation run of csrc/detect.hip shares them)


def _gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def _randn(*shape, seed=0):
    return torch.randn(shape, device=DEV, dtype=torch.float32, generator=_gen(seed))


def _rejected(name, *args):
    with pytest.raises(RuntimeError):
        H.call(name, *args)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ FPN top-down add
UPS = [((5, 7), (10, 14)), ((5, 7), (9, 13)), ((1, 1), (3, 5)), ((7, 5), (7, 5)), ((13, 21), (25, 42)), ((64, 128), (128, 256))]


@pytest.mark.parametrize("C_,pad_t,pad_l", [(256, 0, 0), (256, 8, 4), (4, 4, 12)])
@pytest.mark.parametrize("top_hw,lat_hw", UPS)
def test_upsample_nearest_add(top_hw, lat_hw, C_, pad_t, pad_l):
    """(64, 128) -> (128, 256) with 256 channels is 2 M channel quads, twice the 4096-block cap.  The channel padding of
    both tensors holds NaN: none may leak into the sum and the lateral's padding must still be NaN.  One fp32 add per
    element: exact against the float64 sum rounded once."""
    (th, tw), (Hh, Ww) = top_hw, lat_hw
    N = 1 if Hh * Ww > 10000 else 2
    tcs, lcs = C_ + pad_t, C_ + pad_l
    top = _nan(N, th, tw, tcs)
    top[..., :C_] = _randn(N, th, tw, C_, seed=th * tw)
    lat0 = _nan(N, Hh, Ww, lcs)
    lat0[..., :C_] = _randn(N, Hh, Ww, C_, seed=Hh * Ww + 1)

    def run():
        whole, lat = _padded(lat0.numel())
        lat.copy_(lat0.view(-1))
        H.call("adh_upsample_nearest_add", top.data_ptr(), tcs, th, tw, lat.data_ptr(), lcs, N, Hh, Ww, C_)
        torch.cuda.synchronize()
        assert _pad_untouched(whole, lat0.numel())
        return (lat.view(N, Hh, Ww, lcs),)
    lat, = _twice(run)
    ref = R64.upsample_nearest_add(top[..., :C_], lat0[..., :C_])
    assert not torch.isnan(lat[..., :C_]).any(), "NaN leaked from the channel padding (or an element was skipped)"
    assert torch.equal(lat[..., :C_], ref.float()), "one fp32 add: must equal the float64 sum rounded once"
    assert torch.isnan(lat[..., C_:]).all(), "the lateral's channel padding was written"


def test_upsample_nearest_add_rejects():
    top, lat = _randn(1, 2, 2, 8), _nan(1, 4, 4, 8)
    for C_, tcs, lcs in ((6, 8, 8), (4, 6, 8), (4, 8, 7), (0, 8, 8)):
        _rejected("adh_upsample_nearest_add", top.data_ptr(), tcs, 2, 2, lat.data_ptr(), lcs, 1, 4, 4, C_)
    _rejected("adh_upsample_nearest_add", top.data_ptr(), 8, 0, 2, lat.data_ptr(), 8, 1, 4, 4, 4)
    assert torch.isnan(lat).all()


# ------------------------------------------------------------------------------------------------ RPN decode
def _base_anchors(A, seed):
    g = torch.Generator().manual_seed(seed)
    wh = torch.randint(8, 300, (A, 2), generator=g).float()
    return (torch.cat([-wh, wh], 1) / 2).round().to(DEV).contiguous()


RPN_CASES = [  # N, H, W, A, cls pad, reg pad, stride_h, stride_w
    (2, 5, 7, 1, 0, 0, 4, 4), (2, 5, 7, 3, 0, 0, 64, 64), (2, 5, 7, 3, 5, 4, 8, 16), (1, 9, 4, 15, 1, 4, 8, 16), (2, 1, 1, 15, 0, 0, 64, 64),
    (1, 37, 53, 3, 1, 0, 4, 4), (4, 256, 512, 3, 1, 4, 4, 4)]


@pytest.mark.parametrize("N,Hh,Ww,A,cpad,rpad,sh,sw", RPN_CASES)
def test_rpn_decode(N, Hh, Ww, A, cpad, rpad, sh, sw):
    """(4, 256, 512) with A = 3 is 1.5 M anchors, past the 4096-block cap.  Of every 8 positions one has zero deltas
    (output = clipped anchor, exact), one sits at the log(1000 / 16) clamp, one is pushed fully outside the image (all
    four coordinates clip).  Anchor order: position major, anchor minor."""
    ccs, rcs = A + cpad, 4 * A + rpad
    base = _base_anchors(A, A + sh)
    cls = _nan(N, Hh, Ww, ccs)
    cls[..., :A] = _randn(N, Hh, Ww, A, seed=1)
    reg = _nan(N, Hh, Ww, rcs)
    d = 0.5 * _randn(N, Hh * Ww, A, 4, seed=2)
    pos = torch.arange(Hh * Ww, device=DEV)
    d[:, pos % 8 == 1] = 0.0
    d[:, pos % 8 == 2, :, 2:] = 6.0
    d[:, pos % 8 == 3, :, :2] = 4000.0
    d[:, pos % 8 == 4, :, :2] = -4000.0
    reg[..., :4 * A] = d.view(N, Hh, Ww, 4 * A)
    img_h, img_w = Hh * sh - 2.5, Ww * sw * 0.75
    tot = Hh * Ww * A

    def run():
        wb, boxes = _padded(N * tot * 4)
        wl, logits = _padded(N * tot)
        H.call("adh_rpn_decode", cls.data_ptr(), ccs, reg.data_ptr(), rcs, N, Hh, Ww, A, sh, sw, base.data_ptr(), img_h, img_w,
               boxes.data_ptr(), logits.data_ptr())
        torch.cuda.synchronize()
        assert _pad_untouched(wb, N * tot * 4) and _pad_untouched(wl, N * tot)
        return boxes.view(N, tot, 4), logits.view(N, tot)
    boxes, logits = _twice(run)
    assert _same_bits(logits, cls[..., :A].reshape(N, tot)), "logits are copied"
    anchors = R64.rpn_anchors(Hh, Ww, base, sh, sw)                      # [tot, 4]
    ref, mag, pwh = R64.decode_clip(d.view(N, tot, 4), anchors[None], (1.0, 1.0, 1.0, 1.0), img_h, img_w)
    plain, bound = R64.rpn_decode_bounds(mag, pwh)
    _assert_bound(boxes, ref, bound, "rpn boxes")
    need = (((boxes.double() - ref).abs() - plain) / (EPS * 0.5 * pwh)).max()
    print(f"[measure] rpn_decode: expf units needed beyond the plain roundings: {float(need):.2f}")
    zero = (pos % 8 == 1).repeat_interleave(A)
    clipped = torch.stack([anchors[:, 0].clamp(0, img_w), anchors[:, 1].clamp(0, img_h), anchors[:, 2].clamp(0, img_w),
                           anchors[:, 3].clamp(0, img_h)], -1).float()
    assert torch.equal(boxes[:, zero], clipped[zero][None].expand(N, -1, -1)), "zero deltas: the clipped anchor, exactly"
    out = (pos % 8 == 3).repeat_interleave(A)
    assert (boxes[:, out][..., 0] == np.float32(img_w)).all() and (boxes[:, out][..., 2] == np.float32(img_w)).all()
    out = (pos % 8 == 4).repeat_interleave(A)
    assert (boxes[:, out] == 0).all()


def test_rpn_decode_rejects():
    cls, reg, base = _randn(1, 2, 2, 3), _randn(1, 2, 2, 12), _base_anchors(3, 0)
    boxes, logits = _nan(12, 4), _nan(12)
    for A, ccs, rcs, N in ((3, 2, 12, 1), (3, 3, 11, 1), (0, 3, 12, 1), (3, 3, 12, 0)):
        _rejected("adh_rpn_decode", cls.data_ptr(), ccs, reg.data_ptr(), rcs, N, 2, 2, A, 4, 4, base.data_ptr(), 8.0, 8.0,
                  boxes.data_ptr(), logits.data_ptr())
    assert torch.isnan(boxes).all() and torch.isnan(logits).all()


# ------------------------------------------------------------------------------------------------ NMS
def _run_nms(boxes, groups, thr):
    M = boxes.shape[0]
    words = H.value("adh_nms_words", M)
    assert words == (M + 63) // 64
    b, g = boxes.to(DEV).contiguous(), groups.to(DEV).contiguous()

    def run():
        wm, mask = _padded(M * words, dtype=torch.int64, fill=-7)
        wk, keep = _padded(M, dtype=torch.int32, fill=-7)
        H.call("adh_nms_sorted", b.data_ptr(), g.data_ptr(), M, thr, mask.data_ptr(), keep.data_ptr())
        torch.cuda.synchronize()
        assert _pad_untouched(wm, M * words) and _pad_untouched(wk, M)
        return (keep,)
    keep, = _twice(run)
    assert ((keep == 0) | (keep == 1)).all(), "every keep entry must become 0 or 1"
    return keep.cpu().numpy()


@pytest.mark.parametrize("ngroups", [1, 2, 7])
@pytest.mark.parametrize("M", [1, 2, 63, 64, 65, 128, 129, 1000, 16384])
def test_nms_sorted_integer_boxes(M, ngroups):
    """Integer coordinates below 2^11: every IoU comparison is the same decision in fp32 and float64, so keep is compared
    exactly.  With and without zero-area boxes (0 / 0 = NaN > thr is False: kept, and they suppress nothing)."""
    for zero_area in (False, True):
        boxes, groups = K.int_boxes(M, seed=M + ngroups, ngroups=ngroups, zero_area=zero_area)
        for thr in (0.5, 0.7):
            keep = _run_nms(boxes, groups, thr)
            ref = R64.nms_sorted(boxes.numpy(), groups.numpy(), thr)
            assert np.array_equal(keep, ref), f"zero_area={zero_area} thr={thr}: {int((keep != ref).sum())} of {M} decisions differ"
            if M >= 128:
                assert 0 < ref.sum() < M


def test_nms_sorted_hand_cases():
    for name, (boxes, groups, thr, expect) in K.nms_hand_cases().items():
        assert _run_nms(boxes, groups, thr).tolist() == expect, name


def test_nms_sorted_across_words_and_row_blocks():
    """16384 pairwise disjoint boxes, then: a victim 200 words after its suppressor; the very last box (last bit of the
    last word) a copy of one 155 words earlier; a chain A > B > C spread over three words and row blocks, where B is
    suppressed and C overlaps only B; a copy in another group (kept)."""
    M = 16384
    i = torch.arange(M)
    xy = torch.stack([3 * (i % 128), 3 * (i // 128)], 1).float()
    boxes = torch.cat([xy, xy + 2], 1)
    groups = torch.zeros(M, dtype=torch.int32)
    expect = np.ones(M, dtype=np.int32)
    boxes[64 * 200 + 5] = boxes[3]
    boxes[M - 1] = boxes[64 * 100 + 1]
    expect[[64 * 200 + 5, M - 1]] = 0
    boxes[10] = torch.tensor([1000.0, 1000, 1010, 1010])
    boxes[64 * 3 + 7] = torch.tensor([1000.0, 1003, 1010, 1013])
    boxes[64 * 9 + 1] = torch.tensor([1000.0, 1006, 1010, 1016])
    expect[64 * 3 + 7] = 0
    boxes[64 * 50] = boxes[20]
    groups[64 * 50] = 1
    keep = _run_nms(boxes, groups, 0.5)
    assert np.array_equal(keep, expect), np.nonzero(keep != expect)[0][:10]
    assert np.array_equal(R64.nms_sorted(boxes.numpy(), groups.numpy(), 0.5), expect)
    # M = 1000: the last word holds 40 boxes; suppressor and victim both inside it, and a victim in it from word 0
    M = 1000
    b2, g2 = boxes[:M].clone(), torch.zeros(M, dtype=torch.int32)
    b2[10], b2[64 * 3 + 7], b2[64 * 9 + 1] = boxes[2000], boxes[2001], boxes[2002]       # disjoint again
    b2[999], b2[990] = b2[970], b2[0]
    exp2 = np.ones(M, dtype=np.int32)
    exp2[[999, 990]] = 0
    assert np.array_equal(_run_nms(b2, g2, 0.5), exp2)


def test_nms_sorted_rejects():
    boxes, groups = K.int_boxes(64, 0)
    b, g = boxes.to(DEV), groups.to(DEV)
    mask, keep = torch.full((64,), -7, device=DEV, dtype=torch.int64), _idx(64)
    for M in (0, 16385, -1):
        _rejected("adh_nms_sorted", b.data_ptr(), g.data_ptr(), M, 0.5, mask.data_ptr(), keep.data_ptr())
    _rejected("adh_nms_sorted", b.data_ptr(), g.data_ptr(), 64, 0.5, None, keep.data_ptr())
    assert (keep == -7).all() and (mask == -7).all()


@pytest.mark.parametrize("limit,M", [(256, 1000), (4096, 10000)])
@pytest.mark.parametrize("zero_area", [False, True])
def test_nms_chunked_path_matches_greedy(monkeypatch, zero_area, limit, M):
    """FasterRCNN.nms with more boxes than one launch takes (NMS_LIMIT lowered): group 0 holds 70 % of the boxes and goes
    through in three score-ordered chunks; with 4096-box chunks the IoU against the kept boxes runs in two row blocks.
    Zero-area boxes have IoU 0 / 0 with each other: they are kept by the kernel and by torchvision, so the chunked path
    must keep them too."""
    from adam_dehaze_amd.detection import FasterRCNN
    monkeypatch.setattr(FasterRCNN, "NMS_LIMIT", limit)
    boxes, groups = K.int_boxes(M, seed=77, ngroups=4, zero_area=zero_area, span=200 if M <= 1000 else 1200)
    groups[torch.arange(M) % 10 < 7] = 0
    if zero_area:
        z = torch.arange(5, M, 50)                      # identical zero-area boxes of group 0 in every chunk
        boxes[z] = torch.tensor([30.0, 30, 30, 30])
        groups[z] = 0
    scores = torch.randperm(M, generator=torch.Generator().manual_seed(5)).float() / M      # distinct: no ties in the order
    order = torch.sort(scores, descending=True, stable=True).indices
    ref = order[torch.from_numpy(R64.nms_sorted(boxes[order].numpy(), groups[order].numpy(), 0.5)).bool()]
    got = FasterRCNN.nms(boxes.to(DEV), scores.to(DEV), groups.to(DEV), 0.5).cpu()
    assert torch.equal(got, ref), f"kept {got.numel()} boxes, greedy NMS keeps {ref.numel()}"
    assert ref.numel() > limit, "the kept boxes of the earlier chunks must themselves exceed one row block / chunk"


# ------------------------------------------------------------------------------------------------ RoIAlign over the pyramid
def _levels(shapes, feats, cs):
    L = H.FpnLevels()
    L.nlevels = len(shapes)
    for i, ((Hh, Ww, sc), f) in enumerate(zip(shapes, feats)):
        L.f[i], L.H[i], L.W[i], L.cs[i], L.scale[i] = f.data_ptr(), Hh, Ww, cs, sc
    return L


def _hand_rois():
    rows = [[0, 100.0, 80.0, 100.0 + s, 80.0 + s] for s in (56.0, 112.0, 224.0, 448.0, 896.0)]      # the level boundaries
    rows += [[1, 3000.0, 3000.0, 3100.0, 3100.0], [0, -900.0, -900.0, -700.0, -800.0],                # fully outside: exactly 0
             [1, -40.0, -30.0, 60.0, 90.0], [0, 700.0, 450.0, 800.0, 540.0],                         # straddling the border
             [1, 200.0, 200.0, 201.0, 200.5], [0, 300.25, 100.5, 300.75, 140.0],                     # under one pixel: max(., 1)
             [1, 50.0, 60.0, 50.0, 60.0], [0, 10.0, 20.0, 10.0, 300.0]]                              # zero area: level 0
    return torch.tensor(rows)


@pytest.mark.parametrize("C_,pad", [(4, 0), (8, 4), (256, 8)])
@pytest.mark.parametrize("nlevels", [1, 2, 3, 4])
def test_roi_align_fpn(nlevels, C_, pad):
    N, cs = 2, C_ + pad
    shapes = K.fpn_shapes(nlevels)
    feats = []
    for l, (Hh, Ww, _) in enumerate(shapes):
        f = _nan(N, Hh, Ww, cs)
        f[..., :C_] = _randn(N, Hh, Ww, C_, seed=10 * l + C_)
        feats.append(f)
    rand_rois, left = K.random_rois(64, nlevels, seed=nlevels)
    assert left == 0, "the margin rule left RoIs out"
    rois_cpu = torch.cat([_hand_rois(), rand_rois])
    rois = rois_cpu.to(DEV).contiguous()
    R = rois.shape[0]
    L = _levels(shapes, feats, cs)

    def run():
        whole, out = _padded(R * C_ * 49)
        H.call("adh_roi_align_fpn", C.byref(L), rois.data_ptr(), R, C_, out.data_ptr())
        torch.cuda.synchronize()
        assert _pad_untouched(whole, R * C_ * 49)
        return (out.view(R, C_ * 49),)
    out, = _twice(run)
    lvl, margin = R64.fpn_level(rois_cpu, nlevels)
    assert lvl[:5].tolist() == [min(l, nlevels - 1) for l in (0, 1, 2, 3, 3)] and lvl[-2 - 64:-64].tolist() == [0, 0]
    ref = torch.zeros(R, C_, 7, 7, dtype=torch.float64, device=DEV)
    bound = torch.zeros_like(ref)
    for l, (Hh, Ww, sc) in enumerate(shapes):
        idx = torch.where(lvl == l)[0].to(DEV)
        if idx.numel() == 0:
            continue
        r = rois[idx]
        v, mag = R64.roi_align(feats[l][..., :C_], r, sc)
        ref[idx] = v
        bound[idx] = R64.roi_align_bound(r, mag, sc, feats[l][..., :C_].abs().max().double())
    _assert_bound(out, ref.flatten(1), bound.flatten(1), f"roi_align nlevels={nlevels} C={C_}")
    assert (out[5:7] == 0).all(), "RoIs fully outside the feature map pool to exactly 0"
    assert float(out[7:9].abs().max()) > 0


def test_roi_align_fpn_one_pixel_levels_and_rejects():
    """Levels one row high and one column wide: every sample clamps onto that row / column."""
    C_, cs, N = 8, 12, 2
    shapes = [(1, 24, 0.25), (12, 1, 0.125)]
    feats = [_nan(N, Hh, Ww, cs) for Hh, Ww, _ in shapes]
    for l, f in enumerate(feats):
        f[..., :C_] = _randn(*f.shape[:3], C_, seed=l)
    rois_cpu = torch.tensor([[0, 4.0, 0.0, 60.0, 3.5], [1, 10.0, -2.0, 90.0, 3.0], [0, 0.0, 0.0, 6.0, 90.0], [1, 1.0, 8.0, 300.0, 250.0],
                             [1, 0.0, 0.0, 112.0, 112.0]])
    rois = rois_cpu.to(DEV)
    L = _levels(shapes, feats, cs)
    R = rois.shape[0]
    out = _nan(R, C_ * 49)
    H.call("adh_roi_align_fpn", C.byref(L), rois.data_ptr(), R, C_, out.data_ptr())
    torch.cuda.synchronize()
    lvl, _ = R64.fpn_level(rois_cpu, 2)
    assert lvl.tolist() == [0, 0, 0, 1, 1]
    for l, (Hh, Ww, sc) in enumerate(shapes):
        idx = torch.where(lvl == l)[0].to(DEV)
        v, mag = R64.roi_align(feats[l][..., :C_], rois[idx], sc)
        vmax = float(feats[l][..., :C_].abs().max())
        _assert_bound(out[idx], v.flatten(1), (12 * EPS * mag + 6 * EPS * 80 * 4 * vmax).flatten(1), f"one-pixel level {l}")
    out2 = _nan(R, C_ * 49)
    for Cbad, Rbad in ((6, R), (2, R), (8, 0)):
        _rejected("adh_roi_align_fpn", C.byref(L), rois.data_ptr(), Rbad, Cbad, out2.data_ptr())
    L.nlevels = 5
    _rejected("adh_roi_align_fpn", C.byref(L), rois.data_ptr(), R, C_, out2.data_ptr())
    L.nlevels = 2
    L.cs[1] = 4
    _rejected("adh_roi_align_fpn", C.byref(L), rois.data_ptr(), R, C_, out2.data_ptr())
    assert torch.isnan(out2).all()


# ------------------------------------------------------------------------------------------------ box head post-processing
@pytest.mark.parametrize("R", [1, 3, 1000])
@pytest.mark.parametrize("NC", K.BOXPOST_NC)
def test_box_postprocess(NC, R):
    """Every (RoI, class) pair's score, box and valid flag, not only the detections that survive.  NC = 65 and 129 put one
    class into a second / third trip of the 64-lane class loop; NC = 2 leaves 63 lanes idle."""
    logits_c, deltas_c, props_c, img_c, thresh, left = K.boxpost_inputs(R, NC, seed=NC)
    assert left == 0, "the margin rule left rows out"
    l_cs, d_cs = NC + 3, 4 * NC + 5
    logits = _nan(R, l_cs)
    logits[:, :NC] = logits_c.to(DEV)
    deltas = _nan(R, d_cs)
    deltas[:, :4 * NC] = deltas_c.view(R, 4 * NC).to(DEV)
    props, img = props_c.to(DEV).contiguous(), img_c.to(DEV).contiguous()
    hw = torch.tensor(K.BOXPOST_IMG_HW, device=DEV)
    n = R * (NC - 1)

    def run():
        wb, boxes = _padded(n * 4)
        ws, scores = _padded(n)
        wv, valid = _padded(n, dtype=torch.int32, fill=-7)
        H.call("adh_box_postprocess", logits.data_ptr(), l_cs, deltas.data_ptr(), d_cs, props.data_ptr(), hw.data_ptr(), img.data_ptr(),
               R, NC, thresh, K.BOXPOST_MIN_SIZE, boxes.data_ptr(), scores.data_ptr(), valid.data_ptr())
        torch.cuda.synchronize()
        assert _pad_untouched(wb, n * 4) and _pad_untouched(ws, n) and _pad_untouched(wv, n)
        return boxes.view(R, NC - 1, 4), scores.view(R, NC - 1), valid.view(R, NC - 1)
    boxes, scores, valid = _twice(run)
    rb, rs, rv, mag, pwh = R64.box_postprocess(logits[:, :NC], deltas[:, :4 * NC].view(R, NC, 4), props, hw, img, thresh, K.BOXPOST_MIN_SIZE)
    plain_s, e_s, plain_b, e_b = R64.box_postprocess_bounds(logits[:, :NC], rs, mag, pwh)
    _assert_bound(scores, rs, e_s, f"scores NC={NC}")
    _assert_bound(boxes, rb, e_b, f"boxes NC={NC}")
    need_s = (((scores.double() - rs).abs() - plain_s) / (2 * EPS * rs)).max()
    need_b = (((boxes.double() - rb).abs() - plain_b - 10 * EPS * 0.5 * pwh) / (EPS * 0.5 * pwh)).max()
    print(f"[measure] box_postprocess NC={NC}: expf units needed, scores {float(need_s):.2f}, boxes {float(need_b):.2f}")
    assert ((valid == 0) | (valid == 1)).all()
    assert torch.equal(valid.bool(), rv), f"{int((valid.bool() != rv).sum())} valid flags differ"
    eq = torch.arange(R, device=DEV) % 4 == 2
    if NC in (2, 64) and bool(eq.any()):
        assert (scores[eq] == 1.0 / NC).all(), "equal logits, NC a power of two: exactly 1 / NC"
    if R >= 8:
        assert not valid[torch.arange(R, device=DEV) % 7 == 3].any(), "boxes clipped to zero width are not valid"
        assert bool(valid.any())


def test_box_postprocess_rejects():
    logits, deltas, props = _randn(2, 5), _randn(2, 20), torch.tensor([[0.0, 0, 9, 9]] * 2, device=DEV)
    hw, img = torch.tensor([[32.0, 32.0]], device=DEV), torch.zeros(2, dtype=torch.int32, device=DEV)
    boxes, scores, valid = _nan(2, 4, 4), _nan(2, 4), _idx(2, 4)
    for R, NC, l_cs, d_cs in ((0, 5, 5, 20), (2, 1, 5, 20), (2, 5, 4, 20), (2, 5, 5, 19)):
        _rejected("adh_box_postprocess", logits.data_ptr(), l_cs, deltas.data_ptr(), d_cs, props.data_ptr(), hw.data_ptr(), img.data_ptr(),
                  R, NC, 0.05, 1e-2, boxes.data_ptr(), scores.data_ptr(), valid.data_ptr())
    assert torch.isnan(boxes).all() and torch.isnan(scores).all() and (valid == -7).all()
