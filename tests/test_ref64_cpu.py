"""The float64 references of tests/_ref64.py against the matching oracle.ref_cpu functions (fp32) on small inputs, to
fp64-vs-fp32 accuracy, plus a float64 finite-difference check of the LPIPS gradient formula and the seed checks of the
decision-margin rule used by the GPU tests.  Needs no GPU: this is what says the references are right."""
import math

import numpy as np
import pytest
import torch

from oracle import ref_cpu as R
from tests import _ref64 as R64
from tests import _cases as K

EPS = 2.0 ** -24


def _rand(*shape, seed=0):
    return torch.rand(shape, generator=torch.Generator().manual_seed(seed))


def _randn(*shape, seed=0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed))


def test_fog_vs_oracle():
    clear = _rand(3, 3, 37, 5, seed=1)
    beta, air = torch.tensor([0.0, 0.15, 3.0]), torch.tensor([0.6, 1.0, 0.0])
    got = R64.fog(clear, beta, air).float().clamp(0, 1)
    assert torch.equal(got, R.apply_fog(clear, beta, air))         # both: float64 arithmetic, one rounding to fp32


def test_fog_single_row_and_column():
    for shape in [(1, 3, 1, 1), (2, 3, 1, 9), (2, 3, 9, 1)]:
        clear = _rand(*shape, seed=2)
        beta, air = torch.full((shape[0],), 0.95), torch.full((shape[0],), 0.6)
        assert torch.equal(R64.fog(clear, beta, air).float().clamp(0, 1), R.apply_fog(clear, beta, air))


def test_psnr_vs_oracle():
    p, t = _rand(3, 3, 16, 24, seed=3), _rand(3, 3, 16, 24, seed=4)
    ref = R.psnr_per_image(p, t)
    got = R64.psnr(p.flatten(1), t.flatten(1))
    # the oracle subtracts in fp32: relative 2 EPS on the mse, 10 / ln 10 * that in dB
    assert float((got - ref).abs().max()) <= 10 / math.log(10) * 2 * EPS + 1e-12
    assert torch.isinf(R64.psnr(p.flatten(1), p.flatten(1))).all()


@pytest.mark.parametrize("hw", [(7, 7), (7, 39), (39, 38), (45, 71)])
def test_ssim_vs_oracle(hw):
    p, t = _rand(2, 3, *hw, seed=5), _rand(2, 3, *hw, seed=6)
    ref = R.ssim_per_image(p, t)
    got = R64.ssim_gray(p, t)
    assert float((got - ref).abs().max()) < 1e-12
    c = torch.full((1, 3, *hw), 0.3)
    assert float((R64.ssim_gray(c, c) - 1).abs().max()) < 1e-12


def test_paired_augment_vs_oracle():
    x = _rand(8, 3, 17, 33, seed=7)
    params = torch.tensor([[i & 1, (i >> 1) & 1, (i >> 2) & 1, 0.9 + 0.05 * i, 1.1 - 0.03 * i] for i in range(8)], dtype=torch.float32)
    got, _ = R64.paired_augment(x, params)
    assert float((got - R.paired_augment(x, params).double()).abs().max()) < 16 * EPS
    # out-of-range input: the contrast-first mean is that of the UNCLAMPED image, in the oracle too
    x2 = 1.7 * x - 0.3
    got2, _ = R64.paired_augment(x2, params)
    assert float((got2 - R.paired_augment(x2, params).double()).abs().max()) < 16 * EPS


@pytest.mark.parametrize("dup_mode", [0, 1])
@pytest.mark.parametrize("repeats", [1, 2, 3, 4])
def test_adam_vs_oracle(dup_mode, repeats):
    p, g, m, v = _randn(257, seed=8).double(), _randn(257, seed=9).double(), 0.1 * _randn(257, seed=10).double(), \
        0.01 * _rand(257, seed=11).double()
    kw = dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8)
    (p1, m1, v1), (ep, em, ev) = R64.adam(p, g, m, v, 5, repeats, dup_mode, wd=1e-2, gscale=1.0, **kw)
    po, mo, vo = p.clone(), m.clone(), v.clone()
    (R.adam_step if dup_mode == 0 else R.adam_step_foreach)(po, g, mo, vo, 5, weight_decay=1e-2, repeats=repeats, **kw)
    for a, b in ((p1, po), (m1, mo), (v1, vo)):
        assert float((a - b).abs().max()) < 1e-13                          # float64 on both sides
    assert float(ep.max()) < 1e-6 and float(em.max()) < 1e-5 and float(ev.max()) < 1e-5   # the bounds are fp32-sized


def test_nms_vs_oracle():
    for seed in range(4):
        b, g = K.int_boxes(150, seed, ngroups=3, zero_area=seed % 2 == 1)
        keep = R64.nms_sorted(b.numpy(), g.numpy(), 0.5)
        scores = torch.arange(150, 0, -1).float()
        ref = R.det_nms(b, scores, g, 0.5)
        assert np.array_equal(np.nonzero(keep)[0], ref.numpy())
    for name, (b, g, thr, expect) in K.nms_hand_cases().items():
        assert R64.nms_sorted(b.numpy(), g.numpy(), thr).tolist() == expect, name


def test_roi_align_vs_oracle():
    feat = _randn(2, 4, 9, 13, seed=12)                                    # NCHW for the oracle
    rois = torch.tensor([[0, 3.0, 2.0, 40.0, 30.0], [1, -20.0, -9.0, 17.0, 60.0], [1, 10.0, 10.0, 10.5, 10.2],
                         [0, 300.0, 300.0, 340.0, 350.0], [1, 44.0, 0.0, 52.0, 36.0]])
    ref = R.det_roi_align(feat, rois, 0.25)
    got, mag = R64.roi_align(feat.permute(0, 2, 3, 1).contiguous(), rois, 0.25)
    assert float(((got - ref.double()).abs() - 32 * EPS * mag).max()) <= 0
    assert float(got[3].abs().max()) == 0.0


def test_fpn_level_boundaries():
    sides = torch.tensor([56.0, 112.0, 224.0, 448.0, 896.0, 111.99, 0.0])
    rois = torch.stack([torch.zeros(7), torch.zeros(7), torch.zeros(7), sides, sides], 1)
    lvl, _ = R64.fpn_level(rois, 4)
    assert lvl.tolist() == [0, 1, 2, 3, 3, 0, 0]
    s = torch.sqrt((rois[:, 3] - rois[:, 1]) * (rois[:, 4] - rois[:, 2]))
    ref = (torch.floor(4 + torch.log2(s / 224) + torch.tensor(1e-6)).clamp(2, 5) - 2).long()    # det_box_head's line
    assert lvl.tolist() == ref.tolist()


def test_rpn_decode_vs_oracle():
    H, W, A = 3, 5, 3
    base = R.det_base_anchors(64.0)
    anchors = R64.rpn_anchors(H, W, base, 8, 16)
    sx, sy = torch.arange(W).float() * 16, torch.arange(H).float() * 8
    yy, xx = torch.meshgrid(sy, sx, indexing="ij")
    shifts = torch.stack([xx.reshape(-1), yy.reshape(-1)] * 2, dim=1)
    assert torch.equal(anchors.float(), (shifts.view(-1, 1, 4) + base.view(1, -1, 4)).reshape(-1, 4))   # det_rpn's anchors
    d = _randn(H * W * A, 4, seed=13)
    d[::4, 2:] = 6.0
    ref = R.det_clip(R.det_decode(d, anchors.float(), (1.0, 1.0, 1.0, 1.0)), (20.0, 70.0))
    got, mag, _ = R64.decode_clip(d, anchors, (1.0, 1.0, 1.0, 1.0), 20.0, 70.0)
    assert float(((got - ref.double()).abs() - 16 * EPS * mag).max()) <= 0


def test_box_postprocess_vs_oracle():
    Rn, NC = 6, 5
    logits, deltas = 3 * _randn(Rn, NC, seed=14), 2 * _randn(Rn, NC * 4, seed=15)
    props = torch.tensor([[5.0, 6, 50, 40], [0, 0, 90, 60], [30, 20, 31, 60], [10, 10, 80, 50], [60, 5, 95, 25], [1, 1, 9, 9]])
    b, sc, valid, mag, _ = R64.box_postprocess(logits, deltas.view(Rn, NC, 4), props, torch.tensor([[64.0, 96.0]]),
                                               torch.zeros(Rn, dtype=torch.int32), 0.05, 1e-2)
    rois = torch.cat([torch.zeros(Rn, 1), props], 1)
    ref_b = R.det_clip(R.det_decode(deltas.view(-1, NC, 4), rois[:, None, 1:].expand(-1, NC, -1), (10.0, 10.0, 5.0, 5.0)), (64.0, 96.0))
    assert float(((b - ref_b[:, 1:].double()).abs() - 16 * EPS * mag).max()) <= 0
    assert float((sc - torch.softmax(logits, -1)[:, 1:].double()).abs().max()) < 8 * EPS
    dets = R.det_postprocess(logits, deltas, rois, (64.0, 96.0), 1, nms_thresh=2.0, per_img=10 ** 6)[0]   # IoU <= 1: the NMS keeps all
    assert dets["scores"].numel() == int(valid.sum())


def test_nearest_src_vs_torch():
    for o, i in [(10, 5), (9, 5), (13, 7), (3, 1), (5, 1), (7, 7), (25, 13), (42, 21), (256, 128)]:
        ref = torch.nn.functional.interpolate(torch.arange(i).float().view(1, 1, 1, i), size=(1, o), mode="nearest").view(-1).long()
        assert torch.equal(R64.nearest_src(o, i), ref), (o, i)


def test_lpips_pixel_vs_oracle_lines():
    """ref_cpu.lpips_alex's tap distance: a / (sqrt(sum a^2) + 1e-10), squared difference, 1 x 1 lin, spatial mean."""
    a, b = torch.relu(_randn(2, 8, 5, 7, seed=16)), torch.relu(_randn(2, 8, 5, 7, seed=17))
    w = _rand(8, seed=18)
    na = a / (torch.sqrt(torch.sum(a * a, dim=1, keepdim=True)) + 1e-10)
    nb = b / (torch.sqrt(torch.sum(b * b, dim=1, keepdim=True)) + 1e-10)
    ref = torch.nn.functional.conv2d((na - nb) ** 2, w.view(1, 8, 1, 1)).mean(dim=(2, 3)).view(-1)
    nhwc = lambda t: t.permute(0, 2, 3, 1).reshape(2, 35, 8)
    got = R64.lpips_pixel(nhwc(a), nhwc(b), w).mean(1)
    assert float((got - ref.double()).abs().max()) < 64 * EPS


def test_lpips_s2d_is_the_conv1_rearrangement():
    """conv1 (11 x 11, stride 4, pad 2) of the scaled image == 3 x 3 stride-1 conv of the space-to-depth tensor."""
    img = _rand(2, 3, 19, 27, seed=19).double()
    a3, b3 = torch.tensor([2.0, 3.0, 0.5]), torch.tensor([-1.0, 0.25, 0.0])
    OH, OW = (19 + 4 - 11) // 4 + 1, (27 + 4 - 11) // 4 + 1
    s2d, _ = R64.lpips_s2d(img.float(), a3, b3, OH + 2, OW + 2)
    wgt = _randn(4, 3, 11, 11, seed=20).double()
    scaled = img * a3.double().view(1, 3, 1, 1) + b3.double().view(1, 3, 1, 1)
    ref = torch.nn.functional.conv2d(scaled, wgt, stride=4, padding=2)
    w12 = torch.zeros(4, 3, 12, 12, dtype=torch.float64)
    w12[:, :, :11, :11] = wgt
    w1 = w12.view(4, 3, 3, 4, 3, 4).permute(0, 3, 5, 1, 2, 4).reshape(4, 48, 3, 3)
    got = torch.nn.functional.conv2d(s2d.permute(0, 3, 1, 2), w1)[:, :, :OH, :OW]
    assert float((got - ref).abs().max()) < 1e-11
    # the backward reference is the adjoint of the forward one
    g = _randn(2, OH + 2, OW + 2, 48, seed=21).double()
    lhs = ((s2d - R64.lpips_s2d(torch.zeros(2, 3, 19, 27), a3, b3, OH + 2, OW + 2)[0]) * g).sum()
    rhs = (img * R64.lpips_s2d_bwd(g, a3, 19, 27)).sum()
    assert abs(float(lhs - rhs)) < 1e-10


def test_lpips_grad_finite_difference_and_autograd():
    a, b = torch.relu(_randn(2, 6, 8, seed=22)).double() + 0.0, torch.relu(_randn(2, 6, 8, seed=23)).double()
    a[0, 2] = 0.0                                                       # an all-zero pixel of fa
    w, gv = _rand(8, seed=24).double(), torch.tensor([0.7, -1.3], dtype=torch.float64)
    grad = R64.lpips_layer_grad(a, b, w, gv)
    av = a.clone().requires_grad_(True)
    (R64.lpips_pixel(av, b, w).mean(1) * gv).sum().backward()
    nz = torch.ones(2, 6, dtype=torch.bool)
    nz[0, 2] = False
    assert float((grad[nz] - av.grad[nz]).abs().max()) < 1e-12
    assert torch.isnan(av.grad[0, 2]).all()                             # autograd: NaN at the zero pixel
    assert torch.equal(grad[0, 2], 2 * w * (0 - b[0, 2] / (b[0, 2].norm() + 1e-10)) * (gv[0] / 6) / 1e-10)   # the convention
    f = lambda t: float((R64.lpips_pixel(t, b, w).mean(1) * gv).sum())
    for (n, p, c) in [(0, 0, 1), (1, 3, 5), (1, 5, 0), (0, 4, 7)]:
        h = 1e-6
        ap, am = a.clone(), a.clone()
        ap[n, p, c] += h
        am[n, p, c] -= h
        assert abs((f(ap) - f(am)) / (2 * h) - float(grad[n, p, c])) < 1e-8


def test_margin_rule_seeds_leave_nothing_out():
    """The decision cases of the GPU tests regenerate elements closer than 64 EPS (relative) to a decision boundary; the
    chosen seeds must end with zero such elements."""
    for nlevels in (1, 2, 3, 4):
        rois, left = K.random_rois(64, nlevels, seed=nlevels)
        assert left == 0
        assert float(R64.fpn_level(rois, nlevels)[1].min()) > 512 * EPS
        assert float(K.roi_sample_margin(rois, K.fpn_shapes(nlevels)).min()) > 1e-3
    for NC in K.BOXPOST_NC:
        for Rn in (1, 3, 1000):
            logits, deltas, props, img, thresh, left = K.boxpost_inputs(Rn, NC, seed=NC)
            assert left == 0, (NC, Rn)
            sc = torch.softmax(logits.double(), -1)[:, 1:]
            assert float(((sc - thresh).abs() / thresh).min()) > 64 * EPS
            if Rn == 1000:
                _, _, valid, _, _ = R64.box_postprocess(logits, deltas, props, torch.tensor(K.BOXPOST_IMG_HW), img, thresh, K.BOXPOST_MIN_SIZE)
                assert 0.02 < float(valid.double().mean()) < 0.98          # both outcomes are well represented
