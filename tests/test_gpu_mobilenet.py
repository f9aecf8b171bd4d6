"""MobileNetV2 / V3 HDEN backbones on the MI355X: the depthwise kernels (depthwise.hip) against float64 F.conv2d(groups=C),
the ReLU6 / Hardswish / Hardsigmoid passes against torch autograd at their kinks, and the three backbones against the
float64 restatement in tests/_mobilenet_ref.py (eval forward, train forward + backward, frozen-statistics backward)."""
import warnings

import pytest
import torch
import torch.nn.functional as F

from adam_dehaze_amd import _hip as H
from adam_dehaze_amd import classifier as CL
from adam_dehaze_amd import loss as L
from oracle import ref_cpu as R
from tests import _mobilenet_ref as MR
from tests._util import kink_audit, kink_recording, max_abs, rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAMES = ("mobilenet_v2", "mobilenet_v3_large", "mobilenet_v3_small")
ACTS = {H.ACT_NONE: lambda z: z, H.ACT_RELU: F.relu, H.ACT_RELU6: F.relu6, H.ACT_HARDSWISH: F.hardswish,
        H.ACT_HARDSIGMOID: F.hardsigmoid}


# ------------------------------------------------------------------------------------------------ depthwise kernels
def _dw_run(x, w, k, s, C, cs, scale=None, shift=None, act=H.ACT_NONE, stats=False):
    """x: [N,H,W,cs] (channels [0,C) used), w: [C,1,k,k] -> (out [N,OH,OW,C], stats or None)."""
    N, Hh, Ww, _ = x.shape
    pad = (k - 1) // 2
    OH, OW = (Hh + 2 * pad - k) // s + 1, (Ww + 2 * pad - k) // s + 1
    wp = torch.empty(k * k * C, device=DEV)
    H.call("adh_dwconv_pack_weights", w.data_ptr(), H.WLayout(1, C, k, k, 0, 0, 0, 0, 0), wp.data_ptr())
    out = torch.empty(N, OH, OW, C, device=DEV)
    st = None
    if stats:
        st = torch.empty(H.value("adh_dwconv_num_blocks", N * OH * OW, C), 2, C, device=DEV)
    H.call("adh_dwconv_fwd", x.data_ptr(), cs, N, Hh, Ww, C, k, s, wp.data_ptr(), out.data_ptr(), C, OH, OW, H.ptr(scale),
           H.ptr(shift), act, H.ptr(st))
    return out, st, wp


CASES = [(k, s, C, shp) for k in (3, 5) for s in (1, 2) for C, shp in
         ((16, (2, 33, 47)), (24, (1, 7, 7)), (72, (2, 33, 47)), (88, (1, 20, 24)), (144, (2, 17, 15)), (960, (1, 9, 11)))]


@pytest.mark.parametrize("k,s,C,shp", CASES)
def test_depthwise_fwd_dgrad_wgrad_vs_fp64(k, s, C, shp):
    g = torch.Generator().manual_seed(k * 100 + s * 10 + C)
    N, Hh, Ww = shp
    extra = 8 if C == 72 else 0        # one case reads a channel slice of a wider buffer (x_cs > C)
    xb = torch.randn(N, Hh, Ww, C + extra, generator=g)
    x = xb[..., :C]
    w = torch.randn(C, 1, k, k, generator=g) / k
    xd = xb.to(DEV)
    wd = w.to(DEV)
    out, st, wp = _dw_run(xd, wd, k, s, C, C + extra, stats=True)
    x64 = x.double().permute(0, 3, 1, 2).requires_grad_(True)
    w64 = w.double().requires_grad_(True)
    ref = F.conv2d(x64, w64, None, s, (k - 1) // 2, 1, C)
    refn = ref.detach().permute(0, 2, 3, 1)
    assert rel_err(out, refn) < 1e-5
    # the BatchNorm partial sums: sum y and sum y^2 per channel
    assert rel_err(st[:, 0].sum(0).double(), refn.reshape(-1, C).sum(0)) < 1e-4
    assert rel_err(st[:, 1].sum(0).double(), (refn ** 2).reshape(-1, C).sum(0)) < 1e-5
    # backward of sum(out * gout)
    gout = torch.randn(refn.shape, generator=g, dtype=torch.float64)
    ref.backward(gout.permute(0, 3, 1, 2))
    OH, OW = refn.shape[1], refn.shape[2]
    gd = gout.float().to(DEV).contiguous()
    gx = torch.empty(N, Hh, Ww, C + extra, device=DEV)
    H.call("adh_dwconv_dgrad", gd.data_ptr(), C, N, OH, OW, C, k, s, wp.data_ptr(), gx.data_ptr(), C + extra, Hh, Ww, 0)
    assert rel_err(gx[..., :C], x64.grad.permute(0, 2, 3, 1)) < 1e-5
    nblk = H.value("adh_dwconv_wgrad_num_blocks", N * OH * OW, C)
    part = torch.empty(nblk * k * k * C, device=DEV)
    dw = torch.empty(C, 1, k, k, device=DEV)
    H.call("adh_dwconv_wgrad", xd.data_ptr(), C + extra, N, Hh, Ww, C, k, s, gd.data_ptr(), C, OH, OW, part.data_ptr(), nblk,
           dw.data_ptr(), 0)
    assert rel_err(dw, w64.grad) < 1e-5
    # accumulate forms
    gx2 = gx.clone()
    H.call("adh_dwconv_dgrad", gd.data_ptr(), C, N, OH, OW, C, k, s, wp.data_ptr(), gx2.data_ptr(), C + extra, Hh, Ww, 1)
    assert rel_err(gx2[..., :C], 2 * x64.grad.permute(0, 2, 3, 1)) < 1e-5
    # bit-equal run to run
    out_b, st_b, _ = _dw_run(xd, wd, k, s, C, C + extra, stats=True)
    dw_b = torch.empty_like(dw)
    H.call("adh_dwconv_wgrad", xd.data_ptr(), C + extra, N, Hh, Ww, C, k, s, gd.data_ptr(), C, OH, OW, part.data_ptr(), nblk,
           dw_b.data_ptr(), 0)
    gx_b = torch.empty_like(gx)
    H.call("adh_dwconv_dgrad", gd.data_ptr(), C, N, OH, OW, C, k, s, wp.data_ptr(), gx_b.data_ptr(), C + extra, Hh, Ww, 0)
    torch.cuda.synchronize()
    assert torch.equal(out, out_b) and torch.equal(st, st_b) and torch.equal(dw, dw_b) and torch.equal(gx[..., :C], gx_b[..., :C])


@pytest.mark.parametrize("act", sorted(ACTS))
@pytest.mark.parametrize("k,s", [(3, 1), (3, 2), (5, 1), (5, 2)])
def test_depthwise_eval_epilogue_every_activation(act, k, s):
    g = torch.Generator().manual_seed(7 + act)
    C = 24
    x = torch.randn(2, 13, 18, C, generator=g)
    w = torch.randn(C, 1, k, k, generator=g)
    scale = 0.5 + torch.rand(C, generator=g)
    shift = torch.randn(C, generator=g)
    out, _, _ = _dw_run(x.to(DEV), w.to(DEV), k, s, C, C, scale.to(DEV), shift.to(DEV), act)
    y = F.conv2d(x.double().permute(0, 3, 1, 2), w.double(), None, s, (k - 1) // 2, 1, C).permute(0, 2, 3, 1)
    ref = ACTS[act](y * scale.double() + shift.double())
    assert max_abs(out, ref) < 1e-4 * max(1.0, float(ref.abs().max()))


# ------------------------------------------------------------------------------------------------ activations
@pytest.mark.parametrize("act", [H.ACT_RELU6, H.ACT_HARDSWISH, H.ACT_HARDSIGMOID, H.ACT_RELU])
def test_activation_passes_vs_autograd_at_kinks(act):
    """adh_bn_apply forward, adh_bn_bwd_reduce / adh_bn_bwd_apply backward (train and eval) with pre-activations placed on
    0, 6, +-3 and either side of them: the derivative must follow torch autograd's convention at every kink."""
    C = 16
    kinks = torch.tensor([-3.5, -3.0, -2.75, -0.25, 0.0, 0.25, 2.75, 3.0, 3.5, 5.75, 6.0, 6.25, -1.0, 1.0, 4.0, 8.0])
    P = 64
    z = kinks.repeat(P, 1)[:, torch.randperm(C, generator=torch.Generator().manual_seed(1))]
    z[1::2] = torch.randn(P // 2, C, generator=torch.Generator().manual_seed(2)) * 4
    scale = torch.full((C,), 0.5)       # y = 2 z exactly: z = fma(y, 0.5, 0) hits the kinks bit-exactly
    shift = torch.zeros(C)
    y = (2 * z).to(DEV).contiguous()
    ss = torch.stack([scale, shift]).to(DEV).contiguous()
    out = torch.empty(P, C, device=DEV)
    H.call("adh_bn_apply", y.data_ptr(), C, ss[0].data_ptr(), ss[1].data_ptr(), None, 0, act, out.data_ptr(), C, P, C, None)
    z64 = z.double().requires_grad_(True)
    ref = ACTS[act](z64)
    assert max_abs(out, ref.detach()) < 1e-6
    gout = torch.randn(P, C, generator=torch.Generator().manual_seed(3), dtype=torch.float64)
    ref.backward(gout)
    gd = gout.float().to(DEV)
    # eval (frozen statistics): g_y = scale * act'(z) * g
    coef = torch.zeros(3, C, device=DEV)
    coef[0] = ss[0]
    gy = torch.empty(P, C, device=DEV)
    H.call("adh_bn_bwd_apply", gd.data_ptr(), C, out.data_ptr(), C, act, y.data_ptr(), C, None, None, coef.data_ptr(), 0,
           gy.data_ptr(), C, None, 0, P, C, ss.data_ptr(), None)
    assert max_abs(gy, 0.5 * z64.grad) < 1e-6
    # train: the masked sums of bn_bwd_reduce are sum(act'(z) g) and sum(act'(z) g xhat)
    mean = torch.zeros(C, device=DEV)
    invstd = torch.ones(C, device=DEV)
    nblk = H.value("adh_bn_bwd_num_blocks", P, C)
    part = torch.empty(nblk, 2, C, device=DEV)
    H.call("adh_bn_bwd_reduce", gd.data_ptr(), C, out.data_ptr(), C, act, y.data_ptr(), C, mean.data_ptr(), invstd.data_ptr(),
           part.data_ptr(), P, C, ss.data_ptr(), None)
    gm = z64.grad
    assert max_abs(part[:, 0].sum(0), gm.sum(0)) < 1e-4
    assert max_abs(part[:, 1].sum(0), (gm * 2 * z64.detach()).sum(0)) < 1e-3


# ------------------------------------------------------------------------------------------------ backbones
def _model(name, sd):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m = CL.FogIntensityClassifier(name, 3, pretrained=True)
    m.load_state_dict(sd, strict=True)
    return m.to(DEV)


def _sd64(sd, grads=True):
    out = {k: (v.clone().double() if v.is_floating_point() else v.clone()) for k, v in sd.items()}
    if grads:
        for k, v in out.items():
            if v.is_floating_point() and "running" not in k:
                v.requires_grad_(True)
    return out


@pytest.mark.parametrize("name", NAMES)
def test_backbone_eval_forward_vs_restatement(name):
    sd = MR.state_dict(name, seed=3)
    m = _model(name, sd).eval()
    hazy, _, _ = R.synthetic_batch(3, 96, 160, seed=5)
    with torch.no_grad():
        logits, feats = m(hazy.to(DEV))
        ref_logits, ref_feats = MR.classifier_forward(hazy.double(), _sd64(sd, False), name)
    assert logits.shape == (3, 3) and feats.shape == (3, MR.FEATURE_DIM[name])
    assert rel_err(feats, ref_feats) < 1e-3
    assert max_abs(logits, ref_logits) < 1e-3 * max(1.0, float(ref_logits.abs().max()))
    srt = ref_logits.sort(dim=1, descending=True).values
    safe = (srt[:, 0] - srt[:, 1]) > 1e-3
    assert torch.equal(logits.argmax(1).cpu()[safe], ref_logits.argmax(1)[safe])


GRAD_KEYS = {
    "mobilenet_v2": ("backbone.features.0.0.weight", "backbone.features.2.conv.1.0.weight", "backbone.features.5.conv.2.weight",
                     "backbone.features.7.conv.1.1.weight", "backbone.features.18.0.weight"),
    "mobilenet_v3_large": ("backbone.features.0.0.weight", "backbone.features.4.block.1.0.weight",
                           "backbone.features.4.block.2.fc1.bias", "backbone.features.4.block.2.fc2.weight",
                           "backbone.features.5.block.3.0.weight", "backbone.features.13.block.1.1.weight",
                           "backbone.features.1.block.0.0.weight"),
    "mobilenet_v3_small": ("backbone.features.0.0.weight", "backbone.features.4.block.1.0.weight",
                           "backbone.features.1.block.1.fc1.bias", "backbone.features.9.block.2.fc2.weight",
                           "backbone.features.6.block.3.0.weight", "backbone.features.9.block.1.1.weight"),
}
BN_KEY = {"mobilenet_v2": "backbone.features.3.conv.1.1", "mobilenet_v3_large": "backbone.features.4.block.1.1",
          "mobilenet_v3_small": "backbone.features.4.block.1.1"}


def _check_train_forward_backward_vs_restatement(name):
    """Train-mode BN + cross-entropy backward against the float64 restatement, with the ReLU / ReLU6 derivative masks the
    kernels used replayed in the restatement (engine.RELU_CAPTURE): with only 24 .. 96 samples per BatchNorm channel in the
    last stages, a pre-activation that rounds to the other side of a kink in fp32 moves whole gradients by percents (fp32
    torch itself lands 4 % from fp64 on mobilenet_v2 here); with the masks matched both sides differentiate the same piece
    of the network and the gate is 2e-2 of each gradient's scale.

    The replay touches the derivative only: the restatement's forward under act_masks is relu / relu6 of its own
    pre-activation (6, not 0, above the upper kink; tests/test_kink_audit_cpu.py pins that its values are bit-equal to the
    free run's), so logits, loss and BN buffers are held against a reference that owes nothing to the kernels' output.  The
    masks themselves are audited against the ones float64 chose on its own before they are used (tests/_util.py kink_audit,
    both kinks of ReLU6; the fp32 restatement's own masks are the yardstick)."""
    import adam_dehaze_amd.engine as E
    sd = MR.state_dict(name, seed=4)
    m = _model(name, sd).train()
    fd = MR.FEATURE_DIM[name]
    hazy, _, labels = R.synthetic_batch(4, 64, 96, seed=6)
    ones = (torch.ones(4, 1, 1, fd, device=DEV), torch.ones(4, 1, 1, 256, device=DEV))
    old = E.RELU_CAPTURE
    E.RELU_CAPTURE = {}
    try:
        logits, feats = CL._ClassifierFunction.apply(m, True, hazy.to(DEV).contiguous(), ones, *list(m.parameters()))
        loss = L.cross_entropy3(logits, labels.to(DEV))
        loss.backward()
        torch.cuda.synchronize()
        cap = E.RELU_CAPTURE
    finally:
        E.RELU_CAPTURE = old
    masks, post = {}, {}
    for k, p in m.named_parameters():
        if id(p) in cap:
            o = post[k] = cap[id(p)][..., :p.shape[0]].detach().permute(0, 3, 1, 2).cpu()
            masks[k] = ((o > 0) & (o < 6)) if name == "mobilenet_v2" else (o > 0)   # V2: ReLU6 everywhere; V3: ReLU
    assert len(masks) >= 10
    with torch.no_grad(), kink_recording() as rec32:
        MR.classifier_forward(hazy, {k: v.clone() for k, v in sd.items()}, name, training=True)
    sdr = _sd64(sd)
    with kink_recording() as rec64:      # (its forward values are the free run's: see the docstring)
        ref_logits, _ = MR.classifier_forward(hazy.double(), sdr, name, training=True, act_masks=masks)
    kink_audit(f"{name} train 4x64x96", rec64, family="mobilenet", masks=masks, post=post, rec32=rec32,
               relu6=name == "mobilenet_v2").covers(masks)
    ref_loss = F.cross_entropy(ref_logits, labels)
    ref_loss.backward()
    assert max_abs(logits, ref_logits.detach()) < 2e-3 * max(1.0, float(ref_logits.detach().abs().max()))
    assert abs(float(loss) - float(ref_loss.detach())) < 1e-3
    # running statistics after the step: catches eps / momentum plumbing
    msd = m.state_dict()
    bk = BN_KEY[name]
    assert rel_err(msd[bk + ".running_mean"], sdr[bk + ".running_mean"]) < 1e-4
    assert rel_err(msd[bk + ".running_var"], sdr[bk + ".running_var"]) < 1e-4
    assert int(msd[bk + ".num_batches_tracked"]) == 1
    names = dict(m.named_parameters())
    errs = {k: rel_err(names[k].grad, sdr[k].grad) for k in GRAD_KEYS[name] + ("classifier.1.weight", "classifier.4.weight")}
    bad = {k: e for k, e in errs.items() if not e < 2e-2}
    assert not bad, (bad, errs)


@pytest.mark.parametrize("name", NAMES)
def test_backbone_train_forward_backward_vs_restatement(name):
    _check_train_forward_backward_vs_restatement(name)


def test_v3_small_train_under_sync_bn_in_a_world_of_one(monkeypatch):
    """The synchronised-BatchNorm sequences of the dense and the depthwise layers (local sums in fp64 -> all-reduce ->
    finalize, forward and backward) with an all-reduce that leaves the sums as they are: one rank's sums are the global
    sums, so the step must meet the same float64 restatement within the same bounds."""
    import adam_dehaze_amd.engine as E
    calls = []
    monkeypatch.setattr(E, "SYNC_BN", lambda sums: calls.append(sums.numel()))
    _check_train_forward_backward_vs_restatement("mobilenet_v3_small")
    assert len(calls) >= 2 * 30 and all(n % 2 == 1 for n in calls)      # forward and backward of every BatchNorm: 2 C + 1 doubles


def test_v3_small_eval_mode_with_gradients():
    """frozen-statistics fine-tuning (module.eval() with gradients), as for resnet"""
    name = "mobilenet_v3_small"
    sd = MR.state_dict(name, seed=8)
    m = _model(name, sd).eval()
    hazy, _, labels = R.synthetic_batch(2, 64, 96, seed=9)
    logits, _ = m(hazy.to(DEV))
    loss = L.cross_entropy3(logits, labels.to(DEV))
    loss.backward()
    sdr = _sd64(sd)
    ref_logits, _ = MR.classifier_forward(hazy.double(), sdr, name, training=False)
    F.cross_entropy(ref_logits, labels).backward()
    assert max_abs(logits, ref_logits.detach()) < 1e-3 * max(1.0, float(ref_logits.abs().max()))
    names = dict(m.named_parameters())
    for k in GRAD_KEYS[name] + ("backbone.features.4.block.1.1.bias", "classifier.1.weight"):
        assert rel_err(names[k].grad, sdr[k].grad) < 2e-2, k
    assert int(m.state_dict()["backbone.features.4.block.1.1.num_batches_tracked"]) == 0


def test_mobilenet_v2_eval_full_size():
    name = "mobilenet_v2"
    sd = MR.state_dict(name, seed=10)
    m = _model(name, sd).eval()
    x = torch.rand(1, 3, 512, 1024, generator=torch.Generator().manual_seed(11))
    with torch.no_grad():
        logits, feats = m(x.to(DEV))
        ref_logits, ref_feats = MR.classifier_forward(x.double(), _sd64(sd, False), name)
    assert rel_err(feats, ref_feats) < 1e-3
    assert max_abs(logits, ref_logits) < 1e-3 * max(1.0, float(ref_logits.abs().max()))


def test_mobilenet_v3_large_train_full_size_bit_reproducible():
    name = "mobilenet_v3_large"
    sd = MR.state_dict(name, seed=12)
    x = torch.rand(8, 3, 512, 1024, generator=torch.Generator().manual_seed(13)).to(DEV)
    labels = torch.arange(8, device=DEV) % 3
    ones = (torch.ones(8, 1, 1, 960, device=DEV), torch.ones(8, 1, 1, 256, device=DEV))
    runs = []
    for _ in range(2):
        m = _model(name, sd).train()
        logits, _ = CL._ClassifierFunction.apply(m, True, x, ones, *list(m.parameters()))
        loss = L.cross_entropy3(logits, labels)
        loss.backward()
        torch.cuda.synchronize()
        runs.append((logits.detach().clone(), loss.detach().clone(),
                     {k: p.grad.clone() for k, p in m.named_parameters()}))
    (l0, s0, g0), (l1, s1, g1) = runs
    assert torch.isfinite(l0).all() and torch.isfinite(s0)
    assert torch.equal(l0, l1) and torch.equal(s0, s1)
    assert len(g0) == len(list(m.parameters()))
    for k in g0:
        assert torch.isfinite(g0[k]).all(), k
        assert torch.equal(g0[k], g1[k]), k


def test_joint_training_with_mobilenet_v3_small_hden():
    """train_joint with classifier.model = mobilenet_v3_small (the reference's config key) and the reduced branch widths of
    tests/test_gpu_train.py: two joint steps (classifier in train mode -> soft router -> joint loss -> backward -> Adam over
    every parameter).  Every classifier parameter gets a finite gradient and moves."""
    from adam_dehaze_amd import train as T
    from tests.test_gpu_train import _cfg
    cfg = _cfg()
    cfg["classifier"]["model"] = "mobilenet_v3_small"
    torch.manual_seed(3)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        system = T.build_joint_system(cfg)
    clf = system["classifier"]
    assert clf.model_name == "mobilenet_v3_small"
    clf.train()
    system["router"].train()
    before = {k: p.detach().clone() for k, p in clf.named_parameters()}
    losses = []
    for batch in T.synthetic_loader(4, 64, 2, seed=7, device=DEV):
        losses.append(float(T.joint_train_step(system, batch)["loss"]))
    torch.cuda.synchronize()
    assert len(losses) == 2 and all(l == l and abs(l) < 1e3 for l in losses)
    for k, p in clf.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all(), k
        assert not torch.equal(before[k], p.detach()), k
    assert int(clf.state_dict()["backbone.features.4.block.1.1.num_batches_tracked"]) == 2
