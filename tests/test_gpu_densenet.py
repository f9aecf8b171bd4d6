"""DenseNet121 HDEN training on the HIP engine (csrc/densenet.hip, Engine.bn_relu_preact, _DenseNet121._run_grad) and the
stand-alone classifier driver (train.train_classifier / evaluate_classifier), against float64 torch restatements.

Kernel units go through the C ABI with NaN-prefilled outputs where a kernel stores.  The whole-backbone gate is the fixture
rule err_gpu <= 3 * err_fp32 + 3e-4 of each tensor's scale, err_fp32 the float32 restatement's own error against float64
along the same graph.  Forward tensors (logits, features, loss, the 242 running statistics) are continuous across every kink
and are held against the FREE-RUNNING restatements: a reference that owes nothing to the output under test.  Only the
parameter gradients, which jump at a kink, take the replay of the ReLU masks the kernels used (engine.RELU_CAPTURE) in both
restatements -- after those masks have been audited against the ones float64 chose on its own (tests/_util.py kink_audit)."""
import os
import warnings

import pytest
import torch
import torch.nn.functional as F

import adam_dehaze_amd.classifier as CL
import adam_dehaze_amd.engine as E
from adam_dehaze_amd import _hip as H
from adam_dehaze_amd import loss as L
from oracle import ref_cpu as R
from tests import _densenet_ref as DR
from tests._thirdparty_init import densenet121_sd
from tests._util import kink_audit, kink_recording, max_abs

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _nan(*shape):
    return torch.full(shape, float("nan"), device=DEV)


# ------------------------------------------------------------------------------------------------ kernel units
@pytest.mark.parametrize("C,cs,P", [(4, 8, 1), (36, 100, 513), (256, 260, 2048 + 77), (1024, 1024, 1500), (1024, 1056, 700)])
def test_slice_stats_and_moments_vs_float64(C, cs, P):
    g = torch.Generator().manual_seed(C + P)
    buf = (torch.randn(P, cs, generator=g) * 2.0 + 3.0).to(DEV)
    nblk = H.value("adh_bn_slice_stats_num_blocks", P, C)
    part = _nan(nblk, 2, C)
    H.call("adh_bn_slice_stats", buf.data_ptr(), cs, P, C, part.data_ptr())
    x64 = buf[:, :C].double().cpu()
    assert max_abs(part[:, 0].double().sum(0).cpu(), x64.sum(0)) < 1e-5 * P * 5
    assert max_abs(part[:, 1].double().sum(0).cpu(), (x64 * x64).sum(0)) < 1e-5 * P * 30
    mom = torch.full((2, C + 8), float("nan"), device=DEV, dtype=torch.float64)
    H.call("adh_bn_slice_moments", part.data_ptr(), nblk, C, C, float(P), mom[0, 4:].data_ptr(), mom[1, 4:].data_ptr())
    mean, var = x64.mean(0), x64.var(0, unbiased=False)
    assert max_abs(mom[0, 4:4 + C].cpu(), mean) < 2e-6 * 5
    assert max_abs(mom[1, 4:4 + C].cpu(), var) < 2e-5 * 10
    assert torch.isnan(mom[:, :4]).all() and torch.isnan(mom[:, 4 + C:]).all()      # nothing outside [0, C) written
    part2 = _nan(nblk, 2, C)
    H.call("adh_bn_slice_stats", buf.data_ptr(), cs, P, C, part2.data_ptr())
    assert torch.equal(part, part2)


def test_fold_moments_updates_buffers_like_batchnorm():
    C, P = 40, 37
    x = torch.randn(P, C, dtype=torch.float64) * 1.5 + 0.5
    mean, var = x.mean(0), x.var(0, unbiased=False)
    gamma, beta = torch.rand(C) + 0.5, torch.randn(C) * 0.1
    rm, rv = torch.randn(C) * 0.1, torch.rand(C) + 0.5
    rm_d, rv_d = rm.clone().to(DEV), rv.clone().to(DEV)
    nbt = torch.zeros((), dtype=torch.int64, device=DEV)
    ss, mu, inv = _nan(2, C), _nan(C), _nan(C)
    mean_d, var_d, gamma_d, beta_d = mean.to(DEV), var.to(DEV), gamma.to(DEV), beta.to(DEV)   # (kept alive across the launch)
    H.call("adh_bn_fold_moments", C, mean_d.data_ptr(), var_d.data_ptr(), float(P), gamma_d.data_ptr(), beta_d.data_ptr(), 1e-5,
           0.1, rm_d.data_ptr(), rv_d.data_ptr(), ss[0].data_ptr(), ss[1].data_ptr(), mu.data_ptr(), inv.data_ptr(),
           nbt.data_ptr())
    rm64, rv64 = rm.double().clone(), rv.double().clone()
    y = F.batch_norm(x, rm64, rv64, gamma.double(), beta.double(), training=True, momentum=0.1, eps=1e-5)
    invstd = 1.0 / torch.sqrt(var + 1e-5)
    assert max_abs(x * ss[0].double().cpu() + ss[1].double().cpu(), y) < 1e-5
    assert max_abs(inv.cpu(), invstd) < 1e-6 * float(invstd.max())
    assert max_abs(rm_d.cpu(), rm64) < 1e-6 and max_abs(rv_d.cpu(), rv64) < 1e-6
    assert int(nbt) == 1


@pytest.mark.parametrize("N,Hh,Ww,C,gcs", [(2, 5, 7, 8, 12), (1, 6, 9, 36, 36), (3, 2, 3, 4, 4), (2, 65, 66, 64, 80)])
def test_avgpool2_bwd_vs_autograd(N, Hh, Ww, C, gcs):
    gen = torch.Generator().manual_seed(N * Hh * Ww + C)
    x = torch.randn(N, C, Hh, Ww, dtype=torch.float64, requires_grad=True)
    y = F.avg_pool2d(x, 2, 2)
    gy = torch.randn(y.shape, dtype=torch.float64, generator=gen)
    y.backward(gy)
    OH, OW = Hh // 2, Ww // 2
    g = torch.zeros(N, OH, OW, gcs, device=DEV)
    g[..., :C] = gy.permute(0, 2, 3, 1).float().to(DEV)
    gx = _nan(N, Hh, Ww, C + 4)
    H.call("adh_avgpool2_bwd", g.data_ptr(), gcs, N, Hh, Ww, C, gx.data_ptr(), C + 4, 0)
    ref = x.grad.permute(0, 2, 3, 1)
    assert max_abs(gx[..., :C].cpu(), ref) < 1e-6
    assert torch.isnan(gx[..., C:]).all()
    if Hh % 2:
        assert torch.equal(gx[:, -1, :, :C].cpu(), torch.zeros(N, Ww, C))   # the dropped odd row: exact zeros
    base = torch.randn(N, Hh, Ww, C + 4, generator=gen).to(DEV)
    acc = base.clone()
    H.call("adh_avgpool2_bwd", g.data_ptr(), gcs, N, Hh, Ww, C, acc.data_ptr(), C + 4, 1)
    assert max_abs(acc[..., :C].cpu(), base[..., :C].double().cpu() + ref) < 1e-5
    assert torch.equal(acc[..., C:], base[..., C:])


def _preact_case(P, C, cs, training, seed):
    gen = torch.Generator().manual_seed(seed)
    x64 = torch.randn(P, C, dtype=torch.float64, generator=gen) * 1.3 + 0.2
    dA = torch.randn(P, C, dtype=torch.float64, generator=gen)
    gamma = (torch.rand(C, generator=gen) + 0.5).double()
    beta = (torch.randn(C, generator=gen) * 0.2).double()
    rm = (torch.randn(C, generator=gen) * 0.1).double()
    rv = (torch.rand(C, generator=gen) + 0.5).double()
    buf = torch.zeros(P, cs, device=DEV)
    buf[:, :C] = x64.float().to(DEV)
    xf = buf[:, :C].double().cpu()                     # x as the kernel sees it (fp32)
    xr = xf.clone().requires_grad_(True)
    g_ = gamma.clone().requires_grad_(True)
    b_ = beta.clone().requires_grad_(True)
    z = F.batch_norm(xr.view(P, C, 1, 1), rm.clone(), rv.clone(), g_, b_, training=training, momentum=0.1, eps=1e-5)
    a = F.relu(z).view(P, C)
    a.backward(dA)
    return buf, xf, dA, gamma, beta, rm, rv, xr.grad, g_.grad, b_.grad


@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("P,C,cs", [(700, 64, 96), (1500, 36, 40), (96, 1024, 1056)])
def test_preact_bwd_accumulates_into_strided_gradient(training, P, C, cs):
    """adh_bn_bwd_reduce + adh_bn_bwd_finalize + adh_bn_preact_bwd_accum (the Engine.bn_relu_preact backward) against
    F.batch_norm + relu autograd in float64, added into a non-zero gradient buffer at the buffer's channel stride."""
    buf, xf, dA, gamma, beta, rm, rv, gx_ref, dg_ref, db_ref = _preact_case(P, C, cs, training, P + C)
    gm, bt = gamma.float().to(DEV), beta.float().to(DEV)
    ss = _nan(2, C)
    if training:
        mean, var = xf.mean(0), xf.var(0, unbiased=False)
        mu, inv = _nan(C), _nan(C)
        mean_d, var_d = mean.to(DEV), var.to(DEV)
        H.call("adh_bn_fold_moments", C, mean_d.data_ptr(), var_d.data_ptr(), float(P), gm.data_ptr(), bt.data_ptr(), 1e-5, 0.1,
               None, None, ss[0].data_ptr(), ss[1].data_ptr(), mu.data_ptr(), inv.data_ptr(), None)
    else:
        rmf, rvf = rm.float().to(DEV), rv.float().to(DEV)
        H.call("adh_bn_fold_eval", C, gm.data_ptr(), bt.data_ptr(), rmf.data_ptr(), rvf.data_ptr(), 1e-5, None, ss[0].data_ptr(),
               ss[1].data_ptr())
        mu, inv, junk = rmf, _nan(C), _nan(C)
        H.call("adh_bn_fold_eval", C, None, None, rmf.data_ptr(), rvf.data_ptr(), 1e-5, None, inv.data_ptr(), junk.data_ptr())
    dAd = torch.zeros(P, C + 4, device=DEV)
    dAd[:, :C] = dA.float().to(DEV)
    nblk = H.value("adh_bn_bwd_num_blocks", P, C)
    part = _nan(nblk, 2, C)
    H.call("adh_bn_bwd_reduce", dAd.data_ptr(), C + 4, None, 0, H.ACT_RELU, buf.data_ptr(), cs, mu.data_ptr(), inv.data_ptr(),
           part.data_ptr(), P, C, ss.data_ptr(), None)
    dg, db, coef = _nan(C), _nan(C), _nan(3, C)
    H.call("adh_bn_bwd_finalize", part.data_ptr(), nblk, C, float(P), gm.data_ptr() if training else None, inv.data_ptr(),
           dg.data_ptr(), db.data_ptr(), 0, coef.data_ptr())
    gen = torch.Generator().manual_seed(7)
    prior = torch.randn(P, cs, generator=gen).to(DEV)
    dbuf = prior.clone()
    coef_p = coef if training else ss
    H.call("adh_bn_preact_bwd_accum", dAd.data_ptr(), C + 4, buf.data_ptr(), cs, ss.data_ptr(), mu.data_ptr() if training else None,
           inv.data_ptr() if training else None, coef_p.data_ptr(), int(training), dbuf.data_ptr(), cs, P, C, 1)
    scale = float(gx_ref.abs().max())
    assert max_abs(dbuf[:, :C].double().cpu() - prior[:, :C].double().cpu(), gx_ref) < 2e-5 * max(1.0, scale) * (4 if C == 1024 else 1)
    assert torch.equal(dbuf[:, C:], prior[:, C:])                      # channels past the slice untouched
    assert max_abs(db.cpu(), db_ref) < 1e-5 * P ** 0.5 * 4
    assert max_abs(dg.cpu(), dg_ref) < 1e-5 * P ** 0.5 * 4
    # store form (accumulate = 0) and bit-reproducibility
    st = _nan(P, cs)
    H.call("adh_bn_preact_bwd_accum", dAd.data_ptr(), C + 4, buf.data_ptr(), cs, ss.data_ptr(), mu.data_ptr() if training else None,
           inv.data_ptr() if training else None, coef_p.data_ptr(), int(training), st.data_ptr(), cs, P, C, 0)
    assert torch.isnan(st[:, C:]).all()
    assert max_abs(st[:, :C].double().cpu(), gx_ref) < 2e-5 * max(1.0, scale) * (4 if C == 1024 else 1)
    part2 = _nan(nblk, 2, C)
    H.call("adh_bn_bwd_reduce", dAd.data_ptr(), C + 4, None, 0, H.ACT_RELU, buf.data_ptr(), cs, mu.data_ptr(), inv.data_ptr(),
           part2.data_ptr(), P, C, ss.data_ptr(), None)
    assert torch.equal(part, part2)


# ------------------------------------------------------------------------------------------------ whole backbone
def _model(sd):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m = CL.FogIntensityClassifier("densenet121", 3, pretrained=True)
    m.load_state_dict(sd, strict=True)
    return m.to(DEV)


def _sd(sd, dtype, grads=True):
    out = {k: (v.clone().to(dtype) if v.is_floating_point() else v.clone()) for k, v in sd.items()}
    if grads:
        for k, v in out.items():
            if v.is_floating_point() and "running" not in k:
                v.requires_grad_(True)
    return out


def _gate(name, got, ref64, ref32):
    got, ref64, ref32 = got.detach().double().cpu(), ref64.detach().double().cpu(), ref32.detach().double().cpu()
    scale = max(float(ref64.abs().max()), 1e-30)
    e_gpu = float((got - ref64).abs().max()) / scale
    e_ref = float((ref32 - ref64).abs().max()) / scale
    return None if e_gpu <= 3.0 * e_ref + 3e-4 else (name, e_gpu, e_ref)


def _kinks_of(m, cap):
    """(ReLU masks, post-activation tensors) of engine.RELU_CAPTURE by parameter name, NCHW on the CPU, channel padding cropped"""
    post = {k: cap[id(p)][..., :p.shape[0]].detach().permute(0, 3, 1, 2).cpu() for k, p in m.named_parameters() if id(p) in cap}
    return {k: o > 0 for k, o in post.items()}, post


@pytest.mark.parametrize("N,Hh,Ww", [(2, 64, 96), (2, 70, 90)])
def test_backbone_train_step_every_tensor_vs_float64(N, Hh, Ww):
    sd = densenet121_sd(seed=N + Hh)
    m = _model(sd).train()
    hazy, _, labels = R.synthetic_batch(N, Hh, Ww, seed=Hh)
    gen = torch.Generator().manual_seed(Ww)
    m0 = (torch.rand(N, 1024, generator=gen) >= 0.3).float() / 0.7
    m1 = (torch.rand(N, 256, generator=gen) >= 0.2).float() / 0.8
    masks = (m0.view(N, 1, 1, 1024).to(DEV), m1.view(N, 1, 1, 256).to(DEV))
    old = E.RELU_CAPTURE
    E.RELU_CAPTURE = {}
    try:
        logits, feats = CL._ClassifierFunction.apply(m, True, hazy.to(DEV).contiguous(), masks, *list(m.parameters()))
        loss = L.cross_entropy3(logits, labels.to(DEV))
        loss.backward()
        torch.cuda.synchronize()
        cap = E.RELU_CAPTURE
    finally:
        E.RELU_CAPTURE = old
    relu_masks, post = _kinks_of(m, cap)
    assert len(relu_masks) == 1 + 58 + 58 + 3 + 1      # norm0, every norm1 / norm2, the transitions, norm5
    free, refs = {}, {}
    for dt in (torch.float64, torch.float32):
        # forward tensors (logits, features, loss, running statistics): the FREE-RUNNING restatement, which owes nothing to
        # the output under test -- a channel tail, row or tile a fused BN + ReLU kernel left at zero shows here
        sdf = _sd(sd, dt, grads=False)
        with torch.no_grad(), kink_recording() as rec:
            lg, ft = DR.classifier_forward(hazy.to(dt), sdf, training=True, drop_masks=(m0.to(dt), m1.to(dt)))
            free[dt] = (lg, ft, F.cross_entropy(lg, labels), sdf, rec)
    audit = kink_audit(f"densenet train {N}x{Hh}x{Ww}", free[torch.float64][4], family="densenet", masks=relu_masks, post=post,
                       rec32=free[torch.float32][4])
    audit.covers(relu_masks)
    for dt in (torch.float64, torch.float32):
        # parameter gradients, which jump at a kink: the kernels' own (audited) ReLU masks replayed
        sdr = _sd(sd, dt)
        lg, ft = DR.classifier_forward(hazy.to(dt), sdr, training=True, drop_masks=(m0.to(dt), m1.to(dt)), relu_masks=relu_masks)
        F.cross_entropy(lg, labels).backward()
        refs[dt] = sdr
    (l64, f64_, s64, sdf64, _), (l32, f32_, s32, sdf32, _) = free[torch.float64], free[torch.float32]
    sd64, sd32 = refs[torch.float64], refs[torch.float32]
    bad = [_gate("logits", logits, l64, l32), _gate("features", feats, f64_, f32_), _gate("loss", loss.view(1), s64.view(1),
                                                                                          s32.view(1))]
    msd = m.state_dict()
    names = dict(m.named_parameters())
    nbuf = 0
    for k, v in msd.items():
        if "running" in k:
            bad.append(_gate(k, v, sdf64[k], sdf32[k]))
            nbuf += 1
        elif k.endswith("num_batches_tracked"):
            assert int(v) == 1, k
    assert nbuf == 2 * 121
    for k, p in names.items():
        assert p.grad is not None, k
        bad.append(_gate(k + ".grad", p.grad, sd64[k].grad, sd32[k].grad))
    bad = [b for b in bad if b is not None]
    assert not bad, bad[:10]


def test_eval_mode_trainable_gamma_beta_gradients():
    """frozen statistics (module.eval()) with gradients: every parameter against F.batch_norm(training=False) in float64"""
    N, Hh, Ww = 2, 64, 96
    sd = densenet121_sd(seed=21)
    m = _model(sd).eval()
    hazy, _, labels = R.synthetic_batch(N, Hh, Ww, seed=22)
    old = E.RELU_CAPTURE
    E.RELU_CAPTURE = {}
    try:
        logits, feats = m(hazy.to(DEV))
        loss = L.cross_entropy3(logits, labels.to(DEV))
        loss.backward()
        torch.cuda.synchronize()
        cap = E.RELU_CAPTURE
    finally:
        E.RELU_CAPTURE = old
    relu_masks, post = _kinks_of(m, cap)
    free, refs = {}, {}
    for dt in (torch.float64, torch.float32):      # the logits: free-running; the gradients: the (audited) masks replayed
        with torch.no_grad(), kink_recording() as rec:
            free[dt] = (DR.classifier_forward(hazy.to(dt), _sd(sd, dt, grads=False), training=False)[0], rec)
    audit = kink_audit("densenet eval 2x64x96", free[torch.float64][1], family="densenet", masks=relu_masks, post=post,
                       rec32=free[torch.float32][1])
    audit.covers(relu_masks)
    for dt in (torch.float64, torch.float32):
        sdr = _sd(sd, dt)
        lg, ft = DR.classifier_forward(hazy.to(dt), sdr, training=False, relu_masks=relu_masks)
        F.cross_entropy(lg, labels).backward()
        refs[dt] = sdr
    l64, l32 = free[torch.float64][0], free[torch.float32][0]
    sd64, sd32 = refs[torch.float64], refs[torch.float32]
    bad = [_gate("logits", logits, l64, l32)]
    for k, p in m.named_parameters():
        assert p.grad is not None, k
        bad.append(_gate(k + ".grad", p.grad, sd64[k].grad, sd32[k].grad))
    bad = [b for b in bad if b is not None]
    assert not bad, bad[:10]
    for k, v in m.state_dict().items():
        if "running" in k:
            assert torch.equal(v.cpu(), sd[k]), k
        elif k.endswith("num_batches_tracked"):
            assert int(v) == 0, k


def test_full_size_train_step_with_adam_bit_reproducible():
    """8 x 3 x 512 x 1024 (the config-2 frame): fwd + CE + bwd + Adam twice from the same state: bit-equal loss and gradients,
    the loss equals an fp64 cross-entropy of the logits, every parameter gets a finite non-zero gradient and moves, every BN
    buffer changes."""
    from adam_dehaze_amd.optim import Adam
    sd = densenet121_sd(seed=31)
    x = torch.rand(8, 3, 512, 1024, generator=torch.Generator().manual_seed(32)).to(DEV)
    labels = torch.arange(8, device=DEV) % 3
    ones = (torch.ones(8, 1, 1, 1024, device=DEV), torch.ones(8, 1, 1, 256, device=DEV))
    runs = []
    for _ in range(2):
        m = _model(sd).train()
        opt = Adam(list(m.parameters()), lr=1e-4, weight_decay=1e-4)
        logits, _ = CL._ClassifierFunction.apply(m, True, x, ones, *list(m.parameters()))
        loss = L.cross_entropy3(logits, labels)
        loss.backward()
        grads = {k: p.grad.clone() for k, p in m.named_parameters()}
        opt.step()
        torch.cuda.synchronize()
        runs.append((logits.detach().clone(), loss.detach().clone(), grads, {k: v.clone() for k, v in m.state_dict().items()}))
    (l0, s0, g0, st0), (l1, s1, g1, st1) = runs
    assert torch.isfinite(l0).all() and torch.isfinite(s0)
    ref = F.cross_entropy(l0.double().cpu(), labels.cpu())
    assert abs(float(s0) - float(ref)) < 1e-5 * max(1.0, float(ref))
    assert torch.equal(l0, l1) and torch.equal(s0, s1)
    assert len(g0) == len(list(m.parameters()))
    for k in g0:
        assert torch.isfinite(g0[k]).all(), k
        assert torch.equal(g0[k], g1[k]), k
        assert bool((g0[k] != 0).any()), k
        assert not torch.equal(st0[k].cpu(), sd[k]), k
        assert torch.equal(st0[k], st1[k]), k
    for k, v in st0.items():
        if "running" in k:
            assert not torch.equal(v.cpu(), sd[k]), k
        elif k.endswith("num_batches_tracked"):
            assert int(v) == 1, k


def test_joint_training_with_densenet121_hden():
    """train_joint with classifier.model = densenet121 at the reduced branch widths of tests/test_gpu_train.py: the step
    completes and every classifier parameter takes one Adam step"""
    from adam_dehaze_amd import train as T
    from tests.test_gpu_train import _cfg
    cfg = _cfg()
    cfg["classifier"]["model"] = "densenet121"
    torch.manual_seed(5)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        system = T.build_joint_system(cfg)
    clf = system["classifier"]
    clf.train()
    system["router"].train()
    before = {k: p.detach().clone() for k, p in clf.named_parameters()}
    for batch in T.synthetic_loader(2, 64, 1, seed=9, device=DEV):
        loss = float(T.joint_train_step(system, batch)["loss"])
    torch.cuda.synchronize()
    assert loss == loss and abs(loss) < 1e3
    for k, p in clf.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all(), k
        assert not torch.equal(before[k], p.detach()), k
    assert int(clf.state_dict()["backbone.features.denseblock2.denselayer3.norm1.num_batches_tracked"]) == 1


# ------------------------------------------------------------------------------------------------ classifier driver
@pytest.mark.parametrize("name", ["resnet18", "densenet121"])
def test_train_and_evaluate_classifier_on_synthetic_frames(name, tmp_path):
    from adam_dehaze_amd import train as T
    from training.train_classifier import evaluate_classifier, train_classifier
    from tests.test_gpu_train import _cfg
    cfg = _cfg()
    cfg["classifier"].update({"model": name, "checkpoint_dir": str(tmp_path / "clf"), "learning_rate": 1e-4,
                              "weight_decay": 1e-4, "epochs": 5})
    cfg["dataset"].update({"batch_size": 4, "img_size": 64})
    torch.manual_seed(11)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        model = train_classifier(cfg, steps=2, val_steps=1)
    assert any("SYNTHETIC" in str(x.message) for x in w)
    best = os.path.join(cfg["classifier"]["checkpoint_dir"], "best_model.pth")
    ck = torch.load(best, map_location="cpu")
    assert set(ck) == {"epoch", "model_state_dict", "optimizer_state_dict", "val_acc", "val_loss"}
    assert os.path.exists(os.path.join(cfg["classifier"]["checkpoint_dir"], "checkpoint_epoch_5.pth"))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        fresh = CL.FogIntensityClassifier(name, 3, pretrained=False)
    fresh.load_state_dict(ck["model_state_dict"], strict=True)
    for k, v in model.state_dict().items():                  # the best model was reloaded at the end
        assert torch.equal(v.cpu(), ck["model_state_dict"][k].cpu()), k
    res = evaluate_classifier(model, cfg, steps=2)
    cm = res["confusion_matrix"]
    assert cm.shape == (3, 3) and int(cm.sum()) == 2 * 4
    assert abs(res["accuracy"] - 100.0 * int(cm.trace()) / int(cm.sum())) < 1e-9
    assert "low" in res["classification_report"] and "weighted avg" in res["classification_report"]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        system = T.build_joint_system(cfg)
    got = system["classifier"].state_dict()
    for k, v in ck["model_state_dict"].items():
        assert torch.equal(got[k].cpu(), v.cpu()), k
