"""The two frozen feature extractors behind the training loss -- ContentLoss (VGG16 / VGG19 taps) and PerceptualLoss (LPIPS on
AlexNet) -- against the float64 oracle with the kernels' own kinks replayed (tests/_loss_extractor.py):

  a. every tap of `_features`, at the smallest input at which each layer still exists, at odd sizes where the pool floor
     drops a row and a column, with taps ON conv indices (whose ReLU runs as a pass of its own) and on VGG19;
  b. the loss value and its input gradient under an upstream gradient that is not 1, plus loss(p, p) == 0 exactly, the
     no-grad run and run-to-run bit equality;
  c. the convolutions that occur only in these extractors (3x3 pad 0 on 48 channels, 5x5 pad 2, 3x3 at 192 .. 512 channels
     on maps of 1x1 to 4x6 pixels), layer by layer through Engine.conv as the losses call it.

Gate, everywhere: err_gpu <= 3 * err_ref + floor, errors as max-abs over the float64 tensor's max-abs, err_ref the distance
of the fp32 CPU oracle from the float64 one along the same graph.  Forward tensors (taps, layer outputs, loss values) are
continuous across every kink, so they are held against the FREE-RUNNING oracle: a reference that owes nothing to the output
under test, and a tile, row or channel tail a kernel left at zero shows.  Only the gradients, which jump at a kink, take the
replay: the SAME ReLU masks (engine.RELU_CAPTURE) and max-pool choices (computed here from the captured pool inputs, first
index on ties) forced on the float64 and the fp32 oracle -- after an audit (tests/_util.py kink_audit) of those masks and
choices against the ones the free-running float64 run took on its own: they come from the output under test, and only
near-kinks may differ.  The
factor 3 covers the MFMA kernels' other summation order and F(4x4,3x3), which the project's own comparison puts at up to 3x
the direct kernel's rounding.  Floors (tests/_loss_extractor.py), per convolution in the chain: 4e-6 for forward tensors,
1.2e-5 (at most 3e-4) for gradients.  Every row is printed and appended to profile_out/loss_extractor_gate.txt (or to the
file ADH_GATE_TABLE names);
profiles/loss_extractor_gate.txt is the table of the run these floors were checked against."""
import contextlib
import warnings

import pytest
import torch
import torch.nn.functional as F

import adam_dehaze_amd.engine as E
from adam_dehaze_amd import _hip as H
from adam_dehaze_amd import loss as L
from adam_dehaze_amd.engine import Act, Engine
from oracle import ref_cpu as R
from tests import _loss_extractor as LX
from tests._thirdparty_init import lpips_alex_sd, vgg16_sd, vgg19_sd
from tests._util import DEV, KinkRecord, _same_bits, _twice, kink_audit, kink_recording

pytestmark = pytest.mark.gpu


@contextlib.contextmanager
def _capture():
    old, cap = E.RELU_CAPTURE, {}
    E.RELU_CAPTURE = cap
    try:
        yield cap
    finally:
        E.RELU_CAPTURE = old


@pytest.fixture
def entries(monkeypatch):
    """take(): the conv entry points launched since the last take() (which family Engine._select chose: printed, not
    asserted), so that a row names the launches its own tensor came from: the forward pass's or the backward pass's."""
    called = []
    real_call = H.call

    def recording(name, *a, **kw):
        if name.startswith("adh_conv") and name not in called:
            called.append(name)
        return real_call(name, *a, **kw)
    monkeypatch.setattr(H, "call", recording)

    def take():
        names = ",".join(e[len("adh_conv_"):] for e in called)
        del called[:]
        return names
    return take


@pytest.fixture
def engines(monkeypatch):
    """Every Engine made while the test runs."""
    made = []
    init = Engine.__init__

    def spy(self, device, record):
        init(self, device, record)
        made.append(self)
    monkeypatch.setattr(Engine, "__init__", spy)
    return made


def _images(shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(shape, generator=g), torch.rand(shape, generator=g)


def _engine(record):
    eng = Engine(torch.device(DEV), record)
    eng.wino43 = "dgrad"        # as both losses set it: the forward pass keeps F(2x2,3x3)
    return eng


def _nchw(a: Act):
    return a.t[..., :a.C].permute(0, 3, 1, 2)


def _content(model, names, seed=2):
    sd = (vgg19_sd if model == "vgg19" else vgg16_sd)(seed)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        c = L.ContentLoss(model, list(names))
    c.load_state_dict(sd, strict=True)
    return c.to(DEV), sd


def _perceptual(seed=5):
    sd = lpips_alex_sd(seed)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        pl = L.PerceptualLoss()
    pl.load_state_dict(sd, strict=True)
    return pl.to(DEV), sd


def _kinks(module, cap, pool_sources, k, s):
    """(masks, pools) of the pass whose ReLU outputs `cap` holds (the prediction's: it runs after the target's and files its
    outputs under the same keys).  pool_sources: {oracle pool key: name of the conv whose ReLU output that pool reads}."""
    by_name = {name: cap[id(p)] for name, p in module.named_parameters() if id(p) in cap}
    masks = {name: (o > 0).permute(0, 3, 1, 2).cpu() for name, o in by_name.items()}
    pools = {}
    for key, src in pool_sources.items():
        o = by_name.get(src)
        if o is not None and o.shape[1] >= k and o.shape[2] >= k:
            pools[key] = LX.pool_choice(o.permute(0, 3, 1, 2).cpu(), k, s)
    return masks, pools


def _post(module, cap):
    """{conv weight name: the ReLU output the kernels wrote, NCHW on the CPU}: what _kinks derives the masks from."""
    return {name: cap[id(p)].detach().permute(0, 3, 1, 2).cpu() for name, p in module.named_parameters() if id(p) in cap}


def _vgg_kinks(c, cap, cfg):
    return _kinks(c, cap, {f"model.{p}": f"model.{src}.weight" for p, src in LX.vgg_pool_sources(cfg).items()}, 2, 2)


def _relus_of(cfg, taps):
    """names of the convs whose ReLU runs in features[:max(taps)+1]."""
    out, idx = set(), 0
    for v in cfg:
        if v == "M":
            idx += 1
        else:
            if idx + 1 <= max(taps):
                out.add(f"model.{idx}.weight")
            idx += 2
    return out


def _lpips_kinks(pl, cap):
    return _kinks(pl, cap, LX.LPIPS_POOLS, 3, 2)


# ------------------------------------------------------------------------------------------------ a. per-tap features
SINGLE = [("vgg16", (n,), (1, 3, 32, 32)) for n in LX.LAYER_MAPPING]
MULTI = [("vgg16", LX.DEFAULT_NAMES, (2, 3, 37, 51)), ("vgg16", LX.DEFAULT_NAMES, (3, 3, 33, 32)),
         ("vgg16", ("relu1_1", "relu2_2"), (2, 3, 37, 51)), ("vgg16", ("relu3_1", "relu3_3", "relu4_2"), (2, 3, 37, 51)),
         ("vgg19", LX.DEFAULT_NAMES, (2, 3, 37, 51))]
LPIPS_SHAPES = [(1, 3, 31, 31), (3, 3, 35, 47), (2, 3, 67, 99)]


def _case_id(v):
    return "+".join(map(str, v)) if isinstance(v, tuple) else str(v)


@pytest.mark.parametrize("model,names,shape", SINGLE + MULTI, ids=_case_id)
def test_vgg_taps_vs_float64(model, names, shape, entries):
    c, sd = _content(model, names)
    cfg, taps = LX.CFGS[model], LX.taps_of(names)
    x, _ = _images(shape, 100 + sum(shape) + taps[0])

    def run():
        entries()
        with _capture() as cap:
            feats = c._features(_engine(False), x.to(DEV), c.tap_indices, {})
        run.cap, run.fwd = cap, entries()
        return tuple(_nchw(f) for f in feats)
    feats = _twice(run)
    assert len(feats) == len(taps)
    assert _vgg_kinks(c, run.cap, cfg)[0].keys() == _relus_of(cfg, taps), "every ReLU of the walk is captured, fused or not"
    ref64 = LX.vgg_features(x.double(), LX.cast_sd(sd, torch.float64), taps, cfg)
    ref32 = LX.vgg_features(x, sd, taps, cfg)
    gate = LX.Gate(f"taps {model} {'+'.join(names)} {'x'.join(map(str, shape))}")
    for tap, f, r32, r64 in zip(taps, feats, ref32, ref64):
        gate.check(f"tap{tap}", f, r32, r64, LX.fwd_floor(LX.vgg_convs_up_to(cfg, tap)), run.fwd)
    gate.done()


@pytest.mark.parametrize("shape", LPIPS_SHAPES, ids=_case_id)
def test_lpips_taps_vs_float64(shape, entries):
    pl, sd = _perceptual()
    x, _ = _images(shape, 200 + sum(shape))

    def run():
        entries()
        with _capture() as cap:
            feats = pl._features(_engine(False), x.to(DEV), {})
        run.cap, run.fwd = cap, entries()
        return tuple(_nchw(f) for f in feats)
    feats = _twice(run)
    assert [f.shape[1] for f in feats] == [64, 192, 384, 256, 256]
    masks, pools = _lpips_kinks(pl, run.cap)
    assert len(masks) == 5 and len(pools) == 2, "the stem's ReLU output is captured under the parameter's id"
    ref64 = LX.alex_features(x.double(), LX.cast_sd(sd, torch.float64))
    ref32 = LX.alex_features(x, sd)
    gate = LX.Gate(f"taps lpips {'x'.join(map(str, shape))}")
    for k, (f, r32, r64) in enumerate(zip(feats, ref32, ref64)):
        gate.check(f"relu{k + 1}", f, r32, r64, LX.fwd_floor(k + 1), run.fwd)
    gate.done()


# ------------------------------------------------------------------------------------------------ b. value and input gradient
LOSS_CASES = [("vgg16", ("relu1_1",), (1, 3, 32, 32)), ("vgg16", ("relu3_2",), (1, 3, 32, 32)),
              ("vgg16", ("relu5_3",), (1, 3, 32, 32))] + MULTI


def _exactly_zero_on_identical_inputs(module, pred):
    p = pred.to(DEV).requires_grad_(True)
    v = module(p, pred.to(DEV))
    assert float(v.detach().abs().max()) == 0.0, "loss(p, p) is exactly 0"
    v.sum().backward()
    assert p.grad is not None and float(p.grad.abs().max()) == 0.0, "and so is its input gradient"


def _no_grad_run(module, pred, target, val, engines):
    del engines[:]
    v = module(pred.to(DEV), target.to(DEV))
    assert not v.requires_grad and _same_bits(v.detach(), val), "value without a gradient: the same bits"
    assert engines and all(not e.record and not e.tape for e in engines), "nothing is recorded without a gradient to take"


@pytest.mark.parametrize("model,names,shape", LOSS_CASES, ids=_case_id)
def test_content_loss_value_and_gradient_vs_float64(model, names, shape, entries, engines):
    c, sd = _content(model, names)
    cfg, taps = LX.CFGS[model], tuple(LX.taps_of(names))
    pred, target = _images(shape, 300 + sum(shape) + taps[0])

    def run():
        p = pred.to(DEV).requires_grad_(True)
        entries()
        with _capture() as cap:
            val = c(p, target.to(DEV))
            run.fwd = entries()
            (0.37 * val).backward()
        run.cap, run.bwd = cap, entries()
        return val.detach(), p.grad
    val, grad = _twice(run)
    assert any(e.record for e in engines)
    masks, pools = _vgg_kinks(c, run.cap, cfg)

    def oracle(dt):
        p = pred.to(dt).clone().requires_grad_(True)
        v = R.content_loss(p, target.to(dt), LX.cast_sd(sd, dt), taps=taps, cfg=cfg)
        (0.37 * v).backward()
        return v.detach().reshape(1), p.grad
    with kink_recording() as rec64:
        v64, _ = oracle(torch.float64)                                     # the value: free-running
    with kink_recording() as rec32:
        v32, _ = oracle(torch.float32)
    audit = kink_audit(f"content {model} {'+'.join(names)} {'x'.join(map(str, shape))}", rec64, family="extractors", masks=masks,
                       post=_post(c, run.cap), pools=pools, rec32=rec32)
    _, g64 = LX.run_forced(lambda: oracle(torch.float64), masks, pools, audit)    # the gradient: of the piece the kernels took
    _, g32 = LX.run_forced(lambda: oracle(torch.float32), masks, pools, audit)
    gate = LX.Gate(f"content {model} {'+'.join(names)} {'x'.join(map(str, shape))}")
    nconv = LX.vgg_convs_up_to(cfg, taps[-1])
    gate.check("value", val.reshape(1), v32, v64, LX.fwd_floor(nconv), run.fwd)
    gate.check("grad", grad, g32, g64, LX.grad_floor(nconv), run.bwd)
    gate.done()
    _no_grad_run(c, pred, target, val, engines)
    _exactly_zero_on_identical_inputs(c, pred)


@pytest.mark.parametrize("shape", LPIPS_SHAPES, ids=_case_id)
def test_perceptual_loss_value_and_gradient_vs_float64(shape, entries, engines):
    pl, sd = _perceptual()
    pred, target = _images(shape, 400 + sum(shape))
    N = shape[0]
    wgt = 0.25 + 1.5 * torch.rand(N, generator=torch.Generator().manual_seed(N))     # per-image upstream gradient

    def run():
        p = pred.to(DEV).requires_grad_(True)
        entries()
        with _capture() as cap:
            val = pl(p, target.to(DEV))
            run.fwd = entries()
            assert val.shape == (N, 1, 1, 1)
            (val.view(-1) * wgt.to(DEV)).sum().backward()
        run.cap, run.bwd = cap, entries()
        return val.detach(), p.grad
    val, grad = _twice(run)
    assert any(e.record for e in engines)
    masks, pools = _lpips_kinks(pl, run.cap)
    assert len(masks) == 5 and len(pools) == 2

    def oracle(dt):
        p = pred.to(dt).clone().requires_grad_(True)
        v = R.perceptual_loss(p, target.to(dt), LX.cast_sd(sd, dt))
        (v.view(-1) * wgt.to(dt)).sum().backward()
        return v.detach(), p.grad
    with kink_recording() as rec64:
        v64, _ = oracle(torch.float64)
    with kink_recording() as rec32:
        v32, _ = oracle(torch.float32)
    audit = kink_audit(f"lpips {'x'.join(map(str, shape))}", rec64, family="extractors", masks=masks, post=_post(pl, run.cap),
                       pools=pools, rec32=rec32)
    _, g64 = LX.run_forced(lambda: oracle(torch.float64), masks, pools, audit)
    _, g32 = LX.run_forced(lambda: oracle(torch.float32), masks, pools, audit)
    gate = LX.Gate(f"lpips {'x'.join(map(str, shape))}")
    gate.check("value", val, v32, v64, LX.fwd_floor(5), run.fwd)
    gate.check("grad", grad, g32, g64, LX.grad_floor(5), run.bwd)
    gate.done()
    _no_grad_run(pl, pred, target, val, engines)
    _exactly_zero_on_identical_inputs(pl, pred)


# ------------------------------------------------------------------------------------------------ c. the extractor-only convolutions
def _layer_cases():
    out = []
    for nhw in ((2, 9, 9), (1, 17, 25)):
        out.append((48, 64, 3, 0) + nhw)                       # the space-to-depth AlexNet stem
    for nhw in ((2, 3, 3), (1, 7, 11)):
        out.append((64, 192, 5, 2) + nhw)                      # AlexNet conv2
    for cin, cout in ((192, 384), (384, 256), (256, 256)):     # AlexNet conv3 .. conv5
        for nhw in ((2, 1, 1), (1, 3, 5)):
            out.append((cin, cout, 3, 1) + nhw)
    for cin, cout in ((128, 256), (256, 512), (512, 512)):     # VGG blocks 3 .. 5
        for nhw in ((1, 1, 1), (2, 2, 3), (1, 4, 6)):
            out.append((cin, cout, 3, 1) + nhw)
    for cin, cout in ((3, 64), (64, 64)):                      # VGG block 1 (the image as NHWC8)
        out.append((cin, cout, 3, 1, 1, 5, 7))
    return out


@pytest.mark.parametrize("Cin,Cout,k,pad,N,Hh,Ww", _layer_cases(), ids=lambda v: str(v))
def test_extractor_conv_layer_vs_float64(Cin, Cout, k, pad, N, Hh, Ww, entries):
    """bias, no BatchNorm, fused ReLU, frozen weights, F(4x4,3x3) for the data gradient only: the call of both losses."""
    g = torch.Generator().manual_seed(Cin * 1000 + Cout + Hh)
    x = torch.randn(N, Cin, Hh, Ww, generator=g)
    w = torch.randn(Cout, Cin, k, k, generator=g) / (Cin * k * k) ** 0.5
    b = 0.5 * torch.randn(Cout, generator=g)
    OH, OW = Hh + 2 * pad - k + 1, Ww + 2 * pad - k + 1
    gout = torch.randn(N, Cout, OH, OW, generator=g)
    Cp = 8 if Cin == 3 else Cin
    xd = torch.zeros(N, Hh, Ww, Cp)
    xd[..., :Cin] = x.permute(0, 2, 3, 1)
    xd, wd, bd = xd.to(DEV), w.to(DEV), b.to(DEV)

    def run():
        eng = _engine(True)
        xa = Act(xd, Cp)
        entries()
        with _capture() as cap:
            o = eng.conv(xa, wd, bd, None, k=k, stride=1, pad=pad, relu=True)
        run.fwd = entries()
        assert cap[id(wd)] is o.t and o.t.shape[:3] == (N, OH, OW)
        gpad = torch.zeros(o.t.shape, device=DEV)
        gpad[..., :Cout] = gout.permute(0, 2, 3, 1).to(DEV)
        o.grad = gpad
        eng.backward()
        torch.cuda.synchronize()
        run.bwd = entries()
        return _nchw(o), xa.grad[..., :Cin].permute(0, 3, 1, 2)
    out, gx = _twice(run)
    mask = (out > 0).cpu()

    def oracle(dt, mask=None):
        xr = x.to(dt).clone().requires_grad_(True)
        y = F.conv2d(xr, w.to(dt), b.to(dt), padding=pad)
        rec = KinkRecord()
        rec.relu["conv"] = [y.detach()]
        y = F.relu(y) if mask is None else y * mask.to(dt)
        (y * gout.to(dt)).sum().backward()
        return y.detach(), xr.grad, rec
    (y64, _, rec64), (y32, _, rec32) = oracle(torch.float64), oracle(torch.float32)    # the output: free-running ReLU
    kink_audit(f"conv {Cin}->{Cout} k{k}p{pad} {N}x{Hh}x{Ww}", rec64, family="extractors", masks={"conv": mask},
               post={"conv": out.detach().cpu()}, rec32=rec32)      # the mask about to be replayed: near-kinks only
    (_, g64, _), (_, g32, _) = oracle(torch.float64, mask), oracle(torch.float32, mask)      # the gradient: the kernel's own mask
    gate = LX.Gate(f"conv {Cin}->{Cout} k{k}p{pad} {N}x{Hh}x{Ww}")
    gate.check("out", out, y32, y64, LX.fwd_floor(1), run.fwd)
    gate.check("dgrad", gx, g32, g64, LX.grad_floor(1), run.bwd)
    gate.done()
