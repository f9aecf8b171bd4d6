"""Host side of the weight EMA (ema.WeightEMA, the `ema:` config section), without a GPU: the C ABI and its ctypes mirror,
argument validation, the launches `update()` and `applied()` issue (recorded, as tests/test_grad_clip_cpu.py records the
optimiser's: `_hip.call` is replaced by a recorder that launches nothing), the resident table, the config plumbing of the three
training stages, the epoch loop's record and checkpoint keys, and the commented block of config/config.yaml."""
import ctypes
import os
import re

import pytest
import torch

from adam_dehaze_amd import _hip as H
from adam_dehaze_amd import train as T
from adam_dehaze_amd.ema import WeightEMA
from adam_dehaze_amd.optim import Adam

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("adh_ema_begin", "adh_ema_multi", "adh_ema_swap")


def _header():
    return open(os.path.join(ROOT, "include", "adam_dehaze_hip.h")).read()


def test_symbols_in_header_signatures_and_library():
    declared = set(re.findall(r"^int\s+(adh_\w+)\s*\(", _header(), flags=re.M))
    lib = ctypes.CDLL(H.lib_path())
    for name in NEW:
        assert name in declared, f"{name} is not declared in the header"
        assert name in H._SIGNATURES, f"{name} is not in _hip._SIGNATURES"
        assert hasattr(lib, name), f"{name} is not exported by the library"
        assert name not in H._VALUE_FUNCS
    assert H._SIGNATURES["adh_ema_begin"] == [H.vp, H.vp, H.f64, H.i32, H.vp]
    assert H._SIGNATURES["adh_ema_multi"] == [H.vp, H.vp, H.vp, H.i32, H.vp]
    assert H._SIGNATURES["adh_ema_swap"] == [H.vp, H.vp, H.vp, H.i32]


def _walk(struct):
    """(name, ctype, offset) per member and the total size of `struct` as the header spells it: the C layout rule for scalars
    and pointers"""
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), _header(), flags=re.S).group(1)
    size = {"double": 8, "float": 4, "int32_t": 4, "int64_t": 8, "float*": 8}
    ctype = {"double": ctypes.c_double, "float": ctypes.c_float, "int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64,
             "float*": ctypes.c_void_p}
    offset, align, fields = 0, 1, []
    for decl in (d.strip() for d in body.split(";")):
        if not decl:
            continue
        ty, name = decl.replace("const ", "").split()
        offset = (offset + size[ty] - 1) // size[ty] * size[ty]
        fields.append((name, ctype[ty], offset))
        offset += size[ty]
        align = max(align, size[ty])
    return fields, (offset + align - 1) // align * align


@pytest.mark.parametrize("struct,mirror,total", [("adh_ema_tensor", H.EmaTensor, 24), ("adh_ema_ctrl", H.EmaCtrl, 16),
                                                 ("adh_adam_tensor", H.AdamTensor, 48), ("adh_grad_ctrl", H.GradCtrl, 32)])
def test_struct_layouts_match_header(struct, mirror, total):
    fields, size = _walk(struct)
    assert [f[0] for f in fields] == [f[0] for f in mirror._fields_]
    for name, ty, off in fields:
        assert getattr(mirror, name).offset == off, name
        assert dict(mirror._fields_)[name] is ty, name
    assert ctypes.sizeof(mirror) == size == total
    if struct == "adh_ema_ctrl":
        assert {"updates", "active", "w"} <= set(dict(mirror._fields_))
        assert dict(mirror._fields_)["w"] is ctypes.c_float and size % 8 == 0


class _Recorder:
    def __init__(self):
        self.calls = []

    def __call__(self, name, *args, **kw):
        assert len(args) == len(H._SIGNATURES[name]) - 1, name        # [0] is the stream
        self.calls.append((name, args))


@pytest.fixture
def recorder(monkeypatch):
    rec = _Recorder()
    monkeypatch.setattr(H, "call", rec)
    monkeypatch.setattr(H, "require_cuda", lambda t, what="input": None)
    return rec


def _params():
    chunk = H.value("adh_adam_chunk_elems")
    a, b = torch.randn(chunk + 5), torch.randn(7)
    a.grad, b.grad = torch.randn(chunk + 5), torch.randn(7)
    return [a, b, a]                      # the first tensor is listed twice


def test_argument_validation(monkeypatch):
    p = torch.zeros(3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        WeightEMA([p])                                        # a CPU tensor
    monkeypatch.setattr(H, "require_cuda", lambda t, what="input": None)
    for bad in (1.0, -0.1, float("nan"), 1.5):
        with pytest.raises(ValueError):
            WeightEMA([p], decay=bad)
    with pytest.raises(ValueError):
        WeightEMA([torch.zeros(3, dtype=torch.int64)])        # nothing to shadow
    for dtype in (torch.float16, torch.bfloat16, torch.float64):
        with pytest.raises(TypeError, match="fp32"):          # the kernels read float*: no other width is shadowed
            WeightEMA([p, torch.zeros(4, dtype=dtype)])
    params = _params()
    ema = WeightEMA(params + [torch.zeros(2, dtype=torch.int64)], decay=0.0)
    assert [id(q) for q in ema.params] == [id(params[0]), id(params[1])], "duplicates collapse, integer tensors are left out"
    assert (ema.decay, ema.warmup) == (0.0, True)
    for p, s in zip(ema.params, ema.shadow):
        assert s.dtype == torch.float32 and s.shape == p.shape and torch.equal(s, p) and s.data_ptr() != p.data_ptr()
    assert ema._ctrl.numel() == ctypes.sizeof(H.EmaCtrl) and ema._ctrl.data_ptr() % 8 == 0
    assert WeightEMA(params).decay == 0.999


def test_update_is_begin_then_multi_and_reads_nothing(recorder, monkeypatch):
    params = _params()
    ema = WeightEMA(params, decay=0.9, warmup=False)
    plain = Adam(params)

    def no_read(*a, **k):
        raise AssertionError("WeightEMA.update read a tensor back to the host")
    with monkeypatch.context() as mp:
        for name in ("item", "tolist", "cpu", "numpy", "__float__", "__int__", "__bool__"):
            mp.setattr(torch.Tensor, name, no_read)
        ema.update()
        ema.update(plain)
    assert [c[0] for c in recorder.calls] == ["adh_ema_begin", "adh_ema_multi"] * 2
    ctrl, table, chunks = ema._ctrl.data_ptr(), ema._table_dev.data_ptr(), ema._chunks_dev.data_ptr()
    for k in range(2):
        assert recorder.calls[2 * k][1] == (ctrl, 0.9, 0, None), "no guard block for a plain optimiser"
        assert recorder.calls[2 * k + 1][1] == (table, chunks, 3, ctrl)
    assert ema.uploads == 1, "no re-upload between two updates with unchanged pointers"
    tab = (H.EmaTensor * 2).from_buffer_copy(ema._table_dev.numpy().tobytes())
    assert [(t.p, t.ema, t.n) for t in tab] == [(p.data_ptr(), s.data_ptr(), p.numel()) for p, s in zip(ema.params, ema.shadow)]
    assert ema._chunks_dev.view(torch.int32).tolist() == [0, 0, 0, 1, 1, 0]


def test_guard_block_of_a_guarded_optimiser(recorder):
    params = _params()
    ema = WeightEMA(params, decay=0.99)
    opt = Adam(params, skip_nonfinite=True)
    ema.update(opt)                                           # before its first step the optimiser has no block yet
    assert recorder.calls[0][1] == (ema._ctrl.data_ptr(), 0.99, 1, None)
    opt.step()
    del recorder.calls[:]
    ema.update(opt)
    assert recorder.calls[0] == ("adh_ema_begin", (ema._ctrl.data_ptr(), 0.99, 1, opt._ctrl.data_ptr()))
    assert opt._ctrl.data_ptr() % 8 == 0


def test_reupload_after_a_storage_change(recorder):
    params = _params()
    ema = WeightEMA(params)
    ema.update()
    ema.update()
    assert ema.uploads == 1
    params[1].data = torch.randn(7)                           # the parameter's storage is replaced
    ema.update()
    assert ema.uploads == 2
    tab = (H.EmaTensor * 2).from_buffer_copy(ema._table_dev.numpy().tobytes())
    assert tab[1].p == params[1].data_ptr()
    assert recorder.calls[-1][1][0] == ema._table_dev.data_ptr()
    ema.update()
    assert ema.uploads == 2


def test_applied_swaps_twice_also_when_the_body_raises(recorder, monkeypatch):
    import adam_dehaze_amd.engine as E
    dropped = []
    monkeypatch.setattr(E, "invalidate_weight_cache", lambda: dropped.append(len(recorder.calls)))
    ema = WeightEMA(_params())
    with ema.applied() as inside:
        assert inside is ema and [c[0] for c in recorder.calls] == ["adh_ema_swap"]
        with pytest.raises(RuntimeError):
            ema.update()
        with pytest.raises(RuntimeError):
            with ema.applied():
                pass
    assert [c[0] for c in recorder.calls] == ["adh_ema_swap"] * 2 and dropped == [1, 2]
    assert recorder.calls[0][1] == (ema._table_dev.data_ptr(), ema._chunks_dev.data_ptr(), 3)
    del recorder.calls[:]
    with pytest.raises(KeyError):
        with ema.applied():
            raise KeyError("body")
    assert [c[0] for c in recorder.calls] == ["adh_ema_swap"] * 2
    ema.update()                                              # usable again
    assert ema.uploads == 1


class _Net(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.conv = torch.nn.Conv2d(2, 2, 1)
        self.bn = torch.nn.BatchNorm2d(2)


def test_state_dict_carries_shadows_and_live_buffers(recorder):
    net = _Net()
    ema = WeightEMA(net.parameters())
    for s in ema.shadow:
        s.add_(1.0)
    net.bn.running_mean.fill_(3.0)
    sd = ema.state_dict(net)
    assert list(sd) == list(net.state_dict())
    for name, p in net.named_parameters():
        assert torch.equal(sd[name], p.detach() + 1.0)
    assert torch.equal(sd["bn.running_mean"], net.bn.running_mean) and "bn.num_batches_tracked" in sd
    sd["conv.weight"].zero_()
    assert not torch.equal(ema.shadow[0], sd["conv.weight"]), "state_dict() hands out clones"
    _Net().load_state_dict(sd)                                # loads wherever a model_state_dict loads
    other = _Net()
    twin = WeightEMA(other.parameters())
    twin.load_state_dict(other, ema.state_dict(net), 41)
    for a, b in zip(twin.shadow, ema.shadow):
        assert torch.equal(a, b)
    assert twin.updates() == 41 and ema.updates() == 0
    twin.reseed()
    assert twin.updates() == 0 and all(torch.equal(s, p) for s, p in zip(twin.shadow, twin.params))


# ------------------------------------------------------------------------------------------------ config plumbing
def test_ema_options():
    assert T.ema_options({}) is None
    assert T.ema_options({"ema": None}) is None
    assert T.ema_options({"ema": {}}) == {"decay": 0.999, "warmup": True, "validate": True, "evaluate": False}
    full = {"decay": 0.99, "warmup": False, "validate": False, "evaluate": True}
    assert T.ema_options({"ema": dict(full)}) == full
    with pytest.raises(ValueError):
        T.ema_options({"ema": {"decay": 0.9, "momentum": 0.1}})
    for not_a_mapping in (True, False, 0.99, "on", ["decay"]):
        with pytest.raises(ValueError, match="mapping"):
            T.ema_options({"ema": not_a_mapping})
    assert T.optim_guard_options({"ema": dict(full)}) == {}, "the two sections do not touch each other"


class _Stop(Exception):
    pass


class _Tiny(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.w = torch.nn.Parameter(torch.zeros(2))


class _TinyRouter(torch.nn.Module):
    def __init__(self, models, classifier):
        super().__init__()
        self.classifier, self.models = classifier, torch.nn.ModuleDict(models)


class _FakeAdam:
    guarded = False

    def __init__(self, params, **kw):
        self.params = list(params)
        self.param_groups = [{"lr": kw.get("lr", 0.0)}]


def _drivers(monkeypatch, tmp_path):
    seen = []

    def ema(params, **kw):
        seen.append((list(params), kw))
        return "the ema"

    def stop(*a, **k):
        raise _Stop
    monkeypatch.setattr(T, "WeightEMA", ema)
    monkeypatch.setattr(T, "Adam", _FakeAdam)
    monkeypatch.setattr(T, "_run_epochs", stop)
    for name in ("create_classifier", "create_low_intensity_model", "create_medium_intensity_model",
                 "create_high_intensity_model", "get_dehazing_loss", "get_joint_loss"):
        monkeypatch.setattr(T, name, lambda config: _Tiny())
    monkeypatch.setattr(T, "create_router", lambda models, classifier, config: _TinyRouter(models, classifier))
    ck = str(tmp_path)
    cfg = {"device": "cpu", "seed": 1, "dataset": {"batch_size": 2, "img_size": 8},
           "classifier": {"checkpoint_dir": ck, "learning_rate": 1e-3, "weight_decay": 1e-4, "epochs": 1},
           "dehazing": {"checkpoint_dir": ck, "low": {"learning_rate": 1e-4}},
           "joint_training": {"learning_rate": 5e-5, "checkpoint_dir": ck, "epochs": 1}}

    def joint(c):
        system = T.build_joint_system(c)
        assert system["ema"] == ("the ema" if c.get("ema") is not None else None)
        raise _Stop

    runs = {"joint": joint, "branch": lambda c: T.train_dehazing_model(c, "low"), "classifier": lambda c: T.train_classifier(c)}
    return seen, cfg, runs


@pytest.mark.filterwarnings("ignore")
@pytest.mark.parametrize("stage", ["joint", "branch", "classifier"])
def test_stages_build_an_ema_only_with_the_section(stage, monkeypatch, tmp_path, capsys):
    seen, cfg, runs = _drivers(monkeypatch, tmp_path)
    for absent in (dict(cfg), {**cfg, "ema": None}):
        with pytest.raises(_Stop):
            runs[stage](absent)
        assert seen == [], "absent section: no WeightEMA"
    with pytest.raises(_Stop):
        runs[stage]({**cfg, "ema": {"decay": 0.9, "warmup": False, "evaluate": True}})
    assert len(seen) == 1 and seen[0][1] == {"decay": 0.9, "warmup": False}
    assert len(seen[0][0]) == (4 if stage == "joint" else 1), "every unique parameter once"
    with pytest.raises(_Stop):
        runs[stage]({**cfg, "ema": {}})
    assert seen[1][1] == {"decay": 0.999, "warmup": True}
    with pytest.raises(ValueError):
        runs[stage]({**cfg, "ema": {"beta": 0.9}})


@pytest.mark.filterwarnings("ignore")
def test_evaluators_build_no_ema(monkeypatch, tmp_path):
    """_joint_system_for_evaluation and evaluate_baseline_models only run the router: no shadow copy, whatever the section says"""
    seen, cfg, _ = _drivers(monkeypatch, tmp_path)
    cfg = {**cfg, "ema": {"decay": 0.9, "evaluate": True}}
    assert T.build_joint_system(cfg, 1, with_ema=False)["ema"] is None and seen == []
    built = []
    real = T.build_joint_system

    def build(*a, **k):
        built.append(real(*a, **k))
        raise _Stop
    monkeypatch.setattr(T, "build_joint_system", build)
    for evaluator in (T._joint_system_for_evaluation, T.evaluate_baseline_models):
        with pytest.raises(_Stop):
            evaluator(cfg)
    assert [b["ema"] for b in built] == [None, None] and seen == []


class _Sched:
    def __init__(self, opt):
        self.opt = opt

    def step(self, metric):
        pass


def _block(t):
    return H.EmaCtrl.from_buffer(t.numpy())       # on the CPU the "device" block is host memory: poke it directly


@pytest.mark.parametrize("guarded", [False, True])
def test_epoch_loop_with_an_ema(recorder, tmp_path, capsys, monkeypatch, guarded):
    """_run_epochs with a WeightEMA: validation inside applied() (two swaps around it), `ema_updates` in the history and on the
    report from ONE read-back together with the guard's statistics, both EMA entries in the checkpoint; without one, today's
    records, lines and checkpoint keys."""
    net = _Net()
    params = list(net.parameters())
    for p in params:
        p.grad = torch.zeros_like(p)
    opt = Adam(params, **({"max_grad_norm": 1.0} if guarded else {}))
    ema = WeightEMA(params, decay=0.9)
    seen = []

    def train_epoch(epoch):
        for _ in range(2):
            opt.step()
            ema.update(opt)
            _block(ema._ctrl).updates += 1          # the recorder launches nothing: play ema_begin_kernel's part

    def validate():
        seen.append([c[0] for c in recorder.calls].count("adh_ema_swap"))
        return {"val_loss": 1.0, "val_psnr": 1.0 + len(seen)}

    def checkpoint(epoch, val):
        return {"epoch": epoch, "model_state_dict": net.state_dict()}

    reads = []
    real = torch.Tensor.tolist
    monkeypatch.setattr(torch.Tensor, "tolist", lambda self: (reads.append(self.numel()), real(self))[1])

    def run(**kw):
        return T._run_epochs(0, 2, train_epoch, validate, _Sched(opt), "val_loss", "val_psnr", 0.0, "{}", str(tmp_path), checkpoint,
                             lambda e, t, v: None, **kw)
    hist = run(ema=ema, ema_model=net)
    assert [h["ema_updates"] for h in hist] == [2, 4]
    assert ("grad_norm_mean" in hist[0]) == guarded
    assert reads == [5 if guarded else 1] * 2, "one read-back per epoch, shared with the guard's statistics"
    assert seen == [1, 3] and [c[0] for c in recorder.calls].count("adh_ema_swap") == 4
    out = capsys.readouterr().out
    assert "EMA updates: 2 (validated on the EMA weights)" in out and "EMA updates: 4" in out
    ck = torch.load(os.path.join(str(tmp_path), "best_model.pth"), map_location="cpu")
    assert sorted(ck) == ["ema_state_dict", "ema_updates", "epoch", "model_state_dict"] and ck["ema_updates"] == 4
    assert list(ck["ema_state_dict"]) == list(ck["model_state_dict"])
    # validate: false -> no swap
    del recorder.calls[:], seen[:]
    run(ema=ema, ema_model=net, ema_validate=False)
    assert "adh_ema_swap" not in [c[0] for c in recorder.calls]
    assert "(validated" not in capsys.readouterr().out
    # no EMA: today's records and checkpoint
    del reads[:]
    hist = run()
    keys = ["epoch", "lr", "train_loss", "val_loss", "val_psnr"]
    assert sorted(hist[0]) == sorted(keys + (["grad_norm_max", "grad_norm_mean", "skipped_steps"] if guarded else []))
    assert reads == ([4, 4] if guarded else [])
    assert "EMA" not in capsys.readouterr().out
    assert sorted(torch.load(os.path.join(str(tmp_path), "best_model.pth"), map_location="cpu")) == ["epoch", "model_state_dict"]


def test_resume_restores_or_reseeds(recorder, capsys):
    net = _Net()
    ema = WeightEMA(net.parameters())
    opt = Adam(list(net.parameters()))
    saved = {k: v + 2.0 if v.is_floating_point() else v for k, v in net.state_dict().items()}
    ck = {"epoch": 3, "ema_state_dict": saved, "ema_updates": 17}
    assert T._restore_training_state(ck, opt, _Sched(opt), None, net, ema=ema) == 4
    assert ema.updates() == 17 and torch.equal(ema.shadow[0], saved["conv.weight"])
    assert "no EMA weights" not in capsys.readouterr().out
    assert T._restore_training_state({"epoch": 0}, opt, _Sched(opt), None, net, ema=ema) == 1
    assert ema.updates() == 0 and torch.equal(ema.shadow[0], net.conv.weight.detach())
    assert capsys.readouterr().out.count("Checkpoint has no EMA weights: the EMA starts from the loaded weights") == 1
    assert T._restore_training_state({"epoch": 0}, opt, _Sched(opt), None, net) == 1
    assert capsys.readouterr().out == ""


def test_load_pretrained_model_prefers_ema_on_request(tmp_path, capsys):
    net = _Net()
    raw = net.state_dict()
    shadow = {k: v + 1.0 if v.is_floating_point() else v for k, v in raw.items()}
    both, only_raw = str(tmp_path / "both.pth"), str(tmp_path / "raw.pth")
    torch.save({"model_state_dict": raw, "ema_state_dict": shadow, "ema_updates": 3}, both)
    torch.save({"model_state_dict": raw}, only_raw)
    a, b, c = _Net(), _Net(), _Net()
    assert T.load_pretrained_model(a, both) and torch.equal(a.conv.weight, raw["conv.weight"])
    assert capsys.readouterr().out == f"Loaded pretrained weights from {both}\n", "the default call: today's load and line"
    assert T.load_pretrained_model(b, both, prefer_ema=True) and torch.equal(b.conv.weight, shadow["conv.weight"])
    assert "Loaded EMA weights from" in capsys.readouterr().out
    assert T.load_pretrained_model(c, only_raw, prefer_ema=True) and torch.equal(c.conv.weight, raw["conv.weight"])
    assert "Loaded pretrained weights from" in capsys.readouterr().out
    assert not T.load_pretrained_model(c, str(tmp_path / "missing.pth"), prefer_ema=True)


def _commented_block(lines, head):
    block = []
    for line in lines[lines.index(head):]:
        if not line.startswith("#"):
            break
        block.append(line[2:] if line.startswith("# ") else line[1:])
    return block


def test_commented_blocks_of_config_parse():
    import yaml
    text = open(os.path.join(ROOT, "config", "config.yaml")).read()
    lines = text.splitlines()
    assert "ema" not in yaml.safe_load(text), "the section is commented out by default"
    cfg = yaml.safe_load(text + "\n" + "\n".join(_commented_block(lines, "# ema:")) + "\n")
    assert set(cfg["ema"]) == {"decay", "warmup", "validate", "evaluate"} and "optim" not in cfg
    opts = T.ema_options(cfg)
    assert opts == {"decay": float(cfg["ema"]["decay"]), "warmup": True, "validate": True, "evaluate": False}, \
        "the block spells out the defaults"
    cfg = yaml.safe_load(text + "\n" + "\n".join(_commented_block(lines, "# optim:")) + "\n")
    assert set(cfg["optim"]) == {"grad_clip_norm", "skip_nonfinite"} and "ema" not in cfg
