"""Host side of the gradient guard (optim.Adam(max_grad_norm, skip_nonfinite), the `optim:` config section), without a GPU:
the C ABI and its ctypes mirror, argument validation, the launches `Adam.step` issues (recorded, as tests/_launch_trace.py
records the engine's: `_hip.call` is replaced by a recorder that launches nothing), the config plumbing of the three training
stages and the commented block of config/config.yaml."""
import ctypes
import os
import re

import pytest
import torch

from adam_dehaze_amd import _hip as H
from adam_dehaze_amd import train as T
from adam_dehaze_amd.optim import Adam

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("adh_grad_sumsq", "adh_grad_guard_finalize", "adh_adam_multi_guarded")


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
    assert H._SIGNATURES["adh_adam_multi_guarded"][:-1] == \
        H._SIGNATURES["adh_adam_multi"][:9] + H._SIGNATURES["adh_adam_multi"][10:], "adh_adam_multi minus grad_scale, plus ctrl"


def test_control_block_layout_matches_header():
    body = re.search(r"typedef struct adh_grad_ctrl \{(.*?)\} adh_grad_ctrl;", _header(), flags=re.S).group(1)
    size = {"double": 8, "float": 4, "int32_t": 4}
    ctype = {"double": ctypes.c_double, "float": ctypes.c_float, "int32_t": ctypes.c_int32}
    offset, align, fields = 0, 1, []
    for decl in (d.strip() for d in body.split(";")):
        if not decl:
            continue
        ty, name = decl.split()
        offset = (offset + size[ty] - 1) // size[ty] * size[ty]       # the C layout rule for these scalar types
        fields.append((name, ctype[ty], offset))
        offset += size[ty]
        align = max(align, size[ty])
    total = (offset + align - 1) // align * align
    assert [f[0] for f in fields] == [f[0] for f in H.GradCtrl._fields_]
    for name, ty, off in fields:
        assert getattr(H.GradCtrl, name).offset == off, name
        assert dict(H.GradCtrl._fields_)[name] is ty, name
    assert ctypes.sizeof(H.GradCtrl) == total == 32
    for name in ("sumsq", "norm", "gscale_eff", "finite", "skipped", "skipped_total"):
        assert name in dict(H.GradCtrl._fields_)


def test_adam_argument_validation():
    p = torch.zeros(3)
    for bad in (-1.0, -1e-9, float("nan"), float("-inf")):
        with pytest.raises(ValueError):
            Adam([p], max_grad_norm=bad)
    with pytest.raises(ValueError):
        Adam([p], duplicates="both", max_grad_norm=1.0)
    assert not Adam([p]).guarded
    assert not Adam([p], max_grad_norm=None, skip_nonfinite=False).guarded
    for kw in (dict(max_grad_norm=0.0), dict(max_grad_norm=float("inf")), dict(max_grad_norm=2), dict(skip_nonfinite=True)):
        opt = Adam([p], **kw)
        assert opt.guarded and opt.last_grad_norm is None and opt.skipped_steps() == 0


class _Recorder:
    def __init__(self):
        self.calls = []

    def __call__(self, name, *args, **kw):
        assert len(args) == len(H._SIGNATURES[name]) - 1, name        # [0] is the stream
        self.calls.append((name, args))


def _params():
    chunk = H.value("adh_adam_chunk_elems")
    a, b = torch.randn(chunk + 5), torch.randn(7)
    a.grad, b.grad = torch.randn(chunk + 5), torch.randn(7)
    return [a, b, a]                      # the first tensor is listed twice


@pytest.fixture
def recorder(monkeypatch):
    rec = _Recorder()
    monkeypatch.setattr(H, "call", rec)
    monkeypatch.setattr(H, "require_cuda", lambda t, what="input": None)
    return rec


def test_step_without_the_options_is_the_one_adam_launch(recorder):
    params = _params()
    opt = Adam(params, lr=1e-3, weight_decay=1e-4)
    opt.grad_scale = 0.5
    for k in range(3):
        opt.step()
    assert [c[0] for c in recorder.calls] == ["adh_adam_multi"] * 3
    st = opt.state
    for k, (_, args) in enumerate(recorder.calls):
        table, chunks, nchunks, lr, b1, b2, eps, wd, gscale, dup_mode, max_repeats, csu = args
        assert (table, chunks) == (opt._table_dev.data_ptr(), opt._chunks_dev.data_ptr())
        assert (nchunks, lr, b1, b2, eps, wd, gscale, dup_mode, max_repeats, csu) == (3, 1e-3, 0.9, 0.999, 1e-8, 1e-4, 0.5, 0, 2, k)
    assert st[id(params[0])]["step"] == 6 and st[id(params[1])]["step"] == 3
    assert opt._ctrl is None and opt._partials is None and opt.last_grad_norm is None
    table = (H.AdamTensor * 2).from_buffer_copy(opt._table_dev.numpy().tobytes())
    assert [(t.n, t.step, t.repeats) for t in table] == [(params[0].numel(), 0, 2), (7, 0, 1)]
    assert (table[0].p, table[0].g) == (params[0].data_ptr(), params[0].grad.data_ptr())


def test_step_with_the_options_is_three_launches_and_no_host_read(recorder, monkeypatch):
    params = _params()
    opt = Adam(params, lr=1e-3, weight_decay=1e-4, duplicates="foreach", max_grad_norm=2.5, skip_nonfinite=True)
    opt.grad_scale = 0.5

    def no_read(*a, **k):
        raise AssertionError("Adam.step read a tensor back to the host")
    hooked = []
    opt.step_hook = lambda: hooked.append(len(recorder.calls))
    with monkeypatch.context() as mp:
        for name in ("item", "tolist", "cpu", "numpy", "__float__", "__int__", "__bool__"):
            mp.setattr(torch.Tensor, name, no_read)
        for k in range(2):
            opt.step()
    assert [c[0] for c in recorder.calls] == list(NEW) * 2
    assert hooked == [3, 6]
    table, chunks, ctrl, part = (opt._table_dev.data_ptr(), opt._chunks_dev.data_ptr(), opt._ctrl.data_ptr(),
                                 opt._partials.data_ptr())
    assert opt._partials.dtype == torch.float64 and opt._partials.numel() == 3
    assert opt._ctrl.numel() == ctypes.sizeof(H.GradCtrl) and ctrl % 8 == 0
    for k in range(2):
        s, f, a = (c[1] for c in recorder.calls[3 * k:3 * k + 3])
        assert s == (table, chunks, 3, 0.5, part)
        assert f == (part, 3, 0.5, 2.5, 1, ctrl)
        assert a == (table, chunks, 3, 1e-3, 0.9, 0.999, 1e-8, 1e-4, 1, 2, k, ctrl)
    assert opt.last_grad_norm.dim() == 0 and opt.last_grad_norm.dtype == torch.float32
    assert opt.last_grad_norm.data_ptr() == ctrl + H.GradCtrl.norm.offset
    assert opt.skipped_total.data_ptr() == ctrl + H.GradCtrl.skipped_total.offset


def test_measure_only_and_skip_only_arguments(recorder):
    opt = Adam(_params(), skip_nonfinite=True)
    opt.step()
    assert recorder.calls[1][1][3:5] == (0.0, 1), "no max_grad_norm: max_norm 0 (measure only), skip on"
    del recorder.calls[:]
    opt = Adam(_params(), max_grad_norm=float("inf"))
    opt.step()
    assert recorder.calls[1][1][3:5] == (float("inf"), 0)


def _block(opt):
    return H.GradCtrl.from_buffer(opt._ctrl.numpy())       # on the CPU the "device" block is host memory: poke it directly


def test_reconcile_takes_skipped_steps_back(recorder):
    """The recorder launches nothing, so the test plays the kernel: it bumps the block's counters after a step."""
    params = _params()
    opt = Adam(params, skip_nonfinite=True)
    for k in range(3):
        opt.step()
        if k == 1:
            blk = _block(opt)
            blk.skipped += 1
            blk.skipped_total += 1
    assert opt.state[id(params[0])]["step"] == 6 and opt._calls_since_upload == 3      # optimistic
    sd = opt.state_dict()
    assert float(sd["state"][2]["step"]) == 4 and float(sd["state"][1]["step"]) == 2   # the duplicate packs under index 2
    assert _block(opt).skipped == 0 and _block(opt).skipped_total == 1 and opt.skipped_steps() == 1
    assert opt._table_key is None
    del recorder.calls[:]
    opt.step()                                      # re-upload with the reconciled counts
    assert recorder.calls[2][1][-2] == 0
    table = (H.AdamTensor * 2).from_buffer_copy(opt._table_dev.numpy().tobytes())
    assert [t.step for t in table] == [4, 2]
    # a changed gradient pointer re-uploads too, and reconciles first
    blk = _block(opt)
    blk.skipped += 1
    blk.skipped_total += 1
    params[1].grad = torch.randn(7)
    opt.step()
    assert opt.state[id(params[0])]["step"] == 6 and opt.state[id(params[1])]["step"] == 3
    assert opt._calls_since_upload == 1 and _block(opt).skipped == 0
    fresh = Adam(params, skip_nonfinite=True)
    fresh.step()
    _block(fresh).skipped_total = 5
    fresh.load_state_dict(sd)
    assert bytes(fresh._ctrl.numpy()) == bytes(32) and fresh.skipped_steps() == 0
    assert fresh.state[id(params[0])]["step"] == 4


# ------------------------------------------------------------------------------------------------ config plumbing
def test_optim_guard_options():
    assert T.optim_guard_options({}) == {}
    assert T.optim_guard_options({"optim": None}) == {}
    assert T.optim_guard_options({"optim": {"grad_clip_norm": 1}}) == {"max_grad_norm": 1.0}
    assert T.optim_guard_options({"optim": {"skip_nonfinite": True}}) == {"skip_nonfinite": True}
    assert T.optim_guard_options({"optim": {"skip_nonfinite": False}}) == {}
    assert T.optim_guard_options({"optim": {"grad_clip_norm": 0.5, "skip_nonfinite": True}}) == \
        {"max_grad_norm": 0.5, "skip_nonfinite": True}
    with pytest.raises(ValueError):
        T.optim_guard_options({"optim": {"clip": 1.0}})


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


def _drivers(monkeypatch, tmp_path):
    seen = []

    def adam(params, **kw):
        seen.append(kw)
        raise _Stop

    monkeypatch.setattr(T, "Adam", adam)
    for name in ("create_classifier", "create_low_intensity_model", "create_medium_intensity_model",
                 "create_high_intensity_model", "get_dehazing_loss", "get_joint_loss"):
        monkeypatch.setattr(T, name, lambda config: _Tiny())
    monkeypatch.setattr(T, "create_router", lambda models, classifier, config: _TinyRouter(models, classifier))
    ck = str(tmp_path)
    cfg = {"device": "cpu", "seed": 1, "dataset": {"batch_size": 2, "img_size": 8},
           "classifier": {"checkpoint_dir": ck, "learning_rate": 1e-3, "weight_decay": 1e-4, "epochs": 1},
           "dehazing": {"checkpoint_dir": ck, "low": {"learning_rate": 1e-4}},
           "joint_training": {"learning_rate": 5e-5, "checkpoint_dir": ck, "epochs": 1}}
    runs = {"joint": lambda c: T.build_joint_system(c), "branch": lambda c: T.train_dehazing_model(c, "low"),
            "classifier": lambda c: T.train_classifier(c)}
    return seen, cfg, runs


@pytest.mark.parametrize("stage", ["joint", "branch", "classifier"])
def test_config_reaches_the_optimiser_of_every_stage(stage, monkeypatch, tmp_path, capsys):
    seen, cfg, runs = _drivers(monkeypatch, tmp_path)
    with pytest.raises(_Stop):
        runs[stage](dict(cfg))
    assert "max_grad_norm" not in seen[-1] and "skip_nonfinite" not in seen[-1], "absent section: today's constructor call"
    with pytest.raises(_Stop):
        runs[stage]({**cfg, "optim": {"grad_clip_norm": 0.75, "skip_nonfinite": True}})
    assert seen[-1]["max_grad_norm"] == 0.75 and seen[-1]["skip_nonfinite"] is True
    with pytest.raises(_Stop):
        runs[stage]({**cfg, "optim": {"skip_nonfinite": True}})
    assert "max_grad_norm" not in seen[-1] and seen[-1]["skip_nonfinite"] is True


class _Sched:
    def __init__(self, opt):
        self.opt = opt

    def step(self, metric):
        pass


def test_epoch_loop_reports_norm_and_skips(recorder, tmp_path, capsys):
    """_run_epochs with a guarded optimiser: mean and max of last_grad_norm over the epoch's finite steps and the skip count, in
    the history and on the report; with an unguarded one the records keep today's keys."""
    params = _params()
    opt = Adam(params, max_grad_norm=1.0, skip_nonfinite=True)
    opt.step()                                          # allocates the block
    norms = iter([3.0, float("inf"), 5.0, 2.0])

    def train_epoch(epoch):
        for _ in range(1 if epoch else 3):
            blk, norm = _block(opt), next(norms)        # the recorder launches nothing: play finalize_kernel's part
            blk.norm = norm
            if norm == float("inf"):
                blk.skipped_total += 1
            opt.step()

    def run(optimizer, te):
        return T._run_epochs(0, 2, te, lambda: {"val_loss": 1.0, "val_psnr": 0.0}, _Sched(optimizer), "val_loss", "val_psnr", 1.0,
                             "{}", str(tmp_path), lambda e, v: {}, lambda e, t, v: None)
    hist = run(opt, train_epoch)
    assert (hist[0]["grad_norm_mean"], hist[0]["grad_norm_max"], hist[0]["skipped_steps"]) == (4.0, 5.0, 1)
    assert (hist[1]["grad_norm_mean"], hist[1]["grad_norm_max"], hist[1]["skipped_steps"]) == (2.0, 2.0, 0)
    out = capsys.readouterr().out
    assert "Grad norm: mean 4.0000, max 5.0000; skipped steps: 1" in out
    assert opt.step_hook is None, "the loop takes its hook off again"
    plain = Adam(_params())
    hist = run(plain, lambda epoch: plain.step())
    assert sorted(hist[0]) == ["epoch", "lr", "train_loss", "val_loss", "val_psnr"]
    assert "Grad norm" not in capsys.readouterr().out


def test_commented_optim_block_of_config_parses():
    import yaml
    text = open(os.path.join(ROOT, "config", "config.yaml")).read()
    lines = text.splitlines()
    start = lines.index("# optim:")
    block = []
    for line in lines[start:]:
        if not line.startswith("#"):
            break
        block.append(line[2:] if line.startswith("# ") else line[1:])
    assert "optim" not in yaml.safe_load(text), "the section is commented out by default"
    cfg = yaml.safe_load(text + "\n" + "\n".join(block) + "\n")
    assert set(cfg["optim"]) == {"grad_clip_norm", "skip_nonfinite"}
    opts = T.optim_guard_options(cfg)
    assert opts == {"max_grad_norm": float(cfg["optim"]["grad_clip_norm"]), "skip_nonfinite": True}
    Adam([torch.zeros(2)], **opts)
