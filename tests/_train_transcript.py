"""Transcript of the training and evaluation drivers of adam_dehaze_amd/train.py, taken on the CPU.

The models, the criteria, the optimiser, the metric kernels and the synthetic loader are replaced by tiny CPU stand-ins; the
drivers themselves (`train_dehazing_model`, `train_joint_model`, `train_classifier`, `evaluate_classifier` and the preambles
of the three evaluators) run as they are, single-process and as two gloo ranks.  Only seams that survive a rewrite of
train.py are hooked:

  * the module-level names of train.py: `Adam`, `synthetic_loader`, `psnr_batch`, `ssim_batch`, `get_dehazing_loss`,
    `get_joint_loss`, `create_classifier`, `create_{low,medium,high}_intensity_model`, `create_router`, the `step` of its
    `ReduceLROnPlateau`, plus `adam_dehaze_amd.loss.cross_entropy3` and `adam_dehaze_amd.detection.create_detection_model`;
  * `torch.save`, `torch.load`, `os.replace`;
  * the `torch.distributed` collectives (`all_reduce`, `broadcast`, `barrier`, `monitored_barrier`, `all_gather*`,
    `new_group`);
  * `sys.stdout` and `warnings.showwarning`.

One case records, per rank and in order of occurrence:

    ["out", line]                                   every stdout line
    ["warn", text]                                  every warning
    ["loader", batch, size, steps, seed, rank]      every synthetic_loader call
    ["fwd", model, module.training, batch size]     every model forward
    ["coll", name, shape, dtype]                    every collective (shape / dtype of its first tensor, None without one)
    ["save", file, keys, epoch, {val_*}, state]     every torch.save: basename without the `.tmp.<pid>` suffix, sorted keys,
                                                    the val_* entries, the numbers of every *state_dict entry but the
                                                    optimiser's, and the optimiser's step count
    ["replace", from, to]                           every os.replace (basenames)
    ["load", path]                                  every torch.load
    ["sched", metric, lr]                           every scheduler step: its metric and the learning rate after it
    ["raise", type, message]                        the exception a driver ended with
    ["return", value]                               what the driver returned (see the runners)
    ["modes", {module: training}]                   evaluators: the mode every module the factories made was left in

The case's temporary directory reads <TMP> wherever it appears.  The stand-in arithmetic is exact: inputs, weights and the
optimiser's moves are small multiples of powers of two, sums are scaled by powers of two and nothing takes a logarithm, so
the numbers depend neither on the order of a summation nor on the CPU.

tests/golden/train_drivers.json holds the transcript of every case in CASES.  It is regenerated with

    python -m tests._train_transcript --regen

from the repository root -- and only from a train.py whose drivers are known to be right: the golden is what a change to
the epoch loop, the resume path or the evaluators' preambles is compared against.
"""
import json
import os
import re
import shutil
import sys
import tempfile
import warnings

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

GOLDEN_PATH = os.path.join(ROOT, "tests", "golden", "train_drivers.json")
STEP = 1.0 / 64          # what the optimiser stand-in moves a parameter by
COLLECTIVES = ["all_reduce", "broadcast", "barrier", "monitored_barrier", "new_group"] + \
    sorted(n for n in dir(dist) if n.startswith("all_gather"))


# ---------------------------------------------------------------------------------------------------------------------
# stand-ins
# ---------------------------------------------------------------------------------------------------------------------
class Branch(torch.nn.Module):
    """x -> x * w.  Owns a BatchNorm2d it never normalises with: a train-mode forward adds the batch's first pixel to its
    running mean, so the buffers of two ranks drift apart with their data, as replica-BN statistics do."""

    def __init__(self, rec, name, w):
        super().__init__()
        self.rec, self.name = [rec], name        # (in a list: not a submodule, not in the state_dict)
        self.w = torch.nn.Parameter(torch.tensor(w))
        self.bn = torch.nn.BatchNorm2d(4)

    def forward(self, x):
        self.rec[0].event("fwd", self.name, self.training, x.shape[0])
        if self.training:
            with torch.no_grad():
                self.bn.running_mean += x[0, 0, 0, 0]
                self.bn.num_batches_tracked += 1
        return x * self.w


class Classifier(Branch):
    """x -> (the first pixel of the first three channels * w, None)"""

    def forward(self, x):
        return super().forward(x)[:, :3, 0, 0], None


class Router(torch.nn.Module):
    """(x, logits) -> (a quarter of the sum of the three branches, {}); holds the classifier and the branches."""

    def __init__(self, rec, models, classifier):
        super().__init__()
        self.rec = [rec]
        self.models, self.classifier = torch.nn.ModuleDict(models), classifier

    def forward(self, x, logits=None):
        self.rec[0].event("fwd", "router", self.training, x.shape[0])
        return sum(m(x) for m in self.models.values()) * 0.25, {}


def _l1(out, target):
    return (out - target).abs().sum() * 0.0625


def cross_entropy3(logits, labels):
    """not a cross-entropy: a quarter of the squared distance to the one-hot labels, which needs no exp / log"""
    return ((logits - torch.nn.functional.one_hot(labels, 3).to(logits.dtype)) ** 2).sum() * 0.25


class DehazingLoss(torch.nn.Module):
    def forward(self, out, target):
        l1 = _l1(out, target)
        return l1, {"l1": l1, "content": l1 * 0, "perceptual": l1 * 2, "total": l1}


class JointLoss(torch.nn.Module):
    def forward(self, dehazed, clear, logits, labels):
        d, c = _l1(dehazed, clear), cross_entropy3(logits, labels)
        return d + 0.25 * c, {"dehazing": d, "classification": c, "dehazing_components": {}}


class FixedStep:
    """The optimiser: `step` moves every listed parameter that has a gradient down by STEP (a parameter listed twice, as the
    joint stage lists the branches, moves twice)."""

    def __init__(self, params, lr=1e-3, weight_decay=0.0, **kw):
        self.listed = list(params)
        self.param_groups = [{"lr": lr, "weight_decay": weight_decay}]
        self.steps = 0

    def zero_grad(self):
        for p in self.listed:
            p.grad = None

    def step(self):
        self.steps += 1
        with torch.no_grad():
            for p in self.listed:
                if p.grad is not None:
                    p -= STEP

    def state_dict(self):
        return {"steps": self.steps, "lr": self.param_groups[0]["lr"]}

    def load_state_dict(self, sd):
        self.steps, self.param_groups[0]["lr"] = sd["steps"], sd["lr"]


def psnr_batch(a, b):
    return 40.0 - ((a - b) ** 2).sum(dim=(1, 2, 3))


def ssim_batch(a, b):
    return 1.0 - (a - b).abs().sum(dim=(1, 2, 3)) * 0.0625


def mixed_labels(seed, rank, step, i):
    return (seed + step + i) % 3


def rank1_never_medium(seed, rank, step, i):
    return (seed + step + i) % 3 if rank == 0 else 2 * ((seed + step + i) % 2)


def nobody_medium(seed, rank, step, i):
    return 2 * ((seed + step + i + rank) % 2)


# ---------------------------------------------------------------------------------------------------------------------
# recorder
# ---------------------------------------------------------------------------------------------------------------------
class _Stdout:
    def __init__(self, rec):
        self.rec, self.partial = rec, ""

    def write(self, s):
        *lines, self.partial = (self.partial + s).split("\n")
        for ln in lines:
            self.rec.event("out", ln)
        return len(s)

    def flush(self):
        pass


def _numbers(sd):
    """the entries of a state_dict that can change: the weights, the running means and the batch counts"""
    return {k: [float(x) for x in v.reshape(-1).tolist()] for k, v in sd.items()
            if not k.endswith(("bn.weight", "bn.bias", "bn.running_var"))}


class Recorder:
    def __init__(self, tmp, labels=mixed_labels):
        self.tmp, self.labels = tmp, labels
        self.events = []
        self.made = []          # (name, module) of everything the factories made, in order

    def clean(self, v):
        """JSON-able, with the temporary directory and the pid of a temporary file name taken out"""
        if isinstance(v, str):
            return re.sub(r"\.tmp\.\d+", "", v.replace(self.tmp, "<TMP>"))
        if isinstance(v, dict):
            return {str(k): self.clean(x) for k, x in v.items()}
        if isinstance(v, (list, tuple)):
            return [self.clean(x) for x in v]
        if isinstance(v, torch.Tensor):
            return v.tolist()
        if hasattr(v, "tolist"):        # numpy
            return v.tolist()
        return v

    def event(self, *ev):
        self.events.append(self.clean(ev))

    # ------------------------------------------------------------------ the seams
    def _make(self, cls, name, *a):
        m = cls(self, name, *a)
        self.made.append((name, m))
        return m

    def _router(self, models, classifier, config):
        m = Router(self, models, classifier)
        self.made.append(("router", m))
        return m

    def _loader(self, batch_size, size, steps, seed=42, rank=0, device=None, augment=False):
        self.event("loader", batch_size, size, steps, seed, rank)

        def batches():
            for step in range(steps):
                labels = torch.tensor([self.labels(seed, rank, step, i) for i in range(batch_size)], dtype=torch.int64)
                level = torch.tensor([(1 + (seed + 3 * step + i + rank) % 7) / 8 for i in range(batch_size)])
                hazy = level.reshape(-1, 1, 1, 1).repeat(1, 4, size, size)
                hazy[torch.arange(batch_size), labels] += 0.125
                yield {"hazy": hazy, "clear": hazy * 0.5, "intensity": labels,
                       "name": [f"synthetic_{i}" for i in range(batch_size)]}
        return batches()

    def _save(self, real):
        def save(obj, path, *a, **k):
            state = {key: _numbers(v) for key, v in obj.items()
                     if key.endswith("state_dict") and key not in ("optimizer_state_dict", "scheduler_state_dict")}
            self.event("save", os.path.basename(str(path)), sorted(obj), obj.get("epoch"),
                       {key: v for key, v in obj.items() if key.startswith("val_")}, state,
                       obj.get("optimizer_state_dict", {}).get("steps"))
            return real(obj, path, *a, **k)
        return save

    def _load(self, real):
        def load(path, *a, **k):
            self.event("load", str(path))
            return real(path, *a, **k)
        return load

    def _replace(self, real):
        def replace(src, dst, *a, **k):
            self.event("replace", os.path.basename(str(src)), os.path.basename(str(dst)))
            return real(src, dst, *a, **k)
        return replace

    def _collective(self, name, real):
        def collective(*a, **k):
            t = next((x for x in list(a) + list(k.values()) if isinstance(x, torch.Tensor)), None)
            self.event("coll", name, None if t is None else list(t.shape), None if t is None else str(t.dtype))
            return real(*a, **k)
        return collective

    def _sched_step(self, real):
        def step(sched, metric):
            real(sched, metric)
            self.event("sched", metric, sched.opt.param_groups[0]["lr"])
        return step

    def install(self, mp_):
        """`mp_` is a pytest MonkeyPatch"""
        import adam_dehaze_amd.detection as D
        import adam_dehaze_amd.loss as L
        import adam_dehaze_amd.train as T
        for k in ("WORLD_SIZE", "RANK", "ADH_SYNC_BN", "ADH_DIST_FORCE"):
            if not (dist.is_initialized() and k in ("WORLD_SIZE", "RANK")):
                mp_.delenv(k, raising=False)
        mp_.setattr(T, "Adam", FixedStep)
        mp_.setattr(T, "synthetic_loader", self._loader)
        mp_.setattr(T, "psnr_batch", psnr_batch)
        mp_.setattr(T, "ssim_batch", ssim_batch)
        mp_.setattr(T, "get_dehazing_loss", lambda config: DehazingLoss())
        mp_.setattr(T, "get_joint_loss", lambda config: JointLoss())
        mp_.setattr(T, "create_classifier", lambda config: self._make(Classifier, "classifier", 1.0))
        mp_.setattr(T, "create_low_intensity_model", lambda config: self._make(Branch, "low", 0.5))
        mp_.setattr(T, "create_medium_intensity_model", lambda config: self._make(Branch, "medium", 0.5 + 3 * STEP))
        mp_.setattr(T, "create_high_intensity_model", lambda config: self._make(Branch, "high", 0.5 + 57 * STEP))
        mp_.setattr(T, "create_router", self._router)
        mp_.setattr(T.ReduceLROnPlateau, "step", self._sched_step(T.ReduceLROnPlateau.step))
        mp_.setattr(L, "cross_entropy3", cross_entropy3)
        mp_.setattr(D, "create_detection_model", lambda config: self._make(Branch, "detector", 1.0))
        mp_.setattr(torch, "save", self._save(torch.save))
        mp_.setattr(torch, "load", self._load(torch.load))
        mp_.setattr(os, "replace", self._replace(os.replace))
        for name in COLLECTIVES:
            mp_.setattr(dist, name, self._collective(name, getattr(dist, name)))
        mp_.setattr(sys, "stdout", _Stdout(self))

    def run(self, what, fn, *a, **k):
        """One driver call: its output, warnings, exception or return value go into the transcript."""
        with warnings.catch_warnings():
            warnings.simplefilter("always")
            warnings.showwarning = lambda message, *rest, **kw: self.event("warn", str(message))
            self.event("call", what)
            try:
                return fn(*a, **k)
            except (ValueError, RuntimeError, FileNotFoundError) as e:
                self.event("raise", type(e).__name__, str(e))
                return None


def config(tmp):
    return {"device": "cpu", "seed": 42, "dataset": {"batch_size": 4, "img_size": 2, "test_path": os.path.join(tmp, "data")},
            "classifier": {"checkpoint_dir": os.path.join(tmp, "classifier"), "learning_rate": 0.25, "weight_decay": 0.0,
                           "epochs": 5},
            "dehazing": {"checkpoint_dir": os.path.join(tmp, "dehazing"), "low": {"learning_rate": 0.5},
                         "medium": {"learning_rate": 0.5}, "high": {"learning_rate": 0.5}},
            "routing": {"type": "soft"},
            "joint_training": {"checkpoint_dir": os.path.join(tmp, "joint"), "learning_rate": 0.125, "epochs": 5},
            "detection": {"model": "stand-in", "pretrained": False, "checkpoint_dir": os.path.join(tmp, "detection")},
            "evaluation": {"results_dir": os.path.join(tmp, "results")}}


# ---------------------------------------------------------------------------------------------------------------------
# runners: (recorder, train module, config) -> None
# ---------------------------------------------------------------------------------------------------------------------
def _branch(rec, T, cfg, what, **kw):
    out = rec.run(what, T.train_dehazing_model, cfg, "medium", **kw)
    if out is not None:
        rec.event("return", out[1], _numbers(out[0].state_dict()))


def _joint(rec, T, cfg, what, **kw):
    out = rec.run(what, T.train_joint_model, cfg, **kw)
    if out is not None:
        rec.event("return", out[1], _numbers(out[0]["router"].state_dict()))


def branch_then_resume(rec, T, cfg):
    _branch(rec, T, cfg, "6 epochs", steps=2, epochs=6, val_steps=1)
    _branch(rec, T, cfg, "resume to 7", steps=2, epochs=7, val_steps=1, resume=True)


def branch_refuses_other_checkpoints(rec, T, cfg):
    _joint(rec, T, cfg, "a joint checkpoint", steps_per_epoch=1, epochs=1, val_steps=1)
    cfg["dehazing"]["checkpoint_dir"] = cfg["joint_training"]["checkpoint_dir"]      # <joint>/medium: nothing there
    _branch(rec, T, cfg, "resume: nothing there", resume=True)
    _branch(rec, T, cfg, "resume: a joint checkpoint", resume=os.path.join(cfg["joint_training"]["checkpoint_dir"], "best_model.pth"))
    other = os.path.join(rec.tmp, "other.pth")
    sd = Branch(rec, "other", 0.0).state_dict()
    sd["extra"] = sd.pop("w")
    torch.save({"epoch": 0, "model_state_dict": sd}, other)
    _branch(rec, T, cfg, "resume: another branch's checkpoint", resume=other)


def joint_then_resume(rec, T, cfg):
    _joint(rec, T, cfg, "5 epochs", steps_per_epoch=2, val_steps=1)
    _joint(rec, T, cfg, "resume to 6", steps_per_epoch=2, val_steps=1, epochs=6, resume=True)


def joint_refuses_branch_checkpoint(rec, T, cfg):
    _branch(rec, T, cfg, "a branch checkpoint", steps=1, epochs=1, val_steps=1)
    _joint(rec, T, cfg, "resume: a branch checkpoint",
           resume=os.path.join(cfg["dehazing"]["checkpoint_dir"], "medium", "best_model.pth"))


def classifier_then_evaluate(rec, T, cfg):
    model = rec.run("5 epochs", T.train_classifier, cfg, steps=2, val_steps=1)
    rec.event("return", _numbers(model.state_dict()))
    rec.event("return", rec.run("evaluate", T.evaluate_classifier, model, cfg, steps=1))
    rec.event("modes", {"classifier": model.training})


def classifier_refuses_world2(rec, T, cfg):
    os.environ["WORLD_SIZE"] = "2"      # (the case's MonkeyPatch took the variable out and puts back what was there)
    try:
        rec.run("WORLD_SIZE=2", T.train_classifier, cfg, steps=1, epochs=1)
    finally:
        del os.environ["WORLD_SIZE"]


def _checkpoints(rec, cfg):
    """what the training stages leave behind, written by hand: every weight 0.25"""
    def sd(m):
        return {k: torch.full_like(v, 0.25) if v.is_floating_point() else v for k, v in m.state_dict().items()}
    silent = Recorder(rec.tmp)
    branches = {n: Branch(silent, n, 0.0) for n in ("low", "medium", "high")}
    for n, m in branches.items():
        os.makedirs(os.path.join(cfg["dehazing"]["checkpoint_dir"], n))
        torch.save({"epoch": 0, "model_state_dict": sd(m)}, os.path.join(cfg["dehazing"]["checkpoint_dir"], n, "best_model.pth"))
    for key in ("classifier", "detection"):
        os.makedirs(cfg[key]["checkpoint_dir"])
        torch.save({"epoch": 0, "model_state_dict": sd(branches["low"])}, os.path.join(cfg[key]["checkpoint_dir"], "best_model.pth"))
    os.makedirs(cfg["joint_training"]["checkpoint_dir"])
    router = Router(silent, branches, Classifier(silent, "classifier", 0.0))
    torch.save({"epoch": 0, "router_state_dict": {k: v * 2 if v.is_floating_point() else v for k, v in sd(router).items()}},
               os.path.join(cfg["joint_training"]["checkpoint_dir"], "best_model.pth"))


def evaluators(with_checkpoints):
    """The preambles: no batch goes through (steps=0), so the bodies below them see an empty loader."""
    def run(rec, T, cfg):
        if with_checkpoints:
            _checkpoints(rec, cfg)
        for what, fn, kw in (("joint", T.evaluate_joint_model, dict(use_lpips=False)),
                             ("baseline", T.evaluate_baseline_models, dict(use_lpips=False)),
                             ("detection", T.evaluate_detection, {})):
            rec.made = []
            rec.event("return", rec.run(what, fn, cfg, steps=0, **kw))
            rec.event("modes", {name: m.training for name, m in rec.made})
            rec.event("weights", {name: _numbers(m.state_dict())["w"] for name, m in rec.made if name != "router"})
    return run


def ddp_branch(rec, T, cfg):
    _branch(rec, T, cfg, "5 epochs", steps=2, epochs=5, val_steps=1)


def ddp_branch_nobody(rec, T, cfg):
    _branch(rec, T, cfg, "1 step", steps=1, epochs=1, val_steps=1)


def ddp_joint(rec, T, cfg):
    _joint(rec, T, cfg, "2 epochs", steps_per_epoch=2, epochs=2, val_steps=1)


# name -> (runner, ranks, labels of the synthetic batches)
CASES = {
    "branch/6_epochs_then_resume": (branch_then_resume, 1, mixed_labels),
    "branch/resume_refused": (branch_refuses_other_checkpoints, 1, mixed_labels),
    "joint/5_epochs_then_resume": (joint_then_resume, 1, mixed_labels),
    "joint/resume_refused": (joint_refuses_branch_checkpoint, 1, mixed_labels),
    "classifier/5_epochs_then_evaluate": (classifier_then_evaluate, 1, mixed_labels),
    "classifier/world_size_2": (classifier_refuses_world2, 1, mixed_labels),
    "evaluators/no_checkpoints": (evaluators(False), 1, mixed_labels),
    "evaluators/checkpoints": (evaluators(True), 1, mixed_labels),
    "gloo2/branch_rank1_never_holds_the_level": (ddp_branch, 2, rank1_never_medium),
    "gloo2/branch_nobody_holds_the_level": (ddp_branch_nobody, 2, nobody_medium),
    "gloo2/joint": (ddp_joint, 2, mixed_labels),
}


def _files(tmp):
    return sorted(os.path.relpath(os.path.join(d, f), tmp) for d, _, fs in os.walk(tmp) for f in fs)


def _events(name, tmp):
    runner, _, labels = CASES[name]
    import adam_dehaze_amd.train as T
    rec = Recorder(tmp, labels)
    with pytest.MonkeyPatch.context() as mp_:
        rec.install(mp_)
        runner(rec, T, config(tmp))
    return rec.events


def _worker(rank, world, port, name, tmp, ret):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), WORLD_SIZE=str(world), RANK=str(rank))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        ret[rank] = json.dumps(_events(name, tmp))
        dist.barrier()
    finally:
        dist.destroy_process_group()


def run_case(name):
    """The transcript of one case: {"files": what it left in its directory, "rank0": events[, "rank1": events]}"""
    ranks = CASES[name][1]
    tmp = tempfile.mkdtemp(prefix="adh_transcript_")
    try:
        if ranks == 1:
            out = {"rank0": _events(name, tmp)}
        else:
            ret = mp.Manager().dict()
            port = 32100 + os.getpid() % 400
            mp.spawn(_worker, args=(ranks, port, name, tmp, ret), nprocs=ranks, join=True)
            out = {f"rank{r}": json.loads(ret[r]) for r in range(ranks)}
        out["files"] = _files(tmp)
        return json.loads(json.dumps(out))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def differences(got, want, where=""):
    """The first few differences between two transcripts, as text."""
    out = []
    for key in sorted(set(got) | set(want)):
        g, w = got.get(key), want.get(key)
        if key == "files" or g is None or w is None:
            if g != w:
                out.append(f"{where} {key}: {g} != {w}")
            continue
        for i, (a, b) in enumerate(zip(g, w)):
            if a != b:
                out.append(f"{where} {key}[{i}]: {a} != golden {b}")
        if len(g) != len(w):
            out.append(f"{where} {key}: {len(g)} events, golden has {len(w)}; first extra: {(g + w)[min(len(g), len(w))]}")
    return out[:8]


def main(argv):
    if "--regen" in argv:
        cases = {name: run_case(name) for name in CASES}
        with open(GOLDEN_PATH, "w") as f:
            f.write('{"cases": {\n')
            f.write(",\n".join(' %s: {\n%s}' % (json.dumps(n), ",\n".join(
                '  %s: [\n%s]' % (json.dumps(k), ",\n".join("   " + json.dumps(e, separators=(",", ":")) for e in v))
                for k, v in c.items())) for n, c in cases.items()))
            f.write("\n}}\n")
        print(f"{GOLDEN_PATH}: {len(cases)} cases, {os.path.getsize(GOLDEN_PATH)} bytes")
    else:
        for name in CASES:
            for key, evs in run_case(name).items():
                print(f"--- {name} {key}")
                for e in evs:
                    print("   ", json.dumps(e))


if __name__ == "__main__":
    main(sys.argv[1:])
