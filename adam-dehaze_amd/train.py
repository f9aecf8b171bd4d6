"""The training, validation and evaluation drivers (/root/reference training/train_joint.py:29-310,
training/train_dehazing.py:16-214, training/train_classifier.py:13-226, evaluation/evaluate.py) on the HIP engine.

Hot path: `build_joint_system(config)` reproduces the reference's construction order (classifier, low, medium, high ->
router -> optimiser -> scheduler -> criterion, train_joint.py:36-98) including the duplicated branch parameters in the
optimiser's list; `joint_train_step` is the body of the hot loop (train_joint.py:129-166), `dehazing_train_step` the one of
train_dehazing.py:71-106.

One epoch loop, `_run_epochs`, serves the three stages and is the only statement of the order between ranks: train, take
rank 0's buffers, validate (sample-weighted sums all-reduced, ONE host read-back per epoch), scheduler step on the agreed
validation loss, rank 0 reports and writes `best_model.pth` / every fifth `checkpoint_epoch_N.pth` atomically, barrier.  A
stage plugs in closures: `train_joint_model` (score val_psnr, reports the rank-averaged train loss, leaves its synchronizer
installed), `train_dehazing_model` (score val_psnr, level-filtered steps, uninstalls its synchronizer in a `finally`),
`train_classifier` (score accuracy from -1; single process, no resume, reloads the best model).  Written once beside it:
`_loader_or_synthetic` (the given loader, else the image folders of the split through `data.folder_loader`, else `data.synthetic_loader`),
`_restore_training_state` (what `resume=` restores after the stage's own key check; the reference parses `--resume` and
ignores it, main.py:50-51), `_validation_sums` for `validate_joint` / `validate_dehazing`, `_joint_system_for_evaluation`
for the evaluators.  Checkpoints carry the reference's keys (train_joint.py:272-283, train_dehazing.py:196-203) plus
`scheduler_state_dict`.

Weight EMA (opt-in: the `ema:` config section, `ema_options`; absent, nothing below happens): each stage keeps an `ema.WeightEMA`
of its model, built after the replicas were made identical, and updates it right after every `optimizer.step()`.  With
`validate` the epoch's validation -- and so the scheduler metric and the best-checkpoint decision -- runs on the EMA weights
(`WeightEMA.applied()`).  Checkpoints keep the raw weights under their usual keys, which is what training resumes from, and
gain `ema_state_dict` / `ema_updates`; with `evaluate` the evaluators load the EMA set (`load_pretrained_model(prefer_ema=True)`).

Data-parallel runs (torchrun, one process per GPU): replicas are made identical by broadcasting rank 0's parameters and
buffers after construction / checkpoint loading; gradients go through `parallel.GradientSynchronizer`; every host-side
decision that steers training -- the metric given to ReduceLROnPlateau, "skip this step, the sub-batch is empty" -- is
agreed across ranks first, so learning rates and step counts cannot diverge.
"""
from __future__ import annotations

import contextlib
import glob
import os
import re
import warnings
from typing import Dict, Iterable, Iterator, Optional

import torch

from .classifier import create_classifier
from .data import synthetic_loader  # noqa: F401  (re-exported: round-1 callers import it from here)
from .dehazing import create_high_intensity_model, create_low_intensity_model, create_medium_intensity_model
from .ema import WeightEMA
from .image_io import DEMO_EXTENSIONS  # noqa: F401  (the extensions --mode demo lists: .png .jpg .jpeg .bmp)
from .loss import get_dehazing_loss, get_joint_loss
from .metrics import psnr_batch, ssim_batch
from .optim import Adam
from .parallel import GradientSynchronizer, all_ranks_any, all_reduce_mean_scalar
from .routing import create_router

LEVELS = {"low": 0, "medium": 1, "high": 2}


class ReduceLROnPlateau:
    """optim.lr_scheduler.ReduceLROnPlateau(mode='min', factor, patience) host logic (train_joint.py:92-94)."""

    def __init__(self, optimizer, mode="min", factor=0.5, patience=3, threshold=1e-4, verbose=False):
        assert mode == "min"
        self.opt, self.factor, self.patience, self.threshold = optimizer, factor, patience, threshold
        self.best, self.bad = float("inf"), 0

    def step(self, metric: float):
        if metric < self.best * (1.0 - self.threshold):
            self.best, self.bad = metric, 0
        else:
            self.bad += 1
        if self.bad > self.patience:
            for gr in self.opt.param_groups:
                gr["lr"] *= self.factor
            self.bad = 0

    def state_dict(self):
        return {"best": self.best, "num_bad_epochs": self.bad, "factor": self.factor, "patience": self.patience,
                "threshold": self.threshold}

    def load_state_dict(self, sd):
        self.best, self.bad = sd["best"], sd["num_bad_epochs"]


def _sync_bn(config) -> bool:
    """Data-parallel BatchNorm mode: `parallel: {sync_bn: true}` in the config (or ADH_SYNC_BN=1) selects
    synchronised statistics -- the single-process reference's semantics at the global batch; default: per-replica."""
    return bool(config.get("parallel", {}).get("sync_bn", False)) or os.environ.get("ADH_SYNC_BN", "0") == "1"


def _world_rank():
    return int(os.environ.get("WORLD_SIZE", "1")), int(os.environ.get("RANK", "0"))


def load_pretrained_model(model, checkpoint_path, prefer_ema: bool = False):
    """train_joint.py:18-27: missing checkpoints are not errors.  `prefer_ema`: the file's `ema_state_dict` (the EMA weights a
    run with the `ema:` section writes next to the raw ones) when it has one."""
    if os.path.exists(checkpoint_path):
        checkpoint = torch.load(checkpoint_path, map_location="cpu")
        if prefer_ema and "ema_state_dict" in checkpoint:
            model.load_state_dict(checkpoint["ema_state_dict"])
            print(f"Loaded EMA weights from {checkpoint_path}")
            return True
        model.load_state_dict(checkpoint["model_state_dict"])
        print(f"Loaded pretrained weights from {checkpoint_path}" + (" (the file has no EMA weights)" if prefer_ema else ""))
        return True
    print(f"Checkpoint {checkpoint_path} not found. Starting with random weights.")
    return False


def optim_guard_options(config) -> Dict:
    """The optional `optim:` section of the config as optim.Adam keyword arguments ({} when it is absent: the plain step)."""
    section = config.get("optim") or {}
    unknown = set(section) - {"grad_clip_norm", "skip_nonfinite"}
    if unknown:
        raise ValueError(f"config optim: unknown keys {sorted(unknown)} (grad_clip_norm, skip_nonfinite)")
    opts = {}
    if section.get("grad_clip_norm") is not None:
        opts["max_grad_norm"] = float(section["grad_clip_norm"])
    if section.get("skip_nonfinite"):
        opts["skip_nonfinite"] = True
    return opts


def ema_options(config) -> Optional[Dict]:
    """The optional `ema:` section of the config with its defaults filled in; None when it is absent or null (no EMA)."""
    section = config.get("ema")
    if section is None:
        return None
    known = ("decay", "warmup", "validate", "evaluate")
    if not isinstance(section, dict):
        raise ValueError(f"config ema: expected a mapping with keys among ({', '.join(known)}), got {section!r}")
    unknown = set(section) - set(known)
    if unknown:
        raise ValueError(f"config ema: unknown keys {sorted(unknown)} ({', '.join(known)})")
    return {"decay": float(section.get("decay", 0.999)), "warmup": bool(section.get("warmup", True)),
            "validate": bool(section.get("validate", True)), "evaluate": bool(section.get("evaluate", False))}


def _weight_ema(config, params) -> Optional[WeightEMA]:
    """The stage's WeightEMA over `params`, or None without the `ema:` section.  Built after the replicas were made identical."""
    opts = ema_options(config)
    return None if opts is None else WeightEMA(params, decay=opts["decay"], warmup=opts["warmup"])


def _evaluate_ema(config) -> bool:
    return bool((ema_options(config) or {}).get("evaluate", False))


class _GuardStats:
    """Mean and max of a guarded optimiser's `last_grad_norm` over an epoch's steps, accumulated on the device from the
    optimiser's step hook; `read()` is the epoch's one read-back (norm sum, max, count and the skip count in one vector).  Inert for
    an unguarded optimiser: no hook, `read()` returns {}."""

    def __init__(self, optimizer):
        self.opt = optimizer if getattr(optimizer, "guarded", False) else None
        self.acc, self.skipped_before = None, 0
        if self.opt is not None:
            self.opt.step_hook = self.add

    def add(self):
        norm = self.opt.last_grad_norm
        if self.acc is None:
            self.acc = torch.zeros(3, device=norm.device)      # sum, max, number of finite norms
        # a non-finite norm (a skipped step) shows in the skip count, not in the mean and the max
        finite = torch.isfinite(norm)
        val = torch.where(finite, norm, torch.zeros_like(norm))
        self.acc[0] += val
        self.acc[1] = torch.maximum(self.acc[1], val)
        self.acc[2] += finite

    def read(self, ema: Optional[WeightEMA] = None) -> Dict:
        """`ema`: its update counter comes back in the same read ("ema_updates")."""
        parts = [] if self.acc is None else [self.acc.double(), self.opt.skipped_total.double().view(1)]
        if ema is not None:
            parts.append(ema.updates_dev.double().view(1))
        if not parts:
            return {}
        host = torch.cat(parts).tolist()
        out = {}
        if self.acc is not None:
            total, peak, count, skipped = host[:4]
            out = {"grad_norm_mean": total / max(1.0, count), "grad_norm_max": peak,
                   "skipped_steps": int(skipped) - self.skipped_before}
            self.acc, self.skipped_before = None, int(skipped)
        if ema is not None:
            out["ema_updates"] = int(host[-1])
        return out

    def close(self):
        if self.opt is not None:
            self.opt.step_hook = None


def build_joint_system(config, world_size: int = 1, adam_duplicates: str = "sequential", with_ema: bool = True) -> Dict:
    """`with_ema=False` (the evaluators: they only run the router) builds no WeightEMA whatever the config says."""
    device = torch.device(config["device"])
    classifier = create_classifier(config)
    low = create_low_intensity_model(config)
    medium = create_medium_intensity_model(config)
    high = create_high_intensity_model(config)
    load_pretrained_model(classifier, os.path.join(config["classifier"]["checkpoint_dir"], "best_model.pth"))
    for name, m in (("low", low), ("medium", medium), ("high", high)):
        load_pretrained_model(m, os.path.join(config["dehazing"]["checkpoint_dir"], name, "best_model.pth"))
    models = {"low": low, "medium": medium, "high": high}
    router = create_router(models, classifier, config).to(device)
    # router.parameters() already holds classifier + branches; the reference appends the branches AGAIN
    params = list(router.parameters())
    for m in models.values():
        params.extend(list(m.parameters()))
    optimizer = Adam(params, lr=config["joint_training"]["learning_rate"], weight_decay=0.0001, duplicates=adam_duplicates,
                     **optim_guard_options(config))
    scheduler = ReduceLROnPlateau(optimizer, mode="min", factor=0.5, patience=3)
    criterion = get_joint_loss(config).to(device)
    sync = None
    if world_size > 1:
        # a hard router leaves the branches a rank did not route to without gradients: agree on who produced what
        hard = config.get("routing", {}).get("type", "soft") == "hard"
        if hard and _sync_bn(config):
            # HardRouter skips a branch whose sub-batch is empty on a rank (routing.py): with sync-BN every rank must issue the SAME
            # sequence of per-BatchNorm all-reduces, forward and backward -- a rank that skips a branch would deadlock the others
            # or, worse, pair [2C+1] vectors of different layers.  The reference is single-process; the combination
            # has no meaning to preserve, so it is refused rather than emulated with zero-count dummy collectives.
            raise ValueError("routing.type 'hard' cannot be combined with parallel.sync_bn at world_size > 1: a rank whose "
                             "sub-batch for a branch is empty would skip that branch's BatchNorm collectives; use replica-BN "
                             "(the default) or a soft / gated router")
        sync = GradientSynchronizer(list(router.parameters()), world_size, detect_unused=hard, sync_bn=_sync_bn(config))
        sync.broadcast_parameters(router)
        sync.install()
    # every unique parameter once (router.parameters() holds classifier + branches); after the broadcast: one seed for all ranks
    ema = _weight_ema(config, router.parameters()) if with_ema else None
    return {"classifier": classifier, "models": models, "router": router, "optimizer": optimizer,
            "scheduler": scheduler, "criterion": criterion, "sync": sync, "device": device, "ema": ema}


# the opt-in terms of DehazingLoss: the key a step reports them under (when the config turns them on) -> the epoch report's label
_OPT_IN_TERMS = {"ssim": "1 - SSIM", "fft": "FFT L1", "ms_ssim": "1 - MS-SSIM"}


def joint_train_step(system: Dict, batch: Dict) -> Dict:
    """One iteration of train_joint.py:129-166.  Losses stay on the device (no .item() sync)."""
    dev = system["device"]
    hazy, clear, labels = batch["hazy"].to(dev), batch["clear"].to(dev), batch["intensity"].to(dev)
    sync = system["sync"]
    system["optimizer"].zero_grad()
    if sync is not None:
        sync.begin_step()
    logits, _ = system["classifier"](hazy)
    dehazed, _ = system["router"](hazy, logits)
    loss, comps = system["criterion"](dehazed, clear, logits, labels)
    loss.backward()
    if sync is not None:
        sync.finish()
    system["optimizer"].step()
    if system.get("ema") is not None:
        system["ema"].update(system["optimizer"])
    stats = {"loss": loss.detach(), "dehazing": comps["dehazing"].detach(),
             "classification": comps["classification"].detach()}
    for k in _OPT_IN_TERMS:                            # loss.lambda_ssim / lambda_fft / lambda_msssim > 0 only
        if k in comps["dehazing_components"]:
            stats[k] = comps["dehazing_components"][k].detach()
    return stats


def dehazing_train_step(model, criterion, optimizer, batch: Dict, level: Optional[int], device, sync=None, ema=None):
    """One iteration of train_dehazing.py:71-106: keep only the images of this branch's fog level.  Under data
    parallelism a rank whose sub-batch is empty still takes part in the gradient all-reduce (with zeros) unless the
    sub-batch is empty on EVERY rank, so no rank is left waiting in a collective.  `ema`: updated after every optimiser step (a
    step that returns early because the sub-batch is empty everywhere takes none)."""
    hazy, clear, labels = batch["hazy"], batch["clear"], batch["intensity"]
    if level is not None:
        keep = labels == level
        empty = int(keep.sum()) == 0
        if sync is not None and sync.world > 1:
            if not all_ranks_any(not empty, device):
                return None
        elif empty:
            return None
        hazy, clear = hazy[keep], clear[keep]
    else:
        empty = False
    optimizer.zero_grad()
    if sync is not None:
        sync.begin_step()
    loss = comps = None
    if not empty:
        hazy, clear = hazy.to(device), clear.to(device)
        out = model(hazy)
        loss, comps = criterion(out, clear)
        loss.backward()
    if sync is not None:
        sync.finish()
    optimizer.step()
    if ema is not None:
        ema.update(optimizer)
    if empty:
        return None
    stats = {"loss": loss.detach(), "l1": comps["l1"].detach()}
    for k in _OPT_IN_TERMS:                            # loss.lambda_ssim / lambda_fft / lambda_msssim > 0 only
        if k in comps:
            stats[k] = comps[k].detach()
    return stats


# ---------------------------------------------------------------------------------------------------------------------
# validation (device-side metrics, one read-back per epoch)
# ---------------------------------------------------------------------------------------------------------------------
def _finish_validation(sums: Dict[str, torch.Tensor], count: int, device) -> Dict[str, float]:
    """Sample-weighted means; under data parallelism sums and counts are added over the ranks first."""
    import torch.distributed as dist
    keys = sorted(sums)
    vec = torch.stack([sums[k].double().reshape(()) for k in keys] + [torch.tensor(float(count), dtype=torch.float64,
                                                                                   device=device)])
    if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
        if dist.get_backend() == "nccl":
            dist.all_reduce(vec)
        else:
            host = vec.cpu()
            dist.all_reduce(host)
            vec = host
    host = vec.cpu().tolist()   # the epoch's one host read-back
    n = host[-1]
    out = {k: (v / n if n > 0 else 0.0) for k, v in zip(keys, host[:-1])}
    out["val_samples"] = int(n)
    return out


def _validation_sums(keys, device):
    """The accumulator of a validation pass: (sums, add).  The key set is fixed and every sum starts at zero, so a rank that
    saw nothing still hands the full vector to the all-reduce inside _finish_validation (a rank returning early
    left the others waiting in the collective)."""
    sums = {k: torch.zeros((), dtype=torch.float64, device=device) for k in keys}

    def add(k, v):
        sums[k] = sums[k] + v
    return sums, add


def validate_joint(system: Dict, val_loader: Iterable[Dict]) -> Dict[str, float]:
    """train_joint.py:173-236: eval mode, classifier -> router -> JointLoss, per-image PSNR / SSIM; returns
    {'val_loss','val_dehaze_loss','val_class_loss','val_psnr','val_ssim','val_samples'} (sample-weighted means)."""
    dev = system["device"]
    system["classifier"].eval()
    for m in system["models"].values():
        m.eval()
    system["router"].eval()
    sums, add = _validation_sums(("val_loss", "val_dehaze_loss", "val_class_loss", "val_psnr", "val_ssim"), dev)
    count = 0
    with torch.no_grad():
        for batch in val_loader:
            hazy, clear, labels = batch["hazy"].to(dev), batch["clear"].to(dev), batch["intensity"].to(dev)
            logits, _ = system["classifier"](hazy)
            dehazed, _ = system["router"](hazy, logits)
            loss, comps = system["criterion"](dehazed, clear, logits, labels)
            n = hazy.size(0)
            add("val_loss", loss.detach().double() * n)
            add("val_dehaze_loss", comps["dehazing"].detach().double() * n)
            add("val_class_loss", comps["classification"].detach().double() * n)
            add("val_psnr", psnr_batch(dehazed, clear).double().sum())
            add("val_ssim", ssim_batch(dehazed, clear).double().sum())
            count += n
    return _finish_validation(sums, count, dev)


def validate_dehazing(model, criterion, val_loader: Iterable[Dict], level: Optional[int], device) -> Dict[str, float]:
    """train_dehazing.py:109-166: eval mode, images of this branch's level only; returns
    {'val_loss','val_perceptual','val_psnr','val_ssim','val_samples'}."""
    model.eval()
    device = torch.device(device)
    sums, add = _validation_sums(("val_loss", "val_perceptual", "val_psnr", "val_ssim"), device)
    count = 0
    with torch.no_grad():
        for batch in val_loader:
            hazy, clear = batch["hazy"], batch["clear"]
            if level is not None:
                keep = batch["intensity"] == level
                if int(keep.sum()) == 0:
                    continue
                hazy, clear = hazy[keep], clear[keep]
            hazy, clear = hazy.to(device), clear.to(device)
            out = model(hazy)
            loss, comps = criterion(out, clear)
            n = hazy.size(0)
            add("val_loss", loss.detach().double() * n)
            add("val_perceptual", comps["perceptual"].detach().double() * n)
            add("val_psnr", psnr_batch(out, clear).double().sum())
            add("val_ssim", ssim_batch(out, clear).double().sum())
            count += n
    return _finish_validation(sums, count, device)


# ---------------------------------------------------------------------------------------------------------------------
# checkpoints (reference key sets) and resume
# ---------------------------------------------------------------------------------------------------------------------
def joint_checkpoint(system: Dict, epoch: int, val: Dict[str, float]) -> Dict:
    """train_joint.py:272-283 / 291-302 (+ scheduler_state_dict)."""
    return {"epoch": epoch,
            "router_state_dict": system["router"].state_dict(),
            "low_model_state_dict": system["models"]["low"].state_dict(),
            "medium_model_state_dict": system["models"]["medium"].state_dict(),
            "high_model_state_dict": system["models"]["high"].state_dict(),
            "classifier_state_dict": system["classifier"].state_dict(),
            "optimizer_state_dict": system["optimizer"].state_dict(),
            "val_psnr": val["val_psnr"], "val_ssim": val["val_ssim"], "val_loss": val["val_loss"],
            "scheduler_state_dict": system["scheduler"].state_dict()}


def dehazing_checkpoint(model, optimizer, scheduler, epoch: int, val: Dict[str, float]) -> Dict:
    """train_dehazing.py:196-203 / 208-215 (+ scheduler_state_dict)."""
    return {"epoch": epoch, "model_state_dict": model.state_dict(), "optimizer_state_dict": optimizer.state_dict(),
            "val_psnr": val["val_psnr"], "val_ssim": val["val_ssim"], "val_loss": val["val_loss"],
            "scheduler_state_dict": scheduler.state_dict()}


def save_checkpoint_atomic(obj: Dict, path: str) -> None:
    """torch.save to `<path>.tmp.<pid>` + os.replace: a reader (another rank's load_pretrained_model, a --resume) never
    sees a half-written zip."""
    tmp = f"{path}.tmp.{os.getpid()}"
    try:
        torch.save(obj, tmp)
        os.replace(tmp, path)
    finally:
        if os.path.exists(tmp):
            os.remove(tmp)


def _barrier():
    """All ranks wait here (after rank 0's checkpoint block, before anyone reads what it wrote)."""
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
        dist.barrier()


def _sync_buffers_from_rank0(sync, *modules) -> None:
    """Replica-BN lets the BatchNorm running statistics of the replicas drift apart; before validation and before rank 0
    writes a checkpoint every rank takes rank 0's buffers (what DDP's broadcast_buffers=True does every forward)."""
    if sync is not None and sync.world > 1:
        sync.broadcast_buffers(*modules)


def find_resume_checkpoint(checkpoint_dir: str) -> Optional[str]:
    """Latest `checkpoint_epoch_N.pth`, else `best_model.pth`, else None."""
    best_n, best_p = -1, None
    for p in glob.glob(os.path.join(checkpoint_dir, "checkpoint_epoch_*.pth")):
        m = re.search(r"checkpoint_epoch_(\d+)\.pth$", p)
        if m and int(m.group(1)) > best_n:
            best_n, best_p = int(m.group(1)), p
    best = os.path.join(checkpoint_dir, "best_model.pth")
    if os.path.exists(best):
        if best_p is None:
            return best
        # whichever was written later in training
        try:
            if torch.load(best, map_location="cpu")["epoch"] + 1 > best_n:
                return best
        except Exception:
            pass
    return best_p


def _best_psnr_on_disk(checkpoint_dir: str) -> float:
    p = os.path.join(checkpoint_dir, "best_model.pth")
    if os.path.exists(p):
        try:
            return float(torch.load(p, map_location="cpu").get("val_psnr", 0.0))
        except Exception:
            return 0.0
    return 0.0


def _resolve_resume(resume, checkpoint_dir: str) -> Optional[str]:
    if not resume:
        return None
    path = find_resume_checkpoint(checkpoint_dir) if resume is True else str(resume)
    if path is None or not os.path.exists(path):
        raise FileNotFoundError(f"--resume: no checkpoint to resume from ({path or checkpoint_dir})")
    return path


def checkpoint_stage(path: str, config) -> str:
    """Which training stage wrote `path`: 'joint' (train_joint.py:272-283 key set) or the branch level 'low' / 'medium' /
    'high' whose state_dict key set the checkpoint's `model_state_dict` has (train_dehazing.py:196-203).  Raises
    ValueError for anything else.  main.py uses it to hand an explicit `--resume <file>` to the one stage it belongs to."""
    ck = torch.load(path, map_location="cpu")
    if "router_state_dict" in ck:
        return "joint"
    if "model_state_dict" not in ck:
        raise ValueError(f"--resume {path}: neither a joint nor a branch checkpoint (keys {sorted(ck)[:6]} ...)")
    keys = set(ck["model_state_dict"])
    for level, factory in (("low", create_low_intensity_model), ("medium", create_medium_intensity_model),
                           ("high", create_high_intensity_model)):
        if set(factory(config).state_dict()) == keys:
            return level
    raise ValueError(f"--resume {path}: model_state_dict matches none of the configured branches")


def _restore_training_state(ck: Dict, optimizer, scheduler, sync, module, ema=None) -> int:
    """What every resume does once its stage has checked `ck` and loaded the weights into `module`: optimiser and scheduler
    state, the packed copies of the old weights dropped, the replicas made identical again, the EMA shadow and its counter (a
    checkpoint without them seeds the shadow from the loaded weights).  Returns the epoch to continue with; the best score so
    far is `_best_psnr_on_disk` of the stage's directory."""
    if "optimizer_state_dict" in ck:
        optimizer.load_state_dict(ck["optimizer_state_dict"])
    if "scheduler_state_dict" in ck:
        scheduler.load_state_dict(ck["scheduler_state_dict"])
    from .engine import invalidate_weight_cache
    invalidate_weight_cache()
    if sync is not None:
        sync.broadcast_parameters(module)
    if ema is not None:
        if "ema_state_dict" in ck and "ema_updates" in ck:
            ema.load_state_dict(module, ck["ema_state_dict"], int(ck["ema_updates"]))
        else:
            ema.reseed()
            print("Checkpoint has no EMA weights: the EMA starts from the loaded weights")
    return int(ck["epoch"]) + 1


def resume_joint(system: Dict, path: str) -> int:
    """Restore a joint checkpoint (every rank loads it, then takes rank 0's copy); returns the epoch to continue with."""
    ck = torch.load(path, map_location="cpu")
    if "router_state_dict" not in ck:
        raise ValueError(f"--resume {path}: not a joint-training checkpoint (keys {sorted(ck)[:6]} ...); a branch "
                         "checkpoint resumes `--mode train_dehazing`, not this stage")
    system["router"].load_state_dict(ck["router_state_dict"])   # holds the classifier and the three branches
    start_epoch = _restore_training_state(ck, system["optimizer"], system["scheduler"], system["sync"], system["router"],
                                          ema=system.get("ema"))
    print(f"Resumed joint training from {path} (epoch {ck['epoch'] + 1} done)")
    return start_epoch


def _warn_synthetic(config, what: str, rank: int, stacklevel: int = 3):
    paths = [config.get("dataset", {}).get(k) for k in ("train_path", "val_path", "test_path")]
    if rank == 0:
        msg = (f"{what}: no DataLoader was supplied -- training on SYNTHETIC foggy frames generated on the GPU "
               "(data.synthetic_loader); checkpoints written by this run are trained on noise-like images.")
        if any(paths):
            # (the wording predates data.folder_loader and is pinned by the drivers' golden transcript: the paths were looked
            # at, and no <path>/<split>/{low,medium,high}/hazy or <path>/{low,medium,high}/hazy folder was found under them)
            msg += (f"  Dataset paths are configured ({[p for p in paths if p]}) but this build does not read image "
                    "folders (data/dataset.py needs cv2, out of scope): pass train_loader= / val_loader=.")
        warnings.warn(msg, stacklevel=stacklevel)


def _folder_loader(config, split: str, device):
    """`data.folder_loader` for this process: the train and val splits are sharded over the ranks; the test split is read whole,
    because every driver that reads it runs on one rank (_rank0_only evaluators, the single-process classifier stage)."""
    from .data import folder_loader
    world, rank = (1, 0) if split == "test" else _world_rank()
    return folder_loader(config, split, device, rank=rank, world=world)


def _uses_synthetic(config, device, **loaders) -> bool:
    """True when one of the splits named by the keywords (train=..., val=...) has neither a supplied loader nor image folders,
    so `_loader_or_synthetic` will generate it."""
    return any(loader is None and _folder_loader(config, split, device) is None for split, loader in loaders.items())


def _loader_or_synthetic(loader, config, steps: int, seed_offset: int, device, epoch: int = 0, warn: Optional[str] = None,
                         split: str = "train"):
    """The loader choice of every driver: `loader` as it is (a callable is asked for the epoch's iterable); else the image
    folders of `split` under the configured dataset path (`data.folder_loader`, its cache built once per process); else `steps`
    synthetic batches seeded `seed + seed_offset + epoch`: offset 0 and the epoch for training frames, 500000 for the fixed
    validation set, 900000 / 910000 for the test sets, whose drivers pass their name as `warn` to say so."""
    if loader is None:
        loader = _folder_loader(config, split, device)
    if loader is not None:
        return loader(epoch) if callable(loader) else loader
    rank = _world_rank()[1]
    if warn is not None:
        _warn_synthetic(config, warn, rank, stacklevel=4)
    return synthetic_loader(config["dataset"]["batch_size"], config["dataset"]["img_size"], steps,
                            seed=config["seed"] + seed_offset + epoch, rank=rank, device=device)


def _run_epochs(first_epoch: int, epochs: int, train_epoch, validate, scheduler, loss_key: str, score_key: str, best: float,
                score_text: str, ck_dir: str, checkpoint, report, sync=None, modules=(), device=None, ema=None, ema_model=None,
                ema_validate: bool = True):
    """The epoch loop of the three training stages: the one statement of what the ranks do in which order.  The stage plugs
    in `train_epoch(epoch)`, `validate() -> dict`, `checkpoint(epoch, val) -> dict` and `report(epoch, train_loss, val)`.
    Returns the per-epoch records {"epoch", "train_loss", **val, "lr"}; with the `optim:` guard on they also carry
    "grad_norm_mean", "grad_norm_max" and "skipped_steps" of the epoch (this rank's; after the all-reduce every rank sees the
    same gradient).  With a WeightEMA (`ema`, over the parameters of `ema_model`) they carry "ema_updates", read back together
    with the guard's statistics; validation runs inside `ema.applied()` when `ema_validate`, and every checkpoint gains
    "ema_state_dict" and "ema_updates" next to the raw weights."""
    rank = _world_rank()[1]
    history = []
    guard = _GuardStats(scheduler.opt)

    def with_ema(ck, stats):
        if ema is not None:
            ck["ema_state_dict"], ck["ema_updates"] = ema.state_dict(ema_model), stats["ema_updates"]
        return ck
    if rank == 0:
        os.makedirs(ck_dir, exist_ok=True)
    for epoch in range(first_epoch, epochs):
        # None, or this rank's mean train loss where the stage reports the rank-averaged one (the joint stage)
        train_loss = train_epoch(epoch)
        guard_stats = guard.read(ema)                 # the epoch-end read-back of the step statistics, EMA counter included
        _sync_buffers_from_rank0(sync, *modules)      # validation and rank 0's checkpoint see one model
        with ema.applied() if ema is not None and ema_validate else contextlib.nullcontext():
            val = validate()                          # every rank enters its all-reduce, also one with nothing to validate
        if train_loss is not None:
            train_loss = all_reduce_mean_scalar(train_loss, device)
        scheduler.step(val[loss_key])                 # every rank steps on the same (rank-averaged) value
        history.append({"epoch": epoch, "train_loss": train_loss, **val, "lr": scheduler.opt.param_groups[0]["lr"],
                        **guard_stats})
        if rank == 0:
            report(epoch, train_loss, val)
            if "grad_norm_mean" in guard_stats:
                print("  Grad norm: mean {grad_norm_mean:.4f}, max {grad_norm_max:.4f}; skipped steps: {skipped_steps}"
                      .format(**guard_stats))
            if ema is not None:
                print(f"  EMA updates: {guard_stats['ema_updates']}" + (" (validated on the EMA weights)" if ema_validate else ""))
            if val[score_key] > best:
                save_checkpoint_atomic(with_ema(checkpoint(epoch, val), guard_stats),
                                       os.path.join(ck_dir, "best_model.pth"))
                print("Saved best model with validation " + score_text.format(val[score_key]))
            if (epoch + 1) % 5 == 0:
                save_checkpoint_atomic(with_ema(checkpoint(epoch, val), guard_stats),
                                       os.path.join(ck_dir, f"checkpoint_epoch_{epoch + 1}.pth"))
        best = max(best, val[score_key])
        # nobody runs ahead (into the next stage's load_pretrained_model, a --resume) while rank 0 is still writing
        _barrier()
    guard.close()
    return history


def train_joint_model(config, train_loader=None, val_loader=None, steps_per_epoch: int = 4, epochs: Optional[int] = None,
                      resume=None, val_steps: int = 2):
    """train_joint.py:29 entry point: epochs of (train, validate, scheduler.step(val_loss), best / periodic
    checkpoints).  `train_loader` / `val_loader`: iterables of batch dicts (re-iterated every epoch) or callables
    epoch -> iterable; synthetic frames when None.  Returns (system, history of per-epoch dicts)."""
    world = _world_rank()[0]
    system = build_joint_system(config, world)
    dev = system["device"]
    ck_dir = config["joint_training"]["checkpoint_dir"]
    epochs = config["joint_training"]["epochs"] if epochs is None else epochs
    start_epoch, best_val_psnr = 0, 0.0
    path = _resolve_resume(resume, ck_dir)
    if path is not None:
        start_epoch, best_val_psnr = resume_joint(system, path), _best_psnr_on_disk(ck_dir)
    if _uses_synthetic(config, dev, train=train_loader, val=val_loader):
        _warn_synthetic(config, "train_joint_model", _world_rank()[1])
    term_totals, n = {}, 0       # the opt-in loss terms summed over the epoch's steps on this rank, for the report

    def train_epoch(epoch):
        nonlocal n
        system["classifier"].train()
        for m in system["models"].values():
            m.train()
        system["router"].train()
        total, n = None, 0
        term_totals.clear()
        for batch in _loader_or_synthetic(train_loader, config, steps_per_epoch, 0, dev, epoch):
            stats = joint_train_step(system, batch)
            total = stats["loss"] if total is None else total + stats["loss"]
            for k in _OPT_IN_TERMS:
                if k in stats:
                    term_totals[k] = stats[k] if k not in term_totals else term_totals[k] + stats[k]
            n += 1
        return float(total) / max(1, n) if total is not None else 0.0

    def report(epoch, train_loss, val):
        terms_part = "".join(f" ({_OPT_IN_TERMS[k]}: {float(v) / max(1, n):.4f}, this rank)" for k, v in term_totals.items())
        print(f"Epoch {epoch + 1}/{epochs}:\n  Train Loss: {train_loss:.4f}{terms_part}\n  Val Loss: {val['val_loss']:.4f} "
              f"(Dehaze: {val['val_dehaze_loss']:.4f}, Class: {val['val_class_loss']:.4f})\n"
              f"  Val PSNR: {val['val_psnr']:.2f} dB, Val SSIM: {val['val_ssim']:.4f}")

    def validate():
        return validate_joint(system, _loader_or_synthetic(val_loader, config, val_steps, 500000, dev, split="val"))

    # (unlike the branch stage, this one leaves its synchronizer installed when it returns)
    history = _run_epochs(start_epoch, epochs, train_epoch, validate, system["scheduler"], loss_key="val_loss",
                          score_key="val_psnr", best=best_val_psnr, score_text="PSNR: {:.2f} dB", ck_dir=ck_dir,
                          checkpoint=lambda epoch, val: joint_checkpoint(system, epoch, val), report=report,
                          sync=system["sync"], modules=(system["router"],), device=dev, ema=system["ema"],
                          ema_model=system["router"], ema_validate=(ema_options(config) or {}).get("validate", True))
    return system, history


def train_dehazing_model(config, intensity_level: str, train_loader=None, val_loader=None, steps: int = 4,
                         epochs: int = 1, resume=None, val_steps: int = 2, model=None):
    """train_dehazing.py:16 entry point for one branch: Adam(lr, wd 1e-4) + ReduceLROnPlateau(patience 5) +
    DehazingLoss, level-filtered batches, validation, best / every-5-epochs checkpoints under
    `<dehazing.checkpoint_dir>/<level>/` (the reference runs 30 epochs, :64).  Returns (model, per-step train losses)."""
    world = _world_rank()[0]
    device = torch.device(config["device"])
    factory = {"low": create_low_intensity_model, "medium": create_medium_intensity_model,
               "high": create_high_intensity_model}[intensity_level]
    model = (factory(config) if model is None else model).to(device).train()
    criterion = get_dehazing_loss(config).to(device)
    optimizer = Adam(model.parameters(), lr=config["dehazing"][intensity_level]["learning_rate"], weight_decay=1e-4,
                     **optim_guard_options(config))
    scheduler = ReduceLROnPlateau(optimizer, mode="min", factor=0.5, patience=5)
    level = LEVELS[intensity_level]
    ck_dir = os.path.join(config["dehazing"]["checkpoint_dir"], intensity_level)
    sync = None
    if world > 1:
        sync = GradientSynchronizer(list(model.parameters()), world, sync_bn=_sync_bn(config))
        sync.broadcast_parameters(model)
        sync.install()
    ema = _weight_ema(config, model.parameters())         # after the broadcast: every rank seeds from the same weights
    start_epoch, best_val_psnr = 0, 0.0
    path = _resolve_resume(resume, ck_dir)
    if path is not None:
        ck = torch.load(path, map_location="cpu")
        if "model_state_dict" not in ck:
            raise ValueError(f"--resume {path}: not a branch checkpoint (keys {sorted(ck)[:6]} ...); a joint checkpoint "
                             "resumes `--mode train_joint`")
        missing = set(model.state_dict()) ^ set(ck["model_state_dict"])
        if missing:
            raise ValueError(f"--resume {path}: checkpoint does not belong to the '{intensity_level}' branch "
                             f"({len(missing)} state_dict keys differ, e.g. {sorted(missing)[:3]})")
        model.load_state_dict(ck["model_state_dict"])
        start_epoch = _restore_training_state(ck, optimizer, scheduler, sync, model, ema=ema)
        best_val_psnr = _best_psnr_on_disk(ck_dir)
    if _uses_synthetic(config, device, train=train_loader, val=val_loader):
        _warn_synthetic(config, f"train_dehazing_model[{intensity_level}]", _world_rank()[1])
    losses, opt_in_terms = [], {k: [] for k in _OPT_IN_TERMS}

    def train_epoch(epoch):
        model.train()
        for terms in opt_in_terms.values():
            terms.clear()
        for batch in _loader_or_synthetic(train_loader, config, steps, 0, device, epoch):
            st = dehazing_train_step(model, criterion, optimizer, batch, level, device, sync=sync, ema=ema)
            if st is not None:
                losses.append(st["loss"])
                for k, terms in opt_in_terms.items():
                    if k in st:
                        terms.append(st[k])

    def report(epoch, train_loss, val):
        print(f"Epoch {epoch + 1}/{epochs}:\n  Val Loss: {val['val_loss']:.4f}, Val PSNR: {val['val_psnr']:.2f}, "
              f"Val SSIM: {val['val_ssim']:.4f}")
        for k, terms in opt_in_terms.items():  # the opt-in loss terms, mean over this rank's steps like the L1 term
            if terms:
                print(f"  Train {_OPT_IN_TERMS[k]}: {float(torch.stack(terms).mean()):.4f}")

    def validate():
        val_batches = _loader_or_synthetic(val_loader, config, val_steps, 500000, device, split="val")
        return validate_dehazing(model, criterion, val_batches, level, device)

    try:
        _run_epochs(start_epoch, epochs, train_epoch, validate, scheduler, loss_key="val_loss", score_key="val_psnr",
                    best=best_val_psnr, score_text="PSNR: {:.2f} dB", ck_dir=ck_dir,
                    checkpoint=lambda epoch, val: dehazing_checkpoint(model, optimizer, scheduler, epoch, val), report=report,
                    sync=sync, modules=(model,), ema=ema, ema_model=model,
                    ema_validate=(ema_options(config) or {}).get("validate", True))
    finally:       # train_all: the next stage builds its own synchronizer
        if sync is not None:
            sync.uninstall()
    return model, [float(x) for x in losses]


def _rank0_only(fn):
    """Run `fn` on rank 0 while the other ranks wait -- and make sure they stop waiting: rank 0 reaches the hand-off in a
    `finally`, broadcasts whether it succeeded, and the others exit non-zero if it did not (a rank 0 that raised
    left the others in a barrier until the collective timeout).  The wait itself is a store-based monitored barrier with a
    long timeout when the backend offers one (gloo), so a long evaluation does not trip RCCL's 10-minute watchdog."""
    import functools

    @functools.wraps(fn)
    def wrapper(*a, **k):
        world, rank = _world_rank()
        if world <= 1:
            return fn(*a, **k)
        import datetime
        import torch.distributed as dist
        ok, result, err = 1, None, None
        if rank == 0:
            try:
                result = fn(*a, **k)
            except BaseException as e:     # noqa: BLE001 -- the others must be told before it propagates
                ok, err = 0, e
        group = _eval_wait_group()
        flag = torch.tensor([ok], dtype=torch.int32)
        try:
            dist.monitored_barrier(group=group, timeout=datetime.timedelta(hours=12))
        except (RuntimeError, ValueError, AttributeError):
            dist.barrier(group=group)
        dist.broadcast(flag, src=0, group=group)
        if err is not None:
            raise err
        if int(flag.item()) == 0:
            raise SystemExit(f"rank {rank}: rank 0 failed in {fn.__name__}; exiting")
        return result
    return wrapper


_EVAL_GROUP = None


def _eval_wait_group():
    """A gloo group for the long rank-0-only waits (created once, by every rank, the first time it is needed)."""
    global _EVAL_GROUP
    import datetime
    import torch.distributed as dist
    if _EVAL_GROUP is None:
        try:
            _EVAL_GROUP = dist.new_group(backend="gloo", timeout=datetime.timedelta(hours=12))
        except (RuntimeError, ValueError):
            _EVAL_GROUP = dist.group.WORLD
    return _EVAL_GROUP


def _joint_system_for_evaluation(config):
    """The routed system as an evaluator wants it: built for one process, the joint checkpoint loaded over the individually
    loaded weights if there is one, everything in eval mode.  Returns (system, path of the joint checkpoint it loaded or
    None)."""
    system = build_joint_system(config, 1, with_ema=False)
    ck = os.path.join(config["joint_training"]["checkpoint_dir"], "best_model.pth")
    loaded = None
    if os.path.exists(ck):
        checkpoint = torch.load(ck, map_location="cpu")
        if _evaluate_ema(config) and "ema_state_dict" in checkpoint:
            system["router"].load_state_dict(checkpoint["ema_state_dict"])    # the router's state dict with the EMA weights
            print(f"Loaded joint model (EMA weights) from {ck}")
        else:
            system["router"].load_state_dict(checkpoint["router_state_dict"])
            print(f"Loaded joint model from {ck}")
        loaded = ck
    else:
        print(f"Joint checkpoint {ck} not found. Using the individually loaded / random weights.")
    system["classifier"].eval()
    for m in system["models"].values():
        m.eval()
    system["router"].eval()
    return system, loaded


def _ciede2000_switch(config):
    """`evaluation.ciede2000: true` adds the CIEDE2000 column to the image-quality results; absent or false, the
    metrics object is built exactly as before and the result files keep the reference's keys."""
    return {"use_ciede2000": True} if (config.get("evaluation") or {}).get("ciede2000") else {}


def _ms_ssim_switch(config):
    """`evaluation.ms_ssim: true` adds the columns `ssim_gaussian` and `ms_ssim` to the image-quality results the
    same way; the evaluated frames then need 176 px on the shorter side."""
    return {"use_ms_ssim": True} if (config.get("evaluation") or {}).get("ms_ssim") else {}


def _self_ensemble_mode(config):
    """`evaluation.self_ensemble: 'flip' | 'd8'` averages every evaluated output over 4 or 8 symmetries of its input;
    absent, None: the evaluators make exactly the calls they made before."""
    mode = (config.get("evaluation") or {}).get("self_ensemble")
    if mode is not None and mode not in ("flip", "d8"):
        raise ValueError(f"evaluation.self_ensemble must be 'flip' or 'd8', got {mode!r}")
    return mode


def _record_self_ensemble(path, mode):
    """the top-level `self_ensemble` key of a result file written by ImageQualityMetrics.save_results"""
    import json
    with open(path) as f:
        saved = json.load(f)
    saved["self_ensemble"] = {"mode": mode, "passes": {"flip": 4, "d8": 8}[mode]}
    with open(path, "w") as f:
        json.dump(saved, f, indent=2)


@_rank0_only
def evaluate_joint_model(config, test_loader=None, steps: int = 2, use_lpips: bool = True):
    """evaluation/evaluate.py:94-177 (image-quality part): load the joint checkpoint if present, route every test
    batch, accumulate PSNR / SSIM / LPIPS per intensity category on the device, print and save
    `<evaluation.results_dir>/joint_model_results.json` (schema of evaluation/metrics.py:117-124)."""
    from .metrics import CATEGORY_BY_LABEL, ImageQualityMetrics
    # (every rank scoring its own shard and writing the same JSON concurrently was a race, ADVICE r2: rank 0 evaluates and
    # writes, the others wait for it in _rank0_only)
    ensemble = _self_ensemble_mode(config)
    system, _ = _joint_system_for_evaluation(config)
    dev = system["device"]
    metrics = ImageQualityMetrics(device=dev, use_lpips=use_lpips, **_ciede2000_switch(config), **_ms_ssim_switch(config))
    test_loader = _loader_or_synthetic(test_loader, config, steps, 900000, dev, warn="evaluate_joint_model", split="test")

    def routed(h):                                     # every variant of the ensemble gets logits of its own
        return system["router"](h, system["classifier"](h)[0])
    with torch.no_grad():
        for batch in test_loader:
            hazy, clear = batch["hazy"].to(dev), batch["clear"].to(dev)
            if ensemble is None:
                logits, _ = system["classifier"](hazy)
                dehazed, _ = system["router"](hazy, logits)
            else:
                from .d4 import self_ensemble
                dehazed, _ = self_ensemble(routed, hazy, ensemble)
            cats = [CATEGORY_BY_LABEL.get(int(i), "high_intensity") for i in batch["intensity"].tolist()]
            metrics.add_batch(dehazed, clear, cats)
    results = metrics.print_results()
    out_dir = config.get("evaluation", {}).get("results_dir", "results")
    metrics.save_results(os.path.join(out_dir, "joint_model_results.json"))
    if ensemble is not None:
        _record_self_ensemble(os.path.join(out_dir, "joint_model_results.json"), ensemble)
    return results


@_rank0_only
def evaluate_baseline_models(config, test_loader=None, steps: int = 2, use_lpips: bool = True):
    """evaluation/evaluate.py:32-92: every test image through the branch model of its ground-truth fog intensity (no classifier,
    no router), PSNR / SSIM / LPIPS per category on the device, `<evaluation.results_dir>/baseline_results.json`.  The reference
    runs one image at a time; eval-mode branches are per-sample independent, so the images of a level go through as one batch."""
    from .metrics import CATEGORY_BY_LABEL, ImageQualityMetrics
    ensemble = _self_ensemble_mode(config)
    system = build_joint_system(config, 1, with_ema=False)
    dev = system["device"]
    for level, m in system["models"].items():
        load_pretrained_model(m, os.path.join(config["dehazing"]["checkpoint_dir"], level, "best_model.pth"),
                              prefer_ema=_evaluate_ema(config))
        m.eval()
    by_label = {0: system["models"]["low"], 1: system["models"]["medium"], 2: system["models"]["high"]}
    metrics = ImageQualityMetrics(device=dev, use_lpips=use_lpips, **_ciede2000_switch(config), **_ms_ssim_switch(config))
    test_loader = _loader_or_synthetic(test_loader, config, steps, 900000, dev, warn="evaluate_baseline_models",
                                       split="test")
    with torch.no_grad():
        for batch in test_loader:
            hazy, clear = batch["hazy"].to(dev), batch["clear"].to(dev)
            labels = batch["intensity"].to(dev).clamp(max=2)       # evaluate.py:73-81: anything above 1 is "high"
            for lab, model in by_label.items():
                idx = torch.nonzero(labels == lab).flatten()
                if idx.numel() and ensemble is None:
                    metrics.add_batch(model(hazy[idx].contiguous()), clear[idx].contiguous(),
                                      [CATEGORY_BY_LABEL[lab]] * int(idx.numel()))
                elif idx.numel():
                    from .d4 import self_ensemble
                    dehazed, _ = self_ensemble(lambda b, model=model: (model(b), None), hazy[idx].contiguous(), ensemble)
                    metrics.add_batch(dehazed, clear[idx].contiguous(), [CATEGORY_BY_LABEL[lab]] * int(idx.numel()))
    results = metrics.print_results()
    out_path = os.path.join(config.get("evaluation", {}).get("results_dir", "results"), "baseline_results.json")
    metrics.save_results(out_path)
    if ensemble is not None:
        _record_self_ensemble(out_path, ensemble)
    return results


def run_comprehensive_evaluation(config, steps: int = 2, use_lpips: bool = True):
    """evaluation/evaluate.py:464-540: baseline branches, the adaptive (routed) system, the detector on hazy vs dehazed frames,
    the comparison summary and `comprehensive_results.json` (same keys).  The reference indexes `['overall']['mAP']`
    unconditionally (a KeyError when nothing passed the score threshold, and its division fails for a zero hazy mAP): the
    detection block here is filled with what exists and `improvement_percent` is None in those cases.  Visualisations
    (evaluate.py:385-462) are out of scope."""
    import json
    out_dir = config.get("evaluation", {}).get("results_dir", "results")
    os.makedirs(out_dir, exist_ok=True)
    print("=" * 50 + "\nADAPTIVE FOG INTENSITY DEHAZING FRAMEWORK EVALUATION\n" + "=" * 50)
    print("\n1. Evaluating Individual Dehazing Models:\n" + "-" * 50)
    baseline = evaluate_baseline_models(config, steps=steps, use_lpips=use_lpips)
    print("\n2. Evaluating Adaptive Framework:\n" + "-" * 50)
    joint = evaluate_joint_model(config, steps=steps, use_lpips=use_lpips)
    print("\n3. Evaluating Impact on Object Detection:\n" + "-" * 50)
    det = evaluate_detection(config, steps=max(1, steps // 2))
    world, rank = _world_rank()
    if world > 1 and rank != 0:
        return None
    print("\n4. Comparison Summary:\n" + "-" * 50)
    cats = ("low_intensity", "medium_intensity", "high_intensity")

    def avg_psnr(res):
        vals = [res[c]["psnr"] for c in cats if c in res]
        return float(sum(vals) / len(vals)) if vals else float("nan")
    b_psnr, j_psnr = avg_psnr(baseline), avg_psnr(joint)
    hazy_o = (det.get("hazy") or {}).get("overall", {})
    deh_o = (det.get("dehazed") or {}).get("overall", {})
    improvement = None
    if hazy_o.get("mAP") and "mAP" in deh_o:
        improvement = (deh_o["mAP"] - hazy_o["mAP"]) / hazy_o["mAP"] * 100
    print(f"Image Quality Comparison:\n  Baseline Models Avg PSNR: {b_psnr:.2f} dB\n  Adaptive Framework Avg PSNR: {j_psnr:.2f} dB"
          f"\n  Improvement: {(j_psnr - b_psnr):.2f} dB")
    if improvement is not None:
        print(f"\nObject Detection Comparison:\n  Detection on Hazy Images mAP: {hazy_o['mAP']:.4f}\n"
              f"  Detection on Dehazed Images mAP: {deh_o['mAP']:.4f}\n  Improvement: {improvement:.2f}%")
    comprehensive = {"baseline": baseline, "joint": joint,
                     "detection": {"hazy": hazy_o, "dehazed": deh_o, "improvement_percent": improvement,
                                   "counts": det.get("counts"), "weights": det.get("weights")},
                     "comparison": {"baseline_avg_psnr": b_psnr, "joint_avg_psnr": j_psnr, "psnr_improvement": j_psnr - b_psnr}}
    with open(os.path.join(out_dir, "comprehensive_results.json"), "w") as f:
        json.dump(comprehensive, f, indent=2)
    print(f"\nComprehensive evaluation results saved to {out_dir}/comprehensive_results.json")
    return comprehensive


def fit_niqe_model(config, input: str, out_path: str):
    """`main.py --mode demo --input CLEAR_DIR --fit-niqe OUT.npz`: NIQE's pristine model (nss.NiqeModel.fit) from the
    image files of `input` -- the `clear/` folder of a dataset, say --, `demo.batch_size` files of one size at a time.  Prints
    the image and patch counts and writes the model; builds no network."""
    from .nss import NiqeModel
    if os.path.isdir(input):
        paths = sorted(os.path.join(input, f) for f in os.listdir(input) if f.lower().endswith(DEMO_EXTENSIONS))
    elif os.path.isfile(input):
        paths = [input]
    else:
        raise SystemExit(f"--input {input}: no such file or directory")
    if not paths:
        raise SystemExit(f"--input {input}: no {' / '.join('*' + e for e in DEMO_EXTENSIONS)} files")
    demo = config.get("demo") or {}
    try:
        model = NiqeModel.fit(paths, batch_size=int(demo.get("batch_size", 4)), device=config.get("device", "cuda"))
    except ValueError as e:
        raise SystemExit(f"--fit-niqe: {e}") from None
    model.save(out_path)
    print(f"NIQE model from {model.meta['images']} images, {model.meta['patches']} sharp {model.meta['patch_size']}x"
          f"{model.meta['patch_size']} patches -> {out_path}")
    return model


def run_demo(config, input: str, output: str = "demo", panels: bool = False, target: Optional[str] = None,
             self_ensemble: Optional[str] = None, exif: bool = False, ms_ssim: bool = False, detect: bool = False,
             detect_threshold: Optional[float] = None, niqe: Optional[str] = None, brisque_model: Optional[str] = None,
             brisque_range: Optional[str] = None):
    """main.py:152-217 of the reference loads every checkpoint and stops at a TODO (load sample hazy images, classify, dehaze
    through the router, visualise); this is that mode.  `input` is one image file or a directory whose *.png / *.jpg / *.jpeg /
    *.bmp files are taken; every image goes through the routed system at its own size (image_io.dehaze_files, `demo.batch_size`
    of the config at a time) and comes out as `<output>/<name>.png`, with `panels` also as `<name>_panel.png` (hazy | dehazed).
    `<output>/demo_results.json` lists file, size and routing decision per image.  Single process only.
    `target`: the ground truth, a directory (matched to the inputs by base name, image_io.pair_targets) or one file.  Every
    written file is then scored against its target -- PSNR, SSIM and CIEDE2000, and the same three for the hazy input -- the
    scores are printed and recorded per file, and `<output>/demo_scores.json` holds their means per routed intensity
    (image_io.summarize_scores).  No LPIPS here: without pretrained weights it would score with a random extractor.
    `self_ensemble` ('flip' | 'd8'; or `demo.self_ensemble` of the config): the output is the average over 4 or 8 symmetries of
    the input (d4.self_ensemble).  `exif` (or `demo.exif_orientation: true`): every file, and every target, is turned upright by
    its EXIF orientation tag first.  An argument given here wins over the config; with neither, every call is the plain one.
    `ms_ssim` (or `demo.ms_ssim: true`; needs `target`): every scored record also gains `ssim_gaussian`, `ms_ssim`,
    `hazy_ssim_gaussian` and `hazy_ms_ssim` -- the 11x11 Gaussian-window SSIM per colour channel and the five-level MS-SSIM of
    the published tables -- the printed lines show them and `demo_scores.json` their means; a file under 176 px on
    a side has `ms_ssim: null` (under 11 px `ssim_gaussian: null` too) and is left out of that mean.
    `detect` (or `demo.detect: true`): the detector of evaluate_detection (`_detector_for_evaluation`; `demo.detector` holds
    keyword arguments of DetectionModel, e.g. min_size) runs on every upright hazy input and on every written dehazed file, and the
    detections scoring above `detect_threshold` (or `demo.detect_threshold`; 0.5; within [0, 1]) are recorded per file
    (`detections`, `detect_counts`, `detect_match`: image_io.dehaze_files), printed, and drawn by the HIP overlay kernel into
    `<name>_detect.png`, the hazy | dehazed panel with both panes annotated (`demo.detect_style`: thickness, scale, alpha;
    DESIGN 4.29).  `<output>/demo_detections.json` (overlay.summarize_detections) holds the threshold, where the detector's
    weights came from, and per routed intensity and overall the file count, the mean detections per file on either side and the
    summed matched / gained / lost.  Both sides go through the detector's own transform alone: the second normalisation of
    the reference's IntegratedDetectionSystem is not applied to either, so the comparison is like for like.
    `niqe` (a model file written by `fit_niqe_model` / `--fit-niqe`; or `demo.niqe_model`): every record gains `niqe` and
    `hazy_niqe`, the no-reference NIQE score (lower is better) of the written file and of the input, null for a file
    under 96 px on a side; the scores are printed per file and `<output>/demo_noref.json` (image_io.summarize_noref) holds their
    means per routed intensity and overall.  `brisque_model` (a libsvm epsilon-SVR model file with an RBF kernel, e.g. the
    BRISQUE release's `allmodel`; or `demo.brisque_model`) with the optional svm-scale range file `brisque_range`
    (`demo.brisque_range`): `brisque` and `hazy_brisque` in the same way.  Neither needs `target`; no model file is shipped."""
    import json
    from . import image_io as IO
    if _world_rank()[0] > 1:
        raise SystemExit("--mode demo runs in a single process.  Run it without torchrun (WORLD_SIZE=1).")
    if os.path.isdir(input):
        paths = sorted(os.path.join(input, f) for f in os.listdir(input) if f.lower().endswith(DEMO_EXTENSIONS))
    elif os.path.isfile(input):
        paths = [input]
    else:
        raise SystemExit(f"--input {input}: no such file or directory")
    if not paths:
        raise SystemExit(f"--input {input}: no {' / '.join('*' + e for e in DEMO_EXTENSIONS)} files")
    if target is not None and not os.path.exists(target):
        raise SystemExit(f"--target {target}: no such file or directory")
    demo = config.get("demo") or {}
    self_ensemble = self_ensemble if self_ensemble is not None else demo.get("self_ensemble")
    exif = bool(exif or demo.get("exif_orientation"))
    if self_ensemble is not None and self_ensemble not in ("flip", "d8"):
        raise SystemExit(f"self-ensemble mode {self_ensemble!r}: choose 'flip' (x4) or 'd8' (x8)")
    ms_ssim = bool(ms_ssim or demo.get("ms_ssim"))
    if ms_ssim and target is None:                                           # before anything is built
        raise SystemExit("MS-SSIM scores against ground truth: --ms-ssim (demo.ms_ssim) needs --target")
    detect = bool(detect or demo.get("detect"))
    if detect:                                                               # before anything is built
        detect_threshold = float(detect_threshold if detect_threshold is not None else demo.get("detect_threshold", 0.5))
        if not 0.0 <= detect_threshold <= 1.0:                               # NaN fails too
            raise SystemExit(f"--detect-threshold {detect_threshold}: a detection score lies in [0, 1]")
        unknown = sorted(set(demo.get("detect_style") or {}) - {"thickness", "scale", "alpha"})
        if unknown:
            raise SystemExit(f"demo.detect_style: unknown key(s) {', '.join(unknown)} (thickness, scale, alpha)")
    elif detect_threshold is not None:
        raise SystemExit("--detect-threshold needs --detect (demo.detect)")
    niqe = niqe if niqe is not None else demo.get("niqe_model")
    brisque_model = brisque_model if brisque_model is not None else demo.get("brisque_model")
    brisque_range = brisque_range if brisque_range is not None else demo.get("brisque_range")
    noref = {}                                                               # loaded before anything is built
    if brisque_range is not None and brisque_model is None:
        raise SystemExit("--brisque-range (demo.brisque_range) needs --brisque-model (demo.brisque_model)")
    if niqe is not None or brisque_model is not None:
        from . import nss as NSS
        for what, path in (("--niqe", niqe), ("--brisque-model", brisque_model), ("--brisque-range", brisque_range)):
            if path is not None and not os.path.isfile(path):
                raise SystemExit(f"{what} {path}: no such file")
        try:
            if niqe is not None:
                noref["niqe_model"] = NSS.NiqeModel.load(niqe)
            if brisque_model is not None:
                noref["brisque_model"] = NSS.SvrModel.load(brisque_model, brisque_range)
        except ValueError as e:
            raise SystemExit(str(e)) from None
    if target is None:
        pairs = None
    else:
        pairs = IO.pair_targets(paths, target, exif=True) if exif else IO.pair_targets(paths, target)
    system, _ = _joint_system_for_evaluation(config)
    batch_size = int(demo.get("batch_size", 4))
    options = {}                                       # only what was asked for: absent options leave the call as it was
    if pairs is not None:
        options["targets"] = pairs
    if self_ensemble is not None:
        options["self_ensemble"] = self_ensemble
    if exif:
        options["exif"] = True
    if ms_ssim:
        options["ms_ssim"] = True
    if detect:
        detector, det_weights = _detector_for_evaluation(config, system["device"], **(demo.get("detector") or {}))
        options.update(detector=detector, detect_threshold=detect_threshold)
        if demo.get("detect_style"):
            options["detect_style"] = {k: int(v) for k, v in demo["detect_style"].items()}
    options.update(noref)
    results = IO.dehaze_files(system, paths, output, batch_size=batch_size, panels=panels, **options)
    for r in results:
        print(f"{r['file']}: {r['height']}x{r['width']}  {r['routing']} routing -> {r['intensity']}  weights "
              + " ".join(f"{w:.3f}" for w in r["weights"]))
        if r.get("scored"):
            db = lambda v: "inf" if v is None else f"{v:.2f}"
            print(f"    against {r['target']}: PSNR {db(r['psnr'])} dB  SSIM {r['ssim']:.4f}  CIEDE2000 {r['ciede2000']:.3f}"
                  f"   (hazy input: {db(r['hazy_psnr'])} dB  {r['hazy_ssim']:.4f}  {r['hazy_ciede2000']:.3f})")
            if ms_ssim:
                f4 = lambda v: "n/a (too small)" if v is None else f"{v:.4f}"
                print(f"    SSIM (Gaussian window) {f4(r['ssim_gaussian'])}  MS-SSIM {f4(r['ms_ssim'])}"
                      f"   (hazy input: {f4(r['hazy_ssim_gaussian'])}  {f4(r['hazy_ms_ssim'])})")
        elif pairs is not None:
            print("    not scored: " + (r.get("reason") or "no target"))
        if noref:
            nr = lambda v: "n/a" if v is None else f"{v:.3f}"
            print("    no reference: " + "  ".join(f"{label} {nr(r[k])} (hazy input: {nr(r['hazy_' + k])})"
                                                   for k, label in (("niqe", "NIQE"), ("brisque", "BRISQUE")) if k in r))
        if detect:
            c, m = r["detect_counts"], r["detect_match"]
            print(f"    detections above {detect_threshold:g}: hazy {c['hazy']}, dehazed {c['dehazed']}  (matched {m['matched']}, "
                  f"gained {m['gained']}, lost {m['lost']})")
    with open(os.path.join(output, "demo_results.json"), "w") as f:
        json.dump(results, f, indent=2)
    print(f"{len(results)} of {len(paths)} images dehazed into {output}/ (demo_results.json lists them)")
    if detect:
        from .overlay import summarize_detections
        dsum = summarize_detections(results, detect_threshold, det_weights)
        with open(os.path.join(output, "demo_detections.json"), "w") as f:
            json.dump(dsum, f, indent=2)
        a = dsum["all"]
        if a["files"]:
            print(f"detections per file: hazy {a['mean_hazy']:.2f}, dehazed {a['mean_dehazed']:.2f}; matched {a['matched']}, gained "
                  f"{a['gained']}, lost {a['lost']} over {a['files']} files (demo_detections.json; *_detect.png show them)")
    if noref:
        nsum = IO.summarize_noref(results)
        with open(os.path.join(output, "demo_noref.json"), "w") as f:
            json.dump(nsum, f, indent=2)
        for side in ("dehazed", "hazy"):
            m = nsum[side].get("all")
            if m:
                print(f"{side:>7}: " + "  ".join(f"{label} " + ("n/a" if m[k] is None else f"{m[k]:.3f}")
                                                 for k, label in (("niqe", "NIQE"), ("brisque", "BRISQUE")) if k in m)
                      + f" over {m['samples']} files (demo_noref.json)")
    if pairs is not None:
        summary = IO.summarize_scores(results)
        with open(os.path.join(output, "demo_scores.json"), "w") as f:
            json.dump(summary, f, indent=2)
        for side in ("dehazed", "hazy"):
            m = summary[side].get("all")
            if m:
                print(f"{side:>7}: {m['samples']} scored  PSNR " + ("inf" if m["psnr"] is None else f"{m['psnr']:.2f}")
                      + f" dB  SSIM {m['ssim']:.4f}  CIEDE2000 {m['ciede2000']:.3f}"
                      + ("" if not ms_ssim else "".join(
                          f"  {label} " + ("n/a" if m.get(k) is None else f"{m[k]:.4f}")
                          for k, label in (("ssim_gaussian", "SSIM (Gaussian window)"), ("ms_ssim", "MS-SSIM")))))
        print(f"{sum(1 for r in results if r.get('scored'))} of {len(results)} scored against {target} (demo_scores.json)")
    return results


def _detector_for_evaluation(config, dev, **detector_kwargs):
    """The detector of evaluate_detection and of `--mode demo --detect`, on `dev` in eval mode, and where its weights came from:
    (detector, {"detector_checkpoint": path or None, "detector_random_init": bool}).  evaluation/evaluate.py:201-227: the
    detector's own checkpoint, `detection.checkpoint_dir`/best_model.pth, when there is one; without it the detector runs on what
    it was built with, and says so.  `detector_kwargs` go to DetectionModel (e.g. min_size; `demo.detector` of the config)."""
    from .detection import DetectionModel, create_detection_model
    cfg = dict(config)
    cfg.setdefault("detection", {"model": "faster_rcnn_resnet50_fpn", "pretrained": False})
    if detector_kwargs:
        detector = DetectionModel(num_classes=91, model_name=cfg["detection"]["model"], pretrained=cfg["detection"]["pretrained"],
                                  **detector_kwargs)
    else:
        detector = create_detection_model(cfg)
    detector = detector.to(dev).eval()
    weights = {"detector_checkpoint": None}
    dck = os.path.join(str(cfg["detection"].get("checkpoint_dir", "checkpoints/detection")), "best_model.pth")
    if os.path.exists(dck):
        c = torch.load(dck, map_location="cpu")
        detector.load_state_dict(c["model_state_dict"] if "model_state_dict" in c else c)
        weights["detector_checkpoint"] = dck
        print(f"Loaded detection model from {dck}")
    else:
        print(f"Detection checkpoint {dck} not found: the detector runs on its "
              f"{'pretrained' if cfg['detection'].get('pretrained') else 'RANDOM-INIT'} weights (its detections carry no meaning then).")
    weights["detector_random_init"] = weights["detector_checkpoint"] is None and not cfg["detection"].get("pretrained")
    return detector, weights


@_rank0_only
def evaluate_detection(config, test_loader=None, steps: int = 1, score_threshold: float = 0.5, annotation_file=None):
    """Detection half of evaluation/evaluate.py:179-383 on device: the detector on the hazy frames and on the routed (dehazed)
    frames, detections with score > 0.5 (evaluate.py:327,343) converted to COCO [x, y, w, h], counted per intensity category and
    saved as `<evaluation.results_dir>/detection_results.json`.  With a COCO annotation file
    (`<dataset.test_path>/annotations/instances.json`, evaluate.py:241, or `annotation_file`) the detections go through
    `DetectionMetrics` (evaluation/metrics.py:126-270; image id = the annotation's entry for the batch's file name) and the
    per-intensity mAP tables are written to `hazy_detection_results.json` / `dehazed_detection_results.json` and compared as in
    evaluate.py:346-377.  Without one the reference writes an empty annotation file into the dataset directory and then fails in
    `loadRes` on the first detection; here that case reports the detections only."""
    import json
    from .detection import create_integrated_system, filter_detections
    from .metrics import CATEGORY_BY_LABEL, DetectionMetrics
    # evaluation/evaluate.py:201-227: the JOINT checkpoint into classifier + router + branches, and the detector's own
    # checkpoint when there is one (this used to score 'dehazed' detections with the pre-joint weights and an always
    # random-init detector).  What was used goes into the results file.
    system, joint_ck = _joint_system_for_evaluation(config)
    dev = system["device"]
    router = system["router"]
    detector, det_weights = _detector_for_evaluation(config, dev)
    weights = {"joint_checkpoint": joint_ck, **det_weights}

    class _Routed(torch.nn.Module):        # evaluate.py:262-286 process_batch: classifier -> router
        def forward(self, images):
            logits, _ = system["classifier"](images)
            return router(images, logits)
    integrated = create_integrated_system(_Routed(), detector)
    test_loader = _loader_or_synthetic(test_loader, config, steps, 910000, dev, warn="evaluate_detection", split="test")
    if annotation_file is None:
        annotation_file = os.path.join(str(config.get("dataset", {}).get("test_path", "")), "annotations", "instances.json")
    dm = None
    if os.path.exists(annotation_file):
        dm = {"hazy": DetectionMetrics(annotation_file), "dehazed": DetectionMetrics(annotation_file)}
        with open(annotation_file) as f:
            id_of = {im.get("file_name"): im["id"] for im in json.load(f).get("images", [])}
    else:
        print(f"Annotation file not found: {annotation_file}")
    short = {"low_intensity": "low", "medium_intensity": "medium", "high_intensity": "high"}
    counts = {"hazy": {}, "dehazed": {}}
    records = []
    with torch.no_grad():
        for batch in test_loader:
            hazy = batch["hazy"].to(dev)
            hazy_dets = filter_detections(detector(hazy), score_threshold)
            dehazed_raw, _ = integrated(hazy)
            dehazed_dets = filter_detections(dehazed_raw, score_threshold)
            cats = [CATEGORY_BY_LABEL.get(int(i), "high_intensity") for i in batch["intensity"].tolist()]
            for i, cat in enumerate(cats):
                for tag, dets in (("hazy", hazy_dets), ("dehazed", dehazed_dets)):
                    n = int(dets[i]["scores"].numel())
                    counts[tag][cat] = counts[tag].get(cat, 0) + n
                    for b, l, sc in zip(dets[i]["boxes_xywh"].tolist(), dets[i]["labels"].tolist(), dets[i]["scores"].tolist()):
                        records.append({"source": tag, "image_id": batch["name"][i], "category_id": int(l),
                                        "bbox": [float(v) for v in b], "score": float(sc), "intensity": cat})
                        if dm is not None:
                            dm[tag].add_detection_result(id_of.get(batch["name"][i], batch["name"][i]), int(l), b, sc, short[cat])
    out_dir = config.get("evaluation", {}).get("results_dir", "results")
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "detection_results.json"), "w") as f:
        json.dump({"score_threshold": score_threshold, "weights": weights, "counts": counts, "detections": records}, f, indent=1)
    print(f"Detections with score > {score_threshold}: hazy {counts['hazy']}, dehazed {counts['dehazed']}")
    results = {"counts": counts, "weights": weights}
    if dm is not None:
        for tag, title in (("hazy", "Hazy"), ("dehazed", "Dehazed")):
            print(f"\nObject Detection on {title} Images:")
            results[tag] = dm[tag].evaluate_by_category()
            dm[tag].print_results(results[tag]["overall"])
            dm[tag].save_results(results[tag], os.path.join(out_dir, f"{tag}_detection_results.json"))
        print("\nComparison by Fog Intensity:")
        for intensity in ("low", "medium", "high"):
            if results["hazy"].get(intensity) and results["dehazed"].get(intensity):
                hm, dmap = results["hazy"][intensity]["mAP"], results["dehazed"][intensity]["mAP"]
                print(f"\n{intensity.capitalize()} Intensity:\n  Hazy mAP: {hm:.4f}\n  Dehazed mAP: {dmap:.4f}")
                if hm != 0:
                    print(f"  Improvement: {(dmap - hm) / hm * 100:.2f}%")
    return results


# ---------------------------------------------------------------------------------------------------------------------
# Stand-alone fog-intensity classifier training (/root/reference training/train_classifier.py:13-226): Adam with the
# classifier section's lr / weight_decay, ReduceLROnPlateau(min, 0.5, patience 5) on the validation loss, cross-entropy,
# best-by-validation-accuracy checkpoint with the reference's keys, checkpoint_epoch_{5k}.pth, best model reloaded at the end.
# Accuracy and the 3 x 3 confusion matrix are counted on the device (one host read per validation pass).
# ---------------------------------------------------------------------------------------------------------------------
CLASS_NAMES = ("low", "medium", "high")


def classification_report3(cm) -> str:
    """sklearn.metrics.classification_report(target_names=['low', 'medium', 'high'], digits=2) of a confusion matrix
    (rows = true class, columns = prediction); undefined precision / recall / F1 (0 / 0) are reported as 0 as sklearn does."""
    cm = torch.as_tensor(cm, dtype=torch.float64).cpu()
    tp, support, predicted = cm.diag(), cm.sum(1), cm.sum(0)
    precision = torch.where(predicted > 0, tp / predicted.clamp(min=1), torch.zeros_like(tp))
    recall = torch.where(support > 0, tp / support.clamp(min=1), torch.zeros_like(tp))
    f1 = torch.where(precision + recall > 0, 2 * precision * recall / (precision + recall).clamp(min=1e-300), torch.zeros_like(tp))
    total = float(support.sum())
    w = support / max(total, 1.0)
    width = max(len(n) for n in CLASS_NAMES + ("weighted avg",))
    lines = [f"{'':>{width}} {'precision':>9} {'recall':>9} {'f1-score':>9} {'support':>9}", ""]
    for i, name in enumerate(CLASS_NAMES):
        lines.append(f"{name:>{width}} {float(precision[i]):9.2f} {float(recall[i]):9.2f} {float(f1[i]):9.2f} {int(support[i]):9d}")
    lines.append("")
    acc = float(tp.sum()) / max(total, 1.0)
    lines.append(f"{'accuracy':>{width}} {'':>9} {'':>9} {acc:9.2f} {int(total):9d}")
    lines.append(f"{'macro avg':>{width}} {float(precision.mean()):9.2f} {float(recall.mean()):9.2f} {float(f1.mean()):9.2f} "
                 f"{int(total):9d}")
    lines.append(f"{'weighted avg':>{width}} {float((precision * w).sum()):9.2f} {float((recall * w).sum()):9.2f} "
                 f"{float((f1 * w).sum()):9.2f} {int(total):9d}")
    return "\n".join(lines) + "\n"


def _classifier_pass(model, loader: Iterable[Dict], device, optimizer=None, ema=None) -> Dict:
    """One pass over `loader`: a training epoch when `optimizer` is given, else a no-grad evaluation.  Returns the mean
    batch loss, the confusion matrix (numpy int64 [3, 3], rows = truth) and the sample count."""
    from .loss import cross_entropy3
    loss_sum = torch.zeros((), device=device, dtype=torch.float32)
    cm = torch.zeros(9, device=device, dtype=torch.int64)
    nb = 0
    with torch.set_grad_enabled(optimizer is not None):
        for batch in loader:
            x = batch["hazy"].to(device)
            y = batch["intensity"].to(device)
            if optimizer is not None:
                optimizer.zero_grad()
            logits, _ = model(x)
            loss = cross_entropy3(logits, y)
            if optimizer is not None:
                loss.backward()
                optimizer.step()
                if ema is not None:
                    ema.update(optimizer)
            loss_sum += loss.detach().reshape(())
            cm += torch.bincount(y * 3 + logits.detach().argmax(1), minlength=9)
            nb += 1
    cmh = cm.view(3, 3).cpu().numpy()
    return {"loss": float(loss_sum) / max(nb, 1), "confusion_matrix": cmh, "count": int(cmh.sum())}


def _accuracy(cm) -> float:
    total = int(cm.sum())
    return 100.0 * int(cm.trace()) / total if total else 0.0


def train_classifier(config, train_loader=None, val_loader=None, steps: int = 4, epochs: Optional[int] = None,
                     val_steps: int = 2):
    """training/train_classifier.py:13-185.  Without loaders: `steps` / `val_steps` batches of synthetic foggy frames per
    epoch (labels = fog level).  Single process only (data-parallel classifier training is not built)."""
    if _world_rank()[0] > 1:
        raise RuntimeError("train_classifier runs in a single process; data-parallel classifier training is not implemented")
    device = torch.device(config["device"])
    cc = config["classifier"]
    model = create_classifier(config).to(device)
    optimizer = Adam(list(model.parameters()), lr=cc["learning_rate"], weight_decay=cc["weight_decay"],
                     **optim_guard_options(config))
    scheduler = ReduceLROnPlateau(optimizer, mode="min", factor=0.5, patience=5)
    ema = _weight_ema(config, model.parameters())
    ck_dir = cc["checkpoint_dir"]
    os.makedirs(ck_dir, exist_ok=True)
    epochs = cc["epochs"] if epochs is None else epochs
    if _uses_synthetic(config, device, train=train_loader, val=val_loader):
        _warn_synthetic(config, "train_classifier", _world_rank()[1])
    tr = {}

    def train_epoch(epoch):
        model.train()
        train_batches = _loader_or_synthetic(train_loader, config, steps, 0, device, epoch)
        tr.update(_classifier_pass(model, train_batches, device, optimizer, ema=ema))

    def validate():
        model.eval()
        val = _classifier_pass(model, _loader_or_synthetic(val_loader, config, val_steps, 500000, device, split="val"),
                               device)
        return {**val, "val_acc": _accuracy(val["confusion_matrix"])}

    def report(epoch, train_loss, val):
        print(f"Epoch {epoch + 1}/{epochs}:")
        print(f"  Train Loss: {tr['loss']:.4f}, Train Acc: {_accuracy(tr['confusion_matrix']):.2f}%")
        print(f"  Val Loss: {val['loss']:.4f}, Val Acc: {val['val_acc']:.2f}%")
        print(f"Confusion Matrix:\n{val['confusion_matrix']}")
        print(f"Classification Report:\n{classification_report3(val['confusion_matrix'])}")

    def checkpoint(epoch, val):
        return {"epoch": epoch, "model_state_dict": model.state_dict(), "optimizer_state_dict": optimizer.state_dict(),
                "val_acc": val["val_acc"], "val_loss": val["loss"]}

    # best starts at -1.0 (the reference starts at 0.0 and writes nothing if every epoch scores 0 %, then fails to reload)
    _run_epochs(0, epochs, train_epoch, validate, scheduler, loss_key="loss", score_key="val_acc", best=-1.0,
                score_text="accuracy: {:.2f}%", ck_dir=ck_dir, checkpoint=checkpoint, report=report, ema=ema, ema_model=model,
                ema_validate=(ema_options(config) or {}).get("validate", True))
    best_path = os.path.join(ck_dir, "best_model.pth")
    if os.path.exists(best_path):
        if _evaluate_ema(config):         # the model handed to evaluate_classifier carries the EMA weights
            load_pretrained_model(model, best_path, prefer_ema=True)
        else:
            model.load_state_dict(torch.load(best_path, map_location="cpu")["model_state_dict"])
    return model


def evaluate_classifier(model, config, test_loader=None, steps: int = 2) -> Dict:
    """training/train_classifier.py:187-226: accuracy (%), confusion matrix and the per-class report on the test split
    (synthetic frames without a loader)."""
    device = torch.device(config["device"])
    model = model.to(device).eval()
    test_loader = _loader_or_synthetic(test_loader, config, steps, 900000, device, warn="evaluate_classifier", split="test")
    res = _classifier_pass(model, test_loader, device)
    cm = res["confusion_matrix"]
    acc = _accuracy(cm)
    report = classification_report3(cm)
    print(f"Test Accuracy: {acc:.2f}%")
    print(f"Confusion Matrix:\n{cm}")
    print(f"Classification Report:\n{report}")
    return {"accuracy": acc, "confusion_matrix": cm, "classification_report": report}
