"""Shared by tests/test_gpu_loss_extractors.py and tests/test_loss_extractor_oracle_cpu.py: the cases, the float64 / fp32
oracle runs of the two loss extractors with forced kinks, and the gate  err_gpu <= 3 * err_ref + floor.

Both extractors are piecewise linear: every ReLU and every max-pool window is a kink.  A float64 run that takes the SAME
branch at every kink as the run under test (ReLU masks and pool arg-max positions forced: oracle.ref_cpu.KINK_MASKS /
POOL_INDICES) is the exact value and gradient of the piece that run evaluated; the fp32 CPU oracle forced the same way
differs from it by fp32 rounding along the same graph only, and that distance (err_ref) is the yardstick."""
import os

import torch
import torch.nn.functional as F

from oracle import ref_cpu as R
from tests._util import oracle_with_masks

LAYER_MAPPING = {"relu1_1": 2, "relu1_2": 4, "relu2_1": 7, "relu2_2": 9, "relu3_1": 12, "relu3_2": 14, "relu3_3": 16,
                 "relu4_1": 19, "relu4_2": 21, "relu4_3": 23, "relu5_1": 26, "relu5_2": 28, "relu5_3": 30}
DEFAULT_NAMES = ("relu2_2", "relu3_3", "relu4_3")
CFGS = {"vgg16": R.VGG16_CFG, "vgg19": R.VGG19_CFG}
LPIPS_POOLS = {"loss_fn.net.2": "loss_fn.net.slice1.0.weight", "loss_fn.net.5": "loss_fn.net.slice2.3.weight"}

# Floors of the gate, for tensors whose err_ref happens to be tiny, per convolution in the chain behind the tensor and relative
# to the tensor's scale.  Forward: the losses keep F(2x2,3x3) or the direct kernel there, and 4e-6 is the direct kernel's
# rounding in the project's own comparison (test_winograd_matches_direct_path).  Gradients: the data gradients run
# F(4x4,3x3), 1.2e-5 in the same comparison; never above 3e-4, the floor of test_branches_vs_reference_fixtures.
# profiles/loss_extractor_gate.txt: no forward row is above 1.6e-6 (1.4e-6 behind one convolution, the 5x5 layer: a quarter
# of its bound), the worst gradient is 1.4e-5 behind 13 convolutions and 4.5e-6 behind one (a third of its bound).
FWD_FLOOR_PER_CONV = 4e-6
GRAD_FLOOR_PER_CONV = 1.2e-5
GRAD_FLOOR_MAX = 3e-4


def fwd_floor(nconv):
    return FWD_FLOOR_PER_CONV * nconv


def grad_floor(nconv):
    return min(GRAD_FLOOR_PER_CONV * nconv, GRAD_FLOOR_MAX)


# where Gate.done() appends its rows: the file ADH_GATE_TABLE names, else the profiling scripts' output directory (git ignores
# it).  profiles/loss_extractor_gate.txt is a copy of that file after a run of tests/test_gpu_loss_extractors.py alone.
TABLE = os.environ.get("ADH_GATE_TABLE") or os.path.join("profile_out", "loss_extractor_gate.txt")


def taps_of(names):
    return sorted(LAYER_MAPPING[n] for n in names)


def vgg_convs_up_to(cfg, tap):
    """convolutions of features[:tap+1]."""
    idx = n = 0
    for v in cfg:
        if idx > tap:
            break
        if v == "M":
            idx += 1
        else:
            n += 1
            idx += 2
    return n


def vgg_pool_sources(cfg):
    """{pool index: index of the conv whose ReLU output it pools}."""
    out, idx = {}, 0
    for v in cfg:
        if v == "M":
            out[idx] = idx - 2
            idx += 1
        else:
            idx += 2
    return out


def cast_sd(sd, dtype):
    return {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in sd.items()}


def vgg_features(x, sd, taps, cfg):
    """What ContentLoss._features returns, tap by tap in ascending order: features[:tap+1] of the normalised image."""
    mean = torch.tensor(R.IMAGENET_MEAN, dtype=x.dtype).view(1, 3, 1, 1)
    std = torch.tensor(R.IMAGENET_STD, dtype=x.dtype).view(1, 3, 1, 1)
    a = (x - mean) / std
    return [R.vgg16_prefix(a, sd, i, cfg=cfg) for i in sorted(taps)]


def alex_features(x, sd):
    """What PerceptualLoss._features returns: the five relu taps of the scaled 2x-1 image."""
    shift = torch.tensor(R.LPIPS_SHIFT, dtype=x.dtype).view(1, 3, 1, 1)
    scale = torch.tensor(R.LPIPS_SCALE, dtype=x.dtype).view(1, 3, 1, 1)
    return R._alex_taps(((2 * x - 1) - shift) / scale, sd, "loss_fn.net.")


def run_forced(fn, masks, pools, audit=None):
    """fn() with the listed ReLUs and max-pools of the oracle forced to `masks` / `pools`; `audit`: the KinkAudit
    (tests/_util.py kink_audit) of these very masks and choices: a forced key it did not audit is an error."""
    if audit is not None:
        audit.covers(masks, pools=pools)
    old = R.POOL_INDICES
    R.POOL_INDICES = pools
    try:
        return oracle_with_masks(fn, masks, audit=audit)
    finally:
        R.POOL_INDICES = old


def record_kinks(fn):
    """(fn(), masks, pools): the kinks a free-running oracle pass took, in the form run_forced replays."""
    masks, pools = {}, {}
    old_relu, old_pool = R._relu, R._max_pool

    def relu(y, key):
        masks[key] = y.detach() > 0
        return old_relu(y, key)

    def pool(x, k, s, key):
        pools[key] = F.max_pool2d(x.detach(), k, s, return_indices=True)[1]
        return old_pool(x, k, s, key)
    R._relu, R._max_pool = relu, pool
    try:
        return fn(), masks, pools
    finally:
        R._relu, R._max_pool = old_relu, old_pool


def pool_choice(x_nchw, k, s):
    """arg-max positions of a max-pool over `x_nchw` with the first index in scan order on ties: the rule of adh_maxpool
    (test_maxpool_ties_and_gradient_vs_float64 pins it against this very call)."""
    return F.max_pool2d(x_nchw.double(), k, s, return_indices=True)[1]


def err_over_scale(a, ref64):
    scale = float(ref64.abs().max())
    return float((a.double() - ref64).abs().max()) / max(scale, 1e-300), scale


class Gate:
    """Collects the rows of one test: check() compares, prints and files a row; done() asserts that every row held."""

    def __init__(self, case):
        self.case, self.lines, self.bad = case, [], []

    def check(self, tensor, got, ref32, ref64, floor, entries=""):
        got, ref32, ref64 = got.detach().cpu().double(), ref32.detach().double(), ref64.detach().double()
        assert got.shape == ref64.shape == ref32.shape, (self.case, tensor, got.shape, ref64.shape)
        assert torch.isfinite(got).all(), f"{self.case} {tensor}: not finite"
        err_ref, scale = err_over_scale(ref32, ref64)
        if scale < 1e-12:      # nothing to scale by: the output has to be zero as well
            assert float(got.abs().max()) == 0.0, f"{self.case} {tensor}: reference is zero, output is not"
            return
        err_gpu, _ = err_over_scale(got, ref64)
        line = f"{self.case:44s} {tensor:10s} scale {scale:.3e}  err_ref {err_ref:.2e}  err_gpu {err_gpu:.2e}  " \
               f"bound {3 * err_ref + floor:.2e}  {entries}"
        print(line)
        self.lines.append(line)
        if not err_gpu <= 3.0 * err_ref + floor:
            self.bad.append(line)

    def done(self):
        try:
            os.makedirs(os.path.dirname(os.path.abspath(TABLE)), exist_ok=True)
            with open(TABLE, "a") as f:
                f.write("\n".join(self.lines) + "\n")
        except OSError:
            if os.environ.get("ADH_GATE_TABLE"):      # a table that was asked for by name has to be writable
                raise
        assert not self.bad, "\n".join(self.bad)
