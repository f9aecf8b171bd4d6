"""Forward/backward engine over the HIP library.

A branch forward is a sequence of fused ops on fp32 NHWC activations (`Act`); every op launches
kernels through the C ABI (`_hip.call`) and, when gradients are needed, appends a backward closure to
the tape.  `Engine.backward()` replays the tape in reverse.  torch supplies device memory, the HIP
stream and the outer autograd hook (`functional.BranchFunction`); no torch arithmetic runs here.

Reference semantics cited per op (paths under /root/reference).
"""
from __future__ import annotations

import ctypes as C
import os
import weakref
from typing import Callable, Dict, List, NamedTuple, Optional, Tuple

import torch

from . import _hip as H
from ._hip import ConvDesc, WLayout

BN_EPS = 1e-5
BN_MOMENTUM = 0.1
# Winograd F(2x2,3x3) for eligible 3x3 stride-1 convolutions and their data gradients (ADH_WINOGRAD=0 disables)
USE_WINOGRAD = os.environ.get("ADH_WINOGRAD", "1") != "0"
# F(4x4,3x3) where it applies, else F(2x2,3x3): True / False, or "fwd" / "dgrad" to restrict it to one direction
USE_WINO43 = {"0": False, "1": True}.get(os.environ.get("ADH_WINO43", "1"), os.environ.get("ADH_WINO43", "1"))
# F(4x4,3x3)-domain weight gradient (conv_wgrad43.hip, round-3 redesign: 32 x 96 channels x all 36 frequencies per workgroup):
# 2.75 / 2.50 / 2.52 ms on the 96 / 192 / 384-channel layers against 3.10 / 2.78 / 2.79 for the F(2x2,3x3)-domain kernel
#  -- the default where it applies (Cin % 32 == 0, Cout % 96 == 0); ADH_WINO43_WGRAD=0 falls back
USE_WINO43_WGRAD = os.environ.get("ADH_WINO43_WGRAD", "1") != "0"
# Contraction arithmetic of the F(4x4,3x3) forward / data-gradient launches: "fp32" = v_mfma_f32_32x32x2_f32 (default, the
# headline), "bf16x3" = v_mfma_f32_32x32x16_bf16 over exact three-plane bf16 splits of both operands (opt-in)
CONTRACT = os.environ.get("ADH_CONTRACT", "fp32")
if CONTRACT not in ("fp32", "bf16x3"):
    raise ValueError(f"ADH_CONTRACT must be 'fp32' or 'bf16x3', got {CONTRACT!r}")
W43_WGRAD_ROUNDS = int(os.environ.get("ADH_W43_WGRAD_ROUNDS", "4"))   # dev: rounds of workgroups the pixel splits may form
USE_SMALL_WGRAD = os.environ.get("ADH_SMALL_WGRAD", "1") != "0"     # conv_wgrad_small.hip for the few-channel 3x3 layers
USE_FEWOUT = os.environ.get("ADH_FEWOUT", "1") != "0"               # conv_fewout.hip for the <= 4-output-channel 3x3 heads
# BatchNorm-backward sums of a ConvBlock taken in the epilogue of its single consumer's data-gradient launch
# (adh_conv_wino43_dgrad_bnred) instead of a bn_bwd_reduce pass over the same tensor (A/B switch)
USE_BN_FUSED_REDUCE = os.environ.get("ADH_BN_FUSED_REDUCE", "1") != "0"
# the output-parity class launches of one transposed layer as one grid (adh_conv_wino32_forward_multi,
# adh_conv_wgrad_wino32_multi): one partial last round of workgroups instead of four
MERGE_CLASSES = os.environ.get("ADH_MERGE_CLASSES", "1") != "0"
# Bit-packed ReLU mask for the residual BN layers (1 bit per element written by bn_apply, read by the two backward passes
# instead of `out`): correct and tested, but measured SLOWER on MI355X (bench, ms/step: bn_apply 8.19 -> 8.47,
# bn_bwd_reduce 8.79 -> 9.85, bn_bwd_apply 12.78 -> 12.52; +1.1 ms in all): the byte loads double the number of
# vector-memory instructions of passes that were already running at 5+ TB/s.  Opt-in (ADH_RELU_BITS=1).
USE_RELU_BITS = os.environ.get("ADH_RELU_BITS", "0") != "0"
_WINO_ONLY = os.environ.get("ADH_WINOGRAD_ONLY", "")   # dev: "fwd" or "dgrad" restricts the Winograd path to one direction


def _round_up(a: int, b: int) -> int:
    return (a + b - 1) // b * b


# ---------------------------------------------------------------------------------------------------------------------
# Packed / Winograd-transformed weights are a function of the parameter only: cache them per parameter *version* so that
# the forward pass and the data gradient of one step (and every pass of an eval loop) share one pack launch.
# Key: (id, data_ptr, torch version counter, kind, layout).  torch bumps the version counter on every in-place op
# (optimizers, load_state_dict's copy_); writers that bypass it -- the HIP Adam kernel, or `p.data.op_()` -- must call
# `invalidate_weight_cache()` (optim.Adam.step does).  ADH_PACK_CACHE=0 disables the cache.
# ---------------------------------------------------------------------------------------------------------------------
USE_PACK_CACHE = os.environ.get("ADH_PACK_CACHE", "1") != "0"
_PACK_CACHE: Dict[tuple, Tuple["weakref.ref", torch.Tensor]] = {}
_PACK_CACHE_MAX = 4096


def invalidate_weight_cache() -> None:
    _PACK_CACHE.clear()


def _layout_key(L: WLayout) -> tuple:
    return (L.K, L.Nc, L.KHt, L.KWt, L.tap_off0, L.tap_off_sy, L.tap_off_sx, L.stride_k, L.stride_n)


# ---------------------------------------------------------------------------------------------------------------------
# Gradient sinks and the grad-ready hook (data-parallel training, parallel.GradientSynchronizer).
# GRAD_SINK(param) -> a preallocated contiguous tensor of the parameter's shape (a view of a flat bucket buffer) that the
# engine writes the parameter's gradient into, or None; GRAD_READY(param, grad) is called from inside Engine.backward()
# the moment the gradient is final (all of the parameter's uses in this engine have been processed), so a bucket's
# all-reduce can start while the rest of the backward pass is still running.
# ---------------------------------------------------------------------------------------------------------------------
# Test hook (tests/_util.py: kink_matched): when a dict, every fused conv(+BN)+ReLU op stores its post-activation output
# under id(weight), so a test can replay the ReLU masks this implementation actually used in the float64 oracle.  ReLU6
# layers (Engine.conv / Engine.dwconv) store theirs too: their derivative mask is 0 < out < 6.
RELU_CAPTURE: Optional[Dict[int, torch.Tensor]] = None
# test hook (tests/_util.py kink_matched): {id(AttentionBlock fc.0.weight): (global max-pool arg-max [N, C], per-pixel channel
# arg-max [N, H*W])} of every attention block run while it is a dict -- the other two kinks of the network besides the ReLUs
CBAM_CAPTURE: Optional[Dict[int, Tuple[torch.Tensor, torch.Tensor]]] = None
# Synchronised BatchNorm (parallel.GradientSynchronizer(sync_bn=True)): SYNC_BN(sums) all-reduces (SUM) the fp64 vector
# [sum(C) | second row (C) | count] of one BatchNorm layer over the ranks, in place, ordered after the kernels enqueued so far
# on the current stream; None = per-replica statistics.
SYNC_BN: Optional[Callable[[torch.Tensor], None]] = None
GRAD_SINK: Optional[Callable[[torch.Tensor], Optional[torch.Tensor]]] = None
GRAD_READY: Optional[Callable[[torch.Tensor, torch.Tensor], None]] = None


class Act:
    """An NHWC activation: `t` is a [N,H,W,C] float32 cuda tensor whose last-dim stride is 1 and whose
    pixel stride (t.stride(2)) may exceed C (channel slice of a wider buffer).  `C` is the logical
    channel count; `t.shape[3]` may be larger for the small padded tensors (3->8, 1->4 channels)."""

    __slots__ = ("t", "C", "grad", "needs_grad", "bn_src", "bn_partial")

    def __init__(self, t: torch.Tensor, C: Optional[int] = None, needs_grad: bool = True):
        assert t.dim() == 4 and t.stride(3) == 1
        self.t = t
        self.C = t.shape[3] if C is None else C
        self.grad: Optional[torch.Tensor] = None
        self.bn_src = None       # (y, {scale, shift}, mean) when this is the output of a train-mode Conv+BN+ReLU without residual
        self.bn_partial = None   # (rows, nblk, pitch, g): that layer's BN-backward sums, taken by the launch that wrote `grad`
        self.needs_grad = needs_grad

    @property
    def N(self): return self.t.shape[0]
    @property
    def Hh(self): return self.t.shape[1]
    @property
    def Ww(self): return self.t.shape[2]
    @property
    def cs(self): return self.t.stride(2)
    @property
    def pixels(self): return self.t.shape[0] * self.t.shape[1] * self.t.shape[2]


def _check_dense_pixels(t: torch.Tensor):
    # rows and images must be dense in units of the pixel stride
    cs = t.stride(2)
    assert t.stride(1) == t.shape[2] * cs and t.stride(0) == t.shape[1] * t.shape[2] * cs, "unsupported activation strides"


def new_act(N, Hh, Ww, C, device, alloc_C: Optional[int] = None, zero: bool = False) -> Act:
    ac = C if alloc_C is None else alloc_C
    t = (torch.zeros if zero else torch.empty)((N, Hh, Ww, ac), device=device, dtype=torch.float32)
    return Act(t, C)


class BNState:
    """Parameters/buffers of one BatchNorm2d, by reference to the owning module's tensors, and its eps / momentum
    (torchvision's MobileNetV3 uses 1e-3 / 0.01)."""
    __slots__ = ("weight", "bias", "running_mean", "running_var", "num_batches_tracked", "eps", "momentum")

    def __init__(self, weight, bias, running_mean, running_var, num_batches_tracked, eps: float = BN_EPS,
                 momentum: float = BN_MOMENTUM):
        self.weight, self.bias = weight, bias
        self.running_mean, self.running_var = running_mean, running_var
        self.num_batches_tracked = num_batches_tracked
        self.eps, self.momentum = eps, momentum


_SLAB_BUDGET = 1 << 30      # bytes of split-accumulation slab a weight-gradient launch may write (and its reduce kernel read)


def _rows_nsplit(groups: int, ntiles: int, cus: int = 256, max_rounds: int = 4, max_splits: Optional[int] = None,
                 slab_bytes: int = 0, tile_us: float = 5.0, launches: int = 1) -> int:
    """Pixel splits for the split-accumulating weight-gradient kernels.  One workgroup is resident per CU and every such kernel
    maps its blocks to (group, split) so that XCD x (32 CUs) gets the splits = x mod 8 of every group (csrc/common.h,
    adh_split_grid_blocks / adh_split_grid_decode: the mapping and why).  A launch therefore takes
    rounds = ceil(groups * ceil(nsplit / 8) / 32) workgroup times of ceil(ntiles / nsplit)
    tiles each -- NOT ceil(groups * nsplit / 256): groups = 3, nsplit = 85 is 255 workgroups but 33 on each of XCDs 0-4, two
    rounds (measured: Conv2d k4 s2 96 -> 192 weight gradient 5.92 ms with 85 splits, 3.69 with 80).  Every split also writes
    `slab_bytes` of partial sums that the reduce kernel reads back (80 -> 160 splits on the same layer: 3.69 -> 3.78 ms although
    the rounds * tiles product is the same).  Returns the nsplit (up to `max_rounds` rounds, at most `max_splits`) that
    minimises  launches * rounds * tiles per split * tile_us  +  nsplit * 2 * slab_bytes / (4 TB/s),  smallest on ties."""
    if os.environ.get("ADH_NSPLIT"):          # development: force the split count
        return max(1, min(ntiles, int(os.environ["ADH_NSPLIT"])))
    per_xcd = max(1, cus // 8)
    limit = max(1, min(ntiles, max_rounds * cus // max(1, groups) + 1))
    if max_splits is not None:
        limit = max(1, min(limit, max_splits))
    best, best_cost = 1, None
    for ns in range(1, limit + 1):
        rounds = -(-(groups * (-(-ns // 8))) // per_xcd)
        cost = launches * rounds * (-(-ntiles // ns)) * tile_us + ns * 2.0 * slab_bytes / 4.0e6
        if best_cost is None or cost < best_cost * (1.0 - 5e-3):
            best, best_cost = ns, cost
    return best


# ---------------------------------------------------------------------------------------------------------------------
# Kernel families of the convolution section.  Engine._select names one of _CONV per launch of a forward / data-gradient
# plan; Engine._wgrad tries _WGRAD_WINO43, _WGRAD_WINO, _WGRAD_WINO32 in turn.  Built once, here: a launch only reads them.
# ---------------------------------------------------------------------------------------------------------------------
class _ConvFamily(NamedTuple):
    pack: str                                     # pack entry point
    floats: Callable[[WLayout, int, int], int]    # packed size in floats of (layout, padded K, padded Nc)
    blocks: Optional[str]                         # query: workgroups = statistics rows of a launch; None: writes no statistics
    launch: str                                   # launch entry point
    bf16x3: bool                                  # pack and launch have a `_bf16x3` twin (CONTRACT)
    timer: Optional[str]                          # family a timer accounts the launch under, None: its own name
    exec_factor: Optional[float]                  # executed / algorithmic FLOPs, None: 1


_CONV = {
    # at most four output channels (the reconstruction heads): one pixel per thread instead of a 32-wide MFMA tile
    "fewout": _ConvFamily("adh_pack_weights_fewout", lambda L, Kp, NcP: 9 * Kp * 4, None,
                          "adh_conv_fewout_forward", False, "adh_conv_forward", None),
    # at most four input channels (data gradient of the reconstruction head, 3 -> 48): a per-pixel kernel as well
    "fewin": _ConvFamily("adh_pack_weights_fewin", lambda L, Kp, NcP: 9 * 4 * 64, "adh_conv_fewin_num_blocks",
                         "adh_conv_fewin_forward", False, "adh_conv_forward", None),
    "wino43": _ConvFamily("adh_pack_weights_wino43", lambda L, Kp, NcP: 36 * Kp * NcP, "adh_conv_wino43_num_blocks",
                          "adh_conv_wino43_forward", True, "adh_conv_wino43_forward", 0.25),
    "wino": _ConvFamily("adh_pack_weights_wino", lambda L, Kp, NcP: 16 * Kp * NcP, "adh_conv_wino_num_blocks",
                        "adh_conv_wino_forward", False, None, 4.0 / 9.0),
    # F(3x3,2x2): 2x2-tap forms (one parity class of a transposed conv / of a k4 s2 data gradient) and the k4 s2 forms as
    # four input-parity classes
    "wino32": _ConvFamily("adh_pack_weights_wino32", lambda L, Kp, NcP: (4 if L.KHt == 4 else 1) * 16 * Kp * NcP,
                          "adh_conv_wino32_num_blocks", "adh_conv_wino32_forward", True, "adh_conv_wino32_forward", 4.0 / 9.0),
    # 7x7 stem on the NHWC8 image: (kx, c)-packed 16x16x4 tiles (conv_stem.hip)
    "stem": _ConvFamily("adh_pack_weights_stem", lambda L, Kp, NcP: 7 * 24 * NcP, "adh_conv_stem_num_blocks",
                        "adh_conv_stem_forward", False, None, None),
    "igemm": _ConvFamily("adh_pack_weights", lambda L, Kp, NcP: L.KHt * L.KWt * Kp * NcP, "adh_conv_num_blocks",
                         "adh_conv_forward", False, None, None),
}


def _twin(fam: _ConvFamily) -> str:
    """Entry-point suffix of the opt-in contraction, for the families that have the twin."""
    return "_bf16x3" if fam.bf16x3 and CONTRACT == "bf16x3" else ""


class _WgradFamily(NamedTuple):
    """A weight gradient accumulated in a Winograd domain: `planes` frequency planes of KP x NcP floats per pixel split (and
    class), transformed back by the reduce kernel."""
    groups: str                   # query: workgroup groups of the launch, 0: not this family's shape
    tiles: Optional[str]          # query: tiles the pixel splits divide, None: the 4 x 32-pixel row-tile estimate
    classes: Optional[str]        # query: classes of one descriptor (a k4 s2 form has four input-parity classes), None: 1
    launches: Optional[str]       # query: launches they take (conv_wgrad32v2_kernel runs them in ONE grid: classes x groups
                                  # workgroup groups), None: 1
    planes: int
    tile_us: float                # _rows_nsplit's cost of one tile
    launch: str
    reduce: str
    exec_factor: float            # executed / algorithmic FLOPs


# 3x3 stride-1, Cin % 32 == 0, Cout % 96 == 0: the F(4x4,3x3) domain (36 frequency slabs)
_WGRAD_WINO43 = _WgradFamily("adh_conv_wgrad_wino43_groups", "adh_conv_wgrad_wino43_strips", None, None, 36, 3.6,
                             "adh_conv_wgrad_wino43", "adh_wgrad_reduce_wino43", 0.25)
# 3x3 stride-1: the F(2x2,3x3) domain (16 frequency slabs), G^T(.)G in the reduce
_WGRAD_WINO = _WgradFamily("adh_conv_wgrad_wino_groups", None, None, None, 16, 8.6,
                           "adh_conv_wgrad_wino", "adh_wgrad_reduce_wino", 4.0 / 9.0)
# the 2x2-tap forms (k4 s2 / transposed layers): the F(3x3,2x2) domain, 16 frequency slabs per class, A^T(.)A in the reduce
_WGRAD_WINO32 = _WgradFamily("adh_conv_wgrad_wino32_groups", "adh_conv_wgrad_wino32_tiles", "adh_conv_wgrad_wino32_classes",
                             "adh_conv_wgrad_wino32_launches", 16, 5.0, "adh_conv_wgrad_wino32", "adh_wgrad_reduce_wino32",
                             4.0 / 9.0)


def _forward_taps(L: WLayout, gm: dict) -> Tuple[WLayout, int, int]:
    """The 3x3 and 2x2 kernels walk their taps forwards.  A plan that walks them backwards (a data gradient, a class of a
    transposed form) is the same correlation with the filter flipped in both axes: returns the layout to pack and the
    descriptor's (dy0, dx0) for dstep = 1."""
    if gm["dstep"] == 1:
        return L, gm["dy0"], gm["dx0"]
    last = gm["KH"] - 1
    Lw = WLayout(L.K, L.Nc, gm["KH"], gm["KW"], L.tap_off0 + last * (L.tap_off_sy + L.tap_off_sx), -L.tap_off_sy,
                 -L.tap_off_sx, L.stride_k, L.stride_n)
    return Lw, gm["dy0"] - last, gm["dx0"] - last


def _set_taps(d: ConvDesc, dy0: int, dx0: int, dstep: int) -> None:
    d.dy0, d.dx0 = dy0, dx0
    d.dstep_y = d.dstep_x = dstep


def _virtual_grid(gm: dict, t: torch.Tensor) -> Tuple[int, int]:
    """(VH, VW) of one plan entry over the output (or output-gradient) tensor `t`."""
    if gm["vgrid"] == "in":   # one output-parity class of a stride-2 transposed form
        return (t.shape[1] - gm["out_o"][0] + 1) // 2, (t.shape[2] - gm["out_o"][1] + 1) // 2
    return t.shape[1], t.shape[2]


# What Engine.conv keeps of a layer for Engine._conv_backward, per mode; a bare convolution keeps nothing (None)
class _ConvTrain(NamedTuple):       # batch statistics
    y: torch.Tensor                 # raw convolution output
    mean: torch.Tensor
    invstd: torch.Tensor
    ss: torch.Tensor                # {scale, shift}
    mbits: Optional[torch.Tensor]   # bit-packed ReLU mask of a residual tail (USE_RELU_BITS)


class _ConvEval(NamedTuple):        # frozen BatchNorm folded into the convolution's epilogue
    scale: torch.Tensor


class _ConvEvalAct(NamedTuple):     # frozen statistics, BatchNorm + activation as a pass of their own
    y: torch.Tensor
    ss: torch.Tensor


class Engine:
    def __init__(self, device: torch.device, record: bool):
        self.device = device
        self.record = record
        self.tape: List[Callable[[], None]] = []
        self.param_grads: Dict[int, torch.Tensor] = {}   # id(param) -> grad
        self.params: Dict[int, torch.Tensor] = {}
        self.alias: Dict[int, int] = {}                  # id(reshaped view of a param) -> id(param)
        self.uses: Dict[int, int] = {}                   # id(param) -> uses recorded on the tape and not yet differentiated
        self.upstream: Dict[str, torch.Tensor] = {}      # 'g': device scalar cotangent of a scalar loss
        # None: follow USE_WINO43.  The loss networks set "dgrad": they difference the features of two nearly equal
        # images behind max-pools, so their forward pass keeps F(2x2,3x3) (whose rounding is below the direct kernel's)
        self.wino43: Optional[str] = None

    # ------------------------------------------------------------------ helpers
    def _f(self, *shape, zero=False):
        return (torch.zeros if zero else torch.empty)(shape, device=self.device, dtype=torch.float32)

    def _buf(self, *shape, dtype):
        """An uninitialised buffer that is not float32: int32 indices, uint8 mask bits, float64 sums, a copy of an input."""
        return torch.empty(shape, device=self.device, dtype=dtype)

    def _on_grad(self, o: Act, fn: Callable[[torch.Tensor], None], x: Optional[Act] = None):
        """Record the backward of the op that produced `o`: take and clear o.grad, and call fn(gradient) unless none
        arrived -- or unless `x`, the input the op's only gradient goes to, wants none."""
        def bwd():
            g, o.grad = o.grad, None
            if g is not None and (x is None or x.needs_grad):
                fn(g)
        self.tape.append(bwd)

    def use_param(self, *ps: Optional[torch.Tensor]):
        """Forward-side bookkeeping: each recorded op declares the parameters its backward closure will add a gradient
        for, so that `add_param_grad` knows when a gradient is final (GRAD_READY)."""
        for p in ps:
            if p is not None:
                k = self.alias.get(id(p), id(p))
                self.uses[k] = self.uses.get(k, 0) + 1

    def grad_buffer(self, p: torch.Tensor, zero: bool = False) -> torch.Tensor:
        """Where a backward closure should write the gradient of `p`: the registered sink (a view of a flat bucket
        buffer) when there is one, it has not been used by an earlier op of this engine, and `p.grad` is not already
        populated (gradient accumulation across backward passes must not alias); else a fresh tensor."""
        k = self.alias.get(id(p), id(p))
        if GRAD_SINK is not None and k == id(p) and k not in self.param_grads and getattr(p, "grad", None) is None:
            buf = GRAD_SINK(p)
            if buf is not None and buf.numel() == p.numel():
                buf = buf.view(p.shape)
                if zero:
                    buf.zero_()
                return buf
        return self._f(*p.shape, zero=zero)

    def add_param_grad(self, p: torch.Tensor, g: torch.Tensor):
        k = self.alias.get(id(p), id(p))
        if k in self.param_grads:
            H.call("adh_add_inplace", self.param_grads[k].data_ptr(), g.data_ptr(), g.numel())
        else:
            self.param_grads[k] = g
            self.params[k] = p
        left = self.uses.get(k, 1) - 1
        self.uses[k] = left
        if left == 0 and GRAD_READY is not None:
            GRAD_READY(self.params[k], self.param_grads[k])

    def accum(self, act: Act, g: torch.Tensor):
        """act.grad (+)= g ; g is [N,H,W,>=C] possibly strided."""
        if not act.needs_grad:
            return
        if act.grad is None:
            act.grad = g
        else:
            act.bn_partial = None      # the fused sums covered the first contribution only
            H.call("adh_axpby_strided", act.grad.data_ptr(), act.grad.stride(2), g.data_ptr(), g.stride(2),
                   act.pixels, _round_up(act.C, 4), 1.0, 1.0)

    def backward(self):
        while self.tape:
            self.tape.pop()()

    # ------------------------------------------------------------------ layout at the boundary
    def image_to_nhwc8(self, x: torch.Tensor) -> Act:
        N, Cc, Hh, Ww = x.shape
        assert Cc == 3
        out = self._f(N, Hh, Ww, 8)
        H.call("adh_image_to_nhwc8", x.data_ptr(), N, Hh, Ww, out.data_ptr())
        return Act(out, 8, needs_grad=False)

    def image_normalize_to_nhwc8(self, x: torch.Tensor, mean, std, holder: dict) -> Act:
        """(x - mean[c]) / std[c] -> NHWC8 (loss.py:60-66); the gradient wrt the NCHW image is left in
        holder['gx'] by the backward closure."""
        N, Cc, Hh, Ww = x.shape
        out = self._f(N, Hh, Ww, 8)
        inv = [1.0 / s_ for s_ in std]
        H.call("adh_image_normalize_to_nhwc8", x.data_ptr(), N, Hh, Ww, mean[0], mean[1], mean[2], inv[0], inv[1], inv[2],
               out.data_ptr())
        a = Act(out, 8, needs_grad=self.record)
        if self.record:
            def bwd(g):
                gx = self._buf(*x.shape, dtype=x.dtype)
                H.call("adh_image_normalize_bwd", g.data_ptr(), g.stride(2), N, Hh, Ww, inv[0], inv[1], inv[2], gx.data_ptr())
                holder["gx"] = gx
            self._on_grad(a, bwd)
        return a

    def mse(self, a: Act, b: Act, scale: float, sink: list):
        """sink.append(device scalar mean((a-b)^2) * scale) (F.mse_loss, loss.py:81); gradient flows to `a` only."""
        assert a.t.is_contiguous() and b.t.is_contiguous() and a.t.shape == b.t.shape
        n = a.t.numel()
        nblk = H.value("adh_reduce_num_blocks", n)
        partial = self._f(nblk)
        val = self._f(1)
        H.call("adh_mse_partial", a.t.data_ptr(), b.t.data_ptr(), n, partial.data_ptr())
        H.call("adh_sum_partials", partial.data_ptr(), nblk, scale / n, val.data_ptr())
        sink.append(val)
        if self.record:
            def bwd():
                up = sink_grad.get("g")
                if up is None or not a.needs_grad:
                    return
                ga = self._f(*a.t.shape)
                H.call("adh_mse_bwd", a.t.data_ptr(), b.t.data_ptr(), n, scale / n, up.data_ptr(), ga.data_ptr())
                self.accum(a, ga)
            sink_grad = self.upstream
            self.tape.append(bwd)

    # ------------------------------------------------------------------ convolution family
    @staticmethod
    def _conv_desc(x: Act, Cin: int, out_t: torch.Tensor, Cout: int, NcP: int, VH, VW, KH, KW, in_s, out_s, out_o,
                   dy0, dx0, dstep) -> ConvDesc:
        d = ConvDesc()
        d.in_ = x.t.data_ptr()
        d.N, d.IH, d.IW, d.Cin, d.in_cstride = x.N, x.Hh, x.Ww, Cin, x.cs
        d.out = out_t.data_ptr()
        d.OH, d.OW, d.Cout, d.out_cstride = out_t.shape[1], out_t.shape[2], Cout, out_t.stride(2)
        d.VH, d.VW = VH, VW
        d.in_sy = d.in_sx = in_s
        d.out_sy = d.out_sx = out_s
        d.out_oy, d.out_ox = out_o
        d.KH, d.KW = KH, KW
        d.dy0, d.dx0 = dy0, dx0
        d.dstep_y = d.dstep_x = dstep
        d.act = H.ACT_NONE
        d.NcP = NcP
        return d

    def _packed(self, fn: str, w: torch.Tensor, L: WLayout, nfloats: int) -> torch.Tensor:
        """Run the pack kernel `fn` (adh_pack_weights*) for (w, L), or return the cached result for this version of w."""
        key = None
        if USE_PACK_CACHE:
            key = (id(w), w.data_ptr(), w._version, fn, _layout_key(L), nfloats, str(w.device))
            hit = _PACK_CACHE.get(key)
            if hit is not None and hit[0]() is w:
                return hit[1]
        wp = self._f(nfloats)
        H.call(fn, w.data_ptr(), C.byref(L), wp.data_ptr())
        if key is not None:
            if len(_PACK_CACHE) >= _PACK_CACHE_MAX:
                _PACK_CACHE.clear()
            try:
                _PACK_CACHE[key] = (weakref.ref(w), wp)
            except TypeError:
                pass
        return wp

    def _pack_family(self, fam: _ConvFamily, w: torch.Tensor, L: WLayout) -> torch.Tensor:
        """Weights (w, L) packed for `fam`'s launch entry point."""
        Kp, NcP = _round_up(L.K, 8), _round_up(L.Nc, 32)
        nfloats = fam.floats(L, Kp, NcP)
        twin = _twin(fam)
        if twin:   # three bf16 planes of every fp32 value: 6 bytes instead of 4
            nfloats = nfloats * 3 // 2
        return self._packed(fam.pack + twin, w, L, nfloats)

    def _pack(self, w: torch.Tensor, L: WLayout) -> torch.Tensor:
        """Weights packed for the general kernel (adh_conv_forward)."""
        return self._pack_family(_CONV["igemm"], w, L)

    @staticmethod
    def _launch_plan(kind: str, k: int, stride: int, pad: int, w: torch.Tensor, direction: str):
        """Return a list of launches [(WLayout, geometry dict)] realising one conv layer's forward
        ('fwd'), data gradient ('dgrad') in the gather form.  Weight gradients reuse the 'fwd' plan.

        conv  : Conv2d weight [Cout,Cin,k,k], stride 1 or 2      (base_model.py:11-13)
        convT : ConvTranspose2d weight [Cin,Cout,4,4], s2 p1      (medium_intensity.py:53,63)
        geometry: in_s, out_s, out_o, dy0, dx0, dstep, KH, KW, vgrid ('out'|'in'|'out_half')
        """
        plans = []
        if kind == "conv":
            Cout, Cin = w.shape[0], w.shape[1]
            kk = k * k
            if direction == "fwd":
                L = WLayout(Cin, Cout, k, k, 0, k, 1, kk, Cin * kk)
                plans.append((L, dict(in_s=stride, out_s=1, out_o=(0, 0), dy0=-pad, dx0=-pad, dstep=1, KH=k, KW=k,
                                      vgrid="out")))
            elif stride == 1:   # dgrad of a stride-1 conv: correlation with taps walked backwards
                L = WLayout(Cout, Cin, k, k, 0, k, 1, Cin * kk, kk)
                plans.append((L, dict(in_s=1, out_s=1, out_o=(0, 0), dy0=pad, dx0=pad, dstep=-1, KH=k, KW=k,
                                      vgrid="out")))
            else:               # dgrad of a stride-2 conv = transposed-conv form, one launch per output parity
                assert stride == 2
                for py in range(2):
                    for px in range(2):
                        ky0, kx0 = (py + pad) % 2, (px + pad) % 2
                        Ty, Tx = (k - ky0 + 1) // 2, (k - kx0 + 1) // 2
                        if Ty <= 0 or Tx <= 0:
                            continue    # no tap reaches this parity class (e.g. 1x1 stride-2): gradient is zero there
                        L = WLayout(Cout, Cin, Ty, Tx, ky0 * k + kx0, 2 * k, 2, Cin * kk, kk)
                        plans.append((L, dict(in_s=1, out_s=2, out_o=(py, px), dy0=(py + pad - ky0) // 2,
                                              dx0=(px + pad - kx0) // 2, dstep=-1, KH=Ty, KW=Tx, vgrid="in")))
        else:
            assert kind == "convT" and k == 4 and stride == 2 and pad == 1
            Cin, Cout = w.shape[0], w.shape[1]
            if direction == "fwd":
                for py in range(2):
                    for px in range(2):
                        L = WLayout(Cin, Cout, 2, 2, (1 - py) * 4 + (1 - px), 8, 2, Cout * 16, 16)
                        plans.append((L, dict(in_s=1, out_s=2, out_o=(py, px), dy0=py, dx0=px, dstep=-1, KH=2, KW=2,
                                              vgrid="in")))
            else:               # dgrad of convT = k4 s2 p1 conv of the output gradient
                L = WLayout(Cout, Cin, 4, 4, 0, 4, 1, 16, Cout * 16)
                plans.append((L, dict(in_s=2, out_s=1, out_o=(0, 0), dy0=-1, dx0=-1, dstep=1, KH=4, KW=4,
                                      vgrid="out")))
        return plans

    def _select(self, L: WLayout, gm: dict, d: ConvDesc, residual, want_stats: bool, bnred) -> Tuple[_ConvFamily, WLayout]:
        """The kernel family of one plan entry and the layout to pack for it.  `d` is the entry's descriptor before the
        epilogue pointers are attached; this is the only code that writes its tap fields: a family that walks its taps
        forwards gets _forward_taps' offsets, and the plan's own come back when the family turns the shape down."""
        Kp = d.Cin
        direction = "dgrad" if gm["dstep"] == -1 else "fwd"
        k3 = gm["KH"] == 3 and gm["KW"] == 3
        # 3x3 stride 1 pad 1, forwards or backwards
        k3s1 = k3 and gm["in_s"] == 1 and gm["out_s"] == 1 and (gm["dy0"], gm["dx0"], gm["dstep"]) in ((-1, -1, 1), (1, 1, -1))
        if USE_FEWOUT and k3 and L.Nc <= 4 and residual is None and not want_stats and bnred is None and gm["dstep"] == 1 and \
                H.value("adh_conv_fewout_supported", C.byref(d)):
            return _CONV["fewout"], L
        if USE_FEWOUT and k3s1 and L.K <= 4 and Kp == 8 and 4 <= L.Nc <= 64 and L.Nc % 4 == 0 and residual is None and \
                (not want_stats or L.Nc <= 16):
            Lw, dy0, dx0 = _forward_taps(L, gm)
            _set_taps(d, dy0, dx0, 1)
            if H.value("adh_conv_fewin_supported", C.byref(d)):
                return _CONV["fewin"], Lw
            _set_taps(d, gm["dy0"], gm["dx0"], gm["dstep"])
        if USE_WINOGRAD and k3s1 and Kp % 16 == 0 and (not _WINO_ONLY or _WINO_ONLY == direction):
            Lw, dy0, dx0 = _forward_taps(L, gm)
            _set_taps(d, dy0, dx0, 1)
            w43 = USE_WINO43 if (self.wino43 is None or USE_WINO43 is not True) else self.wino43
            if (w43 is True or w43 == direction) and H.value("adh_conv_wino43_supported", C.byref(d)):
                return _CONV["wino43"], Lw
            if H.value("adh_conv_wino_supported", C.byref(d)):
                return _CONV["wino"], Lw
            _set_taps(d, gm["dy0"], gm["dx0"], gm["dstep"])
        if USE_WINOGRAD and Kp % 16 == 0 and \
                ((gm["KH"] == 2 and gm["KW"] == 2 and gm["in_s"] == 1 and gm["dstep"] in (1, -1)) or
                 (gm["KH"] == 4 and gm["KW"] == 4 and gm["in_s"] == 2 and gm["dstep"] == 1)):
            Lw, dy0, dx0 = _forward_taps(L, gm)
            _set_taps(d, dy0, dx0, 1)
            if H.value("adh_conv_wino32_supported", C.byref(d)):
                return _CONV["wino32"], Lw
            _set_taps(d, gm["dy0"], gm["dx0"], gm["dstep"])
        if gm["KH"] == 7 and L.K <= 3 and residual is None and USE_SMALL_WGRAD and \
                H.value("adh_conv_stem_num_blocks", C.byref(d)):
            return _CONV["stem"], L
        return _CONV["igemm"], L

    @staticmethod
    def _launch(fam, name: str, args: tuple, work: float):
        """`work`: algorithmic FLOPs of the launch, 2 * virtual pixels * taps * real K * real Nc (Winograd executes less)."""
        H.call(name + _twin(fam), *args, work=work, work_exec=None if fam.exec_factor is None else work * fam.exec_factor,
               family=fam.timer)

    def _run_gather(self, plans, src: Act, dst_t: torch.Tensor, dstC: int, w: torch.Tensor, scale=None, shift=None,
                    residual: Optional[torch.Tensor] = None, act=H.ACT_NONE, want_stats=False, bnred=None):
        """Launch every plan of one layer; returns (stats partials or None, number of stat rows).
        `bnred` = (y, scale_shift[2][C4], mean) of the train-mode ConvBlock that produced the tensor this data gradient is
        the gradient of: when the layer runs as ONE F(4x4,3x3) launch the producer's BatchNorm-backward sums are taken in
        its epilogue (adh_conv_wino43_dgrad_bnred) and returned as the stats rows; otherwise (None, 0) comes back and
        nothing was fused."""
        descs = []          # (descriptor, its statistics rows, family, packed weights: alive until the launch is enqueued)
        total_blocks = 0
        for L, gm in plans:
            NcP = _round_up(L.Nc, 32)
            Kp = _round_up(L.K, 8)
            assert src.t.shape[3] >= Kp or src.cs >= Kp, "input activation narrower than the padded contraction"
            VH, VW = _virtual_grid(gm, dst_t)
            d = self._conv_desc(src, Kp, dst_t, dstC, NcP, VH, VW, gm["KH"], gm["KW"], gm["in_s"], gm["out_s"],
                                gm["out_o"], gm["dy0"], gm["dx0"], gm["dstep"])
            fam, Lw = self._select(L, gm, d, residual, want_stats, bnred)
            wp = self._pack_family(fam, w, Lw)
            d.wp = wp.data_ptr()
            d.scale = H.ptr(scale)
            d.shift = H.ptr(shift)
            if residual is not None:
                d.residual = residual.data_ptr()
                d.res_cstride = residual.stride(2)
            d.act = act
            nb = H.value(fam.blocks, C.byref(d)) if fam.blocks else 0
            descs.append((d, nb, fam, wp))
            total_blocks += nb
        launch, extra = None, ()
        if bnred is not None:
            if len(descs) != 1 or descs[0][2] is not _CONV["wino43"] or residual is not None or scale is not None or \
                    shift is not None:
                bnred = None
            else:
                y_p, ss_p, mean_p = bnred
                d0 = descs[0][0]
                d0.residual, d0.res_cstride = y_p.data_ptr(), y_p.stride(2)
                d0.scale, d0.shift = ss_p[0].data_ptr(), ss_p[1].data_ptr()
                want_stats = True
                launch, extra = "adh_conv_wino43_dgrad_bnred", (mean_p.data_ptr(),)
        stats = None
        if want_stats:
            stats = self._f(total_blocks, 2, descs[0][0].NcP)
            row = 0
            for d, nb, _, _ in descs:
                d.stats = stats.data_ptr() + row * 2 * d.NcP * 4
                row += nb
        works = [2.0 * d.N * d.VH * d.VW * d.KH * d.KW * L.K * L.Nc for (d, _, _, _), (L, _) in zip(descs, plans)]
        # The output-parity classes of a transposed form are independent launches whose grids are not multiples of the CU count
        # (e.g. 1056 workgroups = 4.125 rounds of one workgroup per CU: the last round runs on 1/8 of the chip): as ONE grid
        # they have one partial last round of workgroups instead of four
        if MERGE_CLASSES and 2 <= len(descs) <= 4 and all(fam is _CONV["wino32"] and d.KH == 2 for d, _, fam, _ in descs):
            arr = (H.ConvDesc * len(descs))(*[d for d, _, _, _ in descs])
            try:
                self._launch(_CONV["wino32"], "adh_conv_wino32_forward_multi", (arr, len(descs)), sum(works))
                return stats, total_blocks
            except RuntimeError as e:
                if "unsupported" not in str(e).lower():
                    raise           # descriptors that differ in more than the class fields: one launch each, below
        for (d, _, fam, _), work in zip(descs, works):
            self._launch(fam, launch or fam.launch, (C.byref(d),) + extra, work)
        return stats, total_blocks

    def _split_slab(self, groups: int, ntiles: int, floats: int, **cost) -> Tuple[int, torch.Tensor]:
        """(nsplit, slab) of a split-accumulating weight-gradient launch: every pixel split writes `floats` partial sums."""
        nsplit = _rows_nsplit(groups, ntiles, slab_bytes=floats * 4, max_splits=max(1, _SLAB_BUDGET // (floats * 4)), **cost)
        # _rows_nsplit searches within the budget already: this binds only when ADH_NSPLIT forces the count past it
        while nsplit * floats * 4 > _SLAB_BUDGET and nsplit > 1:
            nsplit //= 2
        return nsplit, self._f(nsplit * floats)

    def _wgrad_winograd(self, fam: _WgradFamily, max_rounds: int, d: ConvDesc, L: WLayout, KP: int, dw: torch.Tensor) -> bool:
        """One plan entry's weight gradient accumulated in `fam`'s domain: pixel splits into a slab, then the reduce kernel
        sums the splits and transforms back into `dw`.  False: not the family's shape, nothing was launched."""
        groups = H.value(fam.groups, C.byref(d))
        if not groups:
            return False
        ncls = H.value(fam.classes, C.byref(d)) if fam.classes else 1
        launches = max(1, H.value(fam.launches, C.byref(d))) if fam.launches else 1
        ntiles = H.value(fam.tiles, C.byref(d)) if fam.tiles else d.N * ((d.VH + 3) // 4) * ((d.VW + 31) // 32)
        nsplit, slab = self._split_slab(groups * ncls // launches, ntiles, ncls * fam.planes * KP * d.NcP, tile_us=fam.tile_us,
                                        max_rounds=max_rounds, launches=launches)
        work = 2.0 * d.N * d.VH * d.VW * d.KH * d.KW * L.K * L.Nc
        H.call(fam.launch, C.byref(d), slab.data_ptr(), nsplit, work=work, work_exec=work * fam.exec_factor)
        of_desc = (C.byref(d),) if fam.classes else ()      # the reduce kernel of the class form reads the classes off `d`
        H.call(fam.reduce, slab.data_ptr(), nsplit, *of_desc, KP, d.NcP, C.byref(L), dw.data_ptr(), 0)
        return True

    def _wgrad(self, plans, x: Act, g_y: torch.Tensor, gC: int, w: torch.Tensor) -> torch.Tensor:
        """Weight gradient in the parameter's own layout (OIHW / IOHW)."""
        dw = self.grad_buffer(w)
        if x.C == 8 and x.cs == 8 and w.dim() == 4 and w.shape[1] <= 8 and w.shape[2] == 7 and len(plans) == 1 \
                and plans[0][1]["in_s"] == 1:
            gm = plans[0][1]
            if USE_SMALL_WGRAD and w.shape[1] <= 3:
                L = plans[0][0]
                NcP = _round_up(L.Nc, 32)
                VH, VW = g_y.shape[1], g_y.shape[2]
                d = self._conv_desc(x, 4, g_y, _round_up(gC, 4), NcP, VH, VW, 7, 7, 1, 1, (0, 0), gm["dy0"], gm["dx0"], 1)
                nslabs = H.value("adh_conv_wgrad_stem_slabs", C.byref(d))
                if nslabs:   # (kx, c)-packed 16x16x4 tiles (conv_stem.hip)
                    slab = self._f(nslabs * 49 * 8 * NcP)
                    H.call("adh_conv_wgrad_stem", C.byref(d), slab.data_ptr(), NcP,
                           work=2.0 * d.N * VH * VW * 49 * L.K * L.Nc)
                    H.call("adh_wgrad_reduce_small", slab.data_ptr(), nslabs, 8, NcP, C.byref(L), dw.data_ptr(), 0)
                    return dw
            return self._wgrad_packed_stem(gm, x, g_y, gC, w, dw)
        if MERGE_CLASSES and USE_WINOGRAD and 2 <= len(plans) <= 4 and all(gm["KH"] == 2 and gm["KW"] == 2 for _, gm in plans) \
                and self._wgrad_merged_classes(plans, x, g_y, gC, dw):
            return dw
        for L, gm in plans:
            NcP = _round_up(L.Nc, 32)
            KP = _round_up(L.K, 32)
            VH, VW = _virtual_grid(gm, g_y)
            d = self._conv_desc(x, _round_up(L.K, 4), g_y, _round_up(gC, 4), NcP, VH, VW, gm["KH"], gm["KW"], gm["in_s"],
                                gm["out_s"], gm["out_o"], gm["dy0"], gm["dx0"], gm["dstep"])
            T = gm["KH"] * gm["KW"]
            small = H.value("adh_conv_wgrad_small_slabs", C.byref(d)) if USE_SMALL_WGRAD else 0
            if small:
                # 3x3 stride-1 with few channels (guidance branch, output convolution): 16x16x4 MFMA tiles
                slab = self._f(small * 9 * KP * NcP)
                H.call("adh_conv_wgrad_small", C.byref(d), slab.data_ptr(), KP, NcP,
                       work=2.0 * d.N * d.VH * d.VW * T * L.K * L.Nc)
                H.call("adh_wgrad_reduce_small", slab.data_ptr(), small, KP, NcP, C.byref(L), dw.data_ptr(), 0)
                continue
            if USE_WINOGRAD and ((USE_WINO43_WGRAD and self._wgrad_winograd(_WGRAD_WINO43, W43_WGRAD_ROUNDS, d, L, KP, dw))
                                 or self._wgrad_winograd(_WGRAD_WINO, 4, d, L, KP, dw)
                                 or self._wgrad_winograd(_WGRAD_WINO32, 4, d, L, KP, dw)):
                continue
            # the row-split kernel (conv_wgrad_rows_kernel) where it takes the shape, else the general one: one 512-thread
            # workgroup per CU is resident, aim at ~4 rounds of 256 workgroups
            ntiles_est = x.N * ((VH + 3) // 4) * ((VW + 31) // 32)
            rows_groups = H.value("adh_conv_wgrad_groups", C.byref(d))
            if rows_groups:
                nsplit = _rows_nsplit(rows_groups, ntiles_est)
            else:
                groups = (KP // 32) * max(1, NcP // 96) * (7 if T == 49 else 1)
                nsplit = max(1, min(ntiles_est, max(1, 1024 // groups), 512))
            nslabs = H.value("adh_conv_wgrad_slabs", C.byref(d), nsplit)
            # cap the slab at 1 GiB (the slab count is the kernel's to say: not _split_slab's recipe)
            while nslabs * T * KP * NcP * 4 > _SLAB_BUDGET and nsplit > 1:
                nsplit //= 2
                nslabs = H.value("adh_conv_wgrad_slabs", C.byref(d), nsplit)
            slab = self._f(nslabs * T * KP * NcP)
            H.call("adh_conv_wgrad", C.byref(d), slab.data_ptr(), nsplit,
                   work=2.0 * d.N * d.VH * d.VW * T * L.K * L.Nc)
            H.call("adh_wgrad_reduce", slab.data_ptr(), nslabs, KP, NcP, C.byref(L), dw.data_ptr(), 0)
        return dw

    def _wgrad_merged_classes(self, plans, x: Act, g_y: torch.Tensor, gC: int, dw: torch.Tensor) -> bool:
        """The output-parity classes of a transposed layer through ONE launch of conv_wgrad32v2_kernel
        (adh_conv_wgrad_wino32_multi): classes x groups workgroup groups pack into whole rounds of the chip.  False: not its
        shapes -- the caller launches the classes one by one."""
        descs = []
        for L, gm in plans:
            VH, VW = _virtual_grid(gm, g_y)
            descs.append(self._conv_desc(x, _round_up(L.K, 4), g_y, _round_up(gC, 4), _round_up(L.Nc, 32), VH, VW, gm["KH"],
                                         gm["KW"], gm["in_s"], gm["out_s"], gm["out_o"], gm["dy0"], gm["dx0"], gm["dstep"]))
        L0 = plans[0][0]
        d0, n = descs[0], len(descs)
        KP, NcP = d0.Cin, d0.NcP
        if any(L.K != L0.K or L.Nc != L0.Nc for L, _ in plans) or KP != _round_up(L0.K, 32):
            return False
        fam = _WGRAD_WINO32
        groups = H.value(fam.groups, C.byref(d0))
        if not groups or H.value(fam.classes, C.byref(d0)) != 1:
            return False
        plane = fam.planes * KP * NcP
        nsplit, slab = self._split_slab(groups * n, H.value(fam.tiles, C.byref(d0)), n * plane, tile_us=fam.tile_us)
        arr = (H.ConvDesc * n)(*descs)
        work = sum(2.0 * dd.N * dd.VH * dd.VW * 4 * L.K * L.Nc for dd, (L, _) in zip(descs, plans))
        try:
            H.call("adh_conv_wgrad_wino32_multi", arr, n, slab.data_ptr(), nsplit, work=work, work_exec=work * fam.exec_factor,
                   family=fam.launch)
        except RuntimeError as e:
            if "unsupported" not in str(e).lower():
                raise
            return False
        for m, (L, _) in enumerate(plans):     # the splits are summed: one class plane each
            H.call(fam.reduce, slab.data_ptr() + m * plane * 4, 1, C.byref(descs[m]), KP, NcP, C.byref(L), dw.data_ptr(), 0)
        return True

    def _wgrad_packed_stem(self, gm, x: Act, g_y: torch.Tensor, gC: int, w: torch.Tensor, dw: torch.Tensor):
        """7x7 stem (Cin 3 stored as NHWC8): 4 adjacent pixels x 8 channels fill one 32-wide MFMA row tile, so a
        launch handles taps (ky, group of 4 kx) -- 14 packed taps instead of 49 mostly-empty ones."""
        Cout, Cin, KH, KW = w.shape
        NcP = _round_up(Cout, 32)
        KWg = (KW + 3) // 4
        VH, VW = g_y.shape[1], g_y.shape[2]
        d = self._conv_desc(x, 8, g_y, _round_up(gC, 4), NcP, VH, VW, KH, KWg, 1, 1, (0, 0), gm["dy0"], gm["dx0"], 1)
        d.dstep_x = 4
        ntiles_est = x.N * ((VH + 3) // 4) * ((VW + 31) // 32)
        groups = max(1, NcP // 96) * KWg
        nsplit = max(1, min(ntiles_est, max(1, 1024 // groups), 512))
        slab = self._f(nsplit * KH * KWg * 32 * NcP)
        H.call("adh_conv_wgrad", C.byref(d), slab.data_ptr(), nsplit, work=2.0 * d.N * VH * VW * KH * KW * Cin * Cout)
        H.call("adh_wgrad_reduce_packed", slab.data_ptr(), nsplit, NcP, Cin, KH, KW, Cout, dw.data_ptr(), 0)
        return dw

    # ------------------------------------------------------------------ BatchNorm sequences (bn_act.hip)
    # Every BatchNorm layer of every network -- Engine.conv, dwconv, bn_relu_preact -- folds and differentiates through these.
    def _bn_train_fold(self, bn: BNState, stats: torch.Tensor, nblk: int, pitch: int, P: int, ss: torch.Tensor):
        """Train-mode fold of the per-block sums `stats` [nblk][2][pitch] of a raw layer output over P pixels: {scale, shift}
        into ss[0] / ss[1], the running-buffer update, and (mean, invstd) for the backward pass."""
        Cc = bn.weight.numel()
        mean, invstd = self._f(Cc), self._f(Cc)
        fold = (bn.weight.data_ptr(), bn.bias.data_ptr(), bn.eps, bn.momentum, bn.running_mean.data_ptr(),
                bn.running_var.data_ptr(), ss[0].data_ptr(), ss[1].data_ptr(), mean.data_ptr(), invstd.data_ptr(),
                H.ptr(bn.num_batches_tracked))
        if SYNC_BN is not None:
            # statistics over the GLOBAL batch: local sums in fp64 -> all-reduce of 2 C + 1 doubles -> finalize
            sums = self._buf(2 * Cc + 1, dtype=torch.float64)
            H.call("adh_bn_partial_sums", stats.data_ptr(), nblk, pitch, Cc, float(P), sums.data_ptr())
            SYNC_BN(sums)
            H.call("adh_bn_finalize_sums", sums.data_ptr(), Cc, *fold)
        else:
            H.call("adh_bn_finalize", stats.data_ptr(), nblk, pitch, Cc, float(P), *fold)
        return mean, invstd

    def _bn_fold_eval(self, bn: BNState, scale: torch.Tensor, shift: Optional[torch.Tensor] = None,
                      conv_bias: Optional[torch.Tensor] = None):
        """Eval-mode fold of the running statistics with gamma / beta (and the bias of the convolution in front) into
        `scale` / `shift`.  shift=None is the invstd-only form: without gamma and beta the scale comes out as
        1 / sqrt(running_var + eps), and the shift goes to a buffer nobody reads."""
        gamma, beta = (bn.weight, bn.bias) if shift is not None else (None, None)
        if shift is None:
            shift = self._f(scale.numel())
        H.call("adh_bn_fold_eval", bn.running_mean.numel(), H.ptr(gamma), H.ptr(beta), bn.running_mean.data_ptr(),
               bn.running_var.data_ptr(), bn.eps, H.ptr(conv_bias), scale.data_ptr(), shift.data_ptr())

    def _bn_bwd_reduce(self, g: torch.Tensor, out: Optional[Act], act: int, y: torch.Tensor, mean: torch.Tensor,
                       invstd: torch.Tensor, P: int, C4: int, mask_ss: Optional[torch.Tensor] = None,
                       mbits: Optional[torch.Tensor] = None, work: float = 0.0):
        """(partial [nblk][2][C4], nblk): per-block rows of (sum m g, sum m g xhat), xhat = (y - mean) * invstd and m the
        activation's derivative -- recomputed from y with `mask_ss` = {scale, shift}, read from `mbits`, or from `out`."""
        nblk = H.value("adh_bn_bwd_num_blocks", P, C4)
        partial = self._f(nblk, 2, C4)
        H.call("adh_bn_bwd_reduce", g.data_ptr(), g.stride(2), H.ptr(out.t) if out is not None else None,
               out.cs if out is not None else 0, act, y.data_ptr(), y.stride(2), mean.data_ptr(), invstd.data_ptr(),
               partial.data_ptr(), P, C4, H.ptr(mask_ss), H.ptr(mbits), work=work)
        return partial, nblk

    def _bn_bwd_finalize(self, partial: torch.Tensor, nblk: int, P: int, C4: int, gamma: Optional[torch.Tensor],
                         invstd: torch.Tensor, dgamma: Optional[torch.Tensor], dbeta: torch.Tensor) -> torch.Tensor:
        """Sum the rows of _bn_bwd_reduce into dgamma / dbeta; returns the data-gradient coefficients [3][C4]."""
        coef = self._f(3, C4)
        H.call("adh_bn_bwd_finalize", partial.data_ptr(), nblk, C4, float(P), H.ptr(gamma), invstd.data_ptr(), H.ptr(dgamma),
               dbeta.data_ptr(), 0, coef.data_ptr())
        return coef

    def _bn_bwd_apply(self, g: torch.Tensor, out: Optional[Act], act: int, y: Optional[torch.Tensor],
                      mean: Optional[torch.Tensor], invstd: Optional[torch.Tensor], coef: torch.Tensor, train: int,
                      g_y: torch.Tensor, g_res: Optional[torch.Tensor], P: int, C4: int,
                      mask_ss: Optional[torch.Tensor] = None, mbits: Optional[torch.Tensor] = None, work: float = 0.0):
        """The data-gradient pass: g_y = the gradient at the raw layer output y, g_res = the masked gradient for a residual
        input.  train = 0: g_y = coef[0] * m * g (frozen statistics, or no BatchNorm at all with an identity row)."""
        H.call("adh_bn_bwd_apply", g.data_ptr(), g.stride(2), H.ptr(out.t) if out is not None else None,
               out.cs if out is not None else 0, act, H.ptr(y), y.stride(2) if y is not None else 0, H.ptr(mean), H.ptr(invstd),
               coef.data_ptr(), train, g_y.data_ptr(), g_y.stride(2), H.ptr(g_res), g_res.stride(2) if g_res is not None else 0,
               P, C4, H.ptr(mask_ss), H.ptr(mbits), work=work)

    def _bn_grad_buffers(self, bn: BNState, C4: int):
        """Where the finalize kernels write d-gamma / d-beta (C4 floats each): the parameters' gradient buffers when the
        channel count is a whole number of quads, else scratch the caller slices."""
        if C4 == bn.weight.numel():
            return self.grad_buffer(bn.weight), self.grad_buffer(bn.bias)
        return self._f(C4), self._f(C4)

    @staticmethod
    def _bn_bwd_reads(act: int, mask_ss, mbits) -> int:
        """Tensors a backward pass reads: g and y, and `out` when the ReLU mask can come from nowhere else."""
        return 3 if (act == H.ACT_RELU and mask_ss is None and mbits is None) else 2

    def _bn_train_coef(self, bn: BNState, g, out, act, y, mean, invstd, mask_ss, mbits, P: int, C4: int, fused=None):
        """Train-mode backward up to the data-gradient pass: the reduce (unless `fused` = (rows, nrows, pitch, .) came with g
        from the consumer's data-gradient epilogue), then the finalize.  Returns (coef, dgamma, dbeta); the caller runs its
        own data-gradient pass and then adds the parameter gradients."""
        Cc = bn.weight.numel()
        if SYNC_BN is not None:
            fused = None     # the all-reduce takes the fp64 sums of a reduce pass
        if fused is None:
            partial, nblk = self._bn_bwd_reduce(g, out, act, y, mean, invstd, P, C4, mask_ss, mbits,
                                                work=4.0 * P * Cc * self._bn_bwd_reads(act, mask_ss, mbits))
        dgamma, dbeta = self._bn_grad_buffers(bn, C4)
        if SYNC_BN is not None:
            # d-gamma / d-beta: local sums (averaged with the other gradients); the means inside the input gradient:
            # global sums (torch.nn.SyncBatchNorm's backward)
            coef = self._f(3, C4)
            loc, glob = self._buf(2 * C4 + 1, dtype=torch.float64), self._buf(2 * C4 + 1, dtype=torch.float64)
            H.call("adh_bn_partial_sums", partial.data_ptr(), nblk, C4, C4, float(P), loc.data_ptr())
            glob.copy_(loc)
            SYNC_BN(glob)
            H.call("adh_bn_bwd_finalize_sums", loc.data_ptr(), glob.data_ptr(), C4, bn.weight.data_ptr(), invstd.data_ptr(),
                   dgamma.data_ptr(), dbeta.data_ptr(), 0, coef.data_ptr())
        elif fused is not None:
            # rows of (sum g m, sum g m (y - mean))
            coef = self._f(3, C4)
            H.call("adh_bn_bwd_finalize_centered", fused[0].data_ptr(), fused[1], fused[2], C4, float(P), bn.weight.data_ptr(),
                   invstd.data_ptr(), dgamma.data_ptr(), dbeta.data_ptr(), 0, coef.data_ptr())
        else:
            coef = self._bn_bwd_finalize(partial, nblk, P, C4, bn.weight, invstd, dgamma, dbeta)
        return coef, dgamma[:Cc], dbeta[:Cc]

    def _bn_train_backward(self, bn: BNState, g, out, act, y, mean, invstd, mask_ss, mbits, g_y, g_res, P: int, C4: int,
                           fused=None):
        """Train-mode backward of out = act(BN(y) (+ residual)): _bn_train_coef, the data-gradient pass into g_y (and g_res),
        then the d-gamma / d-beta."""
        coef, dgamma, dbeta = self._bn_train_coef(bn, g, out, act, y, mean, invstd, mask_ss, mbits, P, C4, fused)
        reads = self._bn_bwd_reads(act, mask_ss, mbits) + 1 + (1 if g_res is not None else 0)     # + write g_y (+ g_res)
        self._bn_bwd_apply(g, out, act, y, mean, invstd, coef, 1, g_y, g_res, P, C4, mask_ss, mbits,
                           work=4.0 * P * bn.weight.numel() * reads)
        self.add_param_grad(bn.weight, dgamma)
        self.add_param_grad(bn.bias, dbeta)

    def _bn_frozen_param_grads(self, bn: BNState, g, out, act, y, mean, inv, P: int, C4: int, mask_ss, work: float = 0.0):
        """d-gamma / d-beta of a BatchNorm with frozen statistics and trainable gamma / beta (fine-tuning under
        module.eval()): xhat = (y - running_mean) * invstd.  `mean`: the running mean over C4 channels; `inv`: C4 floats the
        invstd is folded into.  Returns (dgamma, dbeta) for the caller to add after its data-gradient pass."""
        Cc = bn.weight.numel()
        self._bn_fold_eval(bn, inv)
        partial, nblk = self._bn_bwd_reduce(g, out, act, y, mean, inv, P, C4, mask_ss, work=work)
        dgamma, dbeta = self._bn_grad_buffers(bn, C4)
        self._bn_bwd_finalize(partial, nblk, P, C4, None, inv, dgamma, dbeta)
        return dgamma[:Cc], dbeta[:Cc]

    def _bn_act_eval_backward(self, g: torch.Tensor, y: torch.Tensor, ss: torch.Tensor, bn: BNState, act_code: int,
                              g_y: torch.Tensor, P: int, Cc: int, out: Optional[Act] = None,
                              g_res: Optional[torch.Tensor] = None):
        """Backward of out = act(y * scale + shift (+ residual)) with frozen BatchNorm statistics (scale / shift =
        ss[0] / ss[1], folded from the running estimates): g_y = scale * act'(z) * g, g_res = act'(z) * g, and d-gamma /
        d-beta when the BN parameters train.  `out`: the block output of a residual tail (NONE / RELU), whose ReLU mask is
        read from it."""
        C4 = _round_up(Cc, 4)
        coef = self._f(3, C4, zero=True)
        coef[0].copy_(ss[0])
        mask_ss = ss if (act_code != H.ACT_NONE and out is None) else None
        self._bn_bwd_apply(g, out, act_code, y, None, None, coef, 0, g_y, g_res, P, C4, mask_ss)
        if not (bn.weight.requires_grad or bn.bias.requires_grad):
            return
        mean4, inv4 = self._f(C4, zero=True), self._f(C4, zero=True)
        mean4[:Cc].copy_(bn.running_mean)
        dgamma, dbeta = self._bn_frozen_param_grads(bn, g, out, act_code, y, mean4, inv4, P, C4, mask_ss)
        self.add_param_grad(bn.weight, dgamma)
        self.add_param_grad(bn.bias, dbeta)

    def _identity_coef(self, rows: int, C4: int) -> torch.Tensor:
        """[rows][C4] coefficients of no BatchNorm at all: scale 1 in row 0, zeros below."""
        coef = self._f(rows, C4, zero=True)
        coef[0].fill_(1.0)
        return coef

    def _channel_sum(self, g: torch.Tensor, Cc: int) -> torch.Tensor:
        """sum over pixels of g[..., :Cc] (bias gradient) using the BN-backward reduction kernels: with mean = invstd = 0 and
        no mask the first row of sums is sum g, which the finalize writes as d-beta."""
        P = g.shape[0] * g.shape[1] * g.shape[2]
        C4 = _round_up(Cc, 4)
        zeros = self._f(C4, zero=True)
        partial, nblk = self._bn_bwd_reduce(g, None, H.ACT_NONE, g, zeros, zeros, P, C4)
        dbeta = self._f(C4)
        self._bn_bwd_finalize(partial, nblk, P, C4, None, zeros, None, dbeta)
        return dbeta[:Cc]

    # ------------------------------------------------------------------ ConvBlock
    def conv(self, x: Act, w: torch.Tensor, b: Optional[torch.Tensor], bn: Optional[BNState], *, kind: str = "conv",
             k: int = 3, stride: int = 1, pad: int = 1, relu: bool = True, residual: Optional[Act] = None,
             training: bool = False, out: Optional[torch.Tensor] = None, out_alloc_C: Optional[int] = None,
             act: Optional[int] = None, stats: Optional[list] = None, capture: Optional[int] = None) -> Act:
        """ConvBlock / ConvTranspose+BN+ReLU / bare Conv2d as one fused op
        (base_model.py:4-24,26-41; medium_intensity.py:52-56).  `residual` is added after BN and before the
        ReLU (ResidualBlock tail).  `out`: optional preallocated [N,OH,OW,>=Cout] view to write into.
        `act`: an H.ACT_* code, default from `relu`; ReLU6 / Hardswish / Hardsigmoid (MobileNet) need a BatchNorm and no
        residual, and run through adh_bn_apply after the raw conv in both modes.
        `stats`: a list, for a bare convolution (no BatchNorm, bias, residual or activation): the launch's epilogue also
        writes the per-block sums of its output and (partials [nblk][2][pitch], nblk, pitch) is appended (DenseNet's conv2,
        whose output is a growth slice of the block buffer).
        `capture`: the key RELU_CAPTURE files the output under when `w` is a tensor rebuilt on every call (the LPIPS stem's
        space-to-depth weights): id() of the parameter behind it; default id(w)."""
        if kind == "conv":
            Cout = w.shape[0]
            OH = (x.Hh + 2 * pad - k) // stride + 1
            OW = (x.Ww + 2 * pad - k) // stride + 1
        else:
            Cout = w.shape[1]
            OH, OW = x.Hh * 2, x.Ww * 2
        N = x.N
        act_code = act if act is not None else (H.ACT_RELU if relu else H.ACT_NONE)
        relu = act_code == H.ACT_RELU
        if act_code not in (H.ACT_NONE, H.ACT_RELU):
            assert act_code in (H.ACT_RELU6, H.ACT_HARDSWISH, H.ACT_HARDSIGMOID) and bn is not None and residual is None, \
                "MobileNet activations run after a BatchNorm, without a residual"
        if out is None:
            # channel allocation is a multiple of 8 (zero padded) so the tensor can feed the MFMA kernels
            ac = out_alloc_C if out_alloc_C is not None else _round_up(Cout, 8)
            out = self._f(N, OH, OW, ac, zero=(ac != Cout))
        _check_dense_pixels(out)
        geom = (kind, k, stride, pad)
        plans = self._launch_plan(*geom, w, "fwd")
        res_t = residual.t if residual is not None else None
        P = N * OH * OW
        apply_work = 4.0 * P * Cout * (3 if res_t is not None else 2)     # bytes: read y (+ residual), write out
        saved = None     # a bare convolution: nothing but the output is needed

        if bn is not None and training:
            # raw conv output + per-block statistics, then normalise (+residual, ReLU) in one streaming pass
            y = self._f(N, OH, OW, _round_up(Cout, 4))
            stats, nblk = self._run_gather(plans, x, y, Cout, w, shift=b, want_stats=True)
            ss = self._f(2, _round_up(Cout, 4), zero=True)   # {scale, shift}: kept for the backward ReLU mask
            mean, invstd = self._bn_train_fold(bn, stats, nblk, _round_up(Cout, 32), P, ss)
            # residual + ReLU (ResidualBlock tail): the backward ReLU mask cannot be recomputed from y alone; keep it as one
            # bit per element (1/32 of `out`) written by this pass instead of reading `out` twice in the backward pass
            mbits = None
            if USE_RELU_BITS and relu and res_t is not None and self.record and Cout % 8 == 0:
                mbits = self._buf((P * Cout + 7) // 8, dtype=torch.uint8)
            H.call("adh_bn_apply", y.data_ptr(), y.stride(2), ss[0].data_ptr(), ss[1].data_ptr(), H.ptr(res_t),
                   res_t.stride(2) if res_t is not None else 0, act_code, out.data_ptr(), out.stride(2), P, Cout, H.ptr(mbits),
                   work=apply_work)
            saved = _ConvTrain(y, mean, invstd, ss, mbits)
        elif bn is not None:
            # frozen statistics with trainable gamma / beta (fine-tuning under module.eval()): d-gamma needs
            # xhat = (y - running_mean) * invstd, which the block output cannot give back where gamma == 0, so the raw conv
            # output y is kept, as for the MobileNet activations
            bn_trains = self.record and (bn.weight.requires_grad or bn.bias.requires_grad)
            if act_code in (H.ACT_NONE, H.ACT_RELU) and not bn_trains:
                scale, shift = self._f(Cout), self._f(Cout)
                self._bn_fold_eval(bn, scale, shift, conv_bias=b)
                self._run_gather(plans, x, out, Cout, w, scale=scale, shift=shift, residual=res_t, act=act_code)
                saved = _ConvEval(scale)
            else:
                # the MFMA conv epilogues know NONE / RELU only: the raw conv (+ its bias), then the folded BN (+ residual) +
                # activation in one pass (the two passes train mode takes); y is kept for xhat and the derivative at the
                # pre-activation
                assert res_t is None or act_code in (H.ACT_NONE, H.ACT_RELU), \
                    "a MobileNet activation after a residual add is not a layer of any supported network"
                y = self._f(N, OH, OW, _round_up(Cout, 4))
                self._run_gather(plans, x, y, Cout, w, shift=b)
                ss = self._f(2, _round_up(Cout, 4), zero=True)
                self._bn_fold_eval(bn, ss[0], ss[1])
                H.call("adh_bn_apply", y.data_ptr(), y.stride(2), ss[0].data_ptr(), ss[1].data_ptr(), H.ptr(res_t),
                       res_t.stride(2) if res_t is not None else 0, act_code, out.data_ptr(), out.stride(2), P, Cout, None,
                       work=apply_work)
                saved = _ConvEvalAct(y, ss)
        elif stats is not None:
            assert b is None and res_t is None and act_code == H.ACT_NONE, "stats are taken of a bare convolution only"
            partials, nblk = self._run_gather(plans, x, out, Cout, w, want_stats=True)
            stats.append((partials, nblk, partials.shape[2]))
        else:
            self._run_gather(plans, x, out, Cout, w, shift=b, residual=res_t, act=act_code)

        o = Act(out, Cout)
        if self.record and isinstance(saved, _ConvTrain) and relu and residual is None and USE_BN_FUSED_REDUCE and \
                SYNC_BN is None:
            o.bn_src = (saved.y, saved.ss, saved.mean)
        if RELU_CAPTURE is not None and act_code in (H.ACT_RELU, H.ACT_RELU6):
            RELU_CAPTURE[id(w) if capture is None else capture] = out
        if self.record:
            # the parameters _conv_backward will produce a gradient for (must mirror its add_param_grad calls)
            bn_grads = bn is not None and (training or bn.weight.requires_grad or bn.bias.requires_grad)
            self.use_param(w if (w.requires_grad or self.alias.get(id(w)) is not None) else None, b,
                           bn.weight if bn_grads else None, bn.bias if bn_grads else None)
            self._on_grad(o, lambda g: self._conv_backward(g, x, w, b, bn, geom, act_code, residual, o, saved))
        return o

    def _conv_backward(self, g: torch.Tensor, x: Act, w, b, bn, geom, act_code, residual, o: Act, saved):
        """`geom` = (kind, k, stride, pad) of the layer; `saved`: what Engine.conv kept of its mode (_ConvTrain / _ConvEval /
        _ConvEvalAct), None for a bare convolution."""
        Cout = o.C
        C4 = _round_up(Cout, 4)
        N, OH, OW = o.N, o.Hh, o.Ww
        P = N * OH * OW
        C8 = _round_up(Cout, 8)
        g_y = self._f(N, OH, OW, C8, zero=(C8 != C4))   # padded channels must be finite zeros (dgrad reads them)
        g_res = None
        if residual is not None and residual.needs_grad:
            g_res = self._f(N, OH, OW, C4)
        if isinstance(saved, _ConvTrain):
            # without a residual the ReLU mask is recomputed from y (fma(y, scale, shift) > 0, the forward expression):
            # the two backward passes then read two tensors each instead of three
            mask_ss = saved.ss if (act_code != H.ACT_NONE and residual is None) else None
            # the sums came with g, from the consumer's data-gradient epilogue
            fused = o.bn_partial if (o.bn_partial is not None and o.bn_partial[3] is g) else None
            o.bn_partial = None
            self._bn_train_backward(bn, g, o, act_code, saved.y, saved.mean, saved.invstd, mask_ss, saved.mbits, g_y, g_res,
                                    P, C4, fused)
            if b is not None:   # a bias feeding train-mode BN has an exactly zero gradient
                self.add_param_grad(b, self._f(Cout, zero=True))
        elif isinstance(saved, _ConvEvalAct):
            # with a residual the ReLU mask cannot be recomputed from y: it is read from the block output
            self._bn_act_eval_backward(g, saved.y, saved.ss, bn, act_code, g_y, P, Cout,
                                       out=o if residual is not None else None, g_res=g_res)
            if b is not None:
                self.add_param_grad(b, self._channel_sum(g_y, Cout))
        else:
            if isinstance(saved, _ConvEval):
                coef = self._f(3, C4, zero=True)
                coef[0, :Cout].copy_(saved.scale)
            else:
                coef = self._identity_coef(3, C4)
            self._bn_bwd_apply(g, o, act_code, None, None, None, coef, 0, g_y, g_res, P, C4)
            if b is not None:
                self.add_param_grad(b, self._channel_sum(g_y, Cout))
        if g_res is not None:
            self.accum(residual, g_res)
        # weight gradient (skipped for frozen weights, e.g. the VGG16 feature extractor of the content loss)
        if w.requires_grad or self.alias.get(id(w)) is not None:
            self.add_param_grad(w, self._wgrad(self._launch_plan(*geom, w, "fwd"), x, g_y, Cout, w))
        # data gradient
        if x.needs_grad:
            plans = self._launch_plan(*geom, w, "dgrad")
            gsrc = Act(g_y, Cout)
            if x.grad is None:
                sparse = (geom[0] == "conv" and geom[2] == 2 and len(plans) < 4)
                gx = self._f(x.N, x.Hh, x.Ww, _round_up(x.C, 4), zero=sparse)
                # x = ReLU(BN(conv)) of a train-mode ConvBlock and this is the first gradient to reach it: take that BN's
                # backward sums in this launch's epilogue.  They are used only if no other gradient is added to x.grad
                # afterwards (accum / the in-place branch below drop them; the producer checks `grad is gx`).
                rows, nrows = self._run_gather(plans, gsrc, gx, x.C, w, bnred=x.bn_src if SYNC_BN is None else None)
                x.grad = gx
                x.bn_partial = (rows, nrows, _round_up(x.C, 32), gx) if rows is not None else None
            else:   # accumulate in place through the epilogue's residual input
                x.bn_partial = None
                self._run_gather(plans, gsrc, x.grad, x.C, w, residual=x.grad)

    # ------------------------------------------------------------------ attention (base_model.py:43-78)
    def attention(self, x: Act, w1: torch.Tensor, w2: torch.Tensor, wsp: torch.Tensor,
                  out: Optional[torch.Tensor] = None) -> Act:
        N, Hh, Ww, Cc = x.N, x.Hh, x.Ww, x.C
        HW = Hh * Ww
        Ch = w1.shape[0]
        nblk = H.value("adh_cbam_pool_num_blocks", HW)
        partial = self._f(N, nblk, 2, Cc)
        partial_idx = self._buf(N, nblk, Cc, dtype=torch.int32)
        pooled = self._f(N, 2, Cc)
        amax_idx = self._buf(N, Cc, dtype=torch.int32)
        xbytes = 4.0 * N * HW * Cc
        H.call("adh_cbam_pool", x.t.data_ptr(), x.cs, N, HW, Cc, partial.data_ptr(), partial_idx.data_ptr(), nblk,
               pooled.data_ptr(), amax_idx.data_ptr(), work=xbytes)
        ca = self._f(N, Cc)
        hidden = self._f(N, 2, Ch)
        H.call("adh_cbam_mlp", pooled.data_ptr(), w1.data_ptr(), w2.data_ptr(), N, Cc, Ch, ca.data_ptr(),
               hidden.data_ptr())
        smap = self._f(N, HW, 2)
        cidx = self._buf(N, HW, dtype=torch.int32)
        H.call("adh_cbam_spatial_stats", x.t.data_ptr(), x.cs, ca.data_ptr(), N, HW, Cc, smap.data_ptr(),
               cidx.data_ptr(), work=xbytes)
        sa = self._f(N, HW)
        if out is None:
            out = self._f(N, Hh, Ww, Cc)
        _check_dense_pixels(out)
        H.call("adh_cbam_apply", x.t.data_ptr(), x.cs, ca.data_ptr(), smap.data_ptr(), wsp.data_ptr(), N, Hh, Ww, Cc,
               sa.data_ptr(), out.data_ptr(), out.stride(2), work=2 * xbytes)
        o = Act(out, Cc)
        if CBAM_CAPTURE is not None:
            CBAM_CAPTURE[id(w1)] = (amax_idx, cidx)
        if self.record:
            self.use_param(wsp, w1, w2)

            def bwd(g):
                gsa_pre = self._f(N, HW)
                H.call("adh_cbam_bwd_a", g.data_ptr(), g.stride(2), x.t.data_ptr(), x.cs, ca.data_ptr(), sa.data_ptr(),
                       N, HW, Cc, gsa_pre.data_ptr(), work=2 * xbytes)
                nb = H.value("adh_cbam_bwd_b_num_blocks", N, Hh, Ww)
                gsmap = self._f(N, HW, 2)
                dwsp_partial = self._f(nb, 98)
                dwsp = self.grad_buffer(wsp)
                H.call("adh_cbam_bwd_b", gsa_pre.data_ptr(), smap.data_ptr(), wsp.data_ptr(), N, Hh, Ww,
                       gsmap.data_ptr(), dwsp_partial.data_ptr(), nb, dwsp.data_ptr(), 0)
                gca_partial = self._f(N, nblk, Cc)
                H.call("adh_cbam_bwd_c", g.data_ptr(), g.stride(2), x.t.data_ptr(), x.cs, sa.data_ptr(),
                       gsmap.data_ptr(), cidx.data_ptr(), N, HW, Cc, gca_partial.data_ptr(), nblk, work=2 * xbytes)
                gpool = self._f(N, 2, Cc)
                dw1, dw2 = self.grad_buffer(w1), self.grad_buffer(w2)
                scratch = self._f(H.value("adh_cbam_bwd_d_scratch_floats", N, Cc, Ch))
                H.call("adh_cbam_bwd_d", gca_partial.data_ptr(), nblk, ca.data_ptr(), pooled.data_ptr(),
                       hidden.data_ptr(), w1.data_ptr(), w2.data_ptr(), N, Cc, Ch, gpool.data_ptr(), dw1.data_ptr(),
                       dw2.data_ptr(), 0, scratch.data_ptr())
                self.add_param_grad(wsp, dwsp)
                self.add_param_grad(w1, dw1)
                self.add_param_grad(w2, dw2)
                if x.needs_grad:
                    gx = self._f(N, Hh, Ww, Cc)
                    H.call("adh_cbam_bwd_e", g.data_ptr(), g.stride(2), x.t.data_ptr(), x.cs, ca.data_ptr(),
                           sa.data_ptr(), gsmap.data_ptr(), cidx.data_ptr(), gpool.data_ptr(), amax_idx.data_ptr(), N,
                           HW, Cc, gx.data_ptr(), gx.stride(2), work=2 * xbytes)   # reads g, writes gx (x itself is not read)
                    self.accum(x, gx)
            self._on_grad(o, bwd)
        return o

    # ------------------------------------------------------------------ zero-copy concat
    def concat_buffer(self, N, Hh, Ww, channels: Tuple[int, ...]):
        """Allocate [N,H,W,sum(C)] and return (buffer, [slice views]) so producers write in place
        (replaces torch.cat at medium_intensity.py:100,114 / high_intensity.py:117,129)."""
        buf = self._f(N, Hh, Ww, sum(channels))
        views, o = [], 0
        for c in channels:
            views.append(buf[..., o:o + c])
            o += c
        return buf, views

    def concat(self, buf: torch.Tensor, parts: List[Act]) -> Act:
        o = Act(buf)
        offs, off = [], 0
        for p in parts:
            assert p.t.data_ptr() == buf.data_ptr() + off * 4 and p.cs == buf.shape[3], "part is not a slice of buf"
            offs.append(off)
            off += p.C
        assert off == buf.shape[3]
        if self.record:
            def bwd(g):
                for p, of in zip(parts, offs):
                    self.accum(p, g[..., of:of + p.C])
            self._on_grad(o, bwd)
        return o

    # ------------------------------------------------------------------ pooling / resize (alt models, odd sizes)
    def maxpool(self, x: Act, k: int, stride: Optional[int] = None, pad: int = 0) -> Act:
        stride = k if stride is None else stride
        N, Hh, Ww, Cc = x.N, x.Hh, x.Ww, x.C
        OH, OW = (Hh + 2 * pad - k) // stride + 1, (Ww + 2 * pad - k) // stride + 1
        out = self._f(N, OH, OW, Cc)
        idx = self._buf(N, OH, OW, Cc, dtype=torch.int32) if self.record else None
        H.call("adh_maxpool", x.t.data_ptr(), x.cs, N, Hh, Ww, Cc, k, stride, pad, out.data_ptr(), Cc, H.ptr(idx))
        o = Act(out, Cc)
        if self.record:
            def bwd(g):
                gx = self._f(N, Hh, Ww, Cc)
                H.call("adh_maxpool_bwd", g.data_ptr(), g.stride(2), idx.data_ptr(), N, OH, OW, Cc, k, stride, pad, Hh, Ww,
                       gx.data_ptr(), Cc)
                self.accum(x, gx)
            self._on_grad(o, bwd, x)
        return o

    def bilinear(self, x: Act, OH: int, OW: int, align_corners: bool, out: Optional[torch.Tensor] = None) -> Act:
        N, Hh, Ww, Cc = x.N, x.Hh, x.Ww, x.C
        if out is None:
            out = self._f(N, OH, OW, Cc)
        H.call("adh_bilinear", x.t.data_ptr(), x.cs, N, Hh, Ww, Cc, OH, OW, int(align_corners), out.data_ptr(),
               out.stride(2))
        o = Act(out, Cc)
        if self.record:
            def bwd(g):
                gx = self._f(N, Hh, Ww, Cc)
                H.call("adh_bilinear_bwd", g.data_ptr(), g.stride(2), N, Hh, Ww, Cc, OH, OW, int(align_corners),
                       gx.data_ptr(), Cc)
                self.accum(x, gx)
            self._on_grad(o, bwd, x)
        return o

    # ------------------------------------------------------------------ classifier helpers
    def global_avgpool(self, x: Act) -> Act:
        """AdaptiveAvgPool2d(1) -> [N,1,1,C] (torchvision resnet/densenet); reuses the CBAM pooling kernels."""
        N, Hh, Ww, Cc = x.N, x.Hh, x.Ww, x.C
        HW = Hh * Ww
        nblk = H.value("adh_cbam_pool_num_blocks", HW)
        means = self._f(N, Cc)
        for c0 in range(0, Cc, 1024):      # the pooling kernel takes <= 1024 channels per launch (resnet50: 2048): channel slices of x
            cw = min(1024, Cc - c0)
            partial = self._f(N, nblk, 2, cw)
            partial_idx = self._buf(N, nblk, cw, dtype=torch.int32)
            pooled = self._f(N, 2, cw)
            amax_idx = self._buf(N, cw, dtype=torch.int32)
            H.call("adh_cbam_pool", x.t.data_ptr() + 4 * c0, x.cs, N, HW, cw, partial.data_ptr(), partial_idx.data_ptr(), nblk,
                   pooled.data_ptr(), amax_idx.data_ptr())
            means[:, c0:c0 + cw] = pooled[:, 0, :]
        o = Act(means.view(N, 1, 1, Cc), Cc)   # [N,1,1,C] means
        if self.record:
            def bwd(g):
                gc = g.reshape(N, -1)[:, :Cc].contiguous()
                gx = self._f(N, Hh, Ww, Cc)
                H.call("adh_global_avgpool_bwd", gc.data_ptr(), N, HW, Cc, gx.data_ptr(), Cc)
                self.accum(x, gx)
            self._on_grad(o, bwd, x)
        return o

    def avgpool(self, x: Act, k: int) -> Act:
        """AvgPool2d(k, stride k) with floor (torchvision densenet transition); its backward exists for k = 2."""
        assert not self.record or k == 2, "avgpool backward is implemented for the 2x2 pool only"
        N, Hh, Ww, Cc = x.N, x.Hh, x.Ww, x.C
        out = self._f(N, Hh // k, Ww // k, Cc)
        H.call("adh_avgpool", x.t.data_ptr(), x.cs, N, Hh, Ww, Cc, k, out.data_ptr(), Cc)
        o = Act(out, Cc)
        if self.record:
            def bwd(g):
                C4 = _round_up(Cc, 4)
                gx = self._f(N, Hh, Ww, C4)
                H.call("adh_avgpool2_bwd", g.data_ptr(), g.stride(2), N, Hh, Ww, C4, gx.data_ptr(), C4, 0,
                       work=4.0 * (N * Hh * Ww + g.shape[0] * g.shape[1] * g.shape[2]) * Cc)   # bytes: read g, write gx
                self.accum(x, gx)
            self._on_grad(o, bwd, x)
        return o

    def bn_relu_eval(self, x: Act, bn: BNState, out: Optional[torch.Tensor] = None) -> Act:
        """Stand-alone eval-mode BatchNorm + ReLU (DenseNet's pre-activation norm layers), no gradients; with gradients or in
        train mode: bn_relu_preact."""
        assert not self.record, "bn_relu_eval records no backward: use bn_relu_preact"
        N, Hh, Ww, Cc = x.N, x.Hh, x.Ww, x.C
        scale, shift = self._f(Cc), self._f(Cc)
        self._bn_fold_eval(bn, scale, shift)
        if out is None:
            out = self._f(N, Hh, Ww, Cc)
        H.call("adh_bn_apply", x.t.data_ptr(), x.cs, scale.data_ptr(), shift.data_ptr(), None, 0, H.ACT_RELU,
               out.data_ptr(), out.stride(2), x.pixels, Cc, None)
        return Act(out, Cc)

    # ------------------------------------------------------------------ DenseNet121 training (densenet.hip)
    # A dense block's features live in one buffer [N,H,W,total] written in place; its gradient is one buffer of the same shape,
    # `sink['g']`, that every consumer of a channel slice adds into (the transition / norm5, which read every channel, write it
    # first).  Train-mode statistics are per channel and shared by every BatchNorm over the buffer: `moments` = fp64
    # (mean[total], var[total]) filled slice by slice as the block is written.
    def dense_moments(self, x: Act, moments: Tuple[torch.Tensor, torch.Tensor], c0: int,
                      partials: Optional[Tuple[torch.Tensor, int, int]] = None):
        """moments[.][c0 : c0 + x.C] = batch mean / biased variance of the channel slice x: from `partials` (a conv epilogue's
        per-block sums, Engine.conv(stats=...)) or by one adh_bn_slice_stats pass over x."""
        Cc, P = x.C, x.pixels
        if partials is None:
            nblk = H.value("adh_bn_slice_stats_num_blocks", P, Cc)
            part = self._f(nblk, 2, Cc)
            H.call("adh_bn_slice_stats", x.t.data_ptr(), x.cs, P, Cc, part.data_ptr(), work=4.0 * P * Cc)   # bytes: read x
            partials = (part, nblk, Cc)
        part, nblk, pitch = partials
        mean, var = moments
        H.call("adh_bn_slice_moments", part.data_ptr(), nblk, pitch, Cc, float(P), mean[c0:].data_ptr(), var[c0:].data_ptr())

    def dense_input(self, h: Act, buf: torch.Tensor, sink: dict) -> None:
        """Copy the block input into buf[..., :h.C]; its gradient is that slice of the block's gradient buffer."""
        H.call("adh_axpby_strided", buf.data_ptr(), buf.stride(2), h.t.data_ptr(), h.cs, h.pixels, h.C, 0.0, 1.0)
        if self.record:
            def bwd():
                if sink["g"] is not None:
                    self.accum(h, sink["g"][..., :h.C])
            self.tape.append(bwd)

    def dense_output(self, o: Act, sink: dict, c0: int) -> None:
        """`o` was written into buf[..., c0 : c0 + o.C]: before its producer's backward runs, hand it that slice of the block's
        gradient buffer (complete by then: every later reader of the slice comes later on the tape)."""
        if self.record:
            def bwd():
                if sink["g"] is not None:
                    o.grad = sink["g"][..., c0:c0 + o.C]
            self.tape.append(bwd)

    def bn_relu_preact(self, x: Act, bn: BNState, training: bool, moments: Optional[Tuple[torch.Tensor, torch.Tensor]],
                       sink: dict) -> Act:
        """DenseNet's pre-activation BatchNorm + ReLU over x = buf[..., :C] of a dense block, in train mode or with gradients
        (the no-grad eval pass is bn_relu_eval).  training: the batch statistics of `moments`, folded with this layer's gamma /
        beta (adh_bn_fold_moments, with nn.BatchNorm2d's running-buffer update); else the running statistics (frozen BN with
        trainable gamma / beta).  The output is materialised (the 1x1 convolution's weight gradient reads it).  Backward:
        the sums of (dA, x) with the ReLU mask recomputed from x and their finalize (_bn_train_coef / _bn_frozen_param_grads),
        then adh_bn_preact_bwd_accum adds d(loss)/dx into sink['g'][..., :C] at the buffer's channel stride."""
        N, Hh, Ww, Cc = x.N, x.Hh, x.Ww, x.C
        P = x.pixels
        assert Cc % 4 == 0 and x.cs % 4 == 0, "pre-activation BatchNorm needs whole channel quads"
        if training and SYNC_BN is not None:
            raise NotImplementedError("synchronised BatchNorm is not implemented for DenseNet's pre-activation BatchNorm")
        ss = self._f(2, Cc)
        mean = invstd = None
        if training:
            mean, invstd = self._f(Cc), self._f(Cc)
            H.call("adh_bn_fold_moments", Cc, moments[0].data_ptr(), moments[1].data_ptr(), float(P), bn.weight.data_ptr(),
                   bn.bias.data_ptr(), bn.eps, bn.momentum, bn.running_mean.data_ptr(), bn.running_var.data_ptr(),
                   ss[0].data_ptr(), ss[1].data_ptr(), mean.data_ptr(), invstd.data_ptr(), H.ptr(bn.num_batches_tracked))
        else:
            self._bn_fold_eval(bn, ss[0], ss[1])
        out = self._f(N, Hh, Ww, Cc)
        H.call("adh_bn_apply", x.t.data_ptr(), x.cs, ss[0].data_ptr(), ss[1].data_ptr(), None, 0, H.ACT_RELU, out.data_ptr(), Cc,
               P, Cc, None, work=8.0 * P * Cc)                                   # bytes: read x, write out
        o = Act(out, Cc)
        if RELU_CAPTURE is not None:
            RELU_CAPTURE[id(bn.weight)] = out
        if not self.record:
            return o
        bn_grads = training or bn.weight.requires_grad or bn.bias.requires_grad
        self.use_param(bn.weight if bn_grads else None, bn.bias if bn_grads else None)

        def bwd(g):
            dbuf, acc = sink["g"], 1
            if dbuf is None:   # the first writer of the block's gradient: store, and zero what it does not cover
                dbuf, acc = self._f(N, Hh, Ww, sink["C"]), 0
                if Cc < sink["C"]:
                    dbuf[..., Cc:].zero_()
                sink["g"] = dbuf
            coef = ss       # frozen statistics: dx = scale * m * dA (only row 0 is read)
            if training:
                coef, dgamma, dbeta = self._bn_train_coef(bn, g, None, H.ACT_RELU, x.t, mean, invstd, ss, None, P, Cc)
            elif bn_grads:
                dgamma, dbeta = self._bn_frozen_param_grads(bn, g, None, H.ACT_RELU, x.t, bn.running_mean.contiguous(),
                                                            self._f(Cc), P, Cc, ss, work=8.0 * P * Cc)   # bytes: dA, x
            H.call("adh_bn_preact_bwd_accum", g.data_ptr(), g.stride(2), x.t.data_ptr(), x.cs, ss.data_ptr(), H.ptr(mean),
                   H.ptr(invstd), coef.data_ptr(), int(training), dbuf.data_ptr(), dbuf.stride(2), P, Cc, acc,
                   work=4.0 * P * Cc * (4 if acc else 3))                        # bytes: dA, x (, dbuf), write dbuf
            if bn_grads:
                self.add_param_grad(bn.weight, dgamma)
                self.add_param_grad(bn.bias, dbeta)
        self._on_grad(o, bwd)
        return o

    # ------------------------------------------------------------------ MobileNetV2 / V3 (torchvision) building blocks
    def dwconv(self, x: Act, w: torch.Tensor, bn: BNState, *, k: int, stride: int, act: int, training: bool) -> Act:
        """Depthwise Conv2d(C, C, k, stride, (k-1)//2, groups=C, bias=False) -> BatchNorm2d -> act: torchvision's
        Conv2dNormActivation with groups == C (MobileNetV2 / V3).  Train mode: raw y + per-block statistics from the
        depthwise kernel, the train-mode fold, adh_bn_apply.  Eval mode: the folded BN and the activation in the kernel's
        epilogue (with gradients: the raw y is kept and adh_bn_apply runs as a pass of its own)."""
        N, Hh, Ww, Cc = x.N, x.Hh, x.Ww, x.C
        assert tuple(w.shape) == (Cc, 1, k, k) and Cc % 4 == 0, "depthwise weight must be [C,1,k,k], C % 4 == 0"
        pad = (k - 1) // 2
        OH, OW = (Hh + 2 * pad - k) // stride + 1, (Ww + 2 * pad - k) // stride + 1
        P = N * OH * OW
        wp = self._packed("adh_dwconv_pack_weights", w, WLayout(1, Cc, k, k, 0, 0, 0, 0, 0), k * k * Cc)
        ac = _round_up(Cc, 8)
        out = self._f(N, OH, OW, ac, zero=(ac != Cc))
        # algorithmic bytes of one depthwise launch: read x once, write y once
        dw_bytes = 4.0 * (N * Hh * Ww + P) * Cc
        ss = self._f(2, Cc)
        y = mean = invstd = None
        if training or self.record:     # the raw y is kept for the backward pass; the BatchNorm and the activation follow
            y = self._f(N, OH, OW, Cc)
        if training:
            nblk = H.value("adh_dwconv_num_blocks", P, Cc)
            stats = self._f(nblk, 2, Cc)
            H.call("adh_dwconv_fwd", x.t.data_ptr(), x.cs, N, Hh, Ww, Cc, k, stride, wp.data_ptr(), y.data_ptr(), Cc, OH, OW,
                   None, None, H.ACT_NONE, stats.data_ptr(), work=dw_bytes)
            mean, invstd = self._bn_train_fold(bn, stats, nblk, Cc, P, ss)
        else:
            self._bn_fold_eval(bn, ss[0], ss[1])
            if y is not None:
                H.call("adh_dwconv_fwd", x.t.data_ptr(), x.cs, N, Hh, Ww, Cc, k, stride, wp.data_ptr(), y.data_ptr(), Cc, OH,
                       OW, None, None, H.ACT_NONE, None, work=dw_bytes)
            else:
                H.call("adh_dwconv_fwd", x.t.data_ptr(), x.cs, N, Hh, Ww, Cc, k, stride, wp.data_ptr(), out.data_ptr(), ac,
                       OH, OW, ss[0].data_ptr(), ss[1].data_ptr(), act, None, work=dw_bytes)
        if y is not None:
            H.call("adh_bn_apply", y.data_ptr(), Cc, ss[0].data_ptr(), ss[1].data_ptr(), None, 0, act, out.data_ptr(), ac, P, Cc,
                   None, work=8.0 * P * Cc)
        o = Act(out, Cc)
        if RELU_CAPTURE is not None and act in (H.ACT_RELU, H.ACT_RELU6):
            RELU_CAPTURE[id(w)] = out
        # a weight gradient is produced for trainable weights and for reshaped views registered in `alias` (as in conv)
        w_grad = w.requires_grad or self.alias.get(id(w)) is not None
        if self.record:
            bn_grads = training or bn.weight.requires_grad or bn.bias.requires_grad
            self.use_param(w if w_grad else None, bn.weight if bn_grads else None, bn.bias if bn_grads else None)

            def bwd(g):
                g_y = self._f(N, OH, OW, Cc)
                if training:
                    self._bn_train_backward(bn, g, None, act, y, mean, invstd, ss if act != H.ACT_NONE else None, None, g_y,
                                            None, P, Cc)
                else:
                    self._bn_act_eval_backward(g, y, ss, bn, act, g_y, P, Cc)
                if w_grad:
                    nblk_w = H.value("adh_dwconv_wgrad_num_blocks", P, Cc)
                    partial_w = self._f(nblk_w * k * k * Cc)
                    dw = self.grad_buffer(w)
                    H.call("adh_dwconv_wgrad", x.t.data_ptr(), x.cs, N, Hh, Ww, Cc, k, stride, g_y.data_ptr(), Cc, OH, OW,
                           partial_w.data_ptr(), nblk_w, dw.data_ptr(), 0, work=dw_bytes)
                    self.add_param_grad(w, dw)
                if x.needs_grad:
                    if x.grad is None:
                        gx = self._f(N, Hh, Ww, _round_up(Cc, 4))
                        H.call("adh_dwconv_dgrad", g_y.data_ptr(), Cc, N, OH, OW, Cc, k, stride, wp.data_ptr(), gx.data_ptr(),
                               gx.stride(2), Hh, Ww, 0, work=dw_bytes)
                        x.grad = gx
                    else:   # the input has another consumer (a residual): accumulate in place
                        x.bn_partial = None
                        H.call("adh_dwconv_dgrad", g_y.data_ptr(), Cc, N, OH, OW, Cc, k, stride, wp.data_ptr(),
                               x.grad.data_ptr(), x.grad.stride(2), Hh, Ww, 1, work=dw_bytes)
            self._on_grad(o, bwd)
        return o

    def activation(self, x: Act, act: int, capture: Optional[int] = None) -> Act:
        """act(x) as a pass of its own (the squeeze-excitation gate, Hardsigmoid; the ReLU behind a tapped VGG conv):
        adh_bn_apply with scale 1, shift 0.  `capture`: key RELU_CAPTURE files a ReLU / ReLU6 output under (id() of the weight
        of the convolution in front, as Engine.conv does when it fuses the activation); None: not captured."""
        N, Hh, Ww, Cc = x.N, x.Hh, x.Ww, x.C
        C4 = _round_up(Cc, 4)
        ss = self._identity_coef(2, C4)
        out = self._f(N, Hh, Ww, C4)
        H.call("adh_bn_apply", x.t.data_ptr(), x.cs, ss[0].data_ptr(), ss[1].data_ptr(), None, 0, act, out.data_ptr(), C4,
               x.pixels, C4, None)
        o = Act(out, Cc)
        if RELU_CAPTURE is not None and capture is not None and act in (H.ACT_RELU, H.ACT_RELU6):
            RELU_CAPTURE[capture] = out
        if self.record:
            def bwd(g):
                gx = self._f(N, Hh, Ww, C4)
                self._bn_bwd_apply(g, None, act, x.t, None, None, self._identity_coef(3, C4), 0, gx, None, x.pixels, C4,
                                   ss if act != H.ACT_NONE else None)
                self.accum(x, gx)
            self._on_grad(o, bwd, x)
        return o

    def channel_scale(self, x: Act, s: Act) -> Act:
        """x[n,p,c] * s[n,c] (squeeze-excitation, torchvision SqueezeExcitation.forward); s is a [N,1,1,C] map."""
        N, Hh, Ww, Cc = x.N, x.Hh, x.Ww, x.C
        HW = Hh * Ww
        assert s.C == Cc and s.N == N and s.pixels == N and s.cs == s.t.shape[3] and s.t.shape[3] >= Cc and Cc % 4 == 0
        st = s.t.reshape(N, -1)[:, :Cc].contiguous()
        out = self._f(N, Hh, Ww, Cc)
        H.call("adh_channel_scale", x.t.data_ptr(), x.cs, st.data_ptr(), N, HW, Cc, out.data_ptr(), Cc,
               work=8.0 * N * HW * Cc)
        o = Act(out, Cc)
        if self.record:
            def bwd(g):
                nblk = H.value("adh_channel_scale_bwd_num_blocks", HW, Cc)
                partial = self._f(N * nblk * Cc)
                gs = self._f(N, 1, 1, Cc)
                gx = self._f(N, Hh, Ww, Cc) if x.needs_grad else None
                H.call("adh_channel_scale_bwd", g.data_ptr(), g.stride(2), x.t.data_ptr(), x.cs, st.data_ptr(), N, HW, Cc,
                       H.ptr(gx), Cc, partial.data_ptr(), nblk, gs.data_ptr(), work=(12.0 if gx is not None else 8.0) * N * HW * Cc)
                self.accum(s, gs)
                if gx is not None:
                    self.accum(x, gx)
            self._on_grad(o, bwd)
        return o

    def mul_mask(self, x: Act, mask: torch.Tensor) -> Act:
        """x * mask (dropout with a pre-drawn, pre-scaled mask of x's shape and strides)."""
        assert x.t.is_contiguous() and mask.shape == x.t.shape
        out = self._f(*x.t.shape)
        H.call("adh_mul", out.data_ptr(), x.t.data_ptr(), mask.data_ptr(), out.numel())
        o = Act(out, x.C)
        if self.record:
            def bwd(g):
                gx = self._f(*x.t.shape)
                H.call("adh_mul", gx.data_ptr(), g.contiguous().data_ptr(), mask.data_ptr(), gx.numel())
                self.accum(x, gx)
            self._on_grad(o, bwd, x)
        return o

    # ------------------------------------------------------------------ branch heads
    def head_blend(self, mode: int, x_img: torch.Tensor, r: Act, gd: Optional[Act], alpha: Optional[torch.Tensor]):
        """Final blend producing the NCHW output (low_intensity.py:41-45,116; medium_intensity.py:117;
        high_intensity.py:135-138,214)."""
        N, _, Hh, Ww = x_img.shape
        out = self._buf(*x_img.shape, dtype=x_img.dtype)
        H.call("adh_head_blend", mode, x_img.data_ptr(), r.t.data_ptr(), r.cs, H.ptr(gd.t if gd else None),
               gd.cs if gd else 0, H.ptr(alpha), N, Hh, Ww, out.data_ptr())
        holder = {"g": None}
        if self.record:
            if mode == 0:
                self.use_param(alpha)

            def bwd():
                g = holder["g"]
                if g is None:
                    return
                nb = H.value("adh_head_blend_bwd_num_blocks", N, Hh, Ww)
                # the kernel writes r.cs / gd.cs floats per pixel (zeros past channel 3 / 1): size by the pixel strides
                g_r = self._f(N, Hh, Ww, r.cs)
                g_gd = self._f(N, Hh, Ww, gd.cs) if gd else None
                ga_partial = self._f(nb) if mode == 0 else None
                H.call("adh_head_blend_bwd", mode, g.data_ptr(), x_img.data_ptr(), r.t.data_ptr(), r.cs,
                       H.ptr(gd.t if gd else None), gd.cs if gd else 0, H.ptr(alpha), N, Hh, Ww, g_r.data_ptr(),
                       H.ptr(g_gd), H.ptr(ga_partial), nb)
                self.accum(r, g_r)
                if gd:
                    self.accum(gd, g_gd)
                if mode == 0:
                    ga = self.grad_buffer(alpha).reshape(1)
                    H.call("adh_sum_partials", ga_partial.data_ptr(), nb, 1.0, ga.data_ptr())
                    self.add_param_grad(alpha, ga.reshape(alpha.shape))
            self.tape.append(bwd)
        return out, holder
