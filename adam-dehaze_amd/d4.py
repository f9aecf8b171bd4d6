"""The eight symmetries of the square on fp32 [N,C,H,W] batches, on the HIP kernels of csrc/d4.hip: `d4_apply`, the inverse of
every op, the EXIF orientation tags as ops, and `self_ensemble`, inference averaged over the flips (x4) or over all eight
symmetries (x8) of the input.  An op is a pair (transpose, flips): transpose first, then mirror along x if bit 0 of `flips` is set
and along y if bit 1 is (the element definition heads csrc/d4.hip)."""
from __future__ import annotations

from typing import Callable, Optional, Tuple

import torch

from . import _hip as H

D4_OPS = [(0, 0), (0, 1), (0, 2), (0, 3), (1, 0), (1, 1), (1, 2), (1, 3)]
# EXIF tag 0x0112 -> the op that turns the stored pixels upright (what PIL.ImageOps.exif_transpose does)
EXIF_TO_D4 = {1: (0, 0), 2: (0, 1), 3: (0, 3), 4: (0, 2), 5: (1, 0), 6: (1, 1), 7: (1, 3), 8: (1, 2)}
SELF_ENSEMBLE_MODES = {"flip": D4_OPS[:4], "d8": D4_OPS}


def d4_inverse(op: Tuple[int, int]) -> Tuple[int, int]:
    """The op that undoes `op`: a flip is its own inverse; behind a transpose the two mirrors change places."""
    t, f = op
    return (t, f) if not t else (1, ((f & 1) << 1) | ((f >> 1) & 1))


def exif_tag(value) -> int:
    """what a file's orientation entry means: a missing one, or anything but an integer 1..8, is 1 (upright)"""
    return value if isinstance(value, int) and not isinstance(value, bool) and 1 <= value <= 8 else 1


def d4_apply(x: torch.Tensor, op: Tuple[int, int], out: Optional[torch.Tensor] = None, accumulate: bool = False,
             scale: float = 1.0, flip_ops: Optional[torch.Tensor] = None) -> torch.Tensor:
    """`op` of float32 [N,C,H,W] `x` into `out` (a new tensor when None): [N,C,W,H] for a transposing op.  `accumulate`: out +=,
    then `scale` multiplies what is stored (one rounding each).  `flip_ops`: int32 [N] on the device, one flip code per image,
    used (masked with 3) instead of op[1]; the transpose bit is always op[0].  `out` may not overlap `x`."""
    H.require_cuda(x, "d4_apply input")
    if x.dim() != 4:
        raise ValueError(f"d4_apply input must be [N,C,H,W], got {tuple(x.shape)}")
    t, f = int(op[0]), int(op[1])
    x = x.contiguous()
    N, C, h, w = x.shape
    shape = (N, C, w, h) if t else (N, C, h, w)
    if out is None:
        if accumulate:
            raise ValueError("d4_apply: accumulate needs the tensor to accumulate into (out=)")
        out = torch.empty(shape, device=x.device, dtype=torch.float32)
    else:
        H.require_cuda(out, "d4_apply output")
        if tuple(out.shape) != shape or not out.is_contiguous():
            raise ValueError(f"d4_apply: output must be dense {shape}, got {tuple(out.shape)} with strides {out.stride()}")
    if flip_ops is not None:
        if not flip_ops.is_cuda or flip_ops.dtype != torch.int32 or tuple(flip_ops.shape) != (N,) or not flip_ops.is_contiguous():
            raise ValueError(f"d4_apply: flip_ops must be a dense int32 [{N}] on the device, got {flip_ops.dtype} "
                             f"{tuple(flip_ops.shape)} on {flip_ops.device}")
    H.call("adh_d4_apply", x.data_ptr(), N, C, h, w, t, f, H.ptr(flip_ops), out.data_ptr(), int(bool(accumulate)), float(scale))
    return out


def self_ensemble(fn: Callable, x: torch.Tensor, mode: str):
    """`fn` (a batch -> (batch, aux)) averaged over the symmetries of its input: for every op k of the mode ('flip': the first four
    of D4_OPS, 'd8': all eight), in list order, y_k = d4_apply(fn(d4_apply(x, op_k))[0], d4_inverse(op_k)), and the result is
    (((y_0 + y_1) + ...) + y_last) * (1 / len) in exactly that order; 1/4 and 1/8 are exact, so it is reproducible bit for bit.
    The upright pass takes `x` itself, and the scale rides on the last accumulating launch.  Returns (y, aux of the upright
    pass).  No gradient."""
    if mode not in SELF_ENSEMBLE_MODES:
        raise ValueError(f"self_ensemble mode must be one of {sorted(SELF_ENSEMBLE_MODES)}, got {mode!r}")
    ops = SELF_ENSEMBLE_MODES[mode]
    with torch.no_grad():
        y0, aux = fn(x)
        acc = d4_apply(y0, ops[0])              # a buffer of our own: fn may hand out the same storage on its next call
        for k, op in enumerate(ops[1:], 1):
            yk = fn(d4_apply(x, op))[0]
            d4_apply(yk, d4_inverse(op), out=acc, accumulate=True, scale=1.0 / len(ops) if k == len(ops) - 1 else 1.0)
    return acc, aux
