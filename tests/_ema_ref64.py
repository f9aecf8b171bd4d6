"""Float64 restatement of the weight EMA (include/adam_dehaze_hip.h: adh_ema_begin, adh_ema_multi), from the definitions and
not from the kernel, for tests/test_gpu_ema.py and tests/test_ema_hostemu_cpu.py.

    begin   guard given and guard.finite == 0:  active = 0, updates unchanged
            otherwise                           updates += 1, active = 1,
                                                d = min(decay, (1 + updates) / (10 + updates)) with warm-up, else decay,
                                                w = float32(1 - d)        (double arithmetic, rounded to float once)
    multi   active == 0: nothing; otherwise     ema = ema + w * (p - ema) per element

Bound of one update: the kernel evaluates p - ema, w * (.), ema + (.) in fp32: three roundings of quantities no larger than
|p| + |ema| (w <= 1), so |kernel - float64| <= 4 * 2^-24 * (|p| + |ema|) per element with the float w the reference itself
computes.  K chained updates: at most K times that on the running maxima of |p| and |ema| over the trajectory (an update is
a convex combination, it does not amplify an earlier error).
"""
import numpy as np
import torch

EPS = 2.0 ** -24
UNITS = 4


def begin(updates: int, decay: float, warmup: bool, guard_finite=None):
    """-> (updates, active, w as np.float32 or None when inactive)"""
    if guard_finite is not None and guard_finite == 0:
        return updates, 0, None
    updates += 1
    d = min(decay, (1.0 + updates) / (10.0 + updates)) if warmup else decay
    return updates, 1, np.float32(1.0 - d)


def blend(p: torch.Tensor, ema: torch.Tensor, w) -> torch.Tensor:
    """one update in float64 with the float weight `w`"""
    p, ema = p.detach().double().cpu(), ema.detach().double().cpu()
    return ema + float(w) * (p - ema)


def bound(p_abs_max: torch.Tensor, ema_abs_max: torch.Tensor, k: int = 1) -> torch.Tensor:
    """per-element bound after k chained updates; the arguments are the running maxima of |p| and |ema| (float64)"""
    return k * UNITS * EPS * (p_abs_max.double().cpu() + ema_abs_max.double().cpu())


class Trajectory:
    """K chained updates of one tensor in float64 with the running maxima its bound needs."""

    def __init__(self, ema0: torch.Tensor):
        self.ema = ema0.detach().double().cpu().clone()
        self.ema_max = self.ema.abs()
        self.p_max = torch.zeros_like(self.ema)
        self.k = 0

    def step(self, p: torch.Tensor, w) -> None:
        p = p.detach().double().cpu()
        self.p_max = torch.maximum(self.p_max, p.abs())
        self.ema = blend(p, self.ema, w)
        self.ema_max = torch.maximum(self.ema_max, self.ema.abs())
        self.k += 1

    def bound(self) -> torch.Tensor:
        return bound(self.p_max, self.ema_max, self.k)


# The tensors both test files run: (floats, offset of p, offset of ema in floats from a 16-byte-aligned address, scale of the
# N(0, 1) values).  1, 3: below one quad; 4: one quad, no tail; 1021: quads and a tail, both pointers off alignment (scalar
# path); chunk: exactly one workgroup; chunk + 1: a second workgroup with one element, only ema off alignment; 2 chunk + 7:
# three workgroups with a tail.
CHUNK = 16384
TENSORS = [(1, 0, 0, 1.0), (3, 0, 0, 1e3), (4, 0, 0, 1e-3), (1021, 1, 1, 1.0), (CHUNK, 0, 0, 1e-3), (CHUNK + 1, 0, 1, 1e3),
           (2 * CHUNK + 7, 0, 0, 1.0)]


def inputs(seed: int):
    """[(p, ema)] fp32 CPU tensors for TENSORS"""
    g = torch.Generator().manual_seed(seed)
    return [(torch.randn(n, generator=g) * s, torch.randn(n, generator=g) * s) for n, _, _, s in TENSORS]
