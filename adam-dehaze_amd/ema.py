"""Exponential moving average (EMA) of the weights on the device, next to the fused Adam step (csrc/ema.hip).

`WeightEMA(params, decay, warmup)` keeps one fp32 shadow tensor per UNIQUE floating-point parameter.  `update(optimizer)`,
called right after `optimizer.step()`, is two launches on the current stream and never reads back:

* `adh_ema_begin` (one workgroup) advances a 16-byte control block on the device: it counts the update and computes the blend
  weight w = 1 - d, d = min(decay, (1 + updates) / (10 + updates)) with warm-up, else d = decay.  When the optimiser is guarded
  (optim.Adam(max_grad_norm / skip_nonfinite)) it reads the optimiser's own control block first: a step the guard skipped for a
  non-finite gradient leaves the shadow and the count alone.  The decision is taken on the device, like the guard's.
* `adh_ema_multi` blends shadow += w * (p - shadow) over a resident (tensor, chunk) table: 12 bytes of traffic per parameter.

A parameter the joint optimiser lists twice (train_joint.py:81-89) is shadowed once and advances once per step.  Only
parameters are shadowed: buffers -- the BatchNorm running statistics and `num_batches_tracked` -- are shared with the live
model, as BasicSR's `model_ema` does; `state_dict(model)` therefore returns the EMA weights with the model's live buffers.

`applied()` swaps the shadows into the parameters in place (`adh_ema_swap`: contents move, pointers do not, so the optimiser's
resident table, the data-parallel gradient arena and this table stay valid), yields, and swaps back in a `finally`.  Under
data parallelism no collective is added: ranks start from the same broadcast weights and take identical steps and skip
decisions, so they hold identical shadows.  `updates()` is the one explicit device-to-host read.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import math
from typing import Dict, Iterable, List

import numpy as np
import torch

from . import _hip as H


class WeightEMA:
    def __init__(self, params: Iterable[torch.Tensor], decay: float = 0.999, warmup: bool = True):
        decay = float(decay)
        if math.isnan(decay) or not 0.0 <= decay < 1.0:
            raise ValueError(f"ema decay must lie in [0, 1), got {decay!r}")
        self.decay, self.warmup = decay, bool(warmup)
        self.params: List[torch.Tensor] = []
        seen = set()
        for p in params:
            if id(p) in seen or not p.is_floating_point():
                continue
            seen.add(id(p))
            if p.dtype != torch.float32:      # the kernels read float*: any other width would be blended as garbage
                raise TypeError(f"WeightEMA shadows fp32 parameters only, got {p.dtype} (shape {tuple(p.shape)})")
            H.require_cuda(p, "EMA parameter")
            self.params.append(p)
        if not self.params:
            raise ValueError("WeightEMA needs at least one floating-point parameter")
        self.shadow: List[torch.Tensor] = [p.detach().clone().contiguous() for p in self.params]
        # struct adh_ema_ctrl on the device
        self._ctrl = torch.zeros(C.sizeof(H.EmaCtrl), dtype=torch.uint8, device=self.params[0].device)
        self._table_key = None
        self._table_dev = None
        self._chunks_dev = None
        self._table_host = None
        self._nchunks = 0
        self.uploads = 0              # table uploads so far (one per change of a data_ptr)
        self._applied = False

    # ------------------------------------------------------------------ resident table
    def _key(self):
        return tuple((p.data_ptr(), s.data_ptr(), p.numel()) for p, s in zip(self.params, self.shadow))

    def _ensure_table(self) -> None:
        """The pointer table (24 B per tensor) and the (tensor, chunk) list stay on the device; like Adam.step's they are
        uploaded, through a pinned staging buffer and asynchronously on the current stream, only when a data_ptr() changes."""
        key = self._key()
        if key == self._table_key:
            return
        for p in self.params:
            if not p.is_contiguous():
                raise RuntimeError("WeightEMA: parameters must be contiguous")
        dev = self.params[0].device
        chunk = H.value("adh_adam_chunk_elems")
        table = (H.EmaTensor * len(self.params))()
        for t, (pp, sp, n) in zip(table, key):
            t.p, t.ema, t.n = pp, sp, n
        chunks = np.array([(i, c) for i, (_, _, n) in enumerate(key) for c in range((n + chunk - 1) // chunk)],
                          dtype=np.int32).reshape(-1)
        raw = np.frombuffer(bytes(table), dtype=np.uint8)
        host = torch.empty(raw.size + chunks.size * 4, dtype=torch.uint8)
        if dev.type == "cuda":
            host = host.pin_memory()
        host[:raw.size].copy_(torch.from_numpy(raw.copy()))
        host[raw.size:].copy_(torch.from_numpy(chunks.view(np.uint8).copy()))
        both = host.to(dev, non_blocking=True)
        self._table_host = host                          # keep the staging buffer alive until the copy has run
        self._table_dev, self._chunks_dev = both[:raw.size], both[raw.size:]
        self._nchunks = chunks.size // 2
        self._table_key = key
        self.uploads += 1

    # ------------------------------------------------------------------ the step
    @torch.no_grad()
    def update(self, optimizer=None) -> None:
        """One EMA update on the current stream, to be called right after `optimizer.step()`.  A guarded optimiser's control
        block goes to the kernel, which follows its skip decision; nothing is read back."""
        if self._applied:
            raise RuntimeError("WeightEMA.update() inside applied(): the parameters hold the EMA weights")
        self._ensure_table()
        guard = None
        if optimizer is not None and getattr(optimizer, "guarded", False) and getattr(optimizer, "_ctrl", None) is not None:
            guard = optimizer._ctrl.data_ptr()
        H.call("adh_ema_begin", self._ctrl.data_ptr(), self.decay, int(self.warmup), guard)
        H.call("adh_ema_multi", self._table_dev.data_ptr(), self._chunks_dev.data_ptr(), self._nchunks, self._ctrl.data_ptr())

    def _swap(self) -> None:
        self._ensure_table()
        H.call("adh_ema_swap", self._table_dev.data_ptr(), self._chunks_dev.data_ptr(), self._nchunks)
        from .engine import invalidate_weight_cache   # the kernel wrote the parameters behind torch's version counter
        invalidate_weight_cache()

    @contextlib.contextmanager
    def applied(self):
        """Inside the context the parameters hold the EMA weights and the shadows the raw ones (swapped in place); the swap
        back happens in a `finally`.  Does not nest; `update()` inside it raises."""
        if self._applied:
            raise RuntimeError("WeightEMA.applied() does not nest")
        with torch.no_grad():
            self._swap()
        self._applied = True
        try:
            yield self
        finally:
            self._applied = False
            with torch.no_grad():
                self._swap()

    # ------------------------------------------------------------------ read-back and (de)serialisation
    def _ctrl_field(self, name: str) -> torch.Tensor:
        f = getattr(H.EmaCtrl, name)
        return self._ctrl[f.offset:f.offset + f.size].view(torch.float32 if name == "w" else torch.int32).reshape(())

    @property
    def updates_dev(self) -> torch.Tensor:
        """0-d device view of the block's update counter (for a read-back the caller batches with others)"""
        return self._ctrl_field("updates")

    def updates(self) -> int:
        """EMA updates applied so far (a device-to-host read)."""
        return int(self.updates_dev.item())

    def _names(self, model) -> Dict[int, str]:
        return {id(p): name for name, p in model.named_parameters()}

    def state_dict(self, model) -> dict:
        """`model.state_dict()` with every shadowed parameter replaced by a clone of its shadow; the buffers (BatchNorm running
        statistics, num_batches_tracked) are the live model's.  Loads wherever a `model_state_dict` loads."""
        if self._applied:
            raise RuntimeError("WeightEMA.state_dict() inside applied(): parameters and shadows are swapped")
        sd = model.state_dict()
        names = self._names(model)
        for p, s in zip(self.params, self.shadow):
            name = names.get(id(p))
            if name is not None and name in sd:
                sd[name] = s.detach().clone()
        return sd

    @torch.no_grad()
    def load_state_dict(self, model, sd: dict, updates: int) -> None:
        """Restore the shadows from `sd` (a state dict of `model`, as `state_dict(model)` returns it) and the device counter."""
        names = self._names(model)
        for p, s in zip(self.params, self.shadow):
            name = names.get(id(p))
            if name is None or name not in sd:
                raise KeyError(f"ema state dict has no entry for parameter {name!r}")
            s.copy_(sd[name].to(device=s.device, dtype=s.dtype).reshape(s.shape))
        self._ctrl.zero_()
        self._ctrl_field("updates").fill_(int(updates))

    @torch.no_grad()
    def reseed(self) -> None:
        """Shadows = the parameters' current values, counter = 0 (after weights were loaded over the ones it was built from)."""
        for p, s in zip(self.params, self.shadow):
            s.copy_(p.detach())
        self._ctrl.zero_()
