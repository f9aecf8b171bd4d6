"""Launch trace of one joint training step on the GPU with the `ema:` config section absent.

The recorder is tests/_launch_trace.Trace with two changes the GPU asks for: the launches still run (the step reads its own
results), and a pointer is written down as null or not null only (device addresses differ from run to run and the engine's
buffers are not registered).  Everything else of a record is Trace's: entry point, family, work, work_exec and every argument,
ConvDesc and WLayout fields included, so the geometry and the scalars of every launch are pinned, not only its name.

tests/golden/joint_step_launches.json holds [entry point, first 12 hex digits of the SHA-1 of the record's compact JSON] per
launch, recorded from the commit BEFORE the weight EMA existed.  A step with the section absent or null must reproduce it
exactly (tests/test_gpu_ema.py).  It is regenerated, on the GPU and from the repository root of a checkout whose EMA-off step is
known to be right, with

    python -m tests._joint_step_trace --regen
"""
import ctypes as C
import hashlib
import json
import os
import sys
import warnings

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from adam_dehaze_amd import _hip as H              # noqa: E402
from adam_dehaze_amd import train as T             # noqa: E402
from tests._launch_trace import Trace              # noqa: E402

GOLDEN_PATH = os.path.join(ROOT, "tests", "golden", "joint_step_launches.json")
ABSENT = object()                                  # joint_system(ABSENT): the config has no "ema" key at all


class StepTrace(Trace):
    def __init__(self, real):
        super().__init__()
        self.real = real

    def _ptr(self, p):
        return None if not p else "ptr"

    def _arg(self, a, ctype):
        if isinstance(a, (np.integer, np.floating)):
            a = a.item()
        inner = getattr(a, "_obj", a)
        if isinstance(inner, C.Array) and inner._type_ is not H.ConvDesc:      # Trace knows arrays of ConvDesc only
            return {"array": [inner._type_.__name__, len(inner)]}
        return super()._arg(a, ctype)

    def call(self, name, *args, **kw):
        super().call(name, *args, **kw)
        return self.real(name, *args, **kw)


def joint_system(ema_section=ABSENT, seed=2):
    """the reduced-width joint system of tests/test_gpu_train._cfg; `ema_section` becomes config["ema"] (None included)"""
    from tests.test_gpu_train import _cfg
    cfg = _cfg()
    if ema_section is not ABSENT:
        cfg["ema"] = ema_section
    torch.manual_seed(seed)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return T.build_joint_system(cfg)


def train_mode(system, on=True):
    system["classifier"].train(on)
    for m in system["models"].values():
        m.train(on)
    system["router"].train(on)


def digest(record):
    return [record[0], hashlib.sha1(json.dumps(record, separators=(",", ":")).encode()).hexdigest()[:12]]


def record_step(ema_section=ABSENT):
    """(system, [[entry point, record digest], ...]) of one joint_train_step of a freshly built system"""
    from tests._util import DEV
    batch = next(T.synthetic_loader(4, 32, 1, seed=5, device=DEV))
    system = joint_system(ema_section)
    train_mode(system)
    with pytest.MonkeyPatch.context() as mp:
        trace = StepTrace(H.call)
        mp.setattr(H, "call", trace.call)
        T.joint_train_step(system, batch)
    torch.cuda.synchronize()
    return system, [digest(r) for r in trace.records]


def golden():
    with open(GOLDEN_PATH) as f:
        return json.load(f)["launches"]


def first_difference(got, want):
    """None when equal, else a line naming the first launch that differs"""
    for i, (g, w) in enumerate(zip(got, want)):
        if g != w:
            return f"launch {i}: {g} != golden {w}"
    if len(got) != len(want):
        return f"{len(got)} launches, golden has {len(want)}; the longer one goes on with {(got + want)[min(len(got), len(want))]}"
    return None


def main(argv):
    if "--regen" not in argv:
        raise SystemExit("python -m tests._joint_step_trace --regen [path]")
    path = argv[argv.index("--regen") + 1] if len(argv) > argv.index("--regen") + 1 else GOLDEN_PATH
    _, launches = record_step()
    with open(path, "w") as f:
        f.write('{"launches": [\n' + ",\n".join(" " + json.dumps(r, separators=(",", ":")) for r in launches) + "\n]}\n")
    print(f"{path}: {len(launches)} launches, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main(sys.argv[1:])
