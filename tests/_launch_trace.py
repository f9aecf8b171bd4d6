"""Launch trace of the engine's convolution section, taken on the CPU.

`_hip.call` is replaced by a recorder that launches nothing; the `adh_*_supported` / `*_groups` / `*_num_blocks` queries
(`_hip.value`) are host functions and stay real.  One record per `H.call`:

    [entry point, family, work, work_exec, [argument, ...]]

with ints and floats as they are, a null pointer as None, a pointer as {"p": [buffer number in order of first appearance in
the case's trace, byte offset, buffer size in bytes]}, a ConvDesc as {"d": [its fields in declaration order]}, an array of
them as {"da": [...]} and a WLayout as {"l": [its nine fields]}.  Buffer sizes pin slab and pack sizes, offsets pin the
statistics-row offsets.  A pointer that falls in no registered buffer raises.

tests/golden/launch_trace.json holds the trace of every case in CASES.  It is regenerated with

    python -m tests._launch_trace --regen

from the repository root, with the library built -- and only from a version of engine.py whose launches are known to be
right: the golden is what a change to the selection / launch code is compared against.
"""
import ctypes as C
import json
import math
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import adam_dehaze_amd.engine as E                 # noqa: E402
from adam_dehaze_amd import _hip as H              # noqa: E402
from adam_dehaze_amd.engine import Act, BNState, Engine   # noqa: E402

GOLDEN_PATH = os.path.join(ROOT, "tests", "golden", "launch_trace.json")
DESC_FIELDS = [f[0] for f in H.ConvDesc._fields_]
DESC_POINTERS = {f[0] for f in H.ConvDesc._fields_ if f[1] is H.vp}

# A/B variables the library itself reads (csrc/*.hip): they change what the host queries answer
LIBRARY_ENV = ("ADH_WINO43", "ADH_WINO43_GRID", "ADH_WINO_DEBUG", "ADH_WINO32", "ADH_WINO32_TAIL", "ADH_ROWS_FWD",
               "ADH_WINO43_WGRAD", "ADH_WINO32_WGRAD", "ADH_WGRAD32_V2", "ADH_WINO_WGRAD", "ADH_FEWOUT", "ADH_STEM_FWD")

# every engine switch the trace depends on, at its default
DEFAULTS = dict(USE_WINOGRAD=True, USE_WINO43=True, USE_WINO43_WGRAD=True, CONTRACT="fp32", W43_WGRAD_ROUNDS=4,
                USE_SMALL_WGRAD=True, USE_FEWOUT=True, USE_BN_FUSED_REDUCE=True, MERGE_CLASSES=True, USE_RELU_BITS=False,
                _WINO_ONLY="", USE_PACK_CACHE=False, SYNC_BN=None, GRAD_SINK=None, GRAD_READY=None, RELU_CAPTURE=None)


def _r(a, b):
    return (a + b - 1) // b * b


class Trace:
    """Recorder + buffer registry of one case."""

    def __init__(self):
        self.records = []
        self.keep = []          # every registered tensor stays alive for the case: the allocator must not reuse addresses
        self.spans = []         # (start, size in bytes)
        self.numbers = {}       # start -> buffer number, in order of first appearance in the trace
        self.eng = None

    def reg(self, t):
        st = t.untyped_storage()
        if st.nbytes():
            self.keep.append(t)
            self.spans.append((st.data_ptr(), st.nbytes()))
        return t

    def new(self, *shape, dtype=torch.float32):
        return self.reg(torch.zeros(shape, dtype=dtype))

    def engine(self, record=True):
        self.eng = Engine(torch.device("cpu"), record=record)
        return self.eng

    def _ptr(self, p):
        if not p:
            return None
        for start, size in self.spans:
            if start <= p < start + size:
                n = self.numbers.setdefault(start, len(self.numbers))
                return {"p": [n, p - start, size]}
        raise AssertionError(f"pointer {p:#x} falls in no registered buffer")

    def _desc(self, d):
        return [self._ptr(getattr(d, f)) if f in DESC_POINTERS else getattr(d, f) for f in DESC_FIELDS]

    def _arg(self, a, ctype):
        if hasattr(a, "_obj"):       # ctypes.byref(...)
            a = a._obj
        if isinstance(a, H.ConvDesc):
            return {"d": self._desc(a)}
        if isinstance(a, H.WLayout):
            return {"l": [getattr(a, f[0]) for f in H.WLayout._fields_]}
        if isinstance(a, C.Array):
            return {"da": [self._desc(d) for d in a]}
        if ctype is H.vp:
            return self._ptr(a)
        assert isinstance(a, (int, float)), (type(a), ctype)
        return a

    def call(self, name, *args, work=0.0, work_exec=None, family=None):
        argtypes = H._SIGNATURES[name][1:]          # [0] is the stream
        assert len(args) == len(argtypes), (name, len(args), len(argtypes))
        self.records.append([name, family, float(work), None if work_exec is None else float(work_exec),
                             [self._arg(a, t) for a, t in zip(args, argtypes)]])


# ---------------------------------------------------------------------------------------------------------------------
# runners
# ---------------------------------------------------------------------------------------------------------------------
def _weight(T, kind, k, Cin, Cout):
    w = T.new(Cout, Cin, k, k) if kind == "conv" else T.new(Cin, Cout, k, k)
    return w.requires_grad_(True)


def _out_hw(kind, k, s, p, Hh, Ww):
    if kind == "conv":
        return (Hh + 2 * p - k) // s + 1, (Ww + 2 * p - k) // s + 1
    return Hh * 2, Ww * 2


def layer(kind, k, s, p, Cin, Cout, N, Hh, Ww, stats=True, xC=None, parts="fdw", wino43=None):
    """forward (with statistics), data gradient and weight gradient of one layer, the way tests/test_gpu_parity.py calls them"""
    def run(T):
        eng = T.engine(record=False)
        eng.wino43 = wino43
        x = Act(T.new(N, Hh, Ww, _r(Cin, 8)), Cin if xC is None else xC)
        w = _weight(T, kind, k, Cin, Cout)
        OH, OW = _out_hw(kind, k, s, p, Hh, Ww)
        plans = eng._launch_plan(kind, k, s, p, w, "fwd")
        gy = T.new(N, OH, OW, _r(Cout, 8))
        if "f" in parts:
            y = T.new(N, OH, OW, _r(Cout, 4 if stats else 8))
            b = T.new(Cout)
            eng._run_gather(plans, x, y, Cout, w, shift=b, want_stats=stats)
        if "d" in parts:
            gx = T.new(N, Hh, Ww, _r(Cin, 4))
            eng._run_gather(eng._launch_plan(kind, k, s, p, w, "dgrad"), Act(gy, Cout), gx, Cin, w)
        if "w" in parts:
            eng._wgrad(plans, x, gy, Cout, w)
    return run


def epilogue(kind, k, s, p, Cin, Cout, N, Hh, Ww):
    """one forward with scale, shift, residual and ReLU together"""
    def run(T):
        eng = T.engine(record=False)
        x = Act(T.new(N, Hh, Ww, _r(Cin, 8)), Cin)
        w = _weight(T, kind, k, Cin, Cout)
        OH, OW = _out_hw(kind, k, s, p, Hh, Ww)
        y, res = T.new(N, OH, OW, _r(Cout, 8)), T.new(N, OH, OW, _r(Cout, 8))
        eng._run_gather(eng._launch_plan(kind, k, s, p, w, "fwd"), x, y, Cout, w, scale=T.new(Cout), shift=T.new(Cout),
                        residual=res, act=H.ACT_RELU)
    return run


def bnred(Cp, Cn, N, Hh, Ww):
    """the consumer's data gradient with the producer's BatchNorm-backward sums in its epilogue, called directly"""
    def run(T):
        eng = T.engine(record=False)
        w = _weight(T, "conv", 3, Cp, Cn)
        y, ss, mean = T.new(N, Hh, Ww, Cp), T.new(2, _r(Cp, 4)), T.new(Cp)
        gx = T.new(N, Hh, Ww, Cp)
        rows, _ = eng._run_gather(eng._launch_plan("conv", 3, 1, 1, w, "dgrad"), Act(T.new(N, Hh, Ww, Cn), Cn), gx, Cp, w,
                                  bnred=(y, ss, mean))
        assert rows is not None
    return run


def _bn(T, Cc):
    return BNState(T.new(Cc).requires_grad_(True), T.new(Cc).requires_grad_(True), T.new(Cc), T.new(Cc),
                   T.new(1, dtype=torch.int64))


def chain(Cc, N, Hh, Ww, spec):
    """train-mode ConvBlocks through Engine.conv and backward(); spec: (kind, k, stride, pad, residual from the chain's input)"""
    def run(T):
        eng = T.engine(record=True)
        x0 = Act(T.new(N, Hh, Ww, Cc))
        a = x0
        for kind, k, s, p, res in spec:
            a = eng.conv(a, _weight(T, kind, k, Cc, Cc), None, _bn(T, Cc), kind=kind, k=k, stride=s, pad=p, training=True,
                         residual=x0 if res else None)
        a.grad = T.new(*a.t.shape)
        eng.backward()
        assert x0.grad is not None
    return run


def pack_cache(T):
    """the same layer twice with the pack cache on: the second forward records no pack call"""
    E.invalidate_weight_cache()
    try:
        eng = T.engine(record=False)
        x = Act(T.new(1, 20, 36, 32))
        w = _weight(T, "conv", 3, 32, 96)
        plans = eng._launch_plan("conv", 3, 1, 1, w, "fwd")
        for _ in range(2):
            eng._run_gather(plans, x, T.new(1, 20, 36, 96), 96, w)
    finally:
        E.invalidate_weight_cache()


# the layers of the table in the issue this trace was introduced with: (kind, k, stride, pad, Cin, Cout, N, H, W)
C96 = ("conv", 3, 1, 1, 96, 96, 2, 40, 72)
C32_96 = ("conv", 3, 1, 1, 32, 96, 1, 20, 36)
C32 = ("conv", 3, 1, 1, 32, 32, 1, 24, 40)
C16 = ("conv", 3, 1, 1, 16, 16, 1, 24, 40)
C8 = ("conv", 3, 1, 1, 8, 8, 1, 24, 40)
C48_3 = ("conv", 3, 1, 1, 48, 3, 1, 24, 40)
C16_1 = ("conv", 3, 1, 1, 16, 1, 1, 24, 40)
C3_48 = ("conv", 3, 1, 1, 3, 48, 1, 24, 40)
C3_16 = ("conv", 3, 1, 1, 3, 16, 1, 24, 40)
D96 = ("conv", 4, 2, 1, 96, 192, 1, 32, 64)
D16 = ("conv", 4, 2, 1, 16, 32, 1, 16, 32)
D8 = ("conv", 4, 2, 1, 8, 16, 1, 16, 32)
T192 = ("convT", 4, 2, 1, 192, 96, 1, 16, 32)
T32 = ("convT", 4, 2, 1, 32, 16, 1, 7, 9)
T8 = ("convT", 4, 2, 1, 8, 8, 1, 8, 8)
S64 = ("conv", 3, 2, 1, 64, 128, 1, 32, 32)
P64 = ("conv", 1, 1, 0, 64, 256, 1, 16, 16)
P64S = ("conv", 1, 2, 0, 64, 128, 1, 16, 16)
STEM = ("conv", 7, 1, 3, 3, 64, 1, 32, 32)
STEM2 = ("conv", 7, 2, 3, 3, 64, 1, 64, 64)
# wide enough for a forced split count to reach the 1 GiB slab cap
C384 = ("conv", 3, 1, 1, 384, 384, 1, 64, 128)
D384 = ("conv", 4, 2, 1, 384, 384, 1, 64, 128)

# name -> (runner, engine switches that differ from DEFAULTS, environment)
CASES = {
    "c3_96_96": (layer(*C96), {}, {}),
    "c3_32_96": (layer(*C32_96), {}, {}),
    "c3_32_32": (layer(*C32), {}, {}),
    "c3_16_16": (layer(*C16), {}, {}),
    "c3_8_8": (layer(*C8), {}, {}),
    "c3_48_3": (layer(*C48_3, stats=False), {}, {}),
    "c3_16_1": (layer(*C16_1, stats=False), {}, {}),
    "c3_3_48": (layer(*C3_48, stats=False), {}, {}),
    "c3_3_16": (layer(*C3_16), {}, {}),
    "c4s2_96_192": (layer(*D96), {}, {}),
    "c4s2_16_32": (layer(*D16), {}, {}),
    "c4s2_8_16": (layer(*D8), {}, {}),
    "t4_192_96": (layer(*T192), {}, {}),
    "t4_32_16_odd": (layer(*T32), {}, {}),
    "t4_8_8": (layer(*T8), {}, {}),
    "c3s2_64_128": (layer(*S64), {}, {}),
    "c1_64_256": (layer(*P64), {}, {}),
    "c1s2_64_128": (layer(*P64S), {}, {}),
    "c7_stem": (layer(*STEM, xC=8), {}, {}),
    "c7s2_stem": (layer(*STEM2, xC=8), {}, {}),
    # the same shapes under switches
    "c3_96_96/wino43=off": (layer(*C96), dict(USE_WINO43=False), {}),
    "c3_32_32/wino43=off": (layer(*C32), dict(USE_WINO43=False), {}),
    "c3_96_96/wino43=fwd": (layer(*C96, parts="fd"), dict(USE_WINO43="fwd"), {}),
    "c3_96_96/wino43=dgrad": (layer(*C96, parts="fd"), dict(USE_WINO43="dgrad"), {}),
    "c3_96_96/engine.wino43=dgrad": (layer(*C96, parts="fd", wino43="dgrad"), {}, {}),
    "c3_96_96/winograd=off": (layer(*C96), dict(USE_WINOGRAD=False), {}),
    "c3_3_48/winograd=off": (layer(*C3_48, stats=False), dict(USE_WINOGRAD=False), {}),
    "c4s2_96_192/winograd=off": (layer(*D96), dict(USE_WINOGRAD=False), {}),
    "t4_192_96/winograd=off": (layer(*T192), dict(USE_WINOGRAD=False), {}),
    "c3s2_64_128/winograd=off": (layer(*S64), dict(USE_WINOGRAD=False), {}),
    "c3_96_96/wino43_wgrad=off": (layer(*C96, parts="w"), dict(USE_WINO43_WGRAD=False), {}),
    "c7_stem/small_wgrad=off": (layer(*STEM, xC=8), dict(USE_SMALL_WGRAD=False), {}),
    "c3_16_16/small_wgrad=off": (layer(*C16, parts="w"), dict(USE_SMALL_WGRAD=False), {}),
    "c3_48_3/small_wgrad=off": (layer(*C48_3, parts="w"), dict(USE_SMALL_WGRAD=False), {}),
    "c3_48_3/fewout=off": (layer(*C48_3, stats=False, parts="fd"), dict(USE_FEWOUT=False), {}),
    "c3_3_48/fewout=off": (layer(*C3_48, stats=False, parts="fd"), dict(USE_FEWOUT=False), {}),
    "c3_3_16/fewout=off": (layer(*C3_16, parts="fd"), dict(USE_FEWOUT=False), {}),
    "c3_48_3/stats": (layer(*C48_3, parts="f"), {}, {}),
    "c3_3_48/stats": (layer(*C3_48, parts="f"), {}, {}),
    "t4_192_96/merge=off": (layer(*T192), dict(MERGE_CLASSES=False), {}),
    "c4s2_96_192/merge=off": (layer(*D96, parts="d"), dict(MERGE_CLASSES=False), {}),
    "c3_96_96/bf16x3": (layer(*C96, parts="fd"), dict(CONTRACT="bf16x3"), {}),
    "c4s2_96_192/bf16x3": (layer(*D96, parts="fd"), dict(CONTRACT="bf16x3"), {}),
    "t4_192_96/bf16x3": (layer(*T192, parts="fd"), dict(CONTRACT="bf16x3"), {}),
    "t4_192_96/bf16x3,merge=off": (layer(*T192, parts="f"), dict(CONTRACT="bf16x3", MERGE_CLASSES=False), {}),
    "bnred_96": (bnred(96, 96, 2, 40, 72), {}, {}),
    "bnred_96/bf16x3": (bnred(96, 96, 2, 40, 72), dict(CONTRACT="bf16x3"), {}),
    "c3_96_96/w43_rounds=2": (layer(*C96, parts="w"), dict(W43_WGRAD_ROUNDS=2), {}),
    # forced split counts: below and above the slab cap
    "c3_96_96/nsplit=7": (layer(*C96, parts="w"), {}, dict(ADH_NSPLIT="7")),
    "c3_32_32/nsplit=7": (layer(*C32, parts="w"), {}, dict(ADH_NSPLIT="7")),
    "c4s2_96_192/nsplit=7": (layer(*D96, parts="w"), {}, dict(ADH_NSPLIT="7")),
    "t4_192_96/nsplit=7": (layer(*T192, parts="w"), {}, dict(ADH_NSPLIT="7")),
    "c3_384/nsplit=500": (layer(*C384, parts="w"), {}, dict(ADH_NSPLIT="500")),
    "c3_384/nsplit=500,wino43_wgrad=off": (layer(*C384, parts="w"), dict(USE_WINO43_WGRAD=False), dict(ADH_NSPLIT="500")),
    "c3_384/nsplit=500,winograd=off": (layer(*C384, parts="w"), dict(USE_WINOGRAD=False), dict(ADH_NSPLIT="500")),
    "c4s2_384/nsplit=500": (layer(*D384, parts="w"), {}, dict(ADH_NSPLIT="500")),
    # epilogue inputs together
    "c3_96_96/epilogue": (epilogue(*C96), {}, {}),
    "c3_8_8/epilogue": (epilogue(*C8), {}, {}),
    "t4_192_96/epilogue": (epilogue(*T192), {}, {}),
    # through Engine.conv(training=True) and backward()
    "chain_32": (chain(32, 1, 16, 32, [("conv", 3, 1, 1, False)] * 2), {}, {}),
    "chain_96": (chain(96, 1, 32, 64, [("conv", 3, 1, 1, False), ("conv", 3, 1, 1, True), ("conv", 4, 2, 1, False),
                                        ("convT", 4, 2, 1, False)]), {}, {}),
    "chain_32/bn_fused_reduce=off": (chain(32, 1, 16, 32, [("conv", 3, 1, 1, False)] * 2), dict(USE_BN_FUSED_REDUCE=False), {}),
    "pack_cache": (pack_cache, dict(USE_PACK_CACHE=True), {}),
}


def library_env_set():
    return [v for v in LIBRARY_ENV if os.environ.get(v) is not None]


def run_case(name, mp):
    """The trace of one case; `mp` is a pytest MonkeyPatch."""
    runner, switches, env = CASES[name]
    for k, v in {**DEFAULTS, **switches}.items():
        mp.setattr(E, k, v)
    mp.delenv("ADH_NSPLIT", raising=False)
    for k, v in env.items():
        mp.setenv(k, v)
    T = Trace()
    mp.setattr(H, "call", T.call)
    real_f = Engine._f
    mp.setattr(Engine, "_f", lambda self, *shape, zero=False: T.reg(real_f(self, *shape, zero=zero)))
    runner(T)
    return T.records


def differences(got, want, where=""):
    """Exact comparison, except work / work_exec (items 2 and 3 of a record) to 1e-12 relative.  Returns the first few
    differences as text."""
    out = []
    if len(got) != len(want):
        out.append(f"{where}: {len(got)} launches {[r[0] for r in got]}, golden has {len(want)} {[r[0] for r in want]}")
        return out
    for i, (g, w) in enumerate(zip(got, want)):
        at = f"{where}[{i}] {w[0]}"
        if g[:2] != w[:2]:
            out.append(f"{at}: entry point / family {g[:2]} != {w[:2]}")
            continue
        for j, what in ((2, "work"), (3, "work_exec")):
            if (g[j] is None) != (w[j] is None) or (g[j] is not None and not math.isclose(g[j], w[j], rel_tol=1e-12, abs_tol=0.0)):
                out.append(f"{at}: {what} {g[j]!r} != {w[j]!r}")
        if len(g[4]) != len(w[4]):
            out.append(f"{at}: {len(g[4])} arguments != {len(w[4])}")
            continue
        for n, (a, b) in enumerate(zip(g[4], w[4])):
            if a == b:
                continue
            if isinstance(a, dict) and isinstance(b, dict) and a.keys() == b.keys() and ("d" in a or "da" in a):
                ds = zip([a["d"]], [b["d"]]) if "d" in a else zip(a["da"], b["da"])
                for m, (da, db) in enumerate(ds):
                    bad = {f: (x, y) for f, x, y in zip(DESC_FIELDS, da, db) if x != y}
                    if bad:
                        out.append(f"{at}: argument {n} descriptor {m}: (got, golden) {bad}")
            else:
                out.append(f"{at}: argument {n}: {a} != {b}")
    return out[:8]


def summary(records):
    return " ".join(r[0][4:] for r in records)


def main(argv):
    if library_env_set():
        raise SystemExit(f"unset {library_env_set()} first")
    if "--regen" not in argv:
        for name in CASES:
            with pytest.MonkeyPatch.context() as mp:
                print(f"{name}: {summary(run_case(name, mp))}")
        return
    cases = {}
    for name in CASES:
        with pytest.MonkeyPatch.context() as mp:
            cases[name] = run_case(name, mp)
    with open(GOLDEN_PATH, "w") as f:
        f.write('{"conv_desc_fields": %s,\n "cases": {\n' % json.dumps(DESC_FIELDS))
        f.write(",\n".join('  %s: [\n%s]' % (json.dumps(n), ",\n".join("   " + json.dumps(r, separators=(",", ":")) for r in recs))
                           for n, recs in cases.items()))
        f.write("\n }}\n")
    print(f"{GOLDEN_PATH}: {len(cases)} cases, {sum(len(r) for r in cases.values())} launches, {os.path.getsize(GOLDEN_PATH)} bytes")


if __name__ == "__main__":
    main(sys.argv[1:])
