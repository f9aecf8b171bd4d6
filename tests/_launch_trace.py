"""Launch trace of the engine, taken on the CPU: the convolution section (CASES) and every other op (OPS_CASES).

`_hip.call` is replaced by a recorder that launches nothing; the `adh_*_supported` / `*_groups` / `*_num_blocks` queries
(`_hip.value`) are host functions and stay real.  One record per `H.call`:

    [entry point, family, work, work_exec, [argument, ...]]

with ints and floats as they are, a null pointer as None, a pointer as {"p": [buffer number in order of first appearance in
the case's trace, byte offset, buffer size in bytes]}, a ConvDesc as {"d": [its fields in declaration order]}, an array of
them as {"da": [...]} and a WLayout as {"l": [its nine fields]}.  Buffer sizes pin slab and pack sizes, offsets pin the
statistics-row offsets.  A pointer that falls in no registered buffer raises.

The OPS_CASES go through the engine's public methods and backward().  Their recorder also
  - registers every buffer the engine allocates (Engine._f and Engine._buf) and fills the ones not asked for with zero=True
    with NaN (integer buffers: all bits set), so a host-side write that goes missing shows;
  - appends ["SYNC_BN", pointer] where the engine calls SYNC_BN, when a case sets that switch to "trace";
  - gives every record a sixth item: for each non-null pointer of the record, in order, the first 12 hex digits of the SHA-1
    of its buffer's bytes at the time of the call (None for a buffer above 64 KiB).  That pins what torch writes on the host
    and no launch shows (zero=True, coef[0].copy_(...), dbuf[..., C:].zero_(), ...).

tests/golden/launch_trace.json holds the trace of every case in CASES, tests/golden/launch_trace_ops.json of every case in
OPS_CASES.  They are regenerated with

    python -m tests._launch_trace --regen          (--regen-ops for the second)

from the repository root, with the library built -- and only from a version of engine.py whose launches are known to be
right: a golden is what a change to the selection / launch code is compared against.
"""
import ctypes as C
import hashlib
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
OPS_GOLDEN_PATH = os.path.join(ROOT, "tests", "golden", "launch_trace_ops.json")
DIGEST_MAX_BYTES = 64 << 10
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

    def __init__(self, digests=False):
        self.digests = digests  # OPS_CASES: records carry the digests of their pointers' buffers
        self._dig = []
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

    def ramp(self, lo, hi, *shape):
        """a non-constant input: lo .. hi over the elements in storage order"""
        n = math.prod(shape)
        return self.reg(torch.linspace(lo, hi, n, dtype=torch.float32).reshape(shape).clone())

    def alloc(self, t, zero):
        """a buffer the engine allocated: registered, and poisoned unless the engine asked for zeros"""
        if not zero:
            t.fill_(float("nan") if t.is_floating_point() else -1 if t.dtype.is_signed else 255)
        return self.reg(t)

    def sync_bn(self, sums):
        self.records.append(["SYNC_BN", self._ptr(sums.data_ptr())])
        self._dig = []

    def engine(self, record=True):
        self.eng = Engine(torch.device("cpu"), record=record)
        return self.eng

    def _ptr(self, p):
        if not p:
            return None
        for start, size in self.spans:
            if start <= p < start + size:
                n = self.numbers.setdefault(start, len(self.numbers))
                if self.digests:
                    self._dig.append(hashlib.sha1(C.string_at(start, size)).hexdigest()[:12] if size <= DIGEST_MAX_BYTES
                                     else None)
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
        self._dig = []
        rec = [name, family, float(work), None if work_exec is None else float(work_exec),
               [self._arg(a, t) for a, t in zip(args, argtypes)]]
        self.records.append(rec + [self._dig] if self.digests else rec)


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


# ---------------------------------------------------------------------------------------------------------------------
# every other op: through the public methods and backward(), at the smallest shapes that reach every branch
# ---------------------------------------------------------------------------------------------------------------------
def _bn_ramp(T, Cc, trainable=True):
    """non-constant gamma / beta / running statistics: the digests of the buffers they are copied into depend on them"""
    return BNState(T.ramp(0.5, 1.5, Cc).requires_grad_(trainable), T.ramp(-0.2, 0.3, Cc).requires_grad_(trainable),
                   T.ramp(-1.0, 1.0, Cc), T.ramp(0.5, 2.0, Cc), T.new(1, dtype=torch.int64))


def _backward(T, o):
    o.grad = T.ramp(-1.0, 1.0, *o.t.shape)
    T.eng.backward()


def dwconv(k, s, act, mode, second_consumer=False):
    """mode: train | eval_grad (trainable gamma / beta) | eval_frozen | eval_norecord"""
    def run(T):
        Cc = 24
        eng = T.engine(record=mode != "eval_norecord")
        x = Act(T.ramp(-1.0, 1.0, 2, 9, 11, Cc))
        w = T.new(Cc, 1, k, k).requires_grad_(True)
        o = eng.dwconv(x, w, _bn_ramp(T, Cc, trainable=mode != "eval_frozen"), k=k, stride=s, act=act,
                       training=mode == "train")
        if eng.record:
            if second_consumer:
                x.grad = T.new(*x.t.shape)
            _backward(T, o)
            assert x.grad is not None
    return run


def conv_op(k, Cin, Cout, N, Hh, Ww, *, bn=None, training=False, bias=False, residual=False, act=None, relu=True,
            stats=False, twice=False):
    """Engine.conv and its backward; bn: None | "frozen" | "trainable"; twice: the same weight and bias in a second layer"""
    def run(T):
        eng = T.engine(record=True)
        x = Act(T.ramp(-1.0, 1.0, N, Hh, Ww, _r(Cin, 8)), Cin)
        w = _weight(T, "conv", k, Cin, Cout)
        b = T.ramp(-0.5, 0.5, Cout).requires_grad_(True) if bias else None
        res = Act(T.ramp(-2.0, 2.0, N, Hh, Ww, _r(Cout, 8)), Cout) if residual else None
        got = [] if stats else None
        out = T.new(N, Hh, Ww, 2 * _r(Cout, 8))[..., _r(Cout, 8):] if stats else None   # a slice of a wider buffer
        o = x
        for _ in range(2 if twice else 1):
            o = eng.conv(o, w, b, None if bn is None else _bn_ramp(T, Cout, trainable=bn == "trainable"), k=k, stride=1,
                         pad=(k - 1) // 2, relu=relu, act=act, residual=res, training=training, stats=got, out=out)
        assert not stats or len(got) == 1
        _backward(T, o)
        assert x.grad is not None and (res is None or res.grad is not None)
    return run


def sync_chain(T):
    """two train-mode ConvBlocks under SYNC_BN"""
    eng = T.engine(record=True)
    a = x0 = Act(T.ramp(-1.0, 1.0, 1, 16, 32, 32))
    for _ in range(2):
        a = eng.conv(a, _weight(T, "conv", 3, 32, 32), None, _bn_ramp(T, 32), training=True)
    _backward(T, a)
    assert x0.grad is not None


def preact(training):
    """two pre-activation BatchNorms over the first 16 channels of a 32-channel block buffer: in backward() the second is the
    first writer of the block gradient (and zeroes channels 16 .. 31), the first accumulates"""
    def run(T):
        eng = T.engine(record=True)
        buf = T.ramp(-1.0, 1.0, 2, 6, 7, 32)
        sink = {"g": None, "C": 32}
        moments = (T.ramp(-1.0, 1.0, 32).double(), T.ramp(0.5, 2.0, 32).double()) if training else None
        for m in moments or ():
            T.reg(m)
        outs = [eng.bn_relu_preact(Act(buf[..., :16], 16), _bn_ramp(T, 16), training, moments, sink) for _ in range(2)]
        for o in outs:
            o.grad = T.ramp(-1.0, 1.0, *o.t.shape)
        eng.backward()
        assert sink["g"] is not None
    return run


def bn_relu_eval(T):
    eng = T.engine(record=False)
    eng.bn_relu_eval(Act(T.ramp(-1.0, 1.0, 2, 6, 7, 32)[..., :16], 16), _bn_ramp(T, 16))


def dense_block(T):
    """one DenseNet layer the way classifier.py drives it: dense_input, dense_moments without and with a conv epilogue's
    partials, dense_output, and a closing BatchNorm over the whole buffer as the first writer of the block gradient"""
    eng = T.engine(record=True)
    h = Act(T.ramp(-1.0, 1.0, 2, 6, 7, 16))
    buf = eng._f(2, 6, 7, 32)
    sink = {"g": None, "C": 32}
    eng.dense_input(h, buf, sink)
    moments = (T.new(32, dtype=torch.float64), T.new(32, dtype=torch.float64))
    eng.dense_moments(Act(buf[..., :16], 16), moments, 0)
    a = eng.bn_relu_preact(Act(buf[..., :16], 16), _bn_ramp(T, 16), True, moments, sink)
    b = eng.conv(a, _weight(T, "conv", 1, 16, 16), None, _bn_ramp(T, 16), k=1, pad=0, training=True)
    stats = []
    o = eng.conv(b, _weight(T, "conv", 3, 16, 16), None, None, relu=False, out=buf[..., 16:], stats=stats)
    eng.dense_output(o, sink, 16)
    eng.dense_moments(o, moments, 16, partials=stats[0])
    _backward(T, eng.bn_relu_preact(Act(buf, 32), _bn_ramp(T, 32), True, moments, sink))
    assert h.grad is not None


def attention(T):
    eng = T.engine(record=True)
    x = Act(T.ramp(-1.0, 1.0, 2, 9, 11, 16))
    w1, w2, wsp = (T.new(*shape).requires_grad_(True) for shape in ((2, 16), (16, 2), (1, 2, 7, 7)))
    _backward(T, eng.attention(x, w1, w2, wsp))
    assert x.grad is not None


def unary(op, shape, *args):
    """x -> Engine.<op>(x, *args) and its backward"""
    def run(T):
        eng = T.engine(record=True)
        x = Act(T.ramp(-1.0, 1.0, *shape))
        _backward(T, getattr(eng, op)(x, *args))
        assert x.grad is not None
    return run


def concat(T):
    eng = T.engine(record=True)
    buf, views = eng.concat_buffer(2, 3, 5, (8, 16))
    parts = [Act(v) for v in views]
    parts[0].grad = T.new(2, 3, 5, 8)       # the first part already holds a gradient: accum adds into it
    _backward(T, eng.concat(buf, parts))
    assert parts[1].grad is not None


def activation(T):
    eng = T.engine(record=True)
    x = Act(T.ramp(-4.0, 4.0, 2, 3, 5, 8), 6)
    _backward(T, eng.activation(x, H.ACT_HARDSIGMOID))
    assert x.grad is not None


def channel_scale(T):
    eng = T.engine(record=True)
    x, s = Act(T.ramp(-1.0, 1.0, 2, 3, 5, 8)), Act(T.ramp(0.0, 1.0, 2, 1, 1, 8))
    _backward(T, eng.channel_scale(x, s))
    assert x.grad is not None and s.grad is not None


def mul_mask(T):
    eng = T.engine(record=True)
    x = Act(T.ramp(-1.0, 1.0, 2, 3, 5, 8))
    _backward(T, eng.mul_mask(x, T.ramp(0.0, 2.0, 2, 3, 5, 8)))
    assert x.grad is not None


def head_blend(mode):
    def run(T):
        eng = T.engine(record=True)
        x_img = T.ramp(0.0, 1.0, 1, 3, 8, 8)
        r = Act(T.ramp(-1.0, 1.0, 1, 8, 8, 8), 3)
        gd = Act(T.ramp(0.0, 1.0, 1, 8, 8, 4), 1) if mode in (2, 4) else None       # BLEND_GUIDED, BLEND_DUAL
        alpha = T.ramp(0.5, 0.5, 1).requires_grad_(True) if mode == 0 else None      # BLEND_LIGHT
        _, holder = eng.head_blend(mode, x_img, r, gd, alpha)
        holder["g"] = T.ramp(-1.0, 1.0, 1, 3, 8, 8)
        eng.backward()
        assert r.grad is not None and (gd is None or gd.grad is not None)
    return run


def mse(T):
    eng = T.engine(record=True)
    a, b = Act(T.ramp(-1.0, 1.0, 2, 3, 5, 8)), Act(T.ramp(1.0, -1.0, 2, 3, 5, 8), needs_grad=False)
    vals = []
    eng.mse(a, b, 0.5, vals)
    eng.upstream["g"] = T.ramp(1.0, 1.0, 1)
    eng.backward()
    assert len(vals) == 1 and a.grad is not None


def images(T):
    eng = T.engine(record=True)
    x = T.ramp(0.0, 1.0, 1, 3, 8, 8)
    eng.image_to_nhwc8(x)
    holder = {}
    _backward(T, eng.image_normalize_to_nhwc8(x, (0.485, 0.456, 0.406), (0.229, 0.224, 0.225), holder))
    assert holder["gx"].shape == x.shape


SYNC = dict(SYNC_BN="trace")
DW = {"3s2_hswish": (3, 2, H.ACT_HARDSWISH), "5s1_none": (5, 1, H.ACT_NONE)}
OPS_CASES = {
    **{f"dwconv_{g}/{mode}": (dwconv(*a, mode), {}, {}) for g, a in DW.items()
       for mode in ("train", "eval_grad", "eval_frozen", "eval_norecord")},
    **{f"dwconv_{g}/train,sync_bn": (dwconv(*a, "train"), SYNC, {}) for g, a in DW.items()},
    "dwconv_3s2_hswish/train,second_consumer": (dwconv(*DW["3s2_hswish"], "train", second_consumer=True), {}, {}),
    "conv/eval,residual": (conv_op(3, 16, 16, 1, 8, 8, bn="frozen", residual=True), {}, {}),
    "conv/eval_act,relu6": (conv_op(1, 16, 24, 1, 8, 8, bn="frozen", act=H.ACT_RELU6), {}, {}),
    "conv/eval_act,trainable,residual": (conv_op(3, 16, 16, 1, 8, 8, bn="trainable", residual=True), {}, {}),
    "conv/eval_act,trainable,bias": (conv_op(1, 16, 24, 1, 8, 8, bn="trainable", bias=True, act=H.ACT_HARDSWISH), {}, {}),
    "conv/bias": (conv_op(3, 16, 16, 1, 8, 8, bias=True, relu=False), {}, {}),
    "conv/bias,shared_weight": (conv_op(3, 16, 16, 1, 8, 8, bias=True, twice=True), {}, {}),
    "conv/stats": (conv_op(3, 16, 16, 1, 8, 8, relu=False, stats=True), {}, {}),
    "conv/train,sync_bn": (sync_chain, SYNC, {}),
    "conv/train,cout_6": (conv_op(3, 16, 6, 1, 8, 8, bn="trainable", training=True, bias=True), {}, {}),
    "conv/train,residual,relu_bits": (conv_op(3, 16, 16, 1, 8, 8, bn="trainable", training=True, residual=True),
                                      dict(USE_RELU_BITS=True), {}),
    "bn_relu_preact/train": (preact(True), {}, {}),
    "bn_relu_preact/frozen,trainable": (preact(False), {}, {}),
    "bn_relu_eval": (bn_relu_eval, {}, {}),
    "dense_block": (dense_block, {}, {}),
    "attention": (attention, {}, {}),
    "maxpool_3_2_1": (unary("maxpool", (2, 9, 11, 8), 3, 2, 1), {}, {}),
    "bilinear/align": (unary("bilinear", (2, 4, 6, 8), 7, 5, True), {}, {}),
    "bilinear/no_align": (unary("bilinear", (2, 4, 6, 8), 7, 5, False), {}, {}),
    "avgpool_2_odd": (unary("avgpool", (2, 9, 11, 8), 2), {}, {}),
    "global_avgpool_1032": (unary("global_avgpool", (2, 3, 3, 1032)), {}, {}),
    "concat": (concat, {}, {}),
    "activation_hsigmoid_6": (activation, {}, {}),
    "channel_scale": (channel_scale, {}, {}),
    "mul_mask": (mul_mask, {}, {}),
    **{f"head_blend/{m}": (head_blend(m), {}, {}) for m in range(5)},
    "mse": (mse, {}, {}),
    "images": (images, {}, {}),
}


def library_env_set():
    return [v for v in LIBRARY_ENV if os.environ.get(v) is not None]


def run_case(name, mp):
    """The trace of one case of CASES or OPS_CASES; `mp` is a pytest MonkeyPatch."""
    ops = name not in CASES
    runner, switches, env = (OPS_CASES if ops else CASES)[name]
    T = Trace(digests=ops)
    for k, v in {**DEFAULTS, **switches}.items():
        mp.setattr(E, k, T.sync_bn if (k, v) == ("SYNC_BN", "trace") else v)
    mp.delenv("ADH_NSPLIT", raising=False)
    for k, v in env.items():
        mp.setenv(k, v)
    mp.setattr(H, "call", T.call)
    real_f = Engine._f
    if ops:
        real_buf = Engine._buf
        mp.setattr(Engine, "_f", lambda self, *shape, zero=False: T.alloc(real_f(self, *shape, zero=zero), zero))
        mp.setattr(Engine, "_buf", lambda self, *shape, dtype: T.alloc(real_buf(self, *shape, dtype=dtype), False))
    else:
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
        if "SYNC_BN" in (g[0], w[0]):
            if g != w:
                out.append(f"{at}: {g} != {w}")
            continue
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
        if g[5:] != w[5:]:
            out.append(f"{at}: buffer digests {g[5:]} != {w[5:]}")
    return out[:8]


def summary(records):
    return " ".join(r[0][4:] for r in records)


def _write_golden(path, table):
    cases = {}
    for name in table:
        with pytest.MonkeyPatch.context() as mp:
            cases[name] = run_case(name, mp)
    with open(path, "w") as f:
        f.write('{"conv_desc_fields": %s,\n "cases": {\n' % json.dumps(DESC_FIELDS))
        f.write(",\n".join('  %s: [\n%s]' % (json.dumps(n), ",\n".join("   " + json.dumps(r, separators=(",", ":")) for r in recs))
                           for n, recs in cases.items()))
        f.write("\n }}\n")
    print(f"{path}: {len(cases)} cases, {sum(len(r) for r in cases.values())} launches, {os.path.getsize(path)} bytes")


def main(argv):
    if library_env_set():
        raise SystemExit(f"unset {library_env_set()} first")
    if "--regen" in argv:
        _write_golden(GOLDEN_PATH, CASES)
    if "--regen-ops" in argv:
        _write_golden(OPS_GOLDEN_PATH, OPS_CASES)
    if "--regen" not in argv and "--regen-ops" not in argv:
        for name in list(CASES) + list(OPS_CASES):
            with pytest.MonkeyPatch.context() as mp:
                print(f"{name}: {summary(run_case(name, mp))}")


if __name__ == "__main__":
    main(sys.argv[1:])
