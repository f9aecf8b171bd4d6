"""Every split-accumulating weight-gradient kernel against the float64 definition at EVERY pixel-split count its contract
allows on a small shape (tests/_wgrad_split_cases.py: which situations each (case, nsplit) is), not only at the one count
engine._rows_nsplit picks for the shape.  The count is forced through ADH_NSPLIT (read on every call, clamped to the tile
count); the general kernel, whose count the engine does not route through _rows_nsplit, is called through the C ABI.

For every (case, nsplit):
  * the forced count must arrive at the launch entry point of the intended family and at its reduce (H.call is wrapped),
    and no other weight-gradient entry point may run;
  * the tile count the case table derives must be the library's own;
  * every buffer the engine leaves uninitialised (Engine._f(.., zero=False): the slabs and the gradient) comes back full
    of NaN, so an element no kernel writes reaches the result;
  * max|dw - ref64| < 2e-5 max|ref64|, the gate of test_winograd_weight_gradient_matches_direct,
    test_wino32_weight_gradient_matches_direct and test_merged_class_weight_gradient, the same at every count (seeded randn
    inputs: one dropped pixel of one tile moves an element by ~1 / (3 sqrt(N H W)) of the scale, >= 4e-3 here);
  * two runs at the same count are bit-equal (fixed summation order: csrc/common.h, conv_wgrad_reduce.hip).
One line per (family, case, nsplit) goes to the file ADH_SPLIT_SWEEP_TABLE names, by default profile_out/wgrad_split_sweep.txt
(committed as profiles/wgrad_split_sweep.txt)."""
import ctypes as C
import math
import os

import pytest
import torch
import torch.nn.functional as F

from adam_dehaze_amd import _hip as H
from adam_dehaze_amd.engine import Act, Engine
from tests import _wgrad_split_cases as W
from tests.test_gpu_parity import _wgrad_desc

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GATE = 2e-5
SWEEP = os.environ.get("ADH_SPLIT_SWEEP_TABLE") or os.path.join("profile_out", "wgrad_split_sweep.txt")

# kind -> (_launch_plan kind, k, stride, pad)
LAYER = {"conv3": ("conv", 3, 1, 1), "conv4s2": ("conv", 4, 2, 1), "convT": ("convT", 4, 2, 1), "conv1": ("conv", 1, 1, 0),
         "conv3s2": ("conv", 3, 2, 1)}


class Route:
    """How a family is reached and what must be seen on the way.  `launch` / `reduce`: entry points and the position of
    their split argument after the stream; `reduce_count(nsplit)`: what the reduce must receive."""
    def __init__(self, winograd, wino43, merge, launch, larg, reduce, reduce_count, tiles):
        self.winograd, self.wino43, self.merge = winograd, wino43, merge
        self.launch, self.larg, self.reduce, self.reduce_count, self.tiles = launch, larg, reduce, reduce_count, tiles


_W32 = dict(launch="adh_conv_wgrad_wino32", larg=2, reduce="adh_wgrad_reduce_wino32", reduce_count=lambda n: n,
            tiles="adh_conv_wgrad_wino32_tiles")
ROUTES = {
    "wino43": Route(True, True, False, "adh_conv_wgrad_wino43", 2, "adh_wgrad_reduce_wino43", lambda n: n,
                    "adh_conv_wgrad_wino43_strips"),
    "wino23_rows": Route(True, False, False, "adh_conv_wgrad_wino", 2, "adh_wgrad_reduce_wino", lambda n: n, None),
    # conv_wgrad_rows_kernel's four waves write a slab each: the reduce sums 4 nsplit of them (adh_conv_wgrad_slabs)
    "rows_direct": Route(False, False, False, "adh_conv_wgrad", 2, "adh_wgrad_reduce", lambda n: 4 * n, None),
    "wino32_v1": Route(True, True, False, **_W32),
    "wino32_v2": Route(True, True, False, **_W32),
    "wino32_v2c96": Route(True, True, False, **_W32),
    # adh_conv_wgrad_wino32_multi sums the splits itself (adh_wgrad_sum_splits): its per-class reduce calls get one slab
    "wino32_merged": Route(True, True, True, "adh_conv_wgrad_wino32_multi", 3, "adh_wgrad_reduce_wino32", lambda n: 1,
                           "adh_conv_wgrad_wino32_tiles"),
}


@pytest.fixture(scope="module", autouse=True)
def _sweep_file():
    os.makedirs(os.path.dirname(SWEEP) or ".", exist_ok=True)
    with open(SWEEP, "w") as f:
        f.write("# weight-gradient kernels against float64 at every forced pixel-split count (tests/test_gpu_wgrad_splits.py)\n"
                "# gate: max|dw - ref64| / max|ref64| < 2e-5; launched = splits in the grid (padded to a multiple of 8)\n"
                f"# {'family':<14}{'case':<30}{'nsplit':>7}{'T':>5}{'per':>7}{'empty':>7}{'seam':>6}{'launched':>10}"
                f"{'transitions':>14}{'err/scale':>12}\n")
    yield


def _line(c, n, f, err):
    with open(SWEEP, "a") as fh:
        fh.write(f"  {c.family:<14}{c.id:<30}{n:>7}{f.T:>5}{f.per:>7}{f.empty:>7}{f.straddling:>6}{f.launched:>10}"
                 f"{','.join(sorted(f.transitions)) or '-':>14}{err:>12.3e}\n")


def _problem(c):
    """(x NHWC, gy NHWC, zero parameter on the device, float64 weight gradient) of a case, seeded as the parity tests do."""
    kind, k, stride, pad = LAYER[c.kind]
    g = torch.Generator().manual_seed(c.Ci + 7 * c.H)
    x = torch.randn(c.N, c.H, c.W, c.Ci, generator=g)
    xd = x.permute(0, 3, 1, 2).double()
    if kind == "conv":
        OH, OW = (c.H + 2 * pad - k) // stride + 1, (c.W + 2 * pad - k) // stride + 1
        gy = torch.randn(c.N, OH, OW, c.Co, generator=g)
        w = torch.zeros(c.Co, c.Ci, k, k, device=DEV, requires_grad=True)
        ref = torch.nn.grad.conv2d_weight(xd, (c.Co, c.Ci, k, k), gy.permute(0, 3, 1, 2).double(), stride=stride, padding=pad)
    else:
        gy = torch.randn(c.N, 2 * c.H, 2 * c.W, c.Co, generator=g)
        w = torch.zeros(c.Ci, c.Co, 4, 4, device=DEV, requires_grad=True)
        wr = torch.zeros(c.Ci, c.Co, 4, 4, dtype=torch.float64, requires_grad=True)
        (F.conv_transpose2d(xd, wr, stride=2, padding=1) * gy.permute(0, 3, 1, 2).double()).sum().backward()
        ref = wr.grad
    return x.to(DEV), gy.to(DEV), w, ref


def _poisoned_f(self, *shape, zero=False):
    if zero:
        return torch.zeros(shape, device=self.device, dtype=torch.float32)
    return torch.full(shape, float("nan"), device=self.device, dtype=torch.float32)


def _judge(c, results):
    """`results`: [(nsplit, dw of run 1, dw of run 2)] on the host in float64, ref64 last.  Writes the sweep lines, then asserts."""
    *runs, ref = results
    scale = float(ref.abs().max())
    bad = []
    for n, a, b in runs:
        f = W.facts(c, n)
        finite = bool(torch.isfinite(a).all())
        err = float((a - ref).abs().max()) / scale if finite else math.nan
        _line(c, n, f, err)
        print(f"{c.family} {c.id} nsplit={n} per={f.per} empty={f.empty} err/scale={err:.3e}")
        if not finite:
            bad.append((n, f"{int((~torch.isfinite(a)).sum())} elements no kernel wrote (NaN poison)"))
        elif not err < GATE:
            bad.append((n, f"err/scale {err:.3e}"))
        elif not torch.equal(a, b):
            bad.append((n, "two runs differ bitwise"))
    assert not bad, f"{c.family} {c.id}: {bad}"


ENGINE_CASES = [c for c in W.CASES if c.family != "general"]


@pytest.mark.parametrize("c", ENGINE_CASES, ids=[f"{c.family}-{c.id}" for c in ENGINE_CASES])
def test_weight_gradient_at_every_split_count(c, monkeypatch):
    import adam_dehaze_amd.engine as E
    r = ROUTES[c.family]
    monkeypatch.setenv("ADH_WINO32_WGRAD", "2")
    monkeypatch.setattr(E, "USE_WINOGRAD", r.winograd)
    monkeypatch.setattr(E, "USE_WINO43_WGRAD", r.wino43)
    monkeypatch.setattr(E, "MERGE_CLASSES", r.merge)
    monkeypatch.setattr(E, "GRAD_SINK", None)
    monkeypatch.setattr(Engine, "_f", _poisoned_f)
    x, gy, w, ref = _problem(c)
    kind, k, stride, pad = LAYER[c.kind]
    eng = Engine(torch.device(DEV), record=False)
    plans = eng._launch_plan(kind, k, stride, pad, w, "fwd")
    T = W.tiles(c)

    # the tile count the splits divide: the library's query, or the engine's 4 x 32 row-tile estimate
    for pl in plans:
        d = _wgrad_desc(eng, plans, pl, x, gy, c.Co)
        assert (H.value(r.tiles, C.byref(d)) if r.tiles else d.N * ((d.VH + 3) // 4) * ((d.VW + 31) // 32)) == T
        if c.family == "rows_direct":
            assert H.value("adh_conv_wgrad_groups", C.byref(d)) > 0, "not a shape of conv_wgrad_rows_kernel"
        if c.family.startswith("wino32"):   # one grid for the four classes of a k4 s2 form on the v2 kernels, four launches on v1
            ncls = H.value("adh_conv_wgrad_wino32_classes", C.byref(d))
            assert ncls == (4 if c.kind == "conv4s2" else 1)
            assert H.value("adh_conv_wgrad_wino32_launches", C.byref(d)) == (ncls if W.wino32_variant(c) == "v1" else 1)

    calls = []
    real_call = H.call

    def recording(name, *a, **kw):
        calls.append((name, a))
        return real_call(name, *a, **kw)
    monkeypatch.setattr(H, "call", recording)

    nlaunch = 1 if (r.merge or len(plans) == 1) else len(plans)
    results = []
    for n in W.split_counts(c):
        monkeypatch.setenv("ADH_NSPLIT", str(n))
        runs = []
        for _ in range(2):
            calls.clear()
            dw = eng._wgrad(plans, Act(x), gy, c.Co, w)
            runs.append(dw.cpu().double())
            assert [nm for nm, _ in calls if nm == r.launch] == [r.launch] * nlaunch, (n, [nm for nm, _ in calls])
            assert [nm for nm, _ in calls if nm == r.reduce] == [r.reduce] * len(plans), (n, [nm for nm, _ in calls])
            assert {nm for nm, _ in calls} == {r.launch, r.reduce}, (n, [nm for nm, _ in calls])   # no other kernel took a plan
            assert all(a[r.larg] == n for nm, a in calls if nm == r.launch), (n, calls)
            assert all(a[1] == r.reduce_count(n) for nm, a in calls if nm == r.reduce), (n, calls)
        results.append((n, runs[0], runs[1]))
    _judge(c, results + [ref])


GENERAL_CASES = W.cases_of("general")


@pytest.mark.parametrize("c", GENERAL_CASES, ids=[f"{c.family}-{c.id}" for c in GENERAL_CASES])
def test_general_kernel_at_every_split_count(c):
    """conv_wgrad_kernel (launch_wgrad: grid.y = nsplit, tiles dealt round-robin) + adh_wgrad_reduce through the C ABI, on
    shapes adh_conv_wgrad_groups turns down: a 1x1 and a 3x3 stride-2 layer of the classifier backbones."""
    x, gy, w, ref = _problem(c)
    kind, k, stride, pad = LAYER[c.kind]
    eng = Engine(torch.device(DEV), record=False)
    plans = eng._launch_plan(kind, k, stride, pad, w, "fwd")
    assert len(plans) == 1
    L, gm = plans[0]
    d = _wgrad_desc(eng, plans, plans[0], x, gy, c.Co)      # x and gy are on the device already: `d` points into them
    assert H.value("adh_conv_wgrad_groups", C.byref(d)) == 0, "a shape of conv_wgrad_rows_kernel"
    assert d.N * ((d.VH + 3) // 4) * ((d.VW + 31) // 32) == W.tiles(c)
    KP, NcP, taps = (L.K + 31) // 32 * 32, d.NcP, gm["KH"] * gm["KW"]
    results = []
    for n in W.split_counts(c):
        nslabs = H.value("adh_conv_wgrad_slabs", C.byref(d), n)
        assert nslabs == n
        runs = []
        for _ in range(2):
            slab = torch.full((nslabs * taps * KP * NcP,), float("nan"), device=DEV)
            dw = torch.full(tuple(w.shape), float("nan"), device=DEV)
            H.call("adh_conv_wgrad", C.byref(d), slab.data_ptr(), n)
            H.call("adh_wgrad_reduce", slab.data_ptr(), nslabs, KP, NcP, C.byref(L), dw.data_ptr(), 0)
            runs.append(dw.cpu().double())
        results.append((n, runs[0], runs[1]))
    _judge(c, results + [ref])


@pytest.mark.parametrize("N,Ci,Co,Hh,Ww", W.NOT_ROWS_SHAPES)
def test_shapes_the_winograd_rows_kernel_turns_down(N, Ci, Co, Hh, Ww, monkeypatch):
    """conv_wgrad_rows_kernel takes grids of whole 4 x 32 tiles only: with the F(4x4,3x3) domain off, a 3x3 layer whose
    width is no multiple of 32 or whose height is no multiple of 4 is no F(2x2,3x3) shape either, and its weight gradient
    (the general kernel's, at the engine's own split count) still holds the float64 gate."""
    import adam_dehaze_amd.engine as E
    monkeypatch.setattr(E, "USE_WINOGRAD", True)
    monkeypatch.setattr(E, "USE_WINO43_WGRAD", False)
    monkeypatch.setattr(E, "GRAD_SINK", None)
    monkeypatch.setattr(Engine, "_f", _poisoned_f)
    c = W.Case("general", "conv3", N, Ci, Co, Hh, Ww)
    x, gy, w, ref = _problem(c)
    eng = Engine(torch.device(DEV), record=False)
    plans = eng._launch_plan("conv", 3, 1, 1, w, "fwd")
    d = _wgrad_desc(eng, plans, plans[0], x, gy, Co)
    assert H.value("adh_conv_wgrad_wino_groups", C.byref(d)) == 0
    assert H.value("adh_conv_wgrad_groups", C.byref(d)) == 0
    calls = []
    real_call = H.call

    def recording(name, *a, **kw):
        calls.append(name)
        return real_call(name, *a, **kw)
    monkeypatch.setattr(H, "call", recording)
    dw = eng._wgrad(plans, Act(x), gy, Co, w).cpu().double()
    assert calls == ["adh_conv_wgrad", "adh_wgrad_reduce"], calls
    assert bool(torch.isfinite(dw).all())
    assert float((dw - ref).abs().max()) < GATE * float(ref.abs().max())
