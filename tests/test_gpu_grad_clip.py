"""Global-norm gradient clipping and the non-finite-step guard of the Adam step (csrc/train_io.hip: adh_grad_sumsq,
adh_grad_guard_finalize, adh_adam_multi_guarded; optim.Adam(max_grad_norm, skip_nonfinite)).

The tensors are those of tests/test_gpu_train_io.py's Adam tests: sizes 1, 3, 4, 5, chunk - 1, chunk, chunk + 1, 2 chunk + 7 and
1000 carved from one NaN arena per role, the last one off 16-byte alignment (scalar path), NaN guard bands around every tensor.

Gates
  norm          the partials and their sum are float64 (2^-53 per operation over <= 2 chunk + 7 terms and 12 partials, far
                inside 1e-12 relative); the one fp32 rounding is the conversion of sqrt(sumsq): 2 * 2^-24 relative.
  coefficient   one fp32 rounding of grad_scale * coef: 2 * 2^-24 relative; bit-equal to grad_scale where the float64
                coefficient is 1, and where max_norm is 0 or inf (the header's "measure only": the kernel does not clip there).
  Adam          tests/_ref64.adam's own operation-by-operation bounds with gscale = the block's gscale_eff: the kernel multiplies
                every gradient by one fp32 scalar, as adh_adam_multi does.
"""
import copy
import math
import warnings

import numpy as np
import pytest
import torch

from adam_dehaze_amd import _hip as H
from adam_dehaze_amd.optim import Adam
from tests import _ref64 as R64
from tests._util import DEV, EPS, _nan, _same_bits
from tests.test_gpu_train_io import ADAM_KW, ADAM_POW_UNITS, _AdamState, _adam_sizes

pytestmark = pytest.mark.gpu
GATE = 2 * EPS                  # "gate 1" of the issue: a float64 quantity stored as fp32
I_CHUNK1, I_ONE = 6, 0          # the chunk + 1 tensor (its last element is alone in a second chunk) and the one-element tensor


class _Guard:
    """The float64 partials (NaN guard bands) and a control block (0xAB guard bytes) for one _AdamState."""

    def __init__(self, st):
        self.st = st
        self.pwhole = _nan(st.nchunks + 16, dtype=torch.float64)
        self.partials = self.pwhole[8:8 + st.nchunks]
        self.cwhole = torch.full((32 + 2 * 32,), 0xAB, dtype=torch.uint8, device=DEV)
        self.ctrl = self.cwhole[32:64]
        self.ctrl.zero_()

    def sumsq(self, gscale):
        H.call("adh_grad_sumsq", self.st.table.data_ptr(), self.st.chunks.data_ptr(), self.st.nchunks, gscale,
               self.partials.data_ptr())

    def finalize(self, gscale, max_norm, skip):
        H.call("adh_grad_guard_finalize", self.partials.data_ptr(), self.st.nchunks, gscale, max_norm, int(skip),
               self.ctrl.data_ptr())

    def adam(self, dup_mode, wd, csu, max_repeats=4):
        kw = ADAM_KW
        H.call("adh_adam_multi_guarded", self.st.table.data_ptr(), self.st.chunks.data_ptr(), self.st.nchunks, kw["lr"],
               kw["beta1"], kw["beta2"], kw["eps"], wd, dup_mode, max_repeats, csu, self.ctrl.data_ptr())

    def step(self, dup_mode, wd, gscale, csu, max_norm, skip):
        self.sumsq(gscale)
        self.finalize(gscale, max_norm, skip)
        self.adam(dup_mode, wd, csu)

    def read(self):
        return _read_ctrl(self.ctrl)

    def guards_ok(self):
        c = self.cwhole.cpu()
        return bool(torch.isnan(self.pwhole[:8]).all()) and bool(torch.isnan(self.pwhole[8 + self.st.nchunks:]).all()) \
            and bool((c[:32] == 0xAB).all()) and bool((c[64:] == 0xAB).all())


def _read_ctrl(ctrl_bytes):
    return H.GradCtrl.from_buffer_copy(ctrl_bytes.cpu().numpy().tobytes())


def _f32_bits(x):
    return np.float32(x).view(np.uint32)


def _sumsq64(st, gscale, times=None):
    """sum over the tensors of sum (double(g) * gscale)^2 in float64; `times`: how often each tensor is counted"""
    total = 0.0
    for i in range(len(st.sizes)):
        total += (1 if times is None else times[i]) * float((st.view("g", i).double() * gscale).pow(2).sum())
    return total


# ------------------------------------------------------------------------------------------------ 1. norm
@pytest.mark.parametrize("gscale", [1.0, 0.125])
def test_norm_against_float64(gscale):
    sizes = _adam_sizes()
    repeats = [1, 1, 3, 1, 2, 1, 1, 4, 1]
    st = _AdamState(sizes, repeats, seed=21)
    st.set_grads(1, False)
    st.upload([0] * len(sizes))
    gd = _Guard(st)
    runs = []
    for _ in range(2):
        gd.partials.fill_(float("nan"))
        gd.sumsq(gscale)
        gd.finalize(gscale, 0.0, True)
        torch.cuda.synchronize()
        runs.append((gd.partials.clone(), gd.ctrl.clone()))
    assert _same_bits(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1]), "two runs differ"
    assert gd.guards_ok() and st.guards_ok()
    c = gd.read()
    ref = _sumsq64(st, gscale)
    thrice = _sumsq64(st, gscale, times=repeats)
    rel_s = abs(c.sumsq - ref) / ref
    rel_n = abs(float(c.norm) - math.sqrt(ref)) / math.sqrt(ref)
    print(f"[bound] grad norm gscale={gscale}: sumsq rel err {rel_s:.3e} (gate 1e-12), norm rel err / gate {rel_n / GATE:.3f}")
    assert rel_s <= 1e-12
    assert rel_n <= GATE
    assert abs(c.sumsq - thrice) / thrice > 1e-3, "the test cannot tell once from `repeats` times"
    assert c.finite == 1 and c.skipped == 0 and c.skipped_total == 0
    assert _f32_bits(c.gscale_eff) == _f32_bits(gscale)


def test_norm_of_zero_gradient():
    sizes = _adam_sizes()
    st = _AdamState(sizes, [1] * len(sizes), seed=22)
    st.set_grads(0, True)
    st.upload([0] * len(sizes))
    gd = _Guard(st)
    gd.sumsq(0.125)
    gd.finalize(0.125, 1.0, True)
    torch.cuda.synchronize()
    c = gd.read()
    assert c.sumsq == 0.0 and c.norm == 0.0 and c.finite == 1 and c.skipped == 0
    assert _f32_bits(c.gscale_eff) == _f32_bits(0.125), "coefficient of a zero gradient is 1"
    assert gd.guards_ok()


# ------------------------------------------------------------------------------------------------ 2. coefficient
@pytest.mark.parametrize("gscale", [1.0, 0.125])
def test_coefficient(gscale):
    """max_norm at 0.5, 1 and 2 times the float64 norm: torch's formula.  At inf and at 0 the header says "measure only"
    (coef exactly 1): the formula would give 0 at max_norm 0, the kernel's documented rule is what is asserted there."""
    sizes = _adam_sizes()
    st = _AdamState(sizes, [1] * len(sizes), seed=23)
    st.set_grads(2, False)
    st.upload([0] * len(sizes))
    gd = _Guard(st)
    gd.sumsq(gscale)
    norm64 = math.sqrt(_sumsq64(st, gscale))
    worst = 0.0
    for factor in (0.5, 1.0, 2.0, math.inf, 0.0):
        max_norm = factor * norm64
        gd.finalize(gscale, max_norm, False)
        torch.cuda.synchronize()
        c = gd.read()
        coef = 1.0 if factor in (math.inf, 0.0) else min(1.0, max_norm / (norm64 + 1e-6))
        want = gscale * coef
        rel = abs(float(c.gscale_eff) - want) / want
        worst = max(worst, rel)
        assert rel <= GATE, (factor, float(c.gscale_eff), want)
        if coef == 1.0:
            assert _f32_bits(c.gscale_eff) == _f32_bits(gscale), factor
        elif coef < 1.0 - GATE:              # (at 1 x the norm the coefficient is 1 - 1e-6 / norm: it may round to grad_scale)
            assert float(c.gscale_eff) < gscale
        assert c.finite == 1 and c.skipped == 0
    print(f"[bound] clip coefficient gscale={gscale}: worst rel err / gate {worst / GATE:.3f}")
    assert gd.guards_ok()


# ------------------------------------------------------------------------------------------------ 3. unclipped == unguarded
@pytest.mark.parametrize("dup_mode", [0, 1])
@pytest.mark.parametrize("wd", [0.0, 1e-2])
def test_unclipped_guarded_adam_equals_unguarded(dup_mode, wd):
    sizes = _adam_sizes()
    repeats = [1 + i % 4 for i in range(len(sizes))]
    wd32 = float(np.float32(wd))
    st = _AdamState(sizes, repeats, seed=31 + dup_mode)
    st.upload([0] * len(sizes))
    gd = _Guard(st)
    plain = []
    for k in range(5):
        st.set_grads(k, False)
        st.launch(dup_mode, wd32, 0.125, k)
        plain.append({q: st.arena[q].clone() for q in "pmv"})
    st.reset()
    for k in range(5):
        st.set_grads(k, False)
        gd.step(dup_mode, wd32, 0.125, k, math.inf if k % 2 else 1e30, True)
        for q in "pmv":
            assert _same_bits(st.arena[q][st.owned], plain[k][q][st.owned]), f"launch {k}: {q} differs from adh_adam_multi"
    torch.cuda.synchronize()
    assert st.guards_ok() and gd.guards_ok()
    assert gd.read().skipped_total == 0


# ------------------------------------------------------------------------------------------------ 4. clipped step
@pytest.mark.parametrize("dup_mode", [0, 1])
def test_clipped_step_against_float64(dup_mode):
    """Three clipped launches on a resident table, each against one float64 step from the state the kernel started with,
    gscale = the block's gscale_eff, under _ref64.adam's own bounds."""
    sizes = _adam_sizes()
    repeats = [1 + (i + 1) % 4 for i in range(len(sizes))]
    wd32, gscale = float(np.float32(1e-2)), 0.125
    st = _AdamState(sizes, repeats, seed=41 + dup_mode)
    st.upload([0] * len(sizes))
    gd = _Guard(st)
    sls = [slice(o, o + n) for o, n in zip(st.offs, sizes)]
    worst = {"p": 0.0, "m": 0.0, "v": 0.0}
    before = st.init
    for k in range(3):
        st.set_grads(k, False)
        max_norm = 0.5 * math.sqrt(_sumsq64(st, gscale))
        gd.step(dup_mode, wd32, gscale, k, max_norm, True)
        torch.cuda.synchronize()
        c = gd.read()
        assert c.finite == 1 and 0.49 * gscale < float(c.gscale_eff) < 0.51 * gscale
        after = {q: st.arena[q].clone() for q in "pmv"}
        for i, (n, r, sl) in enumerate(zip(sizes, repeats, sls)):
            ref, bounds = R64.adam(before["p"][sl], st.arena["g"][sl], before["m"][sl], before["v"][sl], k * r, r, dup_mode,
                                   wd=wd32, gscale=float(c.gscale_eff), pow_units=ADAM_POW_UNITS, **ADAM_KW)
            for q, want, e in zip("pmv", ref, bounds):
                got = after[q][sl]
                assert not torch.isnan(got).any()
                err = (got.double() - want).abs()
                if float(err.max()) > 0:
                    worst[q] = max(worst[q], float((err / e.clamp_min(1e-300)).max()))
                over = float((err - e).max())
                assert over <= 0, f"tensor {i} (n={n}, repeats={r}) launch {k}: {q} is {over:.3e} over its bound"
        before = after
    assert st.guards_ok() and gd.guards_ok()
    print(f"[bound] clipped adam worst |err| / bound: {worst}")


def _carve(st):
    """the p tensors of an _AdamState as optimiser parameters: gradients are the g arena's views (stable pointers)"""
    params = [st.view("p", i) for i in range(len(st.sizes))]
    for i, p in enumerate(params):
        p.grad = st.view("g", i)
    return params


def _seed_state(opt, st, params):
    """Adam state inside the m / v arenas, so their guard bands watch the optimiser's launches too"""
    for i, p in enumerate(params):
        opt.state[id(p)] = {"step": 0, "m": st.view("m", i), "v": st.view("v", i)}


KW32 = dict(lr=ADAM_KW["lr"], betas=(ADAM_KW["beta1"], ADAM_KW["beta2"]), eps=ADAM_KW["eps"])


def test_clipped_steps_against_torch_float64():
    """optim.Adam(max_grad_norm) for three steps against torch.nn.utils.clip_grad_norm_ + torch.optim.Adam in float64 on the
    CPU, no duplicates.  Tolerance: _ref64.adam's per-step bounds (evaluated along the float64 trajectory, gscale = torch's
    own coefficient) summed over the three steps."""
    sizes = _adam_sizes()
    n = len(sizes)
    wd32 = float(np.float32(1e-2))
    st = _AdamState(sizes, [1] * n, seed=43)
    params = _carve(st)
    st.set_grads(0, False)
    max_norm = 0.5 * math.sqrt(_sumsq64(st, 1.0))
    opt = Adam(params, weight_decay=wd32, max_grad_norm=max_norm, **KW32)
    _seed_state(opt, st, params)
    cpu = [torch.nn.Parameter(st.view("p", i).detach().cpu().double()) for i in range(n)]
    ref = torch.optim.Adam(cpu, lr=KW32["lr"], betas=KW32["betas"], eps=KW32["eps"], weight_decay=wd32, foreach=False)
    for i, q in enumerate(cpu):
        ref.state[q] = {"step": torch.tensor(0.0), "exp_avg": st.view("m", i).cpu().double(),
                        "exp_avg_sq": st.view("v", i).cpu().double()}
    tol = {q: [torch.zeros(s, dtype=torch.float64) for s in sizes] for q in "pmv"}
    for k in range(3):
        st.set_grads(k, False)
        for i, q in enumerate(cpu):
            q.grad = st.view("g", i).cpu().double()
        norm = float(torch.sqrt(sum(q.grad.pow(2).sum() for q in cpu)))
        coef = min(1.0, max_norm / (norm + 1e-6))
        for i, q in enumerate(cpu):
            s = ref.state[q]
            _, bounds = R64.adam(q.detach(), st.view("g", i).cpu(), s["exp_avg"], s["exp_avg_sq"], k, 1, 0, wd=wd32,
                                 gscale=coef, pow_units=ADAM_POW_UNITS, **ADAM_KW)
            for name, e in zip("pmv", bounds):
                tol[name][i] += e
        torch.nn.utils.clip_grad_norm_(cpu, max_norm)
        ref.step()
        opt.step()
        assert coef < 1.0
    torch.cuda.synchronize()
    assert abs(float(opt.last_grad_norm) - norm) <= GATE * norm
    worst = {"p": 0.0, "m": 0.0, "v": 0.0}
    for i, q in enumerate(cpu):
        s = ref.state[q]
        for name, want in (("p", q.detach()), ("m", s["exp_avg"]), ("v", s["exp_avg_sq"])):
            err = (st.view(name, i).cpu().double() - want).abs()
            worst[name] = max(worst[name], float((err / tol[name][i].clamp_min(1e-300)).max()))
    print(f"[bound] clipped adam vs torch float64, 3 steps, worst |err| / summed bound: {worst}")
    assert max(worst.values()) <= 1.0, worst
    assert st.guards_ok()
    assert opt.state_dict()["state"][0]["step"] == 3


# ------------------------------------------------------------------------------------------------ 5. non-finite step
def _nonfinite_sequence(index, value, new_grad_buffer):
    """skip_nonfinite=True: a step with `value` planted in the last element of tensor `index`, then a finite step.  With
    `new_grad_buffer` the second step's gradients live in another allocation, which forces a table re-upload between the two;
    otherwise the table stays resident and calls_since_upload grows across the skip.  Returns the final p, m, v."""
    sizes = _adam_sizes()
    n = len(sizes)
    wd32 = float(np.float32(1e-2))
    st = _AdamState(sizes, [1] * n, seed=51)
    params = _carve(st)
    st.set_grads(0, False)
    max_norm = 0.5 * math.sqrt(_sumsq64(st, 1.0))
    opt = Adam(params, weight_decay=wd32, max_grad_norm=max_norm, skip_nonfinite=True, **KW32)
    _seed_state(opt, st, params)
    st.view("g", index)[-1] = value
    opt.step()
    torch.cuda.synchronize()
    for q in "pmv":
        assert _same_bits(st.arena[q], st.init[q]), f"a skipped step wrote {q} (or its guard bands)"
    assert opt.skipped_steps() == 1
    assert not math.isfinite(float(opt.last_grad_norm))
    st.set_grads(0, False)
    if new_grad_buffer:
        other = st.arena["g"].clone()
        for i, p in enumerate(params):
            p.grad = other[st.offs[i]:st.offs[i] + sizes[i]]
    opt.step()
    torch.cuda.synchronize()
    assert opt._calls_since_upload == (1 if new_grad_buffer else 2)
    assert opt.skipped_steps() == 1 and math.isfinite(float(opt.last_grad_norm))
    got = {q: st.arena[q].clone() for q in "pmv"}
    assert st.guards_ok()
    sd = opt.state_dict()
    assert all(float(sd["state"][i]["step"]) == 1 for i in range(n)), [float(sd["state"][i]["step"]) for i in range(n)]
    # the first step of a fresh optimiser from the same state on the same gradients
    st.reset()
    fresh = Adam(params, weight_decay=wd32, max_grad_norm=max_norm, skip_nonfinite=True, **KW32)
    _seed_state(fresh, st, params)
    fresh.step()
    torch.cuda.synchronize()
    for q in "pmv":
        assert _same_bits(st.arena[q][st.owned], got[q][st.owned]), f"{q}: the step after a skip is not a first step"
    assert fresh.skipped_steps() == 0
    return got


@pytest.mark.parametrize("index,value", [(I_CHUNK1, float("inf")), (I_ONE, float("nan"))])
def test_nonfinite_step_is_skipped(index, value):
    resident = _nonfinite_sequence(index, value, new_grad_buffer=False)
    reuploaded = _nonfinite_sequence(index, value, new_grad_buffer=True)
    for q in "pmv":
        assert _same_bits(resident[q], reuploaded[q]), f"{q}: resident table and re-uploaded table differ"


@pytest.mark.parametrize("index,value", [(I_CHUNK1, float("inf")), (I_ONE, float("nan"))])
def test_nonfinite_step_without_skip_is_todays_behaviour(index, value):
    sizes = _adam_sizes()
    repeats = [1 + i % 4 for i in range(len(sizes))]
    wd32 = float(np.float32(1e-2))
    st = _AdamState(sizes, repeats, seed=52)
    st.set_grads(0, False)
    st.view("g", index)[-1] = value
    st.upload([0] * len(sizes))
    st.launch(0, wd32, 0.125, 0)
    plain = {q: st.arena[q].clone() for q in "pmv"}
    st.reset()
    gd = _Guard(st)
    gd.step(0, wd32, 0.125, 0, 1.0, False)       # max_norm far below the norm: a finite gradient would be clipped
    torch.cuda.synchronize()
    c = gd.read()
    assert c.finite == 1 and c.skipped == 0 and c.skipped_total == 0 and not math.isfinite(float(c.norm))
    assert _f32_bits(c.gscale_eff) == _f32_bits(0.125)
    for q in "pmv":
        assert _same_bits(st.arena[q], plain[q]), q
    assert not torch.isfinite(st.view("v", index)[-1]), "the non-finite gradient reaches the state, as it does today"
    assert gd.guards_ok()


# ------------------------------------------------------------------------------------------------ 6. checkpoint round trip
def _five_grads(st, k, bad_at):
    st.set_grads(k, False)
    if k == bad_at:
        st.view("g", I_CHUNK1)[-1] = float("inf")


@pytest.mark.parametrize("duplicates", ["sequential", "foreach"])
def test_checkpoint_round_trip_across_a_skip(duplicates):
    """3 step() calls of which the second is skipped, state_dict() -> new Adam -> load_state_dict -> 2 more, against the same
    5 step() calls on one optimiser: bit-equal p, m, v and step counts."""
    sizes = _adam_sizes()
    n = len(sizes)
    twice = [i for i in range(n) if i % 2]          # these are listed twice
    wd32 = float(np.float32(1e-2))
    kw = dict(weight_decay=wd32, max_grad_norm=30.0, skip_nonfinite=True, duplicates=duplicates, **KW32)

    def listed(params):
        return params + [params[i] for i in twice]

    st = _AdamState(sizes, [1] * n, seed=61)
    params = _carve(st)
    one = Adam(listed(params), **kw)
    for k in range(5):
        _five_grads(st, k, 1)
        one.step()
    torch.cuda.synchronize()
    want_p = st.arena["p"].clone()
    want_sd = one.state_dict()
    assert one.skipped_steps() == 1
    st.reset()
    a = Adam(listed(params), **kw)
    for k in range(3):
        _five_grads(st, k, 1)
        a.step()
    sd = copy.deepcopy(a.state_dict())
    assert a.skipped_steps() == 1
    b = Adam(listed(params), **kw)
    b.load_state_dict(sd)
    for k in range(3, 5):
        _five_grads(st, k, 1)
        b.step()
    torch.cuda.synchronize()
    assert b.skipped_steps() == 0
    assert _same_bits(st.arena["p"][st.owned], want_p[st.owned])
    got_sd = b.state_dict()
    assert sorted(got_sd["state"]) == sorted(want_sd["state"])
    for idx, s in want_sd["state"].items():
        g = got_sd["state"][idx]
        assert float(g["step"]) == float(s["step"]), (idx, float(g["step"]), float(s["step"]))
        assert _same_bits(g["exp_avg"], s["exp_avg"]) and _same_bits(g["exp_avg_sq"], s["exp_avg_sq"]), idx
    steps = sorted({float(s["step"]) for s in want_sd["state"].values()})
    assert steps == [4.0, 8.0], steps              # 4 steps taken, 8 by the tensors listed twice: the skip consumed none
    assert st.guards_ok()


# ------------------------------------------------------------------------------------------------ 7. rejects
def test_guard_entry_points_reject():
    st = _AdamState([5, 9], [1, 2], seed=71)
    st.set_grads(0, False)
    st.upload([0, 0])
    gd = _Guard(st)
    gd.step(0, 0.0, 1.0, 0, 0.0, True)              # a valid block, so that what must stay unwritten has a value
    torch.cuda.synchronize()
    before = {q: st.arena[q].clone() for q in "pmv"}
    pw, cw = gd.pwhole.clone(), gd.cwhole.clone()
    tab, ch, part, ctrl, nc = st.table.data_ptr(), st.chunks.data_ptr(), gd.partials.data_ptr(), gd.ctrl.data_ptr(), st.nchunks
    kw = ADAM_KW
    hp = (kw["lr"], kw["beta1"], kw["beta2"], kw["eps"], 0.0)
    bad = [("adh_grad_sumsq", (None, ch, nc, 1.0, part)), ("adh_grad_sumsq", (tab, None, nc, 1.0, part)),
           ("adh_grad_sumsq", (tab, ch, nc, 1.0, None)), ("adh_grad_sumsq", (tab, ch, 0, 1.0, part)),
           ("adh_grad_sumsq", (tab, ch, -1, 1.0, part)),
           ("adh_grad_guard_finalize", (None, nc, 1.0, 1.0, 1, ctrl)), ("adh_grad_guard_finalize", (part, nc, 1.0, 1.0, 1, None)),
           ("adh_grad_guard_finalize", (part, 0, 1.0, 1.0, 1, ctrl)), ("adh_grad_guard_finalize", (part, nc, 1.0, 1.0, 2, ctrl)),
           ("adh_adam_multi_guarded", (None, ch, nc) + hp + (0, 4, 0, ctrl)),
           ("adh_adam_multi_guarded", (tab, None, nc) + hp + (0, 4, 0, ctrl)),
           ("adh_adam_multi_guarded", (tab, ch, nc) + hp + (0, 4, 0, None)),
           ("adh_adam_multi_guarded", (tab, ch, 0) + hp + (0, 4, 0, ctrl)),
           ("adh_adam_multi_guarded", (tab, ch, nc) + hp + (0, 4, -1, ctrl)),
           ("adh_adam_multi_guarded", (tab, ch, nc) + hp + (2, 4, 0, ctrl)),
           ("adh_adam_multi_guarded", (tab, ch, nc) + hp + (0, 5, 0, ctrl)),
           ("adh_adam_multi_guarded", (tab, ch, nc) + hp + (0, 0, 0, ctrl))]
    for name, args in bad:
        with pytest.raises(RuntimeError):
            H.call(name, *args)
    torch.cuda.synchronize()
    for q in "pmv":
        assert _same_bits(st.arena[q], before[q]), q
    assert _same_bits(gd.pwhole, pw) and torch.equal(gd.cwhole, cw)


def test_adam_argument_validation_on_device():
    p = torch.zeros(4, device=DEV)
    for bad in (-1.0, float("nan")):
        with pytest.raises(ValueError):
            Adam([p], max_grad_norm=bad)
    opt = Adam([p])
    assert not opt.guarded and opt.last_grad_norm is None and opt.skipped_steps() == 0


# ------------------------------------------------------------------------------------------------ 8. one joint step
def _joint_step(grad_clip_norm):
    from adam_dehaze_amd import train as T
    from tests.test_gpu_train import _cfg
    cfg = _cfg()
    cfg["optim"] = {"grad_clip_norm": grad_clip_norm}
    torch.manual_seed(2)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        system = T.build_joint_system(cfg)
    system["classifier"].train()
    system["router"].train()
    opt = system["optimizer"]
    before = [p.detach().clone() for p in opt.params]
    batch = next(T.synthetic_loader(4, 32, 1, seed=5, device=DEV))
    T.joint_train_step(system, batch)
    torch.cuda.synchronize()
    return opt, before


def test_joint_step_with_clipping():
    """One reduced-width joint step (the system of tests/test_gpu_train.py, 4 x 32 x 32), measured and then clipped to a tenth of
    the measured norm.  A tensor whose gradient and value are both identically zero cannot move (a ConvTranspose bias in front
    of a train-mode BatchNorm: true gradient 0, initial value 0, weight decay of 0); every other one must."""
    free, before_f = _joint_step(float("inf"))
    measured = float(free.last_grad_norm)
    assert math.isfinite(measured) and measured > 0
    sq = sum(float(p.grad.double().pow(2).sum()) for p in free.params if p.grad is not None)
    rel = abs(measured - math.sqrt(sq)) / math.sqrt(sq)
    print(f"[bound] joint step: grad norm {measured:.6g}, rel err vs float64 / gate {rel / GATE:.3f}")
    assert rel <= GATE
    clipped, before_c = _joint_step(0.1 * measured)
    assert len(clipped.params) == len(free.params) and max(clipped.repeats.values()) == 2
    for a, b in zip(before_f, before_c):
        assert torch.equal(a, b), "the twins do not start from the same parameters"
    assert abs(float(clipped.last_grad_norm) - measured) <= 1e-3 * measured, "the twins do not see the same gradient"
    c = _read_ctrl(clipped._ctrl)
    assert c.finite == 1 and abs(float(c.gscale_eff) - 0.1) <= 1e-3
    still, must = [], 0
    for i, (p, b) in enumerate(zip(clipped.params, before_c)):
        if p.grad is None or not (bool((p.grad != 0).any()) or bool((b != 0).any())):
            continue
        must += 1
        if torch.equal(p.detach(), b):
            still.append((i, tuple(p.shape)))
    assert must >= 0.9 * len(clipped.params), (must, len(clipped.params))
    assert not still, still[:8]

    def moved(opt, before):
        return math.sqrt(sum(float((p.detach().double() - b.double()).pow(2).sum()) for p, b in zip(opt.params, before)))
    d_free, d_clip = moved(free, before_f), moved(clipped, before_c)
    print(f"[measure] joint step: |dp| unclipped {d_free:.6e}, clipped to a tenth of the norm {d_clip:.6e}")
    assert d_clip < d_free
    assert clipped.skipped_steps() == 0
