"""The weight EMA on the GPU (csrc/ema.hip: adh_ema_begin, adh_ema_multi, adh_ema_swap; ema.WeightEMA; the `ema:` config section).

The tensors are tests/_ema_ref64.TENSORS: 1, 3, 4, 1021, chunk, chunk + 1 and 2 chunk + 7 floats carved from one NaN-poisoned
arena per role with guard bands around every tensor; the 1021 tensor has p and ema one float off 16-byte alignment (scalar path),
the chunk + 1 tensor only ema.  Values are N(0, 1) scaled per tensor by 1e-3, 1 or 1e3.

Gates
  blend     three fp32 roundings (two where the compiler contracts w * d + ema) of quantities no larger than |p| + |ema|:
            |gpu - float64| <= 4 * 2^-24 * (|p| + |ema|) per element after one update with the float w the reference computes
            itself; K chained updates at most K times that on the running maxima of the float64 trajectory (_ema_ref64).
  weight    w is computed in double and rounded once: it must EQUAL np.float32(1 - d), and `updates` the count.
  the rest  bit equality: skipped steps, swaps, guard bands, run-to-run, EMA weights loaded into a fresh system.
"""
import copy
import os
import re
import warnings

import numpy as np
import pytest
import torch

from adam_dehaze_amd import _hip as H
from adam_dehaze_amd import train as T
from adam_dehaze_amd.ema import WeightEMA
from adam_dehaze_amd.optim import Adam
from tests import _ema_ref64 as R
from tests._util import DEV, _same_bits

pytestmark = pytest.mark.gpu
PAD = 64


class _State:
    """p and ema arenas (NaN everywhere outside the tensors), the device table, the chunk list and a control block between guard
    bytes."""

    def __init__(self, seed):
        self.data = R.inputs(seed)
        self.starts = {"p": [], "e": []}
        cur = {"p": PAD, "e": PAD}
        for n, po, eo, _ in R.TENSORS:
            for q, off in (("p", po), ("e", eo)):
                start = (cur[q] + 3) // 4 * 4 + off
                self.starts[q].append(start)
                cur[q] = start + n + PAD
        self.arena = {q: torch.full((cur[q],), float("nan"), device=DEV) for q in "pe"}
        assert all(a.data_ptr() % 16 == 0 for a in self.arena.values())
        self.owned = {q: torch.zeros(cur[q], dtype=torch.bool, device=DEV) for q in "pe"}
        for i, (p, e) in enumerate(self.data):
            self.view("p", i).copy_(p)
            self.view("e", i).copy_(e)
            for q in "pe":
                self.owned[q][self.starts[q][i]:self.starts[q][i] + p.numel()] = True
        for i, (n, po, eo, _) in enumerate(R.TENSORS):
            assert self.view("p", i).data_ptr() % 16 == 4 * po and self.view("e", i).data_ptr() % 16 == 4 * eo
        self.init = {q: self.arena[q].clone() for q in "pe"}
        table = (H.EmaTensor * len(R.TENSORS))()
        pairs = []
        for i, (n, _, _, _) in enumerate(R.TENSORS):
            table[i].p, table[i].ema, table[i].n = self.view("p", i).data_ptr(), self.view("e", i).data_ptr(), n
            pairs += [(i, c) for c in range((n + R.CHUNK - 1) // R.CHUNK)]
        assert R.CHUNK == H.value("adh_adam_chunk_elems")
        self.table = torch.from_numpy(np.frombuffer(bytes(table), dtype=np.uint8).copy()).to(DEV)
        self.chunks = torch.tensor(pairs, dtype=torch.int32).reshape(-1).to(DEV)
        self.nchunks = len(pairs)
        self.cwhole = torch.full((16 + 2 * 32,), 0xAB, dtype=torch.uint8, device=DEV)
        self.ctrl = self.cwhole[32:48]
        self.ctrl.zero_()

    def view(self, q, i):
        s = self.starts[q][i]
        return self.arena[q][s:s + R.TENSORS[i][0]]

    def reset(self):
        for q in "pe":
            self.arena[q].copy_(self.init[q])
        self.ctrl.zero_()

    def begin(self, decay, warmup, guard=None):
        H.call("adh_ema_begin", self.ctrl.data_ptr(), decay, int(warmup), None if guard is None else guard.data_ptr())

    def multi(self):
        H.call("adh_ema_multi", self.table.data_ptr(), self.chunks.data_ptr(), self.nchunks, self.ctrl.data_ptr())

    def swap(self):
        H.call("adh_ema_swap", self.table.data_ptr(), self.chunks.data_ptr(), self.nchunks)

    def read(self):
        return H.EmaCtrl.from_buffer_copy(self.ctrl.cpu().numpy().tobytes())

    def guards_ok(self, p_too=True):
        """everything outside the tensors holds its poison, bit for bit (and p itself, which an update only reads)"""
        c = self.cwhole.cpu()
        ok = bool((c[:32] == 0xAB).all()) and bool((c[48:] == 0xAB).all())
        for q in "pe":
            ok = ok and _same_bits(self.arena[q][~self.owned[q]], self.init[q][~self.owned[q]])
        return ok and (not p_too or _same_bits(self.arena["p"], self.init["p"]))


def _guard_block(finite):
    blk = H.GradCtrl()
    blk.finite, blk.norm, blk.gscale_eff = finite, 1.0, 1.0
    return torch.from_numpy(np.frombuffer(bytes(blk), dtype=np.uint8).copy()).to(DEV)


def _f32_bits(x):
    return np.float32(x).view(np.uint32)


# ------------------------------------------------------------------------------------------------ 1. the blend
@pytest.mark.parametrize("decay,warmup,steps", [(0.9, False, 1), (0.999, True, 1), (0.9, False, 5), (0.999, True, 5)])
def test_update_against_float64(decay, warmup, steps):
    st = _State(seed=11)
    gen = torch.Generator().manual_seed(12)
    runs = []
    for _ in range(2):
        st.reset()
        gen.manual_seed(12)
        trajs = [R.Trajectory(e) for _, e in st.data]
        updates = 0
        for k in range(steps):
            if k:                                            # the parameters move between updates, as they do in training
                for i, (n, _, _, s) in enumerate(R.TENSORS):
                    st.view("p", i).copy_(torch.randn(n, generator=gen) * s)
            st.begin(decay, warmup)
            st.multi()
            updates, active, w = R.begin(updates, decay, warmup)
            for i, t in enumerate(trajs):
                t.step(st.view("p", i), w)
        torch.cuda.synchronize()
        runs.append((st.arena["e"].clone(), st.ctrl.clone()))
    assert _same_bits(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1]), "two runs differ"
    assert st.guards_ok(p_too=steps == 1)
    c = st.read()
    assert (c.updates, c.active) == (steps, 1) and _f32_bits(c.w) == _f32_bits(w)
    worst = 0.0
    for i, t in enumerate(trajs):
        got = st.view("e", i).cpu()
        assert not torch.isnan(got).any()
        err = (got.double() - t.ema).abs()
        worst = max(worst, float((err / t.bound().clamp_min(1e-300)).max()))
        assert bool((err <= t.bound()).all()), f"tensor {i} (n={R.TENSORS[i][0]}): {float((err - t.bound()).max()):.3e} over its bound"
        assert not torch.equal(got, st.data[i][1]), f"tensor {i}: the shadow did not move"
    print(f"[bound] ema decay={decay} warmup={warmup} {steps} update(s): worst |err| / bound {worst:.3f}")


# ------------------------------------------------------------------------------------------------ 2. blend weight and counter
@pytest.mark.parametrize("decay", [0.999, 0.5])
def test_blend_weight_and_counter(decay):
    st = _State(seed=13)
    for t in range(1, 13):                                   # warm-up on: (1 + t) / (10 + t) passes 0.5 at t = 8
        st.begin(decay, True)
        c = st.read()
        want = np.float32(1.0 - min(decay, (1 + t) / (10 + t)))
        assert c.updates == t and c.active == 1
        assert _f32_bits(c.w) == _f32_bits(want), (t, float(c.w), float(want))
    st.ctrl.zero_()
    for t in range(1, 4):
        st.begin(decay, False)
        c = st.read()
        assert c.updates == t and _f32_bits(c.w) == _f32_bits(np.float32(1.0 - decay))
    assert st.guards_ok()
    assert _same_bits(st.arena["e"], st.init["e"]), "adh_ema_begin touches the control block only"


# ------------------------------------------------------------------------------------------------ 3. skip
def test_skip_follows_the_guard_block():
    st = _State(seed=14)
    st.begin(0.9, True)
    st.multi()
    torch.cuda.synchronize()
    after_one = st.arena["e"].clone()
    st.begin(0.9, True, guard=_guard_block(0))
    st.multi()
    torch.cuda.synchronize()
    c = st.read()
    assert (c.updates, c.active) == (1, 0)
    assert _same_bits(st.arena["e"], after_one), "a skipped update wrote the shadows (or their guard bands)"
    assert st.guards_ok()
    # finite = 1 is the null pointer
    st.reset()
    st.begin(0.9, True, guard=_guard_block(1))
    st.multi()
    torch.cuda.synchronize()
    assert _same_bits(st.arena["e"], after_one)
    c = st.read()
    assert (c.updates, c.active) == (1, 1) and _f32_bits(c.w) == _f32_bits(R.begin(0, 0.9, True)[2])


def _three(lr=1e-2, **kw):
    torch.manual_seed(3)
    params = [torch.randn(n, device=DEV) for n in (5, 300, R.CHUNK + 3)]
    for p in params:
        p.grad = torch.randn_like(p)
    return params, Adam(params, lr=lr, **kw)


def test_skipped_optimiser_step_skips_the_ema():
    params, opt = _three(skip_nonfinite=True)
    ema = WeightEMA(params, decay=0.9, warmup=False)
    for s in ema.shadow:
        s.add_(1.0)                                          # away from the parameters: an update would show
    p0, s0 = [p.clone() for p in params], [s.clone() for s in ema.shadow]
    params[1].grad[17] = float("inf")
    opt.step()
    ema.update(opt)
    torch.cuda.synchronize()
    for p, a, s, b in zip(params, p0, ema.shadow, s0):
        assert _same_bits(p, a) and _same_bits(s, b)
    assert ema.updates() == 0 and opt.skipped_steps() == 1
    params[1].grad[17] = 0.5
    opt.step()
    ema.update(opt)
    torch.cuda.synchronize()
    assert ema.updates() == 1 and opt.skipped_steps() == 1
    w = np.float32(1.0 - 0.9)
    for p, a, s, b in zip(params, p0, ema.shadow, s0):
        assert not torch.equal(p, a) and not torch.equal(s, b)
        err = (s.double().cpu() - R.blend(p, b, w)).abs()
        assert bool((err <= R.bound(p.abs(), torch.maximum(b.abs(), s.abs()))).all())


# ------------------------------------------------------------------------------------------------ 4. swap
def test_swap_exchanges_bit_for_bit():
    st = _State(seed=15)
    st.view("p", 3)[5] = float("nan")
    st.view("e", 6)[R.CHUNK + 3] = float("-inf")
    before = {q: [st.view(q, i).clone() for i in range(len(R.TENSORS))] for q in "pe"}
    whole = {q: st.arena[q].clone() for q in "pe"}
    ptrs = [(st.view("p", i).data_ptr(), st.view("e", i).data_ptr()) for i in range(len(R.TENSORS))]
    st.swap()
    torch.cuda.synchronize()
    for i in range(len(R.TENSORS)):
        if i not in (3, 6):
            assert torch.equal(st.view("p", i), before["e"][i]) and torch.equal(st.view("e", i), before["p"][i]), i
        assert _same_bits(st.view("p", i), before["e"][i]) and _same_bits(st.view("e", i), before["p"][i]), i
    for q in "pe":
        assert _same_bits(st.arena[q][~st.owned[q]], whole[q][~st.owned[q]]), "guard bands"
    st.swap()
    torch.cuda.synchronize()
    for q in "pe":
        assert _same_bits(st.arena[q], whole[q]), "a second swap restores both"
    assert ptrs == [(st.view("p", i).data_ptr(), st.view("e", i).data_ptr()) for i in range(len(R.TENSORS))]
    assert bytes(st.ctrl.cpu().numpy()) == bytes(16)


def test_applied_swaps_in_and_back():
    params, opt = _three()
    ema = WeightEMA(params, decay=0.5, warmup=False)
    opt.step()
    ema.update(opt)
    raw, shadow = [p.clone() for p in params], [s.clone() for s in ema.shadow]
    ptrs = [p.data_ptr() for p in params]
    with pytest.raises(KeyError):
        with ema.applied():
            for p, s, a, b in zip(params, ema.shadow, raw, shadow):
                assert torch.equal(p, b) and torch.equal(s, a) and not torch.equal(a, b)
            with pytest.raises(RuntimeError):
                ema.update(opt)
            raise KeyError("body")
    for p, s, a, b in zip(params, ema.shadow, raw, shadow):
        assert torch.equal(p, a) and torch.equal(s, b)
    assert ptrs == [p.data_ptr() for p in params] and ema.updates() == 1 and ema.uploads == 1


# ------------------------------------------------------------------------------------------------ 5. duplicates
def test_a_parameter_listed_twice_advances_once():
    torch.manual_seed(4)
    a, b = torch.randn(R.CHUNK + 9, device=DEV), torch.randn(33, device=DEV)
    a.grad, b.grad = torch.randn_like(a), torch.randn_like(b)
    listed = [a, b, a]
    opt = Adam(listed, lr=1e-1)
    ema = WeightEMA(listed, decay=0.5, warmup=False)
    assert len(ema.params) == 2 and opt.repeats[id(a)] == 2
    before = [a.clone(), b.clone()]
    opt.step()
    ema.update(opt)
    torch.cuda.synchronize()
    assert ema.updates() == 1
    for p, p0, s in zip((a, b), before, ema.shadow):
        once = R.blend(p, p0, np.float32(0.5))
        twice = R.blend(p, once, np.float32(0.5))
        bound = R.bound(p.abs(), torch.maximum(p0.abs(), s.abs()))
        err = (s.double().cpu() - once).abs()
        assert bool((err <= bound).all())
        assert bool(((twice - once).abs() > 100 * bound).any()), "the test cannot tell one update from two"


# ------------------------------------------------------------------------------------------------ 6. rejects
def test_entry_points_reject():
    st = _State(seed=16)
    tab, ch, nc, ctrl = st.table.data_ptr(), st.chunks.data_ptr(), st.nchunks, st.ctrl.data_ptr()
    guard = _guard_block(1)
    bad = [("adh_ema_begin", (None, 0.9, 1, None)), ("adh_ema_begin", (ctrl, 1.0, 1, None)),
           ("adh_ema_begin", (ctrl, -0.1, 1, None)), ("adh_ema_begin", (ctrl, float("nan"), 1, None)),
           ("adh_ema_begin", (ctrl + 4, 0.9, 1, None)), ("adh_ema_begin", (ctrl, 0.9, 1, guard.data_ptr() + 4)),
           ("adh_ema_multi", (None, ch, nc, ctrl)), ("adh_ema_multi", (tab, None, nc, ctrl)),
           ("adh_ema_multi", (tab, ch, nc, None)), ("adh_ema_multi", (tab, ch, 0, ctrl)),
           ("adh_ema_multi", (tab, ch, nc, ctrl + 4)),
           ("adh_ema_swap", (None, ch, nc)), ("adh_ema_swap", (tab, None, nc)), ("adh_ema_swap", (tab, ch, 0)),
           ("adh_ema_swap", (tab, ch, -1))]
    for name, args in bad:
        with pytest.raises(RuntimeError):
            H.call(name, *args)
    torch.cuda.synchronize()
    assert st.guards_ok() and _same_bits(st.arena["e"], st.init["e"]) and bytes(st.ctrl.cpu().numpy()) == bytes(16)
    with pytest.raises(RuntimeError):
        WeightEMA([torch.zeros(3)])                          # a CPU tensor


# ------------------------------------------------------------------------------------------------ 7. the joint system
def _joint(ema_section, seed=2):
    from tests.test_gpu_train import _cfg
    cfg = _cfg()
    if ema_section is not None:
        cfg["ema"] = ema_section
    torch.manual_seed(seed)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        system = T.build_joint_system(cfg)
    return system


def _train_mode(system, on=True):
    system["classifier"].train(on)
    for m in system["models"].values():
        m.train(on)
    system["router"].train(on)


def _routed(system, hazy):
    with torch.no_grad():
        logits, _ = system["classifier"](hazy)
        out, _ = system["router"](hazy, logits)
    return out.clone()


class _Names:
    """H.call with the entry-point names written down (the launches still run)"""

    def __init__(self, monkeypatch):
        self.names, real = [], H.call

        def call(name, *a, **k):
            self.names.append(name)
            return real(name, *a, **k)
        monkeypatch.setattr(H, "call", call)


def test_joint_system_keeps_validates_and_restores_an_ema(monkeypatch):
    system = _joint({"decay": 0.9, "warmup": False})
    ema, router, opt = system["ema"], system["router"], system["optimizer"]
    unique = list(router.parameters())
    assert isinstance(ema, WeightEMA) and [id(p) for p in ema.params] == [id(p) for p in unique]
    assert max(opt.repeats.values()) == 2 and len(opt._listed) > len(unique), "the optimiser lists the branches twice"
    _train_mode(system)
    trajs = [R.Trajectory(p) for p in unique]                # the shadow starts at the parameters
    w = np.float32(1.0 - 0.9)
    batches = list(T.synthetic_loader(4, 64, 3, seed=7, device=DEV))
    rec = _Names(monkeypatch)
    for batch in batches[:2]:
        T.joint_train_step(system, batch)
        for t, p in zip(trajs, unique):
            t.step(p, w)
    torch.cuda.synchronize()
    assert rec.names[-2:] == ["adh_ema_begin", "adh_ema_multi"] and rec.names.count("adh_ema_multi") == 2
    assert ema.updates() == 2 and ema.uploads == 1
    worst, moved = 0.0, 0
    for t, s, p in zip(trajs, ema.shadow, unique):
        err = (s.double().cpu() - t.ema).abs()
        worst = max(worst, float((err / t.bound().clamp_min(1e-300)).max()))
        assert bool((err <= t.bound()).all())
        moved += int(not torch.equal(s, p.detach()))
    print(f"[bound] joint ema after 2 steps: worst |err| / bound {worst:.3f}; {moved} of {len(unique)} shadows differ from p")
    assert moved >= 0.9 * len(unique)
    # validation weights
    hazy = batches[2]["hazy"]
    _train_mode(system, False)
    raw_out = _routed(system, hazy)
    raw = [p.detach().clone() for p in unique]
    sd = copy.deepcopy(ema.state_dict(router))
    with ema.applied():
        ema_out = _routed(system, hazy)
    assert not torch.equal(ema_out, raw_out), "inside applied() the router runs on other weights"
    for p, a in zip(unique, raw):
        assert _same_bits(p.detach(), a), "applied() did not restore a parameter"
    assert torch.equal(_routed(system, hazy), raw_out), "the packed copies of the EMA weights outlived the context"
    fresh = _joint(None, seed=99)
    assert fresh["ema"] is None
    fresh["router"].load_state_dict(sd)
    from adam_dehaze_amd.engine import invalidate_weight_cache
    invalidate_weight_cache()
    _train_mode(fresh, False)
    assert torch.equal(_routed(fresh, hazy), ema_out), "ema.state_dict(router) in a fresh system is not the applied() model"
    # training goes on
    _train_mode(system)
    before = [s.clone() for s in ema.shadow]
    T.joint_train_step(system, batches[2])
    torch.cuda.synchronize()
    assert ema.updates() == 3
    assert sum(int(not torch.equal(s, b)) for s, b in zip(ema.shadow, before)) >= 0.9 * len(unique)


def test_without_the_section_a_joint_step_is_todays():
    """One joint step with the section absent, and with `ema: null` in the config, launches what the commit before the EMA
    launched: tests/golden/joint_step_launches.json was recorded there, with the recorder of tests/_launch_trace.py made to
    launch and to write a pointer down as null or not (tests/_joint_step_trace.py), so every record pins the entry point, the
    geometry and the scalars of its launch.  With the section present the same records are followed by the two EMA launches
    and by nothing else."""
    from tests import _joint_step_trace as J
    want = J.golden()
    assert want[-1][0] == "adh_adam_multi" and not [n for n, _ in want if n.startswith("adh_ema")]
    for what, section in (("absent", J.ABSENT), ("null", None)):
        system, got = J.record_step(section)
        assert system["ema"] is None, what
        assert J.first_difference(got, want) is None, f"ema section {what}: {J.first_difference(got, want)}"
    system, got = J.record_step({"decay": 0.9})
    assert isinstance(system["ema"], WeightEMA)
    assert J.first_difference(got[:len(want)], want) is None, f"ema section present: {J.first_difference(got[:len(want)], want)}"
    assert [n for n, _ in got[len(want):]] == ["adh_ema_begin", "adh_ema_multi"]


# ------------------------------------------------------------------------------------------------ 8. checkpoints
def _branch_cfg(tmp_path, ema_section):
    from tests.test_gpu_train import _cfg
    cfg = _cfg()
    cfg["dehazing"]["checkpoint_dir"] = str(tmp_path)
    if ema_section is not None:
        cfg["ema"] = ema_section
    return cfg


def _low_batches(n, seed):
    """synthetic batches relabelled 'low', so that every step of the low branch trains and every validation has samples"""
    return [dict(b, intensity=torch.zeros_like(b["intensity"])) for b in T.synthetic_loader(4, 32, n, seed=seed, device=DEV)]


def _ema_lines(text):
    return [int(n) for n in re.findall(r"EMA updates: (\d+)", text)]


def test_branch_checkpoint_round_trip(tmp_path, capsys):
    cfg = _branch_cfg(tmp_path, {"decay": 0.9, "warmup": False})
    train, val = _low_batches(2, 21), _low_batches(1, 22)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        torch.manual_seed(5)
        _, losses = T.train_dehazing_model(cfg, "low", train_loader=train, val_loader=val, epochs=2)
        out = capsys.readouterr().out
        assert len(losses) == 4 and _ema_lines(out) == [2, 4] and "validated on the EMA weights" in out
        path = os.path.join(str(tmp_path), "low", "best_model.pth")
        ck = torch.load(path, map_location="cpu")
        assert {"model_state_dict", "ema_state_dict", "ema_updates"} <= set(ck)
        assert ck["ema_updates"] == 2 * (ck["epoch"] + 1), "one update per step taken"
        raw, shadow = ck["model_state_dict"], ck["ema_state_dict"]
        assert list(raw) == list(shadow)
        differ = [k for k in raw if not torch.equal(raw[k], shadow[k])]
        assert differ and not [k for k in differ if "running" in k or "num_batches" in k], "the buffers are the live model's"
        # resume for one more epoch: the counter goes on
        T.train_dehazing_model(cfg, "low", train_loader=train, val_loader=val, epochs=ck["epoch"] + 2, resume=path)
        out = capsys.readouterr().out
        assert _ema_lines(out) == [ck["ema_updates"] + 2] and "no EMA weights" not in out
        # a checkpoint from before the feature: seeded from the loaded weights, said once
        ck = torch.load(path, map_location="cpu")
        old = {k: v for k, v in ck.items() if not k.startswith("ema_")}
        bare = os.path.join(str(tmp_path), "bare.pth")
        torch.save(old, bare)
        T.train_dehazing_model(cfg, "low", train_loader=train, val_loader=val, epochs=ck["epoch"] + 2, resume=bare)
        out = capsys.readouterr().out
        assert out.count("Checkpoint has no EMA weights: the EMA starts from the loaded weights") == 1 and _ema_lines(out) == [2]
        # which set a loader takes
        ck = torch.load(path, map_location="cpu")
        m_raw, m_ema = T.create_low_intensity_model(cfg), T.create_low_intensity_model(cfg)
        assert T.load_pretrained_model(m_raw, path) and T.load_pretrained_model(m_ema, path, prefer_ema=True)
        out = capsys.readouterr().out
        assert "Loaded pretrained weights from" in out and "Loaded EMA weights from" in out
        k = [k for k in ck["model_state_dict"] if not torch.equal(ck["model_state_dict"][k], ck["ema_state_dict"][k])][0]
        assert torch.equal(m_raw.state_dict()[k], ck["model_state_dict"][k])
        assert torch.equal(m_ema.state_dict()[k], ck["ema_state_dict"][k])


def test_without_the_section_checkpoints_and_report_are_todays(tmp_path, capsys):
    cfg = _branch_cfg(tmp_path, None)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        torch.manual_seed(5)
        T.train_dehazing_model(cfg, "low", train_loader=_low_batches(1, 21), val_loader=_low_batches(1, 22), epochs=1)
    out = capsys.readouterr().out
    assert "EMA" not in out
    ck = torch.load(os.path.join(str(tmp_path), "low", "best_model.pth"), map_location="cpu")
    assert sorted(ck) == sorted(["epoch", "model_state_dict", "optimizer_state_dict", "val_psnr", "val_ssim", "val_loss",
                                 "scheduler_state_dict"])
