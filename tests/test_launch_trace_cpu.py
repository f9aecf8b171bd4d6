"""Which kernel a convolution layer gets, with which descriptor, pack size, split count, slab size and statistics-row offsets:
the launch sequence of Engine._run_gather / _wgrad / conv / backward, recorded on the CPU (tests/_launch_trace.py) and
compared with tests/golden/launch_trace.json.  Every other op of the engine -- the BatchNorm sequences, the depthwise,
DenseNet, attention, pooling and pointwise ops, with the host-side writes between their launches -- is compared with
tests/golden/launch_trace_ops.json the same way."""
import json
import re

import pytest

from adam_dehaze_amd import _hip as H
from tests import _launch_trace as LT


@pytest.fixture(scope="module")
def golden():
    with open(LT.GOLDEN_PATH) as f:
        g = json.load(f)
    assert g["conv_desc_fields"] == LT.DESC_FIELDS, "ConvDesc changed: regenerate the golden (tests/_launch_trace.py)"
    return g["cases"]


@pytest.fixture(scope="module")
def ops_golden():
    with open(LT.OPS_GOLDEN_PATH) as f:
        g = json.load(f)
    assert g["conv_desc_fields"] == LT.DESC_FIELDS, "ConvDesc changed: regenerate the golden (tests/_launch_trace.py)"
    return g["cases"]


@pytest.fixture(autouse=True)
def _no_library_ab_variables():
    if LT.library_env_set():
        pytest.skip(f"library-side A/B variables are set ({', '.join(LT.library_env_set())}): the host queries answer differently")


def test_golden_has_exactly_the_cases(golden):
    assert list(golden) == list(LT.CASES)


@pytest.mark.parametrize("name", list(LT.CASES))
def test_launch_sequence_matches_golden(name, golden, monkeypatch):
    got = LT.run_case(name, monkeypatch)
    diff = LT.differences(got, golden[name], name)
    assert not diff, "\n".join(diff)


def test_ops_golden_has_exactly_the_cases(ops_golden):
    assert list(ops_golden) == list(LT.OPS_CASES) and not set(LT.OPS_CASES) & set(LT.CASES)


@pytest.mark.parametrize("name", list(LT.OPS_CASES))
def test_op_launch_sequence_matches_golden(name, ops_golden, monkeypatch):
    got = LT.run_case(name, monkeypatch)
    diff = LT.differences(got, ops_golden[name], name)
    assert not diff, "\n".join(diff)


def test_every_entry_point_the_engine_names_is_in_a_trace(golden, ops_golden):
    """an op cannot be added to engine.py, or drop out of the traces, silently"""
    with open(LT.E.__file__) as f:
        want = set(re.findall(r'H\.call\("(adh_\w+)"', f.read()))
    assert len(want) >= 50
    seen = {r[0] for cases in (golden, ops_golden) for recs in cases.values() for r in recs}
    assert not want - seen, sorted(want - seen)


def test_second_forward_with_pack_cache_records_no_pack_call(monkeypatch):
    names = [r[0] for r in LT.run_case("pack_cache", monkeypatch)]
    fwd = [i for i, n in enumerate(names) if n == "adh_conv_wino43_forward"]
    assert len(fwd) == 2 and names[:fwd[0]] == ["adh_pack_weights_wino43"] and names[fwd[0] + 1:fwd[1]] == []


def test_every_convolution_entry_point_is_in_the_trace(golden):
    """a family cannot drop out of the trace silently"""
    pat = re.compile(r"adh_conv_\w*forward\w*|adh_conv_wino43_dgrad_bnred\w*|adh_conv_wgrad\w*|adh_wgrad_reduce\w*|adh_pack_weights\w*")
    want = {n for n in H._SIGNATURES if pat.fullmatch(n) and n not in H._VALUE_FUNCS}
    assert len(want) >= 30
    seen = {r[0] for recs in golden.values() for r in recs}
    assert not want - seen, sorted(want - seen)


def test_a_family_that_declines_leaves_the_plans_own_taps(monkeypatch):
    """ConvTranspose2d 16 -> 3: F(3x3,2x2) is tried with forward-walking taps and turns the shape down (Cout % 4 != 0), so the
    four class launches of the general kernel must carry the plan's backward-walking taps again, dy0 = py and dx0 = px.  (Not
    part of the golden: the selection code the golden was recorded from restored dx0 from dy0 here.)"""
    monkeypatch.setitem(LT.CASES, "declined", (LT.layer("convT", 4, 2, 1, 16, 3, 1, 8, 8, parts="f", stats=False), {}, {}))
    recs = [r for r in LT.run_case("declined", monkeypatch) if r[0] == "adh_conv_forward"]
    taps = [[r[4][0]["d"][LT.DESC_FIELDS.index(f)] for f in ("dy0", "dx0", "dstep_y", "dstep_x")] for r in recs]
    assert taps == [[py, px, -1, -1] for py in range(2) for px in range(2)]
