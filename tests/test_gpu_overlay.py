"""adh_draw_boxes (csrc/overlay.hip) on the MI355X: the case table of tests/_overlay_cases.py through the C ABI, and -- its
frames, pitches, box lists and styles, with colours and captions from seeded labels and scores -- through overlay.draw_boxes,
byte for byte against the numpy reference of tests/_overlay_ref.py: the drawn pixels, the alpha bytes, and the poison in pitch
slack, in front of an offset base and in the other pane of a panel; and a second launch on the same input for bit-identical
bytes."""
import numpy as np
import pytest
import torch

from adam_dehaze_amd import _hip as H
from adam_dehaze_amd import overlay as O
from tests import _overlay_cases as K
from tests._overlay_ref import draw_boxes_ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CASES = K.cases()


def _dev(a, dtype):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype)).to(DEV)


def _raw(case, blk, **changed):
    """one launch of the case's arguments on the device block `blk`; the return code"""
    T, G = K.launch_args(case)
    bufs = {"first": _dev(case["first"], np.int32), "boxes": _dev(case["boxes"], np.float32), "colors": _dev(case["colors"], np.uint8),
            "text": _dev(case["text"], np.int8), "glyphs": _dev(case["glyphs"], np.uint8)}
    v = {"img": blk.data_ptr() + case["off"], "rp": case["rp"], "ip": case["ip"], "N": case["N"], "H": case["H"], "W": case["W"],
         "C": case["C"], "M": len(case["boxes"]), "T": T, "G": G, "thickness": case["thickness"], "scale": case["scale"],
         "alpha": case["alpha"], **{k: (None if b is None or b.numel() == 0 else b.data_ptr()) for k, b in bufs.items()}}
    if case["text"] is not None and case["text"].size == 0:                  # T == 0: any pointer will do
        v["text"] = blk.data_ptr()
    if case["glyphs"] is not None and len(case["glyphs"]) == 0:
        v["glyphs"] = blk.data_ptr()
    v.update(changed)
    rc = H.load().adh_draw_boxes(H.stream_ptr(), v["img"], v["rp"], v["ip"], v["N"], v["H"], v["W"], v["C"], v["first"], v["M"],
                                 v["boxes"], v["colors"], v["text"], v["T"], v["glyphs"], v["G"], v["thickness"], v["scale"], v["alpha"])
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_raw_entry_point_equals_the_reference_and_repeats_bit_for_bit(case):
    before, _ = K.block(case)
    want, covered = K.expected(case)
    blk = torch.from_numpy(before).to(DEV)
    assert _raw(case, blk) == 0
    got = blk.cpu().numpy()
    bad = np.nonzero(got != want)[0]
    print(f"{case['name']}: {covered} covered pixels, {bad.size} of {got.size} bytes differ")
    assert bad.size == 0, f"first differing block offsets {bad[:8].tolist()}"
    again = torch.from_numpy(before).to(DEV)
    assert _raw(case, again) == 0
    assert torch.equal(again, blk)


def _dets(case, g):
    """the case's boxes as draw_boxes takes them: labels and scores from a seed, a tie among the scores"""
    out = []
    for n in range(case["N"]):
        lo, hi = (max(0, min(int(case["first"][n + k]), len(case["boxes"]))) for k in (0, 1))
        m = max(hi - lo, 0)
        scores = np.round(g.uniform(0, 1, m), 1)                             # one decimal: ties are certain among many boxes
        out.append({"boxes": torch.from_numpy(case["boxes"][lo:lo + m]).to(DEV), "labels": torch.from_numpy(g.integers(0, 91, m)).to(DEV),
                    "scores": torch.from_numpy(scores).to(DEV)})
    return out


@pytest.mark.parametrize("name", [c["name"] for c in CASES])
def test_draw_boxes_on_views_equals_the_reference(name):
    case = next(c for c in CASES if c["name"] == name)
    g = np.random.default_rng(5)
    dets = _dets(case, g)
    before, idx = K.block(case)
    blk = torch.from_numpy(before).to(DEV)
    N, Hh, W, C = (case[k] for k in "NHWC")
    view = torch.as_strided(blk, (N, Hh, W, C), (case["ip"], case["rp"], C, 1), case["off"])
    style = {"thickness": case["thickness"], "scale": case["scale"], "alpha": case["alpha"]}
    assert O.draw_boxes(view, dets, **style) is view
    torch.cuda.synchronize()
    first, boxes, colors, text = O.pack_detections(dets)
    drawn, covered = draw_boxes_ref(K.pixels(case), first, boxes, colors, text, O.FONT_5X7, **style)
    want = before.copy()
    want[idx] = drawn
    got = blk.cpu().numpy()
    assert np.array_equal(got, want), f"{int((got != want).sum())} bytes differ ({int(covered.sum())} covered pixels)"
    if N == 1:                                                               # [H,W,C] is taken too
        blk3 = torch.from_numpy(before).to(DEV)
        O.draw_boxes(torch.as_strided(blk3, (Hh, W, C), (case["rp"], C, 1), case["off"]), dets, **style)
        assert torch.equal(blk3, blk)


def test_draw_boxes_without_detections_launches_nothing_and_refuses_bad_input():
    u8 = torch.full((2, 16, 16, 3), 7, dtype=torch.uint8, device=DEV)
    empty = {"boxes": torch.zeros((0, 4)), "labels": torch.zeros(0, dtype=torch.int64), "scores": torch.zeros(0)}
    assert O.draw_boxes(u8, [empty, empty]) is u8 and bool((u8 == 7).all())
    one = {"boxes": [[1.0, 1.0, 9.0, 9.0]], "labels": [3], "scores": [0.5]}
    with pytest.raises(ValueError):
        O.draw_boxes(u8, [one])                                              # two images
    with pytest.raises(ValueError):
        O.draw_boxes(torch.zeros((1, 16, 16, 1), dtype=torch.uint8, device=DEV), [one])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        O.draw_boxes(torch.zeros((1, 16, 16, 3), dtype=torch.uint8), [one])
    for bad in ({"thickness": 0}, {"scale": 0}, {"alpha": 256}, {"alpha": -1}):
        with pytest.raises(RuntimeError, match="ADH_E_ARG"):
            O.draw_boxes(u8, [one, empty], **bad)
    assert bool((u8 == 7).all())
    O.draw_boxes(u8, [one, empty])
    torch.cuda.synchronize()
    assert tuple(u8[0, 1, 1].tolist()) == O.class_color(3)[0] and bool((u8[1] == 7).all())


def test_refusals_launch_nothing():
    base = K._case("valid", [(2.0, 10.0, 14.0, 15.0), (0.0, 0.0, 16.0, 16.0)], text=K._text([[1], [2, 3]]), N=2, H=16, W=16, first=[0, 1, 2])
    before = K.block(base)[0]
    blk = torch.from_numpy(before).to(DEV)
    for name, ints, nulled in K.REFUSALS:
        assert _raw(base, blk, **ints, **{k: None for k in nulled}) == -1, name
    assert np.array_equal(blk.cpu().numpy(), before)
    assert _raw(base, blk) == 0 and not np.array_equal(blk.cpu().numpy(), before)
