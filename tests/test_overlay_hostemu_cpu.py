"""csrc/overlay.hip without a GPU: the source file, compiled by the host C++ compiler against tools/host_emu with AddressSanitizer
and UndefinedBehaviorSanitizer (float-cast-overflow included: box coordinates far outside an int reach the kernel), run as a
stand-alone program (tools/host_emu/overlay_main.cpp) on heap blocks of exactly the addressed bytes.  Every case of
tests/_overlay_cases.py: the block after the call equals the numpy reference's byte for byte, which covers the drawn pixels, the
alpha bytes, and the poison in pitch slack, in front of an offset base and in the other pane; a read or write outside the block
is the sanitizer's to report.  The grid cap is set to 2 by -D, so the loops over tile rows and images run."""
import numpy as np
import pytest

from tests import _hostemu as E
from tests import _overlay_cases as K

DRAW = 0


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    d = tmp_path_factory.mktemp("overlay_emu")
    exe = E.build(d, "overlay", "overlay_main.cpp", defines=("OVL_MAX_GRID=2",), sanitize=E.FLOAT_CAST)
    return lambda: E.Script(exe, d)


def _add(s, case, img=None):
    """the call of a case on block `img` (a new one when None); returns (call index, block index)"""
    if img is None:
        img = s.raw(K.block(case)[0], case["off"])
    T, G = K.launch_args(case)
    ro = lambda a, dt: None if a is None else s.vec(np.ascontiguousarray(a, dt), dt)
    bufs = (img, ro(case["first"], np.int32), ro(case["boxes"], np.float32), ro(case["colors"], np.uint8), ro(case["text"], np.int8),
            ro(case["glyphs"], np.uint8))
    ints = (case["rp"], case["ip"], case["N"], case["H"], case["W"], case["C"], len(case["boxes"]), T, G, case["thickness"],
            case["scale"], case["alpha"])
    return s.call(DRAW, ints, bufs), img


def test_every_case_equals_the_reference_and_every_poison_byte_survives(emu):
    s, runs = emu(), []
    for case in K.cases():
        want, covered = K.expected(case)
        runs.append((case["name"], _add(s, case)[1], want, covered))
    assert s.run() == [0] * len(runs)
    total = 0
    for name, img, want, covered in runs:
        got = s.after[img]
        bad = np.nonzero(got != want)[0]
        assert bad.size == 0, f"{name}: {bad.size} bytes differ, first at block offset {bad[:8].tolist()}"
        total += covered
    assert total > 20000, "the table draws too little to mean anything"


def test_an_empty_batch_and_boxes_that_draw_nothing_leave_every_byte(emu):
    s = emu()
    case = next(c for c in K.cases() if c["name"] == "skipped_boxes_draw_nothing")
    before = K.block(case)[0]
    a = _add(s, case)[1]
    b = _add(s, dict(case, first=np.zeros(2, np.int32)))[1]
    # M == 0: a success without a launch, whatever the other pointers are
    c = s.raw(before, case["off"])
    s.call(DRAW, (case["rp"], case["ip"], 1, case["H"], case["W"], 3, 0, 0, 0, 2, 1, 255),
           (c, s.vec(np.zeros(2, np.int32), np.int32), None, None, None, None))
    assert s.run() == [0, 0, 0]
    for k in (a, b, c):
        assert np.array_equal(s.after[k], before)


def test_refusals_write_nothing(emu):
    s = emu()
    base = K._case("valid", [(2.0, 10.0, 14.0, 15.0), (0.0, 0.0, 16.0, 16.0)], text=K._text([[1], [2, 3]]), N=2, H=16, W=16, first=[0, 1, 2])
    before = K.block(base)[0]
    img = s.raw(before, 0)
    ok, _ = _add(s, base, s.raw(before, 0))
    names = ("img", "first", "boxes", "colors", "text", "glyphs")
    bad = []
    for name, ints, nulled in K.REFUSALS:
        T, G = K.launch_args(base)
        v = {"rp": base["rp"], "ip": base["ip"], "N": 2, "H": 16, "W": 16, "C": 3, "M": 2, "T": T, "G": G, "thickness": 2, "scale": 1,
             "alpha": 255, **ints}
        arrays = {"img": img, "first": s.vec(base["first"], np.int32), "boxes": s.vec(base["boxes"], np.float32),
                  "colors": s.vec(base["colors"], np.uint8), "text": s.vec(base["text"], np.int8), "glyphs": s.vec(K.FONT, np.uint8)}
        bad.append(s.call(DRAW, [v[k] for k in ("rp", "ip", "N", "H", "W", "C", "M", "T", "G", "thickness", "scale", "alpha")],
                          [None if k in nulled else arrays[k] for k in names]))
    rcs = s.run()
    assert rcs[ok] == 0
    assert [rcs[k] for k in bad] == [E.ADH_E_ARG] * len(bad), [n for (n, _, _), k in zip(K.REFUSALS, bad) if rcs[k] != E.ADH_E_ARG]
    assert np.array_equal(s.after[img], before)


def test_image_pitch_is_not_looked_at_for_one_image(emu):
    s = emu()
    case = next(c for c in K.cases() if c["name"] == "three_overlapping_alpha128")
    want, _ = K.expected(case)
    k, img = _add(s, dict(case, ip=0))
    assert s.run() == [0]
    assert np.array_equal(s.after[img], want)
