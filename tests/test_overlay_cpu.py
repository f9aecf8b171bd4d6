"""The host side of `main.py --mode demo --detect` without a GPU: the numpy reference of the overlay kernel
(tests/_overlay_ref.py) against cases small enough to work out by hand, the colours and captions of overlay.py, the greedy
matching of hazy against dehazed detections, the arithmetic of demo_detections.json, and what train.run_demo passes on."""
import json
import os
import sys

import numpy as np
import pytest

from adam_dehaze_amd import image_io as IO
from adam_dehaze_amd import overlay as O
from adam_dehaze_amd import train as T
from tests._overlay_ref import box_geometry, draw_boxes_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _mask(rows):
    return np.array([[ch == "#" for ch in r] for r in rows])


# ---------------------------------------------------------------------------------------------------------------- the reference
def test_reference_outline_by_hand():
    pix = np.zeros((1, 5, 6, 3), np.uint8)
    out, covered = draw_boxes_ref(pix, [0, 1], [(1.0, 1.0, 5.0, 4.0)], [[(10, 20, 30), (1, 2, 3)]], None, None, thickness=1)
    want = _mask(["......",
                  ".####.",
                  ".#..#.",
                  ".####.",
                  "......"])
    assert np.array_equal(covered[0], want)
    assert (out[0][want] == (10, 20, 30)).all() and (out[0][~want] == 0).all()
    # thickness 2: the box is 3 rows high, narrower than 2 t, and is filled
    out, covered = draw_boxes_ref(pix, [0, 1], [(1.0, 1.0, 5.0, 4.0)], [[(10, 20, 30), (1, 2, 3)]], None, None, thickness=2)
    assert np.array_equal(covered[0], _mask(["......", ".####.", ".####.", ".####.", "......"]))


def test_reference_coordinates_by_hand():
    assert box_geometry((0.5, 0.5, 2.5, 2.5), 4, 4) == (0, 2, 0, 2)          # floor(x1), ceil(x2) - 1
    assert box_geometry((1.0, 1.0, 3.0, 3.0), 4, 4) == (1, 2, 1, 2)          # an exact x2 is exclusive
    assert box_geometry((-7.0, -0.5, 99.0, 3.5), 4, 4) == (0, 3, 0, 3)       # clamped
    assert box_geometry((-9.0, 1.0, -2.0, 2.0), 4, 4) == (0, 0, 1, 1)        # left of the frame: clamped onto column 0
    assert box_geometry((-1e30, 0.0, 1e30, 1.0), 4, 4) == (0, 3, 0, 0)
    for bad in ((1.0, 1.0, 1.0, 2.0), (2.0, 1.0, 1.0, 2.0), (1.0, 2.0, 2.0, 1.0), (float("nan"), 1.0, 2.0, 2.0),
                (1.0, 1.0, float("inf"), 2.0), (float("-inf"), 1.0, 2.0, 2.0)):
        assert box_geometry(bad, 4, 4) is None, bad


def test_reference_blend_by_hand():
    pix = np.full((1, 3, 3, 4), 200, np.uint8)
    pix[..., 3] = 77
    out, _ = draw_boxes_ref(pix, [0, 1], [(0.0, 0.0, 3.0, 3.0)], [[(10, 255, 0), (0, 0, 0)]], None, None, thickness=1, alpha=128)
    # (128 c + 127 * 200 + 127) / 255 in integers: c = 10 -> 26807 / 255 = 105; c = 255 -> 58167 / 255 = 228; c = 0 -> 25527 / 255 = 100
    assert out[0, 0, 0].tolist() == [105, 228, 100, 77] and out[0, 1, 1].tolist() == [200, 200, 200, 77]
    out0, _ = draw_boxes_ref(pix, [0, 1], [(0.0, 0.0, 3.0, 3.0)], [[(10, 255, 0), (0, 0, 0)]], None, None, thickness=1, alpha=0)
    assert np.array_equal(out0, pix)


def test_reference_tag_and_glyph_by_hand():
    pix = np.zeros((1, 12, 10, 3), np.uint8)
    box, ink = (9, 9, 9), (250, 250, 250)
    out, covered = draw_boxes_ref(pix, [0, 1], [(1.0, 9.0, 9.0, 12.0)], [[box, ink]], [[1, -1]], O.FONT_5X7, thickness=2, scale=1)
    # y_lo = 9 = 9 scale: the tag sits above, rows 0..8; one character: columns 1 .. 1 + 7 - 1.  The glyph's cell starts one
    # pixel in from the tag's corner: the '1' of FONT_5X7 is ..#.. / .##.. / ..#.. x 4 / .###.
    glyph = _mask(["..........",
                   "....#.....",
                   "...##.....",
                   "....#.....",
                   "....#.....",
                   "....#.....",
                   "....#.....",
                   "...###....",
                   "..........",
                   "..........",
                   "..........",
                   ".........."])
    tag = np.zeros((12, 10), bool)
    tag[0:9, 1:8] = True
    filled = np.zeros((12, 10), bool)
    filled[9:12, 1:9] = True                                                 # three rows: narrower than 2 t
    assert np.array_equal(covered[0], tag | filled)
    assert (out[0][glyph] == ink).all() and (out[0][(tag & ~glyph) | filled] == box).all() and (out[0][~(tag | filled)] == 0).all()
    # scale 2 doubles every dot; y_lo = 9 < 18 forces the tag inside, rows 9..11 (cut at the frame), over the outline
    out2, covered2 = draw_boxes_ref(pix, [0, 1], [(1.0, 9.0, 9.0, 12.0)], [[box, ink]], [[1, -1]], O.FONT_5X7, thickness=2, scale=2)
    assert np.array_equal(covered2[0], filled | _mask(["." * 10] * 9 + [".#########"] * 3))
    want_ink = np.zeros((12, 10), bool)
    want_ink[11, 7:9] = True                 # v = (11 - 9 - 2) / 2 = 0: the top row of '1', ..#.., dot 2 -> columns 1 + 2 + 4 .. + 1
    assert np.array_equal((out2[0] == ink).all(axis=2), want_ink)


def test_reference_first_box_in_list_order_wins():
    pix = np.zeros((1, 6, 6, 3), np.uint8)
    cols = [[(1, 1, 1), (0, 0, 0)], [(2, 2, 2), (0, 0, 0)]]
    out, _ = draw_boxes_ref(pix, [0, 2], [(0.0, 0.0, 4.0, 4.0), (2.0, 2.0, 6.0, 6.0)], cols, None, None, thickness=1)
    # [y, x]: (3, 3) and (2, 3) lie on the first box's right edge; (2, 2) is inside it, on the second's corner
    assert out[0, 3, 3, 0] == 1 and out[0, 2, 3, 0] == 1 and out[0, 2, 2, 0] == 2 and out[0, 5, 5, 0] == 2 and out[0, 1, 1, 0] == 0
    out, _ = draw_boxes_ref(pix, [0, 2], [(2.0, 2.0, 6.0, 6.0), (0.0, 0.0, 4.0, 4.0)], cols[::-1], None, None, thickness=1)
    # now (2, 3) and (3, 2) are the 2 x 2 .. 5 x 5 box's top and left edge; (3, 3) is inside it, on the other's corner
    assert out[0, 3, 3, 0] == 1 and out[0, 2, 3, 0] == 2 and out[0, 3, 2, 0] == 2 and out[0, 2, 2, 0] == 2 and out[0, 0, 0, 0] == 1


# ---------------------------------------------------------------------------------------------------------------- overlay.py
def test_font_table():
    assert len(O.FONT_5X7) == len(O.FONT_CHARS) == 13 and O.FONT_CHARS == "0123456789.:%"
    assert all(len(g) == 7 and all(0 <= r < 32 for r in g) for g in O.FONT_5X7)
    assert len(set(O.FONT_5X7)) == 13 and all(any(g) for g in O.FONT_5X7)


def test_class_color_known_values():
    # hue 0: (v, v (1 - s), v (1 - s)) = (0.95, 0.1425, 0.1425) -> (242, 36, 36), luma 97.6: white text
    assert O.class_color(0) == ((242, 36, 36), (255, 255, 255))
    # hue 0.618...: sector 3, (p, q, v) with f = 0.708: q = 0.95 (1 - 0.85 * 0.708204) = 0.378 -> 96
    assert O.class_color(1) == ((36, 96, 242), (255, 255, 255))
    # hue 0.236...: sector 1, (q, v, p), q = 0.6138 -> 157; luma 193.1: black text
    assert O.class_color(2) == ((157, 242, 36), (0, 0, 0))
    assert O.class_color(17) == ((36, 234, 242), (0, 0, 0))
    assert len({O.class_color(i)[0] for i in range(91)}) == 91


def test_caption_and_its_glyph_indices():
    assert O.caption(3, 0.987) == "3:0.99" and O.caption(17, 0.5) == "17:0.50" and O.caption(90, 1.0) == "90:1.00"
    assert O.encode_caption("17:0.50") == [1, 7, 11, 0, 10, 5, 0]
    assert O.encode_caption("a1%") == [13, 1, 12]                            # no such glyph: an index the kernel leaves blank


def test_pack_detections_sorts_by_score_and_keeps_ties():
    dets = [{"boxes": [[0, 0, 1, 1], [1, 1, 2, 2], [2, 2, 3, 3], [3, 3, 4, 4]], "labels": [5, 6, 7, 8], "scores": [0.2, 0.9, 0.2, 0.5]},
            {"boxes": np.zeros((0, 4)), "labels": [], "scores": []},
            {"boxes": [[9, 9, 10, 10]], "labels": [17], "scores": [0.125]}]
    first, boxes, colors, text = O.pack_detections(dets)
    assert first.tolist() == [0, 4, 4, 5] and first.dtype == np.int32
    assert boxes[:, 0].tolist() == [1, 3, 0, 2, 9] and boxes.dtype == np.float32
    assert colors.shape == (5, 2, 3) and tuple(colors[0, 0]) == O.class_color(6)[0] and tuple(colors[4, 1]) == O.class_color(17)[1]
    assert text.dtype == np.int8 and text.shape == (5, 7)
    assert text[0].tolist() == O.encode_caption("6:0.90") + [-1] and text[4].tolist() == O.encode_caption("17:0.12")
    with pytest.raises(ValueError):
        O.pack_detections([{"boxes": [[0, 0, 1, 1]], "labels": [1, 2], "scores": [0.5]}])


def _item(label, score, x, y, w, h):
    return {"label": label, "score": score, "box": [x, y, w, h]}


def test_items_to_dets_adds_in_float32():
    d = O.items_to_dets([_item(3, 0.5, 0.1, 0.2, 16777216.0, 1.0)])
    assert d["boxes"].dtype == np.float32
    assert d["boxes"][0].tolist() == [np.float32(0.1), np.float32(0.2), np.float32(0.1) + np.float32(16777216.0),
                                      np.float32(0.2) + np.float32(1.0)]
    assert O.items_to_dets([])["boxes"].shape == (0, 4)


def test_match_detections_known_answer():
    a = [_item(1, 0.9, 0, 0, 10, 10),        # a0
         _item(1, 0.8, 20, 0, 10, 10),       # a1
         _item(2, 0.7, 0, 0, 10, 10),        # a2: another label at a0's place
         _item(1, 0.6, 100, 100, 10, 10)]    # a3: nothing near it
    b = [_item(1, 0.5, 1, 0, 10, 10),        # b0: IoU 90 / 110 with a0 -- but b2 scores higher and goes first
         _item(1, 0.4, 24, 0, 10, 10),       # b1: IoU 60 / 140 = 0.43 with a1: below 0.5
         _item(1, 0.95, 0, 1, 10, 10),       # b2: IoU 90 / 110 with a0: takes it
         _item(2, 0.3, 0, 0, 10, 10),        # b3: a2 exactly
         _item(3, 0.99, 0, 0, 10, 10)]       # b4: no such label in a
    assert O.match_detections(a, b) == {"matched": 2, "gained": 3, "lost": 2}
    # b0 is left with nothing (a0 is taken); at IoU 0.4, b1 finds a1
    assert O.match_detections(a, b, iou=0.4) == {"matched": 3, "gained": 2, "lost": 1}
    assert O.match_detections([], b) == {"matched": 0, "gained": 5, "lost": 0}
    assert O.match_detections(a, []) == {"matched": 0, "gained": 0, "lost": 4}
    # the highest IoU wins, not the first candidate; an IoU of exactly the threshold counts
    # (taking the first candidate, 0.43, would leave the second detection with 50 / 150 = 0.33 and one match)
    a2 = [_item(1, 0.5, 4, 0, 10, 10), _item(1, 0.5, 1, 0, 10, 10)]
    assert O.match_detections(a2, [_item(1, 0.9, 0, 0, 10, 10), _item(1, 0.8, 6, 0, 10, 10)], iou=0.4) == \
        {"matched": 2, "gained": 0, "lost": 0}
    assert O.match_detections([_item(1, 0.5, 0, 0, 10, 10)], [_item(1, 0.5, 0, 0, 10, 20)], iou=0.5) == \
        {"matched": 1, "gained": 0, "lost": 0}                               # 100 / 200


def _record(name, intensity, hazy, dehazed, match):
    return {"file": name, "intensity": intensity, "detect_counts": {"hazy": hazy, "dehazed": dehazed},
            "detect_match": dict(zip(("matched", "gained", "lost"), match))}


def test_summary_arithmetic():
    recs = [_record("a", "low", 2, 3, (2, 1, 0)), _record("b", "low", 0, 2, (0, 2, 0)), _record("c", "high", 5, 1, (1, 0, 4)),
            {"file": "d", "intensity": "medium"}]                            # a record without detections is not counted
    s = O.summarize_detections(recs, 0.25, {"detector_checkpoint": "x/best_model.pth", "detector_random_init": False})
    assert s["score_threshold"] == 0.25 and s["detector_checkpoint"] == "x/best_model.pth" and s["detector_random_init"] is False
    assert s["by_intensity"] == {"high": {"files": 1, "mean_hazy": 5.0, "mean_dehazed": 1.0, "matched": 1, "gained": 0, "lost": 4},
                                 "low": {"files": 2, "mean_hazy": 1.0, "mean_dehazed": 2.5, "matched": 2, "gained": 3, "lost": 0}}
    assert s["all"] == {"files": 3, "mean_hazy": 7 / 3, "mean_dehazed": 2.0, "matched": 3, "gained": 3, "lost": 4}
    json.dumps(s)
    e = O.summarize_detections([], 0.5)
    assert e["all"] == {"files": 0, "mean_hazy": None, "mean_dehazed": None, "matched": 0, "gained": 0, "lost": 0}
    assert e["by_intensity"] == {} and e["detector_checkpoint"] is None


# ---------------------------------------------------------------------------------------------------------------- run_demo
def _fake_demo(monkeypatch, tmp_path, seen):
    Image = pytest.importorskip("PIL.Image")
    Image.fromarray(np.zeros((16, 16, 3), np.uint8)).save(tmp_path / "a.png")

    def fake_files(system, paths, out_dir, batch_size=4, panels=False, **kw):
        seen.append(kw)
        os.makedirs(out_dir, exist_ok=True)
        rec = {"file": paths[0], "height": 16, "width": 16, "routing": "soft", "weights": [0.2, 0.5, 0.3], "intensity": "medium"}
        if "detector" in kw:
            rec.update(detections={"hazy": [_item(1, 0.9, 0, 0, 4, 4)], "dehazed": []}, detect_counts={"hazy": 1, "dehazed": 0},
                       detect_match={"matched": 0, "gained": 0, "lost": 1})
        return [rec]

    monkeypatch.setattr(IO, "dehaze_files", fake_files)
    monkeypatch.setattr(T, "_joint_system_for_evaluation", lambda config: ({"device": "cpu"}, None))
    monkeypatch.delenv("WORLD_SIZE", raising=False)


def test_run_demo_passes_nothing_new_without_detect(monkeypatch, tmp_path):
    seen = []
    _fake_demo(monkeypatch, tmp_path, seen)
    monkeypatch.setattr(T, "_detector_for_evaluation", lambda *a, **k: pytest.fail("no detector may be built"))
    T.run_demo({}, str(tmp_path / "a.png"), str(tmp_path / "out"), False)
    T.run_demo({"demo": {"detect": False, "detect_threshold": 0.3, "detect_style": {"alpha": 9}, "detector": {"min_size": 160}}},
               str(tmp_path / "a.png"), str(tmp_path / "out"), False)
    assert seen == [{}, {}]
    assert sorted(os.listdir(tmp_path / "out")) == ["demo_results.json"]


def test_run_demo_builds_the_detector_and_writes_the_summary(monkeypatch, tmp_path, capsys):
    seen, built = [], []
    _fake_demo(monkeypatch, tmp_path, seen)

    def fake_detector(config, dev, **kw):
        built.append((dev, kw))
        return "the detector", {"detector_checkpoint": None, "detector_random_init": True}

    monkeypatch.setattr(T, "_detector_for_evaluation", fake_detector)
    out = tmp_path / "out"
    T.run_demo({}, str(tmp_path / "a.png"), str(out), False, detect=True)
    assert seen[-1] == {"detector": "the detector", "detect_threshold": 0.5} and built[-1] == ("cpu", {})
    cfg = {"demo": {"detect": True, "detect_threshold": 0.25, "detect_style": {"thickness": 3, "alpha": 128},
                    "detector": {"min_size": 160, "max_size": 256}}}
    T.run_demo(cfg, str(tmp_path / "a.png"), str(out), False)
    assert seen[-1] == {"detector": "the detector", "detect_threshold": 0.25, "detect_style": {"thickness": 3, "alpha": 128}}
    assert built[-1] == ("cpu", {"min_size": 160, "max_size": 256})
    T.run_demo(cfg, str(tmp_path / "a.png"), str(out), False, detect_threshold=0.75)      # the argument wins over the config
    assert seen[-1]["detect_threshold"] == 0.75
    s = json.load(open(out / "demo_detections.json"))
    assert s["score_threshold"] == 0.75 and s["detector_random_init"] is True and s["detector_checkpoint"] is None
    assert s["all"] == {"files": 1, "mean_hazy": 1.0, "mean_dehazed": 0.0, "matched": 0, "gained": 0, "lost": 1}
    assert s["by_intensity"] == {"medium": s["all"]}
    lines = [ln for ln in capsys.readouterr().out.splitlines() if "hazy 1, dehazed 0" in ln]
    assert len(lines) == 3 and "lost 1" in lines[0]                          # one line per file and run


@pytest.mark.parametrize("bad", [-0.1, 1.5, float("nan")])
def test_run_demo_refuses_a_threshold_outside_the_unit_interval(monkeypatch, tmp_path, bad):
    seen = []
    _fake_demo(monkeypatch, tmp_path, seen)
    monkeypatch.setattr(T, "_joint_system_for_evaluation", lambda config: pytest.fail("nothing may be built"))
    monkeypatch.setattr(T, "_detector_for_evaluation", lambda *a, **k: pytest.fail("nothing may be built"))
    with pytest.raises(SystemExit, match="threshold"):
        T.run_demo({}, str(tmp_path / "a.png"), str(tmp_path / "out"), False, detect=True, detect_threshold=bad)
    with pytest.raises(SystemExit, match="threshold"):
        T.run_demo({"demo": {"detect": True, "detect_threshold": bad}}, str(tmp_path / "a.png"), str(tmp_path / "out"), False)
    with pytest.raises(SystemExit, match="--detect"):                        # a threshold without detection
        T.run_demo({}, str(tmp_path / "a.png"), str(tmp_path / "out"), False, detect_threshold=0.5)
    assert seen == []


def test_main_detect_flags_reach_run_demo(monkeypatch, tmp_path):
    import main as M
    calls = []
    monkeypatch.setattr(T, "run_demo", lambda config, inp, out, panels, **kw: calls.append(kw))
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.chdir(ROOT)
    base = ["main.py", "--mode", "demo", "--input", "pics", "--device", "cpu"]
    for extra in ([], ["--detect"], ["--detect", "--detect-threshold", "0.3"]):
        monkeypatch.setattr(sys, "argv", base + extra)
        M.main()
    assert calls == [{}, {"detect": True}, {"detect": True, "detect_threshold": 0.3}]
    monkeypatch.setattr(sys, "argv", ["main.py", "--mode", "evaluate", "--detect"])
    with pytest.raises(SystemExit, match="--detect"):
        M.main()
