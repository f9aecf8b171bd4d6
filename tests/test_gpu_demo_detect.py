"""`main.py --mode demo --input ... --detect` on the GPU (train.run_demo / image_io.dehaze_files): the reduced-width routed system
of tests/test_gpu_demo.py and the seeded random-weight detector setting of tests/test_gpu_detection.py (which yields detections
from noise) on 96 x 128 PNGs.  Recorded detections against the detector run directly on the files, the annotated panel against
the numpy reference of the overlay kernel, and the unannotated outputs against a run without detection."""
import json
import os
import warnings

import numpy as np
import pytest
import torch

from adam_dehaze_amd import detection as D
from adam_dehaze_amd import image_io as IO
from adam_dehaze_amd import overlay as O
from adam_dehaze_amd import train as T
from tests._overlay_ref import draw_boxes_ref

pytestmark = pytest.mark.gpu
Image = pytest.importorskip("PIL.Image")
DEV = "cuda:0"
KW = dict(min_size=160, max_size=256, rpn_pre_nms_top_n=200, rpn_post_nms_top_n=60, box_score_thresh=0.012)
THRESHOLD = 0.0125                           # just above box_score_thresh
DETECTOR_SEED = 1
STYLE = {"thickness": 1, "scale": 1, "alpha": 160}


def _cfg():
    return {"dataset": {"batch_size": 4, "img_size": 32},
            "classifier": {"model": "resnet18", "pretrained": False, "num_classes": 3, "checkpoint_dir": "/nonexistent"},
            "dehazing": {"checkpoint_dir": "/nonexistent",
                         "low": {"model_type": "lightweight", "channels": 8, "blocks": 2, "learning_rate": 1e-4},
                         "medium": {"model_type": "standard", "channels": 8, "blocks": 6, "learning_rate": 1e-4},
                         "high": {"model_type": "complex", "channels": 16, "blocks": 9, "learning_rate": 1e-4}},
            "routing": {"type": "soft", "temperature": 0.5},
            "joint_training": {"learning_rate": 5e-5, "epochs": 1, "lambda_dehazing": 1.0, "lambda_classification": 0.2,
                               "lambda_detection": 0.5, "checkpoint_dir": "/nonexistent"},
            "detection": {"model": "faster_rcnn_resnet50_fpn", "pretrained": False, "checkpoint_dir": "/nonexistent"},
            "demo": {"batch_size": 1, "detect_threshold": THRESHOLD, "detect_style": STYLE, "detector": KW},
            "device": DEV, "seed": 42}


@pytest.fixture(scope="module")
def system():
    torch.manual_seed(11)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return T._joint_system_for_evaluation(_cfg())[0]


@pytest.fixture(scope="module")
def detector():
    """tests/test_gpu_detection.py's seeded model: random weights, statistics and scales spread so that scores differ"""
    torch.manual_seed(DETECTOR_SEED)
    m = D.DetectionModel(num_classes=91, pretrained=False, **KW)
    g = torch.Generator().manual_seed(DETECTOR_SEED + 1)
    with torch.no_grad():
        for name, buf in m.named_buffers():
            if name.endswith(("running_var", ".weight")) and buf.dim() == 1:
                buf.copy_(0.5 + torch.rand(buf.shape, generator=g))
            elif buf.dim() == 1:
                buf.copy_(0.1 * torch.randn(buf.shape, generator=g))
        m.model.roi_heads.box_predictor.cls_score.weight.mul_(30.0)
        m.model.roi_heads.box_predictor.bbox_pred.weight.mul_(5.0)
        m.model.rpn.head.bbox_pred.weight.mul_(3.0)
    return m.to(DEV).eval()


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    d = tmp_path_factory.mktemp("detect_in")
    g = np.random.default_rng(12)
    arrays = {"a.png": g.integers(0, 256, (96, 128, 3), dtype=np.uint8), "b.png": g.integers(0, 256, (96, 128, 3), dtype=np.uint8),
              "c.png": g.integers(0, 256, (96, 128), dtype=np.uint8)}
    for name, a in arrays.items():
        Image.fromarray(a).save(d / name)
    return d, arrays


def _run(system, detector, inp, out, panels=False, **kw):
    """train.run_demo with the module's system and detector in place of the ones it would build: (records, the detector keywords)"""
    mp = pytest.MonkeyPatch()
    built = []
    mp.setattr(T, "_joint_system_for_evaluation", lambda config: (system, None))

    def fake(config, dev, **k):
        built.append((str(dev), k))
        return detector, {"detector_checkpoint": None, "detector_random_init": True}
    mp.setattr(T, "_detector_for_evaluation", fake)
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            return T.run_demo(_cfg(), str(inp), str(out), panels, **kw), built
    finally:
        mp.undo()


@pytest.fixture(scope="module")
def plain(system, detector, inputs, tmp_path_factory):
    out = tmp_path_factory.mktemp("detect_off")
    return out, _run(system, detector, inputs[0], out, True)[0]


@pytest.fixture(scope="module")
def detected(system, detector, inputs, tmp_path_factory):
    out = tmp_path_factory.mktemp("detect_on")
    records, built = _run(system, detector, inputs[0], out, True, detect=True)
    return out, records, built


def _items(det):
    return [{"label": int(l), "score": float(s), "box": [float(v) for v in b]}
            for b, l, s in zip(det["boxes_xywh"].tolist(), det["labels"].tolist(), det["scores"].tolist())]


def _xyxy(items):
    b = np.asarray([it["box"] for it in items], np.float32).reshape(-1, 4)
    return np.stack([b[:, 0], b[:, 1], b[:, 0] + b[:, 2], b[:, 1] + b[:, 3]], axis=1)       # float32 sums of the recorded numbers


def test_records_are_the_detector_run_directly_on_the_files(detector, inputs, detected):
    out, records, built = detected
    assert built == [(DEV, KW)]
    assert [os.path.basename(r["file"]) for r in records] == ["a.png", "b.png", "c.png"]
    total = {"hazy": 0, "dehazed": 0}
    for r in records:
        name = os.path.basename(r["file"])
        assert set(r) == {"file", "height", "width", "routing", "weights", "intensity", "detections", "detect_counts", "detect_match"}
        for side, path in (("hazy", inputs[0] / name), ("dehazed", out / name)):
            with torch.no_grad():
                direct = D.filter_detections(detector(IO.u8_to_image(IO.load_image(str(path)).to(DEV))), THRESHOLD)
            assert r["detections"][side] == _items(direct[0]), (name, side)
            assert r["detect_counts"][side] == len(r["detections"][side])
            assert all(it["score"] > THRESHOLD for it in r["detections"][side])
            total[side] += r["detect_counts"][side]
        assert r["detect_match"] == O.match_detections(r["detections"]["hazy"], r["detections"]["dehazed"])
        m = r["detect_match"]
        assert m["matched"] + m["lost"] == r["detect_counts"]["hazy"] and m["matched"] + m["gained"] == r["detect_counts"]["dehazed"]
    print("detections in total:", total)
    assert total["hazy"] > 0 and total["dehazed"] > 0, "the seeded weights must produce detections for this test to mean anything"


def test_detect_png_is_the_reference_drawing_of_the_recorded_detections(inputs, detected):
    out, records, _ = detected
    covered_total = 0
    for r in records:
        name = os.path.basename(r["file"])
        src = inputs[1][name]
        hazy = src if src.ndim == 3 else np.repeat(src[:, :, None], 3, axis=2)
        panes = []
        for side, pix in (("hazy", hazy), ("dehazed", IO.load_image(str(out / name)).numpy())):
            items = r["detections"][side]
            first, boxes, colors, text = O.pack_detections([{"boxes": _xyxy(items), "labels": [it["label"] for it in items],
                                                             "scores": [it["score"] for it in items]}])
            drawn, covered = draw_boxes_ref(pix[None], first, boxes, colors, text, O.FONT_5X7, **STYLE)
            covered_total += int(covered.sum())
            panes.append(drawn[0])
        got = IO.load_image(str(out / (name[:-4] + "_detect.png"))).numpy()
        assert got.shape == (96, 256, 3)
        assert np.array_equal(got, np.concatenate(panes, axis=1)), name
    assert covered_total > 0


def test_plain_outputs_are_untouched_and_the_listing_is_the_old_one_plus_the_new(plain, detected):
    off, on = plain[0], detected[0]
    old = sorted(os.listdir(off))
    assert old == sorted([n + s for n in "abc" for s in (".png", "_panel.png")] + ["demo_results.json"])
    assert sorted(os.listdir(on)) == sorted(old + [n + "_detect.png" for n in "abc"] + ["demo_detections.json"])
    for f in old:
        if f.endswith(".png"):
            assert open(off / f, "rb").read() == open(on / f, "rb").read(), f
    keep = ("file", "height", "width", "routing", "weights", "intensity")
    assert [{k: r[k] for k in keep} for r in detected[1]] == plain[1]
    assert json.load(open(on / "demo_results.json")) == detected[1]


def test_summary_file_agrees_with_the_records(detected):
    out, records, _ = detected
    s = json.load(open(out / "demo_detections.json"))
    assert s["score_threshold"] == THRESHOLD and s["detector_checkpoint"] is None and s["detector_random_init"] is True
    assert s == json.loads(json.dumps(O.summarize_detections(records, THRESHOLD, {"detector_checkpoint": None, "detector_random_init": True})))
    assert s["all"]["files"] == 3
    assert s["all"]["mean_hazy"] == sum(r["detect_counts"]["hazy"] for r in records) / 3
    assert s["all"]["mean_dehazed"] == sum(r["detect_counts"]["dehazed"] for r in records) / 3
    for k in ("matched", "gained", "lost"):
        assert s["all"][k] == sum(r["detect_match"][k] for r in records) == sum(e[k] for e in s["by_intensity"].values())
    assert sum(e["files"] for e in s["by_intensity"].values()) == 3 and set(s["by_intensity"]) == {r["intensity"] for r in records}


def test_exif_target_and_detect_in_one_run(system, detector, inputs, tmp_path):
    """a file stored rotated (EXIF orientation 6) with an upright ground truth: detection sees the upright input and the final
    output, the scores are those of the run without detection, and the panel is 2 x the upright width"""
    src, clear = tmp_path / "in", tmp_path / "clear"
    os.makedirs(src), os.makedirs(clear)
    g = np.random.default_rng(13)
    stored = g.integers(0, 256, (128, 96, 3), dtype=np.uint8)                # upright: 96 x 128
    im = Image.fromarray(stored)
    ex = im.getexif()
    ex[IO.ORIENTATION_TAG] = 6
    im.save(src / "r.png", exif=ex)
    Image.fromarray(g.integers(0, 256, (96, 128, 3), dtype=np.uint8)).save(clear / "r.png")
    a, _ = _run(system, detector, src, tmp_path / "off", False, exif=True, target=str(clear))
    b, _ = _run(system, detector, src, tmp_path / "on", False, exif=True, target=str(clear), detect=True)
    assert sorted(os.listdir(tmp_path / "on")) == ["demo_detections.json", "demo_results.json", "demo_scores.json", "r.png", "r_detect.png"]
    assert open(tmp_path / "off" / "r.png", "rb").read() == open(tmp_path / "on" / "r.png", "rb").read()
    new = {"detections", "detect_counts", "detect_match"}
    assert set(b[0]) == set(a[0]) | new and {k: v for k, v in b[0].items() if k not in new} == a[0]
    assert b[0]["scored"] is True and (b[0]["height"], b[0]["width"], b[0]["orientation"]) == (96, 128, 6)
    upright = torch.rot90(torch.from_numpy(stored), -1, (0, 1)).contiguous()  # orientation 6: rotate 90 degrees clockwise to view
    with torch.no_grad():
        direct = {"hazy": D.filter_detections(detector(IO.u8_to_image(upright.to(DEV))), THRESHOLD),
                  "dehazed": D.filter_detections(detector(IO.u8_to_image(IO.load_image(str(tmp_path / "on" / "r.png")).to(DEV))), THRESHOLD)}
    for side in ("hazy", "dehazed"):
        assert b[0]["detections"][side] == _items(direct[side][0]), side
    panel = IO.load_image(str(tmp_path / "on" / "r_detect.png")).numpy()
    assert panel.shape == (96, 256, 3)
    panes = []
    for side, pix in (("hazy", upright.numpy()), ("dehazed", IO.load_image(str(tmp_path / "on" / "r.png")).numpy())):
        items = b[0]["detections"][side]
        first, boxes, colors, text = O.pack_detections([{"boxes": _xyxy(items), "labels": [it["label"] for it in items],
                                                         "scores": [it["score"] for it in items]}])
        panes.append(draw_boxes_ref(pix[None], first, boxes, colors, text, O.FONT_5X7, **STYLE)[0][0])
    assert np.array_equal(panel, np.concatenate(panes, axis=1))
