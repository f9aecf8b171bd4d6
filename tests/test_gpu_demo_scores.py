"""`main.py --mode demo --input ... --target ...` on the GPU (train.run_demo / image_io.dehaze_files with targets): the routed system
of tests/test_gpu_demo.py, reduced widths and random weights, dehazes PNG files and scores what it wrote against ground-truth
files.  Every score is recomputed here from the written PNG and the target file alone."""
import json
import os
import warnings

import numpy as np
import pytest
import torch

from adam_dehaze_amd import image_io as IO
from adam_dehaze_amd import metrics as M
from adam_dehaze_amd import train as T
from tests import _ref64_ciede as R

pytestmark = pytest.mark.gpu
Image = pytest.importorskip("PIL.Image")
DEV = "cuda:0"
CIEDE_TOL = 5e-6
BASE_KEYS = {"file", "height", "width", "routing", "weights", "intensity"}


def _cfg(routing="soft"):
    return {"dataset": {"batch_size": 4, "img_size": 32},
            "classifier": {"model": "resnet18", "pretrained": False, "num_classes": 3, "checkpoint_dir": "/nonexistent"},
            "dehazing": {"checkpoint_dir": "/nonexistent",
                         "low": {"model_type": "lightweight", "channels": 8, "blocks": 2, "learning_rate": 1e-4},
                         "medium": {"model_type": "standard", "channels": 8, "blocks": 6, "learning_rate": 1e-4},
                         "high": {"model_type": "complex", "channels": 16, "blocks": 9, "learning_rate": 1e-4}},
            "routing": {"type": routing, "temperature": 0.5},
            "joint_training": {"learning_rate": 5e-5, "epochs": 1, "lambda_dehazing": 1.0, "lambda_classification": 0.2,
                               "lambda_detection": 0.5, "checkpoint_dir": "/nonexistent"},
            "device": DEV, "seed": 42}


@pytest.fixture(scope="module")
def soft():
    torch.manual_seed(11)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return T._joint_system_for_evaluation(_cfg())[0]


@pytest.fixture(scope="module")
def folders(tmp_path_factory):
    hazy, clear = tmp_path_factory.mktemp("hazy"), tmp_path_factory.mktemp("clear")
    g = np.random.default_rng(14)
    inputs = {"a.png": g.integers(0, 256, (32, 48, 3), dtype=np.uint8), "b.png": g.integers(0, 256, (32, 48, 3), dtype=np.uint8),
              "c.png": g.integers(0, 256, (31, 45), dtype=np.uint8), "m.png": g.integers(0, 256, (32, 48, 3), dtype=np.uint8),
              "n.png": g.integers(0, 256, (32, 48, 3), dtype=np.uint8)}
    targets = {"a.png": g.integers(0, 256, (32, 48, 3), dtype=np.uint8), "b.bmp": g.integers(0, 256, (32, 48, 3), dtype=np.uint8),
               "c.png": g.integers(0, 256, (31, 45), dtype=np.uint8), "m.png": g.integers(0, 256, (16, 16, 3), dtype=np.uint8)}
    for d, files in ((hazy, inputs), (clear, targets)):
        for name, a in files.items():
            Image.fromarray(a).save(d / name)
    return hazy, clear


@pytest.fixture(scope="module")
def scored_run(folders, soft, tmp_path_factory):
    """train.run_demo with a target directory: (output directory, records, warnings)"""
    hazy, clear = folders
    out = tmp_path_factory.mktemp("demo_scored")
    mp = pytest.MonkeyPatch()
    mp.setattr(T, "_joint_system_for_evaluation", lambda config: (soft, None))
    try:
        with warnings.catch_warnings(record=True) as rec:
            warnings.simplefilter("always")
            results = T.run_demo(_cfg(), str(hazy), str(out), False, target=str(clear))
    finally:
        mp.undo()
    return out, results, [str(w.message) for w in rec]


def _planes(path):
    return IO.u8_to_image(IO.load_image(str(path)).to(DEV))


def _six(img_path, hazy_path, target_path):
    """the six scores from the files alone: PSNR and SSIM by a direct call, CIEDE2000 by the float64 reference"""
    tgt = _planes(target_path)
    out = []
    for p in (img_path, hazy_path):
        x = _planes(p)
        out += [float(M.psnr_batch(x, tgt).double()[0]), float(M.ssim_batch(x, tgt).double()[0]),
                float(R.ciede2000(x.cpu().numpy(), tgt.cpu().numpy())[1][0])]
    return out


def test_every_score_is_recomputed_from_the_written_file(folders, scored_run):
    hazy, clear = folders
    out, results, warned = scored_run
    assert [os.path.basename(r["file"]) for r in results] == ["a.png", "b.png", "c.png", "m.png", "n.png"]
    for name, tname in (("a.png", "a.png"), ("b.png", "b.bmp"), ("c.png", "c.png")):
        r = next(r for r in results if os.path.basename(r["file"]) == name)
        assert set(r) == BASE_KEYS | {"target", "scored"} | set(IO.SCORE_KEYS) and r["scored"] is True
        assert r["target"] == str(clear / tname)
        want = _six(out / name, hazy / name, clear / tname)
        for k, w in zip(IO.SCORE_KEYS, want):
            print(f"{name} {k}: recorded {r[k]!r}, recomputed {w!r}")
            if k.endswith("ciede2000"):
                assert abs(r[k] - w) <= CIEDE_TOL, (name, k)
            else:
                assert r[k] == w, (name, k)                    # the same kernels on the same tensors
        assert 0 < r["ciede2000"] < 128 and r["psnr"] is not None


def test_mismatched_and_missing_targets_are_dehazed_unscored_and_named(folders, scored_run):
    hazy, clear = folders
    out, results, warned = scored_run
    by = {os.path.basename(r["file"]): r for r in results}
    assert by["m.png"] == {**{k: by["m.png"][k] for k in BASE_KEYS}, "target": str(clear / "m.png"), "scored": False,
                           "reason": "size 32x48 != 16x16"}
    assert by["n.png"] == {**{k: by["n.png"][k] for k in BASE_KEYS}, "target": None}
    assert sum("n.png" in w and "no target" in w for w in warned) == 1
    for name in ("m.png", "n.png"):
        with Image.open(out / name) as im:
            assert im.mode == "RGB" and (im.height, im.width) == (32, 48)


def test_demo_scores_json_holds_the_means_of_the_records(scored_run):
    out, results, _ = scored_run
    assert sorted(os.listdir(out)) == ["a.png", "b.png", "c.png", "demo_results.json", "demo_scores.json", "m.png", "n.png"]
    assert json.load(open(out / "demo_results.json")) == results
    scores = json.load(open(out / "demo_scores.json"))
    scored = [r for r in results if r.get("scored")]
    assert len(scored) == 3 and set(scores) == {"dehazed", "hazy"}
    cats = {r["intensity"] + "_intensity" for r in scored} | {"all"}
    for side, prefix in (("dehazed", ""), ("hazy", "hazy_")):
        assert set(scores[side]) == cats
        for cat, entry in scores[side].items():
            rs = [r for r in scored if cat == "all" or r["intensity"] + "_intensity" == cat]
            assert set(entry) == {"psnr", "ssim", "ciede2000", "samples"} and entry["samples"] == len(rs)
            for k in ("psnr", "ssim", "ciede2000"):
                assert abs(entry[k] - sum(r[prefix + k] for r in rs) / len(rs)) <= 1e-12, (side, cat, k)


def test_target_equal_to_input_scores_the_hazy_side_as_identical(folders, soft, tmp_path):
    hazy, _ = folders
    paths = [str(hazy / n) for n in ("a.png", "b.png", "c.png")]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        results = IO.dehaze_files(soft, paths, str(tmp_path), batch_size=4, panels=True,
                                  targets=IO.pair_targets(paths, str(hazy)))
    assert len(results) == 3
    for r in results:
        assert r["scored"] is True and r["target"] == r["file"]
        assert (r["hazy_psnr"], r["hazy_ssim"], r["hazy_ciede2000"]) == (None, 1.0, 0.0), r["file"]
        name = os.path.basename(r["file"])
        want = _six(tmp_path / name, hazy / name, hazy / name)           # the panel run scores the right pane = the written file
        assert r["psnr"] == want[0] and r["ssim"] == want[1] and abs(r["ciede2000"] - want[2]) <= CIEDE_TOL
    summary = IO.summarize_scores(results)
    assert summary["hazy"]["all"] == {"psnr": None, "ssim": 1.0, "ciede2000": 0.0, "samples": 3, "psnr_infinite": 3}
    assert "Infinity" not in json.dumps(results)


def test_single_file_against_single_file(folders, soft, tmp_path):
    hazy, clear = folders
    mp = pytest.MonkeyPatch()
    mp.setattr(T, "_joint_system_for_evaluation", lambda config: (soft, None))
    try:
        results = T.run_demo(_cfg(), str(hazy / "b.png"), str(tmp_path), False, target=str(clear / "b.bmp"))
    finally:
        mp.undo()
    assert len(results) == 1 and results[0]["scored"] is True and results[0]["target"] == str(clear / "b.bmp")
    want = _six(tmp_path / "b.png", hazy / "b.png", clear / "b.bmp")
    assert results[0]["psnr"] == want[0] and abs(results[0]["ciede2000"] - want[2]) <= CIEDE_TOL


def test_without_target_nothing_changes(folders, soft, tmp_path):
    hazy, _ = folders
    mp = pytest.MonkeyPatch()
    mp.setattr(T, "_joint_system_for_evaluation", lambda config: (soft, None))
    try:
        results = T.run_demo(_cfg(), str(hazy), str(tmp_path), False)
    finally:
        mp.undo()
    assert sorted(os.listdir(tmp_path)) == ["a.png", "b.png", "c.png", "demo_results.json", "m.png", "n.png"]
    assert all(set(r) == BASE_KEYS for r in results)
