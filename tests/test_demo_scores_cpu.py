"""Host side of `main.py --mode demo --input ... --target ...` without a GPU: how image_io.pair_targets finds the ground-truth file
of every input, the refusal of --target without --input, what reaches train.run_demo, and the arithmetic of
image_io.summarize_scores, an infinite PSNR included."""
import json
import os
import sys
import warnings

import numpy as np
import pytest
import torch

from adam_dehaze_amd import image_io as IO
from adam_dehaze_amd import train as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Image = pytest.importorskip("PIL.Image")


def _img(path, h, w, seed=0, mode="RGB"):
    shape = (h, w) if mode == "L" else (h, w, 3)
    Image.fromarray(np.random.default_rng(seed).integers(0, 256, shape, dtype=np.uint8)).save(path)
    return str(path)


@pytest.fixture()
def folders(tmp_path):
    hazy, clear = tmp_path / "hazy", tmp_path / "clear"
    hazy.mkdir()
    clear.mkdir()
    inputs = {"a": _img(hazy / "a.jpg", 32, 48, 1), "b": _img(hazy / "b.png", 32, 48, 2), "c": _img(hazy / "c.bmp", 31, 45, 3, "L"),
              "m": _img(hazy / "m.png", 32, 48, 4), "n": _img(hazy / "n.png", 32, 48, 5)}
    targets = {"a": _img(clear / "a.png", 32, 48, 6), "b": _img(clear / "b.JPEG", 32, 48, 7), "c": _img(clear / "c.png", 31, 45, 8),
               "m": _img(clear / "m.png", 16, 16, 9)}
    (clear / "n.txt").write_text("not an image")
    return hazy, clear, inputs, targets


def test_pair_targets_matches_by_base_name_across_extensions(folders):
    hazy, clear, inputs, targets = folders
    with pytest.warns(UserWarning, match="n.png") as rec:
        pairs = IO.pair_targets(inputs.values(), str(clear))
    assert len(rec) == 1                                     # only the input without a target is warned about
    assert set(pairs) == set(inputs.values())
    for k in "abc":
        assert pairs[inputs[k]] == {"target": targets[k]}, k
    assert pairs[inputs["m"]] == {"target": targets["m"], "scored": False, "reason": "size 32x48 != 16x16"}
    assert pairs[inputs["n"]] == {"target": None}
    json.dumps(pairs)


def test_pair_targets_refuses_two_targets_of_one_base_name(folders):
    hazy, clear, inputs, targets = folders
    _img(clear / "a.bmp", 32, 48, 10)
    with pytest.raises(ValueError) as ei:
        IO.pair_targets(inputs.values(), str(clear))
    assert "a.bmp" in str(ei.value) and "a.png" in str(ei.value)


def test_pair_targets_single_file_against_single_file(folders, tmp_path):
    hazy, clear, inputs, targets = folders
    gt = _img(tmp_path / "ground_truth.png", 32, 48, 11)
    assert IO.pair_targets([inputs["a"]], gt) == {inputs["a"]: {"target": gt}}          # whatever its name
    small = _img(tmp_path / "small.png", 16, 20, 12)
    assert IO.pair_targets([inputs["a"]], small) == {inputs["a"]: {"target": small, "scored": False,
                                                                    "reason": "size 32x48 != 16x20"}}
    # one file against several inputs serves the input of its base name
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        pairs = IO.pair_targets([inputs["a"], inputs["b"]], targets["b"])
    assert pairs == {inputs["a"]: {"target": None}, inputs["b"]: {"target": targets["b"]}}
    with pytest.raises(ValueError, match="no such file"):
        IO.pair_targets([inputs["a"]], str(tmp_path / "missing"))


def test_main_refuses_target_without_input(monkeypatch, tmp_path):
    import main as M
    monkeypatch.setattr(T, "run_demo", lambda *a, **k: pytest.fail("must not run"))
    monkeypatch.setattr(T, "build_joint_system", lambda *a, **k: pytest.fail("must not build"))
    monkeypatch.setattr(torch.cuda, "set_device", lambda *a, **k: pytest.fail("must not touch a device"))
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.chdir(ROOT)
    for argv in (["--mode", "demo", "--target", str(tmp_path)], ["--mode", "evaluate", "--target", str(tmp_path)],
                 ["--mode", "evaluate", "--input", str(tmp_path), "--target", str(tmp_path)]):
        monkeypatch.setattr(sys, "argv", ["main.py", "--device", "cpu"] + argv)
        with pytest.raises(SystemExit) as ei:
            M.main()
        assert "--target needs --mode demo --input" in str(ei.value)


def test_main_target_reaches_run_demo_and_its_absence_changes_nothing(monkeypatch, tmp_path):
    import main as M
    calls = []
    monkeypatch.setattr(T, "run_demo", lambda *a, **k: calls.append((a[1:], k)))
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.chdir(ROOT)
    monkeypatch.setattr(sys, "argv", ["main.py", "--mode", "demo", "--input", "hazy", "--target", "clear", "--device", "cpu"])
    M.main()
    monkeypatch.setattr(sys, "argv", ["main.py", "--mode", "demo", "--input", "hazy", "--device", "cpu"])
    M.main()
    assert calls == [(("hazy", "demo", False), {"target": "clear"}), (("hazy", "demo", False), {})]


def _record(name, intensity, scores):
    r = {"file": name, "height": 32, "width": 48, "routing": "soft", "weights": [0.2, 0.5, 0.3], "intensity": intensity}
    if scores is not None:
        r.update(target="t/" + name, scored=True, **dict(zip(IO.SCORE_KEYS, scores)))
    return r


def test_summary_arithmetic_with_an_infinite_psnr():
    recs = [_record("a", "low", (20.0, 0.5, 4.0, 10.0, 0.25, 9.0)),
            _record("b", "low", (None, 1.0, 0.0, None, 1.0, 0.0)),
            _record("c", "high", (30.0, 0.75, 2.0, 12.0, 0.5, 7.0)),
            _record("d", "high", None),
            {**_record("e", "medium", None), "target": "t/e", "scored": False, "reason": "size 32x48 != 16x16"},
            {**_record("f", "medium", None), "target": None}]
    s = IO.summarize_scores(recs)
    assert set(s) == {"dehazed", "hazy"}
    assert set(s["dehazed"]) == set(s["hazy"]) == {"low_intensity", "high_intensity", "all"}
    assert s["dehazed"]["low_intensity"] == {"psnr": 20.0, "ssim": 0.75, "ciede2000": 2.0, "samples": 2, "psnr_infinite": 1}
    assert s["dehazed"]["high_intensity"] == {"psnr": 30.0, "ssim": 0.75, "ciede2000": 2.0, "samples": 1}
    assert s["dehazed"]["all"] == {"psnr": 25.0, "ssim": 0.75, "ciede2000": 2.0, "samples": 3, "psnr_infinite": 1}
    assert s["hazy"]["all"] == {"psnr": 11.0, "ssim": (0.25 + 1.0 + 0.5) / 3, "ciede2000": 16.0 / 3, "samples": 3,
                                "psnr_infinite": 1}
    json.loads(json.dumps(s))
    # every PSNR infinite: the mean is null, not NaN and not Infinity (neither is JSON)
    only = IO.summarize_scores([_record("b", "low", (None, 1.0, 0.0, None, 1.0, 0.0))])
    assert only["dehazed"]["all"] == {"psnr": None, "ssim": 1.0, "ciede2000": 0.0, "samples": 1, "psnr_infinite": 1}
    assert "Infinity" not in json.dumps(only) and "NaN" not in json.dumps(only)
    assert IO.summarize_scores([_record("d", "high", None)]) == {"dehazed": {}, "hazy": {}}


def test_run_demo_pairs_before_building_and_writes_the_scores(folders, tmp_path, monkeypatch, capsys):
    hazy, clear, inputs, targets = folders
    seen = {}

    def fake_files(system, paths, out_dir, batch_size=4, panels=False, targets=None):
        seen.update(targets=targets, built=system)
        os.makedirs(out_dir, exist_ok=True)
        out = []
        for p in paths:
            r = {"file": p, "height": 32, "width": 48, "routing": "soft", "weights": [0.2, 0.5, 0.3], "intensity": "medium",
                 **targets[p]}
            if r["target"] is not None and r.get("scored", True):
                r.update(scored=True, **dict(zip(IO.SCORE_KEYS, (21.0, 0.5, 3.0, None, 1.0, 0.0))))
            out.append(r)
        return out

    order = []
    real_pair = IO.pair_targets
    monkeypatch.setattr(IO, "pair_targets", lambda *a: (order.append("pair"), real_pair(*a))[1])
    monkeypatch.setattr(T, "_joint_system_for_evaluation", lambda config: (order.append("build"), ("the system", None))[1])
    monkeypatch.setattr(IO, "dehaze_files", fake_files)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    out = tmp_path / "out"
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        res = T.run_demo({}, str(hazy), str(out), False, target=str(clear))
    assert order == ["pair", "build"]
    assert seen["targets"][inputs["m"]]["scored"] is False and seen["targets"][inputs["n"]] == {"target": None}
    assert json.load(open(out / "demo_results.json")) == res
    scores = json.load(open(out / "demo_scores.json"))
    assert scores == {"dehazed": {k: {"psnr": 21.0, "ssim": 0.5, "ciede2000": 3.0, "samples": 3}
                                  for k in ("medium_intensity", "all")},
                      "hazy": {k: {"psnr": None, "ssim": 1.0, "ciede2000": 0.0, "samples": 3, "psnr_infinite": 3}
                               for k in ("medium_intensity", "all")}}
    text = capsys.readouterr().out
    assert text.count("    against ") == 3 and "3 of 5 scored against" in text and "size 32x48 != 16x16" in text and "no target" in text and "PSNR 21.00 dB" in text
    # a target that does not exist is refused before the system is built
    order.clear()
    with pytest.raises(SystemExit, match="--target"):
        T.run_demo({}, str(hazy), str(out), False, target=str(tmp_path / "missing"))
    assert order == []
