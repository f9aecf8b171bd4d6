"""Host-side checks of the stand-alone classifier stage: `main.py --mode train_classifier` dispatch, the reference's import
path, the report / confusion arithmetic, and the DenseNet training entry points of the C ABI.  No GPU needed."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

from adam_dehaze_amd import _hip as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ABI = ("adh_bn_slice_stats_num_blocks", "adh_bn_slice_stats", "adh_bn_slice_moments", "adh_bn_fold_moments",
           "adh_avgpool2_bwd", "adh_bn_preact_bwd_accum")


def test_densenet_abi_in_header_signatures_and_library():
    header = open(os.path.join(ROOT, "include", "adam_dehaze_hip.h")).read()
    declared = set(re.findall(r"^int\s+(adh_\w+)\s*\(", header, flags=re.M))
    lib = ctypes.CDLL(H.lib_path())
    for name in NEW_ABI:
        assert name in declared, name
        assert name in H._SIGNATURES, name
        assert hasattr(lib, name), name
    assert "adh_bn_slice_stats_num_blocks" in H._VALUE_FUNCS


def test_reference_import_path():
    from training.train_classifier import evaluate_classifier, train_classifier
    from adam_dehaze_amd import train as T
    assert train_classifier is T.train_classifier and evaluate_classifier is T.evaluate_classifier


def _run_main(monkeypatch, argv, env=None):
    import main as M
    monkeypatch.setattr(sys, "argv", ["main.py"] + argv)
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    monkeypatch.chdir(ROOT)
    M.main()


def test_main_train_classifier_trains_then_evaluates(monkeypatch):
    import training.train_classifier as TC
    calls = []
    sentinel = object()

    def fake_train(config, epochs=None, **kw):
        calls.append(("train", config["classifier"]["model"], epochs))
        return sentinel

    def fake_eval(model, config, **kw):
        calls.append(("evaluate", model is sentinel))
        return {"accuracy": 0.0, "confusion_matrix": np.zeros((3, 3), np.int64), "classification_report": ""}

    monkeypatch.setattr(TC, "train_classifier", fake_train)
    monkeypatch.setattr(TC, "evaluate_classifier", fake_eval)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    _run_main(monkeypatch, ["--mode", "train_classifier", "--epochs", "3"])
    assert calls == [("train", "resnet18", 3), ("evaluate", True)]


@pytest.mark.parametrize("argv,env,what", [(["--mode", "train_classifier"], {"WORLD_SIZE": "2"}, "single process"),
                                           (["--mode", "train_classifier", "--resume"], {}, "--resume")])
def test_main_train_classifier_refuses_data_parallel_and_resume(monkeypatch, argv, env, what):
    import training.train_classifier as TC
    monkeypatch.setattr(TC, "train_classifier", lambda *a, **k: pytest.fail("must not train"))
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    with pytest.raises(SystemExit) as ei:
        _run_main(monkeypatch, argv, env)
    assert what in str(ei.value)


def test_classification_report_known_answer():
    from adam_dehaze_amd.train import _accuracy, classification_report3
    cm = np.array([[5, 1, 0],     # low:    support 6, predicted-low column 5 + 2 = 7
                   [2, 3, 1],     # medium: support 6
                   [0, 0, 0]])    # high:   support 0, never predicted correctly (1 predicted): P = 0, R = 0 / 0 -> 0
    assert abs(_accuracy(cm) - 100.0 * 8 / 12) < 1e-12
    rep = classification_report3(cm).splitlines()
    rows = {ln.split()[0]: ln.split()[1:] for ln in rep if ln.strip() and ln.split()[0] in ("low", "medium", "high")}
    # low: P = 5/7, R = 5/6, F1 = 2PR/(P+R) = 10/13; medium: P = 3/4, R = 1/2, F1 = 3/5; high: all 0, support 0
    assert rows["low"] == ["0.71", "0.83", "0.77", "6"]
    assert rows["medium"] == ["0.75", "0.50", "0.60", "6"]
    assert rows["high"] == ["0.00", "0.00", "0.00", "0"]
    acc = [ln for ln in rep if ln.strip().startswith("accuracy")][0].split()
    assert acc[1:] == ["0.67", "12"]
    macro = [ln for ln in rep if ln.strip().startswith("macro avg")][0].split()
    assert macro[2:5] == [f"{(5 / 7 + 3 / 4) / 3:.2f}", f"{(5 / 6 + 1 / 2) / 3:.2f}", f"{(10 / 13 + 3 / 5) / 3:.2f}"]
    weighted = [ln for ln in rep if ln.strip().startswith("weighted avg")][0].split()
    assert weighted[2:5] == [f"{(5 / 7 + 3 / 4) / 2:.2f}", f"{(5 / 6 + 1 / 2) / 2:.2f}", f"{(10 / 13 + 3 / 5) / 2:.2f}"]
