"""`main.py --mode demo --input ...` on the GPU (train.run_demo / image_io.dehaze_files): a routed system at the reduced widths of
tests/test_gpu_train.py with random weights and a fixed seed dehazes PNG files of three modes and two sizes."""
import json
import os
import warnings

import numpy as np
import pytest
import torch

from adam_dehaze_amd import image_io as IO
from adam_dehaze_amd import train as T

pytestmark = pytest.mark.gpu
Image = pytest.importorskip("PIL.Image")
DEV = "cuda:0"
NAMES = ("low", "medium", "high")


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


def _system(routing):
    torch.manual_seed(11)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return T._joint_system_for_evaluation(_cfg(routing))[0]


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    d = tmp_path_factory.mktemp("demo_in")
    g = np.random.default_rng(4)
    arrays = {"a.png": g.integers(0, 256, (32, 48, 3), dtype=np.uint8), "b.png": g.integers(0, 256, (32, 48, 3), dtype=np.uint8),
              "c.png": g.integers(0, 256, (31, 45), dtype=np.uint8), "d.png": g.integers(0, 256, (32, 48, 4), dtype=np.uint8),
              "tiny.png": g.integers(0, 256, (8, 8, 3), dtype=np.uint8)}
    for name, a in arrays.items():
        Image.fromarray(a).save(d / name)
    assert [Image.open(d / n).mode for n in sorted(arrays)] == ["RGB", "RGB", "L", "RGBA", "RGB"]
    return d, arrays


@pytest.fixture(scope="module")
def soft():
    return _system("soft")


@pytest.fixture(scope="module")
def one_by_one(inputs, soft, tmp_path_factory):
    """the run at batch_size = 1 through train.run_demo: (output directory, returned records, warnings)"""
    out = tmp_path_factory.mktemp("demo_bs1")
    cfg = dict(_cfg(), demo={"batch_size": 1})
    mp = pytest.MonkeyPatch()
    mp.setattr(T, "_joint_system_for_evaluation", lambda config: (soft, None))
    try:
        with warnings.catch_warnings(record=True) as rec:
            warnings.simplefilter("always")
            results = T.run_demo(cfg, str(inputs[0]), str(out), False)
    finally:
        mp.undo()
    return out, results, [str(w.message) for w in rec]


def _check_records(results, routing):
    assert [os.path.basename(r["file"]) for r in results] == ["a.png", "b.png", "c.png", "d.png"]
    for r in results:
        assert set(r) == {"file", "height", "width", "routing", "weights", "intensity"} and r["routing"] == routing
        assert len(r["weights"]) == 3 and abs(sum(r["weights"]) - 1.0) <= 1e-6
        assert r["intensity"] == NAMES[int(np.argmax(r["weights"]))]
    assert [(r["height"], r["width"]) for r in results] == [(32, 48), (32, 48), (31, 45), (32, 48)]


def test_batch_size_one_is_the_direct_computation(inputs, soft, one_by_one):
    d, arrays = inputs
    out, results, warned = one_by_one
    assert sum("tiny.png" in w for w in warned) == 1
    assert sorted(os.listdir(out)) == ["a.png", "b.png", "c.png", "d.png", "demo_results.json"]
    for name in ("a.png", "b.png", "c.png", "d.png"):
        with Image.open(out / name) as im:
            assert im.mode == "RGB" and (im.height, im.width) == arrays[name].shape[:2]
        with torch.no_grad():
            y, _ = soft["router"](IO.u8_to_image(IO.load_image(str(d / name)).to(DEV)))
        direct = IO.image_to_u8(y)[0].cpu()
        assert torch.equal(IO.load_image(str(out / name)), direct), name
    assert json.load(open(out / "demo_results.json")) == results
    _check_records(results, "soft")


def test_batch_size_four_is_within_one_level(inputs, soft, one_by_one, tmp_path):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        results = IO.dehaze_files(soft, [str(inputs[0] / n) for n in inputs[1]], str(tmp_path), batch_size=4)
    _check_records(results, "soft")
    for name in ("a.png", "b.png", "c.png", "d.png"):
        a = IO.load_image(str(tmp_path / name)).to(torch.int16)
        b = IO.load_image(str(one_by_one[0] / name)).to(torch.int16)
        worst = int((a - b).abs().max())
        print(f"{name}: batch_size 4 against 1: largest difference {worst} levels")
        assert worst <= 1, name


def test_panels_hold_the_input_and_the_dehazed_file(inputs, soft, tmp_path):
    d, arrays = inputs
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        IO.dehaze_files(soft, [str(d / n) for n in arrays], str(tmp_path), batch_size=4, panels=True)
    assert sorted(os.listdir(tmp_path)) == sorted([n for n in arrays if n != "tiny.png"] +
                                                  [n[:-4] + "_panel.png" for n in arrays if n != "tiny.png"])
    for name in ("a.png", "c.png", "d.png"):
        src = arrays[name] if arrays[name].ndim == 3 else np.repeat(arrays[name][:, :, None], 3, axis=2)
        w = src.shape[1]
        panel = IO.load_image(str(tmp_path / (name[:-4] + "_panel.png"))).numpy()
        assert panel.shape == (src.shape[0], 2 * w, 3)
        assert np.array_equal(panel[:, :w], src[:, :, :3]), f"{name}: the hazy pane is not the file's pixels"
        assert np.array_equal(panel[:, w:], IO.load_image(str(tmp_path / name)).numpy()), name


def test_blend_gather_and_scatter_take_an_image_size_that_is_no_multiple_of_four():
    """a 31 x 45 file gives per = 3 * 31 * 45 = 4185 floats per image: the routers' kernels then move single floats.  2 blocks of
    256 lanes would cover 512; 4185 needs 17, and the images of a batch alternate alignment"""
    from adam_dehaze_amd import _hip as H
    N, per, eps = 3, 3 * 31 * 45, 2.0 ** -24
    g = torch.Generator(device=DEV).manual_seed(21)
    w = torch.softmax(torch.randn(N, 3, device=DEV, generator=g), dim=1).contiguous()
    o = [torch.rand(N, per, device=DEV, generator=g) for _ in range(3)]
    out = torch.full((N, per), float("nan"), device=DEV)
    H.call("adh_soft_blend", w.data_ptr(), o[0].data_ptr(), o[1].data_ptr(), o[2].data_ptr(), N, per, out.data_ptr())
    ref = sum(w.double()[:, i:i + 1] * o[i].double() for i in range(3))
    assert float((out.double() - ref).abs().max()) <= 8 * eps            # three products and two adds of terms in [0, 1]
    sel = torch.tensor([2, 0], device=DEV, dtype=torch.int32)
    dst = torch.full((2, per), float("nan"), device=DEV)
    H.call("adh_gather_images", o[0].data_ptr(), sel.data_ptr(), 2, per, dst.data_ptr())
    assert torch.equal(dst, o[0][sel.long()])
    back = torch.full((N, per), float("nan"), device=DEV)
    H.call("adh_scatter_images", dst.data_ptr(), sel.data_ptr(), 2, per, back.data_ptr())
    assert torch.equal(back[sel.long()], o[0][sel.long()]) and torch.isnan(back[1]).all()


@pytest.mark.parametrize("routing", ["hard", "gated"])
def test_the_other_routers_give_the_same_record(inputs, tmp_path, routing):
    system = _system(routing)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        results = IO.dehaze_files(system, [str(inputs[0] / n) for n in inputs[1]], str(tmp_path), batch_size=4)
    _check_records(results, routing)
    if routing == "hard":
        assert all(sorted(r["weights"]) == [0.0, 0.0, 1.0] for r in results)
    assert sorted(os.listdir(tmp_path)) == ["a.png", "b.png", "c.png", "d.png"]
