"""Self-ensemble inference and EXIF orientation on the GPU: the demo path (image_io.dehaze_batch / dehaze_files / train.run_demo)
and evaluate_joint_model with the routed system of tests/test_gpu_demo.py (reduced widths, random weights, a fixed seed).  The D4
launches are exact, so everything the options add is compared byte for byte with the same router calls composed in torch ops."""
import json
import os
import warnings

import numpy as np
import pytest
import torch

from adam_dehaze_amd import d4 as D
from adam_dehaze_amd import image_io as IO
from adam_dehaze_amd import train as T
from tests import _d4_cases as K
from tests.test_gpu_demo import _cfg, _system

pytestmark = pytest.mark.gpu
Image = pytest.importorskip("PIL.Image")
DEV = "cuda:0"
BASE_KEYS = {"file", "height", "width", "routing", "weights", "intensity"}


@pytest.fixture(scope="module")
def soft():
    return _system("soft")


@pytest.fixture(scope="module")
def batches():
    g = np.random.default_rng(4)
    return [torch.from_numpy(g.integers(0, 256, (2, 32, 48, 3), dtype=np.uint8)),
            torch.from_numpy(g.integers(0, 256, (1, 31, 45, 1), dtype=np.uint8))]


def _composition(system, u8, ops):
    """the ensemble of the same router calls written in torch ops on the device, packed by the same kernel"""
    x = IO.u8_to_image(u8.to(DEV))
    acc = None
    with torch.no_grad():
        for op in ops:
            y, _ = system["router"](K.ref(x, *op).clone())
            t = K.ref(y, *D.d4_inverse(op)).clone()
            acc = t if acc is None else acc + t
    return IO.image_to_u8(acc * (1.0 / len(ops))).cpu()


@pytest.mark.parametrize("mode", ["d8", "flip"])
def test_demo_path_is_the_torch_composition_byte_for_byte(soft, batches, mode):
    ops = D.SELF_ENSEMBLE_MODES[mode]
    for u8 in batches:
        out, panel, records = IO.dehaze_batch(soft, u8, self_ensemble=mode)
        assert panel is None and [r["self_ensemble"] for r in records] == [len(ops)] * u8.shape[0]
        want = _composition(soft, u8, ops)
        assert torch.equal(out, want), (tuple(u8.shape), int((out.int() - want.int()).abs().max()))
        plain, _, plain_records = IO.dehaze_batch(soft, u8)
        assert all("self_ensemble" not in r for r in plain_records)
        differ = int((out != plain).sum())
        print(f"{mode} {tuple(u8.shape)}: {differ} of {out.numel()} bytes differ from the single pass")
        assert differ > 0, "the ensemble changed nothing: it is off, or the model is equivariant"
        assert [{k: r[k] for k in ("routing", "weights", "intensity")} for r in records] == plain_records


def test_panels_hold_the_input_and_the_ensemble(soft, batches):
    u8 = batches[0]
    out, panel, _ = IO.dehaze_batch(soft, u8, True, self_ensemble="flip")
    assert torch.equal(panel[:, :, :48], u8) and torch.equal(panel[:, :, 48:], out)
    assert torch.equal(out, IO.dehaze_batch(soft, u8, self_ensemble="flip")[0])


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    d = tmp_path_factory.mktemp("se_in")
    g = np.random.default_rng(4)
    arrays = {"a.png": g.integers(0, 256, (32, 48, 3), dtype=np.uint8), "b.png": g.integers(0, 256, (32, 48, 3), dtype=np.uint8),
              "c.png": g.integers(0, 256, (31, 45), dtype=np.uint8)}
    for name, a in arrays.items():
        Image.fromarray(a).save(d / name)
    return d, arrays


@pytest.mark.parametrize("routing", ["hard", "soft", "gated"])
def test_all_three_routers_in_flip_mode(inputs, tmp_path, routing):
    system = _system(routing)
    paths = [str(inputs[0] / n) for n in inputs[1]]
    plain = IO.dehaze_files(system, paths, str(tmp_path / "plain"), batch_size=4)
    flip = IO.dehaze_files(system, paths, str(tmp_path / "flip"), batch_size=4, self_ensemble="flip")
    assert all(set(r) == BASE_KEYS for r in plain) and all(set(r) == BASE_KEYS | {"self_ensemble"} for r in flip)
    assert [{k: v for k, v in r.items() if k != "self_ensemble"} for r in flip] == plain      # the upright pass's routing
    assert [r["self_ensemble"] for r in flip] == [4, 4, 4] and [r["routing"] for r in flip] == [routing] * 3
    for name in inputs[1]:
        a, b = IO.load_image(str(tmp_path / "plain" / name)), IO.load_image(str(tmp_path / "flip" / name))
        assert a.shape == b.shape and not torch.equal(a, b), name


@pytest.fixture(scope="module")
def tagged(tmp_path_factory):
    """one 32 x 48 array saved under the eight orientation tags, and what Pillow makes of each, saved without a tag"""
    from PIL import ImageOps
    d, up = tmp_path_factory.mktemp("tagged"), tmp_path_factory.mktemp("upright")
    a = np.random.default_rng(9).integers(0, 256, (32, 48, 3), dtype=np.uint8)
    for tag in range(1, 9):
        exif = Image.Exif()
        exif[0x0112] = tag
        Image.fromarray(a).save(d / f"t{tag}.png", exif=exif)
        with Image.open(d / f"t{tag}.png") as im:
            assert im.getexif().get(0x0112) == tag
            ImageOps.exif_transpose(im).save(up / f"t{tag}.png")
        with Image.open(up / f"t{tag}.png") as im:
            assert im.getexif().get(0x0112) is None and (im.height, im.width) == ((48, 32) if tag >= 5 else (32, 48))
    return d, up, a


def test_exif_end_to_end(soft, tagged, tmp_path):
    d, up, _ = tagged
    names = [f"t{k}.png" for k in range(1, 9)]
    mp = pytest.MonkeyPatch()
    mp.setattr(T, "_joint_system_for_evaluation", lambda config: (soft, None))
    try:
        got = T.run_demo(_cfg(), str(d), str(tmp_path / "exif"), True, exif=True)
        want = T.run_demo(_cfg(), str(up), str(tmp_path / "upright"), True)
    finally:
        mp.undo()
    assert [os.path.basename(r["file"]) for r in got] == names
    assert [(r["height"], r["width"], r["orientation"]) for r in got] == [(32, 48, k) for k in range(1, 5)] + \
        [(48, 32, k) for k in range(5, 9)]
    assert [(r["height"], r["width"]) for r in want] == [(r["height"], r["width"]) for r in got]
    assert all(set(r) == BASE_KEYS | {"orientation"} for r in got) and all(set(r) == BASE_KEYS for r in want)
    assert json.load(open(tmp_path / "exif" / "demo_results.json")) == got
    for name in names:
        for f in (name, name[:-4] + "_panel.png"):                    # the panel's left pane is the upright input
            a, b = IO.load_image(str(tmp_path / "exif" / f)), IO.load_image(str(tmp_path / "upright" / f))
            assert torch.equal(a, b), f
        with Image.open(tmp_path / "exif" / name) as im:
            assert im.getexif().get(0x0112) is None


def test_without_exif_the_tag_is_not_looked_at(soft, tagged, tmp_path):
    d, _, a = tagged
    paths = [str(d / f"t{k}.png") for k in (1, 6, 8)]
    results = IO.dehaze_files(soft, paths, str(tmp_path), batch_size=1)
    assert all(set(r) == BASE_KEYS and (r["height"], r["width"]) == (32, 48) for r in results)
    with torch.no_grad():
        y, _ = soft["router"](IO.u8_to_image(torch.from_numpy(a).to(DEV)))
    direct = IO.image_to_u8(y)[0].cpu()
    for k in (1, 6, 8):
        assert torch.equal(IO.load_image(str(tmp_path / f"t{k}.png")), direct), k


def test_a_tagged_target_scores_as_the_upright_pair(soft, tmp_path):
    from PIL import ImageOps
    g = np.random.default_rng(21)
    dirs = {n: tmp_path / n for n in ("hazy", "clear", "hazy_up", "clear_up")}
    for p in dirs.values():
        p.mkdir()
    # inputs stored 32 x 48; a's target is stored 48 x 32 under a transposing tag of its own, b's 32 x 48 under a flip
    for name, shape, tag, where in (("a.png", (32, 48, 3), 6, "hazy"), ("a.png", (48, 32, 3), 3, "clear"),
                                    ("b.png", (32, 48, 3), 6, "hazy"), ("b.png", (32, 48, 3), 5, "clear")):
        exif = Image.Exif()
        exif[0x0112] = tag
        Image.fromarray(g.integers(0, 256, shape, dtype=np.uint8)).save(dirs[where] / name, exif=exif)
        with Image.open(dirs[where] / name) as im:
            ImageOps.exif_transpose(im).save(dirs[where + "_up"] / name)
    hazy = [str(dirs["hazy"] / n) for n in ("a.png", "b.png")]
    up = [str(dirs["hazy_up"] / n) for n in ("a.png", "b.png")]
    pairs = IO.pair_targets(hazy, str(dirs["clear"]), exif=True)
    assert all(set(v) == {"target"} for v in pairs.values())                       # upright sizes match: 48 x 32 both
    assert "reason" in IO.pair_targets(hazy, str(dirs["clear"]))[hazy[0]]           # stored sizes do not
    got = IO.dehaze_files(soft, hazy, str(tmp_path / "o1"), batch_size=4, targets=pairs, exif=True)
    want = IO.dehaze_files(soft, up, str(tmp_path / "o2"), batch_size=4, targets=IO.pair_targets(up, str(dirs["clear_up"])))
    for r, w in zip(got, want):
        assert r["scored"] is True and w["scored"] is True and (r["height"], r["width"]) == (48, 32)
        for k in IO.SCORE_KEYS:
            print(f"{os.path.basename(r['file'])} {k}: tagged {r[k]!r}, upright {w[k]!r}")
            assert r[k] == w[k], k                                                 # the same kernels on the same tensors


def test_evaluate_joint_model_with_the_flip_ensemble(tmp_path):
    runs = {}
    for name, extra in (("plain", {}), ("flip", {"self_ensemble": "flip"})):
        cfg = _cfg()
        cfg["dataset"] = {"batch_size": 4, "img_size": 32}
        cfg["evaluation"] = {"results_dir": str(tmp_path / name), **extra}
        cfg["joint_training"]["checkpoint_dir"] = str(tmp_path / "nojoint")
        torch.manual_seed(6)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            res = T.evaluate_joint_model(cfg, steps=2, use_lpips=False)
        runs[name] = (res, json.load(open(tmp_path / name / "joint_model_results.json")))
    (plain, plain_saved), (flip, flip_saved) = runs["plain"], runs["flip"]
    assert plain_saved == plain and "self_ensemble" not in plain_saved
    assert flip_saved.pop("self_ensemble") == {"mode": "flip", "passes": 4} and flip_saved == flip
    assert set(flip) == set(plain) and sum(v["samples"] for v in flip.values()) == 8
    for cat in plain:
        print(f"{cat}: PSNR plain {plain[cat]['psnr']!r}, flip {flip[cat]['psnr']!r}")
        assert flip[cat]["samples"] == plain[cat]["samples"] and flip[cat]["psnr"] != plain[cat]["psnr"]
