"""Host side of `main.py --mode demo --input ...` without a GPU: how image_io.dehaze_files sorts, groups and chunks its files
(the device work stubbed out), the one routing record for the three routers, load_image / save_image through Pillow, what
train.run_demo lists and writes, and the refusal under WORLD_SIZE > 1."""
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


def test_plan_chunks_sorts_groups_by_size_and_cuts():
    sizes = {"f.png": (32, 48), "a.png": (32, 48), "c.png": (31, 45), "b.png": (32, 48), "e.png": (48, 32), "d.png": (32, 48),
             "g.png": (32, 48), "tiny.png": (8, 64)}
    with pytest.warns(UserWarning, match="tiny.png") as rec:
        chunks = IO.plan_chunks(sizes, 2)
    assert len(rec) == 1
    assert chunks == [["a.png", "b.png"], ["d.png", "f.png"], ["g.png"], ["c.png"], ["e.png"]]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        assert IO.plan_chunks(sizes, 8) == [["a.png", "b.png", "d.png", "f.png", "g.png"], ["c.png"], ["e.png"]]
        assert [len(c) for c in IO.plan_chunks(sizes, 1)] == [1] * 7
    assert IO.plan_chunks({"x.png": (16, 16)}, 4) == [["x.png"]]            # 16 is not too small
    with pytest.raises(ValueError):
        IO.plan_chunks(sizes, 0)


@pytest.mark.parametrize("aux,kind,weights,names", [
    ({"intensity": torch.tensor([2, 0, 1]), "low_mask": None, "medium_mask": None, "high_mask": None}, "hard",
     [[0.0, 0.0, 1.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]], ["high", "low", "medium"]),
    ({"weights": torch.tensor([[0.2, 0.5, 0.3], [0.7, 0.2, 0.1]]), "individual_outputs": {}}, "soft",
     [[0.2, 0.5, 0.3], [0.7, 0.2, 0.1]], ["medium", "low"]),
    ({"gate_weights": torch.tensor([[0.1, 0.1, 0.8]]), "individual_outputs": {}}, "gated", [[0.1, 0.1, 0.8]], ["high"])])
def test_routing_records_have_one_schema(aux, kind, weights, names):
    recs = IO.routing_records(aux)
    assert [set(r) for r in recs] == [{"routing", "weights", "intensity"}] * len(names)
    assert [r["routing"] for r in recs] == [kind] * len(names) and [r["intensity"] for r in recs] == names
    assert np.allclose([r["weights"] for r in recs], weights, atol=1e-7)
    json.dumps(recs)
    with pytest.raises(KeyError):
        IO.routing_records({"individual_outputs": {}})


def _write_inputs(d):
    Image = pytest.importorskip("PIL.Image")
    g = np.random.default_rng(3)
    files = {"a.png": ("RGB", (32, 48, 3)), "b.png": ("RGB", (32, 48, 3)), "c.png": ("L", (31, 45)), "d.png": ("RGBA", (32, 48, 4)),
             "tiny.png": ("RGB", (8, 8, 3))}
    arrays = {}
    for name, (mode, shape) in files.items():
        arrays[name] = g.integers(0, 256, shape, dtype=np.uint8)
        Image.fromarray(arrays[name]).save(d / name)
        assert Image.open(d / name).mode == mode
    return arrays


def test_load_image_modes_and_save_round_trip(tmp_path):
    Image = pytest.importorskip("PIL.Image")
    arrays = _write_inputs(tmp_path)
    for name, c in (("a.png", 3), ("c.png", 1), ("d.png", 4)):
        t = IO.load_image(str(tmp_path / name))
        assert t.dtype == torch.uint8 and t.dim() == 3 and t.shape[2] == c
        assert np.array_equal(t.numpy().reshape(arrays[name].shape), arrays[name])
        assert IO.image_size(str(tmp_path / name)) == t.shape[:2]
        IO.save_image(str(tmp_path / ("again_" + name)), t)
        assert torch.equal(IO.load_image(str(tmp_path / ("again_" + name))), t)
    # a palette image goes through convert("RGB")
    pal = Image.fromarray(arrays["a.png"]).convert("P", palette=Image.Palette.ADAPTIVE, colors=16)
    pal.save(tmp_path / "p.png")
    assert Image.open(tmp_path / "p.png").mode == "P"
    t = IO.load_image(str(tmp_path / "p.png"))
    assert tuple(t.shape) == (32, 48, 3) and np.array_equal(t.numpy(), np.array(pal.convert("RGB")))
    IO.save_image(str(tmp_path / "x.bmp"), IO.load_image(str(tmp_path / "a.png")))       # the extension names the format
    assert Image.open(tmp_path / "x.bmp").format == "BMP"
    with pytest.raises(ValueError):
        IO.save_image(str(tmp_path / "bad.png"), torch.zeros(4, 4, 2, dtype=torch.uint8))


class _Router:
    def eval(self):
        self.was_eval = True


@pytest.mark.parametrize("panels", [False, True])
def test_dehaze_files_with_the_device_work_stubbed(tmp_path, monkeypatch, panels):
    arrays = _write_inputs(tmp_path)
    batches = []

    def fake_batch(system, u8, want_panels):
        assert u8.dtype == torch.uint8 and not u8.is_cuda and want_panels is panels
        batches.append(tuple(u8.shape))
        rgb = u8.expand(-1, -1, -1, 3) if u8.shape[3] == 1 else u8[..., :3]
        out = 255 - rgb
        panel = torch.cat([rgb, out], dim=2) if want_panels else None
        return out, panel, IO.routing_records({"weights": torch.tensor([[0.2, 0.5, 0.3]] * u8.shape[0])})

    monkeypatch.setattr(IO, "dehaze_batch", fake_batch)
    system = {"router": _Router(), "device": "cpu"}
    paths = [str(tmp_path / n) for n in ("d.png", "tiny.png", "c.png", "b.png", "a.png")]
    out_dir = tmp_path / "out"
    with pytest.warns(UserWarning, match="tiny.png"):
        results = IO.dehaze_files(system, paths, str(out_dir), batch_size=2, panels=panels)
    assert system["router"].was_eval
    # a, b (RGB) | d alone (RGBA stays RGBA: nothing to mix with) | c (grey)
    assert batches == [(2, 32, 48, 3), (1, 32, 48, 4), (1, 31, 45, 1)]
    assert [os.path.basename(r["file"]) for r in results] == ["a.png", "b.png", "c.png", "d.png"]
    assert [(r["height"], r["width"]) for r in results] == [(32, 48), (32, 48), (31, 45), (32, 48)]
    assert all(set(r) == {"file", "height", "width", "routing", "weights", "intensity"} for r in results)
    want = sorted(n for n in arrays if n != "tiny.png")
    if panels:
        want = sorted(want + [n[:-4] + "_panel.png" for n in want])
    assert sorted(os.listdir(out_dir)) == want
    for n in ("a.png", "b.png", "c.png", "d.png"):
        src = arrays[n] if arrays[n].ndim == 3 else np.repeat(arrays[n][:, :, None], 3, axis=2)
        got = IO.load_image(str(out_dir / n)).numpy()
        assert np.array_equal(got, 255 - src[:, :, :3]), n
        if panels:
            pan = IO.load_image(str(out_dir / (n[:-4] + "_panel.png"))).numpy()
            w = src.shape[1]
            assert pan.shape == (src.shape[0], 2 * w, 3) and np.array_equal(pan[:, :w], src[:, :, :3]) and \
                np.array_equal(pan[:, w:], got), n
    # one chunk of mixed channel counts becomes RGB on the host
    batches.clear()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        IO.dehaze_files(system, paths, str(out_dir), batch_size=4, panels=panels)
    assert batches == [(3, 32, 48, 3), (1, 31, 45, 1)]
    with pytest.raises(ValueError, match="base name"):
        IO.dehaze_files(system, [str(tmp_path / "a.png"), str(tmp_path / "sub" / "a.jpg")], str(out_dir))


def test_run_demo_lists_the_directory_and_writes_the_json(tmp_path, monkeypatch, capsys):
    _write_inputs(tmp_path)
    (tmp_path / "notes.txt").write_text("not an image")
    os.rename(tmp_path / "b.png", tmp_path / "B.PNG")
    seen = {}

    def fake_files(system, paths, out_dir, batch_size=4, panels=False):
        seen.update(paths=list(paths), out_dir=out_dir, batch_size=batch_size, panels=panels, system=system)
        os.makedirs(out_dir, exist_ok=True)
        return [{"file": p, "height": 1, "width": 2, "routing": "soft", "weights": [0.2, 0.5, 0.3], "intensity": "medium"}
                for p in paths]

    monkeypatch.setattr(IO, "dehaze_files", fake_files)
    monkeypatch.setattr(T, "_joint_system_for_evaluation", lambda config: ("the system", None))
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    out = tmp_path / "out"
    res = T.run_demo({"demo": {"batch_size": 3}}, str(tmp_path), str(out), True)
    assert [os.path.basename(p) for p in seen["paths"]] == ["B.PNG", "a.png", "c.png", "d.png", "tiny.png"]
    assert (seen["out_dir"], seen["batch_size"], seen["panels"], seen["system"]) == (str(out), 3, True, "the system")
    assert json.load(open(out / "demo_results.json")) == res
    lines = [ln for ln in capsys.readouterr().out.splitlines() if "routing" in ln]
    assert len(lines) == 5 and "medium" in lines[0] and "0.500" in lines[0]
    # one file; the default batch size
    T.run_demo({}, str(tmp_path / "a.png"), str(out), False)
    assert seen["paths"] == [str(tmp_path / "a.png")] and seen["batch_size"] == 4 and seen["panels"] is False
    for bad in (str(tmp_path / "missing"), str(out)):                       # no such path; a directory without images
        with pytest.raises(SystemExit):
            T.run_demo({}, bad, str(out), False)
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(SystemExit, match="single process"):
        T.run_demo({}, str(tmp_path), str(out), False)


def test_main_demo_refuses_data_parallel_before_touching_a_device(monkeypatch, tmp_path):
    import main as M
    monkeypatch.setattr(T, "run_demo", lambda *a, **k: pytest.fail("must not run"))
    monkeypatch.setattr(T, "build_joint_system", lambda *a, **k: pytest.fail("must not build"))
    monkeypatch.setattr(torch.cuda, "set_device", lambda *a, **k: pytest.fail("must not touch a device"))
    monkeypatch.setattr(sys, "argv", ["main.py", "--mode", "demo", "--input", str(tmp_path)])
    monkeypatch.setenv("WORLD_SIZE", "2")
    monkeypatch.chdir(ROOT)
    with pytest.raises(SystemExit) as ei:
        M.main()
    assert "single process" in str(ei.value)


def test_main_demo_flags_reach_run_demo(monkeypatch, tmp_path):
    import main as M
    calls = []
    monkeypatch.setattr(T, "run_demo", lambda config, inp, out, panels: calls.append((inp, out, panels, config["device"])))
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.chdir(ROOT)
    monkeypatch.setattr(sys, "argv", ["main.py", "--mode", "demo", "--input", "pics", "--output", str(tmp_path), "--panels",
                                      "--device", "cpu"])
    M.main()
    monkeypatch.setattr(sys, "argv", ["main.py", "--mode", "demo", "--input", "one.jpg", "--device", "cpu"])
    M.main()
    assert calls == [("pics", str(tmp_path), True, "cpu"), ("one.jpg", "demo", False, "cpu")]
