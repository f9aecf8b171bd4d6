"""Host side of self-ensemble inference and EXIF orientation without a GPU: the D4 tables of adam_dehaze_amd/d4.py against Pillow
and against each other, the chunk planner with orientations, tag parsing, how the flags and config keys travel from main.py
through train.run_demo to image_io.dehaze_files (today's call shapes when they are absent), and the order in which
d4.self_ensemble calls its function -- the device work stubbed by the torch reference of tests/_d4_cases.py."""
import os
import sys
import warnings

import numpy as np
import pytest
import torch

from adam_dehaze_amd import d4 as D
from adam_dehaze_amd import image_io as IO
from adam_dehaze_amd import train as T
from tests import _d4_cases as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cpu_d4_apply(x, op, out=None, accumulate=False, scale=1.0, flip_ops=None):
    """d4.d4_apply as its docstring defines it, in torch ops on the CPU"""
    v = K.ref(x, *op) if flip_ops is None else K.ref_per_image(x, op[0], flip_ops.tolist())
    if out is None:
        assert not accumulate
        return v * scale if scale != 1.0 else v
    out.copy_((out + v if accumulate else v) * scale)
    return out


def test_the_tables():
    assert D.D4_OPS == K.OPS == [(0, 0), (0, 1), (0, 2), (0, 3), (1, 0), (1, 1), (1, 2), (1, 3)]
    assert IO.D4_OPS is D.D4_OPS and IO.EXIF_TO_D4 is D.EXIF_TO_D4 and IO.self_ensemble is D.self_ensemble
    assert sorted(D.EXIF_TO_D4) == list(range(1, 9)) and sorted(D.EXIF_TO_D4.values()) == D.D4_OPS


def test_inverse_composes_to_the_identity():
    x = torch.arange(2 * 3 * 5 * 7, dtype=torch.float32).reshape(2, 3, 5, 7)
    for op in D.D4_OPS:
        inv = D.d4_inverse(op)
        assert inv in D.D4_OPS
        assert torch.equal(K.ref(K.ref(x, *op), *inv), x), op
        assert torch.equal(K.ref(K.ref(x, *inv), *op), x), op
    assert [D.d4_inverse(op) for op in D.D4_OPS] == [(0, 0), (0, 1), (0, 2), (0, 3), (1, 0), (1, 2), (1, 1), (1, 3)]


def test_exif_table_is_pillows_exif_transpose(tmp_path):
    Image = pytest.importorskip("PIL.Image")
    from PIL import ImageOps
    a = np.random.default_rng(0).integers(0, 256, (5, 7, 3), dtype=np.uint8)
    for tag in range(1, 9):
        exif = Image.Exif()
        exif[0x0112] = tag
        Image.fromarray(a).save(tmp_path / f"t{tag}.png", exif=exif)
        with Image.open(tmp_path / f"t{tag}.png") as im:
            upright = np.array(ImageOps.exif_transpose(im))
        t, got = IO.load_image(str(tmp_path / f"t{tag}.png"), orientation=True)
        assert got == tag and np.array_equal(t.numpy(), a)                       # pixels still in file order
        ours = K.ref(t.permute(2, 0, 1).unsqueeze(0), *D.EXIF_TO_D4[tag])[0].permute(1, 2, 0)
        assert np.array_equal(ours.numpy(), upright), tag
        assert IO.image_size(str(tmp_path / f"t{tag}.png"), orientation=True) == (5, 7, tag)
        assert IO.upright_size(5, 7, tag) == upright.shape[:2]


def test_tag_parsing(tmp_path):
    Image = pytest.importorskip("PIL.Image")
    a = np.zeros((4, 6, 3), np.uint8)
    Image.fromarray(a).save(tmp_path / "none.png")
    assert IO.image_size(str(tmp_path / "none.png"), orientation=True) == (4, 6, 1)
    assert IO.load_image(str(tmp_path / "none.png"), orientation=True)[1] == 1
    for bad in (0, 9, 65535):
        exif = Image.Exif()
        exif[0x0112] = bad
        Image.fromarray(a).save(tmp_path / f"bad{bad}.png", exif=exif)
        assert IO.image_size(str(tmp_path / f"bad{bad}.png"), orientation=True) == (4, 6, 1)
        assert IO.load_image(str(tmp_path / f"bad{bad}.png"), orientation=True)[1] == 1
    assert [D.exif_tag(v) for v in (None, 0, 9, -1, "6", 6.0, True, 1, 8, 6)] == [1, 1, 1, 1, 1, 1, 1, 1, 8, 6]
    # the plain forms are what they were
    assert IO.image_size(str(tmp_path / "none.png")) == (4, 6)
    assert isinstance(IO.load_image(str(tmp_path / "none.png")), torch.Tensor)


def test_planner_groups_by_size_and_transpose_bit():
    sizes = {"f.png": (32, 48), "a.png": (32, 48), "c.png": (31, 45), "b.png": (32, 48), "e.png": (48, 32), "d.png": (32, 48),
             "g.png": (32, 48), "tiny.png": (8, 64)}
    tags = {"a.png": 1, "b.png": 6, "d.png": 3, "f.png": 8, "g.png": 2, "c.png": 5, "e.png": 1, "tiny.png": 6}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        plain = IO.plan_chunks(sizes, 2)
        assert IO.plan_chunks(sizes, 2, None) == plain
        assert IO.plan_chunks(sizes, 2, {p: 1 for p in sizes}) == plain          # all upright: the same chunks
        assert IO.plan_chunks(sizes, 2, {p: 3 for p in sizes}) == plain          # no tag transposes: the same chunks
        got = IO.plan_chunks(sizes, 2, tags)
    assert got == [["a.png", "d.png"], ["g.png"], ["b.png", "f.png"], ["c.png"], ["e.png"]]
    with pytest.warns(UserWarning, match="tiny.png"):
        IO.plan_chunks(sizes, 4, tags)


class _Router:
    def eval(self):
        pass


def test_dehaze_files_call_shapes_and_records(tmp_path, monkeypatch):
    """the device work stubbed: which keywords dehaze_batch gets, and what the records gain"""
    Image = pytest.importorskip("PIL.Image")
    g = np.random.default_rng(1)
    for name, tag in (("a.png", None), ("b.png", 6), ("c.png", 3), ("d.png", 8)):
        exif = Image.Exif()
        if tag:
            exif[0x0112] = tag
        Image.fromarray(g.integers(0, 256, (16, 24, 3), dtype=np.uint8)).save(tmp_path / name, exif=exif)
    seen = []

    def fake_batch(system, u8, want_panels, **kw):
        seen.append((tuple(u8.shape), kw))
        n, h, w = u8.shape[:3]
        if kw.get("tags") and D.EXIF_TO_D4[kw["tags"][0]][0]:
            h, w = w, h
        recs = IO.routing_records({"weights": torch.tensor([[0.2, 0.5, 0.3]] * n)})
        return torch.zeros(n, h, w, 3, dtype=torch.uint8), None, recs

    monkeypatch.setattr(IO, "dehaze_batch", fake_batch)
    system = {"router": _Router(), "device": "cpu"}
    paths = [str(tmp_path / n) for n in ("a.png", "b.png", "c.png", "d.png")]
    plain = IO.dehaze_files(system, paths, str(tmp_path / "o1"), batch_size=4)
    assert seen == [((4, 16, 24, 3), {})]
    assert all(set(r) == {"file", "height", "width", "routing", "weights", "intensity"} for r in plain)
    seen.clear()
    res = IO.dehaze_files(system, paths, str(tmp_path / "o2"), batch_size=4, exif=True)
    assert seen == [((2, 16, 24, 3), {"tags": [1, 3]}), ((2, 16, 24, 3), {"tags": [6, 8]})]
    assert [(r["height"], r["width"], r["orientation"]) for r in res] == [(16, 24, 1), (24, 16, 6), (16, 24, 3), (24, 16, 8)]
    assert all(set(r) == {"file", "height", "width", "routing", "weights", "intensity", "orientation"} for r in res)
    with Image.open(tmp_path / "o2" / "b.png") as im:
        assert (im.height, im.width) == (24, 16) and im.getexif().get(0x0112) is None
    seen.clear()
    IO.dehaze_files(system, paths, str(tmp_path / "o3"), batch_size=4, self_ensemble="d8")
    assert seen == [((4, 16, 24, 3), {"self_ensemble": "d8"})]
    with pytest.raises(ValueError, match="self_ensemble"):
        IO.dehaze_files(system, paths, str(tmp_path / "o4"), self_ensemble="x16")


def test_pair_targets_compares_upright_sizes(tmp_path):
    Image = pytest.importorskip("PIL.Image")
    hazy, clear = tmp_path / "hazy", tmp_path / "clear"
    hazy.mkdir(), clear.mkdir()
    exif = Image.Exif()
    exif[0x0112] = 6
    Image.fromarray(np.zeros((16, 24, 3), np.uint8)).save(hazy / "a.png", exif=exif)          # upright 24 x 16
    Image.fromarray(np.zeros((24, 16, 3), np.uint8)).save(clear / "a.png")
    p = str(hazy / "a.png")
    assert IO.pair_targets([p], str(clear), exif=True)[p] == {"target": str(clear / "a.png")}
    assert IO.pair_targets([p], str(clear))[p]["reason"] == "size 16x24 != 24x16"


def test_run_demo_reads_the_config_and_the_argument_wins(tmp_path, monkeypatch):
    Image = pytest.importorskip("PIL.Image")
    Image.fromarray(np.zeros((16, 16, 3), np.uint8)).save(tmp_path / "a.png")
    calls = []

    def fake_files(system, paths, out_dir, **kw):
        calls.append(kw)
        os.makedirs(out_dir, exist_ok=True)
        return [{"file": p, "height": 16, "width": 16, "routing": "soft", "weights": [0.2, 0.5, 0.3], "intensity": "medium"}
                for p in paths]

    pairs = []
    monkeypatch.setattr(IO, "dehaze_files", fake_files)
    monkeypatch.setattr(IO, "pair_targets", lambda *a, **k: (pairs.append((len(a), k)), {})[1])
    monkeypatch.setattr(T, "_joint_system_for_evaluation", lambda config: ("the system", None))
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    inp, out = str(tmp_path / "a.png"), str(tmp_path / "out")
    T.run_demo({}, inp, out, False)
    T.run_demo({"demo": {"batch_size": 2, "self_ensemble": "flip", "exif_orientation": True}}, inp, out, False)
    T.run_demo({"demo": {"self_ensemble": "flip"}}, inp, out, True, self_ensemble="d8")
    T.run_demo({"demo": {"exif_orientation": False}}, inp, out, False, exif=True)
    assert calls == [{"batch_size": 4, "panels": False},
                     {"batch_size": 2, "panels": False, "self_ensemble": "flip", "exif": True},
                     {"batch_size": 4, "panels": True, "self_ensemble": "d8"},
                     {"batch_size": 4, "panels": False, "exif": True}]
    T.run_demo({}, inp, out, False, target=inp)
    T.run_demo({}, inp, out, False, target=inp, exif=True)
    assert pairs == [(2, {}), (2, {"exif": True})]
    assert list(calls[-2]) == ["batch_size", "panels", "targets"] and list(calls[-1]) == ["batch_size", "panels", "targets", "exif"]
    with pytest.raises(SystemExit, match="x16"):
        T.run_demo({"demo": {"self_ensemble": "x16"}}, inp, out, False)


def test_main_flags_reach_run_demo_only_when_given(monkeypatch, tmp_path):
    import main as M
    calls = []
    monkeypatch.setattr(T, "run_demo", lambda *a, **k: calls.append((a[1:], k)))
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.chdir(ROOT)
    base = ["main.py", "--mode", "demo", "--input", "hazy", "--device", "cpu"]
    for extra in ([], ["--self-ensemble", "d8"], ["--exif"], ["--self-ensemble", "flip", "--exif", "--target", "clear"]):
        monkeypatch.setattr(sys, "argv", base + extra)
        M.main()
    assert calls == [(("hazy", "demo", False), {}), (("hazy", "demo", False), {"self_ensemble": "d8"}),
                     (("hazy", "demo", False), {"exif": True}),
                     (("hazy", "demo", False), {"target": "clear", "self_ensemble": "flip", "exif": True})]
    # today's signature still takes the plain call
    monkeypatch.setattr(T, "run_demo", lambda config, inp, out, panels: calls.append("plain"))
    monkeypatch.setattr(sys, "argv", base)
    M.main()
    assert calls[-1] == "plain"
    monkeypatch.setattr(T, "run_demo", lambda *a, **k: pytest.fail("must not run"))
    for argv in (["main.py", "--mode", "evaluate", "--exif"], ["main.py", "--mode", "demo", "--self-ensemble", "d8"]):
        monkeypatch.setattr(sys, "argv", argv + ["--device", "cpu"])
        with pytest.raises(SystemExit, match="--mode demo --input"):
            M.main()
    monkeypatch.setattr(sys, "argv", base + ["--self-ensemble", "x16"])
    with pytest.raises(SystemExit):
        M.main()


@pytest.mark.parametrize("mode,n", [("flip", 4), ("d8", 8)])
def test_self_ensemble_order_count_and_aux(monkeypatch, mode, n):
    monkeypatch.setattr(D, "d4_apply", _cpu_d4_apply)
    x = K.random((2, 3, 5, 7), 2)
    plane = {(5, 7): K.random((1, 1, 5, 7), 3), (7, 5): K.random((1, 1, 7, 5), 4)}
    seen = []

    def fn(b):
        seen.append(b.clone())
        return b * plane[tuple(b.shape[2:])], {"call": len(seen)}

    y, aux = D.self_ensemble(fn, x, mode)
    assert aux == {"call": 1} and len(seen) == n
    for got, op in zip(seen, D.D4_OPS):
        assert torch.equal(got, K.ref(x, *op)), op                       # list order, every variant through fn
    acc = None
    for op in D.D4_OPS[:n]:
        v = K.ref(x, *op)
        t = K.ref(v * plane[tuple(v.shape[2:])], *D.d4_inverse(op))
        acc = t if acc is None else acc + t
    assert torch.equal(y, acc * (1.0 / n)) and not y.requires_grad
    with pytest.raises(ValueError, match="mode"):
        D.self_ensemble(fn, x, "x16")


def test_evaluation_key_is_read_and_checked():
    assert T._self_ensemble_mode({}) is None and T._self_ensemble_mode({"evaluation": {"ciede2000": True}}) is None
    assert T._self_ensemble_mode({"evaluation": {"self_ensemble": "d8"}}) == "d8"
    with pytest.raises(ValueError, match="self_ensemble"):
        T._self_ensemble_mode({"evaluation": {"self_ensemble": True}})
