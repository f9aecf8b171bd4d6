"""The host side of haze synthesis without a GPU: the float64 reference of tests/_haze_synth_ref64.py against plain torch / numpy
expressions, the draw order of data.draw_haze_params, the evaluation draws, data.haze_index, image_io.load_depth, and every
refusal of data.batch_haze_from_windows and of folder_loader's `dataset.synthetic_haze` that needs no device."""
import os

import numpy as np
import pytest
import torch

from adam_dehaze_amd import data as D
from adam_dehaze_amd import image_io as IO
from tests import _dataset_ref64 as R
from tests import _dataset_window_cases as K
from tests import _haze_synth_ref64 as Z


# ------------------------------------------------------------------------------------------------ the reference itself
def test_radial_depth_is_the_reference_expression():
    for CH, CW in ((5, 7), (1, 9), (9, 1), (1, 1)):
        d = Z.radial_depth(CH, CW)
        assert d.shape == (CH, CW)
        for y in range(CH):
            for x in range(CW):
                u, v = (x / (CW - 1) if CW > 1 else 0.0), (y / (CH - 1) if CH > 1 else 0.0)
                assert abs(d[y, x] - (0.3 + 0.7 * ((u - 0.5) ** 2 + (v - 0.2) ** 2) ** 0.5)) <= 1e-15


@pytest.mark.parametrize("radial", [False, True])
def test_haze_ref_against_torch(radial):
    rng = np.random.RandomState(3)
    N, CH, CW = 3, 6, 10
    clear = rng.randint(0, 256, size=(N, CH, CW, 3)).astype(np.uint8)
    depth = None if radial else rng.randint(0, 65536, size=(N, CH, CW)).astype(np.uint16)
    fog = np.array([[0.2, 0.6], [0.55, 0.8], [0.95, 1.0]], np.float32)
    got = Z.haze_ref(clear, depth, fog, (0.25, 1.5))
    J = torch.from_numpy(clear).double().permute(0, 3, 1, 2) / 255
    if radial:
        d = torch.from_numpy(Z.radial_depth(CH, CW)).expand(N, CH, CW)
    else:
        d = 0.25 + 1.25 * torch.from_numpy(depth.astype(np.int64)).double() / 65535
    beta, A = (torch.from_numpy(fog[:, k]).double().view(N, 1, 1, 1) for k in (0, 1))
    t = torch.exp(-beta * d[:, None])
    want = (J * t + A * (1 - t)).clamp(0, 1)
    assert got.shape == (N, 3, CH, CW) and np.abs(got - want.numpy()).max() <= 4e-16
    assert (got >= J.numpy() - 1e-15).any() and got.min() >= 0 and got.max() <= 1
    # the transform is that of the clear reference: beta = 0 leaves the clear pixels, and augment(fog(x)) flips the haze along
    rows = K.param_sets(0, N, 1)[0]
    fog0 = fog.copy()
    fog0[:, 0] = 0
    assert np.abs(Z.haze_ref(clear, depth, fog0, (0.25, 1.5), rows) - R.batch_ref(clear, np.arange(N), rows)).max() <= 1e-15
    for n in range(N):
        assert np.abs(Z.haze_ref(clear, depth, fog, (0.25, 1.5), rows)[n] - Z.augment_ref(got[n], rows[n])).max() == 0


def test_bounds_are_the_written_counts():
    assert Z.HAZE_BOUND == 2 * 2.0 ** -24 + Z.HAZE_F64_UNITS * 2.0 ** -53 and Z.HAZE_BOUND < 2.001 * 2.0 ** -24
    assert Z.HAZE_AUG_BOUND == 9 * 2.0 ** -24 + 2 * Z.HAZE_F64_UNITS * 2.0 ** -53 and Z.HAZE_AUG_BOUND < 9.001 * 2.0 ** -24
    assert Z.resize16_delta(40, 56, 32, 32) == pytest.approx(R.resize_delta(40, 56, 32, 32) * 65535 / 255)


def test_resize16_values_against_interpolate():
    rng = np.random.RandomState(5)
    for (h, w), (OH, OW) in Z.RESIZE16_CASES + Z.RESIZE16_DYADIC:
        src = rng.randint(0, 65536, size=(h, w)).astype(np.uint16)
        want = torch.nn.functional.interpolate(torch.from_numpy(src.astype(np.float64))[None, None], size=(OH, OW), mode="bilinear",
                                               align_corners=False)[0, 0].numpy()
        assert np.abs(Z.resize16_values(src, OH, OW) - want).max() <= 1e-7
    src = rng.randint(0, 65536, size=(7, 5)).astype(np.uint16)
    assert np.array_equal(Z.resize16_values(src, 7, 5), src.astype(np.float64))


def test_case_table_reaches_every_path():
    phases, dphases = set(), set()
    for case in Z.CASES:
        clear, depth, geom, dc, dd, fog = Z.build(case)
        CH, CW = case["crop"]
        assert fog.dtype == np.float32 and fog.shape == (len(geom), 2) and case["dbase"] % 2 == 0
        for (co, cp, do, dp), wc, wd in zip(geom.tolist(), dc, dd):
            assert do % 2 == 0 and dp % 2 == 0
            for y in range(CH):
                assert np.array_equal(clear[co + y * cp:co + y * cp + CW * 3].reshape(CW, 3), wc[y])
                assert np.array_equal(depth[(do + y * dp) // 2:(do + y * dp) // 2 + CW], wd[y])
            if case["pack"] == 4:
                phases.add(co % 4), dphases.add(do % 4)
        ends = [(g[0] + (CH - 1) * g[1] + CW * 3, g[2] + (CH - 1) * g[3] + CW * 2) for g in geom.tolist()]
        if case["name"] in ("5x7_bytes", "8x12_phases", "tight_end_off_4"):      # a window that ends on the last byte of both caches
            assert (clear.size, depth.size * 2) in ends, case["name"]
    assert phases == {0, 1, 2, 3} and dphases == {0, 2}
    names = {c["name"] for c in Z.CASES}
    assert {"5x7_bytes", "8x12_phases", "1x9", "9x1", "40x130"} <= names
    assert any(c["base"] % 4 for c in Z.CASES) and any(c["dbase"] % 4 for c in Z.CASES) and any(c["out_off"] for c in Z.CASES)
    assert any((Z.build(c)[0].size % 4, (Z.build(c)[1].size * 2) % 4) == (3, 2) for c in Z.CASES if not c["gpu_only"])


# ------------------------------------------------------------------------------------------------ draws
def test_draw_haze_params_order_and_ranges():
    labels, fog = D.draw_haze_params(64, np.random.RandomState(11))
    assert labels.dtype == torch.int64 and tuple(labels.shape) == (64,) and fog.dtype == torch.float32 and tuple(fog.shape) == (64, 2)
    rng = np.random.RandomState(11)
    for n in range(64):
        label = rng.randint(0, 3)
        (b0, b1), (a0, a1) = D.FOG_RANGES[D.LEVEL_NAMES[label]]
        beta, A = rng.uniform(b0, b1), rng.uniform(a0, a1)
        assert int(labels[n]) == label and float(fog[n, 0]) == float(np.float32(beta)) and float(fog[n, 1]) == float(np.float32(A))
        assert np.float32(b0) <= fog[n, 0] <= np.float32(b1) and np.float32(a0) <= fog[n, 1] <= np.float32(a1)
    assert set(labels.tolist()) == {0, 1, 2}
    empty = D.draw_haze_params(0, np.random.RandomState(0))
    assert tuple(empty[0].shape) == (0,) and tuple(empty[1].shape) == (0, 2)


def test_evaluation_draws_depend_on_seed_and_sample_alone():
    labels, fog = D.fixed_haze_params(7, range(10))
    again = D.fixed_haze_params(7, range(10))
    assert torch.equal(labels, again[0]) and torch.equal(fog, again[1])
    for world in (2, 3):                                              # a shard draws what the whole split draws for its samples
        for rank in range(world):
            own = list(range(rank, 10, world))
            l, f = D.fixed_haze_params(7, own)
            assert torch.equal(l, labels[own]) and torch.equal(f, fog[own])
    l, f = D.fixed_haze_params(7, [9, 0])
    assert torch.equal(l, labels[[9, 0]]) and torch.equal(f, fog[[9, 0]])
    assert not torch.equal(D.fixed_haze_params(8, range(10))[1], fog)
    for n in range(10):
        (b0, b1), (a0, a1) = D.FOG_RANGES[D.LEVEL_NAMES[int(labels[n])]]
        assert np.float32(b0) <= fog[n, 0] <= np.float32(b1) and np.float32(a0) <= fog[n, 1] <= np.float32(a1)


# ------------------------------------------------------------------------------------------------ files
def test_haze_index_pairs_and_refuses(tmp_path):
    from PIL import Image
    root = str(tmp_path / "data")
    listing = Z.write_tree(root)
    for split in ("train", "val"):
        idx = D.haze_index(root, split)
        assert [r["name"] for r in idx] == listing[split] == sorted(listing[split])
        assert idx.split_dir == os.path.join(root, split)
        for r in idx:
            assert r["clear"] == os.path.join(root, split, "clear", r["name"])
            assert r["depth"] == os.path.join(root, split, "depth", os.path.splitext(r["name"])[0] + ".png")
    assert any(n.endswith(".jpg") for n in listing["train"])
    assert [r["depth"] for r in D.haze_index(root, "train", "radial")] == [None] * len(listing["train"])
    assert D.haze_index(root, "test") is None and D.haze_index("", "train") is None
    assert D.haze_index(str(tmp_path / "nowhere"), "train") is None
    # <root>/clear itself serves when there is no <root>/<split>/clear; other files are not listed
    flat = os.path.join(root, "train")
    open(os.path.join(flat, "clear", "notes.txt"), "w").close()
    Image.fromarray(np.zeros((4, 4, 3), np.uint8)).save(os.path.join(flat, "clear", "upper.PNG"), format="PNG")
    assert [r["name"] for r in D.haze_index(flat, "val", "radial")] == listing["train"] and D.haze_index(flat, "val").split_dir == flat
    with pytest.raises(ValueError, match="folder.*radial"):
        D.haze_index(root, "train", "estimated")
    # a missing depth file, and one of another size, are named
    gone = os.path.join(root, "val", "depth", os.path.splitext(listing["val"][1])[0] + ".png")
    os.remove(gone)
    with pytest.raises(FileNotFoundError) as e:
        D.haze_index(root, "val")
    assert gone in str(e.value)
    assert len(D.haze_index(root, "val", "radial")) == len(listing["val"])
    Image.fromarray(np.zeros((9, 11), np.uint16)).save(gone)
    with pytest.raises(ValueError) as e:
        D.haze_index(root, "val")
    assert gone in str(e.value) and "9x11" in str(e.value) and os.path.join(root, "val", "clear", listing["val"][1]) in str(e.value)


def test_load_depth(tmp_path):
    from PIL import Image
    rng = np.random.RandomState(2)
    a16 = rng.randint(0, 65536, size=(5, 7)).astype(np.uint16)
    a16[0, :2] = (0, 65535)
    a8 = rng.randint(0, 256, size=(5, 7)).astype(np.uint8)
    a8[0, :2] = (0, 255)
    Image.fromarray(a16).save(tmp_path / "d16.png")
    Image.fromarray(a8).save(tmp_path / "d8.png")
    Image.fromarray(rng.randint(0, 256, size=(5, 7, 3)).astype(np.uint8)).save(tmp_path / "rgb.png")
    Image.fromarray(rng.rand(5, 7).astype(np.float32)).save(tmp_path / "f.tiff")
    d = IO.load_depth(str(tmp_path / "d16.png"))
    assert d.dtype == torch.uint16 and tuple(d.shape) == (5, 7) and not d.is_cuda and np.array_equal(d.numpy(), a16)
    assert np.array_equal(IO.load_depth(str(tmp_path / "d16.png"), raw=True).numpy(), a16)
    d = IO.load_depth(str(tmp_path / "d8.png"))
    assert d.dtype == torch.uint16 and np.array_equal(d.numpy(), a8.astype(np.uint16) * 257)
    assert np.array_equal(d.numpy().astype(np.float64) / 65535, a8 / 255.0)
    raw = IO.load_depth(str(tmp_path / "d8.png"), raw=True)
    assert raw.dtype == torch.uint8 and np.array_equal(raw.numpy(), a8)
    for name in ("rgb.png", "f.tiff"):
        with pytest.raises(ValueError) as e:
            IO.load_depth(str(tmp_path / name))
        assert str(tmp_path / name) in str(e.value)
    with pytest.raises(Exception):
        IO.load_depth(str(tmp_path / "missing.png"))


# ------------------------------------------------------------------------------------------------ refusals on the host
def test_batch_haze_from_windows_refuses_on_the_host():
    """CPU caches: every refusal that concerns the windows comes before the one that asks for a device"""
    CH, CW = 4, 6
    clear = torch.zeros(2 * 5 * 8 * 3, dtype=torch.uint8)            # two 5 x 8 images
    depth = torch.zeros(2 * 5 * 8, dtype=torch.uint16)
    fog = torch.tensor([[0.5, 0.8]] * 2)
    good = torch.tensor([[0, 24, 0, 16], [120 + 24 + 6, 24, 80 + 16 + 4, 16]], dtype=torch.int64)     # the second ends both caches

    def call(geom=good, c=clear, d=depth, f=fog, crop=(CH, CW), params=None, **kw):
        return D.batch_haze_from_windows(c, d, geom, f, crop, params, **kw)
    for geom in (good.to(torch.int32), good[:, :2].contiguous(), good[0], good.tolist(), good.numpy()):
        with pytest.raises(TypeError):
            call(geom)
    with pytest.raises(TypeError):
        call(c=clear.numpy())
    for bad in ([0, 24, 1, 16], [0, 24, 0, 15], [0, 24, 0, 10], [0, 24, 2, 17]):      # odd offset, odd pitch, pitch < CW * 2
        with pytest.raises(ValueError, match="even"):
            call(torch.tensor([bad, good[1].tolist()], dtype=torch.int64))
    for bad in ([-3, 24, 0, 16], [0, 17, 0, 16], [153, 24, 0, 16], [150, 27, 0, 16], [2 ** 62, 2 ** 62, 0, 16]):
        with pytest.raises(IndexError, match="clear cache of 240 bytes"):
            call(torch.tensor([good[0].tolist(), bad], dtype=torch.int64))
    for bad in ([0, 24, -2, 16], [0, 24, 102, 16], [0, 24, 100, 18], [0, 24, 2 ** 62, 2 ** 62]):
        with pytest.raises(IndexError, match="depth cache of 160 bytes"):
            call(torch.tensor([good[0].tolist(), bad], dtype=torch.int64))
    with pytest.raises(IndexError):                                  # without a depth cache the last two columns are not read
        call(torch.tensor([[153, 24, 1, 1]], dtype=torch.int64), d=None, f=fog[:1])
    for kw in (dict(crop=(0, 6)), dict(crop=(4, 0)), dict(geom=good[:0]), dict(f=fog[:1]), dict(f=fog.reshape(4)),
               dict(params=torch.zeros(2, 4)), dict(params=torch.zeros(3, 5)), dict(depth_range=(0.3, float("inf")))):
        with pytest.raises(ValueError):
            call(**kw)
    # only now the device: a valid request on CPU caches names what is missing, with and without a depth cache
    for d in (depth, None):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call(d=d)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        call(torch.tensor([[0, 24, 1, 1]], dtype=torch.int64), d=None, f=fog[:1])


def test_synthetic_haze_config_refusals(tmp_path):
    root = str(tmp_path / "data")
    Z.write_tree(root, splits=(("train", 2),))
    cfg = {"seed": 1, "dataset": {"train_path": root, "val_path": root, "img_size": 32, "batch_size": 2, "synthetic_haze": {}}}
    with pytest.raises(RuntimeError, match="no clear/ folder.*not substituted"):     # val has no clear/: no noise frames instead
        D.folder_loader(cfg, "val", "cuda:0")
    cfg["dataset"]["val_path"] = None
    with pytest.raises(RuntimeError, match="no clear/ folder"):
        D.folder_loader(cfg, "val", "cuda:0")
    for bad, err in (({"depth": "estimated"}, "folder.*radial"), ({"depths": "folder"}, "unknown keys"),
                     ({"depth_range": [0.3]}, "near, far"), ({"depth_range": 1.0}, "near, far")):
        cfg["dataset"]["synthetic_haze"] = bad
        with pytest.raises(ValueError, match=err):
            D.folder_loader(cfg, "train", "cuda:0")
    # without the key, or with anything that is no mapping, the stored-pair path answers as before: no level folders, so None
    for off in (None, False):
        cfg["dataset"]["synthetic_haze"] = off
        assert D.folder_loader(cfg, "train", "cuda:0") is None
    del cfg["dataset"]["synthetic_haze"]
    assert D.folder_loader(cfg, "train", "cuda:0") is None
    with pytest.raises(RuntimeError, match="no CPU fallback"):       # the cache class itself asks for a device
        D.HazeSynthDataset(D.haze_index(root, "train"), 32, "cpu")
