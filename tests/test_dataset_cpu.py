"""The host side of the image-folder loader, without a GPU: the folder index, the epoch plan, the float64 references of
tests/_dataset_ref64.py against torch, the unchanged synthetic fallback of the drivers, and the host-side index check."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from adam_dehaze_amd import data as D
from adam_dehaze_amd import train as T
from tests import _dataset_ref64 as R


# ------------------------------------------------------------------------------------------------ index
def test_index_layout_order_labels_and_skips(tmp_path):
    root = str(tmp_path / "ds")
    listing = R.write_tree(root, splits=(("train", 4),))
    base = os.path.join(root, "train")
    from PIL import Image
    im = Image.fromarray(np.zeros((8, 8, 3), np.uint8))
    for name in ("upper.JPG", "long.jpeg", "notes.txt"):              # the extension rule is the reference's, case-sensitive
        im.save(os.path.join(base, "low", "hazy", name), format="PNG")
        im.save(os.path.join(base, "low", "clear", name), format="PNG")
    im.save(os.path.join(base, "medium", "hazy", "aa_orphan.png"))    # no clear file: skipped and counted
    im.save(os.path.join(base, "high", "hazy", "zz_orphan.jpg"))
    os.makedirs(os.path.join(base, "low", "dehazed"))                  # neither required nor read
    idx = D.folder_index(root, "train")
    assert [(D.LEVEL_NAMES[r["intensity"]], r["name"]) for r in idx] == listing["train"]
    assert idx.skipped == 2 and len(idx) == 12
    for r in idx:
        level = D.LEVEL_NAMES[r["intensity"]]
        assert r["hazy"] == os.path.join(base, level, "hazy", r["name"])
        assert r["clear"] == os.path.join(base, level, "clear", r["name"])
    for level in range(3):                                             # each level's names are sorted
        names = [r["name"] for r in idx if r["intensity"] == level]
        assert names == sorted(names) and len(names) == 4
    assert [r["intensity"] for r in idx] == sorted(r["intensity"] for r in idx)


def test_index_root_fallback_and_none(tmp_path):
    root = str(tmp_path / "flat")
    listing = R.write_tree(root, splits=(("val", 2),), sub_split=False)      # <root>/{low,...}: what --data_dir D/val holds
    idx = D.folder_index(root, "val")
    assert [(D.LEVEL_NAMES[r["intensity"]], r["name"]) for r in idx] == listing["val"]
    assert idx.split_dir == root and idx.skipped == 0
    nested = str(tmp_path / "nested")
    R.write_tree(nested, splits=(("val", 2),))
    assert D.folder_index(nested, "val").split_dir == os.path.join(nested, "val")
    assert D.folder_index(nested, "test") is None                     # no test split, and <root> itself holds no level
    only_ann = tmp_path / "ann"
    (only_ann / "annotations").mkdir(parents=True)
    assert D.folder_index(str(only_ann), "test") is None
    assert D.folder_index(str(tmp_path / "missing"), "train") is None
    assert D.folder_index("", "train") is None and D.folder_index(None, "train") is None
    assert D.folder_loader({"dataset": {"test_path": str(only_ann)}}, "test", "cpu") is None


# ------------------------------------------------------------------------------------------------ plan
@pytest.mark.parametrize("M,world,bs", [(10, 3, 2), (7, 2, 4)])
def test_epoch_plan(M, world, bs):
    per_rank = -(-M // world)
    plans = [D.epoch_plan(M, world, r, bs, seed=42, epoch=3, train=True) for r in range(world)]
    assert {len(p) for p in plans} == {-(-per_rank // bs)}            # every rank steps equally often
    seen = set()
    for r, p in enumerate(plans):
        flat = np.concatenate(p)
        assert flat.dtype == np.int64 and flat.size == per_rank
        assert all(b.size == bs for b in p[:-1]) and 1 <= p[-1].size <= bs
        own = set(range(r, M, world))
        assert set(flat.tolist()) == own                              # every own sample, padded by own samples only
        seen |= own
    assert seen == set(range(M))
    again = [D.epoch_plan(M, world, r, bs, seed=42, epoch=3, train=True) for r in range(world)]
    assert all(np.array_equal(a, b) for p, q in zip(plans, again) for a, b in zip(p, q))
    other = np.concatenate(D.epoch_plan(M, world, 0, bs, seed=42, epoch=4, train=True))
    assert not np.array_equal(other, np.concatenate(plans[0]))
    evals = [np.concatenate(D.epoch_plan(M, world, r, bs, seed=42, epoch=0, train=False)) for r in range(world)]
    allv = np.concatenate(evals)
    assert sorted(allv.tolist()) == list(range(M))                    # disjoint, complete, nothing repeats
    for r, e in enumerate(evals):
        assert e.tolist() == list(range(r, M, world))                 # index order


def test_epoch_plan_edges():
    assert [b.tolist() for b in D.epoch_plan(2, 4, 3, 2, 0, 0, train=False)] == []      # a rank with nothing to evaluate
    with pytest.raises(ValueError):
        D.epoch_plan(2, 4, 3, 2, 0, 0, train=True)                                        # ... cannot train
    with pytest.raises(ValueError):
        D.epoch_plan(4, 2, 2, 2, 0, 0, train=True)


# ------------------------------------------------------------------------------------------------ the references themselves
@pytest.mark.parametrize("case", R.RESIZE_CASES + R.RESIZE_DYADIC)
@pytest.mark.parametrize("C", [1, 3, 4])
def test_resize_reference_against_torch(case, C):
    (h, w), (OH, OW) = case
    u8 = np.random.RandomState(h * 100 + w + C).randint(0, 256, size=(h, w, C)).astype(np.uint8)
    x = torch.from_numpy(R.rgb3(u8).astype(np.float64)).permute(2, 0, 1)[None]
    want = F.interpolate(x, size=(OH, OW), mode="bilinear", align_corners=False)[0].permute(1, 2, 0).numpy()
    got = R.resize_values(u8, OH, OW)
    assert got.shape == (OH, OW, 3) and np.abs(got - want).max() <= 1e-9
    if (OH, OW) == (h, w):
        assert np.array_equal(R.resize_bytes(got), R.rgb3(u8))


def test_resize_reference_same_size_and_half_even():
    u8 = np.random.RandomState(1).randint(0, 256, size=(9, 7, 3)).astype(np.uint8)
    assert np.array_equal(R.resize_bytes(R.resize_values(u8, 9, 7)), u8)
    two = np.array([[[0], [1]], [[0], [3]]], np.uint8)                # rows (0, 1), (0, 3): the 2:1 centre is their mean
    assert R.resize_values(two, 1, 1)[0, 0, 0] == 1.0
    assert R.resize_bytes(np.array([0.5, 1.5, 2.5, 254.5, 300.0, -3.0])).tolist() == [0, 2, 2, 254, 255, 0]
    near = R.resize_delta(40, 56, 32, 32)
    assert 0 < near < 1e-2                                            # a near-tie is a narrow band, not a licence


def _torch_batch(cache, index, params):
    out = []
    for n, i in enumerate(index):
        x = torch.from_numpy(cache[i]).double().permute(2, 0, 1) / 255
        if params is not None:
            fh, fv, bfirst, b, c = params[n].double().tolist()
            if fh:
                x = torch.flip(x, dims=[2])
            if fv:
                x = torch.flip(x, dims=[1])
            for step in ((0, 1) if bfirst else (1, 0)):
                if step == 0:
                    x = (b * x).clamp(0, 1)
                else:
                    gray = (0.2989 * x[0] + 0.587 * x[1] + 0.114 * x[2]).mean()
                    x = (c * x + (1 - c) * gray).clamp(0, 1)
        out.append(x)
    return torch.stack(out).numpy()


def test_batch_reference_against_torch():
    cache = R.all_values_cache(5, 6, 7, seed=3)
    assert set(np.unique(cache)) == set(range(256)) and (cache[3] == 0).all() and (cache[4] == 255).all()
    index = [4, 0, 0, 3, 2, 1, 1, 2]
    rows = [[fh, fv, bf, b, c] for (fh, fv), bf, (b, c) in zip([(0, 0), (1, 0), (0, 1), (1, 1)] * 2, [0, 1] * 4,
                                                                 [(0.9, 1.1), (1.1, 0.9), (1.0, 1.0), (1.1, 1.1)] * 2)]
    params = torch.tensor(rows, dtype=torch.float32)
    got = R.batch_ref(cache, index, params.numpy())
    assert np.abs(got - _torch_batch(cache, index, params)).max() <= 1e-15
    plain = R.batch_ref(cache, index)
    assert np.array_equal(plain, _torch_batch(cache, index, None))
    ident = torch.tensor([[1, 1, 0, 1, 1]] * len(index), dtype=torch.float32)
    assert np.array_equal(R.batch_ref(cache, index, ident.numpy()), plain[:, :, ::-1, ::-1])
    ends = R.batch_ref(cache, [4, 3], np.array([[0, 0, 1, 1.1, 1.1], [0, 0, 0, 0.9, 0.9]], np.float32))
    assert (ends[0] == 1.0).all() and (ends[1] == 0.0).all()         # the upper clamp engages on the all-255 image


# ------------------------------------------------------------------------------------------------ fallback and host checks
@pytest.mark.parametrize("paths", ["unset", "empty", "no_folders"])
def test_fallback_stays_synthetic(paths, tmp_path, monkeypatch):
    ds = {"batch_size": 2, "img_size": 16}
    if paths == "empty":
        ds.update(train_path="", val_path="", test_path="")
    elif paths == "no_folders":
        (tmp_path / "annotations").mkdir()
        ds.update(train_path=str(tmp_path), val_path=str(tmp_path / "nowhere"), test_path=str(tmp_path))
    cfg = {"seed": 1, "device": "cpu", "dataset": ds}
    calls = []

    def stub(batch_size, size, steps, seed=42, rank=0, device=None, augment=False):
        calls.append((batch_size, size, steps, seed))
        return iter([{"synthetic": True}] * steps)
    monkeypatch.setattr(T, "synthetic_loader", stub)
    monkeypatch.setattr(D, "FolderDataset", lambda *a, **k: pytest.fail("no cache may be built"))
    for split, offset in (("train", 0), ("val", 500000), ("test", 900000)):
        with pytest.warns(UserWarning, match="SYNTHETIC"):
            got = list(T._loader_or_synthetic(None, cfg, 3, offset, "cpu", epoch=2, warn="driver", split=split))
        assert got == [{"synthetic": True}] * 3
        assert calls[-1] == (2, 16, 3, 1 + offset + 2)
    assert T._uses_synthetic(cfg, "cpu", train=None, val=None)
    assert not T._uses_synthetic(cfg, "cpu", train=[1], val=[2])
    given = [{"mine": 1}]
    assert T._loader_or_synthetic(given, cfg, 3, 0, "cpu") is given                 # a supplied loader wins
    assert T._loader_or_synthetic(lambda e: [e], cfg, 3, 0, "cpu", epoch=5) == [5]


def test_index_is_checked_on_the_host_before_any_device():
    cache = torch.zeros((3, 4, 4, 3), dtype=torch.uint8)              # a CPU tensor: a passing check would fail on the device test
    for bad in ([3], [0, -1], [1, 2, 7]):
        with pytest.raises(IndexError):
            D.batch_from_cache(cache, torch.tensor(bad, dtype=torch.int64))
    with pytest.raises(TypeError):
        D.batch_from_cache(cache, torch.tensor([0], dtype=torch.int32))
    with pytest.raises(TypeError):
        D.batch_from_cache(cache, [0])
    with pytest.raises(RuntimeError, match="cuda"):                   # in range: the next check is the device's
        D.batch_from_cache(cache, torch.tensor([2, 0], dtype=torch.int64))
