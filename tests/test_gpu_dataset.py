"""csrc/dataset.hip and the image-folder loader on the GPU: the resize and the batch assembly against the float64 references of
tests/_dataset_ref64.py, and the drivers end to end on a small tree of PNG / JPG files written with Pillow from a seed."""
import collections
import itertools
import os
import warnings

import numpy as np
import pytest
import torch

from adam_dehaze_amd import _hip as H
from adam_dehaze_amd import data as D
from adam_dehaze_amd import image_io as IO
from adam_dehaze_amd import train as T
from tests import _dataset_ref64 as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FILL = 0x5A


def _bits(t):
    return t.contiguous().view(torch.int32)


# ------------------------------------------------------------------------------------------------ resize
def _resize(u8, OH, OW, slack, off):
    """adh_u8_resize_bilinear on a source with `slack` bytes of pitch padding, `off` bytes into its buffer; the destination has
    64 guard bytes behind it"""
    h, w, C = u8.shape
    rp = w * C + slack
    host = torch.full((off + h * rp + 64,), FILL, dtype=torch.uint8)
    torch.as_strided(host, (h, w * C), (rp, 1), off).copy_(torch.from_numpy(u8).reshape(h, w * C))
    buf = host.to(DEV)
    dst = torch.full((OH * OW * 3 + 64,), FILL, dtype=torch.uint8, device=DEV)
    H.call("adh_u8_resize_bilinear", buf.data_ptr() + off, rp, h, w, C, dst.data_ptr(), OH, OW)
    dst = dst.cpu()
    assert torch.equal(buf.cpu(), host), "the source was written"
    assert (dst[OH * OW * 3:] == FILL).all(), "bytes behind the destination were written"
    return dst[:OH * OW * 3].view(OH, OW, 3).numpy()


@pytest.mark.parametrize("C", [1, 3, 4])
@pytest.mark.parametrize("case", R.RESIZE_CASES)
def test_resize_against_float64(case, C):
    """Bytes equal the float64 reference everywhere, except +-1 where the float64 value lies within delta of a half-integer:
    delta = 2 * 255 * ds + 8 * 255 * 2^-24 with ds the fp32 coordinate error of both axes (tests/_pointwise_ref64.src_err) and
    eight value roundings (counted in tests/_dataset_ref64.resize_delta); such near-ties are at most 5 % of a case."""
    (h, w), (OH, OW) = case
    u8 = np.random.RandomState(h * 100 + w + C).randint(0, 256, size=(h, w, C)).astype(np.uint8)
    R.check_resize(_resize(u8, OH, OW, slack=5, off=3), u8, OH, OW, what=f"C={C} padded")
    R.check_resize(_resize(u8, OH, OW, slack=0, off=0), u8, OH, OW, what=f"C={C} dense")


@pytest.mark.parametrize("C", [1, 3, 4])
@pytest.mark.parametrize("case", R.RESIZE_DYADIC + [((32, 32), (32, 32)), ((17, 67), (17, 67))])
def test_resize_exact_ratios_and_same_size(case, C):
    """2:1, 4:1 and 5:4: coordinates and weights are exact in fp32 and the sums of bytes times dyadic weights too, so the bytes
    are equal with no exception, including the exact ties of 2:1 (half to even).  Same size: the bytes pass through."""
    (h, w), (OH, OW) = case
    u8 = np.random.RandomState(h + w + C).randint(0, 256, size=(h, w, C)).astype(np.uint8)
    got = _resize(u8, OH, OW, slack=3, off=1)
    R.check_resize(got, u8, OH, OW, exact=True, what=f"C={C}")
    if (h, w) == (OH, OW):
        assert np.array_equal(got, R.rgb3(u8))
    if (h, w) == (64, 64):
        val = R.resize_values(u8, OH, OW)
        assert (np.abs(val - np.floor(val) - 0.5) == 0).mean() > 0.15          # the exact ties are there


# ------------------------------------------------------------------------------------------------ batch assembly
ROWS = [[fh, fv, bf, b, c] for fh, fv, bf, b, c in itertools.product((0, 1), (0, 1), (0, 1), (0.9, 1.0, 1.1), (0.9, 1.0, 1.1))]
INDEX3 = [[4, 0, 4], [3, 1, 2], [2, 2, 0], [1, 4, 3]]             # repeated and out of order; 3 = all 0, 4 = all 255


@pytest.mark.parametrize("HW", [(1, 1), (3, 5), (16, 16), (17, 67), (64, 64), (65, 64)])
def test_batch_against_float64(HW):
    """N = 3 over all 72 parameter rows, N = 1 for a few.  With jitter within 8 * 2^-24 of float64 (the roundings are counted at
    tests/_dataset_ref64.BATCH_BOUND) and within twice that of paired_augment(u8_to_image(cache[index])); rows with
    b = c = 1, and params=None, bit-equal to u8_to_image of the flipped bytes; a second call and sample n alone bit-equal."""
    Hh, Ww = HW
    host = R.all_values_cache(5, Hh, Ww, seed=Hh * 131 + Ww)
    cache = torch.from_numpy(host).to(DEV)
    planes = IO.u8_to_image(cache)                                    # [5,3,H,W], exact v / 255
    worst = worst_c = 0.0
    for k in range(0, len(ROWS), 3):
        index = INDEX3[(k // 3) % len(INDEX3)]
        params = torch.tensor(ROWS[k:k + 3], dtype=torch.float32)
        idx = torch.tensor(index, dtype=torch.int64)
        got = D.batch_from_cache(cache, idx, params)
        assert tuple(got.shape) == (3, 3, Hh, Ww) and got.dtype == torch.float32 and got.device == cache.device
        ref = torch.from_numpy(R.batch_ref(host, index, params.numpy()))
        worst = max(worst, float((got.cpu().double() - ref).abs().max()))
        (comp,), _ = D.paired_augment([planes[idx.to(DEV)].contiguous()], params)
        worst_c = max(worst_c, float((got.double() - comp.double()).abs().max()))
        for n, row in enumerate(ROWS[k:k + 3]):
            if row[3] == 1.0 and row[4] == 1.0:
                want = planes[index[n]]
                want = torch.flip(want, dims=[2]) if row[0] else want
                want = torch.flip(want, dims=[1]) if row[1] else want
                assert torch.equal(_bits(got[n]), _bits(want)), (index, row)
        if k % 9 == 0:
            assert torch.equal(_bits(D.batch_from_cache(cache, idx, params)), _bits(got))
            for n in range(3):
                alone = D.batch_from_cache(cache, idx[n:n + 1], params[n:n + 1])
                assert torch.equal(_bits(alone[0]), _bits(got[n])), (index, n)
    print(f"batch {Hh}x{Ww}: max |err| vs float64 {worst / R.EPS:.3f} * 2^-24 (bound 8), vs the composition "
          f"{worst_c / R.EPS:.3f} * 2^-24 (bound 16)")
    assert worst <= R.BATCH_BOUND and worst_c <= 2 * R.BATCH_BOUND
    idx = torch.tensor([3, 0, 4, 4, 1], dtype=torch.int64)
    plain = D.batch_from_cache(cache, idx)
    assert torch.equal(_bits(plain), _bits(planes[idx.to(DEV)]))
    assert torch.equal(_bits(D.batch_from_cache(cache, idx[1:2])), _bits(planes[0:1]))
    other = torch.flip(cache, dims=[0]).contiguous()                  # a pair of caches: one index, one set of rows
    params = torch.tensor(ROWS[13:18], dtype=torch.float32)
    a, b = D.batch_from_cache((cache, other), idx, params)
    assert torch.equal(_bits(a), _bits(D.batch_from_cache(cache, idx, params)))
    assert torch.equal(_bits(b), _bits(D.batch_from_cache(other, idx, params)))
    assert torch.equal(cache.cpu(), torch.from_numpy(host)), "the cache was written"


@pytest.mark.parametrize("HW", [(3, 5), (16, 16), (65, 64)])
def test_batch_unaligned_buffers_and_guard_bytes(HW):
    """the C entry point on a cache at an odd byte address with a padded image pitch and an output off 16-byte alignment (the
    byte and single-float paths): the same bits as the aligned call, nothing written behind N * 3 * H * W floats"""
    Hh, Ww = HW
    M, N, px = 5, 3, Hh * Ww
    host = R.all_values_cache(M, Hh, Ww, seed=7)
    pitch = px * 3 + 7
    raw = torch.full((1 + M * pitch,), FILL, dtype=torch.uint8)
    torch.as_strided(raw, (M, px * 3), (pitch, 1), 1).copy_(torch.from_numpy(host).reshape(M, -1))
    dev_raw = raw.to(DEV)
    index = torch.tensor([4, 1, 1], dtype=torch.int64)
    params = torch.tensor([[1, 0, 1, 0.9, 1.1], [0, 1, 0, 1.1, 0.9], [1, 1, 1, 1.1, 1.1]], dtype=torch.float32)
    want = D.batch_from_cache(torch.from_numpy(host).to(DEV), index, params)
    nblk = H.value("adh_batch_num_blocks", px)
    assert nblk == max(1, -(-px // 4096))
    sentinel = float(np.float32(-1234.5))
    index_dev, params_dev = index.to(DEV), params.to(DEV)             # held: a temporary's block would be handed out again
    for use_params in (True, False):
        out = torch.full((1 + N * 3 * px + 64,), sentinel, dtype=torch.float32, device=DEV)
        partial = torch.zeros(N * nblk, dtype=torch.float64, device=DEV)
        H.call("adh_batch_from_u8", dev_raw.data_ptr() + 1, pitch, M, Hh, Ww, index_dev.data_ptr(),
               params_dev.data_ptr() if use_params else None, N, partial.data_ptr(), nblk, out.data_ptr() + 4)
        got = out[1:1 + N * 3 * px].view(N, 3, Hh, Ww)
        if use_params:
            assert torch.equal(_bits(got), _bits(want))
        else:
            assert torch.equal(_bits(got), _bits(D.batch_from_cache(torch.from_numpy(host).to(DEV), index)))
        assert float(out[0]) == sentinel and (out[1 + N * 3 * px:] == sentinel).all()
    assert torch.equal(dev_raw.cpu(), raw), "the cache or its padding was written"


def test_batch_refusals():
    cache = torch.zeros((2, 4, 4, 3), dtype=torch.uint8, device=DEV)
    with pytest.raises(IndexError):
        D.batch_from_cache(cache, torch.tensor([0, 2], dtype=torch.int64))
    with pytest.raises(TypeError):
        D.batch_from_cache(cache, torch.tensor([0], dtype=torch.int64, device=DEV))       # no device index
    idx, out = torch.zeros(1, dtype=torch.int64, device=DEV), torch.zeros(48, device=DEV)
    with pytest.raises(RuntimeError, match="ADH_E_ARG"):
        H.call("adh_batch_from_u8", cache.data_ptr(), 47, 2, 4, 4, idx.data_ptr(), None, 1, None, 1, out.data_ptr())
    with pytest.raises(RuntimeError, match="ADH_E_ARG"):
        H.call("adh_batch_from_u8", cache.data_ptr(), 48, 2, 4, 4, idx.data_ptr(), None, 1, None, 2, out.data_ptr())
    with pytest.raises(RuntimeError, match="ADH_E_ARG"):
        H.call("adh_u8_resize_bilinear", cache.data_ptr(), 11, 4, 4, 3, out.data_ptr(), 2, 2)


# ------------------------------------------------------------------------------------------------ end to end
@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    """train / val / test with 4 / 2 / 2 files per level; the caches start empty and every folder_index call is counted"""
    root = str(tmp_path_factory.mktemp("folders"))
    listing = R.write_tree(root)
    counts = collections.Counter()
    real_index, real_caches = D.folder_index, D._CACHES

    def counting(r, split):
        counts[split] += 1
        return real_index(r, split)
    counting.uncounted = real_index
    D.folder_index, D._CACHES = counting, {}
    yield root, listing, counts
    D.folder_index, D._CACHES = real_index, real_caches


def _cfg(root, tmp_path):
    from tests.test_gpu_train import _cfg as base
    cfg = base()
    cfg["dataset"].update(train_path=root, val_path=root, test_path=root, num_workers=3)
    cfg["dehazing"]["checkpoint_dir"] = str(tmp_path / "dehazing")
    cfg["joint_training"]["checkpoint_dir"] = str(tmp_path / "joint")
    cfg["evaluation"] = {"results_dir": str(tmp_path / "results")}
    return cfg


def _file_u8(root, split, level, role, name):
    return IO.load_image(os.path.join(root, split, level, role, name)).numpy()


def test_val_split_batches(tree, tmp_path):
    root, listing, counts = tree
    cfg = _cfg(root, tmp_path)
    loader = D.folder_loader(cfg, "val", DEV)
    batches = list(loader(0))
    assert [len(b["name"]) for b in batches] == [4, 2]                # 6 files, batch size 4, the last batch short
    seen = []
    for b in batches:
        n = len(b["name"])
        assert set(b) == {"hazy", "clear", "intensity", "name"}
        for k in ("hazy", "clear"):
            assert tuple(b[k].shape) == (n, 3, 32, 32) and b[k].dtype == torch.float32 and str(b[k].device) == DEV
        assert b["intensity"].dtype == torch.int64 and str(b["intensity"].device) == DEV and tuple(b["intensity"].shape) == (n,)
        for i, name in enumerate(b["name"]):
            level = D.LEVEL_NAMES[int(b["intensity"][i])]
            seen.append((level, name))
            for role in ("hazy", "clear"):
                x = b[role][i].cpu()
                u8 = (x * 255).round().to(torch.uint8)
                assert torch.equal(_bits(x), _bits(u8.float() / 255))                  # exact v / 255
                src = _file_u8(root, "val", level, role, name)
                R.check_resize(u8.permute(1, 2, 0).numpy(), src, 32, 32, exact=src.shape[:2] == (32, 32),
                               what=f"{level}/{role}/{name} C={src.shape[2]}")
    assert seen == listing["val"]                                     # index order, each file once
    assert [tuple(x.shape) for x in (list(loader(1))[0]["hazy"],)] == [(4, 3, 32, 32)]
    assert counts["val"] == 1 and D.folder_loader(cfg, "val", "cuda") is not None and counts["val"] == 1
    train = [b for b in D.folder_loader(cfg, "train", DEV)(0)]
    assert sorted(n for b in train for n in b["name"]) == sorted(n for _, n in listing["train"])
    assert [b["name"] for b in D.folder_loader(cfg, "train", DEV)(0)] == [b["name"] for b in train]
    assert [b["name"] for b in D.folder_loader(cfg, "train", DEV)(1)] != [b["name"] for b in train]


def test_shards_bad_files_and_the_memory_limit(tree, tmp_path, monkeypatch, capsys):
    root, listing, _ = tree
    records = D.folder_index.uncounted(root, "train")               # the drivers' reads are counted, this one is the test's
    shard =D.FolderDataset(records, [32, 32], DEV, rank=1, world=2, threads=64, split="train")
    out = capsys.readouterr().out
    assert "Loaded 12 samples for train split" in out and "skipped 0 hazy files" in out and "6 pairs at 32x32" in out
    own = [r["name"] for r in records[1::2]]
    assert shard.names == own and tuple(shard.hazy.shape) == (6, 32, 32, 3) and shard.labels.tolist() == \
        [r["intensity"] for r in records[1::2]]
    train = list(shard.epoch(0, 4, 42, train=True))
    assert [len(b["name"]) for b in train] == [4, 2] and sorted(n for b in train for n in b["name"]) == sorted(own)
    val = list(shard.epoch(0, 4, 42, train=False))
    assert [n for b in val for n in b["name"]] == own
    whole = D.FolderDataset(records, 32, DEV, split="train")
    for b in val:                                                     # a shard holds the bytes the whole cache holds
        for i, name in enumerate(b["name"]):
            k = whole.names.index(name)
            assert torch.equal(b["hazy"][i], D.batch_from_cache(whole.hazy, torch.tensor([k]))[0])
            assert int(b["intensity"][i]) == int(whole.labels[k])
    bad = [dict(records[0])]
    bad[0]["clear"] = str(tmp_path / "broken.png")
    (tmp_path / "broken.png").write_bytes(b"not an image")
    with pytest.raises(RuntimeError, match="broken.png"):
        D.FolderDataset(bad, 32, DEV)
    monkeypatch.setattr(torch.cuda, "mem_get_info", lambda *a, **k: (2 * 12 * 32 * 32 * 3 * 2 - 2, 1 << 40))
    with pytest.raises(RuntimeError, match="streaming loader is not built"):
        D.FolderDataset(records, 32, DEV)


def _no_synthetic(caught):
    assert not [str(w.message) for w in caught if "SYNTHETIC" in str(w.message)]


def test_branch_stage_trains_on_the_folders(tree, tmp_path, monkeypatch, capsys):
    root, listing, counts = tree
    cfg = _cfg(root, tmp_path)
    vals = []
    real = T.validate_dehazing
    monkeypatch.setattr(T, "validate_dehazing", lambda *a, **k: vals.append(real(*a, **k)) or vals[-1])
    torch.manual_seed(3)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        model, losses = T.train_dehazing_model(cfg, "low", epochs=1)
    _no_synthetic(caught)
    assert 1 <= len(losses) <= 3 and all(np.isfinite(l) for l in losses)           # 12 train files in 3 batches, low ones only
    assert len(vals) == 1 and vals[0]["val_samples"] == sum(level == "low" for level, _ in listing["val"]) == 2
    assert np.isfinite(vals[0]["val_loss"])
    out = capsys.readouterr().out
    assert counts["train"] == 1 and counts["val"] == 1 and counts["test"] <= 1
    assert "samples for train split" not in out or "Loaded 12 samples for train split" in out


def test_joint_stage_and_evaluation_on_the_folders(tree, tmp_path):
    root, listing, counts = tree
    cfg = _cfg(root, tmp_path)
    torch.manual_seed(5)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        system, hist = T.train_joint_model(cfg, epochs=1)
        res = T.evaluate_joint_model(cfg, use_lpips=False)
    _no_synthetic(caught)
    assert len(hist) == 1 and hist[0]["val_samples"] == len(listing["val"]) == 6
    assert all(np.isfinite(hist[0][k]) for k in ("train_loss", "val_loss", "val_psnr", "val_ssim"))
    assert {k: v["samples"] for k, v in res.items()} == {"low_intensity": 2, "medium_intensity": 2, "high_intensity": 2}
    assert counts["train"] == 1 and counts["val"] == 1 and counts["test"] == 1     # once per split per process
