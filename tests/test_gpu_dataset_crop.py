"""Crop training on the GPU: adh_batch_window_from_u8 over the table of tests/_dataset_window_cases.py (bit for bit
data.batch_from_cache on a dense copy of the windows, and the float64 reference of tests/_dataset_ref64.py), and
`dataset.crop_size` end to end on the tree of PNG / JPG files of tests/_dataset_ref64.write_tree: the loader, the upscale of
files smaller than the crop, and the drivers."""
import collections
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
from tests import _dataset_window_cases as K
from tests.test_gpu_dataset import _cfg as _folder_cfg
from tests.test_gpu_dataset import _no_synthetic

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FILL = 0x5A
SENTINEL = float(np.float32(-1234.5))
FRONT = 4                       # sentinel floats in front of the output: it starts 16-byte aligned, plus out_off floats


def _bits(t):
    return t.contiguous().view(torch.int32)


def _window_call(raw, base, nbytes, wd, pd, crop, out_off):
    """the C entry point on the cache `base` bytes into `raw`, its output FRONT + out_off floats into a buffer of sentinels with
    64 more behind; returns [N,3,CH,CW] after checking that the sentinels stand"""
    (CH, CW), N = crop, wd.shape[0]
    n, nblk = N * 3 * CH * CW, H.value("adh_batch_num_blocks", CH * CW)
    at = FRONT + out_off
    out = torch.full((at + n + 64,), SENTINEL, dtype=torch.float32, device=DEV)
    partial = torch.zeros(N * nblk, dtype=torch.float64, device=DEV)
    H.call("adh_batch_window_from_u8", raw.data_ptr() + base, nbytes, wd.data_ptr(), H.ptr(pd), N, CH, CW, partial.data_ptr(), nblk,
           out.data_ptr() + 4 * at)
    assert (out[:at] == SENTINEL).all() and (out[at + n:] == SENTINEL).all(), "a float outside the output was written"
    return out[at:at + n].view(N, 3, CH, CW)


# ------------------------------------------------------------------------------------------------ kernel
@pytest.mark.parametrize("no", range(len(K.CASES)), ids=[c["name"] for c in K.CASES])
def test_windows_against_the_dense_copy_and_float64(no):
    """Every case with and without parameter rows (all 72 rows over a case of three windows).  Bit-equal to batch_from_cache on
    the dense stack of the windows' bytes; within 8 * 2^-24 of float64 (tests/_dataset_ref64.BATCH_BOUND); rows with b = c = 1,
    and params=None, bit-equal to u8_to_image of the flipped bytes; a second call, each sample alone, a cache whose bytes
    outside the windows are all different, and both caches of a pair through one call: the same bits.  The cache is unchanged
    and the floats around the output are untouched."""
    case = K.CASES[no]
    flat, windows, dense = K.build(case)
    crop, base, out_off = case["crop"], case["base"], case["out_off"]
    N = len(windows)
    front = np.full(base, FILL, np.uint8)
    host = torch.from_numpy(np.concatenate([front, flat]))
    raw = host.to(DEV)
    other = np.where(K.window_mask(flat.size, windows, crop), flat, flat ^ 0xFF)         # every byte outside the windows differs
    raw_other = torch.from_numpy(np.concatenate([front, other])).to(DEV)
    dense_dev = torch.from_numpy(dense).to(DEV)
    planes = IO.u8_to_image(dense_dev)                               # [N,3,CH,CW], exact v / 255
    wd, idx, wt = torch.from_numpy(windows).to(DEV), torch.arange(N, dtype=torch.int64), torch.from_numpy(windows)
    worst = 0.0
    for k, params in enumerate([None] + K.param_sets(no, N, 1 if case["gpu_only"] else len(K.ROWS) // N)):
        pt = None if params is None else torch.from_numpy(params)
        pd = None if params is None else pt.to(DEV)
        got = _window_call(raw, base, flat.size, wd, pd, crop, out_off)
        assert torch.equal(_bits(got), _bits(D.batch_from_cache(dense_dev, idx, pt))), (case["name"], k, "differs from the dense copy")
        if params is None:
            assert torch.equal(_bits(got), _bits(planes))
        else:
            ref = torch.from_numpy(R.batch_ref(dense, np.arange(N), params))
            worst = max(worst, float((got.cpu().double() - ref).abs().max()))
            for n, row in enumerate(params.tolist()):
                if row[3] == 1.0 and row[4] == 1.0:
                    want = torch.flip(planes[n], dims=[2]) if row[0] else planes[n]
                    want = torch.flip(want, dims=[1]) if row[1] else want
                    assert torch.equal(_bits(got[n]), _bits(want)), (case["name"], row)
        if k % 8 > 1:
            continue
        assert torch.equal(_bits(_window_call(raw, base, flat.size, wd, pd, crop, out_off)), _bits(got)), "a second call differs"
        assert torch.equal(_bits(_window_call(raw_other, base, flat.size, wd, pd, crop, out_off)), _bits(got)), \
            "bytes outside the windows matter"
        for n in range(N if N > 1 else 0):
            one = _window_call(raw, base, flat.size, wd[n:n + 1].clone(), None if pd is None else pd[n:n + 1].clone(), crop, out_off)
            assert torch.equal(_bits(one[0]), _bits(got[n])), (case["name"], k, n, "alone differs")
        a, b = D.batch_from_windows((raw[base:], raw_other[base:]), wt, crop, pt)         # the wrapper, a pair of caches
        assert tuple(a.shape) == (N, 3) + tuple(crop) and a.dtype == torch.float32 and a.device == raw.device
        assert torch.equal(_bits(a), _bits(got)) and torch.equal(_bits(b), _bits(got))
        assert torch.equal(_bits(D.batch_from_windows(raw[base:], wt, crop, pt)), _bits(got))
    print(f"windows {case['name']}: max |err| vs float64 {worst / R.EPS:.3f} * 2^-24 (bound 8)")
    assert worst <= R.BATCH_BOUND
    assert torch.equal(raw.cpu(), host), "the cache was written"


def test_window_refusals():
    cache = torch.zeros(96, dtype=torch.uint8, device=DEV)
    win = torch.tensor([[0, 12]], dtype=torch.int64)
    with pytest.raises(IndexError):
        D.batch_from_windows(cache, torch.tensor([[0, 12], [52, 12]], dtype=torch.int64), (4, 4))
    with pytest.raises(TypeError):
        D.batch_from_windows(cache, win.to(DEV), (4, 4))              # no device windows
    wd, out = win.to(DEV), torch.zeros(48, device=DEV)
    for nbytes, N, CH, CW, nblk in ((47, 1, 4, 4, 1), (96, 1, 4, 4, 2), (96, 0, 4, 4, 1), (96, 1, 0, 4, 1), (96, 1, 4, 0, 1)):
        with pytest.raises(RuntimeError, match="ADH_E_ARG"):
            H.call("adh_batch_window_from_u8", cache.data_ptr(), nbytes, wd.data_ptr(), None, N, CH, CW, None, nblk, out.data_ptr())
    with pytest.raises(RuntimeError, match="ADH_E_ARG"):              # rows without a workspace
        H.call("adh_batch_window_from_u8", cache.data_ptr(), 96, wd.data_ptr(), out.data_ptr(), 1, 4, 4, None, 1, out.data_ptr())
    assert (out == 0).all()


# ------------------------------------------------------------------------------------------------ end to end
CROP = 24


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    """train / val / test with 4 / 2 / 2 files per level; the caches start empty and every folder_index call is counted"""
    root = str(tmp_path_factory.mktemp("crop_folders"))
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


def _cfg(root, tmp_path, crop=CROP):
    cfg = _folder_cfg(root, tmp_path)
    cfg["dataset"]["crop_size"] = crop
    return cfg


def _files(records):
    """{name: {role: uint8 [h, w, 3] of the file}}"""
    return {r["name"]: {role: R.rgb3(IO.load_image(r[role]).numpy()) for role in ("hazy", "clear")} for r in records}


def _unit(u8):
    return torch.from_numpy(np.ascontiguousarray(u8.transpose(2, 0, 1))).float() / 255


def test_crop_batches_of_the_loader(tree, tmp_path):
    root, listing, counts = tree
    cfg = _cfg(root, tmp_path)
    # validation: the centre windows, bit for bit v / 255 of the file bytes, index order, each file once
    files = _files(D.folder_index.uncounted(root, "val"))
    batches = list(D.folder_loader(cfg, "val", DEV)(0))
    assert [len(b["name"]) for b in batches] == [4, 2]
    seen = []
    for b in batches:
        n = len(b["name"])
        assert set(b) == {"hazy", "clear", "intensity", "name"}
        for role in ("hazy", "clear"):
            assert tuple(b[role].shape) == (n, 3, CROP, CROP) and b[role].dtype == torch.float32 and str(b[role].device) == DEV
        assert b["intensity"].dtype == torch.int64 and str(b["intensity"].device) == DEV and tuple(b["intensity"].shape) == (n,)
        for i, name in enumerate(b["name"]):
            seen.append((D.LEVEL_NAMES[int(b["intensity"][i])], name))
            for role in ("hazy", "clear"):
                u8 = files[name][role]
                y0, x0 = (u8.shape[0] - CROP) // 2, (u8.shape[1] - CROP) // 2
                assert torch.equal(_bits(b[role][i].cpu()), _bits(_unit(u8[y0:y0 + CROP, x0:x0 + CROP]))), (name, role)
    assert seen == listing["val"]
    # training, augmented: within the float64 bound of the file's own bytes at the origin and row re-drawn from the seed
    records = D.folder_index.uncounted(root, "train")
    files = _files(records)
    sizes = np.array([files[r["name"]]["hazy"].shape[:2] for r in records], np.int64)
    seed, bs = int(cfg["seed"]), int(cfg["dataset"]["batch_size"])
    loader = D.folder_loader(cfg, "train", DEV)
    drawn = {}
    for epoch in (0, 1):
        rng = np.random.RandomState(seed + epoch)
        plan = D.epoch_plan(len(records), 1, 0, bs, seed, epoch, True)
        batches = list(loader(epoch))
        assert [b["name"] for b in batches] == [[records[i]["name"] for i in s] for s in plan]
        worst = 0.0
        for b, s in zip(batches, plan):
            params = D.draw_augment_params(len(s), rng)
            origins = D.draw_crop_origins(sizes[s], CROP, rng)
            assert b["intensity"].tolist() == [records[i]["intensity"] for i in s]
            for i, name in enumerate(b["name"]):
                y0, x0 = origins[i].tolist()
                drawn[epoch, name] = (y0, x0)
                for role in ("hazy", "clear"):
                    assert tuple(b[role].shape) == (len(s), 3, CROP, CROP)
                    win = files[name][role][y0:y0 + CROP, x0:x0 + CROP]
                    ref = R.batch_ref(win[None], [0], params[i:i + 1].numpy())[0]
                    worst = max(worst, float(np.abs(b[role][i].cpu().double().numpy() - ref).max()))
        print(f"crop train epoch {epoch}: max |err| vs float64 of the files {worst / R.EPS:.3f} * 2^-24 (bound 8)")
        assert worst <= R.BATCH_BOUND
    assert sum(drawn[0, r["name"]] != drawn[1, r["name"]] for r in records) >= len(records) // 2     # fresh patches per epoch
    # without augmentation the origins are the first draws, and the crops are the files' bytes
    cfg["dataset"]["augmentation"] = False
    rng = np.random.RandomState(seed + 1)
    for b, s in zip(D.folder_loader(cfg, "train", DEV)(1), D.epoch_plan(len(records), 1, 0, bs, seed, 1, True)):
        origins = D.draw_crop_origins(sizes[s], CROP, rng)
        for i, name in enumerate(b["name"]):
            y0, x0 = origins[i].tolist()
            assert torch.equal(_bits(b["clear"][i].cpu()), _bits(_unit(files[name]["clear"][y0:y0 + CROP, x0:x0 + CROP])))
    assert counts["val"] == 1 and counts["train"] == 1               # one cache per split, whatever `augmentation` says


def test_crop_shards_the_memory_limit_and_unequal_pairs(tree, tmp_path, monkeypatch, capsys):
    root, listing, _ = tree
    records = D.folder_index.uncounted(root, "train")
    files = _files(records)
    whole = D.FolderDataset(records, 32, DEV, split="train", crop_size=CROP)
    out = capsys.readouterr().out
    need = 2 * sum(-(-f["hazy"].size // 4) * 4 for f in files.values())
    assert "Loaded 12 samples for train split" in out and "skipped 0 hazy files" in out
    assert f"12 pairs at their own sizes (0 upscaled to hold a {CROP}x{CROP} crop)" in out and f"({need} bytes)" in out
    assert whole.hazy.dim() == 1 and whole.hazy.numel() == whole.clear.numel() == need // 2 == whole.cache_bytes
    assert whole.sizes.dtype == np.int64 and whole.offsets.dtype == np.int64 and (whole.offsets % 4 == 0).all()
    assert whole.sizes.tolist() == [list(files[r["name"]]["hazy"].shape[:2]) for r in records]
    shard = D.FolderDataset(records, 32, DEV, rank=1, world=2, threads=64, split="train", crop_size=[CROP, CROP])
    assert shard.names == [r["name"] for r in records[1::2]] and "(rank 1 of 2)" in capsys.readouterr().out
    for k, name in enumerate(shard.names):                            # a shard holds the bytes the whole cache holds
        j = whole.names.index(name)
        nb = int(shard.sizes[k].prod()) * 3
        assert shard.sizes[k].tolist() == whole.sizes[j].tolist() and int(shard.labels[k]) == int(whole.labels[j])
        for role in ("hazy", "clear"):
            mine = getattr(shard, role)[int(shard.offsets[k]):int(shard.offsets[k]) + nb]
            assert torch.equal(mine, getattr(whole, role)[int(whole.offsets[j]):int(whole.offsets[j]) + nb])
            assert np.array_equal(mine.cpu().numpy().reshape(files[name][role].shape), files[name][role])
    val = list(shard.epoch(0, 4, 42, train=False))
    assert [n for b in val for n in b["name"]] == shard.names and [len(b["name"]) for b in val] == [4, 2]
    mixed = [dict(records[0])]
    other = next(r for r in records if files[r["name"]]["hazy"].shape != files[records[0]["name"]]["hazy"].shape)
    mixed[0]["clear"] = other["clear"]
    with pytest.raises(ValueError) as e:
        D.FolderDataset(mixed, 32, DEV, crop_size=CROP)
    assert records[0]["hazy"] in str(e.value) and other["clear"] in str(e.value)
    assert "40x56" in str(e.value) and "32x32" in str(e.value)
    monkeypatch.setattr(torch.cuda, "mem_get_info", lambda *a, **k: (2 * need - 2, 1 << 40))
    with pytest.raises(RuntimeError, match=f"needs {need} bytes.*streaming loader is not built"):
        D.FolderDataset(records, 32, DEV, crop_size=CROP)
    monkeypatch.setattr(torch.cuda, "mem_get_info", lambda *a, **k: (2 * need, 1 << 40))
    assert len(D.FolderDataset(records, 32, DEV, crop_size=CROP)) == 12


def test_files_smaller_than_the_crop_are_upscaled_once(tree, capsys):
    """crop_size [36, 44]: the 32 x 32 files are cached at 44 x 44 (the resize's float64 reference, near-ties as in
    tests/_dataset_ref64.check_resize: 1.4-1.5 % of random bytes at 32 -> 44), the 40 x 56 files byte for byte"""
    root, listing, _ = tree
    records = D.folder_index.uncounted(root, "val")
    ds = D.FolderDataset(records, 32, DEV, split="val", crop_size=[36, 44])
    small = 0
    for k, r in enumerate(records):
        for role in ("hazy", "clear"):
            src = IO.load_image(r[role]).numpy()
            oh, ow = ds.sizes[k].tolist()
            got = getattr(ds, role)[int(ds.offsets[k]):int(ds.offsets[k]) + oh * ow * 3].cpu().numpy().reshape(oh, ow, 3)
            if src.shape[:2] == (32, 32):
                assert (oh, ow) == (44, 44)
                R.check_resize(got, src, 44, 44, what=f"{r['name']} {role} C={src.shape[2]}")
                small += role == "hazy"
            else:
                assert (oh, ow) == (40, 56) and np.array_equal(got, R.rgb3(src))
    assert small == 3 and f"6 pairs at their own sizes ({small} upscaled to hold a 36x44 crop)" in capsys.readouterr().out
    b = next(iter(ds.epoch(0, 6, 1, train=True)))
    assert tuple(b["hazy"].shape) == (6, 3, 36, 44) and tuple(b["clear"].shape) == (6, 3, 36, 44)


# ------------------------------------------------------------------------------------------------ drivers
def test_drivers_train_on_crops(tree, tmp_path, monkeypatch):
    """crops of 24 x 24: the LPIPS term of DehazingLoss is switched off, because its AlexNet has no output under 31 x 31 (the 11 x 11
    stride-4 convolution leaves 5 x 5, the first 3 x 3 stride-2 pool 2 x 2, the second nothing; torchvision's raises there too)"""
    root, listing, counts = tree
    cfg = _cfg(root, tmp_path)
    cfg["loss"] = {"perceptual": False}
    vals, shapes = [], set()
    real = T.validate_dehazing
    monkeypatch.setattr(T, "validate_dehazing", lambda *a, **k: vals.append(real(*a, **k)) or vals[-1])
    real_windows = D.batch_from_windows
    monkeypatch.setattr(D, "batch_from_windows", lambda *a, **k: [shapes.add(tuple(x.shape[1:])) or x for x in real_windows(*a, **k)])
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        torch.manual_seed(3)
        model, losses = T.train_dehazing_model(cfg, "low", epochs=1)
        torch.manual_seed(5)
        system, hist = T.train_joint_model(cfg, epochs=1)
    _no_synthetic(caught)
    assert 1 <= len(losses) <= 3 and all(np.isfinite(l) for l in losses)
    assert len(vals) == 1 and vals[0]["val_samples"] == sum(level == "low" for level, _ in listing["val"]) == 2
    assert np.isfinite(vals[0]["val_loss"])
    assert len(hist) == 1 and hist[0]["val_samples"] == len(listing["val"]) == 6
    assert all(np.isfinite(hist[0][k]) for k in ("train_loss", "val_loss", "val_psnr", "val_ssim"))
    assert shapes == {(3, CROP, CROP)}                                # every batch of both drivers was a batch of crops
    assert counts["train"] == 1 and counts["val"] == 1               # each split's index is read once per process
