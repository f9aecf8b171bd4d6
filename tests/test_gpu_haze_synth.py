"""Haze synthesis on the GPU: adh_batch_haze_from_u8 and adh_u16_resize_bilinear through the C ABI over the table of
tests/_haze_synth_ref64.py with the contracts of the host-emulated run (guard bytes around both caches and the output), and
`dataset.synthetic_haze` end to end on a tree of clear files and depth maps: the loader, the shards, the drivers, and
`main.py --mode synthesize`."""
import json
import os
import sys
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
from tests import _haze_synth_ref64 as Z
from tests.test_gpu_dataset import _cfg as _folder_cfg
from tests.test_gpu_dataset import _no_synthetic

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILL = 0x5A
GUARD = 16                      # bytes in front of and behind either cache (the front keeps a cache's phase: 16 + base)
SENTINEL = float(np.float32(-1234.5))
FRONT = 4                       # sentinel floats in front of the output: it starts 16-byte aligned, plus out_off floats
RANGE = (0.3, 1.0)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _guarded(arr, base):
    """the array's bytes on the device with GUARD + base filler bytes in front and GUARD behind -> (host copy, device, offset)"""
    a = np.ascontiguousarray(arr).view(np.uint8).reshape(-1)
    host = torch.from_numpy(np.concatenate([np.full(GUARD + base, FILL, np.uint8), a, np.full(GUARD, FILL, np.uint8)]))
    return host, host.to(DEV), GUARD + base


def _haze_call(clear, depth, geom_dev, fog_dev, pd, crop, out_off=0, N=None):
    """the C entry point; clear / depth = (device buffer, offset, bytes) or None.  The output stands FRONT + out_off floats into a
    buffer of sentinels with 64 more behind; returns [N,3,CH,CW] after checking that the sentinels stand"""
    (CH, CW), N = crop, geom_dev.shape[0] if N is None else N
    n, nblk = N * 3 * CH * CW, H.value("adh_batch_num_blocks", CH * CW)
    at = FRONT + out_off
    out = torch.full((at + n + 64,), SENTINEL, dtype=torch.float32, device=DEV)
    partial = torch.zeros(N * nblk, dtype=torch.float64, device=DEV)
    dptr, dbytes = (None, 0) if depth is None else (depth[0].data_ptr() + depth[1], depth[2])
    H.call("adh_batch_haze_from_u8", clear[0].data_ptr() + clear[1], clear[2], dptr, dbytes, geom_dev.data_ptr(), fog_dev.data_ptr(),
           RANGE[0], RANGE[1], H.ptr(pd), N, CH, CW, partial.data_ptr(), nblk, out.data_ptr() + 4 * at)
    assert (out[:at] == SENTINEL).all() and (out[at + n:] == SENTINEL).all(), "a float outside the output was written"
    return out[at:at + n].view(N, 3, CH, CW)


# ------------------------------------------------------------------------------------------------ kernel
@pytest.mark.parametrize("radial", [False, True], ids=["depth", "radial"])
@pytest.mark.parametrize("no", range(len(Z.CASES)), ids=[c["name"] for c in Z.CASES])
def test_cases_on_the_device(no, radial):
    case = Z.CASES[no]
    clear, depth, geom, dclear, ddepth, fog = Z.build(case)
    crop, out_off = case["crop"], case["out_off"]
    N = len(geom)
    chost, cdev, coff = _guarded(clear, case["base"])
    dhost, ddev, doff = _guarded(depth, case["dbase"])
    cw = (cdev, coff, clear.size)
    dw = None if radial else (ddev, doff, depth.size * 2)
    dense_c = (torch.from_numpy(dclear).to(DEV), 0, dclear.size)
    dense_d = None if radial else (torch.from_numpy(ddepth).to(DEV), 0, ddepth.size * 2)
    gd, dgd, fd = torch.from_numpy(geom).to(DEV), torch.from_numpy(Z.dense_geom(N, *crop)).to(DEV), torch.from_numpy(fog).to(DEV)
    f0 = fd.clone()
    f0[:, 0] = 0
    wt = torch.from_numpy(np.ascontiguousarray(geom[:, :2]))
    for params in [None] + K.param_sets(no + int(radial), N, 1):
        pt = None if params is None else torch.from_numpy(params)
        pd = None if params is None else pt.to(DEV)
        got = _haze_call(cw, dw, gd, fd, pd, crop, out_off)
        ref = Z.haze_ref(dclear, None if radial else ddepth, fog, RANGE, params)
        err = float(np.abs(got.cpu().double().numpy() - ref).max())
        bound = Z.HAZE_BOUND if params is None else Z.HAZE_AUG_BOUND
        print(f"{case['name']} radial={radial} rows={params is not None}: max err {err / Z.EPS:.3f} * 2^-24, bound {bound / Z.EPS:.3f}")
        assert float(got.min()) >= 0.0 and float(got.max()) <= 1.0
        assert err <= bound
        assert torch.equal(_bits(_haze_call(cw, dw, gd, fd, pd, crop, out_off)), _bits(got)), "a second call differs"
        assert torch.equal(_bits(_haze_call(dense_c, dense_d, dgd, fd, pd, crop)), _bits(got)), "differs from dense geometry"
        plain = D.batch_from_windows(cdev[coff:coff + clear.size], wt, crop, pt)
        assert torch.equal(_bits(_haze_call(cw, dw, gd, f0, pd, crop, out_off)), _bits(plain)), "beta = 0 differs from the clear window"
        for n in range(N if N > 1 else 0):
            one = _haze_call(cw, dw, gd[n:n + 1].clone(), fd[n:n + 1].clone(), None if pd is None else pd[n:n + 1].clone(), crop, out_off)
            assert torch.equal(_bits(one[0]), _bits(got[n])), (case["name"], n, "alone differs")
        dview = None if radial else ddev[doff:doff + depth.size * 2].view(torch.uint16)       # the wrapper, on views of the buffers
        a = D.batch_haze_from_windows(cdev[coff:coff + clear.size], dview, torch.from_numpy(geom), torch.from_numpy(fog), crop, pt, RANGE)
        assert tuple(a.shape) == (N, 3) + tuple(crop) and a.dtype == torch.float32 and torch.equal(_bits(a), _bits(got))
    assert torch.equal(cdev.cpu(), chost) and torch.equal(ddev.cpu(), dhost), "a cache or its guard bytes were written"


def test_extremes_and_refusals():
    CH, CW = 4, 8
    clear = np.zeros((1, CH, CW, 3), np.uint8)
    clear[:, :, 4:] = 255
    depth = np.zeros((1, CH, CW), np.uint16)
    depth[:, 2:] = 65535
    fog = np.array([[1.0, 1.0]], np.float32)
    cd, dd = torch.from_numpy(clear).to(DEV), torch.from_numpy(depth).to(DEV)
    gd, fd = torch.from_numpy(Z.dense_geom(1, CH, CW)).to(DEV), torch.from_numpy(fog).to(DEV)
    for params in (None, np.array([[1, 0, 1, 1.1, 1.1]], np.float32)):
        pd = None if params is None else torch.from_numpy(params).to(DEV)
        for dwin, dref in (((dd, 0, depth.size * 2), depth), (None, None)):
            got = _haze_call((cd, 0, clear.size), dwin, gd, fd, pd, (CH, CW))
            assert float(got.min()) >= 0 and float(got.max()) <= 1
            assert np.abs(got.cpu().double().numpy() - Z.haze_ref(clear, dref, fog, RANGE, params)).max() <= \
                (Z.HAZE_BOUND if params is None else Z.HAZE_AUG_BOUND)
    out = torch.zeros(3 * CH * CW, device=DEV)
    part = torch.zeros(1, dtype=torch.float64, device=DEV)
    ok = dict(clear=cd.data_ptr(), cb=clear.size, depth=dd.data_ptr(), db=depth.size * 2, geom=gd.data_ptr(), fog=fd.data_ptr(),
              params=None, N=1, CH=CH, CW=CW, partial=part.data_ptr(), nblk=1, out=out.data_ptr())
    for change in (dict(clear=None), dict(geom=None), dict(fog=None), dict(out=None), dict(params=fd.data_ptr(), partial=None),
                   dict(N=0), dict(N=65536), dict(CH=0), dict(CW=0), dict(nblk=2), dict(cb=CH * CW * 3 - 1), dict(db=CH * CW * 2 - 1),
                   dict(depth=dd.data_ptr() + 1)):
        a = dict(ok, **change)
        with pytest.raises(RuntimeError, match="ADH_E_ARG"):
            H.call("adh_batch_haze_from_u8", a["clear"], a["cb"], a["depth"], a["db"], a["geom"], a["fog"], 0.3, 1.0, a["params"], a["N"],
                   a["CH"], a["CW"], a["partial"], a["nblk"], a["out"])
    src = torch.zeros(64, dtype=torch.uint8, device=DEV)
    dst = torch.zeros(8, dtype=torch.uint16, device=DEV)
    for args in ((None, 8, 4, 4, 2, dst.data_ptr(), 2, 2), (src.data_ptr(), 8, 4, 4, 2, None, 2, 2), (src.data_ptr(), 7, 4, 4, 2, dst.data_ptr(), 2, 2),
                 (src.data_ptr(), 8, 4, 4, 3, dst.data_ptr(), 2, 2), (src.data_ptr(), 8, 0, 4, 2, dst.data_ptr(), 2, 2),
                 (src.data_ptr(), 8, 4, 4, 2, dst.data_ptr(), 0, 2), (src.data_ptr() + 1, 8, 4, 4, 2, dst.data_ptr(), 2, 2),
                 (src.data_ptr(), 8, 4, 4, 2, dst.data_ptr() + 1, 2, 2), (src.data_ptr(), 3, 4, 4, 1, dst.data_ptr(), 2, 2)):
        with pytest.raises(RuntimeError, match="ADH_E_ARG"):
            H.call("adh_u16_resize_bilinear", *args)
    assert (out == 0).all() and (dst == 0).all()
    with pytest.raises(TypeError):
        D.batch_haze_from_windows(cd, dd, torch.from_numpy(Z.dense_geom(1, CH, CW)).to(DEV), torch.from_numpy(fog), (CH, CW))
    with pytest.raises(IndexError):
        D.batch_haze_from_windows(cd, dd, torch.tensor([[0, CW * 3, 2, CW * 2]], dtype=torch.int64), torch.from_numpy(fog), (CH, CW))


def _resize16(src, OH, OW, off=0, slack=0):
    """adh_u16_resize_bilinear on a source with `slack` bytes of pitch padding, `off` bytes into its buffer; the destination has
    guard levels on both sides, checked afterwards"""
    h, w = src.shape
    bpp = src.dtype.itemsize
    rows = np.full((h, w * bpp + slack), 0xEE, np.uint8)
    rows[:, :w * bpp] = np.ascontiguousarray(src).view(np.uint8).reshape(h, w * bpp)
    buf = torch.from_numpy(np.concatenate([np.full(off, FILL, np.uint8), rows.reshape(-1)])).to(DEV)
    dst = torch.from_numpy(np.full(8 + OH * OW + 8, 0x5A5A, np.uint16)).to(DEV)
    H.call("adh_u16_resize_bilinear", buf.data_ptr() + off, w * bpp + slack, h, w, bpp, dst.data_ptr() + 16, OH, OW)
    got = dst.cpu().numpy()
    assert (got[:8] == 0x5A5A).all() and (got[8 + OH * OW:] == 0x5A5A).all(), "a level outside the slot was written"
    return got[8:8 + OH * OW].reshape(OH, OW)


def test_resize16_on_the_device():
    for (size, out) in Z.RESIZE16_CASES:
        rng = np.random.RandomState(size[0] * 100 + size[1])
        src = rng.randint(0, 65536, size=size).astype(np.uint16)
        src.reshape(-1)[:2] = (0, 65535)[:min(2, src.size)]
        Z.check_resize16(_resize16(src, *out, off=2, slack=2), src, *out, what="16-bit")
        src8 = rng.randint(0, 256, size=size).astype(np.uint8)
        Z.check_resize16(_resize16(src8, *out, off=1, slack=1), src8.astype(np.uint16) * 257, *out, what="8-bit")
    for (size, out) in Z.RESIZE16_DYADIC:
        rng = np.random.RandomState(size[0] + size[1])
        src = rng.randint(0, 65536, size=size).astype(np.uint16)
        got = _resize16(src, *out)
        Z.check_resize16(got, src, *out, exact=True, what="dyadic")
        src8 = rng.randint(0, 256, size=size).astype(np.uint8)
        got8 = _resize16(src8, *out, off=3)
        Z.check_resize16(got8, src8.astype(np.uint16) * 257, *out, exact=True, what="dyadic 8-bit")
        if size == out:
            assert np.array_equal(got, src) and np.array_equal(got8, src8.astype(np.uint16) * 257)


# ------------------------------------------------------------------------------------------------ end to end
CROP = 24


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    """train / val with 6 / 4 clear files and their depth maps; the caches start empty"""
    root = str(tmp_path_factory.mktemp("haze_folders"))
    listing = Z.write_tree(root)
    real = D._CACHES
    D._CACHES = {}
    yield root, listing
    D._CACHES = real


def _cfg(root, tmp_path, crop=None, **haze):
    cfg = _folder_cfg(root, tmp_path)
    cfg["dataset"]["synthetic_haze"] = dict(haze)
    if crop is not None:
        cfg["dataset"]["crop_size"] = crop
    return cfg


def _files(records):
    """{name: (uint8 [h, w, 3], uint16 [h, w] levels)} of the files themselves"""
    return {r["name"]: (R.rgb3(IO.load_image(r["clear"]).numpy()), IO.load_depth(r["depth"]).numpy()) for r in records}


def _cached(ds, k):
    """image k of a HazeSynthDataset as (uint8 [h, w, 3], uint16 [h, w]) host arrays"""
    if ds.crop is None:
        return ds.clear[k].cpu().numpy(), ds.depth[k].cpu().numpy()
    h, w = ds.sizes[k].tolist()
    c = ds.clear[int(ds.offsets[k]):int(ds.offsets[k]) + h * w * 3].cpu().numpy().reshape(h, w, 3)
    at = int(ds.depth_offsets[k]) // 2
    return c, ds.depth[at:at + h * w].cpu().numpy().reshape(h, w)


def _in_range(labels, fog):
    for lab, (beta, A) in zip(labels.tolist(), fog.tolist()):
        (b0, b1), (a0, a1) = D.FOG_RANGES[D.LEVEL_NAMES[lab]]
        assert np.float32(b0) <= np.float32(beta) <= np.float32(b1) and np.float32(a0) <= np.float32(A) <= np.float32(a1)


@pytest.mark.parametrize("crop", [None, CROP], ids=["dense", "crop24"])
def test_batches_of_the_loader(tree, tmp_path, crop, capsys):
    root, listing = tree
    cfg = _cfg(root, tmp_path, crop)
    seed, bs = int(cfg["seed"]), int(cfg["dataset"]["batch_size"])
    size = (32, 32) if crop is None else (CROP, CROP)
    # the caches hold the files: byte for byte where the size is kept, through the resize kernels otherwise
    loaders = {split: D.folder_loader(cfg, split, DEV) for split in ("train", "val")}
    out = capsys.readouterr().out
    assert "Loaded 6 clear images for train split" in out and "depth: folder" in out
    assert D.folder_loader(cfg, "val", DEV).dataset is loaders["val"].dataset        # one cache per split
    for split in ("train", "val"):
        records, ds = D.haze_index(root, split), loaders[split].dataset
        files = _files(records)
        assert ds.names == listing[split] and ds.depth.dtype == torch.uint16 and ds.clear.dtype == torch.uint8
        if crop is not None:
            assert (ds.offsets % 4 == 0).all() and (ds.depth_offsets % 4 == 0).all() and ds.clear.dim() == 1
            assert ds.sizes.tolist() == [list(files[n][0].shape[:2]) for n in ds.names]
        for k, name in enumerate(ds.names):
            c, d = _cached(ds, k)
            fc, fd = files[name]
            if c.shape == fc.shape:
                assert np.array_equal(c, fc) and np.array_equal(d, fd), name       # the 8-bit depth file arrives as v * 257
            else:
                assert crop is None and fc.shape[:2] == (40, 56)
                R.check_resize(c, fc, 32, 32, what=name)
                Z.check_resize16(d, fd, 32, 32, what=name)
    # validation: the centre crop, no rows, draws that depend on the seed and the sample alone; two epochs are bit-identical
    ds = loaders["val"].dataset
    first, second = list(loaders["val"](0)), list(loaders["val"](3))
    assert [b["name"] for b in first] == [listing["val"]]
    for a, b in zip(first, second):
        assert set(a) == {"hazy", "clear", "intensity", "beta", "airlight", "name"}
        assert torch.equal(a["intensity"], b["intensity"]) and a["name"] == b["name"]
        for key in ("hazy", "clear", "beta", "airlight"):
            assert torch.equal(_bits(a[key]), _bits(b[key])), key
    b = first[0]
    n = len(b["name"])
    labels, fog = D.fixed_haze_params(seed, range(n))
    assert b["intensity"].tolist() == labels.tolist() and str(b["intensity"].device) == DEV and b["intensity"].dtype == torch.int64
    assert torch.equal(b["beta"].cpu(), fog[:, 0]) and torch.equal(b["airlight"].cpu(), fog[:, 1]) and str(b["beta"].device) == DEV
    _in_range(b["intensity"], torch.stack([b["beta"], b["airlight"]], 1).cpu())
    for i, name in enumerate(b["name"]):
        c, d = _cached(ds, i)
        y0, x0 = (c.shape[0] - size[0]) // 2, (c.shape[1] - size[1]) // 2
        wc, wd = c[y0:y0 + size[0], x0:x0 + size[1]], d[y0:y0 + size[0], x0:x0 + size[1]]
        assert tuple(b["hazy"].shape) == (n, 3) + size and b["hazy"].dtype == torch.float32
        ref = Z.haze_ref(wc[None], wd[None], fog[i:i + 1].numpy(), RANGE)[0]
        assert np.abs(b["hazy"][i].cpu().double().numpy() - ref).max() <= Z.HAZE_BOUND, name
        assert torch.equal(_bits(b["clear"][i].cpu()), _bits(torch.from_numpy(np.ascontiguousarray(wc.transpose(2, 0, 1))).float() / 255))
    # a 2-way shard covers every file once, under the draws of the whole split
    seen = {}
    for rank in (0, 1):
        shard = D.folder_loader(cfg, "val", DEV, rank=rank, world=2)
        for sb in shard(1):
            for i, name in enumerate(sb["name"]):
                assert name not in seen
                seen[name] = (int(sb["intensity"][i]), float(sb["beta"][i]), float(sb["airlight"][i]), sb["hazy"][i])
    assert sorted(seen) == sorted(listing["val"])
    for i, name in enumerate(b["name"]):
        assert seen[name][:3] == (int(b["intensity"][i]), float(b["beta"][i]), float(b["airlight"][i]))
        assert torch.equal(_bits(seen[name][3]), _bits(b["hazy"][i]))
    # training: re-drawn from the seed in the documented order; within the float64 bound of the cache under the yielded beta, A
    ds, records = loaders["train"].dataset, D.haze_index(root, "train")
    drawn = {}
    for epoch in (0, 1):
        rng = np.random.RandomState(seed + epoch)
        plan = D.epoch_plan(len(records), 1, 0, bs, seed, epoch, True)
        batches = list(loaders["train"](epoch))
        assert [b["name"] for b in batches] == [[records[i]["name"] for i in s] for s in plan]
        worst = 0.0
        for b, s in zip(batches, plan):
            params = D.draw_augment_params(len(s), rng)
            origins = np.zeros((len(s), 2), np.int64) if crop is None else D.draw_crop_origins(ds.sizes[s], CROP, rng)
            labels, fog = D.draw_haze_params(len(s), rng)
            assert b["intensity"].tolist() == labels.tolist()
            assert torch.equal(b["beta"].cpu(), fog[:, 0]) and torch.equal(b["airlight"].cpu(), fog[:, 1])
            yielded = torch.stack([b["beta"], b["airlight"]], 1).cpu()
            _in_range(b["intensity"], yielded)
            for i, k in enumerate(s.tolist()):
                c, d = _cached(ds, k)
                y0, x0 = origins[i].tolist()
                wc, wd = c[y0:y0 + size[0], x0:x0 + size[1]], d[y0:y0 + size[0], x0:x0 + size[1]]
                ref = Z.haze_ref(wc[None], wd[None], yielded[i:i + 1].numpy(), RANGE, params[i:i + 1].numpy())[0]
                worst = max(worst, float(np.abs(b["hazy"][i].cpu().double().numpy() - ref).max()))
                cref = R.batch_ref(wc[None], [0], params[i:i + 1].numpy())[0]
                assert np.abs(b["clear"][i].cpu().double().numpy() - cref).max() <= R.BATCH_BOUND
                drawn[epoch, records[k]["name"]] = (float(b["beta"][i]), float(b["airlight"][i]))
        print(f"synthetic_haze train epoch {epoch}: max |err| vs float64 {worst / Z.EPS:.3f} * 2^-24 (bound 9)")
        assert worst <= Z.HAZE_AUG_BOUND
    assert all(drawn[0, r["name"]] != drawn[1, r["name"]] for r in records)              # every epoch re-renders every image


def test_radial_without_a_depth_folder_and_the_memory_limit(tmp_path, monkeypatch, capsys):
    root = str(tmp_path / "clear_only")
    listing = Z.write_tree(root, splits=(("train", 4),), depth=False)
    real = D._CACHES
    monkeypatch.setattr(D, "_CACHES", {})
    cfg = _cfg(root, tmp_path, CROP, depth="radial")
    with pytest.raises(FileNotFoundError, match="depth"):
        D.folder_loader(_cfg(root, tmp_path, CROP), "train", DEV)                        # the default asks for the depth folder
    loader = D.folder_loader(cfg, "train", DEV)
    ds = loader.dataset
    assert ds.depth is None and "depth: radial" in capsys.readouterr().out
    rng = np.random.RandomState(int(cfg["seed"]))
    for b, s in zip(loader(0), D.epoch_plan(4, 1, 0, 4, int(cfg["seed"]), 0, True)):
        params = D.draw_augment_params(len(s), rng)
        origins = D.draw_crop_origins(ds.sizes[s], CROP, rng)
        labels, fog = D.draw_haze_params(len(s), rng)
        assert b["intensity"].tolist() == labels.tolist()
        for i, k in enumerate(s.tolist()):
            h, w = ds.sizes[k].tolist()
            c = ds.clear[int(ds.offsets[k]):int(ds.offsets[k]) + h * w * 3].cpu().numpy().reshape(h, w, 3)
            y0, x0 = origins[i].tolist()
            ref = Z.haze_ref(c[None, y0:y0 + CROP, x0:x0 + CROP], None, fog[i:i + 1].numpy(), RANGE, params[i:i + 1].numpy())[0]
            assert np.abs(b["hazy"][i].cpu().double().numpy() - ref).max() <= Z.HAZE_AUG_BOUND
    assert len(D._CACHES) == 1 and D._CACHES is not real
    # 5 bytes per pixel with depth maps, 3 without
    records = D.haze_index(root, "train", "radial")
    px = sum(40 * 56 if k % 2 == 0 else 32 * 32 for k in range(4))
    monkeypatch.setattr(torch.cuda, "mem_get_info", lambda *a, **k: (2 * 3 * px - 2, 1 << 40))
    with pytest.raises(RuntimeError, match=f"needs {3 * px} bytes.*3 bytes per pixel.*streaming loader is not built"):
        D.HazeSynthDataset(records, 32, DEV, crop_size=CROP, depth="radial")
    monkeypatch.setattr(torch.cuda, "mem_get_info", lambda *a, **k: (2 * 3 * 4 * 32 * 32 - 2, 1 << 40))
    with pytest.raises(RuntimeError, match=f"needs {3 * 4 * 32 * 32} bytes.*3 bytes per pixel"):
        D.HazeSynthDataset(records, 32, DEV, depth="radial")
    monkeypatch.setattr(torch.cuda, "mem_get_info", lambda *a, **k: (2 * 3 * px, 1 << 40))
    assert len(D.HazeSynthDataset(records, 32, DEV, crop_size=CROP, depth="radial")) == 4
    full = str(tmp_path / "with_depth")
    Z.write_tree(full, splits=(("train", 4),))
    monkeypatch.setattr(torch.cuda, "mem_get_info", lambda *a, **k: (2 * 5 * px - 2, 1 << 40))
    with pytest.raises(RuntimeError, match=f"needs {5 * px} bytes.*clear images and depth maps.*5 bytes per pixel"):
        D.HazeSynthDataset(D.haze_index(full, "train"), 32, DEV, crop_size=CROP)
    monkeypatch.setattr(torch.cuda, "mem_get_info", lambda *a, **k: (2 * 5 * px, 1 << 40))
    assert len(D.HazeSynthDataset(D.haze_index(full, "train"), 32, DEV, crop_size=CROP)) == 4


def test_drivers_train_on_synthesized_haze(tree, tmp_path, monkeypatch):
    """crops of 24 x 24, so the LPIPS term is off as in tests/test_gpu_dataset_crop.py (its AlexNet has no output under 31 x 31)"""
    root, listing = tree
    cfg = _cfg(root, tmp_path, CROP)
    cfg["loss"] = {"perceptual": False}
    shapes = set()
    real = D.batch_haze_from_windows
    monkeypatch.setattr(D, "batch_haze_from_windows", lambda *a, **k: (lambda x: shapes.add(tuple(x.shape[1:])) or x)(real(*a, **k)))
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        torch.manual_seed(3)
        model, losses = T.train_dehazing_model(cfg, "low", epochs=1)
        torch.manual_seed(5)
        system, hist = T.train_joint_model(cfg, epochs=1)
    _no_synthetic(caught)
    assert 1 <= len(losses) <= 2 and all(np.isfinite(l) for l in losses)
    assert len(hist) == 1 and hist[0]["val_samples"] == len(listing["val"])
    assert all(np.isfinite(hist[0][k]) for k in ("train_loss", "val_loss", "val_psnr", "val_ssim"))
    assert shapes == {(3, CROP, CROP)}                                # every hazy batch of both drivers was rendered by the kernel


def test_mode_synthesize_writes_the_tree(tree, tmp_path, monkeypatch):
    import main as M
    root, listing = tree
    out = str(tmp_path / "rendered")
    clear_dir, depth_dir = os.path.join(root, "val", "clear"), os.path.join(root, "val", "depth")
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.chdir(ROOT)
    monkeypatch.setattr(sys, "argv", ["main.py", "--mode", "synthesize", "--input", clear_dir, "--depth", depth_dir, "--output", out,
                                      "--seed", "9", "--device", DEV])
    M.main()
    with open(os.path.join(out, "synthesize.json")) as f:
        doc = json.load(f)
    assert doc["seed"] == 9 and doc["depth_range"] == [0.3, 1.0] and len(doc["files"]) == 3 * len(listing["val"])
    index = D.folder_index(out, "val")                                # the layout the stored-pair loader reads
    assert index.skipped == 0 and len(index) == 3 * len(listing["val"])
    stems = sorted(os.path.splitext(n)[0] + ".png" for n in listing["val"])
    assert [(r["intensity"], r["name"]) for r in index] == [(lab, n) for lab in range(3) for n in stems]
    rng = np.random.RandomState(9)
    by = {(r["level"], r["name"]): r for r in doc["files"]}
    for name in listing["val"]:
        stem = os.path.splitext(name)[0] + ".png"
        src = R.rgb3(IO.load_image(os.path.join(clear_dir, name)).numpy())
        lev = IO.load_depth(os.path.join(depth_dir, stem)).numpy()
        h, w = lev.shape
        beta, A = D.draw_fog_params(D.LEVEL_NAMES, rng)
        for k, level in enumerate(D.LEVEL_NAMES):
            rec = by[level, stem]
            assert rec["beta"] == float(np.float32(float(beta[k]))) and rec["airlight"] == float(np.float32(float(A[k])))
            (b0, b1), (a0, a1) = D.FOG_RANGES[level]
            assert b0 <= rec["beta"] <= b1 + 1e-6 and a0 <= rec["airlight"] <= a1 + 1e-6 and (rec["height"], rec["width"]) == (h, w)
            assert np.array_equal(R.rgb3(IO.load_image(os.path.join(out, level, "clear", stem)).numpy()), src)
            fog = torch.tensor([[rec["beta"], rec["airlight"]]], dtype=torch.float32)
            planes = D.batch_haze_from_windows(torch.from_numpy(src).to(DEV), torch.from_numpy(lev).to(DEV),
                                               torch.tensor([[0, w * 3, 0, w * 2]], dtype=torch.int64), fog, (h, w))
            hazy = IO.load_image(os.path.join(out, level, "hazy", stem)).numpy()
            assert np.array_equal(hazy, IO.image_to_u8(planes)[0].cpu().numpy()), (level, stem)
            assert np.abs(planes[0].cpu().double().numpy() - Z.haze_ref(src[None], lev[None], fog.numpy(), RANGE)[0]).max() <= Z.HAZE_BOUND
    with pytest.raises(SystemExit, match="--mode synthesize"):
        monkeypatch.setattr(sys, "argv", ["main.py", "--mode", "demo", "--input", clear_dir, "--depth", depth_dir])
        M.main()
    with pytest.raises(SystemExit, match="--input CLEAR_DIR"):
        monkeypatch.setattr(sys, "argv", ["main.py", "--mode", "synthesize"])
        M.main()
