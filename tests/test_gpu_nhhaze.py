"""Patchy, wavelength-dependent haze on the GPU: adh_batch_nhhaze_from_u8 through the C ABI over the table of
tests/_nhhaze_ref64.py with the contracts of the host-emulated run (guard bytes around both caches and the output), the identities
(a)-(d) of tests/test_nhhaze_hostemu_cpu.py on the device, and `dataset.synthetic_haze.nonuniform` / `.chromatic` end to end:
the loader, the shards, a driver, and `main.py --mode synthesize --nonuniform --chromatic`."""
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
from tests import _nhhaze_ref64 as NH
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
CROP = 24


def _bits(t):
    return t.contiguous().view(torch.int32)


def _guarded(arr, base):
    """the array's bytes on the device with GUARD + base filler bytes in front and GUARD behind -> (host copy, device, offset)"""
    a = np.ascontiguousarray(arr).view(np.uint8).reshape(-1)
    host = torch.from_numpy(np.concatenate([np.full(GUARD + base, FILL, np.uint8), a, np.full(GUARD, FILL, np.uint8)]))
    return host, host.to(DEV), GUARD + base


def _out(N, CH, CW, out_off):
    n, at = N * 3 * CH * CW, FRONT + out_off
    return torch.full((at + n + 64,), SENTINEL, dtype=torch.float32, device=DEV), at, n


def _call(name, clear, depth, geom_dev, mid, pd, crop, out_off=0):
    """a haze entry point; clear / depth = (device buffer, offset, bytes) or None; `mid`: the device tensors between geom and the
    depth range (fog; or fog6 and field).  The output stands FRONT + out_off floats into a buffer of sentinels with 64 more behind;
    returns [N,3,CH,CW] after checking that the sentinels stand"""
    (CH, CW), N = crop, geom_dev.shape[0]
    nblk = H.value("adh_batch_num_blocks", CH * CW)
    out, at, n = _out(N, CH, CW, out_off)
    partial = torch.zeros(N * nblk, dtype=torch.float64, device=DEV)
    dptr, dbytes = (None, 0) if depth is None else (depth[0].data_ptr() + depth[1], depth[2])
    H.call(name, clear[0].data_ptr() + clear[1], clear[2], dptr, dbytes, geom_dev.data_ptr(), *[m.data_ptr() for m in mid],
           RANGE[0], RANGE[1], H.ptr(pd), N, CH, CW, partial.data_ptr(), nblk, out.data_ptr() + 4 * at)
    assert (out[:at] == SENTINEL).all() and (out[at + n:] == SENTINEL).all(), "a float outside the output was written"
    return out[at:at + n].view(N, 3, CH, CW)


def _nh(clear, depth, gd, fog6, field, pd, crop, out_off=0):
    return _call("adh_batch_nhhaze_from_u8", clear, depth, gd, (fog6, field), pd, crop, out_off)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ------------------------------------------------------------------------------------------------ kernel
@pytest.mark.parametrize("radial", [False, True], ids=["depth", "radial"])
@pytest.mark.parametrize("no", range(len(NH.CASES)), ids=[c["name"] for c in NH.CASES])
def test_cases_on_the_device(no, radial):
    case = NH.CASES[no]
    clear, depth, geom, dclear, ddepth, fog, fog6, field = NH.build(case)
    crop, out_off = case["crop"], case["out_off"]
    N = len(geom)
    chost, cdev, coff = _guarded(clear, case["base"])
    dhost, ddev, doff = _guarded(depth, case["dbase"])
    cw = (cdev, coff, clear.size)
    dw = None if radial else (ddev, doff, depth.size * 2)
    dense_c = (_dev(dclear), 0, dclear.size)
    dense_d = None if radial else (_dev(ddepth), 0, ddepth.size * 2)
    gd, dgd = _dev(geom), _dev(Z.dense_geom(N, *crop))
    f6, q, f2, g6 = _dev(fog6), _dev(field), _dev(fog), _dev(NH.grey(fog))
    q0 = q.clone()
    q0[:, 4] = 0                                                      # s = 0
    z6 = f6.clone()
    z6[:, :3] = 0                                                     # beta_c = 0
    wt = torch.from_numpy(np.ascontiguousarray(geom[:, :2]))
    for params in [None] + K.param_sets(no + int(radial), N, 1):
        pt = None if params is None else torch.from_numpy(params)
        pd = None if params is None else pt.to(DEV)
        got = _nh(cw, dw, gd, f6, q, pd, crop, out_off)
        ref = NH.nhhaze_ref(dclear, None if radial else ddepth, fog6, field, RANGE, params)
        err = float(np.abs(got.cpu().double().numpy() - ref).max())
        bound = NH.NH_BOUND if params is None else NH.NH_AUG_BOUND
        print(f"{case['name']} radial={radial} rows={params is not None}: max err {err / Z.EPS:.3f} * 2^-24, bound {bound / Z.EPS:.3f}")
        assert float(got.min()) >= 0.0 and float(got.max()) <= 1.0
        assert err <= bound
        assert torch.equal(_bits(_nh(cw, dw, gd, f6, q, pd, crop, out_off)), _bits(got)), "a second call differs"
        assert torch.equal(_bits(_nh(dense_c, dense_d, dgd, f6, q, pd, crop)), _bits(got)), "differs from dense geometry"
        old = _call("adh_batch_haze_from_u8", cw, dw, gd, (f2,), pd, crop, out_off)
        assert torch.equal(_bits(_nh(cw, dw, gd, g6, q0, pd, crop, out_off)), _bits(old)), "(a) s = 0, equal channels"
        plain = D.batch_from_windows(cdev[coff:coff + clear.size], wt, crop, pt)
        assert torch.equal(_bits(_nh(cw, dw, gd, z6, q, pd, crop, out_off)), _bits(plain)), "(d) beta = 0 differs from the clear window"
        if params is None:
            flat = _nh(cw, dw, gd, f6, q0, None, crop, out_off)
            for c in range(3):
                one = _call("adh_batch_haze_from_u8", cw, dw, gd, (f6[:, [c, 3 + c]].contiguous(),), None, crop, out_off)
                assert torch.equal(_bits(flat[:, c]), _bits(one[:, c])), f"(b) plane {c}"
        for n in range(N if N > 1 else 0):
            one = _nh(cw, dw, gd[n:n + 1].clone(), f6[n:n + 1].clone(), q[n:n + 1].clone(), None if pd is None else pd[n:n + 1].clone(),
                      crop, out_off)
            assert torch.equal(_bits(one[0]), _bits(got[n])), (case["name"], n, "alone differs")
        dview = None if radial else ddev[doff:doff + depth.size * 2].view(torch.uint16)       # the wrapper, on views of the buffers
        a = D.batch_nhhaze_from_windows(cdev[coff:coff + clear.size], dview, torch.from_numpy(geom), torch.from_numpy(fog6),
                                        torch.from_numpy(field), crop, pt, RANGE)
        assert tuple(a.shape) == (N, 3) + tuple(crop) and a.dtype == torch.float32 and torch.equal(_bits(a), _bits(got))
    assert torch.equal(cdev.cpu(), chost) and torch.equal(ddev.cpu(), dhost), "a cache or its guard bytes were written"


@pytest.mark.parametrize("name", ["5x7_bytes", "8x12_phases", "40x130"])
def test_crop_sees_the_image_field(name):
    """(c): every window of the case against the same pixels of its whole image; the image's origin is the table's (some near
    2^20), the window's that plus (y0, x0)"""
    case = [c for c in NH.CASES if c["name"] == name][0]
    clear, depth, geom, dclear, ddepth, fog, fog6, field = NH.build(case)
    CH, CW = case["crop"]
    _, cdev, coff = _guarded(clear, case["base"])
    _, ddev, doff = _guarded(depth, case["dbase"])
    cw, dw = (cdev, coff, clear.size), (ddev, doff, depth.size * 2)
    for n, (k, y0, x0) in enumerate(case["windows"]):
        h, w = case["images"][k]
        whole = field[n:n + 1].copy()
        row = whole.copy()
        row[0, 1:3] += (y0, x0)
        gi = geom[n:n + 1] - np.array([[(y0 * w + x0) * 3, 0, (y0 * w + x0) * 2, 0]])
        f6 = _dev(fog6[n:n + 1])
        win = _nh(cw, dw, _dev(geom[n:n + 1]), f6, _dev(row), None, (CH, CW))
        img = _nh(cw, dw, _dev(gi), f6, _dev(whole), None, (h, w))
        assert torch.equal(_bits(win[0]), _bits(img[0, :, y0:y0 + CH, x0:x0 + CW])), (name, n)


def test_extremes_and_refusals():
    CH, CW, N = 4, 8, 2
    clear = np.zeros((N, CH, CW, 3), np.uint8)
    clear[:, :, 4:] = 255
    depth = np.zeros((N, CH, CW), np.uint16)
    depth[:, 2:] = 65535
    fog6 = np.array([[1, 1, 1, 1, 1, 1], [1, 1, 1, 0, 0, 0]], np.float32)
    field = np.array([[5, 0, 0, 2, 0.99, 0.25], [6, 3, 1, 2, 0.99, 0.25]], np.float64)
    cd, dd = _dev(clear), _dev(depth)
    gd, fd, qd = _dev(Z.dense_geom(N, CH, CW)), _dev(fog6), _dev(field)
    for params in (None, np.array([[1, 0, 1, 1.1, 1.1], [0, 1, 0, 0.9, 1.1]], np.float32)):
        pd = None if params is None else _dev(params)
        for dwin, dref in (((dd, 0, depth.size * 2), depth), (None, None)):
            got = _nh((cd, 0, clear.size), dwin, gd, fd, qd, pd, (CH, CW))
            assert float(got.min()) >= 0 and float(got.max()) <= 1
            assert np.abs(got.cpu().double().numpy() - NH.nhhaze_ref(clear, dref, fog6, field, RANGE, params)).max() <= \
                (NH.NH_BOUND if params is None else NH.NH_AUG_BOUND)
    out = torch.zeros(N * 3 * CH * CW, device=DEV)
    part = torch.zeros(N, dtype=torch.float64, device=DEV)
    ok = dict(clear=cd.data_ptr(), cb=clear.size, depth=dd.data_ptr(), db=depth.size * 2, geom=gd.data_ptr(), fog=fd.data_ptr(),
              field=qd.data_ptr(), params=None, N=N, CH=CH, CW=CW, partial=part.data_ptr(), nblk=1, out=out.data_ptr())
    for change in (dict(clear=None), dict(geom=None), dict(fog=None), dict(field=None), dict(out=None),
                   dict(params=fd.data_ptr(), partial=None), dict(N=0), dict(N=65536), dict(CH=0), dict(CW=0), dict(nblk=2),
                   dict(cb=CH * CW * 3 - 1), dict(db=CH * CW * 2 - 1), dict(depth=dd.data_ptr() + 1)):
        a = dict(ok, **change)
        with pytest.raises(RuntimeError, match="ADH_E_ARG"):
            H.call("adh_batch_nhhaze_from_u8", a["clear"], a["cb"], a["depth"], a["db"], a["geom"], a["fog"], a["field"], 0.3, 1.0,
                   a["params"], a["N"], a["CH"], a["CW"], a["partial"], a["nblk"], a["out"])
    assert (out == 0).all()
    geom = torch.from_numpy(Z.dense_geom(N, CH, CW))
    with pytest.raises(ValueError, match="field row 1.*0.5"):         # the host checks the field before the device sees it
        D.batch_nhhaze_from_windows(cd, dd, geom, torch.from_numpy(fog6), torch.tensor([[1, 0, 0, 1, 0.5, 0.5], [1, 0, 0, 2, 0.5, 0.5]],
                                                                                        dtype=torch.float64), (CH, CW))


# ------------------------------------------------------------------------------------------------ end to end
@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    """train / val with 6 / 4 clear files and their depth maps; the caches start empty"""
    root = str(tmp_path_factory.mktemp("nhhaze_folders"))
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


def _cached(ds, k):
    if ds.crop is None:
        return ds.clear[k].cpu().numpy(), ds.depth[k].cpu().numpy()
    h, w = ds.sizes[k].tolist()
    c = ds.clear[int(ds.offsets[k]):int(ds.offsets[k]) + h * w * 3].cpu().numpy().reshape(h, w, 3)
    at = int(ds.depth_offsets[k]) // 2
    return c, ds.depth[at:at + h * w].cpu().numpy().reshape(h, w)


SETTINGS = {"nonuniform": dict(nonuniform={}), "chromatic": dict(chromatic={"angstrom": [0.5, 1.3], "tint": 0.04}),
            "both": dict(nonuniform={"amplitude": [0.3, 0.9], "octaves": 2}, chromatic={})}


@pytest.mark.parametrize("which", list(SETTINGS))
@pytest.mark.parametrize("crop", [None, CROP], ids=["dense", "crop24"])
def test_batches_of_the_loader(tree, tmp_path, crop, which):
    root, listing = tree
    cfg = _cfg(root, tmp_path, crop, **SETTINGS[which])
    plain = _cfg(root, tmp_path, crop)
    seed, bs = int(cfg["seed"]), int(cfg["dataset"]["batch_size"])
    size = (32, 32) if crop is None else (CROP, CROP)
    loaders = {split: D.folder_loader(cfg, split, DEV) for split in ("train", "val")}
    ds = loaders["val"].dataset
    base = D.folder_loader(plain, "val", DEV).dataset
    assert base.clear is ds.clear and base.depth is ds.depth and base.nonuniform is None and base.chromatic is None   # shared caches
    nonuniform, chromatic = ds.nonuniform, ds.chromatic
    assert (nonuniform is None) == (which == "chromatic") and (chromatic is None) == (which == "nonuniform")
    # validation: the centre crop, no rows, draws that depend on the seed and the sample alone; two epochs are bit-identical
    first, second = list(loaders["val"](0)), list(loaders["val"](3))
    for a, b in zip(first, second):
        assert set(a) == {"hazy", "clear", "intensity", "beta", "airlight", "name", "beta_rgb", "airlight_rgb", "haze_field"}
        assert torch.equal(a["intensity"], b["intensity"]) and a["name"] == b["name"] and torch.equal(a["haze_field"], b["haze_field"])
        for key in ("hazy", "clear", "beta", "airlight", "beta_rgb", "airlight_rgb"):
            assert torch.equal(_bits(a[key]), _bits(b[key])), key
    b = first[0]
    n = len(b["name"])
    sizes = [_cached(ds, i)[0].shape[:2] for i in range(n)]
    origins = [((h - size[0]) // 2, (w - size[1]) // 2) for h, w in sizes]
    labels, fog, fog6, field = D.fixed_nh_params(seed, range(n), nonuniform, chromatic, sizes, origins)
    old_labels, old_fog = D.fixed_haze_params(seed, range(n))
    assert torch.equal(labels, old_labels) and torch.equal(fog, old_fog)      # (label, beta, A) are those without the settings
    assert b["intensity"].tolist() == labels.tolist() and torch.equal(b["beta"].cpu(), fog[:, 0]) and torch.equal(b["airlight"].cpu(), fog[:, 1])
    assert torch.equal(b["beta_rgb"].cpu(), fog6[:, :3]) and torch.equal(b["airlight_rgb"].cpu(), fog6[:, 3:])
    assert b["beta_rgb"].dtype == torch.float32 and str(b["beta_rgb"].device) == DEV and tuple(b["airlight_rgb"].shape) == (n, 3)
    assert torch.equal(b["haze_field"], field) and b["haze_field"].dtype == torch.float64 and not b["haze_field"].is_cuda
    assert torch.equal(b["beta_rgb"][:, 1], b["beta"])
    assert field[:, 1:3].tolist() == [[float(y), float(x)] for y, x in origins]
    if which == "chromatic":
        assert (field[:, 4] == 0).all()
    if which == "nonuniform":
        assert torch.equal(fog6[:, :3], fog[:, :1].expand(n, 3)) and torch.equal(fog6[:, 3:], fog[:, 1:].expand(n, 3))
    for i, name in enumerate(b["name"]):
        c, d = _cached(ds, i)
        (y0, x0) = origins[i]
        wc, wd = c[y0:y0 + size[0], x0:x0 + size[1]], d[y0:y0 + size[0], x0:x0 + size[1]]
        ref = NH.nhhaze_ref(wc[None], wd[None], fog6[i:i + 1].numpy(), field[i:i + 1].numpy(), RANGE)[0]
        assert np.abs(b["hazy"][i].cpu().double().numpy() - ref).max() <= NH.NH_BOUND, name
    # a 2-way shard covers every file once, under the draws of the whole split
    seen = {}
    for rank in (0, 1):
        for sb in D.folder_loader(cfg, "val", DEV, rank=rank, world=2)(1):
            for i, name in enumerate(sb["name"]):
                assert name not in seen
                seen[name] = (sb["beta_rgb"][i].cpu(), sb["haze_field"][i], sb["hazy"][i])
    assert sorted(seen) == sorted(listing["val"])
    for i, name in enumerate(b["name"]):
        assert torch.equal(seen[name][0], b["beta_rgb"][i].cpu()) and torch.equal(seen[name][1], b["haze_field"][i])
        assert torch.equal(_bits(seen[name][2]), _bits(b["hazy"][i]))
    # training: re-drawn from the seed in the documented order; within the float64 bound of the cache under the yielded rows
    ds, records = loaders["train"].dataset, D.haze_index(root, "train")
    rng = np.random.RandomState(seed)
    worst = 0.0
    for tb, s in zip(loaders["train"](0), D.epoch_plan(len(records), 1, 0, bs, seed, 0, True)):
        params = D.draw_augment_params(len(s), rng)
        origins = np.zeros((len(s), 2), np.int64) if crop is None else D.draw_crop_origins(ds.sizes[s], CROP, rng)
        labels, fog = D.draw_haze_params(len(s), rng)
        sizes = [(32, 32)] * len(s) if crop is None else ds.sizes[s]
        fog6, field = D.draw_nh_params(len(s), rng, nonuniform, chromatic, sizes, origins, fog)
        assert tb["intensity"].tolist() == labels.tolist() and torch.equal(tb["beta"].cpu(), fog[:, 0])
        assert torch.equal(tb["beta_rgb"].cpu(), fog6[:, :3]) and torch.equal(tb["airlight_rgb"].cpu(), fog6[:, 3:])
        assert torch.equal(tb["haze_field"], field)
        for i, k in enumerate(s.tolist()):
            c, d = _cached(ds, k)
            y0, x0 = origins[i].tolist()
            wc, wd = c[y0:y0 + size[0], x0:x0 + size[1]], d[y0:y0 + size[0], x0:x0 + size[1]]
            ref = NH.nhhaze_ref(wc[None], wd[None], fog6[i:i + 1].numpy(), field[i:i + 1].numpy(), RANGE, params[i:i + 1].numpy())[0]
            worst = max(worst, float(np.abs(tb["hazy"][i].cpu().double().numpy() - ref).max()))
    print(f"synthetic_haze {which} train: max |err| vs float64 {worst / Z.EPS:.3f} * 2^-24 (bound 9)")
    assert worst <= NH.NH_AUG_BOUND


def test_driver_trains_on_patchy_chromatic_haze(tree, tmp_path, monkeypatch):
    """crops of 24 x 24, so the LPIPS term is off (its AlexNet has no output under 31 x 31)"""
    root, listing = tree
    cfg = _cfg(root, tmp_path, CROP, nonuniform={}, chromatic={})
    cfg["loss"] = {"perceptual": False}
    shapes = set()
    real = D.batch_nhhaze_from_windows
    monkeypatch.setattr(D, "batch_nhhaze_from_windows", lambda *a, **k: (lambda x: shapes.add(tuple(x.shape[1:])) or x)(real(*a, **k)))
    monkeypatch.setattr(D, "batch_haze_from_windows", lambda *a, **k: pytest.fail("the uniform renderer was used"))
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        torch.manual_seed(3)
        model, losses = T.train_dehazing_model(cfg, "low", epochs=1)
    _no_synthetic(caught)
    assert 1 <= len(losses) <= 2 and all(np.isfinite(l) for l in losses)
    assert shapes == {(3, CROP, CROP)}


def test_mode_synthesize(tree, tmp_path, monkeypatch):
    import main as M
    root, listing = tree
    clear_dir, depth_dir = os.path.join(root, "val", "clear"), os.path.join(root, "val", "depth")
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.chdir(ROOT)
    out = str(tmp_path / "rendered")
    monkeypatch.setattr(sys, "argv", ["main.py", "--mode", "synthesize", "--input", clear_dir, "--depth", depth_dir, "--output", out,
                                      "--seed", "9", "--device", DEV, "--nonuniform", "--chromatic"])
    M.main()
    with open(os.path.join(out, "synthesize.json")) as f:
        doc = json.load(f)
    assert doc["nonuniform"]["octaves"] == 3 and doc["chromatic"]["tint"] == 0.05 and len(doc["files"]) == 3 * len(listing["val"])
    rng = np.random.RandomState(9)
    by = {(r["level"], r["name"]): r for r in doc["files"]}
    nu, ch = D._nh_settings("nonuniform", True), D._nh_settings("chromatic", True)
    for name in listing["val"]:
        stem = os.path.splitext(name)[0] + ".png"
        src = R.rgb3(IO.load_image(os.path.join(clear_dir, name)).numpy())
        lev = IO.load_depth(os.path.join(depth_dir, stem)).numpy()
        h, w = lev.shape
        beta, A = D.draw_fog_params(D.LEVEL_NAMES, rng)
        fog = torch.stack([beta, A], dim=1).to(torch.float32)
        fog6, field = D.draw_nh_params(3, rng, nu, ch, [(h, w)] * 3, None, fog)
        for k, level in enumerate(D.LEVEL_NAMES):
            rec = by[level, stem]
            assert rec["beta"] == float(fog[k, 0]) and rec["airlight"] == float(fog[k, 1])
            assert rec["beta_rgb"] == fog6[k, :3].tolist() and rec["airlight_rgb"] == fog6[k, 3:].tolist()
            assert rec["haze_field"] == field[k].tolist() and rec["haze_field"][1:3] == [0.0, 0.0]
            planes = D.batch_nhhaze_from_windows(torch.from_numpy(src).to(DEV), torch.from_numpy(lev).to(DEV),
                                                 torch.tensor([[0, w * 3, 0, w * 2]], dtype=torch.int64),
                                                 torch.tensor([rec["beta_rgb"] + rec["airlight_rgb"]], dtype=torch.float32),
                                                 torch.tensor([rec["haze_field"]], dtype=torch.float64), (h, w))
            hazy = IO.load_image(os.path.join(out, level, "hazy", stem)).numpy()
            assert np.array_equal(hazy, IO.image_to_u8(planes)[0].cpu().numpy()), (level, stem)
    # plain --mode synthesize: what synthesize_tree writes without the arguments, byte for byte
    a, b = str(tmp_path / "plain_cli"), str(tmp_path / "plain_call")
    monkeypatch.setattr(sys, "argv", ["main.py", "--mode", "synthesize", "--input", clear_dir, "--depth", depth_dir, "--output", a,
                                      "--seed", "9", "--device", DEV])
    M.main()
    D.synthesize_tree(clear_dir, b, depth_dir=depth_dir, seed=9, device=DEV)
    with open(os.path.join(a, "synthesize.json"), "rb") as fa, open(os.path.join(b, "synthesize.json"), "rb") as fb:
        assert fa.read() == fb.read()
    for level in D.LEVEL_NAMES:
        for role in ("hazy", "clear"):
            names = sorted(os.listdir(os.path.join(a, level, role)))
            assert names == sorted(os.listdir(os.path.join(b, level, role))) and len(names) == len(listing["val"])
            for nme in names:
                with open(os.path.join(a, level, role, nme), "rb") as fa, open(os.path.join(b, level, role, nme), "rb") as fb:
                    assert fa.read() == fb.read()
    with open(os.path.join(a, "synthesize.json")) as f:
        plain = json.load(f)
    assert set(plain) == {"seed", "depth_range", "files"} and set(plain["files"][0]) == {"file", "depth", "level", "name", "height",
                                                                                        "width", "beta", "airlight"}
    with pytest.raises(SystemExit, match="--mode synthesize"):
        monkeypatch.setattr(sys, "argv", ["main.py", "--mode", "demo", "--input", clear_dir, "--nonuniform"])
        M.main()
