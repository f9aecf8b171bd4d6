"""csrc/nss.hip and adam-dehaze_amd/nss.py on the device: the moments and halved planes against the float64
reference of tests/_nss_ref64.py under its counted bounds (tests/_nss_cases.py; the counts must be equal, which the reference
itself is first checked to make fair), features and NIQE scores end to end, bit-equality, the refusals, and the demo path."""
import json
import os
import warnings

import numpy as np
import pytest
import torch

from adam_dehaze_amd import _hip as H
from adam_dehaze_amd import image_io as IO
from adam_dehaze_amd import metrics as M
from adam_dehaze_amd import nss as NSS
from adam_dehaze_amd import train as T
from tests import _nss_cases as K
from tests import _nss_ref64 as R
from tests._util import DEV, _pad_untouched, _padded, _same_bits, _twice

pytestmark = pytest.mark.gpu

NIQE_SHAPE = (96, 192, 96, 192, 96, 96)


def _moments(x, Hc, Wc, rh, rw):
    return _twice(lambda: (NSS.nss_moments(x, rh, rw, Hc, Wc),))[0]


@pytest.mark.parametrize("shape", K.MOMENT_SHAPES + [NIQE_SHAPE, K.MANY_TILES_GPU], ids=lambda s: "x".join(map(str, s)))
def test_moments_vs_float64_bit_equal_twice_and_alone(shape):
    Hh, Ww, Hc, Wc, rh, rw = shape
    if shape == NIQE_SHAPE:
        kinds = K.KINDS
    else:
        kinds = ("u8noise",) if shape == K.MANY_TILES_GPU else (K.KINDS[(K.MOMENT_SHAPES.index(shape) + 1) % 4],)
    for kind in kinds:
        for N in (1, 3):
            x, _, _ = K.moment_reference(kind, N, Hh, Ww, Hc, Wc, rh, rw)
            xd = x.to(DEV)
            got = _moments(xd, Hc, Wc, rh, rw)
            ratio = K.check_moments(got.cpu(), kind, N, Hh, Ww, Hc, Wc, rh, rw)
            print(f"{kind} {N}x3x{Hh}x{Ww} crop {Hc}x{Wc} regions {rh}x{rw}: worst |err| / bound {ratio:.3g}")
            assert ratio <= 1.0
            if N == 3:                                       # image i alone is image i of the batch, bit for bit
                alone = NSS.nss_moments(xd[1:2].contiguous(), rh, rw, Hc, Wc)
                assert _same_bits(alone, got[1:2])


@pytest.mark.parametrize("Hh,Ww", K.HALVE_SIDES + [(96, 192)])
def test_halved_planes_vs_float64(Hh, Ww):
    for N in (1, 3):
        x, Y, ref, bound = K.halve_reference("u8noise", N, Hh, Ww, Hh, Ww)
        a, b = _twice(lambda: (NSS.nss_halve(x.to(DEV)), NSS.nss_halve(Y.to(DEV))))
        assert tuple(a.shape) == (N, (Hh + 1) // 2, (Ww + 1) // 2)
        ratio = max(K.worst(a.cpu(), ref, bound), K.worst(b.cpu(), ref, bound))
        print(f"halve {N}x{Hh}x{Ww}: worst |err| / bound {ratio:.3g}")
        assert ratio <= 1.0


def test_second_scale_of_a_crop():
    """100 x 200 cropped to 96 x 192, halved to 48 x 96, moments in 48 x 48 regions: the plane the kernel halved, held to the
    reference's plane with the halving's bound as the pixels' own error"""
    for kind in ("u8noise", "ramp"):
        x, Y, ref, bound = K.halve_reference(kind, 3, 100, 200, 96, 192)
        y2 = NSS.nss_halve(x.to(DEV), 96, 192)
        assert K.worst(y2.cpu(), ref, bound) <= 1.0
        got = _moments(y2, 48, 96, 48, 48)
        mb, taus, ps = R.moment_bounds(ref, 48, 48, R.flat_windows(ref), dY=bound)
        for tau, p in zip(taus, ps):
            assert bool((p.abs()[p != 0] > tau[p != 0]).all()), "a bad case"
        ratio = K.worst(got.cpu(), R.moments(ref, 48, 48), mb)
        print(f"second scale {kind}: worst |err| / bound {ratio:.3g}")
        assert ratio <= 1.0


def test_outputs_stay_inside_their_tensors():
    x = K.inputs("uniform", 2, 23, 45).to(DEV)
    nt = K.tiles(10, 40)
    wp, partial = _padded(2 * 2 * nt * 24, dtype=torch.float64)
    wo, out = _padded(2 * 2 * 24, dtype=torch.float64)
    wd, dst = _padded(2 * 10 * 20, dtype=torch.float64)
    H.call("adh_nss_moments", x.data_ptr(), 1, 2, 23, 45, 20, 40, 10, 40, partial.data_ptr(), nt, out.data_ptr())
    H.call("adh_nss_halve", x.data_ptr(), 1, 2, 23, 45, 20, 40, dst.data_ptr())
    torch.cuda.synchronize()
    assert _pad_untouched(wp, partial.numel()) and _pad_untouched(wo, out.numel()) and _pad_untouched(wd, dst.numel())
    assert not torch.isnan(out).any() and not torch.isnan(dst).any() and not torch.isnan(partial).any()


@pytest.mark.parametrize("kind,seed", [("u8noise", 0), ("ramp", 0), ("halfflat", 0)])
def test_features_end_to_end(kind, seed):
    Hh, Ww = 96, 192
    x = K.inputs(kind, 3, Hh, Ww, seed)
    xd = x.to(DEV)
    Y = R.grey(x)
    # NIQE: patches at both scales
    f, sh = NSS.niqe_patch_features(xd)
    assert tuple(f.shape) == (3, 2, 36) and tuple(sh.shape) == (3, 2)
    f = f.cpu().view(3, 1, 2, 36)
    m1 = NSS.nss_moments(xd, 96, 96).cpu()
    _, r1, b1 = K.moment_reference(kind, 3, Hh, Ww, Hh, Ww, 96, 96, seed)
    edge = K.check_features(f[..., :18], m1, r1, b1, 96 * 96)
    y2 = NSS.nss_halve(xd)
    Y2, hb = R.halve(Y), R.halve_bound(Y)
    b2, _, _ = R.moment_bounds(Y2, 48, 48, R.flat_windows(Y2), dY=hb)
    edge += K.check_features(f[..., 18:], NSS.nss_moments(y2, 48, 48).cpu(), R.moments(Y2, 48, 48), b2, 48 * 48)
    assert bool(((sh.cpu().view(3, 1, 2) - r1[..., 2] / 9216.0).abs() <= b1[..., 2] / 9216.0).all())
    # BRISQUE: the whole plane at both scales
    g = NSS.brisque_features(xd).cpu()
    assert tuple(g.shape) == (3, 36)
    _, rw1, bw1 = K.moment_reference(kind, 3, Hh, Ww, Hh, Ww, Hh, Ww, seed)
    edge += K.check_features(g[:, :18].view(3, 1, 1, 18), NSS.nss_moments(xd, Hh, Ww).cpu(), rw1, bw1, Hh * Ww)
    bw2, _, _ = R.moment_bounds(Y2, 48, 96, R.flat_windows(Y2), dY=hb)
    edge += K.check_features(g[:, 18:].view(3, 1, 1, 18), NSS.nss_moments(y2, 48, 96).cpu(), R.moments(Y2, 48, 96), bw2, 48 * 96)
    print(f"features {kind}: {edge} alpha(s) on a decision point")
    assert edge <= 1, "more than one alpha of the case sits on a decision point: choose another seed"
    ref = R.brisque_features(x)
    fin = ~torch.isnan(ref)
    assert float((g - ref).abs()[fin].max()) <= 0.001 + 1e-9             # and plainly: the same 36 numbers


def test_niqe_scores_end_to_end():
    x = K.inputs("u8noise", 3, 96, 288).to(DEV)
    y = K.inputs("ramp", 2, 100, 200).to(DEV)
    model = NSS.NiqeModel.fit([x], sharpness_threshold=0.75)
    fx, shx = (t.cpu() for t in NSS.niqe_patch_features(x))
    mu, cov, rows = R.niqe_model(list(fx.numpy()), list(shx.numpy()))
    assert model.meta["images"] == 3 and model.meta["patches"] == rows
    assert float(np.abs(model.mu - mu).max()) <= 1e-12 * float(np.abs(mu).max())
    assert float(np.abs(model.cov - cov).max()) <= 1e-12 * float(np.abs(cov).max())
    scores = M.niqe_batch(y, model)
    fy = NSS.niqe_patch_features(y)[0].cpu().numpy()
    assert fy.shape == (2, 2, 36)
    for s, f in zip(scores, fy):                             # the formula written out, on the kernel's features
        want = R.niqe_distance(model.mu, model.cov, f)
        assert s is not None and s > 0 and abs(s - want) <= 1e-9 * want
    assert M.niqe_batch(y[:1].contiguous(), model)[0] == scores[0]       # image i alone
    one = NSS.NiqeModel.fit([x[:1].contiguous()], sharpness_threshold=0.0)
    assert M.niqe_batch(x[:1].contiguous(), one) == [0.0]
    assert M.niqe_batch(torch.rand(2, 3, 64, 64, device=DEV), model) == [None, None]
    assert M.niqe_batch(torch.full((1, 3, 96, 192), 0.25, device=DEV), model) == [None]       # constant: NaN features
    f = NSS.brisque_features(torch.full((1, 3, 40, 40), 0.25, device=DEV))
    assert bool(torch.isnan(f[:, list(R.ALPHA_COLUMNS)]).all())


def test_brisque_batch_is_the_closed_form_on_the_features(tmp_path):
    (tmp_path / "allmodel").write_text(K.SVR_MODEL)
    svr = NSS.SvrModel.load(str(tmp_path / "allmodel"))
    x = K.inputs("u8noise", 2, 40, 52).to(DEV)
    got = M.brisque_batch(x, svr)
    want = svr.predict(NSS.brisque_features(x).cpu()).tolist()
    assert all(abs(a - b) <= 1e-12 for a, b in zip(got, want))
    assert M.brisque_batch(torch.full((1, 3, 40, 40), 0.5, device=DEV), svr) == [None]


def test_refusals():
    x = K.inputs("uniform", 1, 12, 16).to(DEV)
    wp, partial = _padded(24, dtype=torch.float64)
    wo, out = _padded(24, dtype=torch.float64)

    def rejected(name, *args):
        with pytest.raises(RuntimeError, match="ADH_E_ARG"):
            H.call(name, *args)
    ok = [x.data_ptr(), 1, 1, 12, 16, 12, 16, 12, 16, partial.data_ptr(), 1, out.data_ptr()]
    for i, v in ((0, None), (9, None), (11, None), (1, 2), (2, 0), (5, 13), (6, 17), (7, 5), (8, 5), (10, 2), (11, x.data_ptr()),
                 (9, x.data_ptr()), (9, out.data_ptr())):
        rejected("adh_nss_moments", *(ok[:i] + [v] + ok[i + 1:]))
    okh = [x.data_ptr(), 1, 1, 12, 16, 12, 16, out.data_ptr()]
    for i, v in ((0, None), (7, None), (1, 3), (2, 0), (5, 13), (6, 17), (7, x.data_ptr())):
        rejected("adh_nss_halve", *(okh[:i] + [v] + okh[i + 1:]))
    torch.cuda.synchronize()
    assert bool(torch.isnan(wp).all()) and bool(torch.isnan(wo).all())
    with pytest.raises(ValueError, match="at least 96x96"):
        NSS.niqe_patch_features(torch.rand(1, 3, 95, 200, device=DEV))
    with pytest.raises(ValueError, match="do not tile"):
        NSS.nss_moments(x, 5, 16)
    with pytest.raises(RuntimeError, match=r"\[N,3,H,W\]"):
        NSS.brisque_features(torch.rand(1, 1, 40, 40, device=DEV))
    with pytest.raises(RuntimeError, match="float32"):
        NSS.brisque_features(torch.rand(1, 3, 40, 40, device=DEV, dtype=torch.float64))


# ------------------------------------------------------------------------------------------------ demo
BASE_KEYS = {"file", "height", "width", "routing", "weights", "intensity"}
NOREF = {"niqe", "hazy_niqe", "brisque", "hazy_brisque"}


@pytest.fixture(scope="module")
def demo(tmp_path_factory):
    """files of 96 x 192 (two), 100 x 200 (cropped) and 64 x 64 (niqe: null) through fit_niqe_model and run_demo"""
    Image = pytest.importorskip("PIL.Image")
    from tests.test_gpu_demo_scores import _cfg
    hazy, clear, models = (tmp_path_factory.mktemp(n) for n in ("hazy", "clear", "models"))
    g = np.random.default_rng(7)
    for name, (h, w) in (("a.png", (96, 192)), ("b.png", (96, 192)), ("c.png", (100, 200)), ("s.png", (64, 64))):
        gt = g.integers(0, 256, (h, w, 3), dtype=np.uint8)
        hz = np.clip(gt.astype(np.int32) // 2 + 100 + g.integers(-8, 9, gt.shape), 0, 255).astype(np.uint8)
        Image.fromarray(gt).save(clear / name)
        Image.fromarray(hz).save(hazy / name)
    (models / "allmodel").write_text(K.SVR_MODEL)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                       # s.png is under 96 px: skipped with a warning
        fitted = T.fit_niqe_model(_cfg(), str(clear), str(models / "niqe.npz"))
    torch.manual_seed(11)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        system = T._joint_system_for_evaluation(_cfg())[0]
    flags = {"niqe": str(models / "niqe.npz"), "brisque_model": str(models / "allmodel")}
    runs = {}
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(T, "_joint_system_for_evaluation", lambda config: (system, None))
        for key, kw in (("off", {}), ("on", flags), ("off_target", {"target": str(clear)}),
                        ("on_target", dict(flags, target=str(clear))), ("niqe_only", {"niqe": flags["niqe"]})):
            out = tmp_path_factory.mktemp("demo_" + key)
            runs[key] = (out, T.run_demo(_cfg(), str(hazy), str(out), False, **kw))
    return hazy, models, fitted, runs


def test_fitted_model_file(demo):
    _, models, fitted, _ = demo
    m = NSS.NiqeModel.load(str(models / "niqe.npz"))
    assert m.meta == fitted.meta and m.meta["images"] == 3 and 2 <= m.meta["patches"] <= 6
    assert bool((m.mu == fitted.mu).all()) and bool((m.cov == fitted.cov).all())


def test_demo_records_and_means(demo):
    hazy, models, fitted, runs = demo
    svr = NSS.SvrModel.load(str(models / "allmodel"))
    planes = lambda path: IO.u8_to_image(IO.load_image(str(path)).to(DEV))
    for key, extra in (("on", set()), ("on_target", {"target", "scored"} | set(IO.SCORE_KEYS))):
        out, results = runs[key]
        assert len(results) == 4
        for r in results:
            name = os.path.basename(r["file"])
            assert set(r) == BASE_KEYS | NOREF | extra
            for prefix, img in (("", planes(out / name)), ("hazy_", planes(hazy / name))):
                assert r[prefix + "niqe"] == M.niqe_batch(img, fitted)[0]          # recomputed from the files alone
                assert r[prefix + "brisque"] == M.brisque_batch(img, svr)[0]
            assert (r["niqe"] is None) == (name == "s.png") and r["brisque"] is not None
        assert json.load(open(out / "demo_results.json")) == results
        s = json.load(open(out / "demo_noref.json"))
        for side, prefix in (("dehazed", ""), ("hazy", "hazy_")):
            al = s[side]["all"]
            assert al["samples"] == 4 and al["niqe_null"] == 1 and "brisque_null" not in al
            have = [r[prefix + "niqe"] for r in results if r[prefix + "niqe"] is not None]
            assert abs(al["niqe"] - sum(have) / 3) <= 1e-12 and abs(al["brisque"] - sum(r[prefix + "brisque"] for r in results) / 4) <= 1e-12
        assert os.path.exists(out / "demo_scores.json") == (key == "on_target")
    out, results = runs["niqe_only"]
    assert all(set(r) == BASE_KEYS | {"niqe", "hazy_niqe"} for r in results)
    assert set(json.load(open(out / "demo_noref.json"))["hazy"]["all"]) == {"niqe", "niqe_null", "samples"}


def test_demo_without_the_flags_is_todays(demo):
    _, _, _, runs = demo
    for off, on in (("off", "on"), ("off_target", "on_target")):
        out_off, res_off = runs[off]
        out_on, res_on = runs[on]
        assert not os.path.exists(out_off / "demo_noref.json")
        stripped = [{k: v for k, v in r.items() if k not in NOREF} for r in res_on]
        # byte-equal apart from the added keys (and the output directory has no part in a record)
        assert json.dumps(stripped, indent=2) == open(out_off / "demo_results.json").read()
        for name in ("a.png", "c.png", "s.png"):
            assert open(out_off / name, "rb").read() == open(out_on / name, "rb").read()
        if off == "off_target":
            assert open(out_off / "demo_scores.json").read() == open(out_on / "demo_scores.json").read()
