"""Patchy, wavelength-dependent haze without a GPU: the float64 reference of tests/_nhhaze_ref64.py against itself (range, slope,
crop consistency), a pure-Python integer hash and tests/_haze_synth_ref64.haze_ref; the draws of `data.draw_nh_params`; every
refusal of `data.batch_nhhaze_from_windows` that comes before a device is asked for, of the config keys and of
`data.synthesize_tree`'s arguments."""
import numpy as np
import pytest
import torch

from adam_dehaze_amd import data as D
from tests import _haze_synth_ref64 as Z
from tests import _nhhaze_ref64 as NH


# ------------------------------------------------------------------------------------------------ the reference itself
def test_hash_known_answers():
    known = {(0, 0, 0, 0): 0x0, (1, 0, 0, 0): 0x6D523710, (0, 1, 0, 0): 0xC4A0E45C, (0, 0, 1, 0): 0xAA6F94B3,
             (0, 0, 0, 1): 0x688990C0, (3, 5, 2, 12345): 0xFDA69E14, (2 ** 20 + 7, 2 ** 20 - 3, 3, 2 ** 32 - 1): 0x92782DBD,
             (2 ** 31 - 1, 2 ** 31 - 1, 3, 7): 0x3A8C22E6}
    for (ix, iy, k, seed), h in known.items():
        assert NH.hash32_py(ix, iy, k, seed) == h
        assert int(NH.hash32(np.array([ix]), np.array([iy]), k, seed)[0]) == h
    rng = np.random.RandomState(0)
    ix, iy = rng.randint(0, 2 ** 31, 200), rng.randint(0, 2 ** 31, 200)
    for k, seed in ((0, 0), (3, 2 ** 32 - 1), (2, 99)):
        assert NH.hash32(ix, iy, k, seed).tolist() == [NH.hash32_py(int(a), int(b), k, seed) for a, b in zip(ix, iy)]


def test_field_range_mean_and_slope():
    f0 = float(np.float32(1 / 64))
    f = NH.field_ref(256, 384, (12345, 0, 0, 3, 0.5, f0))
    assert 0.0 <= f.min() < 0.25 and 0.75 < f.max() <= 1.0 and 0.4 < f.mean() < 0.6
    for K, f0, seed in ((3, f0, 12345), (1, 0.5, 1), (2, 0.25, 2), (4, 0.0625, 3), (4, float(np.float32(1 / 17)), 4)):
        f = NH.field_ref(64, 96, (seed, 5, 9, K, 0.0, f0))
        assert f.min() >= 0.0 and f.max() <= 1.0
        step = max(np.abs(np.diff(f, axis=0)).max(), np.abs(np.diff(f, axis=1)).max())
        assert step <= NH.slope_bound(K, f0) * (1 + 1e-12), (K, f0, step)
    means = [NH.field_ref(96, 96, (s, 0, 0, 3, 0.0, 1 / 48.0)).mean() for s in range(40)]
    assert abs(np.mean(means) - 0.5) < 0.03


def test_a_crop_sees_the_image_field_exactly():
    for row, (y0, x0) in (((12345, 0, 0, 3, 0.5, float(np.float32(1 / 64))), (100, 200)), ((7, 2 ** 20 - 3, 2 ** 20 + 1, 4, 0.5, 0.0625), (3, 5)),
                          ((9, 1, 2, 2, 0.5, 0.25), (2, 3)), ((9, 11, 13, 1, 0.5, 0.37), (17, 1))):
        whole = NH.field_ref(140, 260, row)
        seed, oy, ox, K, s, f0 = row
        crop = NH.field_ref(40, 50, (seed, oy + y0, ox + x0, K, s, f0))
        assert np.array_equal(crop, whole[y0:y0 + 40, x0:x0 + 50])


def test_reductions_to_the_uniform_model():
    rng = np.random.RandomState(4)
    N, CH, CW = 3, 6, 10
    clear = rng.randint(0, 256, size=(N, CH, CW, 3)).astype(np.uint8)
    depth = rng.randint(0, 65536, size=(N, CH, CW)).astype(np.uint16)
    fog = np.stack([rng.uniform(0.1, 1.0, N), rng.uniform(0.5, 1.0, N)], 1).astype(np.float32)
    rows = np.array([[1, 0, 0, 1.1, 0.9], [0, 1, 1, 0.9, 1.1], [1, 1, 0, 1.0, 0.9]], np.float32)
    field = np.array([[5, 3, 4, 2, 0.0, 0.25], [6, 0, 0, 3, 0.0, 0.1], [7, 9, 9, 1, 0.0, 0.5]], np.float64)
    fog6 = NH.chromatic(fog, [0.4, 1.3, 0.0], rng.uniform(-0.05, 0.05, (N, 3)))
    assert np.array_equal(fog6[:, 1], fog[:, 0])
    for d in (depth, None):
        for p in (None, rows):
            # s = 0, equal channels: the uniform model, exactly
            assert np.array_equal(NH.nhhaze_ref(clear, d, NH.grey(fog), field, (0.25, 1.5), p), Z.haze_ref(clear, d, fog, (0.25, 1.5), p))
        # s = 0, chromatic: plane c is the uniform model under (beta_c, A_c)
        got = NH.nhhaze_ref(clear, d, fog6, field, (0.25, 1.5))
        for c in range(3):
            assert np.array_equal(got[:, c], Z.haze_ref(clear, d, fog6[:, [c, 3 + c]], (0.25, 1.5))[:, c])
    # the field matters when s > 0, and scales the optical depth inside [1 - s, 1 + s]
    field[:, 4] = 0.9
    lo, hi = fog.copy(), fog.copy()
    lo[:, 0] *= np.float32(0.1)
    hi[:, 0] *= np.float32(1.9)
    got = NH.nhhaze_ref(clear, depth, NH.grey(fog), field)
    assert not np.array_equal(got, Z.haze_ref(clear, depth, fog))
    A = fog[:, 1].astype(np.float64)[:, None, None, None]
    d_lo, d_hi = np.abs(Z.haze_ref(clear, depth, lo) - A), np.abs(Z.haze_ref(clear, depth, hi) - A)
    assert (np.abs(got - A) <= d_lo + 1e-6).all() and (np.abs(got - A) >= d_hi - 1e-6).all()


def test_bounds_are_the_written_counts():
    assert NH.NH_F64_UNITS >= 2 * (72 + 5) * 4 * 16 + 644
    assert NH.NH_F64_UNITS * NH.U53 <= NH.NH_F64_CAP / 4 and 2 * NH.NH_F64_UNITS * NH.U53 <= NH.NH_F64_CAP
    assert NH.NH_BOUND == 2 * 2.0 ** -24 + NH.NH_F64_UNITS * 2.0 ** -53 and NH.NH_BOUND < 2.001 * 2.0 ** -24
    assert NH.NH_AUG_BOUND == 9 * 2.0 ** -24 + 2 * NH.NH_F64_UNITS * 2.0 ** -53 and NH.NH_AUG_BOUND < 9.001 * 2.0 ** -24


def test_field_rows_reach_every_path_and_pass_the_host_check():
    assert set(NH.FIELD_ROWS) == {c["name"] for c in NH.CASES}
    rows = [r for v in NH.FIELD_ROWS.values() for r in v]
    assert {r[3] for r in rows} == {1, 2, 3, 4} and min(r[4] for r in rows) == 0.0 and max(r[4] for r in rows) == 0.99
    assert any(r[1] > 2 ** 19 for r in rows) and any(r[2] > 2 ** 19 for r in rows)
    assert any(r[5] * 2 ** (r[3] - 1) == 0.5 for r in rows) and any(np.log2(r[5]) % 1 for r in rows)
    for case in NH.CASES:
        rows = NH.FIELD_ROWS[case["name"]]
        assert len(rows) == len(case["windows"])
        D.check_haze_field(torch.tensor(rows, dtype=torch.float64), len(rows), case["crop"])
        if case["crop"] in ((5, 7), (8, 12)):
            assert any(r[5] == 0.25 and r[3] == 2 and (r[1] % 4 or r[2] % 4) for r in rows)
    big = [r for r in NH.FIELD_ROWS["40x130"] if r[5] == 1 / 64 and r[3] == 3]
    assert len(big) == 2


# ------------------------------------------------------------------------------------------------ draws
NU = D._nh_settings("nonuniform", {})
CH = D._nh_settings("chromatic", {})


def test_defaults():
    assert NU == {"amplitude": (0.2, 0.8), "cell": (0.15, 0.5), "octaves": 3} and CH == {"angstrom": (0.0, 1.3), "tint": 0.05}
    assert D._nh_settings("nonuniform", None) is None and D._nh_settings("chromatic", True) == CH
    assert D._nh_settings("nonuniform", {"octaves": 2, "cell": [0.2, 0.2]}) == {"amplitude": (0.2, 0.8), "cell": (0.2, 0.2), "octaves": 2}


def test_draw_nh_params_order_and_ranges():
    n = 64
    sizes = np.array([(480, 640), (300, 200)] * (n // 2))
    origins = np.stack([np.arange(n), 2 * np.arange(n)], 1)
    for nu, ch in ((NU, CH), (NU, None), (None, CH)):
        rng = np.random.RandomState(11)
        labels, fog = D.draw_haze_params(n, rng)
        fog6, field = D.draw_nh_params(n, rng, nu, ch, sizes, origins, fog)
        plain = D.draw_haze_params(n, np.random.RandomState(11))
        assert torch.equal(labels, plain[0]) and torch.equal(fog, plain[1])       # (label, beta, A) do not depend on the settings
        assert fog6.dtype == torch.float32 and tuple(fog6.shape) == (n, 6) and field.dtype == torch.float64 and tuple(field.shape) == (n, 6)
        assert torch.equal(fog6[:, 1], fog[:, 0])                                 # green keeps beta
        assert float(fog6[:, 3:].min()) >= 0.0 and float(fog6[:, 3:].max()) <= 1.0
        assert field[:, 1:3].tolist() == origins.astype(np.float64).tolist()
        D.check_haze_field(field, n, (224, 224))
        again = np.random.RandomState(11)
        D.draw_haze_params(n, again)
        for i in range(n):
            beta, A = float(fog[i, 0]), float(fog[i, 1])
            if nu is not None:
                s, cell = again.uniform(0.2, 0.8), again.uniform(0.15, 0.5)
                f0 = float(np.float32(1.0 / (cell * float(sizes[i].min()))))      # the image's shorter side, not the crop's
                seed = int(again.randint(0, 2 ** 32))
                assert field[i].tolist() == [seed, origins[i, 0], origins[i, 1], 3, s, f0]
            else:
                assert field[i, 3:].tolist() == [1, 0.0, 0.5] and field[i, 0] == 0
            if ch is not None:
                alpha = again.uniform(0.0, 1.3)
                tint = again.uniform(-0.05, 0.05, 3)
                want = [beta * (610 / 550) ** -alpha, beta, beta * (465 / 550) ** -alpha] + np.clip(A + tint, 0, 1).tolist()
                assert np.allclose(fog6[i].numpy(), np.float32(want), rtol=0, atol=1e-7)
                assert fog6[i, 0] <= fog6[i, 1] <= fog6[i, 2]                     # blue scatters most
            else:
                assert fog6[i].tolist() == [fog[i, 0]] * 3 + [fog[i, 1]] * 3
    # a small image: f0 is capped where the finest cell would fall under 2 pixels
    rng = np.random.RandomState(2)
    fog6, field = D.draw_nh_params(8, rng, NU, None, [(32, 32)] * 8, None, torch.full((8, 2), 0.5))
    assert float((field[:, 5] * 4).max()) <= 0.5 and (field[:, 1:3] == 0).all()
    D.check_haze_field(field, 8, (32, 32))
    # A at the ends of [0, 1] stays inside
    fog6, _ = D.draw_nh_params(2, rng, None, CH, [(32, 32)] * 2, None, torch.tensor([[0.5, 1.0], [0.5, 0.0]]))
    assert float(fog6[:, 3:].min()) >= 0.0 and float(fog6[:, 3:].max()) <= 1.0
    empty = D.draw_nh_params(0, rng, NU, CH, np.zeros((0, 2)), None, torch.zeros(0, 2))
    assert tuple(empty[0].shape) == (0, 6) and tuple(empty[1].shape) == (0, 6)


def test_evaluation_draws_depend_on_seed_and_sample_alone():
    sizes = [(40, 56), (32, 32)] * 5
    origins = [(8, 16), (4, 4)] * 5
    a = D.fixed_nh_params(7, range(10), NU, CH, sizes, origins)
    b = D.fixed_nh_params(7, range(10), NU, CH, sizes, origins)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    labels, fog = D.fixed_haze_params(7, range(10))
    assert torch.equal(a[0], labels) and torch.equal(a[1], fog)
    # a shard (rank 1 of 2) sees the rows of its samples, whatever the epoch: nothing but (seed, sample) goes in
    own = list(range(1, 10, 2))
    part = D.fixed_nh_params(7, own, NU, CH, [sizes[g] for g in own], [origins[g] for g in own])
    for x, y in zip(part, a):
        assert torch.equal(x, y[own])
    other = D.fixed_nh_params(8, range(10), NU, CH, sizes, origins)
    assert not torch.equal(other[3], a[3])
    for g in range(10):
        rng = np.random.RandomState((7, g))
        lab, f2 = D.draw_haze_params(1, rng)
        f6, fld = D.draw_nh_params(1, rng, NU, CH, [sizes[g]], [origins[g]], f2)
        assert torch.equal(f6[0], a[2][g]) and torch.equal(fld[0], a[3][g])


# ------------------------------------------------------------------------------------------------ refusals on the host
def test_batch_nhhaze_from_windows_refuses_on_the_host():
    """CPU caches: every refusal that concerns the windows and the field comes before the one that asks for a device"""
    CH_, CW = 4, 6
    clear = torch.zeros(2 * 5 * 8 * 3, dtype=torch.uint8)            # two 5 x 8 images
    depth = torch.zeros(2 * 5 * 8, dtype=torch.uint16)
    geom = torch.tensor([[0, 24, 0, 16], [120 + 27, 24, 80 + 18, 16]], dtype=torch.int64)
    fog6 = torch.tensor([[0.5, 0.5, 0.6, 0.8, 0.8, 0.9]] * 2)
    good = [[3, 1, 2, 2, 0.5, 0.25], [4, 0, 0, 3, 0.0, 0.125]]

    def call(g=geom, c=clear, d=depth, f=fog6, q=good, crop=(CH_, CW), p=None, r=(0.3, 1.0)):
        q = q if isinstance(q, torch.Tensor) or q is None else torch.tensor(q, dtype=torch.float64)
        return D.batch_nhhaze_from_windows(c, d, g, f, q, crop, p, r)
    with pytest.raises(RuntimeError, match="no CPU fallback"):        # everything is in order but the device
        call()

    def row1(**kw):
        r = dict(seed=4, oy=0, ox=0, K=3, s=0.0, f0=0.125)
        r.update(kw)
        return [good[0], [r["seed"], r["oy"], r["ox"], r["K"], r["s"], r["f0"]]]
    for bad, text in ((row1(seed=-1), "seed"), (row1(seed=2.0 ** 32), "seed"), (row1(seed=1.5), "seed"), (row1(seed=float("nan")), "seed"),
                      (row1(oy=-1), "oy"), (row1(oy=0.5), "oy"), (row1(ox=-2), "ox"), (row1(ox=float("inf")), "ox"),
                      (row1(K=0), "K must"), (row1(K=5), "K must"), (row1(K=2.5), "K must"),
                      (row1(s=-0.1), "0 <= s < 1"), (row1(s=1.0), "0 <= s < 1"), (row1(s=float("nan")), "0 <= s < 1"),
                      (row1(f0=0.0), "f0 must"), (row1(f0=-0.1), "f0 must"), (row1(f0=float("inf")), "f0 must"), (row1(f0=float("nan")), "f0 must"),
                      (row1(f0=0.126), "0.5"), (row1(K=1, f0=0.51), "0.5"),
                      (row1(oy=2.0 ** 33, K=1, f0=0.5), "2\\^31"), (row1(ox=2.0 ** 33 - 6, K=1, f0=0.25), "2\\^31")):
        with pytest.raises(ValueError, match="field row 1.*" + text):
            call(q=bad)
    call_ok_edge = row1(ox=2.0 ** 33 - 7, K=1, f0=0.25)               # (ox + CW) * f0 = 2^31 - 0.25: still inside
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        call(q=call_ok_edge)
    for q in (None, torch.tensor(good, dtype=torch.float32), torch.tensor(good[:1], dtype=torch.float64), good[0]):
        with pytest.raises(TypeError, match="field must be a float64"):
            call(q=q if not isinstance(q, list) else torch.tensor(q, dtype=torch.float64))
    with pytest.raises(ValueError, match="fog6"):
        call(f=fog6[:, :2])
    with pytest.raises(ValueError, match="fog6"):
        call(f=fog6[:1])
    with pytest.raises(TypeError, match="geom"):
        call(g=geom.to(torch.int32))
    with pytest.raises(TypeError, match="caches"):
        call(c=None)
    with pytest.raises(ValueError, match="crop"):
        call(crop=(0, 4))
    with pytest.raises(ValueError, match="no windows"):
        call(g=geom[:0], f=fog6[:0], q=torch.zeros((0, 6), dtype=torch.float64))
    with pytest.raises(ValueError, match="params"):
        call(p=torch.zeros(2, 4))
    with pytest.raises(ValueError, match="depth_range"):
        call(r=(0.3, float("inf")))
    with pytest.raises(ValueError, match="even"):
        call(g=torch.tensor([[0, 24, 1, 16], [0, 24, 0, 16]], dtype=torch.int64))
    with pytest.raises(IndexError, match="clear cache"):
        call(g=torch.tensor([[0, 24, 0, 16], [240 - 24 * 3 - 17, 24, 0, 16]], dtype=torch.int64))
    with pytest.raises(IndexError, match="depth cache"):
        call(g=torch.tensor([[0, 24, 0, 16], [0, 24, 160 - 16 * 3 - 10, 16]], dtype=torch.int64))


def test_config_refusals(tmp_path):
    root = str(tmp_path / "data")
    Z.write_tree(root, splits=(("train", 2),))
    cfg = {"seed": 1, "dataset": {"train_path": root, "img_size": 32, "batch_size": 2, "synthetic_haze": {}}}
    for bad, err in (({"nonuniform": {"amplitude": [0.2, 1.0]}}, "nonuniform.amplitude"), ({"nonuniform": {"amplitude": [0.5, 0.2]}}, "nonuniform.amplitude"),
                     ({"nonuniform": {"amplitude": 0.5}}, "nonuniform.amplitude"), ({"nonuniform": {"amplitude": [-0.1, 0.5]}}, "nonuniform.amplitude"),
                     ({"nonuniform": {"cell": [0.0, 0.5]}}, "nonuniform.cell"), ({"nonuniform": {"cell": [0.5]}}, "nonuniform.cell"),
                     ({"nonuniform": {"cell": ["a", "b"]}}, "nonuniform.cell"),
                     ({"nonuniform": {"octaves": 0}}, "nonuniform.octaves"), ({"nonuniform": {"octaves": 5}}, "nonuniform.octaves"),
                     ({"nonuniform": {"octaves": 2.0}}, "nonuniform.octaves"), ({"nonuniform": {"octave": 2}}, "nonuniform: unknown keys"),
                     ({"nonuniform": [0.2, 0.8]}, "nonuniform must be a mapping"),
                     ({"chromatic": {"angstrom": [1.3, 0.0]}}, "chromatic.angstrom"), ({"chromatic": {"angstrom": [0.0, float("nan")]}}, "chromatic.angstrom"),
                     ({"chromatic": {"tint": -0.1}}, "chromatic.tint"), ({"chromatic": {"tint": 1.5}}, "chromatic.tint"),
                     ({"chromatic": {"tint": "x"}}, "chromatic.tint"), ({"chromatic": {"tints": 0.1}}, "chromatic: unknown keys"),
                     ({"chromatic": 3}, "chromatic must be a mapping"), ({"patchy": {}}, "unknown keys.*nonuniform, chromatic")):
        cfg["dataset"]["synthetic_haze"] = bad
        with pytest.raises(ValueError, match=err):
            D.folder_loader(cfg, "train", "cuda:0")


def test_synthesize_tree_argument_checks(tmp_path):
    src = tmp_path / "clear"
    src.mkdir()
    for kw, err in ((dict(nonuniform={"octaves": 9}), "synthesize.nonuniform.octaves"), (dict(chromatic={"tint": 2}), "synthesize.chromatic.tint"),
                    (dict(nonuniform="yes"), "nonuniform must be a mapping"), (dict(chromatic={"angstrom": [1, 0]}), "chromatic.angstrom")):
        with pytest.raises(ValueError, match=err):                    # before the device, the input directory or a file is looked at
            D.synthesize_tree(str(tmp_path / "missing"), str(tmp_path / "out"), device="cpu", **kw)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        D.synthesize_tree(str(src), str(tmp_path / "out"), device="cpu", nonuniform=True, chromatic=True)
    assert not (tmp_path / "out").exists()
