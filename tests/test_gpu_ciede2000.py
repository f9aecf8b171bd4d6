"""csrc/ciede2000.hip on the GPU against the float64 reference of tests/_ref64_ciede.py, to 5e-6 absolute on the map and on
the mean (tests/_ciede_cases.py derives the bound), plus what the contract promises: both access widths give the same bits, a
missing map changes nothing, the result of an image does not depend on its batch, nothing outside the outputs is written and
every refusal launches nothing."""
import json
import math

import numpy as np
import pytest
import torch

from adam_dehaze_amd import _hip as H
from adam_dehaze_amd import metrics as M
from tests import _ciede_cases as K

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ADH_E_ARG = -1


def _nb(pixels):
    return H.value("adh_ciede2000_num_blocks", pixels)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _check(a, b, lab=False, what=""):
    mean, dmap = M.ciede2000_batch(a.to(DEV), b.to(DEV), lab_input=lab, return_map=True)
    ref_map, ref_mean = K.reference(a, b, lab)
    assert dmap.shape == ref_map.shape and dmap.dtype == torch.float32 and mean.dtype == torch.float32 and mean.is_cuda
    e_map = float(np.abs(dmap.double().cpu().numpy() - ref_map).max())
    e_mean = float(np.abs(mean.double().cpu().numpy() - ref_mean).max())
    print(f"{what}: |map - ref| <= {e_map:.3e}, |mean - ref| <= {e_mean:.3e} (bound {K.TOL:.0e}); largest dE00 {ref_map.max():.3f}")
    assert not torch.isnan(dmap).any() and not torch.isnan(mean).any()
    assert e_map <= K.TOL and e_mean <= K.TOL, what
    return mean, dmap


def test_published_pairs_as_one_lab_image():
    a, b, table = K.sharma_image()
    _, dmap = _check(a, b, True, "published pairs (2 x 7, lab_input)")
    assert float(np.abs(dmap[0].double().cpu().numpy() - table).max()) <= 5e-5 + K.TOL
    ka, kb = K.knife_edge_image()
    _, edge = M.ciede2000_batch(ka.to(DEV), kb.to(DEV), lab_input=True, return_map=True)
    print("hues 180 degrees apart (printed, not asserted):", [f"{v:.7f}" for v in edge.reshape(-1).tolist()], "reference",
          [f"{v:.7f}" for v in K.reference(ka, kb, True)[0].reshape(-1)])


@pytest.mark.parametrize("N,H_,W", K.SHAPES)
def test_random_srgb_pairs(N, H_, W):
    a, b = K.rgb_pair(N, H_, W, seed=H_ * 131 + W)
    _check(a, b, False, f"{N}x{H_}x{W}")


@pytest.fixture(scope="module")
def ragged():
    N, H_, W = K.ragged_shape(_nb)
    a, b = K.rgb_pair(N, H_, W, seed=7)
    return a, b


def test_three_workgroups_with_a_ragged_last_one(ragged):
    a, b = ragged
    assert _nb(a.shape[2] * a.shape[3]) == 3
    _check(a, b, False, f"{tuple(a.shape)}: three workgroups per image")


def test_input_one_float_into_a_larger_allocation():
    for H_, W in ((16, 20), (7, 9)):
        a, b = K.rgb_pair(2, H_, W, seed=3)
        n = a.numel()
        big_a, big_b = torch.zeros(n + 1, device=DEV), torch.zeros(n + 1, device=DEV)
        ua, ub = big_a[1:].view_as(a), big_b[1:].view_as(b)
        ua.copy_(a)
        ub.copy_(b)
        assert ua.data_ptr() % 16 == 4 and ua.is_contiguous()
        mean_u, map_u = M.ciede2000_batch(ua, ub, return_map=True)
        mean_a, map_a = M.ciede2000_batch(a.to(DEV), b.to(DEV), return_map=True)
        ref_map, ref_mean = K.reference(a, b)
        assert float(np.abs(map_u.double().cpu().numpy() - ref_map).max()) <= K.TOL
        assert float(np.abs(mean_u.double().cpu().numpy() - ref_mean).max()) <= K.TOL
        # single floats and 16-byte accesses: the same pixels per lane and the same order of the sums
        assert torch.equal(_bits(map_u), _bits(map_a)) and torch.equal(_bits(mean_u), _bits(mean_a))


def test_crafted_pixels():
    a, b, names = K.crafted_lab()
    _, dmap = _check(a, b, True, "crafted Lab pairs")
    for k, name in enumerate(names):
        print(f"  {name}: {float(dmap[0, 0, k]):.6f}")
        if name.startswith("equal"):
            assert float(dmap[0, 0, k]) == 0.0, name
    a, b, names = K.crafted_rgb()
    _, dmap = _check(a, b, False, "crafted sRGB pairs")
    for k, name in enumerate(names):
        print(f"  {name}: {float(dmap[0, 0, k]):.6f}")
    assert float(dmap[0, 0, names.index("equal")]) == 0.0
    assert float(dmap[0, 0, names.index("all NaN against black")]) == 0.0
    assert abs(float(dmap[0, 0, names.index("black against white")]) - 100.0000002) <= K.TOL


def test_mean_without_map_twice_and_out_of_a_batch(ragged):
    a, b = ragged
    a3, b3 = torch.cat([a, a[:1].flip(-1)]).to(DEV), torch.cat([b, b[:1]]).to(DEV)          # N = 3
    mean, dmap = M.ciede2000_batch(a3, b3, return_map=True)
    assert torch.equal(_bits(M.ciede2000_batch(a3, b3)), _bits(mean)), "map = NULL changes the mean"
    again, dmap2 = M.ciede2000_batch(a3, b3, return_map=True)
    assert torch.equal(_bits(again), _bits(mean)) and torch.equal(_bits(dmap2), _bits(dmap)), "two calls differ"
    for i in range(3):
        m1, d1 = M.ciede2000_batch(a3[i:i + 1], b3[i:i + 1], return_map=True)
        assert torch.equal(_bits(m1), _bits(mean[i:i + 1])) and torch.equal(_bits(d1), _bits(dmap[i:i + 1])), i
    # the mean against the float64 mean of the reference map
    ref_map, _ = K.reference(a3.cpu(), b3.cpu())
    want = np.array([math.fsum(ref_map[i].reshape(-1).tolist()) / ref_map[i].size for i in range(3)])
    assert float(np.abs(mean.double().cpu().numpy() - want).max()) <= K.TOL


def test_nothing_outside_the_outputs_is_written():
    N, H_, W = 2, 8, 10
    a, b = K.rgb_pair(N, H_, W, seed=9)
    a, b = a.to(DEV), b.to(DEV)
    nblk = _nb(H_ * W)
    partial = torch.empty(N * nblk, device=DEV, dtype=torch.float64)
    for off in (4, 5):                                   # a 16-byte-aligned map (float4 stores) and an unaligned one
        big_map = torch.full(((off + N * H_ * W + 7) * 4,), 0x5A, device=DEV, dtype=torch.uint8)
        big_mean = torch.full(((3 + N + 3) * 4,), 0x5A, device=DEV, dtype=torch.uint8)
        fmap, fmean = big_map.view(torch.float32), big_mean.view(torch.float32)
        vmap, vmean = fmap[off:off + N * H_ * W], fmean[3:3 + N]
        H.call("adh_ciede2000", a.data_ptr(), b.data_ptr(), N, H_, W, 0, partial.data_ptr(), nblk, vmap.data_ptr(),
               vmean.data_ptr())
        torch.cuda.synchronize()
        want_mean, want_map = M.ciede2000_batch(a, b, return_map=True)
        assert torch.equal(_bits(vmap), _bits(want_map.reshape(-1))) and torch.equal(_bits(vmean), _bits(want_mean))
        outside = torch.ones(big_map.numel(), dtype=torch.bool, device=DEV)
        outside[off * 4:(off + N * H_ * W) * 4] = False
        assert bool((big_map[outside] == 0x5A).all()), "a byte outside the map was written"
        outside = torch.ones(big_mean.numel(), dtype=torch.bool, device=DEV)
        outside[12:(3 + N) * 4] = False
        assert bool((big_mean[outside] == 0x5A).all()), "a byte outside the means was written"


def test_refusals_launch_nothing():
    N, H_, W = 2, 4, 5
    a, b = K.rgb_pair(N, H_, W, seed=1)
    a, b = a.to(DEV), b.to(DEV)
    keep_a, keep_b = a.clone(), b.clone()
    nblk = _nb(H_ * W)
    partial = torch.full((N * nblk,), -7.0, device=DEV, dtype=torch.float64)
    dmap = torch.full((N, H_, W), -7.0, device=DEV)
    mean = torch.full((N,), -7.0, device=DEV)
    fn, s = H.load().adh_ciede2000, H.stream_ptr()
    P, T_, Q, D, E = a.data_ptr(), b.data_ptr(), partial.data_ptr(), dmap.data_ptr(), mean.data_ptr()
    calls = [(None, T_, N, H_, W, 0, Q, nblk, D, E), (P, None, N, H_, W, 0, Q, nblk, D, E), (P, T_, N, H_, W, 0, None, nblk, D, E),
             (P, T_, N, H_, W, 0, Q, nblk, D, None), (P, T_, 0, H_, W, 0, Q, nblk, D, E), (P, T_, -1, H_, W, 0, Q, nblk, D, E),
             (P, T_, 65536, H_, W, 0, Q, nblk, D, E), (P, T_, N, 0, W, 0, Q, nblk, D, E), (P, T_, N, H_, 0, 0, Q, nblk, D, E),
             (P, T_, N, -2, W, 0, Q, nblk, D, E), (P, T_, N, H_, W, 2, Q, nblk, D, E), (P, T_, N, H_, W, -1, Q, nblk, D, E),
             (P, T_, N, H_, W, 0, Q, nblk + 1, D, E), (P, T_, N, H_, W, 0, Q, 0, D, E),
             (P, T_, N, H_, W, 0, Q, nblk, P, E),                              # the map is the first plane of pred
             (P, T_, N, H_, W, 0, Q, nblk, T_ + 4 * (N * 3 * H_ * W - 1), E)]  # the map starts on target's last float
    for c in calls:
        assert fn(s, *c) == ADH_E_ARG, c
    assert H.load().adh_ciede2000_num_blocks(0) == ADH_E_ARG and H.load().adh_ciede2000_num_blocks(-5) == ADH_E_ARG
    torch.cuda.synchronize()
    assert bool((partial == -7).all()) and bool((dmap == -7).all()) and bool((mean == -7).all())
    assert torch.equal(a, keep_a) and torch.equal(b, keep_b)
    # the Python surface takes the refusals of its neighbours
    with pytest.raises(RuntimeError):
        M.ciede2000_batch(a.cpu(), b.cpu())
    with pytest.raises(RuntimeError):
        M.ciede2000_batch(a, b[:, :, :3])
    with pytest.raises(RuntimeError):
        M.ciede2000_batch(a.double(), b.double())


def test_metric_harness_gains_the_key_only_when_asked(tmp_path):
    a, b = K.rgb_pair(4, 16, 20, seed=5)
    a, b = a.to(DEV), b.to(DEV)
    cats = ["low_intensity", "high_intensity", "low_intensity", "high_intensity"]
    plain = M.ImageQualityMetrics(device=DEV, use_lpips=False)
    plain.add_batch(a, b, cats)
    plain.add_batch(a[:2], b[:2])
    avg = plain.compute_averages()
    assert set(avg) == {"low_intensity", "high_intensity", "all"}
    assert all(set(v) == {"psnr", "ssim", "samples"} for v in avg.values())
    assert all(set(r) == {"psnr", "ssim"} for rs in plain.results.values() for r in rs)
    assert set(M.calculate_image_metrics(a, b)) == {"psnr", "ssim"}
    with_de = M.ImageQualityMetrics(device=DEV, use_lpips=False, use_ciede2000=True)
    with_de.add_batch(a, b, cats)
    with_de.add_batch(a[:2], b[:2])
    avg2 = with_de.print_results()
    assert all(set(v) == {"psnr", "ssim", "ciede2000", "samples"} for v in avg2.values())
    assert all(set(r) == {"psnr", "ssim", "ciede2000"} for rs in with_de.results.values() for r in rs)
    for cat in avg:
        assert avg2[cat]["psnr"] == avg[cat]["psnr"] and avg2[cat]["ssim"] == avg[cat]["ssim"]
    direct = M.ciede2000_batch(a, b).double().cpu()
    assert avg2["low_intensity"]["ciede2000"] == float(direct[[0, 2]].mean())
    assert avg2["all"]["ciede2000"] == float(direct[:2].mean())
    with_de.save_results(str(tmp_path / "r.json"))
    saved = json.load(open(tmp_path / "r.json"))
    assert saved == avg2 and "ciede2000" in saved["high_intensity"]
    plain.save_results(str(tmp_path / "p.json"))
    assert all("ciede2000" not in v for v in json.load(open(tmp_path / "p.json")).values())
