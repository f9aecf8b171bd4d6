"""csrc/ciede2000.hip without a GPU: the source file, compiled by the host C++ compiler against tools/host_emu with
AddressSanitizer and UndefinedBehaviorSanitizer, run as a stand-alone program (tools/host_emu/ciede2000_main.cpp) on heap blocks
of exactly the addressed bytes and held to the float64 reference of tests/_ref64_ciede.py with the bound of the GPU test.  A read
or a write outside a block is the sanitizer's to report.  Nothing is loaded into Python."""
import numpy as np
import pytest
import torch

from tests import _ciede_cases as K
from tests import _hostemu as E

CIEDE, NUM_BLOCKS = 0, 1


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    d = tmp_path_factory.mktemp("ciede_emu")
    exe = E.build(d, "ciede2000", "ciede2000_main.cpp")
    return lambda: E.Script(exe, d)


@pytest.fixture(scope="module")
def num_blocks(emu):
    """adh_ciede2000_num_blocks for every pixel count up to 4096, asked of the compiled source in one script"""
    s = emu()
    for p in range(1, 4097):
        s.call(NUM_BLOCKS, (p,))
    table = s.run()
    assert table[0] == 1 and all(b >= a for a, b in zip(table, table[1:]))
    return lambda pixels: table[pixels - 1]


def _run(emu, num_blocks, a, b, lab=0, with_map=True, off=0):
    """one call on blocks of exactly their bytes; `off`: the inputs start that many floats into blocks that much larger"""
    N, _, H, W = a.shape
    nblk = num_blocks(H * W)
    s = emu()
    ins = []
    for x in (a, b):
        blk = np.concatenate([np.full(off, E.RPOISON, np.uint32), x.numpy().reshape(-1).view(np.uint32)])
        ins.append(s.raw(blk, off * 4))
        s.ro.append(ins[-1])
    partial, mean = s.out(N * nblk, np.float64), s.out(N)
    m = s.out(N * H * W) if with_map else None
    s.call(CIEDE, (N, H, W, lab, nblk), (ins[0], ins[1], partial, m, mean))
    assert s.run() == [0]
    got_mean = s.get(mean)
    E.assert_written(got_mean, "mean")
    got_map = None
    if with_map:
        got_map = s.get(m).view(N, H, W)
        E.assert_written(got_map, "map")
    return got_map, got_mean


def _check(got_map, got_mean, a, b, lab=False, what=""):
    ref_map, ref_mean = K.reference(a, b, lab)
    if got_map is not None:
        E.assert_bound(got_map, ref_map, K.TOL, f"{what} map")
    E.assert_bound(got_mean, ref_mean, K.TOL, f"{what} mean")


def test_published_pairs_as_one_lab_image(emu, num_blocks):
    a, b, table = K.sharma_image()
    got_map, got_mean = _run(emu, num_blocks, a, b, lab=1)
    _check(got_map, got_mean, a, b, True, "published pairs")
    assert float(np.abs(got_map[0].double().numpy() - table).max()) <= 5e-5 + K.TOL
    ka, kb = K.knife_edge_image()
    edge, _ = _run(emu, num_blocks, ka, kb, lab=1)
    print("hues 180 degrees apart (printed, not asserted):", [f"{v:.7f}" for v in edge.reshape(-1).tolist()],
          "reference", [f"{v:.7f}" for v in K.reference(ka, kb, True)[0].reshape(-1)])


@pytest.mark.parametrize("N,H,W", K.SHAPES)
def test_random_srgb_pairs(emu, num_blocks, N, H, W):
    a, b = K.rgb_pair(N, H, W, seed=H * 131 + W)
    got_map, got_mean = _run(emu, num_blocks, a, b)
    _check(got_map, got_mean, a, b, what=f"{N}x{H}x{W}")


def test_three_workgroups_with_a_ragged_last_one_and_no_map(emu, num_blocks):
    N, H, W = K.ragged_shape(num_blocks)
    a, b = K.rgb_pair(N, H, W, seed=7)
    got_map, got_mean = _run(emu, num_blocks, a, b)
    _check(got_map, got_mean, a, b, what=f"{N}x{H}x{W}")
    _, mean_only = _run(emu, num_blocks, a, b, with_map=False)
    assert torch.equal(mean_only.view(torch.int32), got_mean.view(torch.int32)), "map = NULL changes the mean"


@pytest.mark.parametrize("H,W", [(16, 20), (7, 9)])
def test_inputs_one_float_into_a_larger_block(emu, num_blocks, H, W):
    a, b = K.rgb_pair(2, H, W, seed=3)
    aligned_map, aligned_mean = _run(emu, num_blocks, a, b)
    got_map, got_mean = _run(emu, num_blocks, a, b, off=1)
    _check(got_map, got_mean, a, b, what="unaligned base")
    # the pixels a lane takes and the order of the sums are the same on both paths
    assert torch.equal(got_map.view(torch.int32), aligned_map.view(torch.int32))
    assert torch.equal(got_mean.view(torch.int32), aligned_mean.view(torch.int32))


def test_crafted_pixels(emu, num_blocks):
    a, b, names = K.crafted_lab()
    got_map, got_mean = _run(emu, num_blocks, a, b, lab=1)
    _check(got_map, got_mean, a, b, True, "crafted Lab")
    for k, name in enumerate(names):
        if name.startswith("equal"):
            assert float(got_map[0, 0, k]) == 0.0, name
    a, b, names = K.crafted_rgb()
    got_map, got_mean = _run(emu, num_blocks, a, b)
    _check(got_map, got_mean, a, b, False, "crafted sRGB")
    assert float(got_map[0, 0, names.index("equal")]) == 0.0
    assert float(got_map[0, 0, names.index("all NaN against black")]) == 0.0
    assert abs(float(got_map[0, 0, 0]) - 100.0000002) <= K.TOL


def test_refusals(emu, num_blocks):
    N, H, W = 2, 4, 5
    a, b = K.rgb_pair(N, H, W, seed=1)
    nblk = num_blocks(H * W)
    s = emu()
    pa, pb = s.vec(a.reshape(-1)), s.vec(b.reshape(-1))
    partial, mean, m = s.out(N * nblk, np.float64), s.out(N), s.out(N * H * W)
    bad = [s.call(CIEDE, (N, H, W, 0, nblk), bufs) for bufs in
           ((None, pb, partial, m, mean), (pa, None, partial, m, mean), (pa, pb, None, m, mean), (pa, pb, partial, m, None))]
    for n, h, w, lab, nb in ((0, H, W, 0, nblk), (-1, H, W, 0, nblk), (65536, H, W, 0, nblk), (N, 0, W, 0, nblk),
                             (N, H, 0, 0, nblk), (N, -3, W, 0, nblk), (N, H, W, 2, nblk), (N, H, W, -1, nblk),
                             (N, H, W, 0, nblk + 1), (N, H, W, 0, 0)):
        bad.append(s.call(CIEDE, (n, h, w, lab, nb), (pa, pb, partial, m, mean)))
    # the map over an input: its first image is the input's first plane, or it starts inside the other input
    bad.append(s.call(CIEDE, (N, H, W, 0, nblk), (pa, pb, partial, pa, mean)))
    bad.append(s.call(CIEDE, (N, H, W, 0, nblk), (pa, pb, partial, pb, mean)))
    zero = s.call(NUM_BLOCKS, (0,))
    rcs = s.run()                      # Script.run also checks that pa and pb are unchanged
    assert [rcs[k] for k in bad] == [E.ADH_E_ARG] * len(bad), rcs
    assert rcs[zero] == E.ADH_E_ARG
    assert s.unchanged(partial) and s.unchanged(mean) and s.unchanged(m)
