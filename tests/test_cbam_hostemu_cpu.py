"""csrc/cbam.hip without a GPU: the source file, compiled by the host C++ compiler against the stand-in header of tools/host_emu
(its ADH_HOST_EMU_STREAM section: the 8-lane and 64-lane butterflies run on the emulator's __shfl_xor and csrc/wave.h, the
dynamic LDS of the two MLP kernels is a heap block of exactly the bytes the launch asked for) with AddressSanitizer and
UndefinedBehaviorSanitizer, run as a stand-alone program on heap blocks of exactly their sizes (tests/_hostemu.py) and held to
the float64 restatements and bounds of tests/_cbam_ref64.py, the ones tests/test_gpu_cbam.py holds the library to (host = 1: one
more rounding where a bound counts a contracted a * b + c once).  A second program is built with small caps (SMALL below), so
that the block loops of the pooling passes and the grid-stride loops of the per-pixel and two-stream kernels run at a few dozen
pixels.

Every tensor a kernel reads ends at the last used channel of its last pixel and must come back unchanged; every tensor it
writes is poison with checked slack; every call is made twice, on outputs of its own, and the two must agree bit for bit;
arg-max indices are exact."""
import os
import re
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest
import torch

from tests import _cbam_ref64 as R
from tests import _hostemu as E

ENTRY_POINTS = ["adh_cbam_pool_num_blocks", "adh_cbam_pool", "adh_cbam_mlp", "adh_cbam_spatial_stats", "adh_cbam_apply",
                "adh_cbam_bwd_a", "adh_cbam_bwd_b_num_blocks", "adh_cbam_bwd_b", "adh_cbam_bwd_c",
                "adh_cbam_bwd_d_scratch_floats", "adh_cbam_bwd_d", "adh_cbam_bwd_e"]     # the driver's call numbers
(POOL_NBLK, POOL, MLP, SSTATS, APPLY, BWD_A, BWD_B_NBLK, BWD_B, BWD_C, BWD_D_SCRATCH, BWD_D, BWD_E) = range(12)
SMALL = {"POOL_PPB": 32, "CBAM_ROW_MAXBLK": 2, "CBAM_SCALE_MAXBLK": 3}
IPOISON = 0x5A5A5A5A     # Script.out's fill of an int32 output


def test_every_entry_point_is_called():
    src = open(os.path.join(E.ROOT, "adam-dehaze_amd", "csrc", "cbam.hip")).read()
    assert sorted(re.findall(r'extern "C" int (adh_\w+)', src)) == sorted(ENTRY_POINTS)
    me = open(__file__).read()
    for name in ("POOL_NBLK", "POOL", "MLP", "SSTATS", "APPLY", "BWD_A", "BWD_B_NBLK", "BWD_B", "BWD_C", "BWD_D_SCRATCH", "BWD_D",
                 "BWD_E"):
        assert re.search(r"s\.call\(%s," % name, me), name


@pytest.fixture(scope="module")
def emus(tmp_path_factory):
    d = tmp_path_factory.mktemp("cbam_emu")
    dirs = {False: d / "default", True: d / "small"}
    for sub in dirs.values():
        sub.mkdir()
    with ThreadPoolExecutor(2) as pool:
        exe = dict(zip((False, True), pool.map(lambda small: E.build(
            dirs[small], "cbam", "cbam_main.cpp", [f"{k}={v}" for k, v in SMALL.items()] if small else (), sanitize=E.FLOAT_CAST),
            (False, True))))
    return lambda small=False: E.Script(exe[small], d)


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _ints(shape, lo, hi, seed):
    return torch.randint(lo, hi + 1, shape, generator=_gen(seed)).float()


def _randn(*shape, seed=0):
    return torch.randn(shape, generator=_gen(seed))


def _rand(*shape, seed=0):
    return torch.rand(shape, generator=_gen(seed))


def _twice(s, runs):
    """runs: two tuples of output buffers of two identical calls"""
    for k1, k2 in zip(*runs):
        assert (s.after[k1] == s.after[k2]).all(), "two identical calls differ"
    return runs[0]


def _geti(s, k):
    t = s.get(k, np.int32)
    assert not (t == IPOISON).any(), "an index output was not written"
    return t


def _getf(s, k, what):
    t = s.get(k)
    E.assert_written(t, what)
    return t


# ------------------------------------------------------------------------------------------------ pooling and pass C
POOL_C = [4, 20, 96, 1024]


def _pool_hw(ppb):
    return [1, 7, ppb - 1, ppb, ppb + 1, 2 * ppb + 3]


POOL_CASES = [(True, C, _pool_hw(32), 2) for C in POOL_C] + [(False, 20, [513], 1), (False, 96, [1027], 1), (False, 1024, [511], 1)]
_pool_ids = [f"{'small' if c[0] else 'default'}-C{c[1]}" for c in POOL_CASES]


@pytest.mark.parametrize("small,C,hws,N", POOL_CASES, ids=_pool_ids)
def test_cbam_pool_ties_first_index(emus, small, C, hws, N):
    """Values from {0, 1, 2}: ties within a thread's pixels, across the rows of a block and across blocks; channel 1 constant,
    channel 2 all negative.  C = 20: CQ = 5 does not divide 256, the last thread is idle; 96: R = 10, 16 idle; 1024: R = 1; 4:
    64 pixel rows.  SMALL: blocks of 32 pixels, so HW = 67 makes three.  The sums are of small integers and halves: exact."""
    s = emus(small)
    ppb = SMALL["POOL_PPB"] if small else R.POOL_PPB
    x_cs = C + 4
    todo = []
    for HW in hws:
        x = _ints((N, HW, C), 0, 2, seed=C + HW)
        x[..., 1] = 1.5
        x[..., 2] = -_ints((N, HW), 1, 3, seed=C + HW + 1)
        nblk = -(-HW // ppb)
        bx = s.sin(x.view(N * HW, C), x_cs, 4)
        c_n = s.call(POOL_NBLK, [HW])
        runs = []
        for _ in range(2):
            part, pidx = s.out(N * nblk * 2 * C), s.out(N * nblk * C, np.int32)
            pooled, amax = s.out(N * 2 * C), s.out(N * C, np.int32)
            s.call(POOL, [x_cs, N, HW, C, nblk], [bx, part, pidx, pooled, amax])
            runs.append((pooled, amax, part, pidx))
        todo.append((HW, x, nblk, c_n, runs))
    rcs = s.run()
    for HW, x, nblk, c_n, runs in todo:
        assert rcs[c_n] == nblk and rcs[c_n + 1:c_n + 3] == [0, 0], rcs
        pooled, amax, part, pidx = _twice(s, runs)
        _getf(s, part, "partial"), _geti(s, pidx)
        pooled = _getf(s, pooled, "pooled").view(N, 2, C)
        mean, mx, first = R.pool64(x.double())
        assert torch.equal(pooled[:, 0].double(), mean), f"mean HW={HW}"
        assert torch.equal(pooled[:, 1].double(), mx), f"max HW={HW}"
        assert torch.equal(_geti(s, amax).view(N, C).long(), first), f"HW={HW}: arg-max must be the first index in scan order"


@pytest.mark.parametrize("small,C,hws,N", POOL_CASES, ids=_pool_ids)
def test_cbam_bwd_c(emus, small, C, hws, N):
    """the pooling shapes; g at stride C + 4 and x at C + 8, the per-pixel tensors exactly N * HW long"""
    s = emus(small)
    ppb = SMALL["POOL_PPB"] if small else R.POOL_PPB
    todo = []
    for HW in hws:
        sd = 3 * C + HW
        x, g = _ints((N, HW, C), 0, 2, seed=sd), _randn(N, HW, C, seed=sd + 1)
        sa, gsmap = _rand(N, HW, seed=sd + 2), _randn(N, HW, 2, seed=sd + 3)
        cidx = torch.randint(0, C, (N, HW), generator=_gen(sd + 4), dtype=torch.int32)
        nblk = -(-HW // ppb)
        bufs = [s.sin(g.view(N * HW, C), C + 4, 4), s.sin(x.view(N * HW, C), C + 8, 8), s.vec(sa), s.vec(gsmap),
                s.vec(cidx, np.int32)]
        runs = []
        for _ in range(2):
            part = s.out(N * nblk * C)
            s.call(BWD_C, [C + 4, C + 8, N, HW, C, nblk], bufs + [part])
            runs.append((part,))
        todo.append((HW, g, x, sa, gsmap, cidx, nblk, runs))
    rcs = s.run()
    assert rcs == [0] * len(rcs), rcs
    for HW, g, x, sa, gsmap, cidx, nblk, runs in todo:
        (part,) = _twice(s, runs)
        ref, e = R.bwd_c64(g, x, sa, gsmap, cidx)
        E.assert_bound(_getf(s, part, "gca_partial").view(N, nblk, C).double().sum(1), ref, e, f"gca C={C} HW={HW}")


# ------------------------------------------------------------------------------------------------ the two MLP kernels
MLP_CASES = [(16, 1), (96, 6), (1024, 64), (20, 1)]


def _mlp_inputs(C, Ch, N):
    pooled = _randn(N, 2, C, seed=C)
    w1 = _randn(Ch, C, seed=C + 1) / C ** 0.5
    w1[0] = 0.0                                 # hidden unit 0: pre-activation exactly 0 for every image
    w2 = _randn(C, Ch, seed=C + 2) / Ch ** 0.5
    return pooled, w1, w2


@pytest.mark.parametrize("C,Ch", MLP_CASES)
def test_cbam_mlp(emus, C, Ch):
    """2 Ch = 2 waves' worth of wave_sum calls spread over four waves: at Ch = 1 two waves make one call and two none; the
    dynamic LDS is exactly (2 C + 2 Ch) floats"""
    s = emus()
    N = 3
    pooled, w1, w2 = _mlp_inputs(C, Ch, N)
    bufs = [s.vec(pooled), s.vec(w1), s.vec(w2)]
    runs = []
    for _ in range(2):
        ca, hidden = s.out(N * C), s.out(N * 2 * Ch)
        s.call(MLP, [N, C, Ch], bufs + [ca, hidden])
        runs.append((ca, hidden))
    assert s.run() == [0, 0]
    ca, hidden = _twice(s, runs)
    h, e_h, ca_ref, e_ca = R.mlp64(pooled, w1, w2, host=1)
    hidden = _getf(s, hidden, "hidden").view(N, 2, Ch)
    E.assert_bound(hidden, h, e_h, "hidden")
    assert (hidden[:, :, 0] == 0).all()
    E.assert_bound(_getf(s, ca, "ca").view(N, C), ca_ref, e_ca, "ca")


@pytest.mark.parametrize("N", [1, 3])
@pytest.mark.parametrize("C,Ch", MLP_CASES)
def test_cbam_bwd_d_mlp_gradients(emus, C, Ch, N):
    s = emus()
    nblk = 3
    pooled, w1, w2 = _mlp_inputs(C, Ch, N)
    hidden = torch.relu(pooled.double() @ w1.double().t()).float()          # post-ReLU, unit 0 exactly 0
    ca = _rand(N, C, seed=C + 3)
    gcap = _randn(N, nblk, C, seed=C + 4)
    dw10, dw20 = _randn(Ch, C, seed=1), _randn(C, Ch, seed=2)
    nscr = N * (C + 2 * Ch)
    bufs = [s.vec(gcap), s.vec(ca), s.vec(pooled), s.vec(hidden), s.vec(w1), s.vec(w2)]
    c_n = s.call(BWD_D_SCRATCH, [N, C, Ch])
    runs = []
    for acc in (0, 0, 1):
        gpool, scratch = s.out(N * 2 * C), s.out(nscr)
        dw1, dw2 = (s.out(Ch * C, init=dw10), s.out(C * Ch, init=dw20)) if acc else (s.out(Ch * C), s.out(C * Ch))
        s.call(BWD_D, [nblk, N, C, Ch, acc], bufs + [gpool, dw1, dw2, scratch])
        runs.append((gpool, dw1, dw2, scratch))
    rcs = s.run()
    assert rcs[c_n] == nscr and rcs[c_n + 1:] == [0, 0, 0], rcs
    gpool, dw1, dw2, scratch = _twice(s, runs[:2])
    _getf(s, scratch, "scratch")
    gpool, dw1, dw2 = _getf(s, gpool, "gpool").view(N, 2, C), _getf(s, dw1, "d-W1").view(Ch, C), _getf(s, dw2, "d-W2").view(C, Ch)
    assert torch.equal(s.get(runs[2][1]).view(Ch, C), dw10 + dw1) and torch.equal(s.get(runs[2][2]).view(C, Ch), dw20 + dw2), \
        "accumulate=1"
    (gp, g1, g2), (tp, t1, t2), k = R.bwd_d64(gcap, ca, pooled, hidden, w1, w2, host=1)
    E.assert_bound(gpool, gp, k * tp, "gpool")
    E.assert_bound(dw1, g1, k * t1, "d-W1")
    E.assert_bound(dw2, g2, k * t2, "d-W2")


# ------------------------------------------------------------------------------------------------ the per-pixel kernels
ROW_CASES = [(True, C, HW) for C in (4, 36, 96) for HW in (1, 33, 32 * SMALL["CBAM_ROW_MAXBLK"] + 5)] + [(False, 36, 33)]


@pytest.mark.parametrize("small,C,HW", ROW_CASES)
def test_cbam_spatial_stats_and_bwd_a(emus, small, C, HW):
    """8 lanes per pixel: C = 4 leaves seven of them without a quad, C = 36 gives lane 0 a second quad, C = 96 three each.
    SMALL: two blocks of 32 pixels a trip, HW = 69 takes a second trip with five live pixels in one block and none in the
    other.  x from {0, 1, 2} and ca from powers of two: x * ca is exact, ties in the channel max everywhere."""
    s = emus(small)
    N = 2
    x = _ints((N, HW, C), 0, 2, seed=C + HW)
    x[:, ::5, :] = 0.0
    ca = torch.pow(2.0, _ints((N, C), -3, 1, seed=C + HW + 1))
    g, sa = _randn(N, HW, C, seed=C + HW + 2), _rand(N, HW, seed=C + HW + 3)
    bx, bca, bg, bsa = s.sin(x.view(N * HW, C), C + 8, 4), s.vec(ca), s.sin(g.view(N * HW, C), C + 4, 8), s.vec(sa)
    runs = []
    for _ in range(2):
        smap, cidx, gsa = s.out(N * HW * 2), s.out(N * HW, np.int32), s.out(N * HW)
        s.call(SSTATS, [C + 8, N, HW, C], [bx, bca, smap, cidx])
        s.call(BWD_A, [C + 4, C + 8, N, HW, C], [bg, bx, bca, bsa, gsa])
        runs.append((smap, cidx, gsa))
    assert s.run() == [0] * 4
    smap, cidx, gsa = _twice(s, runs)
    smap = _getf(s, smap, "smap").view(N, HW, 2)
    mean, e_mean, mx, first = R.spatial_stats64(x, ca)
    E.assert_bound(smap[..., 0], mean, e_mean, "channel mean")
    assert torch.equal(smap[..., 1].double(), mx), "channel max"
    assert torch.equal(_geti(s, cidx).view(N, HW).long(), first), "channel arg-max must be the first index"
    ref, e = R.bwd_a64(g, x, ca, sa)
    E.assert_bound(_getf(s, gsa, "gsa_pre").view(N, HW), ref, e, "gsa_pre")


# ------------------------------------------------------------------------------------------------ the window and the two streams
WINDOW_HW = R.APPLY_HW + [(10, 37)]        # (10, 37) and (33, 40) cross an 8 x 32 tile in both directions


APPLY_CASES = [(hw, False) for hw in WINDOW_HW] + [(hw, True) for hw in ((6, 33), (10, 37), (33, 40))]


@pytest.mark.parametrize("hw,small", APPLY_CASES, ids=lambda v: "%dx%d" % v if isinstance(v, tuple) else ("small" if v else "default"))
def test_cbam_apply_and_bwd_e(emus, hw, small):
    """C = 24 (six quads: the launch is a multiple of three blocks) at strides 28 / 32 / 36.  SMALL: three blocks at most, so at
    33 x 40 the scale pass takes two trips of eight pixels and pass E three of four."""
    Hh, Ww = hw
    s = emus(small)
    N, C, HW = 2, 24, Hh * Ww
    x_cs, out_cs, g_cs, gx_cs = C + 4, C + 8, C + 12, C + 16
    sd = Hh * 41 + Ww
    x, ca, smap, wsp = _randn(N, HW, C, seed=sd), _rand(N, C, seed=sd + 1), _randn(N, HW, 2, seed=sd + 2), _randn(98, seed=sd + 3) / 98 ** 0.5
    g, sa_in, gsmap = _randn(N, HW, C, seed=sd + 4), _rand(N, HW, seed=sd + 5), _randn(N, HW, 2, seed=sd + 6) * 8
    gpool = _randn(N, 2, C, seed=sd + 7) * 8 * HW ** 0.5
    cidx = torch.randint(0, C, (N, HW), generator=_gen(sd + 8), dtype=torch.int32)
    amax = torch.randint(0, HW, (N, C), generator=_gen(sd + 9), dtype=torch.int32)
    bx, bca, bsm, bw = s.sin(x.view(N * HW, C), x_cs, 4), s.vec(ca), s.vec(smap), s.vec(wsp)
    bg, bsa, bgs, bgp = s.sin(g.view(N * HW, C), g_cs, 8), s.vec(sa_in), s.vec(gsmap), s.vec(gpool)
    bci, bam = s.vec(cidx, np.int32), s.vec(amax, np.int32)
    runs = []
    for _ in range(2):
        sa, out, gx = s.out(N * HW), s.sout(N * HW, C, out_cs, 8), s.sout(N * HW, C, gx_cs, 4)
        s.call(APPLY, [x_cs, N, Hh, Ww, C, out_cs], [bx, bca, bsm, bw, sa, out])
        s.call(BWD_E, [g_cs, x_cs, N, HW, C, gx_cs], [bg, bx, bca, bsa, bgs, bci, bgp, bam, gx])
        runs.append((sa, out, gx))
    assert s.run() == [0] * 4
    sa, out, gx = _twice(s, runs)
    sa = _getf(s, sa, "sa")
    sa_ref, e_sa = R.sa64(smap, wsp, N, Hh, Ww, host=1)
    E.assert_bound(sa.view(N, Hh, Ww), sa_ref, e_sa, "sa")
    want = R.scale_f32(x.view(N, Hh, Ww, C), ca, sa, N, Hh, Ww)
    assert torch.equal(s.get_slice(out, N * HW, C).view(N, Hh, Ww, C), want), "out = x * ca * sa"
    ref, e = R.bwd_e64(g, ca, sa_in, gsmap, cidx, gpool, amax)
    E.assert_bound(s.get_slice(gx, N * HW, C).view(N, HW, C), ref, e, "gx")


@pytest.mark.parametrize("shape", [(2,) + hw for hw in WINDOW_HW] + [(1, 1, 1)], ids=lambda v: "%dx%dx%d" % v)
def test_cbam_bwd_b_transposed_conv_and_weight_gradient(emus, shape):
    """every lane of every wave makes the 98 x 2 wave_sum calls, the ones past N x HW with zeros; the 256-pixel blocks straddle
    images.  The two runs are one with accumulate = 0 and one with accumulate = 1: gsmap and the partial rows must agree bit for
    bit and the accumulated d-wsp must be the prior plus the first run's, exactly.  (Each call costs about half a second whatever
    the shape: cbam_dwsp_final_kernel's 98 workgroups pass eleven barriers each, 256 OS threads apiece.)"""
    s = emus()
    N, Hh, Ww = shape
    HW = Hh * Ww
    gsa, smap, wsp = _randn(N, HW, seed=HW), _randn(N, HW, 2, seed=HW + 1), _randn(98, seed=HW + 2) / 98 ** 0.5
    dw0 = _randn(98, seed=HW + 3)
    nb = -(-N * HW // 256)
    bufs = [s.vec(gsa), s.vec(smap), s.vec(wsp)]
    c_n = s.call(BWD_B_NBLK, [N, Hh, Ww])
    runs = []
    for acc in (0, 1):
        gsmap, part, dw = s.out(N * HW * 2), s.out(nb * 98), s.out(98, init=dw0 if acc else None)
        s.call(BWD_B, [N, Hh, Ww, nb, acc], bufs + [gsmap, part, dw])
        runs.append((gsmap, part, dw))
    rcs = s.run()
    assert rcs[c_n] == nb and rcs[c_n + 1:] == [0, 0], rcs
    gsmap, part = _twice(s, [r[:2] for r in runs])
    dw, dwa = runs[0][2], runs[1][2]
    _getf(s, part, "dwsp_partial")
    gs_ref, e_gs, dw_ref, e_dw = R.bwd_b64(gsa, smap, wsp, N, Hh, Ww, host=1)
    E.assert_bound(_getf(s, gsmap, "gsmap").view(N, Hh, Ww, 2), gs_ref, e_gs, "gsmap")
    dw = _getf(s, dw, "d-wsp")
    E.assert_bound(dw, dw_ref, e_dw, "d-wsp")
    assert torch.equal(s.get(dwa), dw0 + dw), "accumulate=1 adds the fp32 result"


# ------------------------------------------------------------------------------------------------ rejections
def test_argument_rejections_write_nothing(emus):
    s = emus()
    N, HW, C, Ch = 1, 6, 8, 1
    x = _randn(N * HW, C)
    bx, bv, bi = s.sin(x), s.vec(_randn(200)), s.vec(torch.zeros(64), np.int32)
    of, oi, oc = s.out(200), s.out(64, np.int32), s.sout(N * HW, C)
    bad = [s.call(POOL, [C, N, HW, 6, 1], [bx, of, oi, of, oi]), s.call(POOL, [C, N, HW, 1028, 1], [bx, of, oi, of, oi]),
           s.call(POOL, [C, N, HW, C, 2], [bx, of, oi, of, oi]), s.call(POOL, [C, 0, HW, C, 1], [bx, of, oi, of, oi]),
           s.call(POOL, [C, N, HW, C, 1], [bx, of, oi, None, oi]),
           s.call(MLP, [N, C, 0], [bv, bv, bv, of, of]), s.call(MLP, [N, C, Ch], [bv, bv, bv, of, None]),
           s.call(SSTATS, [C, N, HW, 6], [bx, bv, of, oi]), s.call(SSTATS, [C, N, 0, C], [bx, bv, of, oi]),
           s.call(SSTATS, [C, N, HW, C], [bx, bv, of, None]),
           s.call(APPLY, [C, N, 2, 3, 6, C], [bx, bv, bv, bv, of, oc]), s.call(APPLY, [10, N, 2, 3, C, C], [bx, bv, bv, bv, of, oc]),
           s.call(APPLY, [C, N, 2, 3, C, 10], [bx, bv, bv, bv, of, oc]), s.call(APPLY, [C, 65536, 2, 3, C, C], [bx, bv, bv, bv, of, oc]),
           s.call(APPLY, [C, N, 2, 3, C, C], [bx, bv, bv, bv, None, oc]),
           s.call(BWD_A, [C, C, N, HW, 2], [bx, bx, bv, bv, of]), s.call(BWD_A, [C, C, N, HW, C], [bx, bx, bv, None, of]),
           s.call(BWD_B, [N, 2, 3, 2, 0], [bv, bv, bv, of, of, of]), s.call(BWD_B, [N, 2, 3, 1, 0], [bv, bv, None, of, of, of]),
           s.call(BWD_C, [C, C, N, HW, 6, 1], [bx, bx, bv, bv, bi, of]), s.call(BWD_C, [C, C, N, HW, C, 3], [bx, bx, bv, bv, bi, of]),
           s.call(BWD_C, [C, C, N, HW, 1028, 1], [bx, bx, bv, bv, bi, of]),
           s.call(BWD_D, [0, N, C, Ch, 0], [bv, bv, bv, bv, bv, bv, of, of, of, of]),
           s.call(BWD_D, [1, 65536, C, Ch, 0], [bv, bv, bv, bv, bv, bv, of, of, of, of]),
           s.call(BWD_D, [1, N, C, Ch, 0], [bv, bv, bv, bv, bv, bv, of, of, of, None]),
           s.call(BWD_E, [C, C, N, HW, 6, C], [bx, bx, bv, bv, bv, bi, bv, bi, oc]),
           s.call(BWD_E, [C, C, N, HW, C, C], [bx, bx, bv, bv, bv, bi, bv, None, oc])]
    rcs = s.run()
    assert [rcs[i] for i in bad] == [E.ADH_E_ARG] * len(bad), rcs
    for b in (of, oi, oc):
        assert s.unchanged(b), "a rejected call wrote to an output"
