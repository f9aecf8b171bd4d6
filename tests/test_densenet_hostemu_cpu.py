"""csrc/densenet.hip without a GPU: the source file, compiled by the host C++ compiler against the stand-in header of
tools/host_emu (its ADH_HOST_EMU_STREAM section) with AddressSanitizer and UndefinedBehaviorSanitizer, run as a stand-alone
program on heap blocks of exactly their sizes (tests/_hostemu.py) and held to the float64 restatements and bounds of
tests/_stream_ref64.py.  The host compiler does not contract a * b + c: where a bound counts one rounding for such an expression
on the GPU it gets one more here (`host=1`)."""
import numpy as np
import pytest
import torch

from tests import _hostemu as E
from tests import _stream_ref64 as R

SNBLK, STATS, MOMENTS, FOLD, AVGBWD, PREACT = range(6)


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    d = tmp_path_factory.mktemp("densenet_emu")
    exe = E.build(d, "densenet", "densenet_main.cpp")
    return lambda: E.Script(exe, d)


@pytest.mark.parametrize("C,cs,P", [(4, 8, 1), (36, 100, 513), (260, 264, 300), (1028, 1032, 5)])
def test_slice_stats_and_moments_vs_float64(emu, C, cs, P):
    """(36, 100, 513): R = 28 lanes, 4 threads idle, a second block of one pixel; (260, 264, 300): 65 quads, R = 3, the unrolled
    tail clamps; (1028, 1032, 5): a group of 256 quads, then a group of one quad on 256 lanes"""
    s = emu()
    x = torch.randn(P, C, generator=R.gen(C + P)) * 2 + 3
    nblk = -(-P // 512)
    bx, bpart = s.sin(x, cs, 4), s.out(nblk * 2 * C)
    c0 = s.call(SNBLK, [P, C])
    c1 = s.call(STATS, [cs, P, C], [bx, bpart])
    # the moments of those rows, into slices of wider float64 blocks; and of the same rows at a pitch > C behind NaN padding
    bm, bv = s.raw(np.full(C + 2, np.nan), 16), s.raw(np.full(C + 2, np.nan), 16)
    c2 = s.call(MOMENTS, [nblk, C, C], [bpart, bm, bv], [float(P)])
    rcs = s.run()
    assert rcs == [nblk, 0, 0]
    part = s.get(bpart).view(nblk, 2, C)
    E.assert_written(part, "partial rows")
    ref_s, b_s, ref_q, b_q = R.slice_stats64(x, host=1)
    E.assert_bound(part[:, 0].double().sum(0), ref_s, b_s, "sum x")
    E.assert_bound(part[:, 1].double().sum(0), ref_q, b_q, "sum x^2")
    mean, b_m, var, b_v = R.moments64(part, C, float(P))
    gm, gv = s.get(bm, np.float64), s.get(bv, np.float64)
    for got, ref, bound, what in ((gm, mean, b_m, "mean"), (gv, var, b_v, "var")):
        assert torch.isnan(got[:2]).all() and got.numel() == C + 2, what + ": written in front of its slice"
        E.assert_bound(got[2:], ref, bound, what)


@pytest.mark.parametrize("nblk,C,pitch", [(1, 4, 8), (33, 33, 40), (65, 36, 36), (97, 5, 7)])
def test_slice_moments_with_pitch_and_poisoned_padding(emu, nblk, C, pitch):
    """both sides of the two-rows-per-trip loop's bound (b + 32 < nblk) and its tail; C = 33: the second workgroup has one live
    channel; channel 2 has Q / n < mean^2 (the clamp to a zero variance)"""
    s = emu()
    g = R.gen(nblk + C)
    part = torch.full((nblk, 2, pitch), float("nan"))
    m = torch.randn(nblk, C, generator=g)
    part[:, 0, :C] = m
    part[:, 1, :C] = m * m + torch.rand(nblk, C, generator=g)
    part[:, 0, 2], part[:, 1, 2] = 1.5, 2.25 * 0.999
    count = float(nblk)
    bm, bv = s.out(C, np.float64), s.out(C, np.float64)
    s.call(MOMENTS, [nblk, pitch, C], [s.vec(part), bm, bv], [count])
    # the last row ends at its last channel: not one float of padding behind it
    bm2, bv2 = s.out(C, np.float64), s.out(C, np.float64)
    s.call(MOMENTS, [nblk, pitch, C], [s.vec(part.view(-1)[:part.numel() - (pitch - C)]), bm2, bv2], [count])
    assert s.run() == [0, 0]
    mean, b_m, var, b_v = R.moments64(part, C, count)
    assert float(var[2]) == 0.0
    for km, kv in ((bm, bv), (bm2, bv2)):
        E.assert_bound(s.get(km, np.float64), mean, b_m, "mean")
        E.assert_bound(s.get(kv, np.float64), var, b_v, "var")


def test_fold_moments_each_optional_output_null(emu):
    s = emu()
    C, count = 261, 37.0
    g = R.gen(5)
    mean, var = torch.randn(C, dtype=torch.float64, generator=g), torch.rand(C, dtype=torch.float64, generator=g) * 4
    var[::7] = 0.0
    gamma, beta = torch.randn(C, generator=g), torch.randn(C, generator=g)
    rm0, rv0 = torch.randn(C, generator=g), torch.rand(C, generator=g) + 0.5
    names = ["gamma", "beta", "rm", "rv", "save_mean", "save_invstd", "nbt"]
    runs = []
    for null in [None] + names + ["all"]:
        for cnt in ((count, 1.0) if null is None else (count,)):
            on = {n: null != n and null != "all" for n in names}
            b = {"scale": s.out(C), "shift": s.out(C), "mean": s.out(C) if on["save_mean"] else None,
                 "invstd": s.out(C) if on["save_invstd"] else None, "rm": s.out(C, init=rm0) if on["rm"] else None,
                 "rv": s.out(C, init=rv0) if on["rv"] else None, "nbt": s.raw(np.array([5], np.int64)) if on["nbt"] else None}
            s.call(FOLD, [C], [s.vec(mean, np.float64), s.vec(var, np.float64), s.vec(gamma) if on["gamma"] else None,
                               s.vec(beta) if on["beta"] else None, b["rm"], b["rv"], b["scale"], b["shift"], b["mean"],
                               b["invstd"], b["nbt"]], [cnt, R.BN_EPS, R.MOM])
            runs.append((null, cnt, on, b))
    assert s.run() == [0] * len(runs)
    for null, cnt, on, b in runs:
        ref = R.fold64(mean, var, cnt, gamma if on["gamma"] else None, beta if on["beta"] else None, rm0, rv0, host=1)
        for name in ("scale", "shift", "mean", "invstd", "rm", "rv"):
            if b[name] is not None:
                got = s.get(b[name])
                E.assert_written(got, name)
                E.assert_bound(got, *ref[name], f"{name} (null: {null}, count {cnt})")
        if b["nbt"] is not None:
            assert int(s.get(b["nbt"], np.int64)) == 6, "num_batches_tracked goes up by exactly 1"


@pytest.mark.parametrize("N,Hh,Ww,C,gcs,gxcs", [(2, 2, 3, 4, 8, 8), (1, 5, 7, 12, 12, 20), (2, 4, 4, 260, 264, 268),
                                                (3, 2, 2, 36, 40, 36)])
def test_avgpool2_bwd_vs_float64(emu, N, Hh, Ww, C, gcs, gxcs):
    """2 x 2 is the smallest size the entry point accepts; 5 x 7 drops an odd row and an odd column"""
    s = emu()
    OH, OW = Hh // 2, Ww // 2
    g = torch.randn(N, OH, OW, C, generator=R.gen(Hh * Ww + C))
    prior = torch.randn(N * Hh * Ww, C, generator=R.gen(1))
    bg = s.sin(g.view(-1, C), gcs, 4 if gcs > C else 0)
    off = 4 if gxcs > C else 0
    b0, b1 = s.sout(N * Hh * Ww, C, gxcs, off), s.sout(N * Hh * Ww, C, gxcs, off, init=prior)
    s.call(AVGBWD, [gcs, N, Hh, Ww, C, gxcs, 0], [bg, b0])
    s.call(AVGBWD, [gcs, N, Hh, Ww, C, gxcs, 1], [bg, b1])
    assert s.run() == [0, 0]
    ref = R.avgpool2_bwd64(g, Hh, Ww).view(-1, C)
    assert torch.equal(s.get_slice(b0, N * Hh * Ww, C).double(), ref), "g / 4 is exact"
    # accumulate: one addition, rounded once
    E.assert_bound(s.get_slice(b1, N * Hh * Ww, C), ref + prior.double(), R.EPS * (ref.abs() + prior.double().abs()), "accumulate")


@pytest.mark.parametrize("training", [0, 1])
@pytest.mark.parametrize("P,C,dacs,xcs,dcs", [(300, 4, 8, 12, 16), (77, 36, 40, 100, 44), (13, 260, 264, 268, 272)])
def test_preact_bwd_accum_vs_float64(emu, training, P, C, dacs, xcs, dcs):
    """(300, 4): one block, 256 pixel lanes, the second unrolled slot is live for 44 lanes and clamps for the others; (77, 36): 9
    blocks of which most lanes have no pixel; P is never a multiple of the unroll of 8"""
    s = emu()
    g = R.gen(P + C)
    x = R.grid((P, C), -24, 24, 8, P)                      # z = fma(x, scale, shift) exact: the float64 mask is the kernel's
    ss = torch.stack([R.grid((C,), -8, 8, 4, C), R.grid((C,), -16, 16, 8, C + 1)])
    dA = torch.randn(P, C, generator=g)
    mean, invstd = torch.randn(C, generator=g), torch.rand(C, generator=g) + 0.5
    coef = torch.randn(3, C, generator=g)
    prior = torch.randn(P, C, generator=g)
    bdA, bx = s.sin(dA, dacs, 4), s.sin(x, xcs, 8)
    bss, bco = s.vec(ss), s.vec(coef if training else coef[:1])       # frozen statistics read coef[0] only
    bmu, bis = (s.vec(mean), s.vec(invstd)) if training else (None, None)
    b0, b1 = s.sout(P, C, dcs, 4), s.sout(P, C, dcs, 4, init=prior)
    for acc, b in ((0, b0), (1, b1)):
        s.call(PREACT, [dacs, xcs, training, dcs, P, C, acc], [bdA, bx, bss, bmu, bis, bco, b])
    assert s.run() == [0, 0]
    assert float(((x.double() * ss[0].double() + ss[1].double()) == 0).sum()) > 0, "no element sits on the kink"
    ref, bound = R.preact_bwd64(dA, x, ss, mean, invstd, coef, training)
    E.assert_bound(s.get_slice(b0, P, C), ref, bound, "dx")
    E.assert_bound(s.get_slice(b1, P, C), ref + prior.double(), bound + R.EPS * (ref.abs() + bound + prior.double().abs()),
                   "dx accumulated")


def test_argument_rejections_write_nothing(emu):
    s = emu()
    P, C = 6, 8
    x = torch.randn(P, C)
    bx, bpart, bm, bv = s.sin(x), s.out(2 * C), s.out(C, np.float64), s.out(C, np.float64)
    bgx, bvec, bco = s.sout(P, C), s.vec(torch.randn(2, C)), s.vec(torch.randn(3, C))
    md, vd, sc, sh = s.vec(torch.randn(C), np.float64), s.vec(torch.rand(C), np.float64), s.out(C), s.out(C)
    part_in = s.vec(torch.randn(1, 2, C))
    fold = [md, vd, None, None, None, None, sc, sh, None, None, None]
    bad = [s.call(SNBLK, [0, C]),
           s.call(STATS, [C, 0, C], [bx, bpart]), s.call(STATS, [C, P, 6], [bx, bpart]), s.call(STATS, [4, P, C], [bx, bpart]),
           s.call(STATS, [10, P, C], [bx, bpart]), s.call(STATS, [C, P, 4100], [bx, bpart]), s.call(STATS, [C, P, C], [bx, None]),
           s.call(MOMENTS, [0, C, C], [part_in, bm, bv], [6.0]), s.call(MOMENTS, [1, 4, C], [part_in, bm, bv], [6.0]),
           s.call(MOMENTS, [1, C, C], [part_in, bm, bv], [0.0]), s.call(MOMENTS, [1, C, C], [part_in, None, bv], [6.0]),
           s.call(FOLD, [0], fold, [6.0, R.BN_EPS, R.MOM]), s.call(FOLD, [C], fold, [0.0, R.BN_EPS, R.MOM]),
           s.call(FOLD, [C], fold[:6] + [None] + fold[7:], [6.0, R.BN_EPS, R.MOM]),
           s.call(AVGBWD, [C, 1, 1, 6, C, C, 0], [bx, bgx]), s.call(AVGBWD, [C, 1, 2, 1, C, C, 0], [bx, bgx]),
           s.call(AVGBWD, [C, 1, 2, 3, 6, C, 0], [bx, bgx]), s.call(AVGBWD, [4, 1, 2, 3, C, C, 0], [bx, bgx]),
           s.call(AVGBWD, [C, 1, 2, 3, C, 10, 0], [bx, bgx]), s.call(AVGBWD, [C, 0, 2, 3, C, C, 0], [bx, bgx]),
           s.call(PREACT, [C, C, 1, C, P, C, 0], [bx, bx, bvec, None, bvec, bco, bgx]),
           s.call(PREACT, [C, C, 0, C, P, 6, 0], [bx, bx, bvec, None, None, bco, bgx]),
           s.call(PREACT, [4, C, 0, C, P, C, 0], [bx, bx, bvec, None, None, bco, bgx]),
           s.call(PREACT, [C, 10, 0, C, P, C, 0], [bx, bx, bvec, None, None, bco, bgx]),
           s.call(PREACT, [C, C, 0, 4, P, C, 0], [bx, bx, bvec, None, None, bco, bgx]),
           s.call(PREACT, [C, C, 0, C, 0, C, 0], [bx, bx, bvec, None, None, bco, bgx]),
           s.call(PREACT, [C, C, 0, C, P, C, 0], [bx, bx, None, None, None, bco, bgx])]
    rcs = s.run()
    assert [rcs[i] for i in bad] == [E.ADH_E_ARG] * len(bad), rcs
    for b in (bpart, bm, bv, bgx, sc, sh):
        assert s.unchanged(b), "a rejected call wrote to an output"
