"""csrc/depthwise.hip without a GPU: the source file, compiled by the host C++ compiler against the stand-in header of
tools/host_emu (its ADH_HOST_EMU_STREAM section) with AddressSanitizer and UndefinedBehaviorSanitizer, run as a stand-alone
program on heap blocks of exactly their sizes (tests/_hostemu.py) and held to the float64 restatements and bounds of
tests/_stream_ref64.py -- the ones tests/test_gpu_depthwise.py holds the library to.  The shapes are the smallest that reach
each piece of the index arithmetic: one channel quad per block (C = 4), R = 85 pixel lanes and an idle thread (12), a channel
slice of a wider buffer (72 in 80), two channel chunks of which the second has one live quad (260); images down to 1x1, where
24 of a 5x5 kernel's 25 taps fall outside, and odd sizes under stride 2.  Every kernel expression that accumulates is an explicit
fmaf, one rounding on the host as on the GPU, so the bounds need no host allowance."""
import pytest
import torch

from tests import _hostemu as E
from tests import _stream_ref64 as R

PACK, NBLK, FWD, DGRAD, WNBLK, WGRAD, SCALE, SNBLK, SBWD = range(9)
ACT_LIST = [R.ACT_NONE, R.ACT_RELU, R.ACT_RELU6, R.ACT_HARDSWISH, R.ACT_HARDSIGMOID]


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    d = tmp_path_factory.mktemp("depthwise_emu")
    exe = E.build(d, "depthwise", "depthwise_main.cpp")
    return lambda: E.Script(exe, d)


def _flat(t):
    return t.reshape(-1, t.shape[-1])


@pytest.mark.parametrize("C,xcs", R.DW_C)
def test_dwconv_vs_float64(emu, C, xcs):
    s_ = emu()
    ocs, gcs, gxcs = C + 8, C + 4, C + 12
    xoff = 4 if xcs > C else 0
    todo = []
    for ci, ((k, st), (N, Hh, Ww)) in enumerate((ks, im) for ks in R.DW_KS for im in R.DW_IMAGES):
        KK = k * k
        OH, OW = R.dw_out_hw(Hh, Ww, k, st)
        P, Pin = N * OH * OW, N * Hh * Ww
        x, w, g, sc, sh = R.dw_case(N, Hh, Ww, C, k, st, seed=C * 100 + ci)
        act = ACT_LIST[ci % 5]
        bx, bg = s_.sin(_flat(x), xcs, xoff), s_.sin(_flat(g), gcs, 8)
        bw, bwp = s_.vec(w), s_.out(KK * C)
        geo_f = [xcs, N, Hh, Ww, C, k, st]
        c = {"pack": s_.call(PACK, [C, k], [bw, bwp])}
        nblk, wnblk = R.dw_fwd_blocks(P, C), R.dw_wgrad_blocks(P, C)
        c["nblk"] = s_.call(NBLK, [P, C])
        c["wnblk"] = s_.call(WNBLK, [P, C])
        b_raw, b_stats = s_.sout(P, C, ocs, 4), s_.out(nblk * 2 * C)
        c["train"] = s_.call(FWD, geo_f + [ocs, OH, OW, R.ACT_NONE], [bx, bwp, b_raw, None, None, b_stats])
        b_ev, bsc, bsh = s_.sout(P, C, ocs, 4), s_.vec(sc), s_.vec(sh)
        c["eval"] = s_.call(FWD, geo_f + [ocs, OH, OW, act], [bx, bwp, b_ev, bsc, bsh, None])
        prior = torch.randn(Pin, C, generator=R.gen(ci))
        b_gx0, b_gx1 = s_.sout(Pin, C, gxcs, 4), s_.sout(Pin, C, gxcs, 4, init=prior)
        geo_d = [gcs, N, OH, OW, C, k, st, gxcs, Hh, Ww]
        c["dgrad0"] = s_.call(DGRAD, geo_d + [0], [bg, bwp, b_gx0])
        c["dgrad1"] = s_.call(DGRAD, geo_d + [1], [bg, bwp, b_gx1])
        dw_prior = torch.randn(C, 1, k, k, generator=R.gen(ci + 1))
        b_part, b_dw0, b_dw1 = s_.out(wnblk * KK * C), s_.out(C * KK), s_.out(C * KK, init=dw_prior)
        geo_w = geo_f + [gcs, OH, OW, wnblk]
        c["wgrad0"] = s_.call(WGRAD, geo_w + [0], [bx, bg, b_part, b_dw0])
        c["wgrad1"] = s_.call(WGRAD, geo_w + [1], [bx, bg, b_part, b_dw1])
        todo.append(dict(k=k, st=st, N=N, Hh=Hh, Ww=Ww, P=P, Pin=Pin, KK=KK, c=c, x=x, w=w, g=g, sc=sc, sh=sh, act=act, nblk=nblk,
                         wnblk=wnblk, bwp=bwp, b_raw=b_raw, b_stats=b_stats, b_ev=b_ev, b_gx0=b_gx0, b_gx1=b_gx1, prior=prior,
                         b_part=b_part, b_dw0=b_dw0, b_dw1=b_dw1, dw_prior=dw_prior))
    rcs = s_.run()
    multi = 0
    for t in todo:
        k, st, N, Hh, Ww, P, Pin, KK, c = t["k"], t["st"], t["N"], t["Hh"], t["Ww"], t["P"], t["Pin"], t["KK"], t["c"]
        x, w, g, sc, sh, act = t["x"], t["w"], t["g"], t["sc"], t["sh"], t["act"]
        tag = f"C={C} k={k} s={st} image={(N, Hh, Ww)}"
        assert rcs[c["nblk"]] == t["nblk"] and rcs[c["wnblk"]] == t["wnblk"], tag
        multi += t["wnblk"] > 1
        for name in ("pack", "train", "eval", "dgrad0", "dgrad1", "wgrad0", "wgrad1"):
            assert rcs[c[name]] == 0, (tag, name, rcs[c[name]])
        wp = s_.get(t["bwp"]).view(KK, C)
        assert torch.equal(wp, w.view(C, KK).t()), tag + ": packed weights"
        y, terms = R.dw_fwd64(x, w, k, st)
        raw = s_.get_slice(t["b_raw"], P, C)
        E.assert_bound(raw, _flat(y), _flat(R.dw_fwd_bound(terms, k)), tag + " raw output")
        stats = s_.get(t["b_stats"]).view(t["nblk"], 2, C)
        E.assert_written(stats, tag + " statistics rows")
        b1, b2 = R.dw_stats_bounds(y, terms, C, k)
        E.assert_bound(stats[:, 0].double().sum(0), _flat(y).sum(0), b1, tag + " sum y")
        E.assert_bound(stats[:, 1].double().sum(0), (_flat(y) ** 2).sum(0), b2, tag + " sum y^2")
        ref, bound = R.dw_eval64(y, terms, sc, sh, act, k)
        E.assert_bound(s_.get_slice(t["b_ev"], P, C), _flat(ref), _flat(bound), tag + f" eval act {act}")
        gx, gxt, dw, dwt = R.dw_grads64(x, w, g, k, st)
        E.assert_bound(s_.get_slice(t["b_gx0"], Pin, C), _flat(gx), _flat(R.dw_dgrad_bound(gxt, k)), tag + " dgrad")
        pr = t["prior"]
        E.assert_bound(s_.get_slice(t["b_gx1"], Pin, C), _flat(gx) + pr.double(), _flat(R.dw_dgrad_bound(gxt, k)) +
                       R.EPS * (_flat(gxt) + pr.double().abs()), tag + " dgrad accumulate")
        dw0 = s_.get(t["b_dw0"]).view(C, 1, k, k)
        E.assert_written(dw0, tag + " dw")
        E.assert_bound(dw0, dw, R.dw_wgrad_bound(dwt, P, C), tag + " wgrad")
        dwp = t["dw_prior"]
        E.assert_bound(s_.get(t["b_dw1"]).view(C, 1, k, k), dw + dwp.double(), R.dw_wgrad_bound(dwt, P, C, dwp),
                       tag + " wgrad accumulate")
        E.assert_written(s_.get(t["b_part"]), tag + " weight-gradient partial rows")
    if C == 260:
        assert multi > 0, "no case ran the weight gradient over more than one pixel block"


@pytest.mark.parametrize("C,xcs", R.DW_C)
def test_channel_scale_vs_float64(emu, C, xcs):
    """adh_channel_scale / adh_channel_scale_bwd at one pixel, at one pixel block and one pixel, without gx, and over N = 3"""
    s_ = emu()
    _, Rl, _ = R.dw_split(C)
    ocs, gcs, gxcs = C + 8, C + 4, C + 12
    xoff = 4 if xcs > C else 0
    todo = []
    for ci, (N, HW, with_gx) in enumerate([(2, 1, True), (1, 4 * Rl + 1, True), (3, 7, False), (3, 2 * Rl + 3, True)]):
        x, sv, g = R.se_case(N, HW, C, seed=C + ci)
        nblk = R.dw_se_blocks(HW, C)
        bx, bs, bg = s_.sin(x.view(-1, C), xcs, xoff), s_.vec(sv), s_.sin(g.view(-1, C), gcs, 8)
        bo = s_.sout(N * HW, C, ocs, 4)
        bgx = s_.sout(N * HW, C, gxcs, 4) if with_gx else None
        bpart, bgs = s_.out(N * nblk * C), s_.out(N * C)
        c0 = s_.call(SCALE, [xcs, N, HW, C, ocs], [bx, bs, bo])
        c1 = s_.call(SNBLK, [HW, C])
        c2 = s_.call(SBWD, [gcs, xcs, N, HW, C, gxcs if with_gx else 0, nblk], [bg, bx, bs, bgx, bpart, bgs])
        todo.append((N, HW, x, sv, g, nblk, bo, bgx, bpart, bgs, c0, c1, c2))
    rcs = s_.run()
    assert any(t[5] > 1 for t in todo)
    for N, HW, x, sv, g, nblk, bo, bgx, bpart, bgs, c0, c1, c2 in todo:
        tag = f"C={C} N={N} HW={HW}"
        assert (rcs[c0], rcs[c1], rcs[c2]) == (0, nblk, 0), (tag, rcs[c0], rcs[c1], rcs[c2])
        ref, bound = R.se_fwd64(x, sv)
        E.assert_bound(s_.get_slice(bo, N * HW, C), ref.view(-1, C), bound.view(-1, C), tag + " x * s")
        gx, gxb, gs, gsb = R.se_bwd64(g, x, sv, nblk)
        if bgx is not None:
            E.assert_bound(s_.get_slice(bgx, N * HW, C), gx.view(-1, C), gxb.view(-1, C), tag + " gx")
        got = s_.get(bgs).view(N, C)
        E.assert_written(got, tag + " gs")
        E.assert_written(s_.get(bpart), tag + " partial rows")
        E.assert_bound(got, gs, gsb, tag + " gs")


def test_argument_rejections_write_nothing(emu):
    s_ = emu()
    C, k, st, N, Hh, Ww = 8, 3, 1, 1, 4, 4
    x, w, g, sc, sh = R.dw_case(N, Hh, Ww, C, k, st, seed=1)
    P = N * Hh * Ww
    bx, bg, bwp = s_.sin(_flat(x)), s_.sin(_flat(g)), s_.vec(w.view(C, 9).t().contiguous())
    bo, bst, bgx = s_.sout(P, C), s_.out(2 * C), s_.sout(P, C)
    bpart, bdw = s_.out(9 * C), s_.out(9 * C)
    bs, bgs = s_.vec(torch.rand(N, C)), s_.out(N * C)
    outs = [bo, bst, bgx, bpart, bdw, bgs]

    def fwd(C=C, k=k, st=st, xcs=C, ocs=C, OH=Hh, OW=Ww, act=0, b=(bx, bwp, bo, None, None, bst)):
        return s_.call(FWD, [xcs, N, Hh, Ww, C, k, st, ocs, OH, OW, act], b)

    def dgrad(C=C, k=k, st=st, gcs=C, gxcs=C, OH=Hh, b=(bg, bwp, bgx)):
        return s_.call(DGRAD, [gcs, N, OH, Ww, C, k, st, gxcs, Hh, Ww, 0], b)

    def wgrad(C=C, k=k, st=st, xcs=C, gcs=C, OW=Ww, nblk=1, b=(bx, bg, bpart, bdw)):
        return s_.call(WGRAD, [xcs, N, Hh, Ww, C, k, st, gcs, Hh, OW, nblk, 0], b)

    bad = [fwd(C=6), fwd(C=0), fwd(k=4), fwd(st=3), fwd(xcs=4), fwd(ocs=4), fwd(xcs=10), fwd(ocs=10), fwd(OH=3), fwd(OW=5),
           fwd(act=2), fwd(act=R.ACT_RELU), fwd(b=(bx, bwp, bo, bs, None, bst)), fwd(b=(None, bwp, bo, None, None, bst)),
           dgrad(C=6), dgrad(k=7), dgrad(st=0), dgrad(gcs=4), dgrad(gxcs=10), dgrad(OH=5), dgrad(b=(bg, None, bgx)),
           wgrad(C=12 + 2), wgrad(k=1), wgrad(st=4), wgrad(xcs=4), wgrad(gcs=6), wgrad(OW=3), wgrad(nblk=2), wgrad(nblk=0),
           wgrad(b=(bx, bg, None, bdw)),
           s_.call(PACK, [C, 4], [bwp, bst]), s_.call(PACK, [0, 3], [bwp, bst]), s_.call(NBLK, [0, C]), s_.call(NBLK, [5, 6]),
           s_.call(WNBLK, [5, 2]), s_.call(SNBLK, [0, 8]), s_.call(SNBLK, [4, 7]),
           s_.call(SCALE, [C, N, P, 6, C], [bx, bs, bo]), s_.call(SCALE, [4, N, P, C, C], [bx, bs, bo]),
           s_.call(SCALE, [C, N, P, C, 10], [bx, bs, bo]), s_.call(SCALE, [C, N, 0, C, C], [bx, bs, bo]),
           s_.call(SCALE, [C, N, P, C, C], [bx, None, bo]),
           s_.call(SBWD, [C, C, N, P, 6, C, 1], [bg, bx, bs, bgx, bpart, bgs]),
           s_.call(SBWD, [4, C, N, P, C, C, 1], [bg, bx, bs, bgx, bpart, bgs]),
           s_.call(SBWD, [C, 10, N, P, C, C, 1], [bg, bx, bs, bgx, bpart, bgs]),
           s_.call(SBWD, [C, C, N, P, C, 4, 1], [bg, bx, bs, bgx, bpart, bgs]),
           s_.call(SBWD, [C, C, N, P, C, C, 2], [bg, bx, bs, bgx, bpart, bgs]),
           s_.call(SBWD, [C, C, N, P, C, C, 1], [bg, bx, bs, bgx, bpart, None])]
    rcs = s_.run()
    assert [rcs[i] for i in bad] == [E.ADH_E_ARG] * len(bad), rcs
    for b in outs:
        assert s_.unchanged(b), "a rejected call wrote to an output"
