"""csrc/depthwise.hip through the C ABI on the cases of tests/test_depthwise_hostemu_cpu.py, against the same float64
restatements and bounds (tests/_stream_ref64.py; every accumulating expression of these kernels is an explicit fmaf, so the
bounds carry no allowance for contraction either way).  Outputs are NaN-prefilled channel slices (out_cs, g_cs, gx_cs > C)
inside NaN guard bands, and the slack between the pixels must hold its NaN bit for bit afterwards; the slack of every input is
NaN; every call runs twice and must reproduce itself bit for bit.  The first direct test of adh_channel_scale and
adh_channel_scale_bwd, the gx-null form and gs against the float64 sum included."""
import pytest
import torch

from adam_dehaze_amd import _hip as H
from tests import _stream_ref64 as R
from tests._util import DEV, _assert_bound, _nan, _pad_untouched, _padded, _twice

pytestmark = pytest.mark.gpu
ACT_LIST = [R.ACT_NONE, R.ACT_RELU, R.ACT_RELU6, R.ACT_HARDSWISH, R.ACT_HARDSIGMOID]


def _flat(t):
    return t.reshape(-1, t.shape[-1])


def _in(t, cs):
    """[P, C] on the device as a channel slice of a NaN buffer [P, cs]"""
    P, C = t.shape
    b = _nan(P, cs)
    b[:, :C] = t.to(DEV)
    return b


def _out(P, C, cs, init=None):
    """(whole, [P, cs] view): NaN inside NaN guard bands; `init` fills the channel slice (the accumulate forms)"""
    whole, own = _padded(P * cs)
    v = own.view(P, cs)
    if init is not None:
        v[:, :C] = init.to(DEV)
    return whole, v


def _slice(whole, v, C, what):
    """the [P, C] slice of an _out buffer after a run; its slack and guard bands still hold the NaN they were filled with"""
    nan_bits = torch.full((1,), float("nan")).view(torch.int32).item()
    assert bool((v[:, C:].contiguous().view(torch.int32) == nan_bits).all()), f"{what}: written outside its channel slice"
    assert _pad_untouched(whole, v.numel()), f"{what}: written outside its buffer"
    return v[:, :C]


@pytest.mark.parametrize("C,xcs", R.DW_C)
def test_dwconv_vs_float64(C, xcs):
    ocs, gcs, gxcs = C + 8, C + 4, C + 12
    multi = 0
    for ci, ((k, st), (N, Hh, Ww)) in enumerate((ks, im) for ks in R.DW_KS for im in R.DW_IMAGES):
        KK = k * k
        OH, OW = R.dw_out_hw(Hh, Ww, k, st)
        P, Pin = N * OH * OW, N * Hh * Ww
        x, w, g, sc, sh = R.dw_case(N, Hh, Ww, C, k, st, seed=C * 100 + ci)
        act = ACT_LIST[ci % 5]
        tag = f"C={C} k={k} s={st} image={(N, Hh, Ww)}"
        xb, gb, wd, scd, shd = _in(_flat(x), xcs + 4), _in(_flat(g), gcs), w.to(DEV), sc.to(DEV), sh.to(DEV)
        xs = xcs + 4                                             # (the input is a slice on the GPU for every C)
        nblk, wnblk = H.value("adh_dwconv_num_blocks", P, C), H.value("adh_dwconv_wgrad_num_blocks", P, C)
        assert (nblk, wnblk) == (R.dw_fwd_blocks(P, C), R.dw_wgrad_blocks(P, C)), tag
        multi += wnblk > 1
        prior = torch.randn(Pin, C, generator=R.gen(ci))
        dw_prior = torch.randn(C, 1, k, k, generator=R.gen(ci + 1))

        def run():
            wpw, wp = _padded(KK * C)
            H.call("adh_dwconv_pack_weights", wd.data_ptr(), H.WLayout(1, C, k, k, 0, 0, 0, 0, 0), wp.data_ptr())
            raw_w, raw = _out(P, C, ocs)
            stw, stats = _padded(nblk * 2 * C)
            H.call("adh_dwconv_fwd", xb.data_ptr(), xs, N, Hh, Ww, C, k, st, wp.data_ptr(), raw.data_ptr(), ocs, OH, OW, None,
                   None, R.ACT_NONE, stats.data_ptr())
            ev_w, ev = _out(P, C, ocs)
            H.call("adh_dwconv_fwd", xb.data_ptr(), xs, N, Hh, Ww, C, k, st, wp.data_ptr(), ev.data_ptr(), ocs, OH, OW,
                   scd.data_ptr(), shd.data_ptr(), act, None)
            g0_w, g0 = _out(Pin, C, gxcs)
            g1_w, g1 = _out(Pin, C, gxcs, init=prior)
            for gx, acc in ((g0, 0), (g1, 1)):
                H.call("adh_dwconv_dgrad", gb.data_ptr(), gcs, N, OH, OW, C, k, st, wp.data_ptr(), gx.data_ptr(), gxcs, Hh, Ww,
                       acc)
            pw, part = _padded(wnblk * KK * C)
            d0_w, d0 = _padded(C * KK)
            d1_w, d1 = _padded(C * KK)
            d1.copy_(dw_prior.view(-1))
            for dw, acc in ((d0, 0), (d1, 1)):
                H.call("adh_dwconv_wgrad", xb.data_ptr(), xs, N, Hh, Ww, C, k, st, gb.data_ptr(), gcs, OH, OW, part.data_ptr(),
                       wnblk, dw.data_ptr(), acc)
            return wpw, raw_w, stw, ev_w, g0_w, g1_w, pw, d0_w, d1_w, raw, ev, g0, g1

        wpw, raw_w, stw, ev_w, g0_w, g1_w, pw, d0_w, d1_w, raw, ev, g0, g1 = _twice(run)
        for whole, n, what in ((wpw, KK * C, "wp"), (stw, nblk * 2 * C, "stats"), (pw, wnblk * KK * C, "partials"),
                               (d0_w, C * KK, "dw"), (d1_w, C * KK, "dw (accumulate)")):
            assert _pad_untouched(whole, n), f"{tag}: {what} written outside its buffer"
            assert not torch.isnan(whole[64:64 + n]).any(), f"{tag}: {what} has unwritten elements"
        assert torch.equal(wpw[64:64 + KK * C].view(KK, C).cpu(), w.view(C, KK).t()), tag + ": packed weights"
        y, terms = R.dw_fwd64(x, w, k, st)
        _assert_bound(_slice(raw_w, raw, C, tag + " raw"), _flat(y), _flat(R.dw_fwd_bound(terms, k)), tag + " raw output")
        stats = stw[64:64 + nblk * 2 * C].view(nblk, 2, C).double()
        b1, b2 = R.dw_stats_bounds(y, terms, C, k)
        _assert_bound(stats[:, 0].sum(0), _flat(y).sum(0), b1, tag + " sum y")
        _assert_bound(stats[:, 1].sum(0), (_flat(y) ** 2).sum(0), b2, tag + " sum y^2")
        ref, bound = R.dw_eval64(y, terms, sc, sh, act, k)
        _assert_bound(_slice(ev_w, ev, C, tag + " eval"), _flat(ref), _flat(bound), tag + f" eval act {act}")
        gx, gxt, dw, dwt = R.dw_grads64(x, w, g, k, st)
        _assert_bound(_slice(g0_w, g0, C, tag + " gx"), _flat(gx), _flat(R.dw_dgrad_bound(gxt, k)), tag + " dgrad")
        _assert_bound(_slice(g1_w, g1, C, tag + " gx (accumulate)"), _flat(gx) + prior.double(),
                      R.dw_dgrad_bound(_flat(gxt), k, prior), tag + " dgrad accumulate")
        _assert_bound(d0_w[64:64 + C * KK].view(C, 1, k, k), dw, R.dw_wgrad_bound(dwt, P, C), tag + " wgrad")
        _assert_bound(d1_w[64:64 + C * KK].view(C, 1, k, k), dw + dw_prior.double(), R.dw_wgrad_bound(dwt, P, C, dw_prior),
                      tag + " wgrad accumulate")
    if C == 260:
        assert multi > 0, "no case ran the weight gradient over more than one pixel block"


@pytest.mark.parametrize("C,xcs", R.DW_C)
def test_channel_scale_vs_float64(C, xcs):
    """adh_channel_scale / adh_channel_scale_bwd at one pixel, at one pixel block and one pixel, without gx, and over N = 3"""
    _, Rl, _ = R.dw_split(C)
    ocs, gcs, gxcs, xs = C + 8, C + 4, C + 12, xcs + 4
    most = 0
    for ci, (N, HW, with_gx) in enumerate([(2, 1, True), (1, 4 * Rl + 1, True), (3, 7, False), (3, 2 * Rl + 3, True)]):
        x, sv, g = R.se_case(N, HW, C, seed=C + ci)
        tag = f"C={C} N={N} HW={HW}"
        nblk = H.value("adh_channel_scale_bwd_num_blocks", HW, C)
        assert nblk == R.dw_se_blocks(HW, C), tag
        most = max(most, nblk)
        xb, gb, sd = _in(x.view(-1, C), xs), _in(g.view(-1, C), gcs), sv.to(DEV)

        def run():
            ow, o = _out(N * HW, C, ocs)
            H.call("adh_channel_scale", xb.data_ptr(), xs, sd.data_ptr(), N, HW, C, o.data_ptr(), ocs)
            gw, gx = _out(N * HW, C, gxcs)
            pw, part = _padded(N * nblk * C)
            sw, gs = _padded(N * C)
            H.call("adh_channel_scale_bwd", gb.data_ptr(), gcs, xb.data_ptr(), xs, sd.data_ptr(), N, HW, C,
                   gx.data_ptr() if with_gx else None, gxcs if with_gx else 0, part.data_ptr(), nblk, gs.data_ptr())
            return ow, gw, pw, sw, o, gx

        ow, gw, pw, sw, o, gxv = _twice(run)
        ref, bound = R.se_fwd64(x, sv)
        _assert_bound(_slice(ow, o, C, tag + " out"), ref.view(-1, C), bound.view(-1, C), tag + " x * s")
        gx, gxb, gs, gsb = R.se_bwd64(g, x, sv, nblk)
        if with_gx:
            _assert_bound(_slice(gw, gxv, C, tag + " gx"), gx.view(-1, C), gxb.view(-1, C), tag + " gx")
        else:
            assert torch.isnan(gw).all(), tag + ": gx is null, nothing may be written"
        assert _pad_untouched(pw, N * nblk * C) and _pad_untouched(sw, N * C), tag
        assert not torch.isnan(pw[64:64 + N * nblk * C]).any(), tag + ": partial rows have unwritten elements"
        _assert_bound(sw[64:64 + N * C].view(N, C), gs, gsb, tag + " gs")
    assert most > 1


def test_argument_rejections_launch_nothing():
    C, k, N, Hh, Ww = 8, 3, 1, 4, 4
    P = N * Hh * Ww
    x, w, g, sc, sh = R.dw_case(N, Hh, Ww, C, k, 1, seed=1)
    xb, gb, wp, sd = _flat(x).to(DEV), _flat(g).to(DEV), w.view(C, 9).t().contiguous().to(DEV), torch.rand(N, C).to(DEV)
    out, stats, part, dw, gs = _nan(P, C), _nan(2, C), _nan(9, C), _nan(C, 9), _nan(N, C)

    def fwd(C=C, k=k, st=1, xcs=C, ocs=C, OH=Hh, OW=Ww, act=0, scale=None):
        return ("adh_dwconv_fwd", xb.data_ptr(), xcs, N, Hh, Ww, C, k, st, wp.data_ptr(), out.data_ptr(), ocs, OH, OW, scale, None,
                act, stats.data_ptr())

    def dgrad(C=C, k=k, st=1, gcs=C, gxcs=C, OH=Hh):
        return ("adh_dwconv_dgrad", gb.data_ptr(), gcs, N, OH, Ww, C, k, st, wp.data_ptr(), out.data_ptr(), gxcs, Hh, Ww, 0)

    def wgrad(C=C, k=k, st=1, xcs=C, gcs=C, OW=Ww, nblk=1):
        return ("adh_dwconv_wgrad", xb.data_ptr(), xcs, N, Hh, Ww, C, k, st, gb.data_ptr(), gcs, Hh, OW, part.data_ptr(), nblk,
                dw.data_ptr(), 0)

    def scale(C=C, xcs=C, ocs=C, HW=P):
        return ("adh_channel_scale", xb.data_ptr(), xcs, sd.data_ptr(), N, HW, C, out.data_ptr(), ocs)

    def sbwd(C=C, gcs=C, xcs=C, gxcs=C, nblk=1):
        return ("adh_channel_scale_bwd", gb.data_ptr(), gcs, xb.data_ptr(), xcs, sd.data_ptr(), N, P, C, out.data_ptr(), gxcs,
                part.data_ptr(), nblk, gs.data_ptr())

    bad = [fwd(C=6), fwd(C=0), fwd(k=4), fwd(st=3), fwd(xcs=4), fwd(ocs=4), fwd(xcs=10), fwd(ocs=10), fwd(OH=3), fwd(OW=5),
           fwd(act=2), fwd(act=R.ACT_RELU), fwd(scale=sd.data_ptr()),
           dgrad(C=6), dgrad(k=7), dgrad(st=0), dgrad(gcs=4), dgrad(gxcs=10), dgrad(OH=5),
           wgrad(C=14), wgrad(k=1), wgrad(st=4), wgrad(xcs=4), wgrad(gcs=6), wgrad(OW=3), wgrad(nblk=2), wgrad(nblk=0),
           scale(C=6), scale(xcs=4), scale(ocs=10), scale(HW=0),
           sbwd(C=6), sbwd(gcs=4), sbwd(xcs=10), sbwd(gxcs=4), sbwd(nblk=2)]
    for args in bad:
        with pytest.raises(RuntimeError):
            H.call(*args)
    torch.cuda.synchronize()
    for t in (out, stats, part, dw, gs):
        assert torch.isnan(t).all(), "a rejected call must not launch"
