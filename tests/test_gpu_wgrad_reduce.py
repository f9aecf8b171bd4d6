"""The six weight-gradient reduce entry points (csrc/conv_wgrad_reduce.hip) called directly: adh_wgrad_reduce, _small, _packed,
_wino, _wino32 and _wino43, which the engine reaches only through Engine._wgrad, always with accumulate = 0 and with the
split counts it happens to choose.  Slabs from a seeded generator (random in the padded rows and columns too); dst NaN-filled
for accumulate = 0 and seeded for accumulate = 1, inside NaN guards; every element the layout names is written and within the
bound of the float64 reference (tests/_wgrad_reduce_ref.py: the same sums and the same inverse transform on the CPU, bound
(nsplit + c) EPS |M| sum |slab|; c, counted there from the inverse() bodies: 0 for the tap domain, 6 for F(2x2,3x3), 5 for
F(3x3,2x2), 2 for F(4x4,3x3), which computes in float64 and rounds once), nothing else is -- neither the guards nor the elements of a
strided dst the layout skips -- and two runs give equal bits."""
import ctypes as C

import numpy as np
import pytest
import torch

from adam_dehaze_amd import _hip as H
from tests import _wgrad_reduce_ref as R
from tests._util import DEV, _pad_untouched, _padded, _twice

pytestmark = pytest.mark.gpu
ADH_E_ARG = -1
SPLITS = [1, 2, 4, 33, 37]     # adh_wgrad_sum_splits: one split, fewer than its four split groups, the 32-wide trip and its tail


def _call(entry, slab, dst, *args):
    """rc of entry(stream, slab, *args) with `dst` spliced in where args holds the string "dst" """
    a = [dst.data_ptr() if isinstance(x, str) else x for x in args]
    return getattr(H.load(), entry)(H.stream_ptr(), None if slab is None else slab.data_ptr(), *a)


def _run(entry, slab_np, dst0_np, *args):
    """two runs on fresh copies of slab (the Winograd-domain entry points sum it in place) and dst -> dst of the first"""
    n = dst0_np.size
    d0 = torch.from_numpy(dst0_np).to(DEV)
    s0 = torch.from_numpy(np.ascontiguousarray(slab_np)).to(DEV)

    def once():
        whole, dst = _padded(n)
        dst.copy_(d0)
        assert _call(entry, s0.clone(), dst, *args) == 0
        torch.cuda.synchronize()
        assert _pad_untouched(whole, n), f"{entry}: wrote outside dst"
        return (dst,)
    return _twice(once)[0].cpu().numpy()


def _layout_case(cs, nsplit, accumulate, seed, desc=None):
    slab = cs.slab(seed, nsplit)
    dst0 = R.rng_dst(seed, cs.ndst, accumulate)
    L = H.WLayout(*cs.L)
    pre = (nsplit,) if desc is None else (nsplit, C.byref(desc))
    got = _run(cs.entry, slab, dst0, *pre, R.KP, R.NCP, C.byref(L), "dst", accumulate)
    ref, bound, written = R.reference(slab, cs.M, cs.c, cs.L, cs.taps, dst0, accumulate)
    R.check(got, dst0, ref, bound, written, f"{cs.entry} K={cs.L.K} Nc={cs.L.Nc} taps={cs.L.KHt} nsplit={nsplit} acc={accumulate}")


@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("K,Nc", R.SIZES)
def test_direct_reduce_reversed_taps(K, Nc, accumulate):
    """T = 1, 4, 9, 16 taps walked backwards; nsplit: the tail loop alone, the 4-wide trip alone, both, and two tail trips"""
    for KH, nsplit in ((1, 1), (2, 4), (3, 7), (4, 2)):
        _layout_case(R.case("adh_wgrad_reduce", K, Nc, KH, reverse=True), nsplit, accumulate, seed=10 + KH)


@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("nslabs", [1, 63, 64, 130])
def test_wave_reduce(nslabs, accumulate):
    """one wave per element: fewer slabs than lanes, one short of a wave, exactly one, two trips and a partial third"""
    for (K, Nc), reverse in zip(R.SIZES, (True, False)):
        _layout_case(R.case("adh_wgrad_reduce_small", K, Nc, 3, reverse=reverse), nslabs, accumulate, seed=20 + nslabs)


@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("nsplit", [1, 2, 3])
def test_packed_reduce(nsplit, accumulate):
    Cin, KH, KW, Cout = 3, 7, 7, 5
    slab = R.rng_slab(40 + nsplit, nsplit, KH * ((KW + 3) // 4), 32, R.NCP)
    dst0 = R.rng_dst(40, Cout * Cin * KH * KW, accumulate)
    got = _run("adh_wgrad_reduce_packed", slab, dst0, nsplit, R.NCP, Cin, KH, KW, Cout, "dst", accumulate)
    ref, bound = R.packed_reference(slab, Cin, KH, KW, Cout, dst0, accumulate)
    R.check(got, dst0, ref, bound, np.ones(dst0.shape, bool), f"packed nsplit={nsplit} acc={accumulate}")


@pytest.mark.parametrize("nsplit", SPLITS)
@pytest.mark.parametrize("entry", ["adh_wgrad_reduce_wino", "adh_wgrad_reduce_wino43"])
def test_winograd_reduce(entry, nsplit):
    for (K, Nc), reverse in zip(R.SIZES, (True, False)):
        for accumulate in (0, 1):
            _layout_case(R.case(entry, K, Nc, 3, reverse=reverse), nsplit, accumulate, seed=50 + nsplit)


def _desc(KH, in_s, out_s, dstep):
    """a 2x2-tap-form descriptor of 32 -> 32 channels on a 4 x 4 virtual grid (the reduce reads its class structure only)"""
    d = H.ConvDesc()
    d.N, d.Cin, d.in_cstride, d.Cout, d.out_cstride, d.NcP = 1, 32, 32, 32, 32, 32
    d.VH = d.VW = 4
    d.IH = d.IW = 4 * in_s
    d.OH = d.OW = 4 * out_s
    d.in_sy = d.in_sx = in_s
    d.out_sy = d.out_sx = out_s
    d.KH = d.KW = KH
    d.dy0 = d.dx0 = -1 if dstep > 0 else 0
    d.dstep_y = d.dstep_x = dstep
    return d


@pytest.mark.parametrize("nsplit", SPLITS)
def test_wino32_class_forms(nsplit, monkeypatch):
    """Conv2d k4 s2: four kernel-parity classes scattered over a 4x4 layout (the library takes that form only when asked:
    ADH_WINO32_WGRAD=2); one transposed 2x2 class whose taps walk backwards, on a layout with negative tap strides"""
    monkeypatch.setenv("ADH_WINO32_WGRAD", "2")
    conv, convt = _desc(4, 2, 1, 1), _desc(2, 1, 2, -1)
    assert H.value("adh_conv_wgrad_wino32_classes", C.byref(conv)) == 4
    assert H.value("adh_conv_wgrad_wino32_classes", C.byref(convt)) == 1
    for accumulate in (0, 1):
        for K, Nc in R.SIZES:
            _layout_case(R.case("adh_wgrad_reduce_wino32", K, Nc, 4, classes=R.CONV_K4S2_CLASSES), nsplit, accumulate, 60 + nsplit,
                         desc=conv)
        _layout_case(R.case("adh_wgrad_reduce_wino32", 5, 7, 2, reverse=True, classes=R.CONVT_CLASS), nsplit, accumulate,
                     70 + nsplit, desc=convt)


def test_rejections_leave_dst_unwritten(monkeypatch):
    monkeypatch.setenv("ADH_WINO32_WGRAD", "2")
    three, two = R.case("adh_wgrad_reduce_wino", 5, 7, 3), R.case("adh_wgrad_reduce_wino", 5, 7, 2)
    L3, L2 = H.WLayout(*three.L), H.WLayout(*two.L)
    convt = _desc(2, 1, 2, -1)
    slab = torch.from_numpy(three.slab(80, 1)).to(DEV)
    whole, dst = _padded(three.ndst)
    lay = lambda L, ncp=R.NCP: (R.KP, ncp, C.byref(L), "dst", 0)
    bad = []
    for entry in ("adh_wgrad_reduce", "adh_wgrad_reduce_small", "adh_wgrad_reduce_wino", "adh_wgrad_reduce_wino43"):
        bad += [(entry, None, (1,) + lay(L3)), (entry, slab, (0,) + lay(L3))]              # a null slab; nsplit = 0
    bad += [("adh_wgrad_reduce_wino32", None, (1, C.byref(convt)) + lay(L2)), ("adh_wgrad_reduce_wino32", slab, (0, C.byref(convt)) + lay(L2)),
            ("adh_wgrad_reduce_wino32", slab, (1, C.byref(convt)) + lay(L2, 30)),          # NcP % 4 != 0
            ("adh_wgrad_reduce_wino32", slab, (1, C.byref(convt)) + lay(L3))]              # a 3x3 layout for a 2x2-tap form
    for entry in ("adh_wgrad_reduce_wino", "adh_wgrad_reduce_wino43"):
        bad += [(entry, slab, (1,) + lay(L2)), (entry, slab, (1,) + lay(L3, 30))]          # a 2x2 layout; NcP % 4 != 0
    pk = lambda Cin: (R.NCP, Cin, 7, 7, 5, "dst", 0)
    bad += [("adh_wgrad_reduce_packed", slab, (1,) + pk(9)), ("adh_wgrad_reduce_packed", slab, (0,) + pk(3)),
            ("adh_wgrad_reduce_packed", None, (1,) + pk(3))]
    for entry, s, args in bad:
        assert _call(entry, s, dst, *args) == ADH_E_ARG, (entry, args)
    torch.cuda.synchronize()
    assert bool(torch.isnan(whole).all())
