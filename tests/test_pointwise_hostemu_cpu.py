"""csrc/pointwise.hip without a GPU: the source file, compiled by the host C++ compiler against the stand-in header of
tools/host_emu (its ADH_HOST_EMU_STREAM section) with AddressSanitizer and UndefinedBehaviorSanitizer, run as a stand-alone program
on heap blocks of exactly their sizes (tests/_hostemu.py) and held to the float64 restatements and bounds of
tests/_pointwise_ref64.py, the ones tests/test_gpu_pointwise.py holds the library to (plus one unit per a * b + c the host
compiler does not contract: the `host` argument there).  Nothing is loaded into Python.

Two programs are built: "lib" with the grid caps the library has, and "small" with the caps of SMALL_CAPS, under which the shapes
here, a few hundred elements each, run every grid-stride loop more than once and every partial row over more than one block.
Every tensor is a heap block of exactly the bytes the contract of include/adam_dehaze_hip.h gives it, so a read or write one
element outside is the sanitizer's to report; channel slices start 4 floats into their block behind poison; the slack a kernel
may read is NaN, the slack it may write is WPOISON and checked afterwards.  Every call is made twice, on outputs of its own, and
the two must agree bit for bit; inputs come back unchanged; no output element may still hold its poison."""
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import _hostemu as E
from tests import _pointwise_ref64 as P

EPS = E.EPS
ENTRY_POINTS = ["adh_version", "adh_image_to_nhwc8", "adh_image_normalize_to_nhwc8", "adh_image_normalize_bwd", "adh_nchw_to_nhwc",
                "adh_nhwc_to_nchw", "adh_head_blend", "adh_head_blend_bwd_num_blocks", "adh_head_blend_bwd", "adh_softmax3",
                "adh_softmax3_bwd", "adh_soft_blend", "adh_soft_blend_bwd", "adh_argmax3", "adh_route_compact", "adh_gather_images",
                "adh_scatter_images", "adh_reduce_num_blocks", "adh_l1_partial", "adh_mse_partial", "adh_sum_partials", "adh_l1_bwd",
                "adh_mse_bwd", "adh_cross_entropy3", "adh_adam_step", "adh_add_inplace", "adh_axpby_strided", "adh_maxpool",
                "adh_maxpool_bwd", "adh_avgpool", "adh_global_avgpool_bwd", "adh_mul", "adh_bilinear", "adh_bilinear_bwd"]
(VERSION, TO_NHWC8, NORM_NHWC8, NORM_BWD, NCHW_NHWC, NHWC_NCHW, BLEND, BLEND_NB, BLEND_BWD, SOFTMAX3, SOFTMAX3_BWD, SOFT_BLEND,
 SOFT_BLEND_BWD, ARGMAX3, COMPACT, GATHER, SCATTER, RED_NB, L1_PART, MSE_PART, SUM_PART, L1_BWD, MSE_BWD, XENT3, ADAM_STEP, ADD,
 AXPBY, MAXPOOL, MAXPOOL_BWD, AVGPOOL, GAP_BWD, MUL, BILINEAR, BILINEAR_BWD) = range(34)   # tools/host_emu/pointwise_main.cpp
LIB_CAPS = dict(PW_MAXBLK_EW=8192, PW_MAXBLK_SPATIAL=4096, PW_MAXBLK_IMAGE=2048, PW_MAXBLK_GATHER=1024, PW_MAXBLK_RED=2048,
                RED_ELEMS_PER_BLOCK=4096)
SMALL_CAPS = dict(PW_MAXBLK_EW=2, PW_MAXBLK_SPATIAL=2, PW_MAXBLK_IMAGE=2, PW_MAXBLK_GATHER=2, PW_MAXBLK_RED=3,
                  RED_ELEMS_PER_BLOCK=512)
CAPS = {"lib": LIB_CAPS, "small": SMALL_CAPS}
BOTH = pytest.mark.parametrize("caps", ["lib", "small"])
IPOISON, LPOISON = 0x5A5A5A5A, 0x5A5A5A5A5A5A5A5A     # Script.out's fill of an int32 / int64 output


def test_every_entry_point_is_called():
    src = open(os.path.join(E.ROOT, "adam-dehaze_amd", "csrc", "pointwise.hip")).read()
    assert re.findall(r'extern "C" int (adh_\w+)', src) == ENTRY_POINTS             # in the driver's order
    me = open(__file__).read()
    names = re.search(r"\(VERSION,(.*?)\) = range", me, re.S).group(1).replace("\n", " ").split(",")
    for name in ["VERSION"] + [n.strip() for n in names]:
        assert re.search(r"s\.call\(%s[,)]" % name, me), name


@pytest.fixture(scope="module")
def emus(tmp_path_factory):
    d = tmp_path_factory.mktemp("pointwise_emu")
    exe = {"lib": E.build(d, "pointwise", "pointwise_main.cpp", sanitize=E.FLOAT_CAST, exe="emu_lib"),
           "small": E.build(d, "pointwise", "pointwise_main.cpp", [f"{k}={v}" for k, v in SMALL_CAPS.items()],
                            sanitize=E.FLOAT_CAST, exe="emu_small")}
    return lambda caps: E.Script(exe[caps], d)


def _cdiv(a, b):
    return -(-a // b)


def _blocks(total, cap):
    return min(_cdiv(total, 256), cap)


def _twice(s, runs):
    for k1, k2 in zip(*runs):
        if k1 is not None:
            assert (s.after[k1] == s.after[k2]).all(), "two identical calls differ"
    return runs[0]


def _getf(s, k, what="output"):
    t = s.get(k)
    E.assert_written(t, what)
    return t


def _bits(t):
    return torch.as_tensor(t).contiguous().view(torch.int32)


def _ok(s, n=None):
    rcs = s.run()
    assert all(rc == 0 for rc in rcs), rcs
    return rcs


@BOTH
def test_version_and_block_counts(emus, caps):
    """the block counts the other tests compute from the caps are the program's"""
    s, c = emus(caps), CAPS[caps]
    want = [100]
    s.call(VERSION)
    for n in P.LOSS_N_HOST + [3 * 512 * 7]:
        s.call(RED_NB, [n])
        want.append(max(1, min(_cdiv(n, c["RED_ELEMS_PER_BLOCK"]), c["PW_MAXBLK_RED"])))
    for N, Hh, Ww in ((2, 5, 7), (2, 9, 31), (3, 40, 40)):
        s.call(BLEND_NB, [N, Hh, Ww])
        want.append(_blocks(N * Hh * Ww, c["PW_MAXBLK_SPATIAL"]))
    assert s.run() == want


# ------------------------------------------------------------------------------------------------ layout
@BOTH
def test_image_layout_bit_exact(emus, caps):
    """17 x 19 is 323 pixels an image: the second block is partly idle (and under the small caps the loop makes two trips).  The
    results are the same fp32 operations done in numpy float32, bit for bit: nothing can be contracted in (b - m) * is.  Channels
    3..7 are exactly +0."""
    s, N = emus(caps), 2
    mean, inv = np.float32(P.IMAGENET_MEAN), np.float32(1.0) / np.float32(P.IMAGENET_STD)
    cases = []
    for Hh, Ww in ((1, 1), (3, 5), (17, 19)):
        HW = Hh * Ww
        img = P.rand(N, 3, Hh, Ww, seed=HW)
        bimg = s.vec(img)
        for g_cs in (8, 12):
            g = P.randn(N * HW, 3, seed=HW + g_cs)
            bg = s.sin(g, g_cs, 4)
            runs = []
            for _ in range(2):
                o1, o2, gi = s.out(N * HW * 8), s.out(N * HW * 8), s.out(N * 3 * HW)
                s.call(TO_NHWC8, [N, Hh, Ww], [bimg, o1])
                s.call(NORM_NHWC8, [N, Hh, Ww], [bimg, o2], [*mean, *inv])
                s.call(NORM_BWD, [g_cs, N, Hh, Ww], [bg, gi], inv)
                runs.append((o1, o2, gi))
            cases.append((img, g, Hh, Ww, runs))
    _ok(s)
    for img, g, Hh, Ww, runs in cases:
        o1, o2, gi = _twice(s, runs)
        HW = Hh * Ww
        nhwc = img.permute(0, 2, 3, 1).reshape(N * HW, 3).numpy()
        o1, o2 = _getf(s, o1).view(N * HW, 8), _getf(s, o2).view(N * HW, 8)
        assert torch.equal(_bits(o1[:, :3]), _bits(nhwc)) and (_bits(o1[:, 3:]) == 0).all()
        assert torch.equal(_bits(o2[:, :3]), _bits((nhwc - mean) * inv)) and (_bits(o2[:, 3:]) == 0).all()
        want = (g.numpy() * inv).reshape(N, HW, 3).transpose(0, 2, 1)
        assert torch.equal(_bits(_getf(s, gi)), _bits(np.ascontiguousarray(want)).view(-1))


@BOTH
def test_transposes_bit_exact(emus, caps):
    """32 x 32 tiles through LDS: channel and pixel counts on both sides of a tile edge; the stores are scalar, so any stride
    (C, C + 5) is legal.  Bit-exact copies; the slack around the NHWC slice keeps its poison (Script.run checks it)."""
    s, N = emus(caps), 2
    cases = []
    for C in P.LAYOUT_C:
        for HW in P.LAYOUT_HW:
            src = P.randn(N, C, HW, seed=C * 100 + HW)
            bsrc = s.vec(src)
            for cs in (C, C + 5):
                bnhwc = s.sin(src.permute(0, 2, 1).reshape(N * HW, C), cs, 4)
                runs = []
                for _ in range(2):
                    dst, back = s.sout(N * HW, C, cs, 4), s.out(N * C * HW)
                    s.call(NCHW_NHWC, [N, C, HW, 1, cs], [bsrc, dst])
                    s.call(NHWC_NCHW, [cs, N, C, 1, HW], [bnhwc, back])
                    runs.append((dst, back))
                cases.append((src, C, HW, runs))
    _ok(s)
    for src, C, HW, runs in cases:
        dst, back = _twice(s, runs)
        assert torch.equal(_bits(s.get_slice(dst, N * HW, C)), _bits(src.permute(0, 2, 1).reshape(N * HW, C))), (C, HW)
        assert torch.equal(_bits(_getf(s, back)), _bits(src).view(-1)), (C, HW)


# ------------------------------------------------------------------------------------------------ branch heads
@BOTH
@pytest.mark.parametrize("r_cs,gd_cs", [(4, 4), (16, 8)])
def test_head_blend_all_modes(emus, caps, r_cs, gd_cs):
    """9 x 31 x 2 = 558 pixels: three blocks forward, and under the small caps two trips of both loops and an alpha partial row
    of two blocks.  g_r and g_gd are dense [P, r_cs] and [P, gd_cs] blocks: the kernel owns the whole pixel stride and zeroes the
    channels past 3 and 1.  r and gd are read from channel slices whose slack is NaN."""
    s, N = emus(caps), 2
    b_f, b_g, b_a = P.blend_bounds(host=1)
    cases = []
    for mode in range(5):
        for Hh, Ww in ((5, 7), (9, 31)):
            x, rb, gdb = P.blend_inputs(mode, N, Hh, Ww, r_cs, gd_cs, seed=11 + mode + Hh)
            g = P.randn(N, 3, Hh, Ww, seed=14 + mode + Hh)
            Pn, gated = N * Hh * Ww, mode in (2, 4)
            nb = _blocks(Pn, CAPS[caps]["PW_MAXBLK_SPATIAL"])
            bx, bg, br = s.vec(x), s.vec(g), s.sin(rb.view(Pn, r_cs)[:, :3], r_cs, 4)
            bgd = s.sin(gdb.view(Pn, gd_cs)[:, :1], gd_cs, 4) if gated else None
            ba = s.vec(torch.tensor([P.BLEND_ALPHA])) if mode == 0 else None
            runs = []
            for _ in range(2):
                out, g_r = s.out(N * 3 * Hh * Ww), s.out(Pn * r_cs)
                g_gd = s.out(Pn * gd_cs) if gated else None
                gap, ga = (s.out(nb), s.out(1)) if mode == 0 else (None, None)
                s.call(BLEND, [mode, r_cs, gd_cs if gated else 0, N, Hh, Ww], [bx, br, bgd, ba, out])
                s.call(BLEND_BWD, [mode, r_cs, gd_cs if gated else 0, N, Hh, Ww, nb], [bg, bx, br, bgd, ba, g_r, g_gd, gap])
                if mode == 0:
                    s.call(SUM_PART, [nb], [gap, ga], [1.0])
                runs.append((out, g_r, g_gd, gap, ga))
            cases.append((mode, x, rb, gdb, g, runs))
    _ok(s)
    for mode, x, rb, gdb, g, runs in cases:
        out, g_r, g_gd, gap, ga = _twice(s, runs)
        Pn = rb.shape[0] * rb.shape[1] * rb.shape[2]
        y, gr_ref, ggd_ref, ga_ref, terms = P.blend_ref_grads(mode, x, rb, gdb, g)
        assert float((_getf(s, out).view_as(y).double() - y).abs().max()) <= b_f, f"mode {mode}: forward"
        g_r = _getf(s, g_r).view(Pn, r_cs)
        assert P.rel(g_r[:, :3], gr_ref.reshape(Pn, 3)) <= b_g, f"mode {mode}: g_r"
        assert (_bits(g_r[:, 3:]) == 0).all(), "padding channels of g_r must be exactly 0"
        if g_gd is not None:
            g_gd = _getf(s, g_gd).view(Pn, gd_cs)
            assert P.rel(g_gd[:, :1], ggd_ref.reshape(Pn, 1)) <= b_g, f"mode {mode}: g_gd"
            assert (_bits(g_gd[:, 1:]) == 0).all(), "padding channels of g_gd must be exactly 0"
        if mode == 0:
            _getf(s, gap, "alpha partials")
            assert abs(float(_getf(s, ga)) - ga_ref) <= b_a * terms, "alpha gradient"


# ------------------------------------------------------------------------------------------------ routing
def test_softmax3_fwd_bwd(emus):
    """blocks of 64 lanes: N on both sides of one and two of them; the weight gradients arrive as nblk partials per image"""
    s = emus("lib")
    cases = []
    for N in (1, 63, 64, 65, 130):
        lg = P.logits3(N, 71 + N)
        blg = s.vec(lg)
        for T in (0.5, 1.0, 2.0):
            for nblk in (1, 3):
                gwp = P.randn(N, nblk, 3, seed=72 + N + nblk)
                bgwp = s.vec(gwp)
                runs = []
                for _ in range(2):
                    w, gl = s.out(N * 3), s.out(N * 3)
                    s.call(SOFTMAX3, [N], [blg, w], [T])
                    s.call(SOFTMAX3_BWD, [nblk, N], [w, bgwp, gl], [T])
                    runs.append((w, gl))
                cases.append((lg, gwp, T, runs))
    _ok(s)
    for lg, gwp, T, runs in cases:
        w, gl = _twice(s, runs)
        w64, gl64, Gmax = P.softmax3_ref(lg, gwp, T)
        b_w, b_g = P.softmax3_bounds(Gmax, T, host=1)
        assert float((_getf(s, w).view_as(w64).double() - w64).abs().max()) <= b_w
        assert float((_getf(s, gl).view_as(gl64).double() - gl64).abs().max()) <= b_g


def test_argmax3_and_route_compact(emus):
    """ties go to the first index, the output is int64; sel is [3][N] and only the first counts[cls] entries of a row are
    written, in batch order: the rest still hold their poison, exactly"""
    s = emus("lib")
    cases = []
    for N in (1, 37, 64, 65, 300):
        lg = torch.randint(0, 2, (N, 3), generator=P.gen(91 + N)).float()              # ties in most rows
        lg[0] = torch.tensor([1.0, 1.0, 1.0])
        if N > 1:
            lg[1] = torch.tensor([-1.0, 2.0, 2.0])
        blg = s.vec(lg)
        runs = []
        for _ in range(2):
            idx, sel, cnt = s.out(N, np.int64), s.out(3 * N, np.int32), s.out(3, np.int32)
            s.call(ARGMAX3, [N], [blg, idx])
            s.call(COMPACT, [N], [idx, sel, cnt])
            runs.append((idx, sel, cnt))
        cases.append((lg, N, runs))
    _ok(s)
    for lg, N, runs in cases:
        idx, sel, cnt = _twice(s, runs)
        idx = s.get(idx, np.int64)
        assert not (idx == LPOISON).any(), "an index was not written"
        assert torch.equal(idx, P.argmax3_first(lg)) and torch.equal(idx, torch.argmax(lg.double(), dim=1))
        sel, cnt = s.get(sel, np.int32).view(3, N), s.get(cnt, np.int32)
        for c in range(3):
            want = (idx == c).nonzero().flatten().to(torch.int32)
            k = int(cnt[c])
            assert k == want.numel()
            assert torch.equal(sel[c, :k], want), "members of a class must keep their batch order"
            assert (sel[c, k:] == IPOISON).all(), "written past counts[cls]"


SB_PER = [4, 12, 1028, 2060, 3, 5, 1027, 2059]      # per % 4 == 0: 16 bytes a lane; otherwise single floats, and the images of a
#                                                      batch do not start on 16-byte boundaries.  1028 / 4 = 257: two blocks; 2060 / 4
#                                                      = 515 and 2059: past two blocks of 256 lanes (the small caps' loop)


@BOTH
def test_soft_blend_fwd_bwd(emus, caps):
    s, N = emus(caps), 3
    b_o, b_w = P.soft_blend_bounds(host=1)
    w = torch.softmax(P.randn(N, 3, seed=81), dim=1).contiguous()
    bw = s.vec(w)
    cases = []
    for per in SB_PER:
        o = [P.rand(N, per, seed=82 + i + per) for i in range(3)]
        g = P.randn(N, per, seed=85 + per)
        bo, bg = [s.vec(t) for t in o], s.vec(g)
        variants = [(None, 0)] if per & 3 else [(None, 1), (0, 3), (1, 1), (2, 3)]          # (the null gradient, nblk)
        for null, nblk in variants:
            runs = []
            for _ in range(2):
                out = s.out(N * per)
                s.call(SOFT_BLEND, [N, per], [bw, *bo, out])
                gs, gwp = [None] * 3, None
                if nblk:
                    gs = [None if i == null else s.out(N * per) for i in range(3)]
                    gwp = s.out(N * nblk * 3)
                    s.call(SOFT_BLEND_BWD, [N, per, nblk], [bw, bg, *bo, *gs, gwp])
                runs.append((out, *gs, gwp))
            cases.append((o, g, per, nblk, runs))
    _ok(s)
    for o, g, per, nblk, runs in cases:
        out, g0, g1, g2, gwp = _twice(s, runs)
        y, g_ref, gw_ref, terms = P.soft_blend_ref(w, o, g)
        assert float((_getf(s, out).view_as(y).double() - y).abs().max()) <= b_o, f"per {per}"
        if nblk:
            for k, ref in zip((g0, g1, g2), g_ref):
                if k is not None:
                    assert float(((_getf(s, k).view_as(ref).double() - ref).abs() - EPS * ref.abs()).max()) <= 0, "one rounded product"
            gw = _getf(s, gwp).view(N, nblk, 3).double().sum(1)
            assert float(((gw - gw_ref).abs() - b_w * terms).max()) <= 0, f"per {per}: weight gradients"


@BOTH
def test_gather_scatter_images(emus, caps):
    """count < N, both paths; the rows scatter does not select keep their poison"""
    s, N = emus(caps), 5
    sel = torch.tensor([4, 0, 2], dtype=torch.int32)
    bsel = s.vec(sel, np.int32)
    cases = []
    for per in (12, 1028, 2060, 5, 1027, 2059):
        src = P.randn(N, per, seed=95 + per)
        bsrc = s.vec(src)
        runs = []
        for _ in range(2):
            dst, back = s.out(3 * per), s.out(N * per)
            s.call(GATHER, [3, per], [bsrc, bsel, dst])
            s.call(SCATTER, [3, per], [dst, bsel, back])
            runs.append((dst, back))
        cases.append((src, per, runs))
    _ok(s)
    for src, per, runs in cases:
        dst, back = _twice(s, runs)
        assert torch.equal(_bits(_getf(s, dst)).view(3, per), _bits(src[sel.long()]))
        back = _bits(s.get(back)).view(N, per)
        assert torch.equal(back[sel.long()], _bits(src[sel.long()]))
        assert (back[[1, 3]] == E.WPOISON).all(), "scatter wrote a row it was not given"


# ------------------------------------------------------------------------------------------------ losses
@BOTH
def test_diff_partial_sums(emus, caps):
    """a and b are blocks of exactly n floats: the float4 loop must end at n4 * 4 and the n % 4 tail belongs to one thread.
    2 * 4096 + 7 floats: three blocks in either build (under the small caps they loop as well)"""
    s, c = emus(caps), CAPS[caps]
    cases = []
    for n in P.LOSS_N_HOST:
        a, b = P.randn(n, seed=n), P.randn(n, seed=n + 1)
        ba, bb = s.vec(a), s.vec(b)
        nblk = max(1, min(_cdiv(n, c["RED_ELEMS_PER_BLOCK"]), c["PW_MAXBLK_RED"]))
        for sq in (0, 1):
            runs = []
            for _ in range(2):
                part, out = s.out(nblk), s.out(1)
                s.call(MSE_PART if sq else L1_PART, [n], [ba, bb, part])
                s.call(SUM_PART, [nblk], [part, out], [1.0 / n])
                runs.append((part, out))
            cases.append((a, b, sq, runs))
    _ok(s)
    for a, b, sq, runs in cases:
        part, out = _twice(s, runs)
        _getf(s, part, "partials")
        ref = P.diff_mean_ref(a, b, sq)
        assert abs(float(_getf(s, out)) - ref) <= P.LOSS_REL * ref, (a.numel(), sq)


def test_sum_partials(emus):
    """one workgroup of 256 lanes over nblk partials, summed in float64 and stored once: EPS of the result, and float64's own
    roundings of the sum of |terms|"""
    s = emus("lib")
    cases = []
    for nblk in (1, 255, 256, 257, 700):
        part = P.randn(nblk, seed=nblk)
        bp = s.vec(part)
        runs = []
        for _ in range(2):
            out = s.out(1)
            s.call(SUM_PART, [nblk], [bp, out], [0.125])
            runs.append((out,))
        cases.append((part, runs))
    _ok(s)
    for part, runs in cases:
        (out,) = _twice(s, runs)
        ref = float(part.double().sum()) * 0.125
        assert abs(float(_getf(s, out)) - ref) <= EPS * abs(ref) + 2.0 ** -43 * float(part.double().abs().sum())


@BOTH
def test_loss_gradients(emus, caps):
    """sign(0) = 0; upstream null (= 1) and a device scalar"""
    s = emus(caps)
    bup = s.vec(torch.tensor([0.75]))
    cases = []
    for n in (1, 5, 257, 1000):
        a, b = P.randn(n, seed=101 + n), P.randn(n, seed=102 + n)
        b[::3] = a[::3]
        ba, bb = s.vec(a), s.vec(b)
        for up in (None, bup):
            runs = []
            for _ in range(2):
                gl, gm = s.out(n), s.out(n)
                s.call(L1_BWD, [n], [ba, bb, up, gl], [1.0 / n])
                s.call(MSE_BWD, [n], [ba, bb, up, gm], [1.0 / n])
                runs.append((gl, gm))
            cases.append((a, b, 1.0 if up is None else 0.75, runs))
    _ok(s)
    for a, b, u, runs in cases:
        gl, gm = _twice(s, runs)
        gl, gm = _getf(s, gl), _getf(s, gm)
        assert (_bits(gl[::3]) == 0).all(), "sign(0) = 0"
        for got, sq, k in ((gl, 0, P.L1_BWD_EPS), (gm, 1, P.MSE_BWD_EPS)):
            ref = P.diff_bwd_ref(a, b, sq, u)
            assert float(((got.double() - ref).abs() - k * EPS * ref.abs()).max()) <= 0, (a.numel(), sq, u)


def test_cross_entropy3(emus):
    """one block: N on both sides of its 256 lanes; dlogits null and non-null"""
    s = emus("lib")
    cases = []
    for N in (1, 7, 256, 257, 300):
        lg, lab = P.cross_entropy3_inputs(N)
        blg, blab = s.vec(lg), s.vec(lab, np.int64)
        runs = []
        for _ in range(2):
            loss, dl, loss0 = s.out(1), s.out(N * 3), s.out(1)
            s.call(XENT3, [N], [blg, blab, loss, dl])
            s.call(XENT3, [N], [blg, blab, loss0, None])
            runs.append((loss, dl, loss0))
        cases.append((lg, lab, runs))
    _ok(s)
    for lg, lab, runs in cases:
        loss, dl, loss0 = _twice(s, runs)
        ref, dref, b_l, b_d = P.cross_entropy3_ref(lg, lab, host=1)
        assert abs(float(_getf(s, loss)) - ref) <= b_l
        assert torch.equal(_bits(s.get(loss)), _bits(s.get(loss0))), "the loss does not depend on dlogits being asked for"
        assert float((_getf(s, dl).view_as(dref).double() - dref).abs().max()) <= b_d


# ------------------------------------------------------------------------------------------------ optimiser and elementwise
@BOTH
def test_adam_step(emus, caps):
    """p, m and v are blocks of exactly n floats, updated in place; 1500 elements: six blocks, two trips under the small caps"""
    s = emus(caps)
    f32 = lambda v: float(np.float32(v))
    kw = dict(lr=f32(1e-3), beta1=f32(0.9), beta2=f32(0.999), eps=f32(1e-8), wd=f32(1e-2))
    cases = []
    for n in P.ADAM_STEP_N:
        for repeats in (1, 2, 3):
            for step in (0, 7):
                p0, g, m0, v0 = P.adam_step_case(n, seed=n + 10 * repeats + step)
                bg = s.vec(g)
                runs = []
                for _ in range(2):
                    p, m, v = s.out(n, init=p0), s.out(n, init=m0), s.out(n, init=v0)
                    s.call(ADAM_STEP, [n, step, repeats], [p, bg, m, v], [kw["lr"], kw["beta1"], kw["beta2"], kw["eps"], kw["wd"]])
                    runs.append((p, m, v))
                cases.append((p0, g, m0, v0, step, repeats, runs))
    _ok(s)
    for p0, g, m0, v0, step, repeats, runs in cases:
        got = _twice(s, runs)
        refs, bounds = P.adam_step_ref(p0, g, m0, v0, step, repeats, **kw)
        for what, k, ref, e in zip("pmv", got, refs, bounds):
            E.assert_bound(s.get(k), ref, e, f"adam_step n={p0.numel()} repeats={repeats} step={step}: {what}")


@BOTH
def test_add_mul_axpby(emus, caps):
    s = emus(caps)
    cases, ax = [], []
    for n in (1, 5, 257, 1000):
        a, b = P.randn(n, seed=n), P.randn(n, seed=n + 1)
        ba, bb = s.vec(a), s.vec(b)
        runs = []
        for _ in range(2):
            sm, m = s.out(n, init=a), s.out(n)
            s.call(ADD, [n], [sm, bb])
            s.call(MUL, [n], [m, ba, bb])
            runs.append((sm, m))
        cases.append((a, b, runs))
    for Pn in (1, 37):
        for C in (4, 12):
            for pad_d, pad_s in ((0, 0), (4, 8), (8, 4)):
                src, d0 = P.randn(Pn, C, seed=Pn + C), P.randn(Pn, C, seed=Pn + C + 1)
                bsrc = s.sin(src, C + pad_s, 4)
                runs = []
                for _ in range(2):
                    dst = s.sout(Pn, C, C + pad_d, 4)                   # a = 0 must not read dst: its poison is a NaN
                    acc = s.sout(Pn, C, C + pad_d, 4, init=d0)
                    s.call(AXPBY, [C + pad_d, C + pad_s, Pn, C], [dst, bsrc], [0.0, 1.5])
                    s.call(AXPBY, [C + pad_d, C + pad_s, Pn, C], [acc, bsrc], [0.5, -2.0])
                    runs.append((dst, acc))
                ax.append((src, d0, Pn, C, runs))
    _ok(s)
    for a, b, runs in cases:
        sm, m = _twice(s, runs)
        # one correctly rounded operation each: equal to the float64 result rounded to fp32
        assert torch.equal(s.get(sm), (a.double() + b.double()).float()) and torch.equal(_getf(s, m), (a.double() * b.double()).float())
    for src, d0, Pn, C, runs in ax:
        dst, acc = _twice(s, runs)
        got = s.get_slice(dst, Pn, C)
        assert torch.isfinite(got).all() and torch.equal(got, src * 1.5), "a = 0: one exactly scaled product"
        ref = d0.double() * 0.5 - 2.0 * src.double()                  # d * 0.5 and s * -2 are exact; one rounding of the sum
        assert float(((s.get_slice(acc, Pn, C).double() - ref).abs() - EPS * ref.abs()).max()) <= 0


# ------------------------------------------------------------------------------------------------ pools
MP_SHAPES = [(2, 7, 9, 8), (1, 5, 13, 4), (1, 37, 31, 8)]       # the last: more than 512 outputs x quads (the small caps' loop)


@BOTH
def test_maxpool_ties_and_gradient(emus, caps):
    """values in {0, 1, 2}, so ties are everywhere; values, indices and gradient are exact.  One case reads x from a channel
    slice (x_cs = C + 8 at offset 4) and moves the gradients through wider buffers (g_cs = C + 4, gx_cs = C + 12)."""
    s = emus(caps)
    todo = [(sh, cfg, 0, 0, 0) for sh in MP_SHAPES for cfg in P.MP_CFG] + [((2, 7, 9, 8), (3, 2, 1), 8, 4, 12)]
    cases = []
    for (N, Hh, Ww, C), (k, st, p), px, pg, pgx in todo:
        xb, gb = P.maxpool_inputs(N, Hh, Ww, k, st, p, C, C, seed=N + Hh + Ww + 10 * k + px)
        OH, OW = gb.shape[1], gb.shape[2]
        bx, bg = s.sin(xb.view(-1, C), C + px, 4 if px else 0), s.sin(gb.view(-1, C), C + pg, 4 if pg else 0)
        runs = []
        for _ in range(2):
            out, idx = s.sout(N * OH * OW, C, C, 0), s.out(N * OH * OW * C, np.int32)
            gx = s.sout(N * Hh * Ww, C, C + pgx, 4 if pgx else 0)
            s.call(MAXPOOL, [C + px, N, Hh, Ww, C, k, st, p, C], [bx, out, idx])
            s.call(MAXPOOL_BWD, [C + pg, N, OH, OW, C, k, st, p, Hh, Ww, C + pgx], [bg, idx, gx])
            runs.append((out, idx, gx))
        cases.append((xb, gb, k, st, p, runs))
    _ok(s)
    for xb, gb, k, st, p, runs in cases:
        out, idx, gx = _twice(s, runs)
        N, Hh, Ww, C = xb.shape
        OH, OW = gb.shape[1], gb.shape[2]
        y, ind, gref = P.maxpool_ref(xb, gb, k, st, p)
        assert torch.equal(P.nchw64(s.get_slice(out, N * OH * OW, C).view(N, OH, OW, C)), y), "pooled values"
        got = s.get(idx, np.int32)
        assert not (got == IPOISON).any()
        assert torch.equal(got.view(N, OH, OW, C).permute(0, 3, 1, 2).long(), ind), "arg-max indices (first on ties)"
        assert torch.equal(P.nchw64(s.get_slice(gx, N * Hh * Ww, C).view(N, Hh, Ww, C)), gref), "input gradient"


@BOTH
def test_avgpool_floor(emus, caps):
    """AvgPool2d(k) floors: the last rows and columns that fit no window hold NaN, so a finite result proves they are not read.
    k * k - 1 fp32 adds of values >= 0 and a product with fp32(1 / k^2) (exact for k = 2): k^2 + 1 EPS (4 for k = 2, the GPU
    test's).  33 x 40: 640 outputs x quads, the small caps' loop."""
    s, N, C = emus(caps), 2, 8
    cases = []
    for k, Hh, Ww in ((2, 9, 13), (2, 15, 16), (7, 9, 13), (7, 15, 16), (2, 33, 40)):
        OH, OW = Hh // k, Ww // k
        x = P.rand(N, Hh, Ww, C, seed=Hh + k)
        x[:, OH * k:] = float("nan")
        x[:, :, OW * k:] = float("nan")
        bx = s.sin(x.view(-1, C), C + 8, 4)
        runs = []
        for _ in range(2):
            out = s.sout(N * OH * OW, C, C + 4, 4)
            s.call(AVGPOOL, [C + 8, N, Hh, Ww, C, k, C + 4], [bx, out])
            runs.append((out,))
        cases.append((x, k, OH, OW, runs))
    _ok(s)
    for x, k, OH, OW, runs in cases:
        (out,) = _twice(s, runs)
        ref = F.avg_pool2d(P.nchw64(x[:, :OH * k, :OW * k]), k).permute(0, 2, 3, 1)
        got = s.get_slice(out, N * OH * OW, C).view(N, OH, OW, C)
        assert torch.isfinite(got).all(), "a dropped row or column was read"
        assert P.rel(got, ref) <= (4 if k == 2 else k * k + 1) * EPS


@BOTH
def test_global_avgpool_bwd(emus, caps):
    """g * fp32(1 / HW): two roundings of each element"""
    s, N = emus(caps), 2
    cases = []
    for C in (1, 5, 64):
        for HW in (1, 49):
            g = P.randn(N, C, seed=C + HW)
            bg = s.vec(g)
            for pad in (0, 3):
                runs = []
                for _ in range(2):
                    gx = s.sout(N * HW, C, C + pad, 4)
                    s.call(GAP_BWD, [N, HW, C, C + pad], [bg, gx])
                    runs.append((gx,))
                cases.append((g, HW, C, runs))
    _ok(s)
    for g, HW, C, runs in cases:
        (gx,) = _twice(s, runs)
        gref = (g.double() / HW)[:, None, :].expand(N, HW, C).reshape(N * HW, C)
        assert float(((s.get_slice(gx, N * HW, C).double() - gref).abs() - 3 * EPS * gref.abs()).max()) <= 0


# ------------------------------------------------------------------------------------------------ bilinear resize
def _bilinear_case(s, case):
    N, Hh, Ww, C, OH, OW, align, x_cs, out_cs = case
    off = 4 if out_cs > C else 0
    xb, g = P.bilinear_inputs(N, Hh, Ww, C, OH, OW, x_cs)
    bx, bg = s.sin(xb.view(-1, x_cs)[:, :C], x_cs, 0), s.vec(g)
    runs = []
    for _ in range(2):
        ob, gx = s.sout(N * OH * OW, C, out_cs, off), s.out(N * Hh * Ww * C)
        s.call(BILINEAR, [x_cs, N, Hh, Ww, C, OH, OW, align, out_cs], [bx, ob])
        s.call(BILINEAR_BWD, [C, N, Hh, Ww, C, OH, OW, align, C], [bg, gx])
        runs.append((ob, gx))
    return xb[..., :C], g, runs


def _bilinear_check(s, case, x, g, runs):
    N, Hh, Ww, C, OH, OW, align = case[:7]
    ob, gx = _twice(s, runs)
    y, gref = P.bilinear_ref(x, g, OH, OW, align)
    b_f, b_b, ds = P.bilinear_bounds(Hh, Ww, OH, OW, align, host=1)
    e_f = P.rel(s.get_slice(ob, N * OH * OW, C).view(N, OH, OW, C), y)
    assert e_f <= b_f, f"{case} forward: {e_f:.3e} (source-coordinate error {ds:.3e})"
    e_b = P.rel(_getf(s, gx).view(N, Hh, Ww, C), gref)
    assert e_b <= b_b, f"{case} backward: {e_b:.3e} (source-coordinate error {ds:.3e})"


@BOTH
def test_bilinear_cases(emus, caps):
    """the GPU test's cases but the 256 x 512 plane, at its bounds"""
    s = emus(caps)
    cases = [(c, *_bilinear_case(s, c)) for c in P.BL_CASES[:9] if c[1] < 100]
    _ok(s)
    for c, x, g, runs in cases:
        _bilinear_check(s, c, x, g, runs)


def test_bilinear_detector_downsampling(emus):
    """301 x 401 -> 200 x 266: the one case whose backward takes seconds on CPU threads; a script of its own"""
    s = emus("lib")
    c = P.BL_CASES[6]
    assert c[1:3] == (301, 401)
    x, g, runs = _bilinear_case(s, c)
    _ok(s)
    _bilinear_check(s, c, x, g, runs)


@pytest.mark.parametrize("axis", ["H", "W"])
def test_bilinear_one_dimensional_sweep(emus, axis):
    """every (in, out) pair of 1..20 x 1..20, both alignments, along one axis with the other of extent 1 (C = 4 forward, C = 1
    backward), against float64 F.interpolate and its autograd: pins that bilin_cover misses no contributing output and that no
    source index leaves [0, in - 1] (the input and the gradient are blocks of exactly their floats)."""
    s = emus("lib")
    cases = []
    for n_in in range(1, 21):
        for n_out in range(1, 21):
            for align in (0, 1):
                Hh, Ww, OH, OW = (n_in, 1, n_out, 1) if axis == "H" else (1, n_in, 1, n_out)
                x, g = P.rand(1, Hh, Ww, 4, seed=n_in * 21 + n_out), P.rand(1, OH, OW, 1, seed=n_out * 21 + n_in + 1)
                bx, bg = s.vec(x), s.vec(g)
                runs = []
                for _ in range(2):
                    ob, gx = s.out(n_out * 4), s.out(n_in)
                    s.call(BILINEAR, [4, 1, Hh, Ww, 4, OH, OW, align, 4], [bx, ob])
                    s.call(BILINEAR_BWD, [1, 1, Hh, Ww, 1, OH, OW, align, 1], [bg, gx])
                    runs.append((ob, gx))
                cases.append(((Hh, Ww, OH, OW, align), x, g, runs))
    _ok(s)
    for (Hh, Ww, OH, OW, align), x, g, runs in cases:
        ob, gx = _twice(s, runs)
        b_f, b_b, ds = P.bilinear_bounds(Hh, Ww, OH, OW, align, host=1)
        y, _ = P.bilinear_ref(x, P.rand(1, OH, OW, 4), OH, OW, align)
        _, gref = P.bilinear_ref(P.rand(1, Hh, Ww, 1), g, OH, OW, align)
        assert P.rel(_getf(s, ob).view(1, OH, OW, 4), y) <= b_f, (Hh, Ww, OH, OW, align)
        assert P.rel(_getf(s, gx).view(1, Hh, Ww, 1), gref) <= b_b, (Hh, Ww, OH, OW, align)


# ------------------------------------------------------------------------------------------------ argument rejections
def test_argument_rejections_write_nothing(emus):
    """the contract of include/adam_dehaze_hip.h: every bad call returns ADH_E_ARG before anything is launched, so every output
    keeps its poison (and no block is touched out of bounds: the buffers are as small as a legal call's)"""
    s = emus("lib")
    N, Hh, Ww, C = 2, 6, 8, 8
    x16 = s.sin(P.rand(N * Hh * Ww, C), 16, 4)                 # a legal channel slice: cs 16, 16-byte aligned
    xo = s.raw(np.zeros(N * Hh * Ww * C + 1, np.float32), 4)   # a base one float off 16-byte alignment
    out, idx = s.out(N * Hh * Ww * 16), s.out(N * Hh * Ww * C, np.int32)
    outo = s.raw(np.full(N * Hh * Ww * 16 + 1, E.WPOISON, np.uint32), 4)
    bad = []
    for x_cs, out_cs, n, h, w in ((10, 8, N, Hh, Ww), (16, 10, N, Hh, Ww), (4, 8, N, Hh, Ww), (16, 4, N, Hh, Ww), (16, 8, 0, Hh, Ww),
                                  (16, 8, N, 0, Ww), (16, 8, N, Hh, 0), (16, 8, 65536, Hh, Ww)):
        bad.append(s.call(MAXPOOL, [x_cs, n, h, w, C, 2, 2, 0, out_cs], [x16, out, idx]))
        bad.append(s.call(AVGPOOL, [x_cs, n, h, w, C, 2, out_cs], [x16, out]))
        bad.append(s.call(BILINEAR, [x_cs, n, h, w, C, 3, 5, 0, out_cs], [x16, out]))
    bad.append(s.call(MAXPOOL, [8, N, Hh, Ww, C, 2, 2, 0, 8], [xo, out, idx]))
    bad.append(s.call(AVGPOOL, [8, N, Hh, Ww, C, 2, 8], [x16, outo]))
    bad.append(s.call(BILINEAR, [8, N, Hh, Ww, C, 3, 5, 1, 8], [xo, out]))
    # backward entry points
    g, gidx = s.vec(P.rand(N * 3 * 4 * 8)), s.vec(torch.zeros(N * 3 * 4 * 4, dtype=torch.int32), np.int32)
    ok = dict(g_cs=8, N=N, OH=3, OW=4, C=4, k=2, s=2, p=0, H=Hh, W=Ww, gx_cs=8)
    for d in (dict(g_cs=3), dict(gx_cs=3), dict(N=0), dict(OH=0), dict(OW=5), dict(OH=4), dict(C=0), dict(H=0), dict(W=0), dict(p=-1),
              dict(p=2), dict(k=0), dict(s=0)):
        a = {**ok, **d}
        bad.append(s.call(MAXPOOL_BWD, [a[k] for k in ("g_cs", "N", "OH", "OW", "C", "k", "s", "p", "H", "W", "gx_cs")], [g, gidx, out]))
    for g_cs, gx_cs, n in ((3, 8, N), (8, 3, N), (8, 8, 0)):
        bad.append(s.call(BILINEAR_BWD, [g_cs, n, Hh, Ww, 4, 3, 4, 0, gx_cs], [g, out]))
    for n, hw, c, gx_cs in ((N, 48, 4, 3), (0, 48, 4, 8), (N, 0, 4, 8), (N, 48, 0, 8)):
        bad.append(s.call(GAP_BWD, [n, hw, c, gx_cs], [g, out]))
    for g_cs, n, h, w in ((2, N, Hh, Ww), (8, 0, Hh, Ww), (8, N, 0, Ww), (8, N, Hh, 0)):
        bad.append(s.call(NORM_BWD, [g_cs, n, h, w], [g, out], [1.0, 1.0, 1.0]))
    # sizes of the head blends and the layout changes
    one = s.vec(torch.tensor([P.BLEND_ALPHA]))
    for n, h, w in ((0, Hh, Ww), (N, 0, Ww), (N, Hh, 0)):
        for mode in (0, 2):
            bad.append(s.call(BLEND, [mode, 4, 4, n, h, w], [g, g, g, one, out]))
            bad.append(s.call(BLEND_BWD, [mode, 4, 4, n, h, w, _blocks(n * h * w, 4096)], [g, g, g, g, one, out, out, out]))
        bad.append(s.call(TO_NHWC8, [n, h, w], [g, out]))
        bad.append(s.call(NORM_NHWC8, [n, h, w], [g, out], [0, 0, 0, 1, 1, 1]))
        bad.append(s.call(NCHW_NHWC, [n, 3, h, w, 4], [g, out]))
        bad.append(s.call(NHWC_NCHW, [4, n, 3, h, w], [g, out]))
    bad.append(s.call(BLEND, [2, 2, 4, N, 2, 2], [g, g, g, one, out]))
    bad.append(s.call(BLEND, [2, 4, 0, N, 2, 2], [g, g, g, one, out]))
    bad.append(s.call(BLEND_BWD, [0, 4, 4, N, 2, 2, 2], [g, g, g, g, one, out, out, out]))          # nblk is 1
    bad.append(s.call(NCHW_NHWC, [N, 3, 2, 2, 2], [g, out]))
    bad.append(s.call(NHWC_NCHW, [2, N, 3, 2, 2], [g, out]))
    bad.append(s.call(TO_NHWC8, [N, 2, 2], [g, outo]))
    # what moves 16 bytes per lane, at a base one float off
    sel = s.vec(torch.tensor([1, 0], dtype=torch.int32), np.int32)
    bad.append(s.call(SOFT_BLEND, [2, 16], [g, xo, g, g, out]))
    bad.append(s.call(SOFT_BLEND, [2, 16], [g, g, g, g, outo]))
    bad.append(s.call(SOFT_BLEND_BWD, [2, 16, 1], [g, g, g, g, g, outo, None, None, out]))
    bad.append(s.call(SOFT_BLEND_BWD, [2, 18, 1], [g, g, g, g, g, out, None, None, out]))           # per % 4
    bad.append(s.call(GATHER, [2, 16], [xo, sel, out]))
    bad.append(s.call(SCATTER, [2, 16], [g, sel, outo]))
    bad.append(s.call(L1_PART, [16], [xo, g, out]))
    bad.append(s.call(MSE_PART, [16], [g, xo, out]))
    bad.append(s.call(AXPBY, [8, 8, 2, 8], [outo, g], [0.0, 1.0]))
    bad.append(s.call(AXPBY, [4, 8, 2, 8], [out, g], [0.0, 1.0]))
    bad.append(s.call(AXPBY, [8, 6, 2, 8], [out, g], [0.0, 1.0]))
    # null pointers and zero sizes of the rest
    bad.append(s.call(SOFTMAX3, [0], [g, out], [1.0]))
    bad.append(s.call(SOFTMAX3, [2], [g, out], [0.0]))
    bad.append(s.call(SOFTMAX3_BWD, [0, 2], [g, g, out], [1.0]))
    bad.append(s.call(ARGMAX3, [0], [g, out]))
    bad.append(s.call(COMPACT, [0], [g, out, out]))
    bad.append(s.call(SUM_PART, [0], [g, out], [1.0]))
    bad.append(s.call(L1_BWD, [0], [g, g, None, out], [1.0]))
    bad.append(s.call(MSE_BWD, [4], [g, None, None, out], [1.0]))
    bad.append(s.call(XENT3, [0], [g, g, out, out]))
    bad.append(s.call(ADAM_STEP, [4, -1, 1], [out, g, out, out], [1e-3, 0.9, 0.999, 1e-8, 0.0]))
    bad.append(s.call(ADAM_STEP, [4, 0, 0], [out, g, out, out], [1e-3, 0.9, 0.999, 1e-8, 0.0]))
    bad.append(s.call(ADD, [0], [out, g]))
    bad.append(s.call(MUL, [4], [out, g, None]))
    rcs = s.run()
    assert [rcs[k] for k in bad] == [E.ADH_E_ARG] * len(bad), [(k, rcs[k]) for k in bad if rcs[k] != E.ADH_E_ARG]
    for k in (out, idx, outo):
        assert s.unchanged(k), "a rejected call wrote to an output"
