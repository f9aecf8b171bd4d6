"""csrc/bn_act.hip without a GPU: the source file, compiled by the host C++ compiler against the stand-in header of
tools/host_emu (its ADH_HOST_EMU_STREAM section) with AddressSanitizer and UndefinedBehaviorSanitizer, run as a stand-alone
program on heap blocks of exactly their sizes (tests/_hostemu.py) and held to the float64 restatements and bounds of
tests/_stream_ref64.py.  A second program is built with small block caps and blocking factors (SMALL below), so that the
grid-stride loops and the multi-block partial rows run at a few hundred pixels; its caps of 3 blocks are a multiple of
CQ / gcd(CQ, 256) for the C = 8 and 24 it runs.  The host compiler does not contract a * b + c: where a bound counts one
rounding for such an expression on the GPU it gets one more here (`host=1`).

adh_bn_apply's mask nibbles travel between neighbouring lanes by __shfl_xor inside a loop that the lanes of a workgroup leave
after different trip counts; the emulator's shuffle synchronises the two lanes only, and a lane left without its partner shows
as a timeout."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest
import torch

from tests import _hostemu as E
from tests import _stream_ref64 as R

FINALIZE, PSUMS, FIN_SUMS, BWD_FIN_SUMS, FOLD_EVAL, APPLY, BWD_NBLK, BWD_REDUCE, BWD_FIN, BWD_FIN_C, BWD_APPLY = range(11)
SMALL = {"EW_UNROLL": 2, "EW_MAXBLK_APPLY": 3, "EW_MAXBLK_BWD": 3, "BNB_PPB": 32, "BNB_UNROLL": 2}
ACT_LIST = [R.ACT_NONE, R.ACT_RELU, R.ACT_RELU6, R.ACT_HARDSWISH, R.ACT_HARDSIGMOID]


@pytest.fixture(scope="module")
def emus(tmp_path_factory):
    d = tmp_path_factory.mktemp("bn_act_emu")
    dirs = {False: d / "default", True: d / "small"}
    for sub in dirs.values():
        sub.mkdir()
    with ThreadPoolExecutor(2) as pool:                       # the two compilations side by side, each in its own directory
        exe = dict(zip((False, True), pool.map(lambda small: E.build(
            dirs[small], "bn_act", "bn_act_main.cpp", [f"{k}={v}" for k, v in SMALL.items()] if small else ()), (False, True))))
    return lambda small=False: E.Script(exe[small], d)


# ------------------------------------------------------------------------------------------------ the finalize family
FIN_VARIANTS = [
    # affine, running statistics, save outputs, counter, count
    (True, True, True, True, 4.2e6),
    (False, False, False, False, 1.0),
    (True, False, True, False, 2.0),
    (False, True, False, True, 2.0),
]


@pytest.mark.parametrize("nblk", [1, 31, 33, 97, 129, 300])
def test_finalize_family_vs_float64(emus, nblk):
    """nblk on both sides of the unrolled loops' bounds (b + 96 < nblk at four rows a trip, b + 32 < nblk at two) and in their
    tails; C = 33: the second workgroup has one live channel; pitch 40 > C with NaN padding; count = 1 and 2"""
    s = emus()
    C, pitch = 33, 40
    g = R.gen(nblk)
    gamma, beta = torch.randn(C, generator=g), torch.randn(C, generator=g)
    rm0, rv0 = torch.randn(C, generator=g), torch.rand(C, generator=g) + 0.5
    invstd = torch.rand(C, generator=g) + 0.1
    todo = []
    for vi, (affine, running, save, counter, count) in enumerate(FIN_VARIANTS):
        part = R.partials(nblk, C, pitch, count, seed=nblk * 7 + vi)
        bpart = s.vec(part.view(-1)[:part.numel() - (pitch - C)])             # the last row ends at its last channel
        bg, bb = (s.vec(gamma), s.vec(beta)) if affine else (None, None)

        def outs():
            return {"scale": s.out(C), "shift": s.out(C), "mean": s.out(C) if save else None,
                    "invstd": s.out(C) if save else None, "rm": s.out(C, init=rm0) if running else None,
                    "rv": s.out(C, init=rv0) if running else None, "nbt": s.raw(np.array([5], np.int64)) if counter else None}

        def order(o):
            return [o["rm"], o["rv"], o["scale"], o["shift"], o["mean"], o["invstd"], o["nbt"]]

        o1, o2, bsums = outs(), outs(), s.out(2 * C + 1, np.float64)
        s.call(FINALIZE, [nblk, pitch, C], [bpart, bg, bb] + order(o1), [count, R.BN_EPS, R.MOM])
        s.call(PSUMS, [nblk, pitch, C], [bpart, bsums], [count])
        s.call(FIN_SUMS, [C], [bsums, bg, bb] + order(o2), [R.BN_EPS, R.MOM])
        # the backward finalizers read the same kind of rows: dense (pitch C) and centered (pitch 40)
        rows = torch.full((nblk, 2, pitch), float("nan"))
        rows[:, :, :C] = torch.randn(nblk, 2, C, generator=g) * 10
        dense = rows[:, :, :C].contiguous()
        dg0, db0 = torch.randn(C, generator=g), torch.randn(C, generator=g)
        acc = vi % 2
        bw = []
        for fn, ints, src in ((BWD_FIN, [nblk, C, acc], dense), (BWD_FIN_C, [nblk, pitch, C, acc],
                                                                 rows.view(-1)[:rows.numel() - (pitch - C)])):
            b = {"dg": s.out(C, init=dg0 if acc else None) if save else None,
                 "db": s.out(C, init=db0 if acc else None) if running else None, "coef": s.out(3 * C)}
            s.call(fn, ints, [s.vec(src), bg, s.vec(invstd), b["dg"], b["db"], b["coef"]], [count])
            bw.append(b)
        todo.append((affine, count, part, o1, o2, bsums, rows, acc, dg0, db0, bw))
    rcs = s.run()
    assert rcs == [0] * len(rcs), rcs
    for affine, count, part, o1, o2, bsums, rows, acc, dg0, db0, bw in todo:
        tag = f"nblk={nblk} affine={affine} count={count}"
        sums = s.get(bsums, np.float64)
        S, Q = part[:, 0, :C].double(), part[:, 1, :C].double()
        # float64 sums in another order: nblk roundings of 2^-53 of the terms
        E.assert_bound(sums[:C], S.sum(0), nblk * R.U64 * S.abs().sum(0), tag + " sum y")
        E.assert_bound(sums[C:2 * C], Q.sum(0), nblk * R.U64 * Q.abs().sum(0), tag + " sum y^2")
        assert float(sums[2 * C]) == count, "sums[2C] carries the element count exactly"
        ref = R.finalize64(part, C, count, gamma if affine else None, beta if affine else None, rm0, rv0, host=1)
        for o, form in ((o1, "finalize"), (o2, "finalize_sums")):
            for name in ("scale", "shift", "mean", "invstd", "rm", "rv"):
                if o[name] is not None:
                    got = s.get(o[name])
                    E.assert_written(got, name)
                    E.assert_bound(got, *ref[name], f"{form} {name} ({tag})")
            if o["nbt"] is not None:
                assert int(s.get(o["nbt"], np.int64)) == 6, "num_batches_tracked goes up by exactly 1 (one writer)"
        Sr, Qr = rows[:, 0, :C].double(), rows[:, 1, :C].double()
        for b, centered in zip(bw, (False, True)):
            S64 = Sr.sum(0)
            Q64 = Qr.sum(0) * (invstd.double() if centered else 1.0)
            # float64 sums (and the product by invstd) rounded to fp32 once; accumulate adds one fp32 addition
            eS = (R.EPS * S64.abs() + (nblk + 2) * R.U64 * Sr.abs().sum(0))
            eQ = (R.EPS * Q64.abs() + (nblk + 2) * R.U64 * Qr.abs().sum(0) * (invstd.double() if centered else 1.0))
            for key, ref64, e, prior in (("dg", Q64, eQ, dg0), ("db", S64, eS, db0)):
                if b[key] is not None:
                    got = s.get(b[key])
                    E.assert_written(got, key)
                    if acc:
                        E.assert_bound(got, ref64 + prior.double(), e + R.EPS * (ref64.abs() + e + prior.double().abs()),
                                       f"{key} accumulated ({tag})")
                    else:
                        E.assert_bound(got, ref64, e, f"{key} ({tag}, centered={centered})")
            coef = s.get(b["coef"]).view(3, C)
            E.assert_written(coef, "coef")
            assert torch.equal(coef[0], (gamma if affine else torch.ones(C)) * invstd), "coef[0] = gamma * invstd"
            E.assert_bound(coef[1], S64 / count, eS / count + R.U64 * (S64 / count).abs(), f"mean g ({tag})")
            E.assert_bound(coef[2], Q64 / count, eQ / count + R.U64 * (Q64 / count).abs(), f"mean g xhat ({tag})")


@pytest.mark.parametrize("C", [1, 33, 300])
def test_bwd_finalize_sums_and_fold_eval(emus, C):
    s = emus()
    g = R.gen(C)
    local = torch.randn(2 * C + 1, dtype=torch.float64, generator=g) * 100
    glob = local + torch.randn(2 * C + 1, dtype=torch.float64, generator=g) * 100
    local[2 * C], glob[2 * C] = 3000.0, 12000.0
    gamma, invstd = torch.randn(C, generator=g), torch.rand(C, generator=g) + 0.1
    dg0, db0 = torch.randn(C, generator=g), torch.randn(C, generator=g)
    bl, bgl, bgam, bis = s.vec(local, np.float64), s.vec(glob, np.float64), s.vec(gamma), s.vec(invstd)
    runs = []
    for acc, with_gamma, with_dg, with_db in [(0, True, True, True), (1, True, True, True), (0, False, False, True),
                                              (1, True, True, False)]:
        bdg = s.out(C, init=dg0 if acc else None) if with_dg else None
        bdb = s.out(C, init=db0 if acc else None) if with_db else None
        bco = s.out(3 * C)
        s.call(BWD_FIN_SUMS, [C, acc], [bl, bgl, bgam if with_gamma else None, bis, bdg, bdb, bco])
        runs.append((acc, with_gamma, bdg, bdb, bco))
    beta, rm, rv, cb = (torch.randn(C, generator=g), torch.randn(C, generator=g) * 3, torch.rand(C, generator=g) * 4,
                        torch.randn(C, generator=g))
    rv[::7] = 0.0                                            # invstd = 1 / sqrt(eps)
    folds = []
    for affine, bias in [(True, True), (True, False), (False, True), (False, False)]:
        bsc, bsh = s.out(C), s.out(C)
        s.call(FOLD_EVAL, [C], [s.vec(gamma) if affine else None, s.vec(beta) if affine else None, s.vec(rm), s.vec(rv),
                                s.vec(cb) if bias else None, bsc, bsh], [R.BN_EPS])
        folds.append((affine, bias, bsc, bsh))
    rcs = s.run()
    assert rcs == [0] * len(rcs), rcs
    # d-gamma / d-beta: the LOCAL sums rounded to fp32 (plus one fp32 add); coef: the GLOBAL means, one rounding each
    lq, ls = local[C:2 * C].float(), local[:C].float()
    for acc, with_gamma, bdg, bdb, bco in runs:
        if bdg is not None:
            assert torch.equal(s.get(bdg), dg0 + lq if acc else lq)
        if bdb is not None:
            assert torch.equal(s.get(bdb), db0 + ls if acc else ls)
        coef = s.get(bco).view(3, C)
        assert torch.equal(coef[0], gamma * invstd if with_gamma else invstd)
        assert torch.equal(coef[1], (glob[:C] / 12000.0).float()) and torch.equal(coef[2], (glob[C:2 * C] / 12000.0).float())
    for affine, bias, bsc, bsh in folds:
        scale, b_sc, shift, b_sh = R.fold_eval64(gamma if affine else None, beta if affine else None, rm, rv, cb if bias else None)
        got_sc, got_sh = s.get(bsc), s.get(bsh)
        E.assert_written(got_sc, "scale")
        E.assert_written(got_sh, "shift")
        E.assert_bound(got_sc, scale, b_sc, f"fold_eval scale affine={affine}")
        E.assert_bound(got_sh, shift, b_sh, f"fold_eval shift affine={affine} bias={bias}")


# ------------------------------------------------------------------------------------------------ apply
APPLY_VARIANTS = [(a, False) for a in ACT_LIST] + [(R.ACT_NONE, True), (R.ACT_RELU, True)]


@pytest.mark.parametrize("small,C,P", [(False, 8, 300), (False, 8, 100), (False, 24, 300), (False, 24, 100), (False, 1032, 5),
                                       (True, 8, 1000), (True, 24, 300), (True, 24, 1)])
def test_bn_apply_every_activation(emus, small, C, P):
    """Default blocking: the launch's threads cover 128 pixels at once; at P = 300 the third unrolled slot is live for 44 lanes and
    clamps for the others, at P = 100 some lanes of a workgroup have no pixel at all, and at C = 1032 (129 blocks) only five
    lanes in 33024 have one.  SMALL: 3 blocks and an unroll of 2, so that lanes take one or two trips of the grid-stride loop
    (C = 8: 768 pixels a trip, P = 1000; C = 24: 256 a trip, P = 300).  mask_bits, exactly P * CQ / 2 bytes, goes with every ReLU."""
    s = emus(small)
    ycs, rcs_, ocs = C + 8, C + 4, C + 12
    y, r, sc, sh = R.apply_case(P, C, seed=C + P)
    by, br, bsc, bsh = s.sin(y, ycs, 4), s.sin(r, rcs_, 8), s.vec(sc), s.vec(sh)
    runs = []
    for act, res in APPLY_VARIANTS:
        bo = s.sout(P, C, ocs, 4)
        bm = s.out(P * C // 8, np.uint8) if act == R.ACT_RELU else None
        s.call(APPLY, [ycs, rcs_ if res else 0, act, ocs, P, C], [by, bsc, bsh, br if res else None, bo, bm])
        runs.append((act, res, bo, bm))
    # off-grid values: the fma rounds once and the residual add once -- 2 EPS of the terms
    g = R.gen(P)
    yr, rr, scr, shr = (torch.randn(P, C, generator=g) * 3, torch.randn(P, C, generator=g), torch.randn(C, generator=g),
                        torch.randn(C, generator=g))
    byr, brr, bor = s.sin(yr, ycs, 4), s.sin(rr, rcs_, 8), s.sout(P, C, ocs, 4)
    s.call(APPLY, [ycs, rcs_, R.ACT_NONE, ocs, P, C], [byr, s.vec(scr), s.vec(shr), brr, bor, None])
    rcs = s.run()
    assert rcs == [0] * len(rcs), rcs
    z0 = y.double() * sc.double() + sh.double()
    for act, res, bo, bm in runs:
        z = z0 + r.double() if res else z0
        got, ref = s.get_slice(bo, P, C), R.ACTS[act](z)
        if act in (R.ACT_HARDSWISH, R.ACT_HARDSIGMOID):
            # z and z * clamp(z + 3, 0, 6) are exact on this grid; the division by 6 rounds once (4 EPS: room for a
            # reciprocal multiply)
            E.assert_bound(got, ref, 4 * R.EPS * ref.abs(), f"act {act}")
        else:
            assert torch.equal(got.double(), ref), f"act {act} residual {res}: must be exact on grid inputs"
        if bm is not None:
            assert torch.equal(s.get(bm, np.uint8), R.packbits(z > 0)), "mask_bits: bit p * C + c must be fma(y, sc, sh) + r > 0"
    t = yr.double() * scr.double()
    E.assert_bound(s.get_slice(bor, P, C), t + shr.double() + rr.double(), 2 * R.EPS * (t.abs() + shr.double().abs() +
                                                                                      rr.double().abs()), "random values")


# ------------------------------------------------------------------------------------------------ backward
def _bwd_variants(C, full):
    """(mask source, activation, g_res, training)"""
    src = [("out", R.ACT_RELU), ("ss", R.ACT_RELU), ("ss", R.ACT_RELU6), ("ss", R.ACT_HARDSWISH), ("ss", R.ACT_HARDSIGMOID),
           ("none", R.ACT_NONE)] + ([("bits", R.ACT_RELU)] if C % 8 == 0 else [])
    if full:
        return [(m, a, res, tr) for m, a in src for res in (0, 1) for tr in (0, 1)]
    if C < 1024:
        return [(m, a, i % 2, (i // 2 + 1) % 2) for i, (m, a) in enumerate(src)] + [("out", R.ACT_RELU, 0, 0)]
    # bn_bwd_apply launches C / 4 blocks here: every mask source once, in seconds
    big = [("out", R.ACT_RELU, 1, 1), ("ss", R.ACT_HARDSWISH, 0, 1), ("none", R.ACT_NONE, 1, 0), ("ss", R.ACT_RELU6, 0, 1)] + \
        ([("bits", R.ACT_RELU, 1, 1)] if C % 8 == 0 else [])
    return big if C < 2048 else big[:3]


@pytest.mark.parametrize("small,C,full", [(False, 12, True), (False, 24, True), (False, 1028, False), (False, 1032, False),
                                          (False, 2052, False), (True, 12, False), (True, 24, False)])
def test_bn_bwd_reduce_and_apply_vs_float64(emus, small, C, full):
    """P = one block of pixels and three.  C = 1028: a channel group of 256 quads, then a group of one quad on 256 pixel
    lanes; 2052: two full groups and that one; 12, 1028 and 2052 have an odd number of quads (no mask bits), 24 and 1032 (a
    last group of two quads) carry the mask_bits source.  SMALL: blocks of 32 pixels, an unroll of 2, and bn_bwd_apply
    grid-strides (3 blocks, 2 pixels a trip)."""
    s = emus(small)
    ppb = SMALL["BNB_PPB"] if small else 512
    P = 515                                                 # SMALL: 17 blocks, and past bn_bwd_apply's 512 (256) pixels a trip
    nblk = -(-P // ppb)
    gcs, ycs, ocs, gycs, grcs = C + 4, C + 8, C + 12, C + 16, C + 20
    y, _, sc, sh = R.apply_case(P, C, seed=C)               # z = fma(y, scale, shift) exact: the float64 masks are the kernel's
    ss = torch.stack([sc, sh])
    z = y.double() * sc.double() + sh.double()
    gen = R.gen(C + 1)
    g = torch.randn(P, C, generator=gen)
    mean, invstd = torch.randn(C, generator=gen), torch.rand(C, generator=gen) + 0.5
    gamma = torch.randn(C, generator=gen)
    coef = torch.randn(3, C, generator=gen)
    bg, by, bo = s.sin(g, gcs, 4), s.sin(y, ycs, 8), s.sin(torch.relu(z).float(), ocs, 4)
    bss, bmu, bis, bgam, bco = s.vec(ss), s.vec(mean), s.vec(invstd), s.vec(gamma), s.vec(coef)
    bbits = s.vec(R.packbits(z > 0), np.uint8) if C % 8 == 0 else None
    c_n = s.call(BWD_NBLK, [P, C])
    runs = []
    for src, act, res, tr in _bwd_variants(C, full):
        m_out, m_ss, m_bits = (bo if src == "out" else None), (bss if src == "ss" else None), (bbits if src == "bits" else None)
        bpart, bdg, bdb, bc2 = s.out(nblk * 2 * C), s.out(C), s.out(C), s.out(3 * C)
        if tr:
            s.call(BWD_REDUCE, [gcs, ocs, act, ycs, P, C], [bg, m_out, by, bmu, bis, bpart, m_ss, m_bits])
            s.call(BWD_FIN, [nblk, C, 0], [bpart, bgam, bis, bdg, bdb, bc2], [float(P)])
        bgy, bgr = s.sout(P, C, gycs, 4), (s.sout(P, C, grcs, 8) if res else None)
        need_y = tr or src == "ss"
        s.call(BWD_APPLY, [gcs, ocs, act, ycs, tr, gycs, grcs if res else 0, P, C],
               [bg, m_out, by if need_y else None, bmu if tr else None, bis if tr else None, bco if tr else s.vec(coef[:1]), bgy,
                bgr, m_ss, m_bits])
        runs.append((src, act, res, tr, bpart, bdg, bdb, bc2, bgy, bgr))
    rcs = s.run()
    assert rcs[c_n] == nblk and rcs[:c_n] + rcs[c_n + 1:] == [0] * (len(rcs) - 1), rcs
    for src, act, res, tr, bpart, bdg, bdb, bc2, bgy, bgr in runs:
        tag = f"C={C} mask source {src} act {act} g_res {res} training {tr}"
        gp, ka = R.act_bwd64(act, z, g.double())
        if tr:
            part = s.get(bpart).view(nblk, 2, C)
            E.assert_written(part, tag + " partial rows")
            db, e_db, dg, e_dg = R.bwd_reduce64(gp, ka, y, mean, invstd, P, ppb, host=1)
            E.assert_bound(part[:, 0].double().sum(0), db, e_db, tag + " sum g'")
            E.assert_bound(part[:, 1].double().sum(0), dg, e_dg, tag + " sum g' xhat")
            # the finalize of those rows: their float64 sums rounded once
            E.assert_bound(s.get(bdb), db, e_db + R.EPS * (db.abs() + e_db), tag + " d-beta")
            E.assert_bound(s.get(bdg), dg, e_dg + R.EPS * (dg.abs() + e_dg), tag + " d-gamma")
            c2 = s.get(bc2).view(3, C)
            assert torch.equal(c2[0], gamma * invstd)
            E.assert_bound(c2[1], db / P, (e_db + R.EPS * (db.abs() + e_db)) / P, tag + " mean g'")
        ref, bound = R.bwd_apply64(gp, ka, y, mean, invstd, coef, tr)
        E.assert_bound(s.get_slice(bgy, P, C), ref, bound, tag + " g_y")
        if res:
            got = s.get_slice(bgr, P, C)
            if float(ka.max()) == 0:
                assert torch.equal(got.double(), gp), tag + ": g_res must be the masked g exactly"
            else:
                E.assert_bound(got, gp, ka, tag + " g_res")


def test_argument_rejections_write_nothing(emus):
    s = emus()
    P, C = 6, 8
    x = torch.randn(P, C)
    bx, bv, bss, bco = s.sin(x), s.vec(torch.randn(C)), s.vec(torch.randn(2, C)), s.vec(torch.randn(3, C))
    bo, bm, bpart, bdv, bsums = s.sout(P, C), s.out(P * C // 8, np.uint8), s.out(2 * C), s.out(3 * C), s.out(2 * C + 1, np.float64)
    bits, part_in, sums_in = s.vec(torch.zeros(P * C // 8), np.uint8), s.vec(torch.randn(1, 2, C)), s.vec(torch.rand(2 * C + 1), np.float64)
    fin = [part_in, None, None, None, None, bdv, bdv, None, None, None]

    def apply(C=C, P=P, ycs=C, ocs=C, rcs=0, act=0, b=(bx, bv, bv, None, bo, None)):
        return s.call(APPLY, [ycs, rcs, act, ocs, P, C], b)

    def reduce(C=C, P=P, act=R.ACT_RELU, b=(bx, bx, bx, bv, bv, bpart, None, None)):
        return s.call(BWD_REDUCE, [C, C, act, C, P, C], b)

    def bapply(C=C, P=P, act=R.ACT_RELU, tr=1, b=(bx, bx, bx, bv, bv, bco, bo, None, None, None)):
        return s.call(BWD_APPLY, [C, C, act, C, tr, C, 0, P, C], b)

    bad = [apply(C=6), apply(C=0), apply(P=0), apply(ycs=10), apply(ocs=10), apply(rcs=6), apply(act=2), apply(act=3),
           apply(b=(bx, bv, bv, None, bo, bm)), apply(C=12, act=R.ACT_RELU, b=(bx, bv, bv, None, bo, bm)),
           apply(b=(bx, None, bv, None, bo, None)), apply(b=(bx, bv, bv, None, None, None)),
           reduce(C=6), reduce(C=4100), reduce(P=0), reduce(b=(bx, None, bx, bv, bv, bpart, None, None)),
           reduce(act=R.ACT_RELU6), reduce(act=2), reduce(act=R.ACT_NONE, b=(bx, None, bx, bv, bv, bpart, None, bits)),
           reduce(C=12, b=(bx, None, bx, bv, bv, bpart, None, bits)), reduce(b=(bx, bx, bx, bv, bv, None, None, None)),
           bapply(C=6), bapply(P=0), bapply(b=(bx, bx, None, bv, bv, bco, bo, None, None, None)),
           bapply(b=(bx, bx, bx, None, bv, bco, bo, None, None, None)), bapply(tr=0, b=(bx, None, bx, None, None, bco, bo, None, None, None)),
           bapply(act=R.ACT_NONE, b=(bx, None, bx, bv, bv, bco, bo, None, bss, None)), bapply(act=R.ACT_HARDSWISH),
           bapply(tr=0, b=(bx, None, None, None, None, bco, bo, None, bss, None)),
           bapply(C=12, b=(bx, None, bx, bv, bv, bco, bo, None, None, bits)), bapply(b=(bx, bx, bx, bv, bv, bco, None, None, None, None)),
           s.call(FINALIZE, [0, C, C], fin, [6.0, R.BN_EPS, R.MOM]), s.call(FINALIZE, [1, 4, C], fin, [6.0, R.BN_EPS, R.MOM]),
           s.call(FINALIZE, [1, C, C], fin, [0.0, R.BN_EPS, R.MOM]), s.call(FINALIZE, [1, C, 0], fin, [6.0, R.BN_EPS, R.MOM]),
           s.call(PSUMS, [0, C, C], [part_in, bsums], [6.0]), s.call(PSUMS, [1, 4, C], [part_in, bsums], [6.0]),
           s.call(PSUMS, [1, C, C], [part_in, bsums], [-1.0]), s.call(PSUMS, [1, C, C], [part_in, None], [6.0]),
           s.call(FIN_SUMS, [0], [sums_in] + fin[1:], [R.BN_EPS, R.MOM]), s.call(FIN_SUMS, [C], [None] + fin[1:], [R.BN_EPS, R.MOM]),
           s.call(BWD_FIN_SUMS, [0, 0], [sums_in, sums_in, None, bv, None, None, bdv]),
           s.call(BWD_FIN_SUMS, [C, 0], [sums_in, sums_in, None, None, None, None, bdv]),
           s.call(FOLD_EVAL, [0], [None, None, bv, bv, None, bdv, bdv], [R.BN_EPS]),
           s.call(FOLD_EVAL, [C], [None, None, None, bv, None, bdv, bdv], [R.BN_EPS]),
           s.call(BWD_FIN, [0, C, 0], [part_in, None, bv, None, None, bdv], [6.0]),
           s.call(BWD_FIN, [1, C, 0], [part_in, None, bv, None, None, bdv], [0.0]),
           s.call(BWD_FIN, [1, C, 0], [part_in, None, None, None, None, bdv], [6.0]),
           s.call(BWD_FIN_C, [1, 4, C, 0], [part_in, None, bv, None, None, bdv], [6.0]),
           s.call(BWD_FIN_C, [1, C, C, 0], [part_in, None, bv, None, None, None], [6.0])]
    rcs = s.run()
    assert [rcs[i] for i in bad] == [E.ADH_E_ARG] * len(bad), rcs
    for b in (bo, bm, bpart, bdv, bsums):
        assert s.unchanged(b), "a rejected call wrote to an output"
