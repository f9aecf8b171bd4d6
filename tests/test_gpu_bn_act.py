"""The BatchNorm streaming kernels of csrc/bn_act.hip through the C ABI, each against a float64 torch restatement of the same
operation, at the edges the ConvBlock / ResidualBlock fixtures never reach: the unrolled fp64 loops of the finalize kernels
and their tails, the null-affine / null-running-statistics forms, count = 1 and 2, the sync-BN (all-reduced sums) forms, odd
numbers of channel quads, bn_bwd_reduce's loop over groups of 1024 channels with a ragged last group, the ReLU mask-bit
layout, channel-slice strides of every tensor argument, and the grid-stride loops past their block caps.

Every output buffer is prefilled with NaN: a kernel must write every element it owns, and everything outside the channel
slice it owns must still be NaN afterwards.  Every kernel runs twice (running statistics and num_batches_tracked reset in
between) and must reproduce itself bit for bit.  Tolerances are in units of EPS = 2^-24, the fp32 unit roundoff, and each
comment says which fp32 operations bound it.

The frozen-statistics tests at the end run Engine.conv with module.eval() semantics and trainable gamma / beta (the
classifier of the joint step) against float64 F.batch_norm(training=False)."""
import pytest
import torch
import torch.nn.functional as F

from adam_dehaze_amd import _hip as H
from adam_dehaze_amd.engine import Act, BNState, Engine

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS = 2.0 ** -24
BN_EPS = float(torch.tensor(1e-5, dtype=torch.float32))       # the fp32 values the kernels receive
MOM = float(torch.tensor(0.1, dtype=torch.float32))
NAN = float("nan")


def _nan(*shape, dtype=torch.float32):
    return torch.full(shape, NAN, device=DEV, dtype=dtype)


def _gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def _randn(*shape, seed=0, dtype=torch.float32):
    return torch.randn(shape, device=DEV, dtype=dtype, generator=_gen(seed))


def _rand(*shape, seed=0, dtype=torch.float32):
    return torch.rand(shape, device=DEV, dtype=dtype, generator=_gen(seed))


def _grid(shape, lo, hi, den, seed):
    """integers in [lo, hi] / den as fp32: sums and products of a few of them are exact in fp32 and float64."""
    return torch.randint(lo, hi + 1, shape, device=DEV, generator=_gen(seed)).float() / den


def _same_bits(u, v):
    if u.is_floating_point():
        it = torch.int32 if u.dtype == torch.float32 else torch.int64
        u, v = u.view(it), v.view(it)       # bit patterns: NaN == NaN, -0 != +0
    return torch.equal(u, v)


def _twice(fn):
    """Run `fn` (which returns a tuple of fresh tensors or None) twice; the runs must agree bit for bit."""
    a = fn()
    b = fn()
    torch.cuda.synchronize()
    for i, (u, v) in enumerate(zip(a, b)):
        if u is not None:
            assert _same_bits(u, v), f"output {i} differs between two identical runs"
    return a


def _ulp(ref64):
    """the fp32 spacing at ref (the ulp of ref rounded to fp32)."""
    _, e = torch.frexp(ref64.float())
    return torch.ldexp(torch.ones_like(ref64), (e.to(torch.int64) - 24).clamp_min(-149))


def _assert_ulps(got, ref64, n, what):
    assert not torch.isnan(got).any(), f"{what}: NaN (an element was not written)"
    err = (got.double() - ref64).abs()
    assert float((err - n * _ulp(ref64)).max()) <= 0, f"{what}: {float((err / _ulp(ref64)).max()):.2f} ulp"


def _assert_bound(got, ref64, bound, what):
    """|got - ref| <= bound elementwise; a NaN in got fails."""
    assert not torch.isnan(got).any(), f"{what}: NaN (an element was not written)"
    d = (got.double() - ref64).abs() - bound
    assert float(d.max()) <= 0, f"{what}: exceeds its bound by {float(d.max()):.3e}"


# ------------------------------------------------------------------------------------------------ finalize
def _partials(nblk, C, NcP, count, seed):
    """fp32 per-block (sum y, sum y^2) of a virtual batch of `count` elements split unevenly over nblk blocks.  Block means
    scatter around a per-channel mean of up to ~3 sigma, so Q / n - mean^2 >= sigma^2 > 0 (Jensen); channel 2 has
    Q / n < mean^2 (the clamp to a zero variance).  The padding columns [C, NcP) are NaN: the kernels must not read them."""
    g = _gen(seed)
    mu = torch.randn(1, C, device=DEV, dtype=torch.float64, generator=g) * 2
    sig2 = torch.rand(1, C, device=DEV, dtype=torch.float64, generator=g) * 4 + 0.25
    m_b = mu + 0.25 * torch.randn(nblk, C, device=DEV, dtype=torch.float64, generator=g)
    w = torch.rand(nblk, 1, device=DEV, dtype=torch.float64, generator=g) + 0.5
    w = w / w.sum() * count
    part = _nan(nblk, 2, NcP)
    part[:, 0, :C] = (w * m_b).float()
    part[:, 1, :C] = (w * (sig2 + m_b * m_b)).float()
    if C > 2:
        part[:, 0, 2] = (w[:, 0] * 1.5).float()
        part[:, 1, 2] = (w[:, 0] * 2.25 * 0.999).float()
    return part


def _finalize_ref(part, C, count, gamma, beta, rm, rv):
    S = part[:, 0, :C].double().sum(0)
    Q = part[:, 1, :C].double().sum(0)
    mean = S / count
    var = (Q / count - mean * mean).clamp_min(0)
    invstd = 1.0 / torch.sqrt(var + BN_EPS)
    gm = gamma.double() if gamma is not None else torch.ones_like(mean)
    bt = beta.double() if beta is not None else torch.zeros_like(mean)
    unb = var * count / (count - 1) if count > 1 else var     # BatchNorm2d's unbiased running estimate; none at n = 1
    out = {"scale": gm * invstd, "shift": bt - mean * gm * invstd, "mean": mean, "invstd": invstd}
    if rm is not None:
        # (1 - m) r + m v: the roundings of fp32(v), of (1 - m), of both products and of the sum -- 4 EPS of the terms
        out["rm"] = ((1 - MOM) * rm.double() + MOM * mean, 4 * EPS * ((1 - MOM) * rm.double().abs() + MOM * mean.abs()))
        out["rv"] = ((1 - MOM) * rv.double() + MOM * unb, 4 * EPS * ((1 - MOM) * rv.double().abs() + MOM * unb.abs()))
    return out


FIN_VARIANTS = [
    # affine, running statistics, count
    (True, True, 4.2e6),
    (False, False, 1.0),
    (True, True, 2.0),
    (False, True, 1.0),
    (True, False, 2.0),
    (False, True, 2.0),
]


def _run_finalize(part, nblk, NcP, C, count, gamma, beta, rm0, rv0, with_save=True):
    def run():
        rm = rm0.clone() if rm0 is not None else None        # reset between the two runs
        rv = rv0.clone() if rv0 is not None else None
        nbt = torch.full((), 5, device=DEV, dtype=torch.int64)
        sc, sh, sm, si = _nan(C + 3), _nan(C + 3), _nan(C + 3), _nan(C + 3)
        H.call("adh_bn_finalize", part.data_ptr(), nblk, NcP, C, count, H.ptr(gamma), H.ptr(beta), BN_EPS, MOM, H.ptr(rm),
               H.ptr(rv), sc.data_ptr(), sh.data_ptr(), sm.data_ptr() if with_save else None,
               si.data_ptr() if with_save else None, nbt.data_ptr())
        return sc, sh, sm, si, rm, rv, nbt
    return _twice(run)


@pytest.mark.parametrize("C", [1, 4, 31, 33, 96, 2048])
@pytest.mark.parametrize("nblk", [1, 31, 32, 33, 127, 128, 129, 1000])
def test_bn_finalize_vs_float64(nblk, C):
    NcP = (C + 31) // 32 * 32
    for vi, (affine, running, count) in enumerate(FIN_VARIANTS):
        part = _partials(nblk, C, NcP, count, seed=nblk * 7 + C + vi)
        gamma = _randn(C, seed=C + vi) if affine else None
        beta = _randn(C, seed=C + vi + 100) if affine else None
        rm0 = _randn(C, seed=C + 3) if running else None
        rv0 = _rand(C, seed=C + 4) + 0.5 if running else None
        sc, sh, sm, si, rm, rv, nbt = _run_finalize(part, nblk, NcP, C, count, gamma, beta, rm0, rv0)
        ref = _finalize_ref(part, C, count, gamma, beta, rm0, rv0)
        tag = f"affine={affine} running={running} count={count}"
        # fp64 sums of the fp32 partials (in another order), one rounding to fp32 at the end: 1 ulp of the float64 value
        _assert_ulps(sc[:C], ref["scale"], 1, "scale " + tag)
        _assert_ulps(sh[:C], ref["shift"], 1, "shift " + tag)
        _assert_ulps(sm[:C], ref["mean"], 1, "save_mean " + tag)
        _assert_ulps(si[:C], ref["invstd"], 1, "save_invstd " + tag)
        for t in (sc, sh, sm, si):
            assert torch.isnan(t[C:]).all(), "written past C"
        if running:
            _assert_bound(rm, *ref["rm"], "running_mean " + tag)
            _assert_bound(rv, *ref["rv"], "running_var " + tag)
        assert int(nbt) == 6, "num_batches_tracked must go up by exactly 1 (one writer over all blocks)"


def test_bn_finalize_without_save_outputs():
    C, nblk = 96, 129
    part = _partials(nblk, C, 96, 4.2e6, seed=3)
    sc, sh, sm, si, _, _, nbt = _run_finalize(part, nblk, 96, C, 4.2e6, None, None, None, None, with_save=False)
    ref = _finalize_ref(part, C, 4.2e6, None, None, None, None)
    _assert_ulps(sc[:C], ref["scale"], 1, "scale")
    _assert_ulps(sh[:C], ref["shift"], 1, "shift")
    assert torch.isnan(sm).all() and torch.isnan(si).all()
    assert int(nbt) == 6


# ------------------------------------------------------------------------------------------------ sync-BN forms
SYNC_CASES = [(1, 4), (33, 96), (129, 33), (1000, 2048), (64, 1)]


def _partial_sums(part, nblk, pitch, C, count):
    sums = _nan(2 * C + 1, dtype=torch.float64)
    H.call("adh_bn_partial_sums", part.data_ptr(), nblk, pitch, C, count, sums.data_ptr())
    return sums


def _finalize_sums(sums, C, gamma, beta, rm0, rv0):
    rm, rv = rm0.clone(), rv0.clone()
    nbt = torch.full((), 5, device=DEV, dtype=torch.int64)
    sc, sh, sm, si = _nan(C), _nan(C), _nan(C), _nan(C)
    H.call("adh_bn_finalize_sums", sums.data_ptr(), C, H.ptr(gamma), H.ptr(beta), BN_EPS, MOM, rm.data_ptr(), rv.data_ptr(),
           sc.data_ptr(), sh.data_ptr(), sm.data_ptr(), si.data_ptr(), nbt.data_ptr())
    return sc, sh, sm, si, rm, rv, nbt


@pytest.mark.parametrize("nblk,C", SYNC_CASES)
def test_bn_sync_sums_match_single_process(nblk, C):
    NcP = (C + 31) // 32 * 32
    count = 4.2e6
    part = _partials(nblk, C, NcP, count, seed=nblk + C)
    gamma, beta = _randn(C, seed=1), _randn(C, seed=2)
    rm0, rv0 = _randn(C, seed=3), _rand(C, seed=4) + 0.5

    (sums,) = _twice(lambda: (_partial_sums(part, nblk, NcP, C, count),))
    S = part[:, 0, :C].double()
    Q = part[:, 1, :C].double()
    # fp64 sums of fp32 values in another order: 1e-13 of the sum of |terms|
    _assert_bound(sums[:C], S.sum(0), 1e-13 * S.abs().sum(0), "sum y")
    _assert_bound(sums[C:2 * C], Q.sum(0), 1e-13 * Q.abs().sum(0), "sum y^2")
    assert float(sums[2 * C]) == count, "sums[2C] must carry the element count exactly"

    got = _twice(lambda: _finalize_sums(sums, C, gamma, beta, rm0, rv0))
    want = _run_finalize(part, nblk, NcP, C, count, gamma, beta, rm0, rv0)
    # the two forms round the same fp64 values (summed in different orders) to fp32 once
    for name, a, b in zip(("scale", "shift", "save_mean", "save_invstd"), got[:4], want[:4]):
        _assert_ulps(a, b[:C].double(), 1, name)
    for name, a, b in zip(("running_mean", "running_var"), got[4:6], want[4:6]):
        _assert_bound(a, b.double(), 4 * EPS * b.double().abs(), name)
    assert int(got[6]) == 6

    # data parallel: the all-reduce (the sum of the two ranks' vectors) then finalize == finalizing every partial at once
    if nblk >= 2:
        k = nblk // 2
        sa = _partial_sums(part[:k].contiguous(), k, NcP, C, count / 2)
        sb = _partial_sums(part[k:].contiguous(), nblk - k, NcP, C, count / 2)
        red = sa + sb
        assert float(red[2 * C]) == count
        ddp = _finalize_sums(red, C, gamma, beta, rm0, rv0)
        for name, a, b in zip(("scale", "shift", "save_mean", "save_invstd"), ddp[:4], got[:4]):
            _assert_ulps(a, b.double(), 1, "all-reduced " + name)


@pytest.mark.parametrize("C", [4, 96, 1000])
@pytest.mark.parametrize("accumulate", [0, 1])
def test_bn_bwd_finalize_sums(C, accumulate):
    local = _randn(2 * C + 1, seed=C, dtype=torch.float64) * 100
    glob = local + _randn(2 * C + 1, seed=C + 1, dtype=torch.float64) * 100
    local[2 * C] = 3000.0
    glob[2 * C] = 12000.0
    gamma, invstd = _randn(C, seed=2), _rand(C, seed=3) + 0.1
    dg0, db0 = _randn(C, seed=4), _randn(C, seed=5)

    def run():
        dg = dg0.clone() if accumulate else _nan(C)
        db = db0.clone() if accumulate else _nan(C)
        coef = _nan(3, C)
        H.call("adh_bn_bwd_finalize_sums", local.data_ptr(), glob.data_ptr(), C, gamma.data_ptr(), invstd.data_ptr(),
               dg.data_ptr(), db.data_ptr(), accumulate, coef.data_ptr())
        return dg, db, coef

    dg, db, coef = _twice(run)
    # d-gamma / d-beta: the LOCAL sums rounded to fp32 (plus one fp32 add); coef: the GLOBAL means, one rounding each
    lq, ls = local[C:2 * C].float(), local[:C].float()
    assert torch.equal(dg, dg0 + lq if accumulate else lq)
    assert torch.equal(db, db0 + ls if accumulate else ls)
    assert torch.equal(coef[0], gamma * invstd)
    assert torch.equal(coef[1], (glob[:C] / 12000.0).float())
    assert torch.equal(coef[2], (glob[C:2 * C] / 12000.0).float())


# ------------------------------------------------------------------------------------------------ fold_eval
@pytest.mark.parametrize("C", [1, 96, 1000])
@pytest.mark.parametrize("affine,bias", [(True, True), (True, False), (False, True), (False, False)])
def test_bn_fold_eval(C, affine, bias):
    gamma = _randn(C, seed=1) if affine else None
    beta = _randn(C, seed=2) if affine else None
    rm = _randn(C, seed=3) * 3
    rv = _rand(C, seed=4) * 4
    rv[::7] = 0.0                                            # invstd = 1 / sqrt(eps)
    cb = _randn(C, seed=5) if bias else None

    def run():
        sc, sh = _nan(C + 2), _nan(C + 2)
        H.call("adh_bn_fold_eval", C, H.ptr(gamma), H.ptr(beta), rm.data_ptr(), rv.data_ptr(), BN_EPS, H.ptr(cb),
               sc.data_ptr(), sh.data_ptr())
        return sc, sh

    sc, sh = _twice(run)
    invstd = 1 / torch.sqrt(rv.double() + BN_EPS)
    scale = invstd * gamma.double() if affine else invstd
    shift = -rm.double() * scale
    terms = shift.abs()
    if affine:
        shift = shift + beta.double()
        terms = terms + beta.double().abs()
    if bias:
        shift = shift + cb.double() * scale
        terms = terms + (cb.double() * scale).abs()
    # rv + eps, sqrtf, the reciprocal, the gamma product: 8 EPS of the scale (room for approximate sqrt / rcp); the shift
    # adds two products of that scale and two sums
    _assert_bound(sc[:C], scale, 8 * EPS * scale.abs(), "scale")
    _assert_bound(sh[:C], shift, 12 * EPS * terms, "shift")
    assert torch.isnan(sc[C:]).all() and torch.isnan(sh[C:]).all()


# ------------------------------------------------------------------------------------------------ apply
ACTS = {H.ACT_NONE: lambda z: z, H.ACT_RELU: F.relu, H.ACT_RELU6: F.relu6, H.ACT_HARDSWISH: F.hardswish,
        H.ACT_HARDSIGMOID: F.hardsigmoid}
APPLY_C = [4, 12, 20, 48, 96, 384, 960, 1280, 2048]


def _packbits(m):
    """[P, C] bool -> bytes holding bit p * C + c of the flat array (LSB first): adh_bn_apply's nibble layout, byte
    (p * CQ + cq) / 2 holding quad cq's four channels in nibble cq % 2."""
    b = m.reshape(-1, 8).to(torch.int32) << torch.arange(8, device=m.device, dtype=torch.int32)
    return b.sum(1).to(torch.uint8)


def _run_apply(yb, ys, sc, sh, rb, rs, act, P, C, out_cs, mask):
    def run():
        ob = _nan(P, out_cs)
        mb = torch.full(((P * C + 7) // 8,), 0x5A, device=DEV, dtype=torch.uint8) if mask else None
        H.call("adh_bn_apply", yb.data_ptr(), ys, sc.data_ptr(), sh.data_ptr(), H.ptr(rb), rs if rb is not None else 0, act,
               ob.data_ptr(), out_cs, P, C, H.ptr(mb))
        return ob, mb
    return _twice(run)


@pytest.mark.parametrize("C", APPLY_C)
def test_bn_apply_every_activation_exact(C):
    """Grid inputs: y in [-3, 3] step 1/8, scale in [-2, 2] step 1/4 (0 included), shift and residual in [-2, 2] step 1/8.
    z = fma(y, scale, shift) (+ r) is then exact in fp32, and lands on 0, +-3 and 6 often: every activation's kinks.
    y, the residual and out are channel slices of wider buffers (y_cs, res_cs, out_cs > C).  C = 12 and 20 have an odd
    number of quads; 960 and 1280 have gcd(CQ, 256) < CQ (the grid is a multiple of CQ / gcd blocks)."""
    P = 3 * 37 * 53
    ys, rs, out_cs = C + 8, C + 4, C + 12
    yb = _grid((P, ys), -24, 24, 8, C)
    rb = _grid((P, rs), -16, 16, 8, C + 1)
    sc = _grid((C,), -8, 8, 4, C + 2)
    sh = _grid((C,), -16, 16, 8, C + 3)
    z0 = yb[:, :C].double() * sc.double() + sh.double()
    for act, res in [(a, False) for a in ACTS] + [(H.ACT_NONE, True), (H.ACT_RELU, True)]:
        z = z0 + rb[:, :C].double() if res else z0
        mask = act == H.ACT_RELU and C % 8 == 0
        ob, mb = _run_apply(yb, ys, sc, sh, rb if res else None, rs, act, P, C, out_cs, mask)
        ref = ACTS[act](z)
        if act in (H.ACT_HARDSWISH, H.ACT_HARDSIGMOID):
            # z and z * clamp(z + 3, 0, 6) are exact on this grid; the division by 6 rounds once (4 EPS: room for a
            # reciprocal multiply)
            _assert_bound(ob[:, :C], ref, 4 * EPS * ref.abs(), f"act {act}")
        else:
            assert torch.equal(ob[:, :C].double(), ref), f"act {act} residual {res}: must be exact on grid inputs"
        assert torch.isnan(ob[:, C:]).all(), "written outside its channel slice"
        if mask:
            assert torch.equal(mb, _packbits(z > 0)), "mask_bits: bit p * C + c must be fma(y, sc, sh) + r > 0"


def test_bn_apply_random_values_vs_float64():
    # off-grid values: the fma rounds once and the residual add once -- 2 EPS of the terms
    P, C = 5003, 96
    yb = _randn(P, C + 8, seed=1) * 3
    rb = _randn(P, C + 4, seed=2)
    sc, sh = _randn(C, seed=3), _randn(C, seed=4)
    for res in (False, True):
        ob, _ = _run_apply(yb, C + 8, sc, sh, rb if res else None, C + 4, H.ACT_NONE, P, C, C + 12, False)
        t = yb[:, :C].double() * sc.double()
        z = t + sh.double()
        terms = t.abs() + sh.double().abs()
        if res:
            z = z + rb[:, :C].double()
            terms = terms + rb[:, :C].double().abs()
        _assert_bound(ob[:, :C], z, 2 * EPS * terms, f"residual {res}")


@pytest.mark.parametrize("C,act", [(12, H.ACT_RELU), (20, H.ACT_RELU), (4, H.ACT_RELU), (96, H.ACT_NONE),
                                   (96, H.ACT_RELU6), (96, H.ACT_HARDSWISH)])
def test_bn_apply_mask_bits_rejects_odd_quads_and_other_activations(C, act):
    P = 64
    y, sc, sh, out = _randn(P, C, seed=1), _randn(C, seed=2), _randn(C, seed=3), _nan(P, C)
    mb = torch.zeros(P * C // 8 + 1, device=DEV, dtype=torch.uint8)
    with pytest.raises(RuntimeError):
        H.call("adh_bn_apply", y.data_ptr(), C, sc.data_ptr(), sh.data_ptr(), None, 0, act, out.data_ptr(), C, P, C,
               mb.data_ptr())
    torch.cuda.synchronize()
    assert torch.isnan(out).all(), "a rejected call must not launch"


def test_bn_apply_past_the_grid_cap():
    """C = 4 (one quad per pixel), P = 2^28 + 5: past EW_MAXBLK_APPLY x 256 threads x EW_UNROLL = 2^28 quads, so the
    grid-stride loop takes a second trip (4.3 GB per tensor).  Grid inputs make the result exact, checked in chunks after
    each of the two runs."""
    C, P = 4, (1 << 28) + 5
    sc = torch.tensor([0.5, -1.25, 2.0, 0.0], device=DEV)
    sh = torch.tensor([0.125, 1.0, -0.5, 0.75], device=DEV)
    y = torch.empty(P, C, device=DEV)
    CH = 1 << 24
    for p0 in range(0, P, CH):
        p1 = min(P, p0 + CH)
        i = torch.arange(p0 * C, p1 * C, device=DEV, dtype=torch.int64)
        y[p0:p1] = (((i * 7919) % 49) - 24).float().view(-1, C) / 8
        del i
    out = torch.empty(P, C, device=DEV)
    for run in range(2):
        out.fill_(NAN)
        H.call("adh_bn_apply", y.data_ptr(), C, sc.data_ptr(), sh.data_ptr(), None, 0, H.ACT_RELU, out.data_ptr(), C, P, C,
               None)
        torch.cuda.synchronize()
        for p0 in range(0, P, CH):
            p1 = min(P, p0 + CH)
            ref = torch.relu(y[p0:p1].double() * sc.double() + sh.double())
            assert torch.equal(out[p0:p1].double(), ref), f"run {run}, pixels [{p0}, {p1})"
            del ref
    del y, out
    torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------ backward
BWD_C = [4, 12, 96, 1024, 1028, 2048, 4096]
BWD_P = [1, 511, 512, 513]


class _Bwd:
    """One forward (adh_bn_apply) and everything the backward passes read; every tensor is a channel slice of a wider
    buffer (g_cs, y_cs, out_cs, gy_cs, gres_cs, res_cs all > C)."""

    def __init__(self, P, C, act, residual, seed):
        self.P, self.C, self.act = P, C, act
        self.gcs, self.ycs, self.ocs, self.gycs, self.grcs, self.rcs = C + 4, C + 8, C + 12, C + 16, C + 20, C + 24
        mu = torch.cat([_randn(C, seed=seed) * 2, torch.zeros(8, device=DEV)])
        self.gb = _randn(P, self.gcs, seed=seed + 1)
        self.yb = _randn(P, self.ycs, seed=seed + 2) * (_rand(self.ycs, seed=seed + 3) + 0.5) + mu
        self.rb = _randn(P, self.rcs, seed=seed + 4) if residual else None
        y = self.yb[:, :C].double()
        self.mean = y.mean(0).float()
        self.invstd = (1 / torch.sqrt(((y - y.mean(0)) ** 2).mean(0) + BN_EPS)).float()
        self.gamma = _randn(C, seed=seed + 5)
        self.gamma[::5] = 0.0
        beta = _randn(C, seed=seed + 6)
        self.ss = torch.empty(2, C, device=DEV)
        self.ss[0] = self.gamma * self.invstd
        self.ss[1] = beta - self.mean * self.ss[0]
        self.ob = _nan(P, self.ocs)
        self.mb = None
        if act == H.ACT_RELU and C % 8 == 0:
            self.mb = torch.empty((P * C + 7) // 8, device=DEV, dtype=torch.uint8)
        H.call("adh_bn_apply", self.yb.data_ptr(), self.ycs, self.ss[0].data_ptr(), self.ss[1].data_ptr(), H.ptr(self.rb),
               self.rcs if residual else 0, act, self.ob.data_ptr(), self.ocs, P, C, H.ptr(self.mb))
        self.nblk = H.value("adh_bn_bwd_num_blocks", P, C)

    def sources(self):
        """the ReLU mask sources the kernels accept for this forward"""
        if self.act != H.ACT_RELU:
            return ["none"]
        s = ["out"]
        if self.rb is None:
            s.append("ss")
        if self.mb is not None:
            s.append("bits")
        return s

    def run(self, src, training, accumulate=False, dg0=None, db0=None):
        P, C = self.P, self.C
        out = self.ob.data_ptr() if src == "out" else None
        mss = self.ss.data_ptr() if src == "ss" else None
        mbits = self.mb.data_ptr() if src == "bits" else None
        g_res = _nan(P, self.grcs) if self.rb is not None else None
        g_y = _nan(P, self.gycs)
        dg = db = None
        if training:
            part = _nan(self.nblk, 2, C)
            H.call("adh_bn_bwd_reduce", self.gb.data_ptr(), self.gcs, out, self.ocs, self.act, self.yb.data_ptr(), self.ycs,
                   self.mean.data_ptr(), self.invstd.data_ptr(), part.data_ptr(), P, C, mss, mbits)
            dg = dg0.clone() if accumulate else _nan(C)
            db = db0.clone() if accumulate else _nan(C)
            coef = _nan(3, C)
            H.call("adh_bn_bwd_finalize", part.data_ptr(), self.nblk, C, float(P), self.gamma.data_ptr(),
                   self.invstd.data_ptr(), dg.data_ptr(), db.data_ptr(), int(accumulate), coef.data_ptr())
        else:
            coef = torch.zeros(3, C, device=DEV)
            coef[0] = self.ss[0]
        H.call("adh_bn_bwd_apply", self.gb.data_ptr(), self.gcs, out, self.ocs, self.act,
               self.yb.data_ptr() if (training or mss is not None) else None, self.ycs,
               self.mean.data_ptr() if training else None, self.invstd.data_ptr() if training else None, coef.data_ptr(),
               int(training), g_y.data_ptr(), self.gycs, H.ptr(g_res), self.grcs if g_res is not None else 0, P, C, mss, mbits)
        return dg, db, coef, g_y, g_res

    def reference(self):
        """float64: g' = act'(z) g with the forward's ReLU decisions, then BatchNorm's training-mode backward with xhat built
        from the fp32 mean / invstd the kernels receive (the batch statistics of y)."""
        C, P = self.C, self.P
        g = self.gb[:, :C].double()
        if self.act == H.ACT_RELU:
            z = self.yb[:, :C].double() * self.ss[0].double() + self.ss[1].double()
            if self.rb is not None:
                z = z + self.rb[:, :C].double()
            m = self.ob[:, :C] > 0
            far = z.abs() > 1e-5 * (float(z.abs().max()) + 1)      # beyond rounding distance of the kink
            assert torch.equal(m[far], (z > 0)[far]), "forward ReLU mask"
            gp = torch.where(m, g, torch.zeros_like(g))
        else:
            gp = g
        xhat = (self.yb[:, :C].double() - self.mean.double()) * self.invstd.double()
        db = gp.sum(0)
        dg = (gp * xhat).sum(0)
        k0 = self.gamma.double() * self.invstd.double()
        mg, mgx = db / P, dg / P
        return gp, xhat, db, dg, k0 * (gp - mg - xhat * mgx), k0, mg, mgx


def _bwd_bounds(P, gp, xhat, k0, mg, mgx):
    """bn_bwd_reduce: per thread an fp32 chain over at most 512 / R pixels of a block, then R rows (R = 256 / quads in the
    channel group), fp64 over the blocks -- at most 513 + 2 roundings deep for any C, relative to the sum of |terms|
    (g' xhat adds the roundings of y - mean and two products).  bn_bwd_apply: y - mean, the products by
    kx = invstd * mgx and by k0 and the two differences -- 6 EPS of the terms, plus the means' own errors."""
    e_db = 516 * EPS * gp.abs().sum(0)
    e_dg = 520 * EPS * (gp * xhat).abs().sum(0)
    e_mg = e_db / P + EPS * mg.abs()
    e_mgx = e_dg / P + 2 * EPS * mgx.abs()
    e_gy = k0.abs() * (e_mg + xhat.abs() * e_mgx + 6 * EPS * (gp.abs() + mg.abs() + (xhat * mgx).abs()))
    return e_db, e_dg, e_mg, e_mgx, e_gy


def _check_bwd(P, C, act, residual, seed):
    b = _Bwd(P, C, act, residual, seed)
    gp, xhat, db_ref, dg_ref, gy_ref, k0, mg, mgx = b.reference()
    e_db, e_dg, e_mg, e_mgx, e_gy = _bwd_bounds(P, gp, xhat, k0, mg, mgx)
    first = None
    for src in b.sources():
        res = _twice(lambda: b.run(src, True))
        dg, db, coef, g_y, g_res = res
        _assert_bound(db, db_ref, e_db, f"d-beta ({src})")
        _assert_bound(dg, dg_ref, e_dg, f"d-gamma ({src})")
        assert torch.equal(coef[0], b.gamma * b.invstd), "coef[0] = gamma * invstd"
        _assert_bound(coef[1], mg, e_mg, f"mean g' ({src})")
        _assert_bound(coef[2], mgx, e_mgx, f"mean g' xhat ({src})")
        _assert_bound(g_y[:, :C], gy_ref, e_gy, f"g_y ({src})")
        assert torch.isnan(g_y[:, C:]).all(), "g_y written outside its channel slice"
        if residual:
            assert torch.equal(g_res[:, :C].double(), gp), f"g_res must be the masked g exactly ({src})"
            assert torch.isnan(g_res[:, C:]).all(), "g_res written outside its channel slice"
        if first is None:
            first = res
        else:
            for i, (u, v) in enumerate(zip(first, res)):
                if u is not None:
                    assert _same_bits(u, v), f"mask source {src}: output {i} differs from source {b.sources()[0]}"
        # eval (frozen statistics): g_y = coef[0] * g', one correctly rounded product
        _, _, _, gy_e, gres_e = _twice(lambda: b.run(src, False))
        assert torch.equal(gy_e[:, :C], b.ss[0] * gp.float()), f"eval g_y ({src})"
        assert torch.isnan(gy_e[:, C:]).all()
        if residual:
            assert torch.equal(gres_e[:, :C].double(), gp)
    # accumulate = 1: the finalize adds its fp32 results to what the buffers hold
    dg0, db0 = _randn(C, seed=seed + 50), _randn(C, seed=seed + 51)
    dga, dba, _, _, _ = b.run(b.sources()[0], True, accumulate=True, dg0=dg0, db0=db0)
    assert torch.equal(dga, dg0 + first[0]) and torch.equal(dba, db0 + first[1]), "accumulate=1"
    return b


@pytest.mark.parametrize("P", BWD_P)
@pytest.mark.parametrize("C", BWD_C)
def test_bn_bwd_relu_vs_float64(C, P):
    """C = 1024 .. 4096 run bn_bwd_reduce's channel-group loop one to four times; 1028 ends on a group of one quad.
    C = 12 and 1028 have an odd number of quads (no mask bits)."""
    _check_bwd(P, C, H.ACT_RELU, residual=False, seed=C + P)


@pytest.mark.parametrize("P", [511, 513])
@pytest.mark.parametrize("C", [12, 96, 1028, 2048])
def test_bn_bwd_residual_tail(C, P):
    # ResidualBlock tail act(BN(y) + r): the mask comes from `out` or the mask bits, the residual gets the masked g
    _check_bwd(P, C, H.ACT_RELU, residual=True, seed=C + P + 7)
    _check_bwd(P, C, H.ACT_NONE, residual=True, seed=C + P + 8)


def test_bn_bwd_past_the_grid_cap():
    """C = 24, P = 3 x 1031 x 1031: 19.1M quads, past EW_MAXBLK_BWD x 256 threads x EW_UNROLL = 2^24, so bn_bwd_apply's
    grid-stride loop takes a second trip (with 6 quads per pixel the grid is a multiple of 3 blocks)."""
    b = _check_bwd(3 * 1031 * 1031, 24, H.ACT_RELU, residual=True, seed=99)
    del b
    torch.cuda.empty_cache()


def test_bn_bwd_finalize_centered():
    """adh_bn_bwd_finalize_centered from test-built rows (sum g m, sum g m (y - mean)): d-gamma = invstd * row 1."""
    C, nblk, pitch = 96, 77, 128
    rows = _nan(nblk, 2, pitch)
    rows[:, :, :C] = _randn(nblk, 2, C, seed=1) * 10
    gamma, invstd = _randn(C, seed=2), _rand(C, seed=3) + 0.1
    count = 1e5

    def run():
        dg, db, coef = _nan(C), _nan(C), _nan(3, C)
        H.call("adh_bn_bwd_finalize_centered", rows.data_ptr(), nblk, pitch, C, count, gamma.data_ptr(), invstd.data_ptr(),
               dg.data_ptr(), db.data_ptr(), 0, coef.data_ptr())
        return dg, db, coef

    dg, db, coef = _twice(run)
    S = rows[:, 0, :C].double().sum(0)
    Q = rows[:, 1, :C].double().sum(0) * invstd.double()
    # fp64 sums and product, one rounding to fp32
    _assert_ulps(db, S, 1, "d-beta")
    _assert_ulps(dg, Q, 1, "d-gamma = invstd * row 1")
    assert torch.equal(coef[0], gamma * invstd)
    _assert_ulps(coef[1], S / count, 1, "mean g")
    _assert_ulps(coef[2], Q / count, 1, "mean g xhat")


# ------------------------------------------------------------------------------------------------ frozen statistics (engine)
FROZEN_CASES = [
    # k, Cin, Cout, relu, residual, conv bias
    (3, 16, 24, True, False, False),       # ConvBlock
    (3, 16, 24, True, True, False),        # ResidualBlock tail: relu(BN(conv) + r)
    (1, 32, 24, False, False, True),       # 1x1 conv + BN, no activation
    (3, 8, 16, False, True, True),         # residual add without an activation
]


@pytest.mark.parametrize("case", FROZEN_CASES, ids=lambda c: "k%d-%dto%d-relu%d-res%d-bias%d" % c)
def test_frozen_statistics_bn_backward_vs_float64(case):
    """Engine.conv(training=False) with trainable gamma / beta (module.eval() fine-tuning): d-gamma, d-beta, the data,
    residual and bias gradients against float64 F.batch_norm(training=False), the ReLU decisions replayed from the block
    output.  Channels take gamma in {0, 1e-3, 1} x beta in {-0.5, 0.5}: d-gamma = sum g' xhat needs xhat where gamma == 0
    (beta = 0.5 keeps the ReLU open there), and at gamma = 1e-3 xhat cannot be recovered from the block output to better
    than ~1e-4."""
    k, Cin, Cout, relu, residual, bias = case
    N, Hh, Ww = 2, 13, 17
    pad = k // 2
    x = _randn(N, Hh, Ww, Cin, seed=1)
    w = (_randn(Cout, Cin, k, k, seed=2) / (Cin * k * k) ** 0.5).requires_grad_(True)
    b = (_randn(Cout, seed=3) * 0.1).requires_grad_(True) if bias else None
    r = _randn(N, Hh, Ww, Cout, seed=4) * 0.5 if residual else None
    g = _randn(N, Hh, Ww, Cout, seed=5)
    gam = torch.tensor([0.0, 1e-3, 1.0], device=DEV).repeat(Cout)[:Cout].clone().requires_grad_(True)
    bet = torch.tensor([-0.5, 0.5], device=DEV).repeat_interleave(3).repeat(Cout)[:Cout].clone().requires_grad_(True)
    rm = _randn(Cout, seed=6) * 0.1
    rv = _rand(Cout, seed=7) + 0.5
    nbt = torch.zeros((), device=DEV, dtype=torch.int64)
    eng = Engine(torch.device(DEV), record=True)
    xa = Act(x.clone())
    ra = Act(r.clone()) if residual else None
    o = eng.conv(xa, w, b, BNState(gam, bet, rm, rv, nbt), kind="conv", k=k, stride=1, pad=pad, relu=relu, residual=ra,
                 training=False)
    assert o.t.shape[3] == Cout
    o.grad = g
    out = o.t.clone()
    eng.backward()
    torch.cuda.synchronize()
    assert int(nbt) == 0, "eval mode must not count batches"

    x64 = x.double().permute(0, 3, 1, 2).requires_grad_(True)
    w64 = w.detach().double().requires_grad_(True)
    b64 = b.detach().double().requires_grad_(True) if bias else None
    g64, be64 = gam.detach().double().requires_grad_(True), bet.detach().double().requires_grad_(True)
    y = F.conv2d(x64, w64, b64, 1, pad)
    z = F.batch_norm(y, rm.double(), rv.double(), g64, be64, training=False, eps=BN_EPS)
    r64 = None
    if residual:
        r64 = r.double().permute(0, 3, 1, 2).requires_grad_(True)
        z = z + r64
    mask = (out > 0).permute(0, 3, 1, 2).double() if relu else 1.0
    # the conv's fp32 accumulation (Cin k^2 products) dominates the forward: 2e-5 of the output's scale (a ReLU decision
    # that rounding flips moves the output by no more than that either)
    refr = torch.relu(z.detach()) if relu else z.detach()
    assert float((out.double() - refr.permute(0, 2, 3, 1)).abs().max()) <= 2e-5 * float(refr.abs().max()), "forward"
    (z * mask).backward(g.double().permute(0, 3, 1, 2))
    gp = g.double().permute(0, 3, 1, 2) * mask
    invstd = 1 / torch.sqrt(rv.double() + BN_EPS)
    terms_b = gp.abs().sum((0, 2, 3))
    # xhat inherits y's conv error (<= 2e-5 of max|y|) times invstd; the sums are <= 513-deep fp32 chains
    e_y = 2e-5 * float(y.detach().abs().max())
    xhat = (y.detach() - rm.double().view(1, -1, 1, 1)) * invstd.view(1, -1, 1, 1)
    _assert_bound(eng.param_grads[id(gam)], g64.grad,
                  terms_b * e_y * invstd + 520 * EPS * (gp * xhat).abs().sum((0, 2, 3)), "d-gamma")
    _assert_bound(eng.param_grads[id(bet)], be64.grad, 516 * EPS * terms_b, "d-beta")
    gxr = x64.grad.permute(0, 2, 3, 1)
    assert float((xa.grad[..., :Cin].double() - gxr).abs().max()) <= 2e-5 * float(gxr.abs().max()), "data gradient"
    if residual:
        assert torch.equal(ra.grad[..., :Cout].double(), r64.grad.permute(0, 2, 3, 1)), "residual gradient = masked g"
    if bias:
        gy_terms = (gp * (gam.detach().double() * invstd).view(1, -1, 1, 1)).abs().sum((0, 2, 3))
        _assert_bound(eng.param_grads[id(b)], b64.grad, 1e-5 * gy_terms, "conv bias gradient")


# ------------------------------------------------------------------------------------------------ one-pass statistics
# family: (entry point that must run, kind, k, stride, Cin, Cout, N, H, W, engine switches)
DC_FAMILIES = {
    "wino43": ("adh_conv_wino43_forward", "conv", 3, 1, 32, 96, 4, 256, 1024, {"USE_WINOGRAD": True, "USE_WINO43": True}),
    "wino_f23": ("adh_conv_wino_forward", "conv", 3, 1, 32, 96, 4, 256, 1024, {"USE_WINOGRAD": True, "USE_WINO43": False}),
    "wino32": ("adh_conv_wino32_forward", "convT", 4, 2, 32, 48, 4, 128, 512, {"USE_WINOGRAD": True}),
    # conv_rows: 3x3 on a 16 x 32-aligned grid with Cin % 16 == 0 and Cout % 32 == 0 (adh_conv_forward offers it first)
    "rows": ("adh_conv_forward", "conv", 3, 1, 32, 96, 4, 256, 1024, {"USE_WINOGRAD": False}),
    # conv_igemm: a 1x1 conv is no rows-kernel shape
    "igemm": ("adh_conv_forward", "conv", 1, 1, 32, 48, 4, 256, 1024, {"USE_WINOGRAD": False}),
    "stem": ("adh_conv_stem_forward", "conv", 7, 1, 3, 96, 4, 256, 1024, {}),     # the dehazing stem (7x7 s1, NHWC8 image)
    # conv_fewout.hip: its few-input form writes statistics; the <= 4-output form is never asked for them (Engine._run_gather)
    "fewin": ("adh_conv_fewin_forward", "conv", 3, 1, 3, 16, 4, 256, 1024, {}),
}


def _dc_ratio_and_ref(y64, gamma, beta):
    """per-channel mean / std of float64 y and the float64 normalized output gamma * (y - mean) / sqrt(var + eps) + beta"""
    dims = (0, 2, 3)
    mean = y64.mean(dims, keepdim=True)
    var = ((y64 - mean) ** 2).mean(dims, keepdim=True)
    ratio = float((mean.abs() / var.sqrt()).min())
    z = (y64 - mean) / torch.sqrt(var + BN_EPS) * gamma.double().view(1, -1, 1, 1) + beta.double().view(1, -1, 1, 1)
    return ratio, z.permute(0, 2, 3, 1)


def _check_dc(out, ref, ratio, what):
    assert ratio >= 25, f"{what}: mean / std of y is only {ratio:.1f}"
    err = float((out.double() - ref).abs().max())
    scale = float(ref.abs().max())
    assert err <= 2e-5 * scale, f"{what}: normalized output off by {err / scale:.2e} of its scale at mean / std {ratio:.0f}"


@pytest.mark.parametrize("family", list(DC_FAMILIES))
def test_train_bn_one_pass_statistics_with_dc_offset(family, monkeypatch):
    """Train-mode Engine.conv on outputs whose per-channel mean is 30 standard deviations (a conv bias puts it there), for
    every conv family whose epilogue writes the BatchNorm sums; the recorded entry point shows which family ran.

    The one-pass limit: the epilogues add fp32 sum y and sum y^2 per thread, and adh_bn_finalize forms
    var = Q / n - mean^2 in fp64, so the fp32 rounding of Q is amplified by (mean / sigma)^2 in var.  A CPU model of
    sequential fp32 per-thread sums over 2^20 pixels gave relative invstd errors of ~2e-6 at mean / sigma = 30 and ~3e-5
    at 100: past ~60 a centred-sums epilogue would be needed.  At 30 the normalized output must stay within 2e-5 of its
    scale (the full-size test's tolerance)."""
    import adam_dehaze_amd.engine as E
    entry, kind, k, stride, Cin, Cout, N, Hh, Ww, switches = DC_FAMILIES[family]
    for name, val in switches.items():
        monkeypatch.setattr(E, name, val)
    monkeypatch.setattr(E, "CONTRACT", "fp32")
    called = []
    real_call = H.call

    def recording(name, *a, **kw):
        called.extend((name, kw.get("family")))      # the entry point and the family it is accounted under
        return real_call(name, *a, **kw)
    monkeypatch.setattr(H, "call", recording)

    few = Cin <= 4
    x = _randn(N, Hh, Ww, 8 if few else Cin, seed=Cout + k)
    if few:
        x[..., Cin:] = 0.0                     # the NHWC8 image layout
    wshape = (Cin, Cout, k, k) if kind == "convT" else (Cout, Cin, k, k)
    fan = Cin * k * k // (4 if kind == "convT" else 1)
    w = _randn(*wshape, seed=Cout + k + 1) / fan ** 0.5
    x64 = x[..., :Cin].permute(0, 3, 1, 2).double()
    pad = 1 if kind == "convT" else (k - 1) // 2

    def conv64(bias):
        if kind == "convT":
            return F.conv_transpose2d(x64, w.double(), bias, stride=2, padding=1)
        return F.conv2d(x64, w.double(), bias, stride, pad)

    y0 = conv64(None)
    m0, s0 = y0.mean((0, 2, 3)), y0.std((0, 2, 3))
    del y0
    b = (30 * s0 - m0).float()                  # the bias puts every channel's mean at 30 standard deviations
    gamma, beta = _rand(Cout, seed=4) + 0.5, _randn(Cout, seed=5)
    bn = BNState(gamma, beta, torch.zeros(Cout, device=DEV), torch.ones(Cout, device=DEV),
                 torch.zeros((), device=DEV, dtype=torch.int64))
    eng = Engine(torch.device(DEV), record=False)
    o = eng.conv(Act(x, Cin if few else None), w, b, bn, kind=kind, k=k, stride=stride, pad=pad, relu=False, training=True)
    out = o.t[..., :Cout]
    torch.cuda.synchronize()
    assert entry in called, f"{family}: expected {entry} to run, got {sorted(set(called))}"
    y64 = conv64(b.double())
    ratio, ref = _dc_ratio_and_ref(y64, gamma, beta)
    del x64, y64
    _check_dc(out, ref, ratio, family)


def test_train_bn_one_pass_statistics_with_dc_offset_depthwise(monkeypatch):
    """The same for the depthwise kernel (Engine.dwconv, no bias): the offset comes from the input.  mu / sigma = 30 on x
    and taps near 1/9 (sum 1, norm ~1/3) give mu / sigma ~ 29 on y (the zero-padded borders add to its spread)."""
    called = []
    real_call = H.call

    def recording(name, *a, **kw):
        called.extend((name, kw.get("family")))      # the entry point and the family it is accounted under
        return real_call(name, *a, **kw)
    monkeypatch.setattr(H, "call", recording)
    N, Hh, Ww, C = 4, 256, 1024, 32
    x = 30.0 + _randn(N, Hh, Ww, C, seed=11)
    w = (1.0 + 0.1 * _randn(C, 1, 3, 3, seed=12)) / 9
    gamma, beta = _rand(C, seed=13) + 0.5, _randn(C, seed=14)
    bn = BNState(gamma, beta, torch.zeros(C, device=DEV), torch.ones(C, device=DEV),
                 torch.zeros((), device=DEV, dtype=torch.int64))
    eng = Engine(torch.device(DEV), record=False)
    o = eng.dwconv(Act(x), w, bn, k=3, stride=1, act=H.ACT_NONE, training=True)
    out = o.t[..., :C]
    torch.cuda.synchronize()
    assert "adh_dwconv_fwd" in called
    y64 = F.conv2d(x.permute(0, 3, 1, 2).double(), w.double(), None, 1, 1, 1, C)
    ratio, ref = _dc_ratio_and_ref(y64, gamma, beta)
    del y64
    _check_dc(out, ref, ratio, "depthwise")
