"""Float64 restatements, on the CPU, of the streaming kernels of csrc/depthwise.hip, csrc/densenet.hip and csrc/bn_act.hip, with
the error bounds their tests hold the kernels to.  Shared by the host-emulation tests (tests/test_*_hostemu_cpu.py) and
tests/test_gpu_depthwise.py.  Every function takes the float32 tensors the kernel receives and returns float64.

Bounds count roundings in units of EPS = 2^-24 times the sum of the absolute terms (the same operation on |inputs|): a chain of n
fused multiply-adds or additions is off by at most n EPS / (1 - n EPS) <= (n + 1) EPS of that sum.  `host` adds the roundings
the host compiler makes where the GPU compiler contracts a * b + c into one: the kernels' explicit fmaf is one rounding on both."""
import torch
import torch.nn.functional as F

EPS = 2.0 ** -24
ACT_NONE, ACT_RELU, ACT_RELU6, ACT_HARDSWISH, ACT_HARDSIGMOID = 0, 1, 4, 5, 6
ACTS = {ACT_NONE: lambda z: z, ACT_RELU: F.relu, ACT_RELU6: F.relu6, ACT_HARDSWISH: F.hardswish, ACT_HARDSIGMOID: F.hardsigmoid}


def gen(seed):
    return torch.Generator().manual_seed(seed)


# ------------------------------------------------------------------------------------------------ depthwise.hip
DW_C = [(4, 4), (12, 12), (72, 80), (260, 260)]            # (C, buffer width of the input): CQB = 1; R = 85 and an idle thread;
#                                                            a slice of a wider buffer; two chunks, the second with one live quad
DW_KS = [(3, 1), (3, 2), (5, 1), (5, 2)]
DW_IMAGES = [(1, 1, 1), (2, 2, 3), (1, 5, 7), (2, 9, 11)]  # k = 5 on 1x1: 24 of 25 taps outside; odd sizes under stride 2


def dw_out_hw(Hh, Ww, k, s):
    pad = (k - 1) // 2
    return (Hh + 2 * pad - k) // s + 1, (Ww + 2 * pad - k) // s + 1


def dw_split(C):
    """(CQB, R, chunks) of csrc/depthwise.hip's block layout: up to 64 channel quads times R = 256 / CQB pixel lanes"""
    CQ = C // 4
    CQB = min(CQ, 64)
    return CQB, 256 // CQB, (CQ + CQB - 1) // CQB


def _dw_ppb(P, C, target, lo, hi):
    CQB, R, chunks = dw_split(C)
    want = max(1, target // chunks)
    ppt = min(max((P + want * R - 1) // (want * R), lo), hi)
    return ppt * R


def dw_fwd_blocks(P, C):
    return -(-P // _dw_ppb(P, C, 2048, 2, 16))


def dw_wgrad_blocks(P, C):
    return -(-P // _dw_ppb(P, C, 1024, 16, 64))


def dw_se_blocks(HW, C):
    return -(-HW // _dw_ppb(HW, C, 64, 4, 64))


def dw_case(N, Hh, Ww, C, k, s, seed):
    """x [N, H, W, C], w [C, 1, k, k], g [N, OH, OW, C], per-channel scale / shift: float32"""
    g = gen(seed)
    OH, OW = dw_out_hw(Hh, Ww, k, s)
    x = torch.randn(N, Hh, Ww, C, generator=g)
    w = torch.randn(C, 1, k, k, generator=g) / k
    gr = torch.randn(N, OH, OW, C, generator=g)
    sc = torch.randn(C, generator=g)
    sc[::5] = 0.0
    sh = torch.randn(C, generator=g) * 2
    return x, w, gr, sc, sh


def _nchw(t):
    return t.double().permute(0, 3, 1, 2)


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def dw_fwd64(x, w, k, s):
    """(y, terms): the depthwise convolution and the same sum over |x| |w|, [N, OH, OW, C]"""
    C = x.shape[3]
    pad = (k - 1) // 2
    y = F.conv2d(_nchw(x), w.double(), None, s, pad, 1, C)
    ya = F.conv2d(_nchw(x).abs(), w.double().abs(), None, s, pad, 1, C)
    return _nhwc(y), _nhwc(ya)


def dw_grads64(x, w, g, k, s):
    """(gx, gx terms, dw, dw terms) by autograd on the float64 convolution (and on the absolute values)"""
    C = x.shape[3]
    pad = (k - 1) // 2
    out = []
    for xx, ww, gg in ((_nchw(x), w.double(), _nchw(g)), (_nchw(x).abs(), w.double().abs(), _nchw(g).abs())):
        xx, ww = xx.clone().requires_grad_(True), ww.clone().requires_grad_(True)
        gx, dw = torch.autograd.grad(F.conv2d(xx, ww, None, s, pad, 1, C), (xx, ww), gg)
        out += [_nhwc(gx), dw]
    return out[0], out[2], out[1], out[3]


def dw_depth(P, C, max_ppt):
    """fp32 additions behind one per-block partial: a lane's chain over its pixels, then the R lanes of its channel quad"""
    _, R, _ = dw_split(C)
    return min(max_ppt, -(-P // R)) + R


def dw_fwd_bound(terms, k):
    # k^2 fused multiply-adds, one rounding each
    return (k * k + 1) * EPS * terms


def dw_stats_bounds(y, terms, C, k):
    """sums over all pixels of y and y^2 (the test adds the per-block rows in float64): every y is off by dw_fwd_bound; the
    square doubles that relative error and its fma rounds once; then the accumulation chain"""
    P = y.shape[0] * y.shape[1] * y.shape[2]
    d = dw_depth(P, C, 16)
    t1 = terms.reshape(P, C).sum(0)
    t2 = (terms * terms).reshape(P, C).sum(0)
    return (k * k + 1 + d + 1) * EPS * t1, (2 * (k * k + 1) + 1 + d + 1) * EPS * t2


def dw_eval64(y, terms, sc, sh, act, k):
    """(act(y * scale + shift), bound).  z = fma(y, scale, shift): the error of y times |scale| and one rounding.  ReLU and
    ReLU6 are exact and 1-Lipschitz.  Hardsigmoid adds the rounding of z + 3 and a division by 6 (4 EPS of the result: room
    for a reciprocal multiply); Hardswish, of slope at most 1.5, adds the product's rounding to those."""
    sc, sh = sc.double(), sh.double()
    z = y * sc + sh
    ez = dw_fwd_bound(terms, k) * sc.abs() + EPS * ((y * sc).abs() + sh.abs())
    ref = ACTS[act](z)
    if act == ACT_HARDSIGMOID:
        return ref, (ez + EPS * (z.abs() + 3)) / 6 + 4 * EPS * ref.abs()
    if act == ACT_HARDSWISH:
        return ref, 1.5 * ez + z.abs() * EPS * (z.abs() + 3) / 6 + 5 * EPS * ref.abs()
    return ref, ez


def dw_dgrad_bound(terms, k, prior=None):
    # at most k^2 fused multiply-adds; accumulate: one more addition, rounded once
    b = (k * k + 1) * EPS * terms
    return b if prior is None else b + EPS * (terms + prior.double().abs())


def dw_wgrad_bound(terms, P, C, prior=None):
    # a lane's fma chain and the R lanes in fp32, the blocks in float64, one rounding to fp32; accumulate: one more addition
    b = (dw_depth(P, C, 64) + 2) * EPS * terms
    return b if prior is None else b + EPS * (terms + prior.double().abs())


def se_case(N, HW, C, seed):
    g = gen(seed)
    return torch.randn(N, HW, C, generator=g), torch.rand(N, C, generator=g), torch.randn(N, HW, C, generator=g)


def se_fwd64(x, s):
    """(x * s[n], bound): one correctly rounded product"""
    ref = x.double() * s.double()[:, None, :]
    return ref, EPS * ref.abs()


def se_bwd64(g, x, s, nblk):
    """(gx, gx bound, gs, gs bound): gx = g * s[n] rounds once; gs[n] = sum over the pixels of g * x: a lane's fma chain, the R
    lanes of the channel quad and the nblk per-block rows, all in fp32"""
    N, HW, C = x.shape
    gx = g.double() * s.double()[:, None, :]
    gs = (g.double() * x.double()).sum(1)
    terms = (g.double() * x.double()).abs().sum(1)
    return gx, EPS * gx.abs(), gs, (dw_depth(HW, C, 64) + nblk + 1) * EPS * terms


# ------------------------------------------------------------------------------------------------ densenet.hip / bn_act.hip
BN_EPS = float(torch.tensor(1e-5, dtype=torch.float32))       # the fp32 values the kernels receive
MOM = float(torch.tensor(0.1, dtype=torch.float32))
U64 = 2.0 ** -53                                               # float64 unit roundoff


def grid(shape, lo, hi, den, seed):
    """integers in [lo, hi] / den as fp32: sums and products of a few of them are exact in fp32 and float64"""
    return torch.randint(lo, hi + 1, shape, generator=gen(seed)).float() / den


def group_lanes(C):
    """per channel, R = 256 / (quads of its group of 1024 channels): the pixel lanes of bn_slice_stats / bn_bwd_reduce"""
    c = torch.arange(C)
    quads = torch.clamp(C - c // 1024 * 1024, max=1024) // 4
    return 256 // quads


def rows_depth(P, C, ppb):
    """fp32 additions behind one per-block row of those kernels, per channel: a lane's chain over its pixels, then R lanes"""
    R = group_lanes(C)
    return (min(P, ppb) + R - 1) // R + R


def slice_stats64(x, ppb=512, host=0):
    """(sum x, bound, sum x^2, bound) over all pixels of x [P, C] (the test adds the per-block rows in float64).  x * x + q is
    one rounding where the compiler contracts it and two (`host` = 1) where it does not."""
    P, C = x.shape
    d = rows_depth(P, C, ppb).double()
    x = x.double()
    s, q = x.sum(0), (x * x).sum(0)
    return s, (d + 1) * EPS * x.abs().sum(0), q, (d + 1 + host) * EPS * q


def moments64(part, C, count):
    """(mean, bound, var, bound) of partials [nblk, 2, pitch]: float64 sums in another order, a division, and for the variance a
    product and a difference -- nblk + 4 roundings of 2^-53 of the terms"""
    nblk = part.shape[0]
    S, Q = part[:, 0, :C].double().sum(0), part[:, 1, :C].double().sum(0)
    Sa, Qa = part[:, 0, :C].double().abs().sum(0), part[:, 1, :C].double().abs().sum(0)
    mean = S / count
    var = (Q / count - mean * mean).clamp_min(0)
    return mean, (nblk + 4) * U64 * Sa / count, var, (nblk + 4) * U64 * (Qa / count + 2 * (Sa / count) ** 2)


def fold64(mean, var, count, gamma, beta, rm, rv, host=0):
    """adh_bn_finalize's arithmetic after its reduce, from float64 moments: {name: (value, bound)}.  scale, shift, mean and
    invstd are float64 values (a few roundings of 2^-53 of their terms) rounded to fp32 once.  The running statistics
    (1 - m) r + m v round fp32(v), 1 - m, one product and the contracted product-sum: 4 EPS of the terms, 5 on the host."""
    invstd = 1.0 / torch.sqrt(var + BN_EPS)
    gm = gamma.double() if gamma is not None else torch.ones_like(mean)
    bt = beta.double() if beta is not None else torch.zeros_like(mean)
    unb = var * count / (count - 1) if count > 1 else var      # BatchNorm2d's unbiased running estimate; none at n = 1
    t = mean * gm * invstd
    out = {"scale": (gm * invstd, (EPS + 8 * U64) * (gm * invstd).abs()),
           "shift": (bt - t, EPS * (bt - t).abs() + 8 * U64 * (bt.abs() + t.abs())),
           "mean": (mean, (EPS + 8 * U64) * mean.abs()), "invstd": (invstd, (EPS + 8 * U64) * invstd)}
    if rm is not None:
        out["rm"] = ((1 - MOM) * rm.double() + MOM * mean, (4 + host) * EPS * ((1 - MOM) * rm.double().abs() + MOM * mean.abs()))
    if rv is not None:
        out["rv"] = ((1 - MOM) * rv.double() + MOM * unb, (4 + host) * EPS * ((1 - MOM) * rv.double().abs() + MOM * unb.abs()))
    return out


def avgpool2_bwd64(g, Hh, Ww):
    """g [N, H/2, W/2, C] -> gx [N, H, W, C]: g / 4 (exact) under the 2x2 windows, 0 in a dropped odd row / column"""
    N, OH, OW, C = g.shape
    gx = torch.zeros(N, Hh, Ww, C, dtype=torch.float64)
    gx[:, :2 * OH, :2 * OW] = (g.double() / 4).repeat_interleave(2, 1).repeat_interleave(2, 2)
    return gx


def preact_bwd64(dA, x, ss, mean, invstd, coef, training):
    """(dx, bound) of adh_bn_preact_bwd_accum's store form.  The mask is fma(x, scale, shift) > 0: callers pass grid values
    for x and ss, so that z is exact and the float64 mask is the kernel's.  training: kx = invstd * coef2, x - mean, its
    product by kx, the two differences and the product by coef0 -- six roundings (the GPU contracts one away), each at most
    EPS / (1 - 6 EPS) of the terms: 7 EPS.  Frozen statistics: one product."""
    dA, x, ss, coef = dA.double(), x.double(), ss.double(), coef.double()
    gp = torch.where(x * ss[0] + ss[1] > 0, dA, torch.zeros_like(dA))
    if not training:
        r = coef[0] * gp
        return r, EPS * r.abs()
    t = (x - mean.double()) * (invstd.double() * coef[2])
    return coef[0] * (gp - coef[1] - t), 7 * EPS * coef[0].abs() * (gp.abs() + coef[1].abs() + t.abs())


# ------------------------------------------------------------------------------------------------ bn_act.hip
def partials(nblk, C, pitch, count, seed):
    """fp32 per-block (sum y, sum y^2) [nblk, 2, pitch] of a virtual batch of `count` elements split unevenly over the blocks.
    Block means scatter around a per-channel mean, so Q / n - mean^2 >= sigma^2 > 0; channel 2 has Q / n < mean^2 (the clamp
    to a zero variance).  The padding columns [C, pitch) are NaN: the kernels must not read them."""
    g = gen(seed)
    mu = torch.randn(1, C, dtype=torch.float64, generator=g) * 2
    sig2 = torch.rand(1, C, dtype=torch.float64, generator=g) * 4 + 0.25
    m_b = mu + 0.25 * torch.randn(nblk, C, dtype=torch.float64, generator=g)
    w = torch.rand(nblk, 1, dtype=torch.float64, generator=g) + 0.5
    w = w / w.sum() * count
    part = torch.full((nblk, 2, pitch), float("nan"))
    part[:, 0, :C] = (w * m_b).float()
    part[:, 1, :C] = (w * (sig2 + m_b * m_b)).float()
    if C > 2:
        part[:, 0, 2] = (w[:, 0] * 1.5).float()
        part[:, 1, 2] = (w[:, 0] * 2.25 * 0.999).float()
    return part


def finalize64(part, C, count, gamma, beta, rm, rv, host=0):
    """adh_bn_finalize from the rows: fold64 of moments64, the moments' own float64 errors carried to first order (doubled)
    through invstd = (var + eps)^-1/2 into scale and shift"""
    mean, b_m, var, b_v = moments64(part, C, count)
    out = fold64(mean, var, count, gamma, beta, rm, rv, host)
    invstd = out["invstd"][0]
    gm = gamma.double().abs() if gamma is not None else torch.ones_like(mean)
    e_is = invstd ** 3 * b_v                                   # 2 x |d invstd / d var| b_v
    extra = {"scale": gm * e_is, "shift": gm * (2 * b_m * invstd + mean.abs() * e_is), "mean": b_m, "invstd": e_is,
             "rm": MOM * b_m, "rv": MOM * 2 * b_v}
    return {k: (v, b + extra[k]) for k, (v, b) in out.items()}


def fold_eval64(gamma, beta, rm, rv, bias):
    """(scale, bound, shift, bound) of adh_bn_fold_eval, all fp32: rv + eps, sqrtf, the reciprocal and the gamma product -- 8
    EPS of the scale (room for an approximate sqrt / reciprocal); the shift adds two products of that scale and two sums (12 EPS
    of its terms), and on the host the two roundings a contraction would save (14)"""
    invstd = 1 / torch.sqrt(rv.double() + BN_EPS)
    scale = invstd * gamma.double() if gamma is not None else invstd
    shift = -rm.double() * scale
    terms = shift.abs()
    if beta is not None:
        shift, terms = shift + beta.double(), terms + beta.double().abs()
    if bias is not None:
        shift, terms = shift + bias.double() * scale, terms + (bias.double() * scale).abs()
    return scale, 8 * EPS * scale.abs(), shift, 14 * EPS * terms


def packbits(m):
    """[P, C] bool -> bytes holding bit p * C + c of the flat array (LSB first): adh_bn_apply's nibble layout, byte
    (p * CQ + cq) / 2 holding quad cq's four channels in nibble cq % 2"""
    b = m.reshape(-1, 8).to(torch.int32) << torch.arange(8, dtype=torch.int32)
    return b.sum(1).to(torch.uint8)


def apply_case(P, C, seed):
    """grid inputs: y in [-3, 3] step 1/8, scale in [-2, 2] step 1/4 (0 included), shift and residual in [-2, 2] step 1/8:
    z = fma(y, scale, shift) (+ r) is exact in fp32, and lands on 0, +-3 and 6 often: every activation's kinks"""
    return grid((P, C), -24, 24, 8, seed), grid((P, C), -16, 16, 8, seed + 1), grid((C,), -8, 8, 4, seed + 2), \
        grid((C,), -16, 16, 8, seed + 3)


def act_bwd64(act, z, g):
    """(g' = g times the activation's derivative at z with torch autograd's kink conventions, the error the kernel's own
    arithmetic leaves in it).  Hardswish: g (z / 3 + 0.5) rounds the division (4 EPS of |z| / 3: room for a reciprocal
    multiply), the sum and the product (1 EPS of |z| / 3 + 0.5 each): the terms cancel near z = -1.5, so the error is 6 EPS
    of |g| (|z| / 3 + 0.5), not of the result.  Hardsigmoid: one division, 4 EPS.  The others select, exactly."""
    zero = torch.zeros_like(g)
    if act == ACT_RELU:
        return torch.where(z > 0, g, zero), zero
    if act == ACT_RELU6:
        return torch.where((z > 0) & (z < 6), g, zero), zero
    if act == ACT_HARDSWISH:
        return torch.where(z <= -3, zero, torch.where(z < 3, g * (z / 3 + 0.5), g)), 6 * EPS * g.abs() * (z.abs() / 3 + 0.5)
    if act == ACT_HARDSIGMOID:
        return torch.where((z > -3) & (z < 3), g / 6, zero), 4 * EPS * g.abs() / 6
    return g, zero


def bwd_reduce64(gp, e_gp, y, mean, invstd, P, ppb, host=0):
    """(sum g', bound, sum g' xhat, bound) over all pixels (the test adds the per-block rows in float64).  Per term: the error
    e_gp inside g', and for g' xhat the roundings of y - mean and of two products; then a lane's chain over its pixels of the
    block and the R lanes of its channel quad, the product-sum contracted on the GPU and not on the host."""
    C = gp.shape[1]
    d = rows_depth(P, C, ppb).double()
    xhat = (y.double() - mean.double()) * invstd.double()
    return (gp.sum(0), (d + 1) * EPS * gp.abs().sum(0) + e_gp.sum(0), (gp * xhat).sum(0),
            (d + 4 + host) * EPS * (gp * xhat).abs().sum(0) + (e_gp * xhat.abs()).sum(0))


def bwd_apply64(gp, e_gp, y, mean, invstd, coef, training):
    """(g_y, bound).  training: coef0 (g' - coef1 - (y - mean) (invstd coef2)) -- kx = invstd * coef2, y - mean, its product by
    kx, the two differences and the product by coef0: six roundings (the GPU contracts one away), 7 EPS of the terms, and
    the error e_gp inside g'.  Frozen statistics: coef0 g', one product."""
    coef = coef.double()
    if not training:
        r = coef[0] * gp
        return r, EPS * r.abs() + coef[0].abs() * e_gp
    t = (y.double() - mean.double()) * (invstd.double() * coef[2])
    return coef[0] * (gp - coef[1] - t), coef[0].abs() * (7 * EPS * (gp.abs() + coef[1].abs() + t.abs()) + e_gp)
