"""Float64 restatements, case builders and error bounds of the entry points of csrc/pointwise.hip, shared by
tests/test_gpu_pointwise.py (the library on the GPU) and tests/test_pointwise_hostemu_cpu.py (the same source compiled for the
host under the sanitizers).  Everything here runs on CPU tensors; the GPU test moves the inputs to the device.  Bounds are in
units of EPS = 2^-24, the fp32 unit roundoff; each comment says which fp32 operations a bound counts.

`host`: the host compiler does not contract a * b + c.  Where a bound counts ONE rounding for such an expression, because the
device contracts it into an fma, host = 1 adds one unit of the absolute terms per expression; where a bound already counts the
product and the addition apart, nothing is added.  The GPU test passes host = 0 everywhere: its bounds are the ones it has
always held the library to."""
import torch
import torch.nn.functional as F

from tests import _ref64 as R64

EPS = 2.0 ** -24


def gen(seed):
    return torch.Generator().manual_seed(seed)


def rand(*shape, seed=0):
    return torch.rand(shape, dtype=torch.float32, generator=gen(seed))


def randn(*shape, seed=0):
    return torch.randn(shape, dtype=torch.float32, generator=gen(seed))


def rel(a, ref):
    """max|a - ref| / max|ref| (a's NaNs count as infinitely wrong)."""
    d = (a.double() - ref).abs()
    if torch.isnan(d).any():
        return float("inf")
    return float(d.max() / ref.abs().max().clamp_min(1e-300))


def nchw64(t_nhwc):
    return t_nhwc.permute(0, 3, 1, 2).double().contiguous()


# ------------------------------------------------------------------------------------------------ MaxPool
MP_CFG = [(2, 2, 0), (4, 4, 0), (3, 2, 1), (3, 2, 0), (1, 2, 0)]


def maxpool_inputs(N, Hh, Ww, k, s, p, x_cs, g_cs, seed):
    """values from {0, 1, 2}: nearly every window ties.  Gradients are multiples of 1/4 in [-2, 2]: every sum the backward
    forms is exact in fp32, so the gradient must equal float64 autograd exactly.  -> (xb [N, H, W, x_cs], gb [N, OH, OW, g_cs])"""
    xb = torch.randint(0, 3, (N, Hh, Ww, x_cs), generator=gen(seed)).float()
    OH, OW = (Hh + 2 * p - k) // s + 1, (Ww + 2 * p - k) // s + 1
    gb = torch.randint(-8, 9, (N, OH, OW, g_cs), generator=gen(seed + 1)).float() / 4
    return xb, gb


def maxpool_ref(x, g, k, s, p):
    """x [N, H, W, C], g [N, OH, OW, C] -> (pooled, arg-max indices, input gradient), NCHW float64 / int64"""
    x64 = nchw64(x).requires_grad_(True)
    y, ind = F.max_pool2d(x64, k, s, p, return_indices=True)
    y.backward(nchw64(g))
    return y.detach(), ind, x64.grad


# ------------------------------------------------------------------------------------------------ bilinear resize
def src_err(n_in, n_out, align):
    """max |fp32 - float64| of the source coordinate along one axis: the only error of the resize weights."""
    o = torch.arange(n_out, dtype=torch.float64)
    if align:
        s64 = o * ((n_in - 1) / (n_out - 1) if n_out > 1 else 0.0)
        s32 = o.float() * torch.tensor((n_in - 1) / (n_out - 1) if n_out > 1 else 0.0, dtype=torch.float32)
    else:
        s64 = ((o + 0.5) * (n_in / n_out) - 0.5).clamp_min(0)
        s32 = ((o.float() + 0.5) * torch.tensor(n_in / n_out, dtype=torch.float32) - 0.5).clamp_min(0)
    return float((s32.double() - s64).abs().max())


BL_CASES = [
    # N, H, W, C, OH, OW, align_corners, x_cs, out_cs (out_cs > C: written at channel offset 4 of a wider buffer)
    (2, 19, 23, 16, 38, 46, 1, 16, 16),          # x2 (CORUN-inspired, DualBranch)
    (1, 13, 17, 8, 52, 68, 1, 16, 8),            # x4, input read from a channel slice
    (2, 1, 9, 4, 3, 33, 1, 4, 4),                # one-row input
    (2, 5, 9, 4, 1, 17, 1, 4, 4),                # OH = 1: the `out > 1 ? ... : 0` branch
    (2, 7, 1, 4, 15, 1, 1, 4, 4),                # one-column input, OW = 1
    (2, 8, 12, 12, 17, 25, 0, 12, 12),           # non-integer up-sampling
    (1, 301, 401, 12, 200, 266, 0, 12, 12),      # non-integer down-sampling (detector transform); backward loops
    (2, 9, 11, 16, 19, 23, 0, 16, 28),           # into a channel slice of a concat buffer (_UNetTrunk's out=)
    (1, 1, 7, 4, 5, 13, 0, 4, 4),                # one-row input, align_corners=False
    (1, 256, 512, 32, 512, 1024, 1, 32, 32),     # x2 at a CORUN-sized plane: both grid-stride loops run several times
]


def bilinear_inputs(N, Hh, Ww, C, OH, OW, x_cs):
    """-> (xb [N, H, W, x_cs] in [0, 1), g [N, OH, OW, C]); g is positive: |reference| ~ the sum of |terms| the backward adds"""
    return rand(N, Hh, Ww, x_cs, seed=Hh * 7 + Ww), rand(N, OH, OW, C, seed=OH + OW)


def bilinear_ref(x, g, OH, OW, align):
    """x [N, H, W, C], g [N, OH, OW, C] -> (resized, input gradient) as NHWC float64"""
    x64 = nchw64(x).requires_grad_(True)
    y = F.interpolate(x64, size=(OH, OW), mode="bilinear", align_corners=bool(align))
    y.backward(nchw64(g))
    return y.detach().permute(0, 2, 3, 1), x64.grad.permute(0, 2, 3, 1)


def bilinear_bounds(Hh, Ww, OH, OW, align, host=0):
    """(forward, backward) bounds of rel(), and the source-coordinate error ds they are made of.
    Both sides use ATen's source-coordinate formula; the kernel evaluates it in fp32 like ATen's fp32 path.  An error ds in a
    coordinate moves an output by at most ds * (neighbour difference <= max|x| for x in [0, 1)) and a weight by ds.
    Backward: up to (2 * ratio + 1)^2 fp32 products summed per input element, in two levels (row sums, then rows).
    host: the three a * b + c of the forward's lerp; one per level of the backward's sums."""
    ds = src_err(Hh, OH, align) + src_err(Ww, OW, align)
    return 4 * ds + (8 + 3 * host) * EPS, 8 * ds + (64 + 2 * host) * EPS, ds


# ------------------------------------------------------------------------------------------------ branch-head blends
BLEND_ALPHA = 0.3125


def blend_ref(mode, x, r, gd, a):
    if mode == 0:
        return (1 - a) * x + a * torch.sigmoid(r)
    if mode == 1:
        return torch.clamp(x + torch.tanh(r), 0, 1)
    if mode == 2:
        return torch.clamp(x + torch.tanh(r) * torch.sigmoid(gd), 0, 1)
    if mode == 3:
        return torch.clamp(x + (torch.sigmoid(r) - 0.5) * 2, 0, 1)
    return torch.clamp(x + torch.tanh(r) * (1 - torch.sigmoid(gd)), 0, 1)


def raw(mode, x, r, gd):
    """x + delta before the clamp."""
    if mode == 1:
        return x + torch.tanh(r)
    if mode == 2:
        return x + torch.tanh(r) * torch.sigmoid(gd)
    if mode == 3:
        return x + (torch.sigmoid(r) - 0.5) * 2
    return x + torch.tanh(r) * (1 - torch.sigmoid(gd))


def blend_inputs(mode, N, Hh, Ww, r_cs, gd_cs, seed):
    """x in [0, 1], pre-activations r (channels 0..2 of r_cs) and gd (channel 0 of gd_cs).  Every 5th pixel has r = 0 and
    x on a clamp bound, where x + delta is exactly 0 or 1 in both fp32 and float64 (tanh(0) = 0, sigmoid(0) = 0.5): torch's
    clamp passes the gradient there.  Elsewhere r is zeroed wherever float64 puts x + delta within 1e-4 of a bound, so that
    fp32 rounding cannot flip the clamp mask."""
    x = rand(N, 3, Hh, Ww, seed=seed)
    rb = randn(N, Hh, Ww, r_cs, seed=seed + 1) * 1.5
    gdb = randn(N, Hh, Ww, gd_cs, seed=seed + 2) * 2
    edge = (torch.arange(N * Hh * Ww) % 5 == 0).view(N, Hh, Ww)
    x[:, 0][edge] = 0.0
    x[:, 1][edge] = 1.0
    x[:, 2][edge] = torch.where(torch.arange(int(edge.sum())) % 2 == 0, 0.0, 1.0)
    rb[..., :3][edge] = 0.0
    if mode != 0:
        rw = raw(mode, x.double(), rb[..., :3].permute(0, 3, 1, 2).double(), gdb[..., :1].permute(0, 3, 1, 2).double())
        near = ((rw.abs() < 1e-4) | ((rw - 1).abs() < 1e-4)).permute(0, 2, 3, 1)
        rb[..., :3][near] = 0.0
    return x.contiguous(), rb, gdb


def blend_ref_grads(mode, x, rb, gdb, g, alpha=BLEND_ALPHA):
    """-> (y [N, 3, H, W], g_r [N, H, W, 3], g_gd [N, H, W, 1], g_alpha, the sum of |terms| of g_alpha), float64"""
    r64 = rb[..., :3].permute(0, 3, 1, 2).double().requires_grad_(True)
    gd64 = gdb[..., :1].permute(0, 3, 1, 2).double().requires_grad_(True)
    a64 = torch.tensor([alpha], dtype=torch.float64, device=x.device).requires_grad_(True)
    y = blend_ref(mode, x.double(), r64, gd64, a64)
    y.backward(g.double())
    terms = (g.double() * (torch.sigmoid(r64.detach()) - x.double())).abs().sum()
    ggd = gd64.grad.permute(0, 2, 3, 1) if gd64.grad is not None else None
    return y.detach(), r64.grad.permute(0, 2, 3, 1), ggd, (float(a64.grad) if a64.grad is not None else None), float(terms)


def blend_bounds(host=0):
    """(forward, absolute; gradients, of rel(); alpha gradient, per unit of the sum of |terms|)
    forward: expf / tanhf are faithful to a few ulp, then two or three fp32 operations on values of size <= 2
    gradients: products of a few faithfully rounded factors (the gate gradient adds three of them)
    alpha: fp32 sums per thread, wave and block, then fp64 over the block partials
    host: x + t * gate and (1 - a) x + a s of the forward (terms <= 2); 1 - t * t (<= 2) times a factor of the size of the
    result, and ggd += m * t, in the gradients; ga += gv * (sr - xv)"""
    return (16 + 2 * host) * EPS, (32 + 4 * host) * EPS, (64 + host) * EPS


# ------------------------------------------------------------------------------------------------ routing
def logits3(N, seed):
    lg = randn(N, 3, seed=seed) * 4
    lg[::7] = torch.tensor([80.0, -80.0, 3.0])
    lg[3::7] = torch.tensor([-80.0, -80.0, 80.0])
    return lg


def softmax3_ref(lg, gwp, T):
    """-> (weights, g_logits, max |summed weight gradient|), float64"""
    l64 = lg.double().requires_grad_(True)
    w64 = torch.softmax(l64 / T, dim=1)
    G = gwp.double().sum(1)
    w64.backward(G)
    return w64.detach(), l64.grad, float(G.abs().max())


def softmax3_bounds(Gmax, T, host=0):
    """(weights: expf and one division per weight (weights <= 1); g_logits: w * (g - dot) / T, a few roundings of terms bounded
    by max|G| / T).  host: the two a * b + c of the three-term dot"""
    return 8 * EPS, (32 + 2 * host) * EPS * Gmax / T


def soft_blend_ref(w, o, g):
    """w [N, 3], o three [N, per], g [N, per] -> (out, [g_i], gw, the sums of |terms| of gw [N, 3]), float64"""
    w64 = w.double().requires_grad_(True)
    o64 = [t.double() for t in o]
    y = sum(w64[:, i:i + 1] * o64[i] for i in range(3))
    y.backward(g.double())
    terms = torch.stack([(g.double() * o64[i]).abs().sum(1) for i in range(3)], 1)
    return y.detach(), [g.double() * w.double()[:, i:i + 1] for i in range(3)], w64.grad, terms


def soft_blend_bounds(host=0):
    """(out: three products and two adds of terms in [0, 1], absolute; gw: fp32 per-lane sums, wave and block trees, per unit of
    the sum of |terms|).  g_i is one rounded product on either compiler: EPS |ref|.  host: two a * b + c in the blend; the
    products of the weight sums are contracted into the pairwise adds on the device only"""
    return (8 + 2 * host) * EPS, (64 + host) * EPS


def argmax3_first(lg):
    return torch.tensor([max(range(3), key=lambda j, row=row: (row[j], -j)) for row in lg.tolist()])


# ------------------------------------------------------------------------------------------------ losses
LOSS_N = [1, 3, 4097, 4096 * 2048 + 5, 8 * 3 * 512 * 1024]            # the GPU test's: past the 2048-block cap
LOSS_N_HOST = [1, 3, 4, 5, 4097, 2 * 4096 + 7]                          # the host test's: blocks of exactly n floats
LOSS_REL = 1e-6     # all terms are >= 0: fp32 per-lane sums of 4-element pairs, wave and block trees (< 32 roundings deep in all),
#                     fp64 over the blocks; 1e-6 relative bounds it with room to spare (contracted or not)


def diff_mean_ref(a, b, sq):
    d = a.double() - b.double()
    return float((d * d).mean() if sq else d.abs().mean())


def diff_bwd_ref(a, b, sq, u):
    """gradient of u * mean(|a - b|) or u * mean((a - b)^2) with respect to a, float64"""
    x = a.double().clone().requires_grad_(True)
    d = x - b.double()
    ((d * d).mean() * u if sq else d.abs().mean() * u).backward()
    return x.grad


L1_BWD_EPS = 3      # +-fp32(fp32(1/n) * upstream): two roundings, relative to the result
MSE_BWD_EPS = 5     # 2 * fp32(a - b) * fp32(fp32(1/n) * upstream): four roundings


def cross_entropy3_inputs(N):
    lg = randn(N, 3, seed=N + 200) * 3
    lg[::2] *= 300                       # logits of order +-1e3 in every other row
    lab = torch.randint(0, 3, (N,), generator=gen(N + 201), dtype=torch.int64)
    return lg, lab


def cross_entropy3_ref(lg, lab, host=0):
    """-> (loss, dlogits, the loss bound, the dlogits bound)
    loss: per row, log(sum) + max - logit in fp32: a few roundings of terms as large as |max| + |logit|
    dlogits: softmax / N - onehot / N: expf, a sum, two products, a division and a subtraction of terms <= 1 / N; host: the
    subtraction is contracted with the product on the device only"""
    N = lg.shape[0]
    l64 = lg.double().requires_grad_(True)
    ref = F.cross_entropy(l64, lab)
    ref.backward()
    scale = float((lg.double().abs().max(1).values * 2 + 2).mean())
    return float(ref.detach()), l64.grad, 8 * EPS * scale, (16 + host) * EPS / N


# ------------------------------------------------------------------------------------------------ Adam, one tensor
ADAM_POW_UNITS = R64.ADAM_POW_UNITS      # powf of the bias corrections: adam_kernel calls the same powf, per element
ADAM_STEP_N = [1, 255, 257, 1500]


def adam_step_case(n, seed):
    """p, g, m, v (v >= 0) of one tensor"""
    p, g, m = randn(n, seed=seed), randn(n, seed=seed + 1) * 2, randn(n, seed=seed + 2) * 0.1
    return p, g, m, (randn(n, seed=seed + 3) * 0.01).abs()


def adam_step_ref(p, g, m, v, step, repeats, lr, beta1, beta2, eps, wd):
    """adh_adam_step: `repeats` consecutive full updates (tests/_ref64.adam, dup_mode 0) -> ((p, m, v), their bounds)"""
    return R64.adam(p, g, m, v, step, repeats, 0, lr=lr, beta1=beta1, beta2=beta2, eps=eps, wd=wd, gscale=1.0,
                    pow_units=ADAM_POW_UNITS)


# ------------------------------------------------------------------------------------------------ layout
LAYOUT_C = [1, 3, 31, 32, 33, 40]
LAYOUT_HW = [1, 31, 32, 33, 70]
IMAGENET_MEAN, IMAGENET_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
