"""Float64 restatements of the entry points of csrc/cbam.hip (the AttentionBlock, base_model.py:43-78) and their error bounds in
units of EPS = 2^-24, the fp32 unit roundoff, relative to the sum of |terms| a kernel adds; each comment says which fp32
operations a bound counts.  Shared by tests/test_gpu_cbam.py (the library on the GPU) and tests/test_cbam_hostemu_cpu.py (the
same source compiled for the host under the sanitizers); device-agnostic: every function computes on the device of its inputs.

`host`: the host compiler does not contract a * b + c.  Where a bound counts ONE rounding for such an expression, because the
device contracts it into an fma, host = 1 adds one more per expression; where a bound already counts the product and the
addition apart, nothing is added."""
import torch
import torch.nn.functional as F

EPS = 2.0 ** -24
POOL_PPB = 512          # pixels per block of the pooling partials (cbam.hip)
# images smaller than the 7 x 7 window, and both edges of the 32 x 8 tiles of cbam_sa_kernel
APPLY_HW = [(1, 1), (1, 40), (2, 7), (6, 33), (7, 8), (8, 6), (33, 40), (40, 2), (7, 7), (2, 1)]


def first_argmax(x, dim):
    """index of the FIRST maximum along dim (torch.argmax does not promise which of equal maxima it returns)."""
    n = x.shape[dim]
    shape = [1] * x.dim()
    shape[dim] = n
    ar = torch.arange(n, device=x.device).view(shape)
    return torch.where(x == x.amax(dim, keepdim=True), ar, n).amin(dim)


def assert_bound(got, ref64, bound, what):
    assert not torch.isnan(got).any(), f"{what}: NaN (an element was not written)"
    d = (got.double() - ref64).abs() - bound
    assert float(d.max()) <= 0, f"{what}: exceeds its bound by {float(d.max()):.3e}"


# ------------------------------------------------------------------------------------------------ forward
def pool64(x):
    """x [N, HW, C] float64 whose sums are exact in fp32 -> (mean rounded to fp32 once, max, first arg-max), all exact"""
    return (x.sum(1) / x.shape[1]).float().double(), x.amax(1), first_argmax(x, 1)


def mlp64(pooled, w1, w2, host=0):
    """-> (hidden, its bound, ca, its bound)"""
    C, Ch = w1.shape[1], w1.shape[0]
    p64, W1, W2 = pooled.double(), w1.double(), w2.double()
    pre = p64 @ W1.t()                                        # [N, 2, Ch]
    pre_abs = p64.abs() @ W1.abs().t()
    # hidden: C / 64 fp32 products per lane, then a 64-lane tree: C / 64 + 8 roundings of the sum of |terms|
    e_h = (C / 64 * (1 + host) + 8) * EPS * pre_abs
    h = torch.relu(pre)
    logit = (h[:, 0] + h[:, 1]) @ W2.t()
    # ca: two Ch-term fp32 sums and their sum, the hidden errors through |W2|; sigmoid' <= 1/4, expf and the division
    e_logit = (Ch * (1 + host) + 4) * EPS * ((h[:, 0] + h[:, 1]) @ W2.abs().t()) + (e_h[:, 0] + e_h[:, 1]) @ W2.abs().t()
    return h, e_h, torch.sigmoid(logit), 0.25 * e_logit + 8 * EPS


def spatial_stats64(x, ca):
    """x [N, HW, C], ca [N, C] with x * ca and its channel sums exact in fp32 -> (mean, its bound, max, first arg-max)"""
    v = x.double() * ca.double()[:, None, :]
    mean = v.sum(2) / x.shape[2]
    # the sum is exact (multiples of 1/8 below 2^12); times fp32(1 / C): two roundings
    return mean, 3 * EPS * mean.abs(), v.amax(2), first_argmax(v, 2)


def sa64(smap, wsp, N, Hh, Ww, host=0):
    """-> (sa [N, Hh, Ww], its bound)"""
    s = smap.view(N, Hh, Ww, 2).permute(0, 3, 1, 2).double()
    pre = F.conv2d(s, wsp.double().view(1, 2, 7, 7), padding=3)[:, 0]
    terms = F.conv2d(s.abs(), wsp.double().abs().view(1, 2, 7, 7), padding=3)[:, 0]
    # 98 products summed in one fp32 chain (ky, kx, channel order); sigmoid' <= 1/4; expf and the division
    return torch.sigmoid(pre), 0.25 * (100 + 98 * host) * EPS * terms + 8 * EPS


def scale_f32(x, ca, sa, N, Hh, Ww):
    """out = (x * ca) * sa, two roundings in that order: the same two fp32 products (x [N, Hh, Ww, C], the kernel's own sa)"""
    return x * ca.view(N, 1, 1, -1) * sa.view(N, Hh, Ww, 1)


# ------------------------------------------------------------------------------------------------ backward
def bwd_a64(g, x, ca, sa):
    """g, x [N, HW, C], ca [N, C], sa [N, HW] -> (gsa_pre, its bound)"""
    C = x.shape[2]
    t = g.double() * x.double() * ca.double()[:, None, :]
    s64, a = sa.double(), t.sum(2)
    # two products per term, C / 32 per lane, the quad and the 8-lane tree, then two products: relative to sum |terms|
    e = ((C / 32 + 10) * EPS * t.abs().sum(2)) * s64 * (1 - s64) + 3 * EPS * (a * s64 * (1 - s64)).abs()
    return a * s64 * (1 - s64), e


def bwd_b64(gsa, smap, wsp, N, Hh, Ww, host=0):
    """-> (gsmap [N, Hh, Ww, 2], its bound, d-wsp [98], its bound): float64 autograd of F.conv2d(smap, wsp, padding=3)"""
    s = smap.view(N, Hh, Ww, 2).permute(0, 3, 1, 2).double().requires_grad_(True)
    w = wsp.double().view(1, 2, 7, 7).requires_grad_(True)
    F.conv2d(s, w, padding=3).backward(gsa.double().view(N, 1, Hh, Ww))
    # gsmap: up to 49 products in one fp32 chain; relative to the sum of |terms|
    ta = F.conv_transpose2d(gsa.double().abs().view(N, 1, Hh, Ww), w.detach().abs(), padding=3)
    # d-wsp: the product, a 64-lane tree, four waves, fp64 over the blocks: 10 roundings of the sum of |terms|
    tw = torch.nn.grad.conv2d_weight(s.detach().abs(), (1, 2, 7, 7), gsa.double().abs().view(N, 1, Hh, Ww), padding=3)
    return (s.grad.permute(0, 2, 3, 1), (52 + 49 * host) * EPS * ta.permute(0, 2, 3, 1), w.grad.flatten(),
            12 * EPS * tw.flatten())


def bwd_c64(g, x, sa, gsmap, cidx):
    """g, x [N, HW, C]; sa [N, HW]; gsmap [N, HW, 2]; cidx [N, HW] -> (gca [N, C] summed over the blocks, its bound)"""
    C = x.shape[2]
    onehot = F.one_hot(cidx.long(), C).double()
    gm, gx = gsmap[..., 0:1].double(), gsmap[..., 1:2].double()
    gx1 = g.double() * sa.double()[..., None] + gm / C + gx * onehot
    t = gx1 * x.double()
    ta = (g.double() * sa.double()[..., None]).abs() + gm.abs() / C + gx.abs() * onehot
    # gx1 takes 3 roundings, the product 1; per thread <= 512 / R pixels, then R rows: <= 513 + 4 deep
    return t.sum(1), 520 * EPS * (ta * x.double().abs()).sum(1)


def bwd_d64(gcap, ca, pooled, hidden, w1, w2, host=0):
    """gcap [N, nblk, C] -> ((gpool, d-W1, d-W2), the same sums over |terms|, k): float64 autograd of the MLP with the forward's
    hidden ReLU decisions (a unit whose pre-activation is exactly 0 passes no gradient, like torch's ReLU); bound = k * terms"""
    N, C, Ch = ca.shape[0], w1.shape[1], w1.shape[0]

    def ref(sign):
        """sign = identity: the gradients; abs: the same sums over |terms| (the error scale)"""
        p = sign(pooled.double()).requires_grad_(True)
        W1 = sign(w1.double()).requires_grad_(True)
        W2 = sign(w2.double()).requires_grad_(True)
        a = ca.double()
        gpre = sign(gcap.double().sum(1) * a * (1 - a))
        mask = (hidden > 0).double()
        h = (p @ W1.t()) * mask
        ((h[:, 0] + h[:, 1]) @ W2.t() * gpre).sum().backward()
        return p.grad, W1.grad, W2.grad

    # gpre: fp64 over the partials, then two products; the hidden gradient: C / 64 products per lane and a 64-lane tree;
    # gpool: Ch products; the weight gradients: N products per element
    k = (C / 64 + 2 * Ch + 2 * N + 16 + host * (C / 64 + Ch + 2 * N)) * EPS
    return ref(lambda t: t), ref(torch.abs), k


def bwd_e64(g, ca, sa, gsmap, cidx, gpool, amax):
    """g [N, HW, C] -> (gx, its bound): gx = (g sa + gmean / C + gmax [c == cidx]) ca + gavg / HW + gpmax [p == amax_idx]"""
    N, HW, C = g.shape
    onehot_c = F.one_hot(cidx.long(), C).double()                                        # [N, HW, C]
    onehot_p = F.one_hot(amax.long(), HW).double().permute(0, 2, 1)                       # [N, HW, C]
    gm, gxs = gsmap[..., 0:1].double(), gsmap[..., 1:2].double()
    a = ca.double()[:, None, :]
    gx1 = g.double() * sa.double()[..., None] + gm / C + gxs * onehot_c
    gavg, gmax = gpool[:, 0].double()[:, None, :], gpool[:, 1].double()[:, None, :]
    want = gx1 * a + gavg / HW + gmax * onehot_p
    terms = ((g.double() * sa.double()[..., None]).abs() + gm.abs() / C + gxs.abs() * onehot_c) * a + \
        gavg.abs() / HW + gmax.abs() * onehot_p
    # gx1 three roundings, the product by ca and the two sums: 8 EPS of the terms (a misplaced max gradient is a whole
    # term of up to 8 sqrt(HW) off)
    return want, 8 * EPS * terms
