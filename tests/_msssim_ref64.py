"""Float64 reference of the Gaussian-window SSIM and of MS-SSIM (csrc/msssim.hip): the definitions restated with
F.conv2d and F.avg_pool2d, the closed-form gradient of one level next to autograd, the chain across the levels, and the
magnitudes of the terms that the error bounds of the tests are stated in.  CPU only; every function takes and returns float64
(fp32 inputs are converted exactly).

  g[i] = exp(-(i-5)^2 / (2 * 1.5^2)), i = 0..10, normalised to sum 1; G = g (x) g; "valid" filtering
  per plane: mx = G*x, my = G*y, mxx = G*(x x), myy = G*(y y), mxy = G*(x y); C1 = (0.01 R)^2, C2 = (0.03 R)^2
  D1 = mx^2 + my^2 + C1, D2 = (mxx - mx^2) + (myy - my^2) + C2, l = (2 mx my + C1) / D1, cs = (2 (mxy - mx my) + C2) / D2
  SSIM[n,c] = mean(l cs), CS[n,c] = mean(cs); ssim_gaussian[n] = mean_c SSIM[n,c]
  MS-SSIM: level s+1 = avg_pool2d(level s, 2); V_s = CS_s for s < L-1, V_{L-1} = SSIM_{L-1}; M[n,c] = prod_s max(V_s, 0)^beta_s;
  ms_ssim[n] = mean_c M[n,c]"""
import torch
import torch.nn.functional as F

WIN = 11
MS_SSIM_WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)
U53 = 2.0 ** -53

# ---- the error budget, in units u = 2^-53 of the |terms| below.  M = 1.1 R bounds |pixel| over the tests' inputs.
#   a moment (two 11-tap passes of fused multiply-adds, the product under it, the weights: exp, an 11-term sum and a division,
#     which the kernel and this file each do their own way, so they enter twice per pass): (12 + 11 + 4 * 13) = 75, with the
#     one rounding of a pooled level's pixel 77: <= 80 u of the moment of absolute values
#   D1 = mx^2 + my^2 + C1: d(mx^2) <= 160 u a|x| |mx|, and a|x| |mx| / (mx^2 + C1) <= M / (2 sqrt C1) = 55: k1 = 2 * 160 * 55 =
#     17,600 u of D1 itself
#   D2 = (mxx - mx^2) + (myy - my^2) + C2: each variance cancels, d <= (80 a(xx) + 160 a|x|^2) u <= 240 M^2 u, and D2 >= C2 = 9e-4 R^2:
#     k2 = 2 * 240 * 1.21 / 9e-4 = 645,400 u of D2 itself -- the conditioning the float64 statistics are there to pay for
#   forward, l cs: 160 (numerator of l) + k1 + 162 (numerator of cs) + k2 + the two divisions and the product: 663,200 u of lb csb;
#     the tile tree (8 levels), the per-plane sum and the 1 / (OH OW): < 100 more.  The reference sums 121 terms per moment with
#     F.conv2d, so its own k2 is 2 * (121 * 3) * 1.21 / 9e-4 = 976,000 u: together 1,640,000 <= 2^21.
#   backward, the worst term B = -(a l + b) (2 (mxy - mx my) + C2) / D2^2: 160 + k1 + 162 + 2 k2 + six operations = 1,308,800 u; the
#     two transposed passes 75, the combination with x and y, 1 / (OH OW) and the pool adjoint 10: 1,308,900 u.  The reference
#     (autograd through the same denominators, 121-term sums) is granted 1.5 times as much: 3,272,000 <= 2^22.
# An fp32 accumulation anywhere behind the loads would cost 2^-24 of the terms = 2^8 / 2^7 times these bounds.
FWD_UNITS = 2.0 ** 21
BWD_UNITS = 2.0 ** 22


def window():
    i = torch.arange(WIN, dtype=torch.float64)
    g = torch.exp(-((i - WIN // 2) ** 2) / (2.0 * 1.5 ** 2))
    return g / g.sum()


def _G():
    g = window()
    return (g[:, None] * g[None, :]).view(1, 1, WIN, WIN)


def filt(z):
    """G * z, valid, per plane: [N,C,H,W] -> [N,C,H-10,W-10]"""
    N, C, H, W = z.shape
    return F.conv2d(z.reshape(N * C, 1, H, W), _G()).view(N, C, H - WIN + 1, W - WIN + 1)


def filt_t(z):
    """G^T * z, the transposed ("full") filter: [N,C,h,w] -> [N,C,h+10,w+10]"""
    N, C, h, w = z.shape
    return F.conv_transpose2d(z.reshape(N * C, 1, h, w), _G()).view(N, C, h + WIN - 1, w + WIN - 1)


def consts(data_range):
    return (0.01 * data_range) ** 2, (0.03 * data_range) ** 2


def maps(x, y, data_range=1.0):
    """(l, cs) maps [N,C,OH,OW] of two float64 batches; differentiable"""
    C1, C2 = consts(data_range)
    mx, my = filt(x), filt(y)
    mxx, myy, mxy = filt(x * x), filt(y * y), filt(x * y)
    D1 = mx * mx + my * my + C1
    D2 = (mxx - mx * mx) + (myy - my * my) + C2
    return (2 * mx * my + C1) / D1, (2 * (mxy - mx * my) + C2) / D2


def level_stats(x, y, data_range=1.0):
    """(SSIM [N,C], CS [N,C])"""
    l, cs = maps(x.double(), y.double(), data_range)
    return (l * cs).flatten(2).mean(2), cs.flatten(2).mean(2)


def level_terms(x, y, data_range=1.0):
    """(T_ssim [N,C], T_cs [N,C]): SSIM and CS with every moment replaced by the moment of absolute values and every numerator by
    the sum of its absolute terms; the denominators keep their values (their conditioning is in FWD_UNITS)."""
    x, y = x.double(), y.double()
    C1, C2 = consts(data_range)
    mx, my = filt(x), filt(y)
    D1 = mx * mx + my * my + C1
    D2 = (filt(x * x) - mx * mx) + (filt(y * y) - my * my) + C2
    ax, ay, axy = filt(x.abs()), filt(y.abs()), filt((x * y).abs())
    lb, csb = (2 * ax * ay + C1) / D1, (2 * (axy + ax * ay) + C2) / D2
    return (lb * csb).flatten(2).mean(2), csb.flatten(2).mean(2)


def ssim_gaussian(pred, target, data_range=1.0):
    """[N]: the mean over the planes of SSIM[n,c]"""
    return level_stats(pred, target, data_range)[0].mean(1)


def pool(z):
    return F.avg_pool2d(z, 2)


def min_side(levels):
    return WIN * 2 ** (levels - 1)


def pyramid_values(pred, target, data_range=1.0, levels=5):
    """V [L,N,C] (CS of the levels but the last, SSIM of the last) and the level images; differentiable in pred"""
    x, y = pred, target
    V, imgs = [], []
    for s in range(levels):
        imgs.append((x, y))
        l, cs = maps(x, y, data_range)
        V.append((cs if s < levels - 1 else l * cs).flatten(2).mean(2))
        if s < levels - 1:
            x, y = pool(x), pool(y)
    return torch.stack(V), imgs


def combine(V, weights):
    """ms_ssim [N] from V [L,N,C]: mean_c prod_s max(V_s, 0)^beta_s"""
    beta = torch.tensor(weights, dtype=torch.float64).view(-1, 1, 1)
    pos = (V > 0).all(0)
    # a plane with a factor <= 0 is exactly 0 with the gradient exactly 0 (max(v, 0)^beta has none at 0): masked, not left to
    # autograd, which would form 0 * inf there
    M = (torch.where(pos.expand_as(V), V, torch.ones_like(V)) ** beta).prod(0)
    return torch.where(pos, M, torch.zeros_like(M)).mean(1)


def ms_ssim(pred, target, data_range=1.0, weights=MS_SSIM_WEIGHTS):
    """[N] float64"""
    V, _ = pyramid_values(pred.double(), target.double(), data_range, len(weights))
    return combine(V, weights)


def level_closed_form(x, y, a, b, data_range=1.0, g_coarse=None):
    """(gradient, sum of |terms|), both [N,C,H,W], of sum_{n,c} a[n,c] SSIM[n,c] + b[n,c] CS[n,c] with respect to x, plus a quarter of
    g_coarse [N,C,H/2,W/2] at every pixel of its 2x2 block (the terms then carry a quarter of |g_coarse| too)."""
    x, y = x.double(), y.double()
    N, C, H, W = x.shape
    a, b = (torch.as_tensor(v, dtype=torch.float64).view(N, C, 1, 1) for v in (a, b))
    C1, C2 = consts(data_range)
    mx, my = filt(x), filt(y)
    mxx, myy, mxy = filt(x * x), filt(y * y), filt(x * y)
    D1 = mx * mx + my * my + C1
    D2 = (mxx - mx * mx) + (myy - my * my) + C2
    l, cs = (2 * mx * my + C1) / D1, (2 * (mxy - mx * my) + C2) / D2
    dl, dcs = (2 * my - 2 * mx * l) / D1, (-2 * my + 2 * mx * cs) / D2
    A = a * (cs * dl + l * dcs) + b * dcs
    w = a * l + b
    B, Cc = -w * cs / D2, 2 * w / D2
    cnt = float((H - WIN + 1) * (W - WIN + 1))
    grad = (filt_t(A) + 2 * x * filt_t(B) + y * filt_t(Cc)) / cnt
    ax, ay, axy = filt(x.abs()), filt(y.abs()), filt((x * y).abs())
    lb, csb = (2 * ax * ay + C1) / D1, (2 * (axy + ax * ay) + C2) / D2
    dlb, dcsb = (2 * ay + 2 * ax * lb) / D1, (2 * ay + 2 * ax * csb) / D2
    wb = a.abs() * lb + b.abs()
    Ab = a.abs() * (csb * dlb + lb * dcsb) + b.abs() * dcsb
    terms = (filt_t(Ab) + 2 * x.abs() * filt_t(wb * csb / D2) + y.abs() * filt_t(2 * wb / D2)) / cnt
    if g_coarse is not None:
        up = torch.zeros_like(x)
        PH, PW = H // 2, W // 2
        up[:, :, :2 * PH, :2 * PW] = 0.25 * g_coarse.double().repeat_interleave(2, 2).repeat_interleave(2, 3)
        grad, terms = grad + up, terms + up.abs()
    return grad, terms


def level_autograd(x, y, a, b, data_range=1.0):
    """the same gradient (without g_coarse) by autograd"""
    leaf = x.double().clone().requires_grad_(True)
    S, CS = level_stats(leaf, y.double(), data_range)
    N, C = S.shape
    (S * torch.as_tensor(a, dtype=torch.float64).view(N, C) + CS * torch.as_tensor(b, dtype=torch.float64).view(N, C)).sum().backward()
    return leaf.grad


def coefficients(V, weights, g_up):
    """d sum_n g_up[n] ms_ssim[n] / d V_s [L,N,C]: g_up beta_s M / (3 V_s) where every factor of the plane is > 0, else exactly 0"""
    beta = torch.tensor(weights, dtype=torch.float64).view(-1, 1, 1)
    pos = (V > 0).all(0, keepdim=True)
    M = (V.clamp_min(0) ** beta).prod(0, keepdim=True)
    safe = torch.where(pos, V, torch.ones_like(V))
    d = torch.as_tensor(g_up, dtype=torch.float64).view(1, -1, 1) * beta * M / (V.shape[2] * safe)
    return torch.where(pos, d, torch.zeros_like(d))


def ms_ssim_closed_form(pred, target, g_up, data_range=1.0, weights=MS_SSIM_WEIGHTS, rel=None):
    """(ms_ssim [N], gradient [N,C,H,W], sum of |terms| [N,C,H,W]) of sum_n g_up[n] ms_ssim[n] by the chain the kernels walk: the
    coefficients from V, then from the coarsest level up one closed-form level each with the coarser gradient folded in.
    `rel` [N,C] (optional): the relative error granted to the coefficients; it scales every level's own terms by (1 + rel / unit)
    -- see pyramid_bounds."""
    L = len(weights)
    V, imgs = pyramid_values(pred.double(), target.double(), data_range, L)
    d = coefficients(V, weights, g_up)
    grad = terms = None
    zero = torch.zeros_like(d[0])
    for s in reversed(range(L)):
        x, y = imgs[s]
        a, b = (d[s], zero) if s == L - 1 else (zero, d[s])
        g, t = level_closed_form(x, y, a, b, data_range)
        if rel is not None:
            t = t * rel.view(*rel.shape, 1, 1)
        if grad is not None:
            gc, tc = level_closed_form(x, y, zero, zero, data_range, grad)[0], level_closed_form(x, y, zero, zero, data_range, terms)[0]
            g, t = g + gc, t + tc
        grad, terms = g, t
    return combine(V, weights), grad, terms


def ms_ssim_autograd(pred, target, g_up, data_range=1.0, weights=MS_SSIM_WEIGHTS):
    """(ms_ssim [N], gradient) by autograd through the definitions"""
    leaf = pred.double().clone().requires_grad_(True)
    val = ms_ssim(leaf, target, data_range, weights)
    (val * torch.as_tensor(g_up, dtype=torch.float64)).sum().backward()
    return val.detach(), leaf.grad


def pyramid_bounds(pred, target, g_up, data_range=1.0, weights=MS_SSIM_WEIGHTS):
    """(value bound [N], gradient bound [N,C,H,W]) for the fp32 results of the pyramid, without their EPS |ref| for the one fp32
    store.  V_s carries FWD_UNITS u T_s.  M = prod V_s^beta_s then carries, relative to itself, r = sum_s beta_s FWD_UNITS u T_s / V_s +
    16 L u (pow and the product); the value bound is mean_c M r.  A coefficient beta_s M / (3 V_s) carries r + FWD_UNITS u T_s / V_s + 4 u
    relative to itself, at most rho = r + max_s(...) + 4 u; a level's own gradient terms scale with its coefficient, so they enter
    with BWD_UNITS u + rho.  Planes with a factor <= 0 have the value 0 and the gradient 0, exactly (bound 0)."""
    L = len(weights)
    V, imgs = pyramid_values(pred.double(), target.double(), data_range, L)
    T = torch.stack([level_terms(x, y, data_range)[0 if s == L - 1 else 1] for s, (x, y) in enumerate(imgs)])
    beta = torch.tensor(weights, dtype=torch.float64).view(-1, 1, 1)
    pos = (V > 0).all(0)
    relV = torch.where(pos.expand_as(V), FWD_UNITS * U53 * T / V.clamp_min(1e-300), torch.zeros_like(V))
    r = (beta * relV).sum(0) + 16 * L * U53
    M = (V.clamp_min(0) ** beta).prod(0)
    vbound = (M * r * pos).mean(1)
    rho = r + relV.max(0).values + 4 * U53
    _, _, gterms = ms_ssim_closed_form(pred, target, g_up, data_range, weights, rel=BWD_UNITS * U53 + rho)
    return vbound, gterms, V
