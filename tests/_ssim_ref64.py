"""Float64 reference of the SSIM loss term: the arithmetic of tests/_ref64.py::ssim_gray made differentiable in `pred`,
and the magnitude of the closed form's terms that the error bounds of tests/test_gpu_ssim_loss.py are
stated in.  CPU only."""
import torch
import torch.nn.functional as F

CN = 49.0 / 48.0


def _win(z):
    return F.avg_pool2d(z, 7, 1)


def _consts(data_range):
    return (0.01 * data_range) ** 2, (0.03 * data_range) ** 2


def ssim_from_gray(x, y, data_range=1.0):
    """Per-image SSIM [N] of two grayscale batches [N,1,H,W] (x from pred, y from target), skimage's defaults: the
    expressions of _ref64.ssim_gray in the dtype of x; differentiable."""
    C1, C2 = _consts(data_range)
    ux, uy = _win(y), _win(x)                                                # im1 = target, im2 = pred, as _ref64 has them
    vx, vy, vxy = CN * (_win(y * y) - ux * ux), CN * (_win(x * x) - uy * uy), CN * (_win(y * x) - ux * uy)
    S = ((2 * ux * uy + C1) * (2 * vxy + C2)) / ((ux * ux + uy * uy + C1) * (vx + vy + C2))
    return S.flatten(1).mean(1)


def gray(img):
    """channel mean as np.mean(axis=2) forms it, in the dtype of img: ((c0 + c1) + c2) / 3."""
    return (((img[:, 0] + img[:, 1]) + img[:, 2]) / torch.tensor(3.0, dtype=img.dtype))[:, None]


def ssim_of_images(pred, target, data_range=1.0):
    """Differentiable per-image SSIM [N] of two [N,3,H,W] batches, everything (the grayscale too) in pred's dtype: the
    loss an oracle network's output goes into."""
    return ssim_from_gray(gray(pred), gray(target.to(pred.dtype)), data_range)


def closed_form(pred, target, g, data_range=1.0):
    """(gradient [N,3,H,W], sum of |terms| [N,1,H,W]) of sum_n g[n] ssim[n] from the closed form, float64, on the fp32
    grayscale of the fp32 images `pred` / `target`.

    |terms|: every quantity that enters a product is replaced by what bounds its rounding error -- window means by the
    window means of absolute values (mx -> mean|x|, mxy -> mean|xy|), A1 = 2 mx my + C1 and A2 = 2 cn (mxy - mx my) + C2 by
    the sums of their absolute terms -- while the denominators B1 = mx^2 + my^2 + C1 and B2 = vx + vy + C2 keep their values
    (their conditioning is part of the factor K of the test); then the four terms of a, b and c enter with absolute
    values, and so do x[p] and y[p]."""
    N, _, H, W = pred.shape
    x, y = gray(pred.float()).double(), gray(target.float()).double()
    g = torch.as_tensor(g, dtype=torch.float64).view(N, 1, 1, 1)
    C1, C2 = _consts(data_range)
    mx, my = _win(x), _win(y)
    vx, vy, vxy = CN * (_win(x * x) - mx * mx), CN * (_win(y * y) - my * my), CN * (_win(x * y) - mx * my)
    A1, A2, B1, B2 = 2 * mx * my + C1, 2 * vxy + C2, mx * mx + my * my + C1, vx + vy + C2
    S = A1 * A2 / (B1 * B2)
    a = 2 * my * A2 / (B1 * B2) - 2 * mx * S / B1 + 2 * CN * mx * S / B2 - 2 * CN * my * A1 / (B1 * B2)
    b = -CN * S / B2
    c = 2 * CN * A1 / (B1 * B2)
    ones = torch.ones(1, 1, 7, 7, dtype=torch.float64)

    def box(z):                                                              # sum over the valid windows that contain p
        return F.conv_transpose2d(z, ones)
    scale = 1.0 / (3.0 * 49.0 * (H - 6) * (W - 6))
    grad = (g * scale * (box(a) + 2 * x * box(b) + y * box(c))).expand(N, 3, H, W)
    ax, ay, axy = _win(x.abs()), _win(y.abs()), _win((x * y).abs())
    A1b, A2b = 2 * ax * ay + C1, 2 * CN * (axy + ax * ay) + C2
    Sb = A1b * A2b / (B1 * B2)
    ab = 2 * ay * A2b / (B1 * B2) + 2 * ax * Sb / B1 + 2 * CN * ax * Sb / B2 + 2 * CN * ay * A1b / (B1 * B2)
    bb = CN * Sb / B2
    cb = 2 * CN * A1b / (B1 * B2)
    terms = g.abs() * scale * (box(ab) + 2 * x.abs() * box(bb) + y.abs() * box(cb))
    return grad, terms


def ssim_and_grad(pred, target, g, data_range=1.0):
    """((ssim [N], d sum_n g[n] ssim[n] / d pred [N,3,H,W]), sum of |terms| [N,1,H,W]), all float64 on the CPU.

    Value and gradient: torch autograd through the arithmetic of _ref64.ssim_gray with pred as a float64 leaf.  The
    grayscale the window statistics see is the fp32 one, ((c0 + c1) + c2) / 3 rounded as _ref64 and the kernels round it;
    its derivative is the exact 1/3 per channel."""
    pred, target = pred.detach().cpu().float(), target.detach().cpu().float()
    leaf = pred.double().requires_grad_(True)
    x64 = gray(leaf)
    x = x64 + (gray(pred).double() - x64).detach()                           # value: the fp32 gray; derivative: that of x64
    y = gray(target).double()
    val = ssim_from_gray(x, y, data_range)
    gv = torch.as_tensor(g, dtype=torch.float64).view(-1)
    (val * gv).sum().backward()
    _, terms = closed_form(pred, target, gv, data_range)
    return (val.detach(), leaf.grad), terms
