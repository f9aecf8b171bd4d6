"""Float64 restatements of the operations behind csrc/train_io.hip, csrc/detect.hip and csrc/lpips.hip, written from the
operations' definitions (numpy / torchvision / lpips / torch.optim semantics), not from the kernels.  Inputs are the fp32
tensors a kernel receives; everything is promoted to float64 first, so a result is the exact operation on those inputs
up to float64 rounding.  tests/test_ref64_cpu.py checks each function against oracle.ref_cpu on small inputs; the GPU
tests compare the kernels with these, and so do the host-emulation tests of the same sources (tests/test_lpips_hostemu_cpu.py,
tests/test_detect_hostemu_cpu.py); the error bounds of the LPIPS distance kernels, in EPS = 2^-24 relative to the sum of |terms|
added, are at the end of the file for both to share.  All functions run on whatever device their inputs live on."""
import math

import numpy as np
import torch
import torch.nn.functional as F

BBOX_XFORM_CLIP = math.log(1000.0 / 16)


def _d(x):
    return torch.as_tensor(x).double()


# ------------------------------------------------------------------------------------------------ train_io
def fog(clear, beta, airlight):
    """I = J t + A (1 - t), t = exp(-beta depth), depth = 0.3 + 0.7 sqrt((x - .5)^2 + (y - .2)^2) on np.linspace grids,
    BEFORE the rounding to float32 and the clip (the caller applies both)."""
    N, _, Hh, Ww = clear.shape
    xs = torch.from_numpy(np.linspace(0, 1, Ww)).to(clear.device)
    ys = torch.from_numpy(np.linspace(0, 1, Hh)).to(clear.device)
    depth = 0.3 + 0.7 * torch.sqrt((xs[None, :] - 0.5) ** 2 + (ys[:, None] - 0.2) ** 2)
    t = torch.exp(-_d(beta).view(N, 1, 1, 1) * depth)
    return _d(clear) * t + _d(airlight).view(N, 1, 1, 1) * (1 - t)


def mse(pred, target):
    """float64 mean of the squared EXACT difference per image: [N, per] -> [N]."""
    d = _d(target) - _d(pred)
    return (d * d).flatten(1).mean(1)


def psnr(pred, target, data_range=1.0):
    return 10.0 * torch.log10(data_range ** 2 / mse(pred, target))


def ssim_gray(pred, target, data_range=1.0):
    """skimage structural_similarity defaults on the channel-mean grayscale (np.mean(axis=2) of a float32 image:
    ((c0 + c1) + c2) / 3 in float32), each 7 x 7 window's statistics in float64, mean of S over the valid windows."""
    def gray(x):
        return ((x[:, 0] + x[:, 1]) + x[:, 2]) / torch.tensor(3.0, dtype=x.dtype, device=x.device)
    a, b = gray(target.float()).double()[:, None], gray(pred.float()).double()[:, None]      # im1 = target, im2 = pred

    def win(x):
        return F.avg_pool2d(x, 7, 1)
    ux, uy = win(a), win(b)
    cn = 49.0 / 48.0
    vx, vy, vxy = cn * (win(a * a) - ux * ux), cn * (win(b * b) - uy * uy), cn * (win(a * b) - ux * uy)
    C1, C2 = (0.01 * data_range) ** 2, (0.03 * data_range) ** 2
    S = ((2 * ux * uy + C1) * (2 * vxy + C2)) / ((ux * ux + uy * uy + C1) * (vx + vy + C2))
    return S.flatten(1).mean(1)


def paired_augment(x, params):
    """torchvision RandomHorizontalFlip / RandomVerticalFlip / ColorJitter(brightness, contrast) on float images:
    brightness = clamp(b x, 0, 1); contrast = clamp(c x + (1 - c) mean(gray(x)), 0, 1), gray of the image the contrast
    step RECEIVES (clamped only if brightness ran before it).  params[n] = (flip_h, flip_v, brightness_first, b, c).
    Returns (out, mean(|gray terms|) per image) -- the latter for error bounds."""
    out, gabs = [], []
    for n in range(x.shape[0]):
        fh, fv, bfirst, b, c = [float(v) for v in params[n]]
        img = _d(x[n])
        if fh:
            img = img.flip(-1)
        if fv:
            img = img.flip(-2)

        def bright(t):
            return (b * t).clamp(0, 1)

        def contrast(t):
            gabs.append((0.2989 * t[0].abs() + 0.587 * t[1].abs() + 0.114 * t[2].abs()).mean())
            return (c * t + (1.0 - c) * (0.2989 * t[0] + 0.587 * t[1] + 0.114 * t[2]).mean()).clamp(0, 1)
        out.append(contrast(bright(img)) if bfirst else bright(contrast(img)))
    return torch.stack(out), torch.stack(gabs)


def adam(p, g, m, v, step, repeats, dup_mode, lr, beta1, beta2, eps, wd, gscale, pow_units=0.0):
    """One optimizer.step() of torch.optim.Adam on a parameter listed `repeats` times, `step` = count before the call.
    dup_mode 0 (single-tensor loop): `repeats` consecutive full updates.  dup_mode 1 (foreach, duplicates alias): weight
    decay from the original p, m lerped `repeats` times, v *= beta2 `repeats` times then += (1 - beta2) g^2 `repeats`
    times, ONE bias correction at step + repeats, `repeats` identical subtractions.  All arguments as float64 of the fp32
    values the kernel receives.  Returns (p, m, v) and, alongside, first-order fp32 forward-error bounds (ep, em, ev) of an
    implementation that does each arithmetic operation once in fp32 (EPS per operation, relative to its result) and whose
    beta^t carries `pow_units` EPS of relative error."""
    E = 2.0 ** -24
    p, g, m, v = _d(p).clone(), _d(g) * gscale, _d(m).clone(), _d(v).clone()
    ep, em, ev = torch.zeros_like(p), torch.zeros_like(p), torch.zeros_like(p)

    def bias(t):
        b1t, b2t = beta1 ** t, beta2 ** t
        bc1, bc2sq = 1 - b1t, 1 - b2t
        r1 = (pow_units * b1t / bc1 + 1) * E                       # relative error of 1 - beta1^t
        r2 = 0.5 * (pow_units * b2t / bc2sq + 1) * E + E           # ... of sqrt(1 - beta2^t)
        return bc1, math.sqrt(bc2sq), r1, r2

    def apply(t, times):
        nonlocal p, ep
        bc1, bc2, r1, r2 = bias(t)
        s = v.sqrt()
        es = torch.where(s > 0, ev / (2 * s.clamp_min(1e-300)), ev.sqrt()) + E * s
        den = s / bc2 + eps
        eden = es / bc2 + (s / bc2) * (r2 + E) + E * den
        upd = (lr / bc1) * (m / den)
        eupd = upd.abs() * (r1 + 3 * E) + (lr / bc1) * (em / den + m.abs() * eden / den ** 2)
        for _ in range(times):
            p = p - upd
            ep = ep + eupd + E * p.abs()

    if dup_mode == 0 or repeats == 1:
        for r in range(repeats):
            gv = g + wd * p
            eg = 2 * E * (g.abs() + (wd * p).abs()) + wd * ep
            m_new = beta1 * m + (1 - beta1) * gv
            em = beta1 * em + 3 * E * ((beta1 * m).abs() + ((1 - beta1) * gv).abs()) + (1 - beta1) * eg
            m = m_new
            ev = beta2 * ev + 3 * E * (beta2 * v + (1 - beta2) * gv * gv) + 2 * (1 - beta2) * gv.abs() * eg
            v = beta2 * v + (1 - beta2) * gv * gv
            apply(step + r + 1, 1)
    else:
        gv = g + wd * p
        eg = 2 * E * (g.abs() + (wd * p).abs())
        for _ in range(repeats):
            em = beta1 * em + 3 * E * (m.abs() + gv.abs()) * (1 - beta1) + E * m.abs() + (1 - beta1) * eg
            m = m + (gv - m) * (1 - beta1)
        for _ in range(repeats):
            ev = beta2 * ev + E * v
            v = v * beta2
        for _ in range(repeats):
            ev = ev + 3 * E * ((1 - beta2) * gv * gv) + E * v + 2 * (1 - beta2) * gv.abs() * eg
            v = v + (1 - beta2) * gv * gv
        apply(step + repeats, repeats)
    return (p, m, v), (ep, em, ev)


# ---- the bounds and cases tests/test_gpu_train_io.py and tests/test_train_io_hostemu_cpu.py hold csrc/train_io.hip to
# float64 part of the fog kernel (x * (1 / (W - 1)) against linspace, sqrt, exp, six more operations, the exponent's
# condition number beta * depth <= 3 * 1.2): 64 units of 2^-53 by that count.  It cannot be measured through the fp32
# store, where it only shows as a flipped rounding: measured 0 (every element within half an fp32 ulp), bound 64.
FOG_F64_UNITS = 64
# float64 log10 and the float64 sums: not observable through the fp32 store of the results; the sums are of at most
# per / (1024 * 256) serial terms per thread plus a 20-level tree: 128 units of 2^-53 cover them.  measured 2 (the vector
# and the scalar path's float64 sums of the same data differ by at most 2 units; 2^-50 = 8 is asserted by the tests), bound 128.
PSNR_F64_UNITS = 128
# powf(beta, t) of the bias corrections, in EPS relative to beta^t: measured 1, bound 4 (test_adam_bias_correction_powf of the GPU
# test prints it: 0.96 at worst over t = 1..128, 1000, 10000, 100001).  It matters because 1 - beta2^t amplifies it by
# beta2^t / (1 - beta2^t), ~1000 at t = 1: the first update is good to ~57 EPS, not to 1.
ADAM_POW_UNITS = 4
ADAM_KW = dict(lr=1e-3, beta1=float(np.float32(0.9)), beta2=float(np.float32(0.999)), eps=float(np.float32(1e-8)))
AUG_BC = [(0.9, 1.1), (1.1, 0.9), (1.05, 0.9), (1.0, 1.0)]


def aug_params(b, c):
    """all eight (flip_h, flip_v, brightness_first) combinations with one (b, c): params [8, 5]"""
    return torch.tensor([[i & 1, (i >> 1) & 1, (i >> 2) & 1, b, c] for i in range(8)], dtype=torch.float32)


def aug_bound(x, params, gabs):
    """fp32 forward error of brightness = clamp(b x) and contrast = clamp(c x + (1 - c) mean) in either order: one
    rounding for b x; for the contrast step the products c x and (1 - c) mean, the difference 1 - c and the sum (3 |c x| +
    4 |(1 - c) mean| roundings, FMA or not); the mean itself: fp32 grayscale (three coefficient roundings, three
    products, two sums: 6 EPS of mean |gray terms|), summed in float64.  The clamps are 1-Lipschitz."""
    E = 2.0 ** -24
    out = []
    for n in range(x.shape[0]):
        fh, fv, bfirst, b, c = [float(v) for v in params[n]]
        img = x[n].double()
        if fh:
            img = img.flip(-1)
        if fv:
            img = img.flip(-2)
        xin = (b * img).clamp(0, 1) if bfirst else img
        e_in = E * (b * img).abs() if bfirst else torch.zeros_like(img)
        mean = (0.2989 * xin[0] + 0.587 * xin[1] + 0.114 * xin[2]).mean()
        e = E * (3 * (c * xin).abs() + 4 * abs((1 - c) * mean)) + abs(1 - c) * 6 * E * gabs[n] + abs(c) * e_in
        if not bfirst:
            e = abs(b) * e + E * abs(b) * (c * xin + (1 - c) * mean).clamp(0, 1)
        out.append(e)
    return torch.stack(out)


# ------------------------------------------------------------------------------------------------ detect
def nearest_src(out_size, in_size):
    """source index of F.interpolate(mode='nearest'): min(floor(i * (in / out)), in - 1), the scale and the product in fp32."""
    scale = np.float32(in_size) / np.float32(out_size)
    i = np.arange(out_size, dtype=np.float32)
    return torch.from_numpy(np.minimum(np.floor(i * scale).astype(np.int64), in_size - 1))


def upsample_nearest_add(top, lat):
    """lat + nearest-upsampled top, NHWC."""
    iy = nearest_src(lat.shape[1], top.shape[1]).to(top.device)
    ix = nearest_src(lat.shape[2], top.shape[2]).to(top.device)
    return _d(lat) + _d(top)[:, iy][:, :, ix]


def decode_clip(deltas, boxes, weights, img_h, img_w):
    """BoxCoder(weights).decode_single + clip_boxes_to_image; deltas / boxes [..., 4], img_h / img_w broadcastable."""
    deltas, boxes = _d(deltas), _d(boxes)
    wx, wy, ww, wh = weights
    w, h = boxes[..., 2] - boxes[..., 0], boxes[..., 3] - boxes[..., 1]
    cx, cy = boxes[..., 0] + 0.5 * w, boxes[..., 1] + 0.5 * h
    dw = (deltas[..., 2] / ww).clamp(max=BBOX_XFORM_CLIP)
    dh = (deltas[..., 3] / wh).clamp(max=BBOX_XFORM_CLIP)
    pcx, pcy = deltas[..., 0] / wx * w + cx, deltas[..., 1] / wy * h + cy
    pw, ph = torch.exp(dw) * w, torch.exp(dh) * h
    zero = torch.zeros((), dtype=torch.float64, device=boxes.device)
    img_w, img_h = _d(img_w).to(boxes.device), _d(img_h).to(boxes.device)
    x1, x2 = (pcx - 0.5 * pw).maximum(zero).minimum(img_w), (pcx + 0.5 * pw).maximum(zero).minimum(img_w)
    y1, y2 = (pcy - 0.5 * ph).maximum(zero).minimum(img_h), (pcy + 0.5 * ph).maximum(zero).minimum(img_h)
    # error scale of one coordinate: the magnitudes the subtraction pcx -+ pw / 2 combines
    mag = torch.stack([pcx.abs() + 0.5 * pw + (deltas[..., 0] / wx * w).abs(), pcy.abs() + 0.5 * ph + (deltas[..., 1] / wy * h).abs()] * 2, -1)
    return torch.stack([x1, y1, x2, y2], -1), mag, torch.stack([pw, ph, pw, ph], -1)


def rpn_anchors(H, W, base, stride_h, stride_w):
    """AnchorGenerator.grid_anchors of one level: position major (y, x), anchor minor -> [H * W * A, 4]."""
    ys, xs = torch.arange(H, dtype=torch.float64) * stride_h, torch.arange(W, dtype=torch.float64) * stride_w
    yy, xx = torch.meshgrid(ys, xs, indexing="ij")
    shifts = torch.stack([xx, yy, xx, yy], -1).reshape(-1, 1, 4).to(base.device)
    return (shifts + _d(base)[None]).reshape(-1, 4)


def nms_sorted(boxes, groups, thr):
    """Greedy batched NMS over score-sorted boxes (numpy): keep[i] unless an earlier KEPT box of i's group has
    IoU > thr with it.  IoU = inter / (area_i + area_j - inter); 0 / 0 is NaN and NaN > thr is False (kept)."""
    b = np.asarray(boxes, dtype=np.float64)
    g = np.asarray(groups)
    M = b.shape[0]
    area = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    removed = np.zeros(M, dtype=bool)
    keep = np.zeros(M, dtype=np.int32)
    with np.errstate(invalid="ignore", divide="ignore"):
        for i in range(M):
            if removed[i]:
                continue
            keep[i] = 1
            r = b[i + 1:]
            iw = np.clip(np.minimum(b[i, 2], r[:, 2]) - np.maximum(b[i, 0], r[:, 0]), 0, None)
            ih = np.clip(np.minimum(b[i, 3], r[:, 3]) - np.maximum(b[i, 1], r[:, 1]), 0, None)
            inter = iw * ih
            iou = inter / (area[i] + area[i + 1:] - inter)
            removed[i + 1:] |= (iou > thr) & (g[i + 1:] == g[i])
    return keep


def fpn_level(rois, nlevels):
    """LevelMapper(k_min 2, k_max 5, canonical 224 / 4, eps 1e-6): (level index, float64 distance of the floor's argument
    to the nearest integer)."""
    r = _d(rois)
    s = torch.sqrt((r[:, 3] - r[:, 1]) * (r[:, 4] - r[:, 2]))
    t = 4 + torch.log2(s / 224) + 1e-6
    lvl = (torch.floor(t).clamp(2, 5) - 2).clamp(max=nlevels - 1)
    lvl = torch.where(torch.isnan(t), torch.zeros_like(lvl), lvl)
    return lvl.long(), (t - torch.round(t)).abs()


def roi_align(feat, rois, scale, out=7, ratio=2):
    """torchvision.ops.roi_align(aligned=False, sampling_ratio=2) on an NHWC level: feat [N, H, W, C], rois [R, 5]
    -> (pooled [R, C, out, out], sum of |weight * value| / (ratio^2) [R, C, out, out])."""
    feat, rois = _d(feat), _d(rois)
    N, Hh, Ww, C = feat.shape
    R = rois.shape[0]
    n = rois[:, 0].long()
    x1, y1 = rois[:, 1] * scale, rois[:, 2] * scale
    rw, rh = (rois[:, 3] * scale - x1).clamp(min=1.0), (rois[:, 4] * scale - y1).clamp(min=1.0)
    bw, bh = rw / out, rh / out
    k = torch.arange(out * ratio, dtype=torch.float64, device=feat.device)
    frac = (k // ratio) + ((k % ratio) + 0.5) / ratio                      # sample position in bins
    ys, xs = y1[:, None] + frac[None] * bh[:, None], x1[:, None] + frac[None] * bw[:, None]     # [R, out * ratio]

    def axis(c, size):
        ok = (c >= -1.0) & (c <= size)
        c = c.clamp(min=0.0)
        lo = c.floor().long()
        top = lo >= size - 1
        lo = torch.where(top, torch.full_like(lo, size - 1), lo)
        hi = torch.where(top, lo, lo + 1)
        c = torch.where(top, lo.double(), c)
        l = c - lo
        return ok, lo, hi, l, 1.0 - l
    oky, yl, yh, ly, hy = axis(ys, Hh)
    okx, xl, xh, lx, hx = axis(xs, Ww)
    acc = torch.zeros((R, out * ratio, out * ratio, C), dtype=torch.float64, device=feat.device)
    mag = torch.zeros_like(acc)
    nn = n[:, None, None]
    for yi, wy in ((yl, hy), (yh, ly)):
        for xi, wx in ((xl, hx), (xh, lx)):
            wgt = (wy[:, :, None] * wx[:, None, :])[..., None]
            val = feat[nn, yi[:, :, None], xi[:, None, :]]
            acc += wgt * val
            mag += wgt * val.abs()
    ok = (oky[:, :, None] & okx[:, None, :])[..., None]
    acc, mag = acc * ok, mag * ok

    def pool(t):
        return t.view(R, out, ratio, out, ratio, C).sum(dim=(2, 4)).permute(0, 3, 1, 2) / (ratio * ratio)
    return pool(acc), pool(mag)


def box_postprocess(logits, deltas, props, img_hw, img, thresh, min_size):
    """roi_heads.postprocess_detections up to the NMS: softmax scores, BoxCoder(10, 10, 5, 5) decode per class, clip,
    valid = score > thresh and w, h >= min_size; the background class 0 dropped.  logits [R, NC], deltas [R, NC, 4]."""
    sc = torch.softmax(_d(logits), -1)[:, 1:]
    hw = _d(img_hw)[img.long()]
    b, mag, wh = decode_clip(_d(deltas)[:, 1:], _d(props)[:, None, :], (10.0, 10.0, 5.0, 5.0), hw[:, 0, None], hw[:, 1, None])
    valid = (sc > thresh) & ((b[..., 2] - b[..., 0]) >= min_size) & ((b[..., 3] - b[..., 1]) >= min_size)
    return b, sc, valid, mag, wh


# ------------------------------------------------------------------------------------------------ lpips
def lpips_s2d(img, a3, b3, OHp, OWp):
    """The scaling layer x * a + b followed by the space-to-depth that turns conv1 (11 x 11, stride 4, pad 2) into a 3 x 3
    stride-1 convolution: out[n, r, q, (by * 4 + bx) * 3 + c] = scaled[n, c, 4 r + by - 2, 4 q + bx - 2], 0 outside."""
    N, _, Hh, Ww = img.shape
    a, b = _d(a3).to(img.device).view(1, 3, 1, 1), _d(b3).to(img.device).view(1, 3, 1, 1)
    s = _d(img) * a + b
    mag = (_d(img) * a).abs() + b.abs()

    def s2d(t):
        big = torch.zeros((N, 3, 4 * OHp, 4 * OWp), dtype=torch.float64, device=img.device)
        hh, ww = min(Hh, 4 * OHp - 2), min(Ww, 4 * OWp - 2)
        big[:, :, 2:2 + hh, 2:2 + ww] = t[:, :, :hh, :ww]
        return big.view(N, 3, OHp, 4, OWp, 4).permute(0, 2, 4, 3, 5, 1).reshape(N, OHp, OWp, 48)
    return s2d(s), s2d(mag)


def lpips_s2d_bwd(g, a3, Hh, Ww):
    """adjoint of lpips_s2d with respect to the image: g [N, OHp, OWp, 48] -> [N, 3, H, W]."""
    N, OHp, OWp, _ = g.shape
    big = _d(g).view(N, OHp, OWp, 4, 4, 3).permute(0, 5, 1, 3, 2, 4).reshape(N, 3, 4 * OHp, 4 * OWp)
    out = torch.zeros((N, 3, Hh, Ww), dtype=torch.float64, device=g.device)
    hh, ww = min(Hh, 4 * OHp - 2), min(Ww, 4 * OWp - 2)
    out[:, :, :hh, :ww] = big[:, :, 2:2 + hh, 2:2 + ww]
    return out * _d(a3).to(g.device).view(1, 3, 1, 1)


def lpips_pixel(fa, fb, w):
    """per pixel: sum_c w_c (a_c / (|a| + 1e-10) - b_c / (|b| + 1e-10))^2; fa, fb [N, HW, C] -> [N, HW]."""
    a, b = _d(fa), _d(fb)
    na = a / (a.pow(2).sum(-1, keepdim=True).sqrt() + 1e-10)
    nb = b / (b.pow(2).sum(-1, keepdim=True).sqrt() + 1e-10)
    return ((na - nb) ** 2 * _d(w)).sum(-1)


def lpips_layer_grad(fa, fb, w, g_val):
    """d / d fa of sum_n g_val[n] * mean_p lpips_pixel, closed form:
        delta = 2 w (na - nb) g / HW;  grad = delta / s - a (delta . a) / (r s^2),  r = |a|, s = r + 1e-10.
    CONVENTION at r = 0 (an all-zero pixel of fa, where sqrt is not differentiable and autograd gives NaN): the second
    term is dropped, i.e. the gradient is that of a / s with s held constant: grad = delta / 1e-10."""
    a, b, w = _d(fa), _d(fb), _d(w)
    HW = a.shape[1]
    r = a.pow(2).sum(-1, keepdim=True).sqrt()
    s = r + 1e-10
    na, nb = a / s, b / (b.pow(2).sum(-1, keepdim=True).sqrt() + 1e-10)
    delta = 2 * w * (na - nb) * (_d(g_val).view(-1, 1, 1) / HW)
    dot = (delta * a).sum(-1, keepdim=True)
    k2 = torch.where(r > 0, dot / (r.clamp_min(1e-300) * s * s), torch.zeros_like(r))
    return delta / s - a * k2


# ---- the bounds tests/test_gpu_lpips.py and tests/test_lpips_hostemu_cpu.py hold the distance kernels to; the comments name the
# fp32 operations behind each count.  (Every product and sum is counted apart, so a host build, which does not contract
# a * b + c, is held to the same figures.)
EPS = 2.0 ** -24


def lpips_features(N, HW, C_, randn, rand):
    """post-ReLU-like features: |randn| with ~30 % zeros; by pixel index (p + n) % 7: 1 -> fa all zero, 2 -> fb all zero,
    3 -> both all zero, 4 -> fa == fb, 5 -> one channel of fa dominant by 1e4.  randn / rand(k, *shape): the k-th draw.
    -> (fa, fb, w, the pixel classes [N, HW])"""
    def base(k):
        return randn(k, N, HW, C_).abs() * (rand(k + 1, N, HW, C_) > 0.3)
    fa, fb = base(0), base(2)
    fam = (torch.arange(HW, device=fa.device)[None, :] + torch.arange(N, device=fa.device)[:, None]) % 7
    fa[(fam == 1) | (fam == 3)] = 0.0
    fb[(fam == 2) | (fam == 3)] = 0.0
    fb[fam == 4] = fa[fam == 4]
    dom = fa[..., C_ // 2]
    dom[fam == 5] = 1e4
    w = rand(4, C_)
    return fa.contiguous(), fb.contiguous(), w, fam


def lpips_lane_terms(C_):
    """roundings of a C-channel sum as the kernels do it: four products summed pairwise per quad (3), C / 32 quads added
    serially per lane, a 3-level tree over the 8 lanes of the pixel group."""
    return -(-C_ // 32) + 6


def lpips_norm_terms(C_):
    """relative error of 1 / (sqrt(sum a^2) + 1e-10) in EPS: half the sum's, sqrtf, the fp32 constant and sum, the reciprocal."""
    return lpips_lane_terms(C_) / 2 + 3


def lpips_layer_blocks(fa, fb, w, ppb):
    """-> (per-pixel distance [N, HW], per-block sums [N, nblk], the bound of the per-block sums) for blocks of ppb pixels"""
    N, HW, C_ = fa.shape
    nblk = -(-HW // ppb)
    a, b, w64 = fa.double(), fb.double(), w.double()
    na = a / (a.pow(2).sum(-1, keepdim=True).sqrt() + 1e-10)
    nb = b / (b.pow(2).sum(-1, keepdim=True).sqrt() + 1e-10)
    dpix = lpips_pixel(fa, fb, w)                                                       # [N, HW]
    # per pixel: na and nb carry (norm + 1) EPS each, their difference one more; w df^2 doubles df's error and adds two
    # products; the channel sum of the terms: lpips_lane_terms
    kin = lpips_norm_terms(C_)
    e_df = EPS * ((kin + 1) * (na.abs() + nb.abs()) + (na - nb).abs())
    # (w e_df^2 is the second-order term: it is all there is where na == nb)
    e_pix = (w64 * (2 * (na - nb).abs() * e_df + e_df ** 2)).sum(-1) + (lpips_lane_terms(C_) + 2) * EPS * dpix
    # per block: 32 pixels added serially per thread, a 6-level wave tree, two more sums
    pad = nblk * ppb - HW
    blk = lambda t: F.pad(t, (0, pad)).view(N, nblk, ppb).sum(-1)
    return dpix, blk(dpix), blk(e_pix) + 40 * EPS * blk(dpix)


def lpips_layer_grad_bound(fa, fb, w, g_val, ref):
    """the bound of lpips_layer_grad's result `ref` as csrc/lpips.hip computes it"""
    N, HW, C_ = fa.shape
    a, b, w64 = fa.double(), fb.double(), w.double()
    r = a.pow(2).sum(-1, keepdim=True).sqrt()
    s = r + 1e-10
    na, nb = a / s, b / (b.pow(2).sum(-1, keepdim=True).sqrt() + 1e-10)
    kin, kl = lpips_norm_terms(C_), lpips_lane_terms(C_)
    gk = (g_val.double() / HW).view(-1, 1, 1)
    # delta = w (na - nb) (2 gk): the difference as in the forward, gk = g / HW (1), three products
    e_df = EPS * ((kin + 1) * (na.abs() + nb.abs()) + (na - nb).abs())
    dl = 2 * w64 * (na - nb) * gk
    e_dl = 2 * (w64 * gk).abs() * e_df + 4 * EPS * dl.abs()
    # dot = sum delta a: the terms' own errors, one product each and the channel sum
    dota = (dl * a).abs().sum(-1, keepdim=True)
    e_dot = (a.abs() * e_dl).sum(-1, keepdim=True) + (kl + 1) * EPS * dota
    # k2 = dot / (r s s): sqrtf's and the sum's error three times over, two products, one division
    den = (r * s * s).clamp_min(1e-300)
    pos = r > 0
    e_k2 = torch.where(pos, (e_dot + (3 * kin + 3) * EPS * dota) / den, torch.zeros_like(r))
    k2 = torch.where(pos, (dl * a).sum(-1, keepdim=True) / den, torch.zeros_like(r))
    # out = delta / s - a k2: 1 / s carries kin, two products, one difference
    return e_dl / s + (kin + 1) * EPS * (dl / s).abs() + a.abs() * e_k2 + 2 * EPS * (a * k2).abs() + EPS * ref.abs()


# ---- the bounds tests/test_gpu_detect_kernels.py and tests/test_detect_hostemu_cpu.py hold the detector kernels to
# expf of the box decodes (rpn_decode_kernel, box_postprocess_kernel), in EPS relative to its result: measured 1, bound 4
# (the GPU tests print "expf units needed": at most 0.57 beyond the plain roundings in the RPN decode, nothing beyond them in
# the box head, scores or boxes)
EXP_UNITS = 4


def rpn_decode_bounds(mag, pwh):
    """(the plain roundings, the whole bound) of adh_rpn_decode's boxes from decode_clip's magnitudes.
    Anchor width / centre are exact (small integers and halves).  pcx = d w + cx: two roundings (one with FMA) of
    |d w| + |pcx|; pw = expf(dw) w: expf and a product; the clamp constant log(1000 / 16) is fp32: half an ulp of 4.1 is
    4 EPS on the exponent, so 4 EPS of pw; pcx -+ pw / 2: one more rounding, of the result"""
    plain = EPS * 2 * mag
    return plain, plain + (EXP_UNITS + 6) * EPS * 0.5 * pwh


def roi_align_bound(rois, mag, scale, vmax):
    """rois [R, 5] of one level, mag from roi_align, vmax = max |feature| of the level.
    Per sample: hy = 1 - ly, the weight product, four products with the values and three sums (6 EPS of the sum of
    |weight * value|); four samples added (3) and the exact scale by 0.25; 12 with margin for the order.
    Sample coordinate: x2 s - x1 s, / 7, ph * bin, (i + .5) * bin / 2 and two sums: 6 roundings of at most
    |start| + extent; a coordinate error d moves a bilinear sample by at most d * 2 max|value| per axis."""
    rd = rois.double()
    ext = (rd[:, 1:3].abs().amax(1) + (rd[:, 3:5] - rd[:, 1:3]).abs().amax(1)) * scale + 1.0
    return 12 * EPS * mag + (6 * EPS * ext * 4 * vmax).view(-1, 1, 1, 1)


def box_postprocess_bounds(logits, rs, mag, pwh):
    """logits [R, NC]; rs, mag, pwh from box_postprocess -> (plain score roundings, score bound, plain box roundings, box bound).
    score = expf(l - m) / sum: l - m rounds once (EPS |l - m| on the exponent), expf, the NC-term sum of expf values
    (each its own expf error, ceil(NC / 64) serial additions per lane and a 6-level tree), one division; its own exponent
    roundings weigh in by the softmax-weighted mean of |l - m| <= ln NC.
    box: d / 10 and d / 5 round once each (the latter moves expf by EPS |dw| <= 4.2 EPS), then as in the RPN decode
    (product 1, fp32 clamp constant 4): 10 EPS of pw / 2 besides expf"""
    NC = logits.shape[1]
    lg = logits.double()
    dist = (lg.amax(1, keepdim=True) - lg)[:, 1:]
    plain_s = (dist + -(-NC // 64) + 8 + math.log(NC)) * EPS * rs + 1e-37
    plain_b = EPS * 3 * mag
    return plain_s, plain_s + 2 * EXP_UNITS * EPS * rs, plain_b, plain_b + (EXP_UNITS + 10) * EPS * 0.5 * pwh
