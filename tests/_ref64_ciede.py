"""CIEDE2000 in float64 numpy, written from the definition (Sharma, Wu and Dalal 2005, kL = kC = kH = 1), for
tests/test_ciede2000_ref_cpu.py, tests/test_gpu_ciede2000.py, tests/test_ciede2000_hostemu_cpu.py and
tests/test_gpu_demo_scores.py.  Nothing here knows the kernel: whole-array expressions, np.where for every branch.

    rgb2lab(rgb)            [..., 3] sRGB, any float dtype -> [..., 3] L, a, b (skimage's rgb2lab constants, inputs clamped to [0, 1],
                            NaN = 0)
    delta_e(lab1, lab2)     [..., 3] x 2 -> [...] dE00
    ciede2000(pred, target, lab_input=False)   [N,3,H,W] x 2 -> (map [N,H,W], mean [N]), float64
"""
import numpy as np

SHARMA_PAIRS = [  # (L, a, b), (L, a, b), dE00 to the table's four decimals
    ((50, 2.6772, -79.7751), (50, 0, -82.7485), 2.0425),
    ((50, 3.1571, -77.2803), (50, 0, -82.7485), 2.8615),
    ((50, 2.8361, -74.0200), (50, 0, -82.7485), 3.4412),
    ((50, -1.3802, -84.2814), (50, 0, -82.7485), 1.0000),
    ((50, -1.1848, -84.8006), (50, 0, -82.7485), 1.0000),
    ((50, -0.9009, -85.5211), (50, 0, -82.7485), 1.0000),
    ((50, 0, 0), (50, -1, 2), 2.3669),
    ((50, -1, 2), (50, 0, 0), 2.3669),
    ((50, 2.49, -0.001), (50, -2.49, 0.0009), 7.1792),
    ((50, 2.49, -0.001), (50, -2.49, 0.0011), 7.2195),
    ((50, 2.49, -0.001), (50, -2.49, 0.0012), 7.2195),
    ((50, -0.001, 2.49), (50, 0.0009, -2.49), 4.8045),
    ((50, -0.001, 2.49), (50, 0.0011, -2.49), 4.7461),
    ((50, 2.5, 0), (50, 0, -2.5), 4.3065),
]
# hues exactly 180 degrees apart: the branch hangs on the last bit of an arctangent.  Printed, never asserted.
KNIFE_EDGE_PAIRS = [((50, 2.49, -0.001), (50, -2.49, 0.0010)), ((50, -0.001, 2.49), (50, 0.0010, -2.49))]

SRGB_KNEE = 0.04045
LAB_KNEE = (6.0 / 29.0) ** 3
_M = np.array([[0.412453, 0.357580, 0.180423], [0.212671, 0.715160, 0.072169], [0.019334, 0.119193, 0.950227]])
_WHITE = np.array([0.95047, 1.0, 1.08883])


def rgb2lab(rgb):
    v = np.asarray(rgb).astype(np.float64)
    with np.errstate(invalid="ignore"):
        c = np.where(v > 0, np.minimum(v, 1.0), 0.0)                 # NaN > 0 is false
    lin = np.where(c <= SRGB_KNEE, c / 12.92, ((c + 0.055) / 1.055) ** 2.4)
    xyz = (lin[..., None, :] * _M).sum(-1) / _WHITE
    f = np.where(xyz > LAB_KNEE, np.cbrt(xyz), xyz / (3.0 * (6.0 / 29.0) ** 2) + 4.0 / 29.0)
    fx, fy, fz = f[..., 0], f[..., 1], f[..., 2]
    return np.stack([116.0 * fy - 16.0, 500.0 * (fx - fy), 200.0 * (fy - fz)], axis=-1)


def _hue(b, ap):
    h = np.degrees(np.arctan2(b, ap))
    h = np.where(h < 0, h + 360.0, h)
    return np.where((ap == 0) & (b == 0), 0.0, h)


def delta_e(lab1, lab2):
    lab1, lab2 = np.asarray(lab1, dtype=np.float64), np.asarray(lab2, dtype=np.float64)
    L1, a1, b1 = lab1[..., 0], lab1[..., 1], lab1[..., 2]
    L2, a2, b2 = lab2[..., 0], lab2[..., 1], lab2[..., 2]
    Cm = (np.hypot(a1, b1) + np.hypot(a2, b2)) / 2
    G = 0.5 * (1 - np.sqrt(Cm ** 7 / (Cm ** 7 + 25.0 ** 7)))
    ap1, ap2 = (1 + G) * a1, (1 + G) * a2
    Cp1, Cp2 = np.hypot(ap1, b1), np.hypot(ap2, b2)
    h1, h2 = _hue(b1, ap1), _hue(b2, ap2)
    grey = (Cp1 * Cp2) == 0
    dL, dC = L2 - L1, Cp2 - Cp1
    hd = h2 - h1
    dh = np.where(grey, 0.0, np.where(hd > 180, hd - 360, np.where(hd < -180, hd + 360, hd)))
    dH = 2 * np.sqrt(Cp1 * Cp2) * np.sin(np.radians(dh / 2))
    Lm, Cpm = (L1 + L2) / 2, (Cp1 + Cp2) / 2
    hs = h1 + h2
    hm = np.where(grey, hs, np.where(np.abs(h1 - h2) <= 180, hs / 2, np.where(hs < 360, (hs + 360) / 2, (hs - 360) / 2)))
    T = (1 - 0.17 * np.cos(np.radians(hm - 30)) + 0.24 * np.cos(np.radians(2 * hm)) + 0.32 * np.cos(np.radians(3 * hm + 6))
         - 0.20 * np.cos(np.radians(4 * hm - 63)))
    dtheta = 30 * np.exp(-(((hm - 275) / 25) ** 2))
    RC = 2 * np.sqrt(Cpm ** 7 / (Cpm ** 7 + 25.0 ** 7))
    SL = 1 + 0.015 * (Lm - 50) ** 2 / np.sqrt(20 + (Lm - 50) ** 2)
    SC = 1 + 0.045 * Cpm
    SH = 1 + 0.015 * Cpm * T
    RT = -np.sin(np.radians(2 * dtheta)) * RC
    tL, tC, tH = dL / SL, dC / SC, dH / SH
    return np.sqrt(np.maximum(tL ** 2 + tC ** 2 + tH ** 2 + RT * tC * tH, 0.0))


def ciede2000(pred, target, lab_input=False):
    """pred, target: [N,3,H,W] arrays or torch CPU tensors"""
    p = np.moveaxis(np.asarray(pred), 1, -1)
    t = np.moveaxis(np.asarray(target), 1, -1)
    if not lab_input:
        p, t = rgb2lab(p), rgb2lab(t)
    m = delta_e(p, t)
    return m, m.reshape(m.shape[0], -1).mean(axis=1)
