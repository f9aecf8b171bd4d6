"""Float64 reference, error bound and cases of the weight-gradient reduce entry points (csrc/conv_wgrad_reduce.hip), shared by
tests/test_gpu_wgrad_reduce.py (the library on the GPU) and tests/test_wgrad_reduce_hostemu_cpu.py (the same source compiled
for the host under the sanitizers).

Every entry point computes, per element (tap, k, n) the layout names,
    dst[off(tap, k, n)] (+)= sum over planes f of M[tap][f] * (sum over splits s of slab[s][f][k][n])
with M the inverse transform of the slab's domain (the identity for the tap-domain slabs).  The reference evaluates that in
float64.  The bound per element is
    (nsplit + c) * EPS * (sum_f |M[tap][f]| * sum_s |slab[s][f][k][n]|)
-- any summation order of nsplit terms loses at most (nsplit - 1) EPS of the sum of absolute values to first order, and every
further floating-point operation on the longest path from a slab element to the output (c of them) at most one EPS of the
absolute-coefficient transform; the one unit left over covers the second-order terms.  With accumulate = 1 the final
`dst + value` is one more operation on the path and |dst| joins the absolute sum.  c, counted from the inverse() bodies of
csrc/conv_wgrad_reduce.hip (an exact scaling by a power of two counted like any other operation):
    tap domain  0
    F(2x2,3x3)  6   per side: u1 +- u2, * 0.5, + u0 (or + u3); two sides
    F(3x3,2x2)  5   * (0.5 | 0.25), then per side two additions
    F(4x4,3x3)  2   evaluated in float64 (32 operations of 2^-53 each and the rounded 1 / N constants: below one EPS
                    together, counted as one) and rounded to float once
"""
from typing import NamedTuple

import numpy as np

from tests._util import EPS


class Layout(NamedTuple):         # struct adh_wlayout
    K: int
    Nc: int
    KHt: int
    KWt: int
    tap_off0: int
    tap_off_sy: int
    tap_off_sx: int
    stride_k: int
    stride_n: int


def layout(K, Nc, KH, KW, reverse=False, slack=(0, 0), base=0):
    """[n][k][KH][KW] (Conv2d OIHW with k = ci, n = co) of a tensor with slack[0] more k and slack[1] more n than the layout
    names, starting `base` elements into dst; reverse: the taps walked backwards (negative tap strides, tap_off0 on the last
    tap), as engine._wgrad_layout makes them.  Returns (Layout, number of dst elements)."""
    Kt, Nt = K + slack[0], Nc + slack[1]
    L = Layout(K, Nc, KH, KW, base, KW, 1, KH * KW, Kt * KH * KW)
    if reverse:
        L = L._replace(tap_off0=base + (KH - 1) * KW + (KW - 1), tap_off_sy=-KW, tap_off_sx=-1)
    return L, base + Nt * Kt * KH * KW


def offsets(L):
    """int64 [KHt][KWt][K][Nc]: the dst offset of every element the layout names"""
    ty, tx, k, n = np.meshgrid(np.arange(L.KHt), np.arange(L.KWt), np.arange(L.K), np.arange(L.Nc), indexing="ij")
    return L.tap_off0 + ty * L.tap_off_sy + tx * L.tap_off_sx + k * L.stride_k + n * L.stride_n


def _sandwich(left, scale, right):
    """M[(i, j), (a, b)] = left[a][i] * scale[a][b] * right[b][j]: w = left^T (scale . u) right as one matrix on u.flatten()"""
    left, right = np.asarray(left, np.float64), np.asarray(right, np.float64)
    return np.einsum("ai,ab,bj->ijab", left, np.asarray(scale, np.float64), right).reshape(left.shape[1] * right.shape[1], -1)


def _f23():
    G = [[1, 0, 0], [.5, .5, .5], [.5, -.5, .5], [0, 0, 1]]
    s = np.array([1., 1., 1., -1.])                       # the signs the accumulating kernel deferred
    return _sandwich(G, np.outer(s, s), G)


def _f32():
    A = [[1, 0], [1, 1], [1, -1], [0, -1]]
    h = np.array([1., .5, .5, 1.])                        # the halves of G the accumulating kernel deferred
    return _sandwich(A, np.outer(h, h), A)


def _f43():
    a, b = 0.75, 1.25
    n0, na, nb = a * a * b * b, 2 * a * a * (a * a - b * b), 2 * b * b * (b * b - a * a)
    inv = np.array([1 / n0, 1 / na, 1 / na, 1 / nb, 1 / nb, 1.0])
    A = np.array([[1, 1, 1, 1, 1, 0], [0, a, -a, b, -b, 0], [0, a * a, a * a, b * b, b * b, 1]]).T     # A' [6][3]
    return _sandwich(A, np.outer(inv, inv), A)


# domain -> (inverse transform M [output taps][planes], c)
DOMAINS = {"f23": (_f23(), 6), "f32": (_f32(), 5), "f43": (_f43(), 2)}


def tap_domain(T):
    return np.eye(T), 0


# the kernel-parity classes of the F(3x3,2x2) form (csrc/conv_wgrad32.hip, wgrad32_plan): (tap0, tap_sy, tap_sx, rev) per class;
# output tap (hy, hx) of a class is tap index tap0 + ty tap_sy + tx tap_sx of the layer's taps, (ty, tx) = (1 - hy, 1 - hx) if rev
CONV_K4S2_CLASSES = [(py * 4 + px, 8, 2, 0) for py in range(2) for px in range(2)]     # Conv2d k4 s2: ky = 2 ty + py
CONVT_CLASS = [(0, 2, 1, 1)]                                                             # one 2x2 class, taps walked backwards


def class_taps(classes, KWt):
    """[class][4 output taps (hy, hx)] -> (ty, tx) of the layout"""
    out = []
    for tap0, sy, sx, rev in classes:
        row = []
        for hy in range(2):
            for hx in range(2):
                t = tap0 + ((1 - hy) if rev else hy) * sy + ((1 - hx) if rev else hx) * sx
                row.append((t // KWt, t % KWt))
        out.append(row)
    return out


def reference(slab, M, c, L, taps, dst0, accumulate):
    """slab: float32 [nsplit][classes][planes][KP][NcP]; taps[class][output tap] = (ty, tx) of L; dst0: float32 dst before the
    call.  Returns (ref float64 [len(dst0)], bound float64, written bool): the expected dst, its bound, the elements named."""
    nsplit = slab.shape[0]
    s = slab.astype(np.float64)[:, :, :, :L.K, :L.Nc]
    val = np.einsum("tf,cfkn->ctkn", M, s.sum(0))
    mag = np.einsum("tf,cfkn->ctkn", np.abs(M), np.abs(s).sum(0))
    off = offsets(L)
    ref = dst0.astype(np.float64)
    bound = np.zeros_like(ref)
    written = np.zeros(ref.shape, bool)
    for ci, row in enumerate(taps):
        for ti, (ty, tx) in enumerate(row):
            o = off[ty, tx]
            assert not written[o].any(), "the layout names an element twice"
            written[o] = True
            if accumulate:
                bound[o] = (nsplit + c + 1) * EPS * (mag[ci, ti] + np.abs(ref[o]))
                ref[o] = ref[o] + val[ci, ti]
            else:
                bound[o] = (nsplit + c) * EPS * mag[ci, ti]
                ref[o] = val[ci, ti]
    return ref, bound, written


def all_taps(L):
    return [[(ty, tx) for ty in range(L.KHt) for tx in range(L.KWt)]]


def packed_reference(slab, Cin, KH, KW, Cout, dst0, accumulate):
    """adh_wgrad_reduce_packed: slab float32 [nsplit][KH * KWg][32 = (kx % 4) * 8 + ci][NcP] -> OIHW [Cout][Cin][KH][KW]"""
    nsplit = slab.shape[0]
    s = slab.astype(np.float64)
    co, ci, ky, kx = np.meshgrid(np.arange(Cout), np.arange(Cin), np.arange(KH), np.arange(KW), indexing="ij")
    KWg = (KW + 3) // 4
    pick = s[:, ky * KWg + kx // 4, (kx % 4) * 8 + ci, co].reshape(nsplit, -1)
    ref = dst0.astype(np.float64)
    if accumulate:
        bound = (nsplit + 1) * EPS * (np.abs(pick).sum(0) + np.abs(ref))
        return ref + pick.sum(0), bound
    return pick.sum(0), nsplit * EPS * np.abs(pick).sum(0)


def check(got, dst0, ref, bound, written, what):
    """every named element within its bound, every other element of dst bit-for-bit what it was; prints the worst ratio"""
    assert not np.isnan(got[written]).any(), f"{what}: an element the layout names was not written"
    err = np.abs(got[written].astype(np.float64) - ref[written])
    b = bound[written]
    worst = float((err / np.maximum(b, 1e-300)).max()) if err.size else 0.0
    print(f"[bound] {what}: worst |err| / bound = {worst:.3f}")
    assert (err <= b).all(), f"{what}: |err| / bound = {worst:.3f}"
    assert np.array_equal(got[~written].view(np.int32), dst0[~written].view(np.int32)), \
        f"{what}: an element the layout does not name was written"


def rng_slab(seed, *shape):
    return np.random.default_rng(seed).standard_normal(shape, dtype=np.float32)


def rng_dst(seed, n, accumulate):
    """NaN for accumulate = 0 (an unwritten element stays visible), seeded values for accumulate = 1"""
    if accumulate:
        return np.random.default_rng(seed + 1000).standard_normal(n, dtype=np.float32)
    return np.full(n, np.nan, np.float32)


# ------------------------------------------------------------------------------------------------ cases
KP = NCP = 32                      # padded slab sizes of every case
SIZES = [(5, 7), (32, 32)]         # (L.K, L.Nc): real sizes below the padded ones, and equal to them
ENTRY_DOMAIN = {"adh_wgrad_reduce_wino": "f23", "adh_wgrad_reduce_wino43": "f43", "adh_wgrad_reduce_wino32": "f32"}


class Case(NamedTuple):
    entry: str
    L: Layout
    ndst: int
    M: np.ndarray        # inverse transform [output taps][planes]
    c: int
    taps: list           # [class][output tap] -> (ty, tx)
    classes: list        # wino32: (tap0, tap_sy, tap_sx, rev) per class, else []

    def slab(self, seed, nsplit):
        return rng_slab(seed, nsplit, len(self.taps), self.M.shape[1], KP, NCP)


def case(entry, K, Nc, KH=3, reverse=False, strided=True, classes=None):
    """A case of `entry` on a KH x KH-tap layout of K x Nc real channels; strided: dst is a larger tensor of which the layout
    names a part (one more k, two more n, three elements in front); classes: the class table of the wino32 form."""
    L, ndst = layout(K, Nc, KH, KH, reverse=reverse, slack=(1, 2) if strided else (0, 0), base=3 if strided else 0)
    if entry in ENTRY_DOMAIN:
        M, c = DOMAINS[ENTRY_DOMAIN[entry]]
        taps = class_taps(classes, KH) if classes else all_taps(L)
    else:
        (M, c), taps = tap_domain(KH * KH), all_taps(L)
    return Case(entry, L, ndst, M, c, taps, list(classes or []))
