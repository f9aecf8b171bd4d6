"""float64 reference of adh_batch_nhhaze_from_u8 (csrc/dataset.hip): patchy, wavelength-dependent haze.  Used by
tests/test_nhhaze_cpu.py (which checks it against itself, a pure-Python integer hash and tests/_haze_synth_ref64.haze_ref), the
host-emulated run and tests/test_gpu_nhhaze.py, with the field rows that go with the case table of tests/_haze_synth_ref64.py.

Per source pixel (y, x) of window n and channel c:  d as in haze_ref;  f = field(y + oy, x + ox; seed, f0, K) in [0, 1];
m = 1 + s (2 f - 1);  t_c = exp(-((beta_c m) d));  h_c = clip(J_c t_c + A_c (1 - t_c), 0, 1);  then augment_ref.

The field is K octaves of value noise on an integer-hashed lattice: octave k has frequency f_k = f0 2^k (exact), the position
p = (double)coordinate * f_k is ONE multiplication, so its floor -- the lattice cell -- is the same number wherever IEEE doubles
are multiplied; the lattice values are 32-bit hashes / 2^32 (exact as doubles), blended by the cubic fade u u (3 - 2 u)."""
import numpy as np

from tests import _haze_synth_ref64 as Z

EPS, U53 = Z.EPS, Z.U53
C_X, C_Y, C_K = 0x9E3779B1, 0x85EBCA77, 0xC2B2AE3D
MIX_1, MIX_2 = 0x7FEB352D, 0x846CA68B
LAMBDA_NM = (610.0, 550.0, 465.0)
MAX_OCTAVES = 4

# Double arithmetic of the field and of what it feeds, kernel against numpy, counted as HAZE_F64_UNITS counts: every rounding
# that the two sides could take differently, each at a magnitude below 4 (<= 2^-51 = 4 units of 2^-53).  The kernel's field code
# is compiled with floating-point contraction off, so the products coordinate * f_k are the same IEEE operation on both sides
# (they are large: up to 2^31); everything after them works on fractions in [0, 1).
#   per octave: 2 products, 2 exact subtractions, two fades of 3 roundings (u u, 3 - 2 u, their product), three lerps of 3
#               (b - a, w *, a +), the addition into the sum (2^-k scales exactly): 2 + 6 + 9 + 1 = 18; four octaves: 72
#   then:       the division by the sum of the weights, 2 f - 1 (2 f is exact), s *, 1 +, beta_c *: 5
# 77 roundings per side, passed on with a gain of 2 s < 2 into m, beta_c <= 4 into beta_c m and d <= 2 into the exponent (exp's
# slope is <= 1 there and |J - A| <= 1): 77 * 4 * 16 = 4928 per side, 9856 for both, plus the 644 of the uniform model (with
# beta_c m <= 4 in the place of beta): 10500, stated as 16384 units of 2^-53 = 2^-39.
NH_F64_UNITS = 16384
NH_F64_CAP = 2.0 ** -36           # 1 / 4096 of an fp32 unit: the float64 term cannot hide an fp32 error
# The fp32 terms are HAZE_BOUND's and HAZE_AUG_BOUND's: the model adds no fp32 rounding.
NH_BOUND = 2 * EPS + NH_F64_UNITS * U53
NH_AUG_BOUND = 9 * EPS + 2 * NH_F64_UNITS * U53


# ------------------------------------------------------------------------------------------------ hash and field
def hash32_py(ix, iy, k, seed):
    """the lattice hash on Python integers"""
    M = 0xFFFFFFFF
    h = ((ix * C_X) & M) ^ ((iy * C_Y) & M) ^ ((k * C_K) & M) ^ (seed & M)
    h ^= h >> 16
    h = (h * MIX_1) & M
    h ^= h >> 15
    h = (h * MIX_2) & M
    h ^= h >> 16
    return h


def hash32(ix, iy, k, seed):
    """the same on integer arrays -> uint64 arrays of values below 2^32"""
    M = np.uint64(0xFFFFFFFF)
    ix, iy = np.asarray(ix).astype(np.int64).astype(np.uint64) & M, np.asarray(iy).astype(np.int64).astype(np.uint64) & M
    h = ((ix * np.uint64(C_X)) & M) ^ ((iy * np.uint64(C_Y)) & M) ^ np.uint64((k * C_K) & 0xFFFFFFFF) ^ np.uint64(int(seed) & 0xFFFFFFFF)
    h ^= h >> np.uint64(16)
    h = (h * np.uint64(MIX_1)) & M
    h ^= h >> np.uint64(15)
    h = (h * np.uint64(MIX_2)) & M
    h ^= h >> np.uint64(16)
    return h


def field_ref(CH, CW, row):
    """float64 [CH, CW]: the density field of the window whose first pixel is image pixel (oy, ox); row = {seed, oy, ox, K, s, f0}"""
    seed, oy, ox, K, _, f0 = [float(v) for v in row]
    seed, oy, ox, K = int(seed), int(oy), int(ox), int(K)
    y = (np.arange(CH, dtype=np.int64) + oy).astype(np.float64)[:, None]
    x = (np.arange(CW, dtype=np.int64) + ox).astype(np.float64)[None, :]
    acc, norm = np.zeros((CH, CW)), 0.0
    for k in range(K):
        fk = f0 * 2.0 ** k
        py, px = y * fk, x * fk
        iy, ix = np.floor(py), np.floor(px)
        uy, ux = py - iy, px - ix
        wy, wx = uy * uy * (3.0 - 2.0 * uy), ux * ux * (3.0 - 2.0 * ux)
        iy = np.broadcast_to(iy, (CH, CW)).astype(np.int64)
        ix = np.broadcast_to(ix, (CH, CW)).astype(np.int64)
        v00, v01 = [hash32(ix + a, iy, k, seed).astype(np.float64) / 4294967296.0 for a in (0, 1)]
        v10, v11 = [hash32(ix + a, iy + 1, k, seed).astype(np.float64) / 4294967296.0 for a in (0, 1)]
        top, bot = v00 + wx * (v01 - v00), v10 + wx * (v11 - v10)
        acc = acc + 2.0 ** -k * (top + wy * (bot - top))
        norm += 2.0 ** -k
    return acc / norm


def slope_bound(K, f0):
    """how far two neighbouring pixels' field values can lie apart: the fade's slope is at most 1.5 per cell, octave k has 2^k f0
    cells per pixel and weight 2^-k"""
    return 1.5 * K * f0 / sum(2.0 ** -k for k in range(K))


def nhhaze_ref(clear, depth, fog6, field, depth_range=(0.3, 1.0), params=None):
    """clear uint8 [N, CH, CW, 3], depth uint16 [N, CH, CW] or None (radial), fog6 [N, 6] {beta_r beta_g beta_b A_r A_g A_b} (their
    float32 values), field float64 [N, 6] {seed oy ox K s f0}, params [N, 5] or None -> float64 [N, 3, CH, CW]"""
    clear = np.asarray(clear)
    N, CH, CW, _ = clear.shape
    fog6 = np.asarray(fog6, dtype=np.float32).astype(np.float64).reshape(N, 6)
    field = np.asarray(field, dtype=np.float64).reshape(N, 6)
    near, far = float(depth_range[0]), float(depth_range[1])
    out = []
    for n in range(N):
        J = clear[n].astype(np.float64).transpose(2, 0, 1) / 255.0
        d = Z.radial_depth(CH, CW) if depth is None else near + (far - near) * (np.asarray(depth[n]).astype(np.float64) / 65535.0)
        m = 1.0 + field[n, 4] * (2.0 * field_ref(CH, CW, field[n]) - 1.0)
        t = np.stack([np.exp(-((fog6[n, c] * m) * d)) for c in range(3)])
        x = np.clip(J * t + fog6[n, 3:6, None, None] * (1.0 - t), 0.0, 1.0)
        if params is not None:
            x = Z.augment_ref(x, params[n])
        out.append(np.ascontiguousarray(x))
    return np.stack(out)


# ------------------------------------------------------------------------------------------------ cases
CASES = Z.CASES
BIG = 2 ** 20
F32 = lambda v: float(np.float32(v))      # noqa: E731
# {seed, oy, ox, K, s, f0} per window of each case.  5 x 7 and 8 x 12: f0 = 0.25 with K = 2 (cells of 4 and 2 pixels: several
# lattice columns inside one quad, the 0.5 limit reached), origins off a multiple of the cell, one near 2^20; K = 1 and K = 4,
# s = 0 and s = 0.99, frequencies that are no power of two; 40 x 130: f0 = 1/64, K = 3, where most quads sit inside one cell.
FIELD_ROWS = {
    "5x7_bytes": [(7, 3, 5, 2, 0.6, 0.25), (2 ** 32 - 1, BIG - 3, BIG + 1, 2, 0.99, 0.25), (0, 0, 0, 1, 0.0, 0.5)],
    "8x12_phases": [(11, 1, 2, 2, 0.5, 0.25), (12, 5, 7, 2, 0.99, 0.25), (13, 0, 0, 1, 0.3, 0.5),
                    (14, BIG - 3, BIG - 5, 4, 0.8, 0.0625), (15, 6, 3, 2, 0.0, 0.25)],
    "8x12_out_off": [(21, 3, 1, 2, 0.7, 0.25), (22, 9, 14, 4, 0.99, 0.0625), (23, 2, 2, 3, 0.4, 0.125)],
    "1x9": [(31, 0, 0, 2, 0.5, 0.25), (32, 7, BIG - 1, 1, 0.9, F32(0.3)), (33, 3, 3, 4, 0.2, F32(1 / 17))],
    "9x1": [(41, 5, 9, 2, 0.6, 0.25), (42, BIG - 6, 0, 3, 0.99, 0.11)],
    "40x130": [(51, 0, 0, 3, 0.5, 1 / 64), (52, 100, 200, 3, 0.8, 1 / 64), (53, 17, 33, 4, 0.99, F32(1 / 48))],
    "tight_end_off_4": [(61, 1, 2, 2, 0.5, 0.25), (62, 0, 3, 1, 0.99, 0.37)],
    "tight_base_3_cw8": [(71, 0, 1, 2, 0.6, 0.25), (72, 4, 4, 3, 0.3, 0.1)],
    "512x516": [(81, 1, 3, 3, 0.6, F32(1 / 160))],
}


def chromatic(fog, alpha, tint):
    """fog [N, 2] {beta, A}, alpha [N], tint [N, 3] -> float32 [N, 6]: beta_c = beta (lambda_c / lambda_g)^-alpha, green keeps
    beta; A_c = clip(A + tint_c, 0, 1)"""
    fog = np.asarray(fog, dtype=np.float32).astype(np.float64)
    ratio = np.array(LAMBDA_NM) / LAMBDA_NM[1]
    beta = fog[:, :1] * ratio[None, :] ** (-np.asarray(alpha, dtype=np.float64)[:, None])
    beta[:, 1] = fog[:, 0]
    A = np.clip(fog[:, 1:2] + np.asarray(tint, dtype=np.float64), 0.0, 1.0)
    return np.concatenate([beta, A], axis=1).astype(np.float32)


def grey(fog):
    """fog [N, 2] -> float32 [N, 6] with equal channels"""
    fog = np.asarray(fog, dtype=np.float32)
    return np.ascontiguousarray(np.concatenate([np.repeat(fog[:, :1], 3, 1), np.repeat(fog[:, 1:], 3, 1)], axis=1))


def build(case):
    """Z.build(case) plus fog6 float32 [N, 6] (the case's beta in [0.1, 1] spread by an Angstrom exponent in [0, 1.3]: beta_c m
    stays below 2.6, and a tint of +-0.05) and field float64 [N, 6]"""
    clear, depth, geom, dclear, ddepth, fog = Z.build(case)
    N = len(geom)
    rng = np.random.RandomState(1000 + sum(ord(ch) for ch in case["name"]))
    fog6 = chromatic(fog, rng.uniform(0.0, 1.3, N), rng.uniform(-0.05, 0.05, (N, 3)))
    field = np.array(FIELD_ROWS[case["name"]], dtype=np.float64).reshape(N, 6)
    return clear, depth, geom, dclear, ddepth, fog, fog6, field
