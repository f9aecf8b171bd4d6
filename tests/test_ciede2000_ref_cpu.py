"""The float64 CIEDE2000 reference of tests/_ref64_ciede.py against what is published and what the definition fixes: the pairs
of Sharma, Wu and Dalal's table that sit on the formula's branches, to half a unit of the table's fourth decimal; zero for equal
colours; sRGB black against white; the clamp and NaN rule; both sides of the two piecewise thresholds."""
import numpy as np
import pytest

from tests import _ref64_ciede as R

TABLE_TOL = 5e-5 + 1e-9


@pytest.mark.parametrize("k", range(len(R.SHARMA_PAIRS)))
def test_published_pairs(k):
    lab1, lab2, want = R.SHARMA_PAIRS[k]
    got = float(R.delta_e(np.array(lab1, dtype=np.float64), np.array(lab2, dtype=np.float64)))
    print(f"pair {k}: {lab1} vs {lab2}: dE00 {got:.10f} (table {want:.4f})")
    assert abs(got - want) <= TABLE_TOL


def test_knife_edge_pairs_are_printed_not_asserted():
    for lab1, lab2 in R.KNIFE_EDGE_PAIRS:
        got = float(R.delta_e(np.array(lab1, dtype=np.float64), np.array(lab2, dtype=np.float64)))
        print(f"hues 180 degrees apart: {lab1} vs {lab2}: dE00 {got:.10f}")
        assert np.isfinite(got)


def test_pairs_as_one_array_equal_the_pairs_one_by_one():
    a = np.array([p[0] for p in R.SHARMA_PAIRS], dtype=np.float64)
    b = np.array([p[1] for p in R.SHARMA_PAIRS], dtype=np.float64)
    whole = R.delta_e(a, b)
    for k in range(len(R.SHARMA_PAIRS)):
        assert whole[k] == float(R.delta_e(a[k], b[k]))


def test_identical_colours_give_zero():
    g = np.random.default_rng(0)
    rgb = g.random((64, 3))
    lab = R.rgb2lab(rgb)
    assert (R.delta_e(lab, lab) == 0).all()
    assert (R.delta_e(np.array([[50.0, 0, 0], [0.0, 0, 0], [100.0, 0, 0]]), np.array([[50.0, 0, 0], [0.0, 0, 0], [100.0, 0, 0]])) == 0).all()
    x = np.broadcast_to(rgb.T.reshape(1, 3, 8, 8), (2, 3, 8, 8))
    m, mean = R.ciede2000(x, x)
    assert m.shape == (2, 8, 8) and (m == 0).all() and (mean == 0).all()


def test_srgb_black_against_white():
    black, white = np.zeros(3), np.ones(3)
    lab_b, lab_w = R.rgb2lab(black), R.rgb2lab(white)
    assert lab_b[0] == 0 and abs(lab_b[1]) < 1e-12 and abs(lab_b[2]) < 1e-12
    got = float(R.delta_e(lab_b, lab_w))
    print(f"black against white: {got:.10f}")
    assert abs(got - 100.0000002) <= 5e-8             # half a unit of the last decimal stated
    assert float(R.delta_e(lab_w, lab_b)) == got


def test_clamp_and_nan_rule():
    f32 = np.float32
    odd = np.array([[-0.5, 1.5, np.nan], [-np.inf, np.inf, -0.0], [2.0, -1e-30, 1.0 + 2.0 ** -23]], dtype=f32)
    same = np.array([[0.0, 1.0, 0.0], [0.0, 1.0, 0.0], [1.0, 0.0, 1.0]], dtype=f32)
    assert np.array_equal(R.rgb2lab(odd), R.rgb2lab(same))
    assert (R.delta_e(R.rgb2lab(odd), R.rgb2lab(same)) == 0).all()


def test_both_sides_of_the_srgb_knee():
    below, above = np.nextafter(R.SRGB_KNEE, 0), np.nextafter(R.SRGB_KNEE, 1)
    for v, linear in ((below, True), (R.SRGB_KNEE, True), (above, False)):
        # a grey of that value: Y is the decoded value itself (the middle row of the matrix sums to 1)
        L = R.rgb2lab(np.array([v, v, v]))[0]
        lin = v / 12.92 if linear else ((v + 0.055) / 1.055) ** 2.4
        y = lin * (0.212671 + 0.715160 + 0.072169)
        assert y <= R.LAB_KNEE
        assert abs(L - (116 * (y / (3 * (6 / 29) ** 2) + 4 / 29) - 16)) <= 1e-13
    # the two pieces do not meet exactly: 0.04045 is the rounded knee.  The step is far below anything a test resolves.
    step = ((R.SRGB_KNEE + 0.055) / 1.055) ** 2.4 - R.SRGB_KNEE / 12.92
    print(f"sRGB decoding steps by {step:.3e} at 0.04045")
    assert abs(step) < 1e-7


def test_both_sides_of_the_lab_knee():
    # a grey whose Y lies just below / above (6/29)^3: f switches from the line to the cube root
    for y, cube in ((np.nextafter(R.LAB_KNEE, 0), False), (R.LAB_KNEE, False), (np.nextafter(R.LAB_KNEE, 1), True)):
        lin = y                                        # Y = lin * 1.0 up to rounding; solve for the sRGB value
        v = 1.055 * lin ** (1 / 2.4) - 0.055
        L = R.rgb2lab(np.array([v, v, v]))[0]
        f = np.cbrt(y) if cube else y / (3 * (6 / 29) ** 2) + 4 / 29
        assert abs(L - (116 * f - 16)) <= 1e-9         # v is y only to rounding; the pieces meet at the knee (both give 6/29)
    assert abs(np.cbrt(R.LAB_KNEE) - (R.LAB_KNEE / (3 * (6 / 29) ** 2) + 4 / 29)) <= 1e-15
    assert abs(116 * (6 / 29) - 16 - 8.0) <= 1e-13     # L = 8 at the knee, the familiar number


def test_symmetry_and_hue_wrap():
    # dE00 is symmetric in its arguments; pairs straddling 0 / 360 degrees take the wrapped difference and mean
    a = np.array([[60.0, 20.0, -1.0], [60.0, 20.0, 1.0], [40.0, -5.0, -30.0]])
    b = np.array([[55.0, 18.0, 2.0], [61.0, 19.0, -3.0], [45.0, 6.0, -28.0]])
    assert np.allclose(R.delta_e(a, b), R.delta_e(b, a), rtol=0, atol=1e-12)
    near = R.delta_e(np.array([50.0, 10.0, -0.5]), np.array([50.0, 10.0, 0.5]))      # hues 357 and 3 degrees
    assert near < 1.0
