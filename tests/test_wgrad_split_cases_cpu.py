"""The case table of the weight-gradient split sweep (tests/_wgrad_split_cases.py), checked without a GPU: the facts it
derives for the F(4x4,3x3) shapes are pinned, and the table as a whole must put every kernel family through every situation
a forced split count can put it in -- so that a later edit of a shape cannot quietly stop exercising one."""
import pytest

from tests import _wgrad_split_cases as W


def _case(family, kind, *shape):
    hits = [c for c in W.cases_of(family) if (c.kind, c.N, c.Ci, c.Co, c.H, c.W) == (kind,) + shape]
    assert len(hits) == 1, (family, kind, shape)
    return hits[0]


def test_partitions_cover_every_tile_once_and_respect_the_contract():
    for c, n in W.sweep():
        T = W.tiles(c)
        assert 1 <= n <= T, (c, n)                       # never above the engine's clamp
        parts = W.split_tiles(c, n)
        assert len(parts) == n
        assert sorted(t for p in parts for t in p) == list(range(T)), (c, n)
        f = W.facts(c, n)
        if W.PARTITION[c.family] != "ceil":
            assert f.empty == 0, (c, n)                  # floor + remainder and strided splits all have tiles for nsplit <= T
        else:
            per = -(-T // n)
            assert f.empty == n - -(-T // per), (c, n)
        assert f.launched == (-(-n // 8) * 8 if c.family != "general" else n)
    assert all(len({g.T for g in W.grids(c)}) == 1 for c in W.CASES)    # the classes of a layer share one tile count


def test_split_counts_follow_the_rule():
    for c in W.CASES:
        T, ns = W.tiles(c), W.split_counts(c)
        assert set(ns) >= {n for n in (1, 2, 3, 5, 8, 9, 13, T - 1, T) if 1 <= n <= T}, c
        assert ns == sorted(set(ns)) and ns[0] >= 1 and ns[-1] == T
        if W.PARTITION[c.family] == "ceil" and T >= 8:
            more = [n for n in ns if T / 2 < n < T and n not in (8, 9, 13, T - 1) and W.facts(c, n).empty > 0]
            assert len(more) >= 2, (c, more)


def test_wino43_shape_2x96x96x20x136():
    c = _case("wino43", "conv3", 2, 96, 96, 20, 136)
    g = W.grids(c)[0]
    assert (g.T, g.TY * g.TX, g.TX) == (90, 45, 9)
    assert sum(g.interior) == 42
    assert g.ragged_x and all(not g.interior[t] for t in range(g.TX - 1, g.T, g.TX))     # the ragged last strip of a row is a border strip
    for n in (1, 2, 3, 4, 5, 8, 9, 13):
        assert W.facts(c, n).transitions == {"BB", "BI", "IB", "II"}, n
    for n in (1, 3, 4, 5, 8, 9, 13):
        assert W.facts(c, n).straddling >= 1, n
    assert W.facts(c, 2).straddling == 0                 # 45 strips per split: the seam is a split boundary
    f = W.facts(c, 89)
    assert max(f.sizes) == 2 and f.empty == 44
    assert set((1, 2, 3, 4, 5, 8, 9, 13, 89, 90)) <= set(W.split_counts(c))


def test_wino43_shape_3x32x96x8x40():
    c = _case("wino43", "conv3", 3, 32, 96, 8, 40)
    g = W.grids(c)[0]
    assert (g.T, g.TY * g.TX) == (18, 6)
    assert not any(g.interior)
    f = W.facts(c, 4)
    assert max(f.sizes) == 5 and f.sizes == (5, 5, 5, 3) and f.straddling == 2
    assert [W.facts(c, n).empty for n in (8, 10, 13, 17)] == [2, 1, 4, 8]
    assert [W.facts(c, n).launched for n in (13, 17)] == [16, 24]
    assert set((4, 8, 10, 13, 17)) <= set(W.split_counts(c))


def test_wino43_shape_1x192x96x12x72():
    c = _case("wino43", "conv3", 1, 192, 96, 12, 72)
    assert W.tiles(c) == 15 and c.Ci // 32 * (c.Co // 96) == 6
    assert W.facts(c, 2).sizes == (8, 7)
    assert [W.facts(c, n).empty for n in (9, 10, 13, 14)] == [1, 2, 5, 6]
    assert set((2, 9, 10, 13, 14)) <= set(W.split_counts(c))


def test_wino43_shape_1x64x192x8x16():
    c = _case("wino43", "conv3", 1, 64, 192, 8, 16)
    assert W.tiles(c) == 2 and c.Ci // 32 * (c.Co // 96) == 4
    assert W.split_counts(c) == [1, 2]


def test_rows_and_wino32_geometry():
    """Tile counts and interior tiles of one shape per remaining family, worked out by hand from the kernel sources."""
    # rows kernel, 3x3: 3 x 3 tiles of 4 x 32 per image; only the middle one has its 6 x 34 halo inside the 12 x 96 image
    g = W.grids(_case("wino23_rows", "conv3", 2, 32, 96, 12, 96))[0]
    assert g.T == 18 and [t for t in range(g.T) if g.interior[t]] == [4, 13]
    # rows kernel, Conv2d k4 s2 on 24 x 128: class grid 12 x 64 = 3 x 2 tiles; class (py, px) = (0, 0) reads from input pixel
    # (-1, -1): tile rows 1, 2 of tile column 1 are interior; class (1, 1) reads from (0, 0) and 9 rows / 65 columns of
    # stride 2: tile rows 0, 1 of tile column 0
    gs = W.grids(_case("rows_direct", "conv4s2", 2, 32, 64, 24, 128))
    assert len(gs) == 4 and gs[0].T == 12
    assert [t for t in range(6) if gs[0].interior[t]] == [3, 5]
    assert [t for t in range(6) if gs[3].interior[t]] == [0, 2]
    # conv_wgrad32_kernel, transposed 10 x 50: regions of 3 x 48 -> 4 x 2 per image, ragged in both directions
    g = W.grids(_case("wino32_v1", "convT", 2, 96, 32, 10, 50))[0]
    assert (g.T, g.TY, g.TX, g.ragged_y, g.ragged_x) == (16, 4, 2, True, True)
    # v2: strips of 3 x 24 on the 7 x 50 class grid of Conv2d k4 s2 on 14 x 100 -> 3 x 3 per image
    g = W.grids(_case("wino32_v2", "conv4s2", 2, 64, 96, 14, 100))[0]
    assert (g.T, g.TY, g.TX, g.ragged_y, g.ragged_x) == (18, 3, 3, True, True)
    # which F(3x3,2x2) kernel takes a shape
    assert W.wino32_variant(W.Case("x", "convT", 1, 64, 96, 3, 24)) == "v2"
    assert W.wino32_variant(W.Case("x", "convT", 1, 96, 64, 3, 24)) == "v2c96"
    assert W.wino32_variant(W.Case("x", "convT", 1, 192, 192, 3, 24)) == "v2"
    assert W.wino32_variant(W.Case("x", "convT", 1, 96, 32, 3, 24)) == "v1"
    assert W.wino32_variant(W.Case("x", "convT", 1, 64, 48, 3, 24)) == "v1"
    for c in W.CASES:
        if c.family.startswith("wino32_v"):
            assert "wino32_" + W.wino32_variant(c) == c.family, c
        if c.family == "wino32_merged":
            assert c.kind == "convT" and W.wino32_variant(c) != "v1", c


@pytest.mark.parametrize("family", sorted(W.PARTITION))
def test_every_family_meets_every_situation(family):
    s = W.family_summary(family)
    rule = W.PARTITION[family]
    assert s["straddling"], "a split that crosses an image seam"
    assert s["odd_above_8"], "a split count above 8 that is no multiple of 8"
    assert s["border"]
    assert s["single"] or family in ("wino43", "general"), "a launch of a single tile"   # wino43: the issue's smallest is 2 strips
    if rule == "ceil":
        assert s["empty"], "empty trailing splits"
    if W.PADS_GRID[family]:
        assert s["padded"], "launched splits beyond nsplit"
    if W.TWO_STAGING_PATHS[family]:
        assert s["interior"]
        assert s["transitions"] == {"BB", "BI", "IB", "II"}, s["transitions"]
    if family in ("wino23_rows", "rows_direct"):
        assert not s["ragged_x"] and not s["ragged_y"]          # the rows kernel takes grids of whole tiles only
    elif family == "wino43":
        assert s["ragged_x"]                                     # H % 4 == 0: strips are never ragged in y
    else:
        assert s["ragged_x"] and s["ragged_y"]


def test_families_that_share_a_merged_launch_cover_both_channel_splits():
    assert {W.wino32_variant(c) for c in W.cases_of("wino32_merged")} == {"v2", "v2c96"}
    assert {c.kind for c in W.cases_of("rows_direct")} == {"conv3", "conv4s2", "convT"}
    assert {c.kind for c in W.cases_of("general")} == {"conv1", "conv3s2"}
    assert any(c.Co % 96 != 0 for c in W.cases_of("wino23_rows"))


def test_regression_lines_are_part_of_the_sweep():
    ids = {(c.family, c.id, n) for c, n in W.sweep()}
    for r in W.REGRESSIONS:
        assert r in ids, r


def test_shapes_the_rows_kernel_turns_down():
    """wgrad_rows_plan: VW % 32 == 0 and VH % 4 == 0."""
    for N, Ci, Co, H, Wd in W.NOT_ROWS_SHAPES:
        assert H % 4 != 0 or Wd % 32 != 0
    for c in W.cases_of("wino23_rows"):
        assert c.H % 4 == 0 and c.W % 32 == 0 and c.Ci % 32 == 0
