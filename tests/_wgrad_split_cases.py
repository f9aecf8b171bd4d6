"""Case table of the pixel-split sweep of the weight-gradient kernels (tests/test_gpu_wgrad_splits.py) and, in plain Python,
the partition rule and tile geometry each kernel family applies to a forced split count -- restated from the kernel sources,
so that tests/test_wgrad_split_cases_cpu.py can assert WITHOUT a GPU which situations every (case, nsplit) puts a kernel in.

Families (csrc file, kernel, what the splits divide, how):
  wino43        conv_wgrad43.hip  conv_wgrad_wino43_kernel        strips of 4 x 16 pixels           ceil
  wino23_rows   conv_wgrad.hip    conv_wgrad_rows_kernel<WINO>    tiles of 4 x 32 pixels            floor + remainder
  rows_direct   conv_wgrad.hip    conv_wgrad_rows_kernel          tiles of 4 x 32 (class) pixels    floor + remainder
  wino32_v1     conv_wgrad32.hip  conv_wgrad32_kernel             regions of 3 x 48 class pixels    floor + remainder
  wino32_v2     conv_wgrad32.hip  conv_wgrad32v2_kernel           strips of 3 x 24 class pixels     ceil
  wino32_v2c96  conv_wgrad32.hip  conv_wgrad32v2c96_kernel        strips of 3 x 24 class pixels     ceil
  wino32_merged conv_wgrad32.hip  the v2 kernels, the four classes of a transposed layer in ONE grid  ceil
  general       conv_wgrad.hip    conv_wgrad_kernel               tiles of TH x 32 pixels           strided (grid.y = nsplit)

  ceil:              per = ceil(T / nsplit), split i takes [i per, min((i + 1) per, T)): trailing splits may be EMPTY and must
                     still write a zero slab
  floor + remainder: per = T // nsplit, rem = T - per nsplit, split i takes per + (i < rem) tiles from i per + min(i, rem):
                     never empty for nsplit <= T
  strided:           split i takes tiles i, i + nsplit, ..: never empty for nsplit <= T
Tiles are numbered image-major, then tile row, then tile column.  Every family but `general` launches
ceil(nsplit / 8) * 8 splits per workgroup group (csrc/common.h, adh_split_grid_blocks): the padded ones return at once.

A tile is staged by one of two code paths: INTERIOR (its whole halo lies inside the image: unconditional LDS-DMA pieces,
in the F(4x4,3x3) and v2 kernels issued from inside the contraction of the tile before) or BORDER (zero fill + masked
pieces).  The stage-ahead loops therefore have four transitions between consecutive tiles of a split: BB, BI, IB, II.
The halo of a class starts at input pixel (ymin, xmin) for class pixel (0, 0), `xps` input pixels apart:
  3x3 s1 p1                ymin = xmin = -1, xps = 1
  Conv2d k4 s2 p1          kernel-parity class (py, px): ymin = py - 1, xmin = px - 1, xps = 2; class grid = (H / 2, W / 2)
  ConvTranspose2d k4 s2 p1 output-parity class (py, px), taps walked backwards: ymin = py - 1, xmin = px - 1, xps = 1;
                           class grid = (H, W) of the layer's input
"""
from typing import Dict, List, NamedTuple, Set, Tuple


class Case(NamedTuple):
    family: str
    kind: str      # conv3: Conv2d k3 s1 p1; conv4s2: Conv2d k4 s2 p1; convT: ConvTranspose2d k4 s2 p1; conv1: Conv2d k1;
    N: int         # conv3s2: Conv2d k3 s2 p1
    Ci: int
    Co: int
    H: int         # of the layer's INPUT
    W: int
    extra: Tuple[int, ...] = ()    # split counts on top of split_counts()' rule

    @property
    def id(self) -> str:
        return f"{self.kind}-{self.N}x{self.Ci}x{self.Co}x{self.H}x{self.W}"


PARTITION = {"wino43": "ceil", "wino23_rows": "floor", "rows_direct": "floor", "wino32_v1": "floor", "wino32_v2": "ceil",
             "wino32_v2c96": "ceil", "wino32_merged": "ceil", "general": "strided"}
PADS_GRID = {f: f != "general" for f in PARTITION}           # adh_split_grid_blocks
TWO_STAGING_PATHS = {f: f != "general" for f in PARTITION}   # the general kernel masks every lane of every tile alike

CASES: List[Case] = [
    # ---- F(4x4,3x3) domain: Cin % 32 == 0, Cout % 96 == 0, H % 4 == 0, W % 4 == 0
    Case("wino43", "conv3", 2, 96, 96, 20, 136, extra=(4,)),    # 45 strips per image, 42 interior, ragged last strip of a row
    Case("wino43", "conv3", 3, 32, 96, 8, 40, extra=(4, 10)),    # 6 strips per image, all border
    Case("wino43", "conv3", 1, 192, 96, 12, 72, extra=(10,)),    # six input-channel groups
    Case("wino43", "conv3", 1, 64, 192, 8, 16),                 # two strips, four groups: the smallest launch
    # ---- F(2x2,3x3) domain on the rows kernel.  Its plan (wgrad_rows_plan) takes H % 4 == 0, W % 32 == 0, Cin % 32 == 0 only:
    # the F(4x4,3x3) shapes above (W = 136, 40, 72, 16) and any H % 4 != 0 go to the general kernel instead, see
    # NOT_ROWS_SHAPES.  A grid of whole tiles has no ragged edge in either direction
    Case("wino23_rows", "conv3", 2, 32, 96, 12, 96),            # 9 tiles per image, the middle one interior; seams
    Case("wino23_rows", "conv3", 3, 64, 32, 8, 32),             # Cout % 96 != 0 (one n-tile per workgroup), all border, seams
    Case("wino23_rows", "conv3", 1, 96, 64, 12, 128),           # three input-channel groups, two n-tiles; two interior tiles in a row
    Case("wino23_rows", "conv3", 1, 32, 48, 4, 32),             # a single tile, partial last n-tile
    # ---- the rows kernel accumulating taps directly (Winograd off)
    Case("rows_direct", "conv3", 2, 32, 96, 12, 96),
    Case("rows_direct", "conv3", 1, 96, 64, 12, 128),           # two interior tiles in a row
    Case("rows_direct", "conv3", 1, 32, 48, 4, 32),             # a single tile, partial last n-tile
    Case("rows_direct", "conv4s2", 2, 32, 64, 24, 128),         # four kernel-parity launches, class grid 12 x 64
    Case("rows_direct", "convT", 2, 64, 32, 12, 64),            # four output-parity launches, taps walked backwards
    Case("rows_direct", "convT", 1, 32, 32, 4, 32),             # a single tile per class
    # ---- F(3x3,2x2) domain, conv_wgrad32_kernel (shapes the v2 kernels do not take)
    Case("wino32_v1", "conv4s2", 3, 32, 96, 6, 20),             # class grid 3 x 10: one region per image, a seam in every split > 1 tile
    Case("wino32_v1", "convT", 2, 96, 32, 10, 50),              # class grid 10 x 50: 4 x 2 regions, ragged in both directions
    Case("wino32_v1", "convT", 1, 32, 64, 12, 144),             # class grid 12 x 144: 4 x 3 exact regions, interior ones
    Case("wino32_v1", "conv4s2", 1, 32, 48, 6, 20),             # a single region, partial last n-tile
    # ---- F(3x3,2x2) domain, conv_wgrad32v2_kernel (Cin % 64 == 0, Cout % 96 == 0)
    Case("wino32_v2", "conv4s2", 2, 64, 96, 14, 100),           # four classes in one grid; class grid 7 x 50: 3 x 3 strips, ragged in both
    Case("wino32_v2", "convT", 2, 64, 192, 11, 37),             # two output-channel groups, 4 x 2 strips, ragged in both
    Case("wino32_v2", "convT", 1, 128, 96, 6, 72),              # two input-channel groups, 2 x 3 exact strips
    Case("wino32_v2", "convT", 1, 64, 96, 3, 24),               # a single strip
    # ---- conv_wgrad32v2c96_kernel (Cin % 96 == 0, Cout % 64 == 0)
    Case("wino32_v2c96", "conv4s2", 2, 96, 64, 14, 100),
    Case("wino32_v2c96", "convT", 1, 96, 128, 11, 37),          # two output-channel groups, ragged in both
    Case("wino32_v2c96", "convT", 1, 192, 64, 6, 72),           # two input-channel groups, 2 x 3 exact strips
    Case("wino32_v2c96", "convT", 1, 96, 64, 3, 24),            # a single strip
    # ---- the four classes of a transposed layer in one grid (adh_conv_wgrad_wino32_multi), both channel splits
    Case("wino32_merged", "convT", 2, 64, 192, 11, 37),
    Case("wino32_merged", "convT", 1, 128, 96, 6, 72),
    Case("wino32_merged", "convT", 1, 96, 128, 11, 37),
    Case("wino32_merged", "convT", 1, 64, 96, 3, 24),           # a single strip per class
    # ---- the general kernel, through the C ABI (the engine does not route its count through _rows_nsplit)
    Case("general", "conv1", 2, 48, 40, 9, 50),                 # 1x1 (classifier backbones): partial channel tiles on both sides
    Case("general", "conv3s2", 2, 32, 64, 18, 70),              # 3x3 stride 2 (classifier backbones): output grid 9 x 35
]

# 3x3 stride-1 shapes the F(2x2,3x3) rows kernel must turn down (adh_conv_wgrad_wino_groups == 0): the F(4x4,3x3) shapes,
# whose widths are no multiples of 32, and a height that is no multiple of 4
NOT_ROWS_SHAPES = [(2, 96, 96, 20, 136), (3, 32, 96, 8, 40), (1, 192, 96, 12, 72), (1, 64, 192, 8, 16), (1, 32, 96, 10, 64)]

# (family, case id, nsplit) that failed on the GPU when the sweep was first run, kept as named regression lines: every
# one of them is part of the sweep (test_wgrad_split_cases_cpu.py asserts it)
REGRESSIONS: List[Tuple[str, str, int]] = []


def cases_of(family: str) -> List[Case]:
    return [c for c in CASES if c.family == family]


def _ceil_div(a: int, b: int) -> int:
    return -(-a // b)


def wino32_variant(c: Case) -> str:
    """Which F(3x3,2x2) kernel wgrad32_plan gives a shape: 'v2' (Cin % 64 == 0, Cout % 96 == 0), 'v2c96' (Cin % 96 == 0,
    Cout % 64 == 0) -- both only where Cout is a multiple of 32 -- else 'v1'."""
    NcP = _ceil_div(c.Co, 32) * 32
    if c.Co == NcP and c.Ci % 64 == 0 and NcP % 96 == 0:
        return "v2"
    if c.Co == NcP and c.Ci % 96 == 0 and NcP % 64 == 0:
        return "v2c96"
    return "v1"


class Grid(NamedTuple):
    """The tiles one class (one grid or one launch) of a case is divided into."""
    N: int
    TY: int
    TX: int
    interior: Tuple[bool, ...]    # per tile, image-major then row then column
    ragged_y: bool                # the last tile row reaches beyond the class grid
    ragged_x: bool                # the last tile column does

    @property
    def T(self) -> int:
        return self.N * self.TY * self.TX

    def image(self, t: int) -> int:
        return t // (self.TY * self.TX)


def _classes(c: Case):
    """[(ymin, xmin, xps, VH, VW)] of the classes of a layer; (IH, IW) = (c.H, c.W) for every kind here."""
    if c.kind == "conv3":
        return [(-1, -1, 1, c.H, c.W)]
    if c.kind == "conv4s2":
        return [(py - 1, px - 1, 2, c.H // 2, c.W // 2) for py in range(2) for px in range(2)]
    if c.kind == "convT":
        return [(py - 1, px - 1, 1, c.H, c.W) for py in range(2) for px in range(2)]
    raise ValueError(c.kind)


def _halo_grid(c: Case, cls, TH: int, TW: int, halo_rows: int, halo_cols: int, whole_tiles_only: bool) -> Grid:
    """Tiles of TH x TW class pixels; a tile is interior when its `halo_rows` x `halo_cols` halo pixels (xps input pixels
    apart, from (ymin, xmin)) lie inside the image -- and, for the v2 kernels, the tile inside the class grid."""
    ymin, xmin, xps, VH, VW = cls
    TY, TX = _ceil_div(VH, TH), _ceil_div(VW, TW)
    interior = []
    for _ in range(c.N):
        for ty in range(TY):
            for tx in range(TX):
                iy0, ix0 = ty * TH * xps + ymin, tx * TW * xps + xmin
                whole = ty * TH + TH <= VH and tx * TW + TW <= VW
                inside = iy0 >= 0 and iy0 + (halo_rows - 1) * xps < c.H and ix0 >= 0 and ix0 + (halo_cols - 1) * xps < c.W
                interior.append(inside and (whole or not whole_tiles_only))
    return Grid(c.N, TY, TX, tuple(interior), VH % TH != 0, VW % TW != 0)


def wino43_grid(c: Case) -> Grid:
    """conv_wgrad_wino43_kernel: TY = H / 4 strip rows, SX = ceil((W / 4) / 4) strips of four 4x4 tiles per row,
    S = N TY SX; strip (ty, sx) starts at y0 = 4 ty, x0 = 16 sx and is interior when
    y0 >= 1 and y0 + 5 <= H and x0 >= 1 and x0 + 17 <= W (strip_origin)."""
    assert c.kind == "conv3" and c.H % 4 == 0 and c.W % 4 == 0 and c.Ci % 32 == 0 and c.Co % 96 == 0
    TY, SX = c.H // 4, _ceil_div(c.W // 4, 4)
    interior = []
    for _ in range(c.N):
        for ty in range(TY):
            for sx in range(SX):
                y0, x0 = 4 * ty, 16 * sx
                interior.append(y0 >= 1 and y0 + 5 <= c.H and x0 >= 1 and x0 + 17 <= c.W)
    return Grid(c.N, TY, SX, tuple(interior), False, c.W % 16 != 0)


def grids(c: Case) -> List[Grid]:
    """One Grid per class of the case (all of one case have the same tile count)."""
    f = c.family
    if f == "wino43":
        return [wino43_grid(c)]
    if f in ("wino23_rows", "rows_direct"):
        # conv_wgrad_rows_kernel: tiles of WR_TH = 4 rows x 32 columns on a grid of whole tiles; halo (4 + KH - 1) x (32 + KW - 1)
        k = 3 if c.kind == "conv3" else 2
        out = []
        for cls in _classes(c):
            assert cls[3] % 4 == 0 and cls[4] % 32 == 0 and c.Ci % 32 == 0, "not a shape of the rows kernel"
            out.append(_halo_grid(c, cls, 4, 32, 4 + k - 1, 32 + k - 1, False))
        return out
    if f == "wino32_v1":
        assert wino32_variant(c) == "v1"
        # conv_wgrad32_kernel: regions of G32_TH = 3 x G32_TW = 48; halo G32_HR = 4 rows x G32_HP = 49 pixels
        return [_halo_grid(c, cls, 3, 48, 4, 49, False) for cls in _classes(c)]
    if f in ("wino32_v2", "wino32_v2c96", "wino32_merged"):
        assert wino32_variant(c) in {"wino32_v2": ("v2",), "wino32_v2c96": ("v2c96",), "wino32_merged": ("v2", "v2c96")}[f]
        # h2_workgroup: strips of 3 x 24 (eight 3x3 tiles); halo 4 rows x 28 pixel slots; interior needs the whole strip in the grid
        return [_halo_grid(c, cls, 3, 24, 4, 28, True) for cls in _classes(c)]
    if f == "general":
        # conv_wgrad_kernel: the engine sizes the split count by its 4 x 32 row-tile estimate of the OUTPUT grid; the kernel's own
        # tile height is 4 or less (wgrad_geometry halves it until two buffers fit the LDS), so it has at least as many tiles
        VH, VW = (c.H, c.W) if c.kind == "conv1" else ((c.H + 1) // 2, (c.W + 1) // 2)
        TY, TX = _ceil_div(VH, 4), _ceil_div(VW, 32)
        return [Grid(c.N, TY, TX, (False,) * (c.N * TY * TX), VH % 4 != 0, VW % 32 != 0)]
    raise ValueError(f)


def tiles(c: Case) -> int:
    """T: what the pixel splits of the case divide (the library's tiles / strips query, or the engine's row-tile estimate)."""
    return grids(c)[0].T


def split_counts(c: Case) -> List[int]:
    """{1, 2, 3, 5, 8, 9, 13, T - 1, T} within [1, T]; for the ceil families two more counts in (T / 2, T), which leave
    empty trailing splits (per = 2 there: ceil(T / 2) splits have strips); and the case's own `extra` counts.  Never above
    T: 1 <= nsplit <= T is the engine's contract with the kernels."""
    T = tiles(c)
    ns = {1, 2, 3, 5, 8, 9, 13, T - 1, T} | set(c.extra)
    if PARTITION[c.family] == "ceil":
        ns |= {n for n in (_ceil_div(T, 2) + 2, _ceil_div(T, 2) + 3) if T / 2 < n < T}
    return sorted(n for n in ns if 1 <= n <= T)


def split_tiles(c: Case, nsplit: int) -> List[List[int]]:
    """The tiles of every split, in the order the kernel walks them."""
    T = tiles(c)
    assert 1 <= nsplit <= T
    rule = PARTITION[c.family]
    if rule == "ceil":
        per = _ceil_div(T, nsplit)
        return [list(range(min(i * per, T), min((i + 1) * per, T))) for i in range(nsplit)]
    if rule == "floor":
        per, rem = T // nsplit, T % nsplit
        out = []
        for i in range(nsplit):
            b = i * per + min(i, rem)
            out.append(list(range(b, b + per + (1 if i < rem else 0))))
        return out
    return [list(range(i, T, nsplit)) for i in range(nsplit)]


class Facts(NamedTuple):
    T: int
    sizes: Tuple[int, ...]         # tiles per split
    empty: int                     # splits without a tile
    straddling: int                # splits whose tiles belong to more than one image
    transitions: frozenset         # of "BB", "BI", "IB", "II": consecutive tiles inside a split, over all classes
    launched: int                  # splits in the launched grid (padded to a multiple of 8)

    @property
    def per(self) -> str:
        """tiles per split as the sweep table prints them: 'max' or 'min-max' over the non-empty splits"""
        used = [s for s in self.sizes if s]
        return str(max(used)) if min(used) == max(used) else f"{min(used)}-{max(used)}"


def facts(c: Case, nsplit: int) -> Facts:
    gs = grids(c)
    parts = split_tiles(c, nsplit)
    assert sorted(t for p in parts for t in p) == list(range(gs[0].T)), "the splits cover every tile exactly once"
    trans: Set[str] = set()
    straddling = 0
    for p in parts:
        if len({gs[0].image(t) for t in p}) > 1:
            straddling += 1
        if TWO_STAGING_PATHS[c.family]:
            for g in gs:
                for a, b in zip(p, p[1:]):
                    trans.add("BI"[g.interior[a]] + "BI"[g.interior[b]])
    launched = _ceil_div(nsplit, 8) * 8 if PADS_GRID[c.family] else nsplit
    return Facts(gs[0].T, tuple(len(p) for p in parts), sum(1 for p in parts if not p), straddling, frozenset(trans), launched)


def sweep() -> List[Tuple[Case, int]]:
    return [(c, n) for c in CASES for n in split_counts(c)]


def family_summary(family: str) -> Dict[str, object]:
    """What the family's cases put its kernel through, over all their split counts."""
    s = dict(empty=False, straddling=False, padded=False, odd_above_8=False, single=False, ragged_y=False, ragged_x=False,
             interior=False, border=False, transitions=set())
    for c in cases_of(family):
        gs = grids(c)
        s["single"] |= gs[0].T == 1
        s["ragged_y"] |= gs[0].ragged_y
        s["ragged_x"] |= gs[0].ragged_x
        s["interior"] |= any(any(g.interior) for g in gs)
        s["border"] |= any(not all(g.interior) for g in gs)
        for n in split_counts(c):
            f = facts(c, n)
            s["empty"] |= f.empty > 0
            s["straddling"] |= f.straddling > 0
            s["padded"] |= f.launched > n
            s["odd_above_8"] |= n > 8 and n % 8 != 0
            s["transitions"] |= f.transitions
    return s
