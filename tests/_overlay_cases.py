"""The case table of adh_draw_boxes, shared by tests/test_overlay_hostemu_cpu.py and tests/test_gpu_overlay.py (not a test file).
A case is a dict: the geometry (N, H, W, C, row_pitch `rp`, image_pitch `ip`, `off` bytes in front of the first pixel), the launch
arguments (first, boxes, colors, text, glyphs, thickness, scale, alpha) and a seed for its pixels.  `block` lays a case out as a
byte block that is POISON everywhere outside the addressed pixels; `expected` is that block after the call by the reference of
tests/_overlay_ref.py, poison included, so one comparison checks the drawn bytes, the untouched ones and the alpha bytes.

Frames are 37 x 53 (one tile column, three tile rows of 16) and 16 x 16; 70 x 130 once, for a second and third tile column."""
import numpy as np

from adam_dehaze_amd.overlay import FONT_5X7
from tests._image_io_cases import layout
from tests._overlay_ref import draw_boxes_ref

POISON = 0x5A
H0, W0 = 37, 53
FONT = np.asarray(FONT_5X7, np.uint8)


def _colors(g, M):
    return g.integers(0, 256, (M, 2, 3), dtype=np.uint8)


def _text(rows, T=None):
    T = max([len(r) for r in rows] + [1]) if T is None else T
    t = np.full((len(rows), T), -1, np.int8)
    for i, r in enumerate(rows):
        t[i, :len(r)] = r
    return t


def _case(name, boxes, text=None, glyphs=FONT, N=1, H=H0, W=W0, C=3, rpad=0, ipad=0, off=0, rp=None, first=None, thickness=2,
          scale=1, alpha=255, seed=0, colors=None):
    boxes = np.asarray(boxes, np.float32).reshape(-1, 4)
    M = len(boxes)
    g = np.random.default_rng(1000 + seed)
    rp = W * C + rpad if rp is None else rp
    return {"name": name, "N": N, "H": H, "W": W, "C": C, "rp": rp, "ip": H * rp + ipad, "off": off,
            "first": np.asarray([0, M] if first is None else first, np.int32), "boxes": boxes,
            "colors": _colors(g, M) if colors is None else np.asarray(colors, np.uint8), "text": text, "glyphs": glyphs,
            "thickness": thickness, "scale": scale, "alpha": alpha, "seed": seed}


GEOMETRIES = [(10.0, 12.0, 40.0, 30.0),                 # inside the frame
              (0.0, 0.0, W0, H0),                       # the whole frame
              (-5.0, 8.0, 20.0, 20.0), (30.0, 5.0, 60.0, 15.0), (5.0, -4.0, 25.0, 9.0), (8.0, 28.0, 30.0, 45.0),   # over each edge
              (-9.0, -9.0, 99.0, 99.0),                 # over all four
              (12.0, 3.0, 20.0, 11.0), (12.5, 3.5, 20.5, 11.5), (3.0, 20.5, 9.5, 27.0),                            # exact .0 and .5
              (40.0, 10.0, 43.0, 30.0), (5.0, 31.0, 30.0, 33.5)]                                                   # narrower than 2 t
SKIPPED = [(10.0, 10.0, 10.0, 20.0), (10.0, 10.0, 20.0, 10.0), (20.0, 10.0, 10.0, 20.0), (10.0, 20.0, 20.0, 10.0),  # zero-area, inverted
           (np.nan, 1.0, 20.0, 20.0), (1.0, 1.0, np.nan, 20.0), (1.0, np.inf, 20.0, 30.0), (-np.inf, 1.0, 20.0, 20.0),
           (1.0, 1.0, np.inf, 20.0), (1.0, -np.inf, 20.0, np.inf)]
HUGE = [(-1e30, 5.0, 1e30, 9.0), (3.0, -3e9, 7.0, 3e9), (2147483648.0, 1.0, 4294967296.0, 9.0)]   # finite, far outside an int


def _captions(g, M, G=len(FONT), longest=7):
    return _text([list(g.integers(0, G, g.integers(1, longest + 1))) for _ in range(M)])


def cases():
    g = np.random.default_rng(7)
    out = []
    # every geometry on its own, plain and with a caption, C 3 and 4, thickness 1, 2, 3
    for i, b in enumerate(GEOMETRIES):
        out.append(_case(f"geometry{i}", [b], C=3 + i % 2, thickness=1 + i % 3, seed=i))
        out.append(_case(f"geometry{i}_caption", [b], text=_captions(g, 1), C=4 - i % 2, thickness=1 + (i + 1) % 3, seed=i))
    out.append(_case("skipped_boxes_draw_nothing", SKIPPED, text=_captions(g, len(SKIPPED)), seed=20))
    out.append(_case("skipped_between_drawn", [GEOMETRIES[0]] + SKIPPED[:5] + [GEOMETRIES[7]] + SKIPPED[5:] + [GEOMETRIES[2]],
                     text=_captions(g, 3 + len(SKIPPED)), seed=21))
    out.append(_case("finite_but_huge", HUGE, text=_captions(g, len(HUGE)), seed=22))
    # layering: three boxes overlapping in a fixed order, outlines over tags over outlines; and the reverse order
    three = [(8.0, 14.0, 34.0, 30.0), (15.0, 10.0, 45.0, 24.0), (4.0, 18.0, 28.0, 35.0)]
    for alpha in (255, 128, 0):
        out.append(_case(f"three_overlapping_alpha{alpha}", three, text=_captions(g, 3), alpha=alpha, thickness=3, seed=30))
        out.append(_case(f"three_overlapping_reversed_alpha{alpha}", three[::-1], text=_captions(g, 3), alpha=alpha, C=4, seed=31))
    # pitches: dense, padded, an odd base; the right pane of a 37 x 106 panel
    for C in (3, 4):
        out.append(_case(f"padded_rows_odd_base_C{C}", three, text=_captions(g, 3), C=C, rpad=5, off=3, alpha=128, seed=40 + C))
        out.append(_case(f"right_pane_of_a_panel_C{C}", three + [(0.0, 0.0, W0, H0)], text=_captions(g, 4), C=C, rp=2 * W0 * C,
                         off=W0 * C, seed=42 + C))
    # N = 2 with image_pitch slack, one image without boxes; then first entries out of range, which the device clamps
    out.append(_case("two_images_second_empty", three, text=_captions(g, 3), N=2, ipad=7, rpad=1, off=1, first=[0, 3, 3], seed=50))
    out.append(_case("two_images_first_empty", three, text=_captions(g, 3), N=2, ipad=8, first=[0, 0, 3], C=4, seed=51))
    out.append(_case("three_images_split", three + GEOMETRIES[:4], text=_captions(g, 7), N=3, ipad=3, first=[0, 2, 3, 7], seed=52))
    out.append(_case("first_is_clamped", three, text=_captions(g, 3), N=2, first=[-4, 2, 99], seed=53))
    out.append(_case("first_decreasing_draws_nothing", three, text=_captions(g, 3), N=2, first=[3, 1, 0], seed=54))
    # 300 boxes over one tile (the LDS list holds 256: two chunks), random order of sizes; with and without blending
    many = np.stack([g.uniform(-3, 30, 300), g.uniform(-3, 10, 300), g.uniform(10, 60, 300), g.uniform(4, 20, 300)], axis=1)
    for alpha in (255, 128):
        out.append(_case(f"300_boxes_alpha{alpha}", many, text=_captions(g, 300, longest=4), alpha=alpha, thickness=1, seed=60))
    # the 257th box is the only one that covers the bottom tile row: a survivor of the second chunk alone
    tail = np.concatenate([np.tile([[2.0, 1.0, 50.0, 9.0]], (256, 1)), [[5.0, 33.0, 30.0, 36.5]], [[1.0, 30.0, 40.0, 37.0]]])
    out.append(_case("second_chunk_alone", tail, text=_captions(g, 258, longest=3), alpha=128, seed=61))
    # tags: above the box; forced inside (y_lo < 9 scale); truncated at the right and at the bottom; scale 1 and 2
    for scale in (1, 2):
        out.append(_case(f"tag_above_scale{scale}", [(4.0, 20.0, 50.0, 34.0)], text=_captions(g, 1, longest=3), scale=scale, seed=70))
        out.append(_case(f"tag_inside_scale{scale}", [(4.0, 9.0 * scale - 1, 50.0, 36.0)], text=_captions(g, 1, longest=3),
                         scale=scale, seed=71))
        out.append(_case(f"tag_cut_at_the_right_scale{scale}", [(38.0, 20.0, 50.0, 30.0)], text=_text([[1, 2, 3, 4, 5, 6, 7]]),
                         scale=scale, seed=72))
        out.append(_case(f"tag_cut_at_the_bottom_scale{scale}", [(3.0, 8.0, 40.0, 14.0)], text=_text([[8, 9, 0]]), H=16, W=16 + 21 * scale,
                         scale=scale, thickness=1, seed=73))
    out.append(_case("tag_at_row_zero_exactly", [(4.0, 9.0, 50.0, 30.0)], text=_text([[1, 11, 10, 12]]), seed=74))
    out.append(_case("tag_wider_than_the_box", [(20.0, 20.0, 24.0, 30.0)], text=_text([[1, 2, 3, 4]]), alpha=128, seed=75))
    # captions: len 0, all negative, a terminator in the middle, T = 0, no text at all, indices at and above G, G = 0
    out.append(_case("len_zero_has_no_tag", three, text=_text([[], [3], []], T=4), seed=80))
    out.append(_case("terminator_in_the_middle", three, text=np.asarray([[1, -1, 5, 6], [-7, 1, 2, 3], [4, 5, -128, 9]], np.int8), seed=81))
    out.append(_case("T_zero", three, text=np.zeros((3, 0), np.int8), seed=82))
    out.append(_case("no_text", three, text=None, seed=83))
    out.append(_case("no_text_no_glyphs", three, text=None, glyphs=None, seed=83))
    out.append(_case("glyph_index_at_and_above_G", three, text=_text([[13, 1, 127], [1, 14, 2], [12, 13, 12]]), scale=2, seed=84))
    out.append(_case("G_zero_gives_blank_tags", three, text=_captions(g, 3), glyphs=np.zeros((0, 7), np.uint8), seed=85))
    out.append(_case("G_zero_no_glyphs", three, text=_captions(g, 3), glyphs=None, seed=85))
    # random glyph bitmaps (every bit of the low five, and the three high bits, which no column reads)
    rnd = g.integers(0, 256, (40, 7), dtype=np.uint8)
    out.append(_case("random_glyphs", three + GEOMETRIES[2:6], text=_captions(g, 7, G=40), glyphs=rnd, C=4, alpha=128, seed=86))
    out.append(_case("random_glyphs_scale3", [(1.0, 30.0, 50.0, 36.0)], text=_captions(g, 1, G=40, longest=2), glyphs=rnd, scale=3, seed=87))
    # the small frame; one pixel; a single row and a single column
    out.append(_case("frame16", [(2.0, 10.0, 14.0, 15.0), (0.0, 0.0, 16.0, 16.0)], text=_text([[1], [2, 3]]), H=16, W=16, seed=90))
    out.append(_case("frame16_thick", [(1.0, 1.0, 15.0, 15.0)], H=16, W=16, thickness=9, alpha=128, seed=91))
    out.append(_case("one_pixel", [(0.0, 0.0, 1.0, 1.0)], text=_text([[5]]), H=1, W=1, C=4, off=1, seed=92))
    out.append(_case("one_row", [(3.0, 0.0, 30.0, 1.0)], text=_text([[5, 6]]), H=1, seed=93))
    out.append(_case("one_column", [(0.0, 3.0, 1.0, 30.0)], text=_text([[5, 6]]), W=1, rpad=2, seed=94))
    # three tile columns and five tile rows: boxes across the tile borders at x = 64, 128 and y = 16 .. 64
    wide = [(60.0, 12.0, 70.0, 20.0), (2.0, 2.0, 129.5, 69.0), (63.0, 15.0, 65.0, 17.0), (100.0, 40.0, 140.0, 80.0), (20.0, 30.0, 110.0, 50.0)]
    out.append(_case("three_tile_columns", wide, text=_captions(g, 5), H=70, W=130, alpha=128, thickness=3, seed=95))
    out.append(_case("three_tile_columns_two_images", wide, text=_captions(g, 5), N=2, H=70, W=130, C=4, scale=2, first=[0, 2, 5], ipad=5,
                     off=3, seed=96))
    # huge thickness and scale: a filled box, and a tag that is one solid block
    out.append(_case("huge_thickness_and_scale", three, text=_captions(g, 3), thickness=2 ** 31 - 1, scale=2 ** 31 - 1, alpha=128, seed=97))
    names = [c["name"] for c in out]
    assert len(set(names)) == len(names)
    return out


def pixels(case):
    """the seeded pixels of a case, uint8 [N,H,W,C]"""
    return np.random.default_rng(case["seed"]).integers(0, 256, (case["N"], case["H"], case["W"], case["C"]), dtype=np.uint8)


def block(case):
    """(the byte block before the call: POISON with the pixels laid in; the block index of byte (n, y, x, c))"""
    size, idx = layout(case["N"], case["H"], case["W"], case["C"], case["rp"], case["ip"], case["off"])
    blk = np.full(size, POISON, np.uint8)
    blk[idx] = pixels(case)
    return blk, idx


def expected(case):
    """the block after the call, and how many pixels some box covers"""
    blk, idx = block(case)
    drawn, covered = draw_boxes_ref(pixels(case), case["first"], case["boxes"], case["colors"], case["text"], case["glyphs"],
                                    case["thickness"], case["scale"], case["alpha"])
    if case["C"] == 4:
        assert np.array_equal(drawn[..., 3], pixels(case)[..., 3])
    blk[idx] = drawn
    return blk, int(covered.sum())


def launch_args(case):
    """(T, G) of a case"""
    return (0 if case["text"] is None else case["text"].shape[1]), (0 if case["glyphs"] is None else len(case["glyphs"]))


# argument lists adh_draw_boxes must refuse, as changes to a valid call on a 2 x 16 x 16 x 3 block: (name, ints changed, buffers nulled)
REFUSALS = [("null_img", {}, ("img",)), ("null_first", {}, ("first",)), ("null_boxes", {}, ("boxes",)), ("null_colors", {}, ("colors",)),
            ("null_text", {}, ("text",)), ("null_glyphs", {}, ("glyphs",)),
            ("N0", {"N": 0}, ()), ("N-1", {"N": -1}, ()), ("H0", {"H": 0}, ()), ("W0", {"W": 0}, ()), ("H-3", {"H": -3}, ()),
            ("C1", {"C": 1}, ()), ("C2", {"C": 2}, ()), ("C5", {"C": 5}, ()), ("C0", {"C": 0}, ()),
            ("row_pitch_short", {"rp": 16 * 3 - 1}, ()), ("image_pitch_short", {"ip": 16 * 48 - 1}, ()),
            ("thickness0", {"thickness": 0}, ()), ("thickness-1", {"thickness": -1}, ()), ("scale0", {"scale": 0}, ()),
            ("alpha-1", {"alpha": -1}, ()), ("alpha256", {"alpha": 256}, ()), ("M-1", {"M": -1}, ()), ("T-1", {"T": -1}, ()),
            ("G-1", {"G": -1}, ())]
