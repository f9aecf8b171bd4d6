"""The definition of adh_draw_boxes (include/adam_dehaze_hip.h) restated in numpy, pixel by pixel, from its text and not from the
kernel: shared by tests/test_overlay_cpu.py, tests/test_overlay_hostemu_cpu.py, tests/test_gpu_overlay.py and
tests/test_gpu_demo_detect.py (not a test file).  Every quantity is a Python int or an int64 array, so nothing rounds."""
import math

import numpy as np


def box_geometry(box, H, W):
    """(x_lo, x_hi, y_lo, y_hi) of one xyxy box, or None for a box that is skipped"""
    x1, y1, x2, y2 = (float(v) for v in box)
    if not all(math.isfinite(v) for v in (x1, y1, x2, y2)) or x2 <= x1 or y2 <= y1:
        return None
    clamp = lambda v, hi: max(0, min(int(v), hi))
    return clamp(math.floor(x1), W - 1), clamp(math.ceil(x2) - 1, W - 1), clamp(math.floor(y1), H - 1), clamp(math.ceil(y2) - 1, H - 1)


def caption_len(row):
    n = 0
    for v in row:
        if int(v) < 0:
            break
        n += 1
    return n


def draw_boxes_ref(pix, first, boxes, colors, text, glyphs, thickness=2, scale=1, alpha=255):
    """pix uint8 [N,H,W,C] (C = 3 or 4) -> (the drawn copy, bool [N,H,W]: the pixels some box covers).  first: N + 1 ints;
    boxes [M,4]; colors uint8 [M,2,3]; text int8 [M,T] or None; glyphs uint8 [G,7] or None."""
    pix = np.asarray(pix)
    N, H, W, C = pix.shape
    assert pix.dtype == np.uint8 and C in (3, 4)
    boxes = np.asarray(boxes, np.float32).reshape(-1, 4)
    M = boxes.shape[0]
    colors = np.asarray(colors, np.uint8).reshape(M, 2, 3).astype(np.int64)
    text = None if text is None or M == 0 else np.asarray(text, np.int8).reshape(M, -1)
    glyphs = np.zeros((0, 7), np.uint8) if glyphs is None else np.asarray(glyphs, np.uint8).reshape(-1, 7)
    G = glyphs.shape[0]
    out = pix.copy()
    covered = np.zeros((N, H, W), bool)
    Y, X = np.meshgrid(np.arange(H, dtype=np.int64), np.arange(W, dtype=np.int64), indexing="ij")
    t, s = int(thickness), int(scale)
    for n in range(N):
        lo, hi = (max(0, min(int(first[n + k]), M)) for k in (0, 1))
        undecided = np.ones((H, W), bool)
        for m in range(lo, hi):
            g = box_geometry(boxes[m], H, W)
            if g is None:
                continue
            x_lo, x_hi, y_lo, y_hi = g
            outline = (X >= x_lo) & (X <= x_hi) & (Y >= y_lo) & (Y <= y_hi) & \
                ~((X >= x_lo + t) & (X <= x_hi - t) & (Y >= y_lo + t) & (Y <= y_hi - t))
            tag = np.zeros((H, W), bool)
            glyph = np.zeros((H, W), bool)
            ln = 0 if text is None else caption_len(text[m])
            if ln > 0:
                w_t, h_t = s * (6 * ln + 1), 9 * s
                r0, r1 = (y_lo - h_t, y_lo - 1) if y_lo - h_t >= 0 else (y_lo, min(y_lo + h_t - 1, H - 1))
                tag = (X >= x_lo) & (X <= min(x_lo + w_t - 1, W - 1)) & (Y >= r0) & (Y <= r1)
                nx, ny = X - x_lo - s, Y - r0 - s
                ok = tag & (nx >= 0) & (ny >= 0)
                u, v = np.where(ok, nx, 0) // s, np.where(ok, ny, 0) // s
                k, r = u // 6, u % 6
                ok &= (k < ln) & (r < 5) & (v < 7)
                idx = text[m].astype(np.int64)[np.where(ok, k, 0)]          # text[k] >= 0 for k < len
                ok &= idx < G
                if G:
                    rows = glyphs.astype(np.int64)[np.where(ok, idx, 0), np.where(ok, v, 0)]
                    glyph = ok & (((rows >> (4 - np.where(ok, r, 0))) & 1) == 1)
            for mask, kind in ((undecided & glyph, "text"), (undecided & tag & ~glyph, "box"), (undecided & ~tag & outline, "blend")):
                if not mask.any():
                    continue
                c = colors[m, 1 if kind == "text" else 0]
                old = out[n, :, :, :3][mask].astype(np.int64)
                new = np.broadcast_to(c, old.shape) if kind != "blend" else (alpha * c + (255 - alpha) * old + 127) // 255
                out[n, :, :, :3][mask] = new.astype(np.uint8)
            hit = undecided & (tag | outline)
            covered[n] |= hit
            undecided &= ~hit
    return out, covered
