"""Detections drawn over 8-bit images on the device: box outlines and caption tags by the one kernel of csrc/overlay.hip
(`adh_draw_boxes`, whose contract heads that file and stands in include/adam_dehaze_hip.h), for `main.py --mode demo --detect`
(image_io.dehaze_files).  The reference draws with matplotlib on the host (utils/visualize.py:93-150); here the panel never leaves
the device before it is written.

`draw_boxes` takes a uint8 [N,H,W,C] tensor or a pane view of one, as image_io.image_to_u8 writes them, and one detection dict
per image; colours come from the label (`class_color`), captions are `<label>:<score>` (`caption`) in the 5 x 7 font `FONT_5X7`.
`match_detections` and `summarize_detections` are the host arithmetic of the hazy-against-dehazed comparison."""
from __future__ import annotations

import colorsys
from typing import Dict, Iterable, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _hip as H

FONT_CHARS = "0123456789.:%"
# 7 rows of 5 bits per character of FONT_CHARS, bit 4 the leftmost column
FONT_5X7 = (
    (0b01110, 0b10001, 0b10011, 0b10101, 0b11001, 0b10001, 0b01110),   # 0
    (0b00100, 0b01100, 0b00100, 0b00100, 0b00100, 0b00100, 0b01110),   # 1
    (0b01110, 0b10001, 0b00001, 0b00010, 0b00100, 0b01000, 0b11111),   # 2
    (0b11110, 0b00001, 0b00001, 0b01110, 0b00001, 0b00001, 0b11110),   # 3
    (0b00010, 0b00110, 0b01010, 0b10010, 0b11111, 0b00010, 0b00010),   # 4
    (0b11111, 0b10000, 0b11110, 0b00001, 0b00001, 0b10001, 0b01110),   # 5
    (0b00110, 0b01000, 0b10000, 0b11110, 0b10001, 0b10001, 0b01110),   # 6
    (0b11111, 0b00001, 0b00010, 0b00100, 0b01000, 0b01000, 0b01000),   # 7
    (0b01110, 0b10001, 0b10001, 0b01110, 0b10001, 0b10001, 0b01110),   # 8
    (0b01110, 0b10001, 0b10001, 0b01111, 0b00001, 0b00010, 0b01100),   # 9
    (0b00000, 0b00000, 0b00000, 0b00000, 0b00000, 0b01100, 0b01100),   # .
    (0b00000, 0b01100, 0b01100, 0b00000, 0b01100, 0b01100, 0b00000),   # :
    (0b11000, 0b11001, 0b00010, 0b00100, 0b01000, 0b10011, 0b00011),   # %
)
GOLDEN_RATIO_FRAC = 0.61803398875
MAX_CAPTION = 127            # glyph indices travel as int8 rows; a longer caption is cut


def class_color(label: int) -> Tuple[Tuple[int, int, int], Tuple[int, int, int]]:
    """(box RGB, text RGB) of a class label: hue = frac(label * 0.61803398875) at saturation 0.85 and value 0.95, so that
    neighbouring labels lie far apart; the text is black on a light box (luma (299 R + 587 G + 114 B) / 1000 >= 128), else white."""
    hue = (int(label) * GOLDEN_RATIO_FRAC) % 1.0
    r, g, b = (int(round(v * 255)) for v in colorsys.hsv_to_rgb(hue, 0.85, 0.95))
    text = (0, 0, 0) if (299 * r + 587 * g + 114 * b) / 1000 >= 128 else (255, 255, 255)
    return (r, g, b), text


def caption(label: int, score: float) -> str:
    return f"{int(label)}:{float(score):.2f}"


def encode_caption(s: str) -> List[int]:
    """glyph indices into FONT_5X7; a character the font lacks becomes index len(FONT_5X7), which the kernel leaves blank"""
    return [FONT_CHARS.find(ch) if ch in FONT_CHARS else len(FONT_5X7) for ch in s[:MAX_CAPTION]]


_glyphs: Dict[torch.device, torch.Tensor] = {}


def _font(device) -> torch.Tensor:
    device = torch.device(device)
    if device not in _glyphs:
        _glyphs[device] = torch.tensor(FONT_5X7, dtype=torch.uint8).to(device)
    return _glyphs[device]


def _host(v, dtype):
    return (v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)).astype(dtype)


def pack_detections(dets: Sequence[Dict]) -> Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
    """What one launch takes, on the host: (first int32 [N+1], boxes float32 [M,4], colors uint8 [M,2,3], text int8 [M,T]) from
    one {"boxes" (xyxy), "labels", "scores"} per image; each image's boxes sorted by descending score, ties in their order."""
    first, boxes, colors, rows = [0], [], [], []
    for d in dets:
        b = _host(d["boxes"], np.float32).reshape(-1, 4)
        labels, scores = _host(d["labels"], np.int64).reshape(-1), _host(d["scores"], np.float64).reshape(-1)
        if not (len(b) == len(labels) == len(scores)):
            raise ValueError(f"boxes, labels and scores disagree in length: {len(b)}, {len(labels)}, {len(scores)}")
        for i in np.argsort(-scores, kind="stable"):
            boxes.append(b[i])
            colors.append(class_color(labels[i]))
            rows.append(encode_caption(caption(labels[i], scores[i])))
        first.append(len(boxes))
    T = max((len(r) for r in rows), default=0)
    text = np.full((len(rows), T), -1, np.int8)
    for i, r in enumerate(rows):
        text[i, :len(r)] = r
    return (np.asarray(first, np.int32), np.asarray(boxes, np.float32).reshape(-1, 4),
            np.asarray(colors, np.uint8).reshape(-1, 2, 3), text)


def draw_boxes(u8: torch.Tensor, dets: Sequence[Dict], thickness: int = 2, scale: int = 1, alpha: int = 255) -> torch.Tensor:
    """Draw every image's detections on `u8` in place and return it.  `u8`: uint8 [N,H,W,C] (or [H,W,C]) on the device, C = 3
    or 4, or a view whose last two dimensions are dense, e.g. one pane of a panel; bytes outside the view, and the alpha of
    C = 4, are left alone.  `dets`: one {"boxes" (xyxy, pixels), "labels", "scores"} per image.  Outlines are `thickness` pixels,
    blended by `alpha` / 255; captions `<label>:<score>` sit in an opaque tag above each box, `scale` pixels per font dot.  The
    strongest detection is on top.  One launch for the batch."""
    from .image_io import _u8_view
    view, row_pitch, image_pitch = _u8_view(u8, "draw_boxes image")
    N, h, w, c = view.shape
    if c not in (3, 4):
        raise ValueError(f"draw_boxes takes RGB or RGBA pixels, got C = {c}")
    if len(dets) != N:
        raise ValueError(f"{len(dets)} detection lists for {N} images")
    first, boxes, colors, text = pack_detections(dets)
    if len(boxes) == 0:
        return u8
    dev = view.device
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    first_d, boxes_d, colors_d, text_d, glyphs = up(first), up(boxes), up(colors), up(text), _font(dev)
    H.call("adh_draw_boxes", view.data_ptr(), row_pitch, image_pitch, N, h, w, c, first_d.data_ptr(), len(boxes),
           boxes_d.data_ptr(), colors_d.data_ptr(), text_d.data_ptr(), text.shape[1], glyphs.data_ptr(), glyphs.shape[0],
           int(thickness), int(scale), int(alpha))
    return u8


# ---------------------------------------------------------------------------------------------------------------- comparison
def detection_items(det: Dict) -> List[Dict]:
    """one image's filtered detections ({"boxes_xywh", "labels", "scores"}, detection.filter_detections) as the record's list:
    {"label", "score", "box": [x, y, w, h]}"""
    return [{"label": int(l), "score": float(s), "box": [float(v) for v in b]}
            for b, l, s in zip(det["boxes_xywh"].tolist(), det["labels"].tolist(), det["scores"].tolist())]


def items_to_dets(items: Iterable[Dict]) -> Dict:
    """a record's list back to what `draw_boxes` takes: the drawn corners are (x, y, x + w, y + h) in float32 of the recorded
    numbers, so that a picture can be redrawn from the record alone"""
    items = list(items)
    b = np.asarray([it["box"] for it in items], np.float32).reshape(-1, 4)
    return {"boxes": np.stack([b[:, 0], b[:, 1], b[:, 0] + b[:, 2], b[:, 1] + b[:, 3]], axis=1),
            "labels": np.asarray([it["label"] for it in items], np.int64), "scores": np.asarray([it["score"] for it in items], np.float64)}


def _iou_xywh(p, q) -> float:
    ix = min(p[0] + p[2], q[0] + q[2]) - max(p[0], q[0])
    iy = min(p[1] + p[3], q[1] + q[3]) - max(p[1], q[1])
    inter = max(ix, 0.0) * max(iy, 0.0)
    union = p[2] * p[3] + q[2] * q[3] - inter
    return inter / union if union > 0 else 0.0


def match_detections(a: Sequence[Dict], b: Sequence[Dict], iou: float = 0.5) -> Dict[str, int]:
    """How the detections `b` of an image (the dehazed one) relate to the detections `a` of the same scene (the hazy one); both
    lists of {"label", "score", "box": [x, y, w, h]}.  Greedy in `b`'s score order (descending, ties in list order): a `b`
    detection is matched to the still unmatched `a` detection of its label with the highest IoU at or above `iou` (the first
    such on a tie).  {"matched": pairs, "gained": `b` detections without a partner, "lost": `a` detections without one}."""
    free = list(range(len(a)))
    matched = 0
    for j in sorted(range(len(b)), key=lambda j: -b[j]["score"]):
        best, best_iou = None, float(iou)
        for i in free:
            if a[i]["label"] != b[j]["label"]:
                continue
            v = _iou_xywh(a[i]["box"], b[j]["box"])
            if v >= best_iou and (best is None or v > best_iou):
                best, best_iou = i, v
        if best is not None:
            free.remove(best)
            matched += 1
    return {"matched": matched, "gained": len(b) - matched, "lost": len(a) - matched}


def summarize_detections(records: Iterable[Dict], threshold: float, weights: Optional[Dict] = None) -> Dict:
    """`demo_detections.json`: the threshold, where the detector's weights came from (`detector_checkpoint`,
    `detector_random_init`), and per routed intensity (`by_intensity`) and over all files (`all`): `files`, the mean number of
    detections per file on the hazy input and on the dehazed output, and the summed `matched` / `gained` / `lost` of the
    records' `detect_match`."""
    records = [r for r in records if "detect_counts" in r]

    def entry(rs):
        n = len(rs)
        return {"files": n,
                "mean_hazy": sum(r["detect_counts"]["hazy"] for r in rs) / n if n else None,
                "mean_dehazed": sum(r["detect_counts"]["dehazed"] for r in rs) / n if n else None,
                **{k: sum(r["detect_match"][k] for r in rs) for k in ("matched", "gained", "lost")}}
    weights = weights or {}
    return {"score_threshold": float(threshold), "detector_checkpoint": weights.get("detector_checkpoint"),
            "detector_random_init": weights.get("detector_random_init"),
            "by_intensity": {name: entry([r for r in records if r["intensity"] == name])
                             for name in sorted({r["intensity"] for r in records})},
            "all": entry(records)}
