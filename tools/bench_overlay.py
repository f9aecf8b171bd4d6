"""Time the detection overlay of `--mode demo --detect` (csrc/overlay.hip, overlay.draw_boxes) on hazy | dehazed panel buffers with
100 seeded boxes per pane, at 2160 x 7680, 1080 x 3840 and 512 x 2048, and in the same run, alternated with it, the two routes it
replaces:

  * `kernel`            the two launches (one per pane view) with the box lists already on the device, opaque (alpha 255) and
                        blended (alpha 128); `draw_boxes` adds packing the lists on the host and their five small uploads
  * `torch_slices`      the same picture by torch slice assignments on the device: per box, lowest score first, four edge
                        strips and a caption patch (rendered on the host once, outside the timing, and uploaded); compared with
                        the kernel's bytes once per size
  * `pil_host`          PIL.ImageDraw on the host: rectangle outlines, tag rectangles and `draw.text` in Pillow's default font
                        (a like-for-like amount of drawing, not the same pixels)
  * `copy_back`         the device-to-host copy of the panel, which writing the file needs on every route; `pil_route` is
                        copy_back + pil_host, `kernel_route` is kernel + copy_back

Also recorded: the pixels the kernel covers and the image bytes it writes and reads (3 per covered pixel written; 3 per outline
pixel read when blending, none when opaque), counted by drawing white on a black panel, the tiles that hold a survivor, and the
bytes of box records the cull reads (16 per box and tile).  Device events around back-to-back calls, warm-up first, samples
alternated; the host routes by a host clock around work that ends in a synchronise.

    python tools/bench_overlay.py [--rounds 5] [--out profiles/bench_overlay.json]

Prints one JSON object (and writes it to --out when given)."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from adam_dehaze_amd import _hip as H  # noqa: E402
from adam_dehaze_amd import overlay as O  # noqa: E402

SIZES = [(2160, 3840), (1080, 1920), (512, 1024)]      # one pane; the panel is twice as wide
BOXES = 100
THICKNESS, SCALE = 2, 1
TILE = (16, 64)                                         # OVL_TH, OVL_TW of csrc/overlay.hip


def _dets(h, w, seed):
    """100 boxes of 4 .. 40 % of the pane's sides, inside the frame, scores descending from a seed"""
    g = np.random.default_rng(seed)
    bw, bh = g.uniform(0.04, 0.4, BOXES) * w, g.uniform(0.04, 0.4, BOXES) * h
    x1, y1 = g.uniform(0, w - bw), g.uniform(12, h - bh)
    return {"boxes": np.stack([x1, y1, x1 + bw, y1 + bh], axis=1).astype(np.float32), "labels": g.integers(1, 91, BOXES),
            "scores": np.sort(g.uniform(0.5, 1.0, BOXES))[::-1].copy()}


def _time_us(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / n


def _host_us(fn, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6 / n


class Pane:
    """one pane's lists on the device and the raw launch on a view"""

    def __init__(self, det, dev):
        self.first, self.boxes, self.colors, self.text = O.pack_detections([det])
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        self.d = [up(self.first), up(self.boxes), up(self.colors), up(self.text)]
        self.glyphs = O._font(dev)

    def launch(self, view, alpha, colors=None):
        h, w = view.shape[1], view.shape[2]
        H.call("adh_draw_boxes", view.data_ptr(), view.stride(1), view.stride(0), 1, h, w, 3, self.d[0].data_ptr(), BOXES,
               self.d[1].data_ptr(), (self.d[2] if colors is None else colors).data_ptr(), self.d[3].data_ptr(), self.text.shape[1],
               self.glyphs.data_ptr(), self.glyphs.shape[0], THICKNESS, SCALE, alpha)


def _geometry(b, h, w):
    x1, y1, x2, y2 = (float(v) for v in b)
    clamp = lambda v, hi: max(0, min(int(v), hi))
    return clamp(np.floor(x1), w - 1), clamp(np.ceil(x2) - 1, w - 1), clamp(np.floor(y1), h - 1), clamp(np.ceil(y2) - 1, h - 1)


def _patches(pane, dev):
    """per box the caption tag as a small uint8 image on the device, rendered from FONT_5X7 on the host"""
    out = []
    for m in range(BOXES):
        row = [int(v) for v in pane.text[m] if v >= 0]
        tag = np.empty((9 * SCALE, SCALE * (6 * len(row) + 1), 3), np.uint8)
        tag[:] = pane.colors[m, 0]
        for k, gi in enumerate(row):
            for v in range(7):
                for r in range(5):
                    if gi < len(O.FONT_5X7) and (O.FONT_5X7[gi][v] >> (4 - r)) & 1:
                        y, x = SCALE * (1 + v), SCALE * (1 + 6 * k + r)
                        tag[y:y + SCALE, x:x + SCALE] = pane.colors[m, 1]
        out.append(torch.from_numpy(tag).to(dev))
    return out


def _torch_slices(view, pane, patches, colors_dev):
    """the kernel's picture at alpha 255 by slice assignments: boxes from the last to the first, so the first ends on top"""
    h, w = view.shape[1], view.shape[2]
    img, t = view[0], THICKNESS
    for m in range(BOXES - 1, -1, -1):
        x0, x1, y0, y1 = _geometry(pane.boxes[m], h, w)
        c = colors_dev[m, 0]
        img[y0:min(y0 + t, y1 + 1), x0:x1 + 1] = c
        img[max(y1 - t + 1, y0):y1 + 1, x0:x1 + 1] = c
        img[y0:y1 + 1, x0:min(x0 + t, x1 + 1)] = c
        img[y0:y1 + 1, max(x1 - t + 1, x0):x1 + 1] = c
        p = patches[m]
        r0 = y0 - p.shape[0] if y0 - p.shape[0] >= 0 else y0
        ph, pw = min(p.shape[0], h - r0), min(p.shape[1], w - x0)
        img[r0:r0 + ph, x0:x0 + pw] = p[:ph, :pw]


def _pil(host_panel, dets, w):
    from PIL import Image, ImageDraw
    im = Image.fromarray(host_panel)
    draw = ImageDraw.Draw(im)
    for side, det in enumerate(dets):
        for m in range(BOXES - 1, -1, -1):
            x1, y1, x2, y2 = (float(v) for v in det["boxes"][m])
            box, ink = O.class_color(det["labels"][m])
            cap = O.caption(det["labels"][m], det["scores"][m])
            draw.rectangle([side * w + x1, y1, side * w + x2 - 1, y2 - 1], outline=box, width=THICKNESS)
            draw.rectangle([side * w + x1, y1 - 9, side * w + x1 + 6 * len(cap), y1 - 1], fill=box)
            draw.text((side * w + x1 + 1, y1 - 10), cap, fill=ink)
    return np.asarray(im)


def _measure(h, w, rounds, dev):
    dets = [_dets(h, w, 1), _dets(h, w, 2)]
    panes = [Pane(d, dev) for d in dets]
    g = torch.Generator(device=dev).manual_seed(0)
    panel = torch.randint(0, 256, (1, h, 2 * w, 3), dtype=torch.uint8, device=dev, generator=g)
    views = [panel[:, :, :w], panel[:, :, w:]]
    # what the kernel touches: white on black
    black = torch.zeros_like(panel)
    white = torch.full((BOXES, 2, 3), 255, dtype=torch.uint8, device=dev)
    for v, p in zip((black[:, :, :w], black[:, :, w:]), panes):
        p.launch(v, 255, colors=white)
    hit = black[0].any(dim=2)
    covered = int(hit.sum())
    th, tw = TILE
    pad = torch.zeros((-(-h // th) * th, -(-2 * w // tw) * tw), dtype=torch.bool, device=dev)
    pad[:h, :2 * w] = hit
    tiles_hit = int(pad.view(pad.shape[0] // th, th, pad.shape[1] // tw, tw).any(dim=3).any(dim=1).sum())
    tiles = 2 * (-(-h // th)) * (-(-w // tw))
    # the blended launch reads the outline pixels only: draw the tags black, the outlines white
    black.zero_()
    ring = white.clone()
    ring[:, 1] = 0
    tagless = [Pane(dict(d), dev) for d in dets]
    for v, p in zip((black[:, :, :w], black[:, :, w:]), tagless):
        p.d[3] = torch.full_like(p.d[3], -1)                                # no captions: outlines alone
        p.launch(v, 255, colors=white)
    outline_only = int(black[0].any(dim=2).sum())
    # the torch route draws the same bytes (alpha 255)
    patches = [_patches(p, dev) for p in panes]
    a, b = panel.clone(), panel.clone()
    for k in (0, 1):
        panes[k].launch((a[:, :, :w], a[:, :, w:])[k], 255)
        _torch_slices((b[:, :, :w], b[:, :, w:])[k], panes[k], patches[k], panes[k].d[2])
    same = bool(torch.equal(a, b))
    host_panel = panel[0].cpu().numpy()
    fns = {
        "kernel_alpha255": (_time_us, lambda: [p.launch(v, 255) for v, p in zip(views, panes)]),
        "kernel_alpha128": (_time_us, lambda: [p.launch(v, 128) for v, p in zip(views, panes)]),
        "draw_boxes": (_host_us, lambda: [O.draw_boxes(v, [d], THICKNESS, SCALE, 255) for v, d in zip(views, dets)]),
        "torch_slices": (_host_us, lambda: [_torch_slices(v, p, pt, p.d[2]) for v, p, pt in zip(views, panes, patches)]),
        "copy_back": (_host_us, lambda: panel.cpu()),
        "pil_host": (_host_us, lambda: _pil(host_panel, dets, w)),
    }
    calls = {"kernel_alpha255": 50, "kernel_alpha128": 50, "draw_boxes": 10, "torch_slices": 3, "copy_back": 3, "pil_host": 2}
    for k, (timer, fn) in fns.items():
        timer(fn, 2)
    us = {k: [] for k in fns}
    for _ in range(rounds):
        for k, (timer, fn) in fns.items():
            us[k].append(timer(fn, calls[k]))
    med = {k: statistics.median(v) for k, v in us.items()}
    return {"panel": {"H": h, "W": 2 * w, "bytes": h * 2 * w * 3}, "boxes_per_pane": BOXES, "thickness": THICKNESS, "scale": SCALE,
            "torch_slices_equal_kernel_bytes": same,
            "kernel_touches": {"covered_pixels": covered,
                               "outline_pixels_without_captions": outline_only, "image_bytes_written": 3 * covered,
                               "image_bytes_read_alpha255": 0, "image_bytes_read_alpha128_at_most": 3 * outline_only,
                               "tiles": tiles, "tiles_with_a_survivor_at_least": tiles_hit, "box_record_bytes_read_by_the_cull": 16 * BOXES * tiles,
                               "share_of_panel_bytes_written": round(3 * covered / (h * 2 * w * 3), 5)},
            "us": {k: {"median": round(med[k], 1), "min": round(min(v), 1), "max": round(max(v), 1), "timer": fns[k][0].__name__.strip("_")}
                   for k, v in us.items()},
            "routes_us": {"kernel_route": round(med["kernel_alpha255"] + med["copy_back"], 1),
                          "draw_boxes_route": round(med["draw_boxes"] + med["copy_back"], 1),
                          "torch_route": round(med["torch_slices"] + med["copy_back"], 1),
                          "pil_route": round(med["copy_back"] + med["pil_host"], 1)},
            "ratios": {"torch_slices_over_kernel": round(med["torch_slices"] / med["kernel_alpha255"], 1),
                       "torch_slices_over_draw_boxes": round(med["torch_slices"] / med["draw_boxes"], 2),
                       "pil_host_over_kernel": round(med["pil_host"] / med["kernel_alpha255"], 1),
                       "pil_host_over_draw_boxes": round(med["pil_host"] / med["draw_boxes"], 2)}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5, help="samples per variant, alternated")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_overlay.py needs the GPU: there is no CPU timing to report")
    dev = "cuda:0"
    res = {"samples": a.rounds, "sizes": [_measure(h, w, a.rounds, dev) for h, w in SIZES]}
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
