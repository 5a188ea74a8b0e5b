"""numpy restatement of DESIGN.md "Track rendering" (test helper; the product never imports it).

``render(frames, items, bgr, font)`` draws items -- dicts with ``image``, ``rect`` (x0, y0, x1, y1), ``window`` (bool
[y1 - y0, x1 - x0] over the rect, or None), ``box`` (4 floats), ``rgb``, ``label`` (bytes) -- in the order given, rule by rule,
with whole-array numpy operations.  The HIP renderer must produce the same bytes.  The label scale comes from the direct f64
formula (utils/track_visualizer.label_scale), not from the renderer's breakpoint table.
"""
import math

import numpy as np

F32 = np.float32
CLAMP = F32(1.0e8)
MAX_LINES = 4


def frame_constants(H, W):
    D = max(math.floor(math.sqrt(H * W) / 90), 10)
    return D, max(D // 4, 1), max(D // 15, 1)


def label_scale(h, H, W):
    D = frame_constants(H, W)[0]
    size = float(np.clip((float(h) / np.sqrt(float(H) * float(W)) - 0.02) / 0.08 + 1, 1.2, 2)) * 0.5 * D
    return max(1, math.floor(size / 9 + 0.5))


def _clampf(v):
    return min(max(F32(v), -CLAMP), CLAMP)


def _round(v):                      # floor(v + 0.5) in f32
    return int(np.floor(_clampf(v) + F32(0.5)))


def _twice(v):                      # floor(2v + 0.5) in f32
    return int(np.floor(F32(2) * _clampf(v) + F32(0.5)))


def mask_rect(item, H, W):
    """The window rect clipped to the frame and the set pixels inside it (bool array over that rect), or None."""
    if item.get("window") is None:
        return None, None
    x0, y0, x1, y1 = item["rect"]
    cx0, cy0, cx1, cy1 = max(x0, 0), max(y0, 0), min(x1, W), min(y1, H)
    if cx0 >= cx1 or cy0 >= cy1:
        return None, None
    win = np.asarray(item["window"], bool)
    return (cx0, cy0, cx1, cy1), win[cy0 - y0:cy1 - y0, cx0 - x0:cx1 - x0]


def layout(item, H, W):
    """Rule 5: dict(s, top, lines=[(left, bytes)], bg, centred, A2) of the item's label (lines empty: no label)."""
    mr, sub = mask_rect(item, H, W)
    M = int(sub.sum()) if sub is not None else 0
    if M > 0:
        ys, xs = np.nonzero(sub)
        xs = xs + mr[0]
        ys = ys + mr[1]
        B = [F32(xs.min()), F32(ys.min()), F32(xs.max() + 1), F32(ys.max() + 1)]
        A2 = [int(round(2 * np.median(xs))), int(round(2 * np.median(ys)))]
        centred = True
    else:
        B = [_clampf(v) for v in item["box"]]
        A2 = [_twice(B[0]), _twice(B[1])]
        centred = False
    bh = F32(B[3] - B[1])
    if F32(F32(B[2] - B[0]) * bh) < F32(1000) or bh < F32(40):
        if B[3] >= F32(H - 5):
            A2 = [_twice(B[2]), _twice(B[1])]
        else:
            A2 = [_twice(B[0]), _twice(B[3])]
    s = label_scale(float(bh), H, W)
    top = A2[1] // 2
    text = item.get("label") or b""
    lines = []
    if text:
        for ln in text.split(b"\n")[:MAX_LINES]:
            w = s * max(6 * len(ln) - 1, 0)
            left = (A2[0] - w) // 2 if centred else A2[0] // 2
            lines.append((left, ln, w))
    bg = None
    if lines:
        bg = (min(l for l, _, _ in lines) - s, top, max(l + w for l, _, w in lines) + s, top + 9 * s * len(lines))
    return dict(s=s, top=top, lines=[(l, t) for l, t, _ in lines], bg=bg, centred=centred, A2=A2, B=B)


def _clip(r, H, W):
    x0, y0, x1, y1 = max(r[0], 0), max(r[1], 0), min(r[2], W), min(r[3], H)
    return (x0, y0, x1, y1) if x0 < x1 and y0 < y1 else None


def _blend(img, sel, c, a):
    px = img[sel]
    img[sel] = (a * np.asarray(c, np.int32) + (256 - a) * px + 128) >> 8


def reach(item, H, W):
    """Frame-clipped union of the box outline, the mask rect and the label background (None: nothing drawn)."""
    _, tb, _ = frame_constants(H, W)
    a = tb // 2
    R = [_round(v) for v in item["box"]]
    rects = [(R[0] - a, R[1] - a, R[2] + a, R[3] + a)]
    mr, _ = mask_rect(item, H, W)
    if mr is not None:
        rects.append(mr)
    bg = layout(item, H, W)["bg"]
    if bg is not None:
        rects.append(bg)
    rects = [c for c in (_clip(r, H, W) for r in rects) if c is not None]
    if not rects:
        return None
    return (min(r[0] for r in rects), min(r[1] for r in rects), max(r[2] for r in rects), max(r[3] for r in rects))


def render(frames, items, bgr, font):
    frames = np.asarray(frames, np.uint8)
    single = frames.ndim == 3
    if single:
        frames = frames[None]
    out = frames.copy()
    Bn, H, W, _ = frames.shape
    _, tb, te = frame_constants(H, W)
    font = np.asarray(font, np.uint8).reshape(95, 7)
    for b in range(Bn):
        img = out[b].astype(np.int32)
        its = [it for it in items if it["image"] == b]
        for it in its:
            c = np.asarray(it["rgb"][:3], np.int32)
            c = c[::-1] if bgr else c
            # rule 2: box outline
            a, bb = tb // 2, tb - tb // 2
            R = [_round(v) for v in it["box"]]
            sel = np.zeros((H, W), bool)
            o = _clip((R[0] - a, R[1] - a, R[2] + a, R[3] + a), H, W)
            if o is not None:
                sel[o[1]:o[3], o[0]:o[2]] = True
                i = _clip((R[0] + bb, R[1] + bb, R[2] - bb, R[3] - bb), H, W)
                if i is not None:
                    sel[i[1]:i[3], i[0]:i[2]] = False
                _blend(img, sel, c, 128)
            # rules 3, 4: fill, then the edge band opaque in the darker colour
            mr, sub = mask_rect(it, H, W)
            if mr is not None and sub.any():
                pad = np.pad(sub, te, constant_values=False)
                er = np.ones_like(sub)
                h, w = sub.shape
                for dy in range(2 * te + 1):
                    for dx in range(2 * te + 1):
                        er &= pad[dy:dy + h, dx:dx + w]
                edge = sub & ~er
                fill = np.zeros((H, W), bool)
                fill[mr[1]:mr[3], mr[0]:mr[2]] = sub & ~edge
                _blend(img, fill, c, 128)
                es = np.zeros((H, W), bool)
                es[mr[1]:mr[3], mr[0]:mr[2]] = edge
                img[es] = (c * 77 + 128) >> 8
        for it in its:
            # rule 5: label background, then glyphs in the lighter colour
            c = np.asarray(it["rgb"][:3], np.int32)
            c = c[::-1] if bgr else c
            light = c + (((255 - c) * 179 + 128) >> 8)
            L = layout(it, H, W)
            if L["bg"] is None:
                continue
            g = _clip(L["bg"], H, W)
            if g is not None:
                sel = np.zeros((H, W), bool)
                sel[g[1]:g[3], g[0]:g[2]] = True
                _blend(img, sel, (0, 0, 0), 205)
            s = L["s"]
            for li, (left, text) in enumerate(L["lines"]):
                y = L["top"] + 9 * s * li + s
                for j, ch in enumerate(text):
                    gi = ch - 32 if 32 <= ch <= 126 else ord("?") - 32
                    x = left + 6 * s * j
                    for gy in range(7):
                        for gx in range(5):
                            if (font[gi, gy] >> (4 - gx)) & 1:
                                r = _clip((x + gx * s, y + gy * s, x + gx * s + s, y + gy * s + s), H, W)
                                if r is not None:
                                    img[r[1]:r[3], r[0]:r[2]] = light
        out[b] = img.astype(np.uint8)
    return out[0] if single else out


def pack_bits(win, x0):
    """bool window over [x0, x0 + w) -> int64 words [h, ((x0 + w + 63) >> 6) - (x0 >> 6)], bit i of word k = column
    ((x0 >> 6) << 6) + 64k + i (WindowMask.bits layout)."""
    win = np.asarray(win, bool)
    h, w = win.shape
    off = x0 & 63
    nw = ((x0 + w + 63) >> 6) - (x0 >> 6)
    full = np.zeros((h, nw * 64), bool)
    full[:, off:off + w] = win
    bits = full.reshape(h, nw, 64).astype(np.uint64) << np.arange(64, dtype=np.uint64)
    return bits.sum(axis=2, dtype=np.uint64).view(np.int64)
