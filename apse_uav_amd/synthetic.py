"""Synthetic 3840x2160 UAV-like frames (no video ships with the reference).

SURVEY.md 8d: smooth background + K filled rotated rectangles (~250x110 px,
distinct colours).  "static": no motion; "dynamic": linear motion, one vehicle
leaves the frame for a span so blank CSV cells occur (as in
/root/reference/data/dynamic_dcnn_data.csv, blank id_1 cells at frames 867-1212).
Frames are u8 HxWx3 BGR like ``cv2.VideoCapture.read`` returns
(/root/reference/dcnn/scripts/tests/visualize_uav.py:188).
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

COLORS = [(40, 40, 200), (200, 60, 40), (60, 190, 60), (220, 220, 230), (30, 30, 30), (200, 180, 40)]


class SyntheticSequence:
    def __init__(self, kind="static", height=2160, width=3840, n_vehicles=4, seed=1234):
        self.kind, self.h, self.w, self.k = kind, height, width, n_vehicles
        g = torch.Generator().manual_seed(seed)
        sy, sx = height / 2160.0, width / 3840.0
        coarse = torch.rand(1, 3, 34, 60, generator=g) * 120.0 + 60.0
        bg = F.interpolate(coarse, size=(height, width), mode="bilinear", align_corners=False)[0]
        self.bg = bg.permute(1, 2, 0).round().clamp(0, 255).to(torch.uint8).numpy()
        self.veh = []
        for i in range(n_vehicles):
            cx = (0.12 + 0.76 * (i + 0.5) / n_vehicles) * width + float(torch.rand(1, generator=g)) * 40 * sx
            cy = (0.25 + 0.5 * float(torch.rand(1, generator=g))) * height
            ang = (float(torch.rand(1, generator=g)) - 0.5) * 0.6
            vx = (1.0 + float(torch.rand(1, generator=g))) * (1 if i % 2 == 0 else -1) * sx
            vy = (float(torch.rand(1, generator=g)) - 0.5) * sy
            self.veh.append(dict(cx=cx, cy=cy, ang=ang, vx=vx, vy=vy, L=250.0 * sx, Wd=110.0 * sy,
                                 color=COLORS[i % len(COLORS)]))

    def pose(self, v, t, idx):
        if self.kind == "static":
            return v["cx"], v["cy"], True
        cx, cy = v["cx"] + v["vx"] * t, v["cy"] + v["vy"] * t
        visible = not (idx == 1 and 20 <= t < 40)       # vehicle 1 disappears for a span
        return cx, cy, visible

    def boxes(self, t):
        """Axis-aligned boxes (x1, y1, x2, y2) of the visible vehicles in frame t, f32."""
        out = []
        for i, v in enumerate(self.veh):
            cx, cy, vis = self.pose(v, t, i)
            if not vis:
                continue
            c, s = abs(math.cos(v["ang"])), abs(math.sin(v["ang"]))
            hw = 0.5 * (v["L"] * c + v["Wd"] * s)
            hh = 0.5 * (v["L"] * s + v["Wd"] * c)
            out.append([max(cx - hw, 0.0), max(cy - hh, 0.0), min(cx + hw, float(self.w)), min(cy + hh, float(self.h))])
        return np.asarray(out, np.float32).reshape(-1, 4)

    def frame(self, t):
        img = self.bg.copy()
        for i, v in enumerate(self.veh):
            cx, cy, vis = self.pose(v, t, i)
            if not vis:
                continue
            r = 0.5 * math.hypot(v["L"], v["Wd"]) + 2
            x0, x1 = max(int(cx - r), 0), min(int(cx + r) + 1, self.w)
            y0, y1 = max(int(cy - r), 0), min(int(cy + r) + 1, self.h)
            if x1 <= x0 or y1 <= y0:
                continue
            yy, xx = np.mgrid[y0:y1, x0:x1]
            dx, dy = xx + 0.5 - cx, yy + 0.5 - cy
            ca, sa = math.cos(v["ang"]), math.sin(v["ang"])
            u = dx * ca + dy * sa
            w_ = -dx * sa + dy * ca
            inside = (np.abs(u) <= v["L"] / 2) & (np.abs(w_) <= v["Wd"] / 2)
            img[y0:y1, x0:x1][inside] = np.asarray(v["color"], np.uint8)
        return img


def synthetic_dataset(root, n, seed=0, num_classes=4):
    """n generated images (PNG) of three sizes with random box-polygon ground truth -> annotation file path."""
    import json
    import os
    from PIL import Image
    g = np.random.default_rng(seed)
    sizes = [(270, 480), (240, 320), (300, 400)]
    seqs = {s: SyntheticSequence("dynamic", *s) for s in sizes}
    images, anns = [], []
    os.makedirs(root, exist_ok=True)
    for i in range(n):
        h, w = sizes[int(g.integers(0, len(sizes)))]
        name = "%06d.png" % i
        Image.fromarray(seqs[(h, w)].frame(i)[:, :, ::-1].copy()).save(os.path.join(root, name))
        images.append(dict(id=i + 1, file_name=name, height=h, width=w))
        for _ in range(int(g.integers(1, 8))):
            bw, bh = float(g.integers(8, w // 3)), float(g.integers(8, h // 3))
            x, y = float(g.integers(0, w - int(bw))), float(g.integers(0, h - int(bh)))
            anns.append(dict(id=len(anns) + 1, image_id=i + 1, category_id=int(g.integers(0, num_classes)), bbox=[x, y, bw, bh],
                             area=bw * bh, iscrowd=int(g.random() < .02),
                             segmentation=[[x, y, x + bw, y, x + bw, y + bh, x, y + bh]]))
    path = os.path.join(root, "annotations.json")
    with open(path, "w") as fh:
        json.dump(dict(images=images, annotations=anns, categories=[dict(id=c, name="c%d" % c) for c in range(num_classes)]), fh)
    return path


def write_synthetic_mots(root, seqs=("0000", "0001"), frames=14, height=160, width=288):
    """A tiny KITTI MOTS-layout dataset under ``root`` for dry runs of association-head training (tools/
    train_association_head.py --synthetic, the loader tests): <root>/instances_txt/<seq>.txt (one RLE row per visible vehicle,
    ids 1001.. for class 1 and 2001.. for class 2, plus one ignore region, id 10000), <root>/training/image_02/<seq>/%06d.png
    (PIL, RGB) and <root>/train.seqmap.  Frame 1 of every sequence has no objects.  Returns the seqmap path."""
    import os
    from PIL import Image
    from .utils import rle
    os.makedirs(os.path.join(root, "instances_txt"), exist_ok=True)
    lines_map = []
    jit = np.random.default_rng(5)          # per-object box jitter: the same id is seen with different crops
    for s, seq in enumerate(seqs):
        ss = SyntheticSequence("dynamic", height, width, n_vehicles=6, seed=77 + s)
        img_dir = os.path.join(root, "training", "image_02", seq)
        os.makedirs(img_dir, exist_ok=True)
        rows = []
        for t in range(frames):
            Image.fromarray(ss.frame(t)[:, :, ::-1].copy()).save(os.path.join(img_dir, "%06d.png" % t))
            if t == 1:
                continue
            for i, v in enumerate(ss.veh):
                cx, cy, vis = ss.pose(v, t, i)
                if not vis:
                    continue
                sc = jit.uniform(0.5, 1.6, 2)
                cx, cy = cx + jit.uniform(-0.3, 0.3) * v["L"], cy + jit.uniform(-0.3, 0.3) * v["Wd"]
                hw, hh = 0.35 * v["L"] * sc[0], 0.45 * v["Wd"] * sc[1]
                x0, x1 = int(max(cx - hw, 0)), int(min(cx + hw, width))
                y0, y1 = int(max(cy - hh, 0)), int(min(cy + hh, height))
                if x1 - x0 < 2 or y1 - y0 < 2:
                    continue
                m = np.zeros((height, width), np.uint8)
                m[y0:y1, x0:x1] = 1
                cls = 1 if i % 2 == 0 else 2
                rows.append("%d %d %d %d %d %s" % (t, cls * 1000 + 1 + i, cls, height, width, rle.encode(m)["counts"].decode()))
            ign = np.zeros((height, width), np.uint8)
            ign[:8, :16] = 1
            rows.append("%d 10000 10 %d %d %s" % (t, height, width, rle.encode(ign)["counts"].decode()))
        with open(os.path.join(root, "instances_txt", seq + ".txt"), "w") as f:
            f.write("\n".join(rows) + "\n")
        lines_map.append("%s empty %06d %06d" % (seq, 0, frames - 1))
    seqmap = os.path.join(root, "train.seqmap")
    with open(seqmap, "w") as f:
        f.write("\n".join(lines_map) + "\n")
    return seqmap


# ---- YUV 4:2:0 test input (what a decoder would hand out): host numpy, float coefficients.  Test and dry-run input only --
# nothing pins these bytes; the conversion BACK is the library's (structures/yuv_frame.py, tests/yuv_ref.py).
_YUV_KRKB = {"cv601": (0.299, 0.114, False), "bt601": (0.299, 0.114, False), "bt709": (0.2126, 0.0722, False),
             "bt601-full": (0.299, 0.114, True), "bt709-full": (0.2126, 0.0722, True)}


def _bgr_to_yuv420(frame, matrix):
    """HxWx3 uint8 BGR -> (Y [H][W], U [CH][CW], V [CH][CW]) uint8: rint of the float transform, chroma the mean of each 2x2 block
    (edge blocks of an odd frame average the pixels that exist)."""
    kr, kb, full = _YUV_KRKB[matrix]
    f = np.asarray(frame, np.float64)
    b, g, r = f[..., 0], f[..., 1], f[..., 2]
    y = kr * r + (1.0 - kr - kb) * g + kb * b
    u, v = (b - y) / (2.0 * (1.0 - kb)), (r - y) / (2.0 * (1.0 - kr))
    H, W = y.shape
    CH, CW = (H + 1) // 2, (W + 1) // 2

    def pool(c):
        p = np.pad(c, ((0, 2 * CH - H), (0, 2 * CW - W)), mode="edge")
        return p.reshape(CH, 2, CW, 2).mean(axis=(1, 3))
    sy, oy, sc = (1.0, 0.0, 1.0) if full else (219.0 / 255.0, 16.0, 224.0 / 255.0)
    q = lambda a: np.clip(np.rint(a), 0, 255).astype(np.uint8)
    return q(y * sy + oy), q(pool(u) * sc + 128.0), q(pool(v) * sc + 128.0)


def bgr_to_nv12(frame, matrix="cv601", pitch=None):
    """HxWx3 uint8 BGR -> a ``YuvFrame`` (NV12, host) of the same size; ``pitch`` (default: the width rounded up to even) pads the
    rows like a decoder surface, with a byte pattern that is not zero."""
    from .structures.yuv_frame import YuvFrame
    Y, U, V = _bgr_to_yuv420(frame, matrix)
    H, W = Y.shape
    CH, CW = U.shape
    pitch = max(W, 2 * CW) if pitch is None else int(pitch)
    data = np.full((H + CH, pitch), 0x5a, np.uint8)
    data[:H, :W] = Y
    data[H:, 0:2 * CW:2] = U
    data[H:, 1:2 * CW:2] = V
    return YuvFrame(data, W, "NV12")


def bgr_to_i420(frame, matrix="cv601"):
    """HxWx3 uint8 BGR (even H and W) -> a ``YuvFrame`` (I420, host)."""
    from .structures.yuv_frame import YuvFrame
    Y, U, V = _bgr_to_yuv420(frame, matrix)
    H, W = Y.shape
    if (H | W) & 1:
        raise ValueError("I420 needs an even width and height, got %dx%d" % (W, H))
    data = np.concatenate([Y.reshape(-1), U.reshape(-1), V.reshape(-1)]).reshape(3 * H // 2, W)
    return YuvFrame(data, W, "I420")


def encoded_source(get_frame, input_format="BGR", matrix="cv601"):
    """A BGR frame source ``t -> HxWx3`` as one that yields frames in ``input_format`` ("BGR": unchanged; "NV12" / "I420":
    encoded with the functions above) -- how the tools feed synthetic sequences to a run with cfg.INPUT.FORMAT = NV12 / I420."""
    fmt = str(input_format).upper()
    if fmt == "BGR":
        return get_frame
    enc = {"NV12": bgr_to_nv12, "I420": bgr_to_i420}[fmt]
    return lambda t: enc(get_frame(t), matrix)
