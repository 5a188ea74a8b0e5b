"""Host side of the track renderer: labels, palette, order, scale table, font, and the numpy restatement of the rules on hand-built
cases (DESIGN.md "Track rendering").  No GPU needed."""
import ctypes as C
import math

import numpy as np
import pytest

import render_ref as rr


def _font():
    from apse_uav_amd import _lib
    lib = _lib.load()
    n = lib.apse_render_font_host(None, 0)
    buf = (C.c_uint8 * n)()
    assert lib.apse_render_font_host(buf, n) == n
    return np.frombuffer(bytes(buf), np.uint8)


class _Meta:
    def __init__(self, d):
        self._d = d

    def get(self, k, default=None):
        return self._d.get(k, default)


def test_text_labels_both_metadata_shapes():
    from apse_uav_amd.utils.track_visualizer import create_text_labels
    names = ["car", "truck", "bus", "van"]
    for meta in ({"thing_classes": names}, _Meta({"thing_classes": names})):
        got = create_text_labels([1, 0], [0.876, 0.5], [7, 12], meta.get("thing_classes", None))
        assert got == ["truck 88%\nid: 7", "car 50%\nid: 12"]
    assert create_text_labels([0, 0], [0.994, 0.125], [1, 2], ["car"]) == ["99%", "12%"]
    assert create_text_labels([0], [0.3], [1], None) == ["30%"]
    assert create_text_labels([0], None, [1], names) is None


def test_labels_without_ids_use_index_plus_one():
    import torch
    from apse_uav_amd.structures.instances import Boxes, Instances
    from apse_uav_amd.utils.track_visualizer import TrackVisualizer
    inst = Instances((100, 200))
    inst.pred_boxes = Boxes(torch.tensor([[0, 0, 10, 10], [0, 0, 50, 50]], dtype=torch.float32))
    inst.scores = torch.tensor([0.9, 0.25])
    inst.pred_classes = torch.tensor([2, 1])
    vis = TrackVisualizer({"thing_classes": ["a", "b", "c"]}, device="cpu")
    items, labels, _ = vis._items(inst, 2, 100, 200)
    # the larger box is drawn first; ids are 1-based input positions
    assert labels == [b"b 25%\nid: 2", b"c 90%\nid: 1"]
    assert list(items[0].box) == [0, 0, 50, 50]
    assert items[0].bits is None and items[0].label_off == 0 and items[1].label_off == len(labels[0])


def test_palette_is_stable():
    from apse_uav_amd.utils.track_visualizer import track_color
    cols = [track_color(i) for i in range(1, 200)]
    assert cols == [track_color(i) for i in range(1, 200)]
    assert all(all(0 <= v <= 255 for v in c) for c in cols)
    assert len(set(cols[:20])) == 20
    import colorsys
    h = (0.6180339887498949 * 5) % 1.0
    assert track_color(5) == tuple(int(math.floor(255 * v + 0.5)) for v in colorsys.hsv_to_rgb(h, 0.65, 0.95))


def test_palette_same_across_visualizers():
    from apse_uav_amd.structures.instances import Boxes
    from apse_uav_amd.structures.object_instances import ObjectInstances
    from apse_uav_amd.utils.track_visualizer import TrackVisualizer
    import torch
    objs = ObjectInstances((100, 100))
    objs.set("ids", [4, 9])
    objs.set("pred_boxes", [Boxes(torch.tensor([[0., 0., 5., 5.]])), Boxes(torch.tensor([[0., 0., 9., 9.]]))])
    objs.set("scores", [0.5, 0.6])
    objs.set("pred_classes", [0, 0])
    a = TrackVisualizer({"thing_classes": ["x"]}, device="cpu")._items(objs, 2, 100, 100)[0]
    b = TrackVisualizer({"thing_classes": ["x"]}, device="cpu")._items(objs, 2, 100, 100)[0]
    assert [bytes(i.rgb) for i in a] == [bytes(i.rgb) for i in b]
    from apse_uav_amd.utils.track_visualizer import track_color
    assert tuple(a[0].rgb)[:3] == track_color(9) and tuple(a[1].rgb)[:3] == track_color(4)


def test_draw_order_stable_by_area():
    from apse_uav_amd.utils.track_visualizer import draw_order
    boxes = [[0, 0, 10, 10], [5, 5, 25, 25], [0, 0, 20, 20], [1, 1, 11, 11], [0, 0, 1, 400]]
    assert list(draw_order(boxes)) == [1, 2, 4, 0, 3]
    assert list(draw_order(np.zeros((0, 4)))) == []
    same = [[0, 0, 4, 4]] * 6
    assert list(draw_order(same)) == list(range(6))


@pytest.mark.parametrize("hw", [(217, 389), (375, 1242), (2160, 3840)])
def test_scale_breaks_match_direct_f64(hw):
    from apse_uav_amd.utils.track_visualizer import label_scale, render_scale_breaks
    H, W = hw
    br = render_scale_breaks(H, W)
    assert br.dtype == np.float32 and len(br) <= 64
    for h in range(1, H + 1):
        table = 1 + int(np.count_nonzero(np.float32(h) >= br))
        assert table == label_scale(h, H, W) == rr.label_scale(h, H, W), h
    # fractional f32 heights right at each break
    for b in br[np.isfinite(br)]:
        below = np.nextafter(b, np.float32(-1))
        assert label_scale(float(b), H, W) > label_scale(float(below), H, W)


def test_font_table():
    f = _font().reshape(95, 7)
    assert f.shape == (95, 7) and int(f.max()) < 32
    assert not f[0].any()
    assert all(f[i].any() for i in range(1, 95))
    assert len({bytes(r) for r in f}) == 95


# ---------------------------------------------------------------- the restatement on hand-built cases
def _box_item(box, label=b"50%", image=0):
    return dict(image=image, rect=(0, 0, 0, 0), window=None, box=box, rgb=(200, 40, 10), label=label)


def test_small_object_rule_branches():
    H, W = 200, 300
    # large box: anchor at (x0, y0), left-aligned
    L = rr.layout(_box_item([20.25, 30.5, 120, 130]), H, W)
    assert L["A2"] == [41, 61] and not L["centred"] and L["top"] == 30 and L["lines"][0][0] == 20
    # small by area, away from the bottom: (x0, y1)
    L = rr.layout(_box_item([10, 10, 30, 30]), H, W)
    assert L["A2"] == [20, 60]
    # short (height < 40) but wide: small as well
    L = rr.layout(_box_item([10, 10, 200, 45]), H, W)
    assert L["A2"] == [20, 90]
    # small and touching the bottom band (y1 >= H - 5): (x1, y0)
    L = rr.layout(_box_item([10, 180, 30, 195]), H, W)
    assert L["A2"] == [60, 360]
    L = rr.layout(_box_item([10, 180, 30, 194.5]), H, W)
    assert L["A2"] == [20, 389]


def test_empty_mask_falls_back_to_box_anchor():
    H, W = 120, 160
    it = dict(image=0, rect=(10, 10, 80, 90), window=np.zeros((80, 70), bool), box=[12, 14, 70, 88], rgb=(1, 2, 3), label=b"x")
    L = rr.layout(it, H, W)
    assert not L["centred"] and L["A2"] == [24, 28]


def test_median_even_and_odd_counts():
    H, W = 300, 300
    win = np.zeros((100, 100), bool)
    win[10:60, 20:70] = True                   # 2500 pixels (even): x 30..79, y 20..69 in the frame
    it = dict(image=0, rect=(10, 10, 110, 110), window=win, box=[0, 0, 1, 1], rgb=(1, 2, 3), label=b"ab")
    L = rr.layout(it, H, W)
    assert L["centred"] and L["A2"] == [109, 89]          # medians 54.5, 44.5
    win2 = win.copy()
    win2[99, 99] = True                                   # 2501 pixels (odd): medians are pixels
    L2 = rr.layout(dict(it, window=win2), H, W)
    xs, ys = np.nonzero(win2.T)[0] + 10, np.nonzero(win2)[0] + 10
    assert L2["A2"] == [int(2 * np.median(xs)), int(2 * np.median(ys))]
    assert L2["A2"][0] % 2 == 0 and L2["A2"][1] % 2 == 0
    s = L["s"]
    w = s * (6 * 2 - 1)
    assert L["lines"][0][0] == (109 - w) // 2


@pytest.mark.parametrize("where", ["left", "top", "right", "bottom"])
def test_label_clipped_at_each_border(where):
    H, W = 64, 96
    box = dict(left=[-30, 20, 40, 60], top=[30, -8, 80, 40], right=[90, 10, 140, 60], bottom=[20, 50, 60, 63])[where]
    it = _box_item(box, label=b"truck 99%\nid: 12")
    frame = np.full((H, W, 3), 77, np.uint8)
    out = rr.render(frame, [it], False, _font())
    L = rr.layout(it, H, W)
    bg = L["bg"]
    off = dict(left=bg[0] < 0, top=bg[1] < 0, right=bg[2] > W, bottom=bg[3] > H)
    assert off[where], (where, bg)
    assert out.shape == frame.shape
    x0, y0, x1, y1 = max(bg[0], 0), max(bg[1], 0), min(bg[2], W), min(bg[3], H)
    assert x0 < x1 and y0 < y1
    region = out[y0:y1, x0:x1]
    assert (region != 77).all(axis=2).all()      # background (and glyphs) cover the clipped rect


def test_render_ref_rules_on_tiny_frame():
    H, W = 40, 50
    frame = np.full((H, W, 3), 100, np.uint8)
    it = dict(image=0, rect=(0, 0, 0, 0), window=None, box=[10, 10, 20, 20], rgb=(255, 0, 0), label=b"")
    out = rr.render(frame, [it], False, _font())
    _, tb, _ = rr.frame_constants(H, W)
    assert tb == 2                                     # D = 10
    blended = (128 * np.array([255, 0, 0]) + 128 * 100 + 128) >> 8
    assert (out[9, 9] == blended).all() and (out[10, 10] == blended).all() and (out[11, 11] == 100).all()
    assert (out[20, 20] == blended).all() and (out[21, 21] == 100).all() and (out[15, 19] == blended).all()
    # BGR puts R in byte 2
    assert (rr.render(frame, [it], True, _font())[9, 9] == blended[::-1]).all()
