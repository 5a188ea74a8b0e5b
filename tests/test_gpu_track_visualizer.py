"""-m gpu: the HIP track renderer (csrc/render.hip) against the numpy restatement of DESIGN.md "Track rendering" (tests/render_ref.py),
byte for byte; TrackVisualizer end to end behind RcnnTracker; the tracker's CSV and records unchanged by rendering."""
import ctypes as C

import numpy as np
import pytest
import torch

import render_ref as rr

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
LABELS = [b"car 87%\nid: 12", b"55%", b"truck 100%\nid: 3", b"bus 9%\nid: 1234567", b"\xc3\xa9t\xe9 ~{|}\nid: 7"]


def _font():
    from apse_uav_amd import _lib
    buf = (C.c_uint8 * 665)()
    _lib.load().apse_render_font_host(buf, 665)
    return np.frombuffer(bytes(buf), np.uint8)


def _shape_window(rng, h, w):
    yy, xx = np.mgrid[0:h, 0:w]
    kind = rng.integers(0, 3)
    if kind == 0:                                           # ellipse
        cy, cx = rng.uniform(0, h), rng.uniform(0, w)
        ry, rx = rng.uniform(1, h / 1.5 + 1), rng.uniform(1, w / 1.5 + 1)
        return ((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1
    if kind == 1:                                           # rectangle
        y0, x0 = rng.integers(0, h), rng.integers(0, w)
        return (yy >= y0) & (yy < rng.integers(y0, h + 1)) & (xx >= x0) & (xx < rng.integers(x0, w + 1))
    return rng.random((h, w)) < 0.7                         # ragged


def _random_items(rng, H, W, n, images=1):
    items = []
    for k in range(n):
        bw, bh = rng.uniform(2, W / 3), rng.uniform(2, H / 3)
        x0, y0 = rng.uniform(-bw / 2, W - bw / 2), rng.uniform(-bh / 2, H - bh / 2)
        box = np.float32([x0, y0, x0 + bw, y0 + bh])
        it = dict(image=int(k % images), box=box, rgb=tuple(int(v) for v in rng.integers(0, 256, 3)),
                  label=LABELS[k % len(LABELS)], rect=(0, 0, 0, 0), window=None)
        if rng.random() < 0.75:                             # paste-window-like rect around the box, inside the frame
            rx0 = int(np.clip(np.floor(box[0]) - 2, 0, W - 1))
            ry0 = int(np.clip(np.floor(box[1]) - 2, 0, H - 1))
            rx1 = int(np.clip(np.ceil(box[2]) + 2, rx0 + 1, W))
            ry1 = int(np.clip(np.ceil(box[3]) + 2, ry0 + 1, H))
            win = _shape_window(rng, ry1 - ry0, rx1 - rx0)
            if rng.random() < 0.1:
                win[:] = False                              # empty mask: box anchor
            it.update(rect=(rx0, ry0, rx1, ry1), window=win)
        items.append(it)
    return items


def _render_gpu(frames, items, bgr, inplace):
    """apse_render_instances on host frames [B, H, W, 3] -> host result."""
    from apse_uav_amd import _lib
    from apse_uav_amd.utils.track_visualizer import render_scale_breaks
    lib = _lib.load()
    B, H, W, _ = frames.shape
    n = len(items)
    arr = (_lib.RenderItem * max(n, 1))()
    keep, labels = [], b""
    for k, it in enumerate(items):
        a = arr[k]
        a.image = it["image"]
        a.box[:] = [float(v) for v in it["box"]]
        a.rgb[:] = list(it["rgb"]) + [0]
        a.label_off, a.label_len = len(labels), len(it["label"])
        labels += it["label"]
        if it["window"] is not None:
            words = torch.from_numpy(rr.pack_bits(it["window"], it["rect"][0])).to(DEV)
            keep.append(words)
            a.bits = words.data_ptr()
            a.rect[:] = list(it["rect"])
            a.words_per_row = words.shape[1]
    items_dev = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(DEV)
    labels_dev = torch.frombuffer(bytearray(labels + b"\0"), dtype=torch.uint8).to(DEV)
    src = torch.from_numpy(frames).to(DEV)
    out = src if inplace else torch.full_like(src, 3)
    ws_bytes = lib.apse_render_workspace_bytes(H, W, n)
    ws = torch.full((ws_bytes,), 0xAB, dtype=torch.uint8, device=DEV)
    br = render_scale_breaks(H, W)
    _lib.check(lib.apse_render_instances(_lib.ptr(src), _lib.ptr(out), B, H, W, int(bgr), _lib.ptr(items_dev), n,
                                         _lib.ptr(labels_dev), len(labels), _lib.ptr(br), len(br), _lib.ptr(ws), ws_bytes,
                                         _lib.stream_ptr()), None, "apse_render_instances")
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _check(frames, items, bgr, inplace, font):
    got = _render_gpu(frames, items, bgr, inplace)
    want = rr.render(frames, items, bgr, font)
    if not np.array_equal(got, want):
        bad = np.argwhere((got != want).any(axis=3))
        pytest.fail("%d pixels differ, first %s: got %s want %s" % (len(bad), bad[:4].tolist(), got[tuple(bad[0])],
                                                                    want[tuple(bad[0])]))
    return got


@pytest.mark.parametrize("hw", [(217, 389), (375, 1242), (2160, 3840)])
@pytest.mark.parametrize("n", [0, 1, 8, 100])
def test_render_equals_restatement(hw, n):
    H, W = hw
    rng = np.random.default_rng(1000 * n + H)
    font = _font()
    frames = rng.integers(0, 256, (1, H, W, 3), dtype=np.uint8)
    items = _random_items(rng, H, W, n)
    got = _check(frames, items, bgr=bool(n % 2), inplace=False, font=font)
    # out of place: every pixel outside all reaches is the input
    outside = np.ones((H, W), bool)
    for it in items:
        r = rr.reach(it, H, W)
        if r is not None:
            outside[r[1]:r[3], r[0]:r[2]] = False
    assert np.array_equal(got[0][outside], frames[0][outside])
    if n in (8, 100):
        _check(frames, items, bgr=not bool(n % 2), inplace=True, font=font)


@pytest.mark.parametrize("hw", [(217, 389), (375, 1242), (2160, 3840)])
def test_labels_at_all_borders_and_whole_frame_window(hw):
    H, W = hw
    rng = np.random.default_rng(H + W)
    font = _font()
    frames = rng.integers(0, 256, (1, H, W, 3), dtype=np.uint8)
    s = 40
    boxes = [[-30, H / 2, 20, H / 2 + 60], [W / 2, -12, W / 2 + 200, 50], [W - 5, H / 3, W + 40, H / 3 + 100],
             [W / 3, H - 30, W / 3 + 80, H + 10], [-10, -10, s, s], [W - s, H - s, W + 10, H + 10]]
    items = [dict(image=0, box=np.float32(b), rgb=(10 * k, 200, 255 - 30 * k), label=LABELS[k % len(LABELS)], rect=(0, 0, 0, 0),
                  window=None) for k, b in enumerate(boxes)]
    whole = _shape_window(np.random.default_rng(5), H, W) | (np.random.default_rng(6).random((H, W)) < 0.02)
    items.insert(0, dict(image=0, box=np.float32([0, 0, W, H]), rgb=(90, 180, 30), label=b"road 99%\nid: 1", rect=(0, 0, W, H),
                         window=whole))
    for bgr in (False, True):
        for inplace in (False, True):
            _check(frames, items, bgr, inplace, font)


def test_batch2_items_on_both_images():
    H, W = 375, 1242
    rng = np.random.default_rng(7)
    frames = rng.integers(0, 256, (2, H, W, 3), dtype=np.uint8)
    items = _random_items(rng, H, W, 24, images=2)
    _check(frames, items, False, False, _font())
    _check(frames, items, True, True, _font())


def test_odd_width_and_unaligned_windows():
    H, W = 101, 333
    rng = np.random.default_rng(11)
    frames = rng.integers(0, 256, (1, H, W, 3), dtype=np.uint8)
    items = _random_items(rng, H, W, 30)
    _check(frames, items, False, False, _font())


def test_pack_mask_matches_layout():
    from apse_uav_amd import _lib
    H, W = 77, 200
    m = torch.from_numpy(np.random.default_rng(3).random((H, W)) < 0.5)
    words = torch.empty((H, (W + 63) >> 6), dtype=torch.int64, device=DEV)
    dense = m.to(DEV).view(torch.uint8)
    _lib.check(_lib.load().apse_render_pack_mask(_lib.ptr(dense), H, W, _lib.ptr(words), _lib.stream_ptr()), None, "pack")
    torch.cuda.synchronize()
    assert np.array_equal(words.cpu().numpy(), rr.pack_bits(m.numpy(), 0))


# ---------------------------------------------------------------- TrackVisualizer behind the tracker
def _tracker(hw):
    from apse_uav_amd.config import setup_cfg
    from apse_uav_amd.engines.rcnn_tracker import RcnnTracker
    from apse_uav_amd.weights import UAV4K_R101_CLS_BIAS, synthetic_association_state, synthetic_detector_state
    sd = synthetic_detector_state(0, cls_bias=UAV4K_R101_CLS_BIAS)
    return RcnnTracker(setup_cfg(), hw, synthetic_association_state(1), detector_state=sd)


def _expected(frame, objs, meta, font, bgr=False):
    from apse_uav_amd.utils.track_visualizer import create_text_labels, draw_order, track_color
    H, W = frame.shape[:2]
    n = len(objs)
    if n == 0:
        return frame.copy()
    boxes = np.stack([np.asarray(b.tensor[0].cpu(), np.float32) for b in objs.pred_boxes])
    texts = create_text_labels([int(c) for c in objs.pred_classes], [float(s) for s in objs.scores], list(objs.ids),
                               meta["thing_classes"])
    items = []
    for k in draw_order(boxes):
        m = objs.pred_masks[k]
        dense = m.dense().cpu().numpy() if m.bits is not None else None
        items.append(dict(image=0, box=boxes[k], rgb=track_color(objs.ids[k]), label=texts[k].encode("ascii", "replace"),
                          rect=(0, 0, W, H), window=dense))
    return rr.render(frame, items, bgr, font)


@pytest.mark.parametrize("hw", [(2160, 3840), (375, 1242)])
def test_visualizer_end_to_end(hw, logdir):
    from apse_uav_amd.structures.object_instances import ObjectInstances
    from apse_uav_amd.synthetic import SyntheticSequence
    from apse_uav_amd.utils.track_visualizer import TrackVisualizer, visualize_tracks
    meta = {"thing_classes": ["car", "truck", "bus", "van"]}
    font = _font()
    seq = SyntheticSequence("dynamic", *hw)
    frames = [seq.frame(t) for t in range(9)]
    ahead, plain = _tracker(hw), _tracker(hw)
    vis = TrackVisualizer(meta)
    colours, drawn = {}, 0
    for t in range(8):
        objs = ahead.next_frame(frames[t], upcoming=frames[t + 1])          # run-ahead: the next frame's forward is enqueued
        ref_objs = plain.next_frame(frames[t])
        img = vis.draw_instance_predictions(frames[t], objs).get_image()
        want = _expected(frames[t], objs, meta, font)
        assert np.array_equal(img, want), t
        assert np.array_equal(img, _expected(frames[t], ref_objs, meta, font)), t            # this frame's masks
        if len(objs):                                       # a surviving id keeps its colour
            from apse_uav_amd.utils.track_visualizer import draw_order
            items = vis._items(objs, len(objs), *hw)[0]
            order = draw_order(np.stack([np.asarray(bx.tensor[0].cpu(), np.float32) for bx in objs.pred_boxes]))
            for j, k in enumerate(order):
                c = tuple(items[j].rgb)[:3]
                assert colours.setdefault(objs.ids[k], c) == c
        drawn += len(objs)
        bgr = visualize_tracks(np.ascontiguousarray(frames[t][:, :, ::-1]), objs, vis)
        assert np.array_equal(bgr, _expected(np.ascontiguousarray(frames[t][:, :, ::-1]), objs, meta, font, bgr=True))
        # device frame in place
        dev = torch.from_numpy(frames[t]).to(DEV)
        out = vis.draw_instance_predictions(dev, objs, inplace=True)
        assert out.tensor.data_ptr() == dev.data_ptr()
        assert np.array_equal(dev.cpu().numpy(), want)
    empty = ObjectInstances(image_size=hw)
    assert np.array_equal(vis.draw_instance_predictions(frames[0], empty).get_image(), frames[0])
    with open(logdir + "/track_visualizer.log", "a") as f:
        f.write("e2e %s objects drawn over 8 frames: %d, ids seen: %d\n" % (hw, drawn, len(colours)))
    if hw == (2160, 3840):
        assert drawn > 0


def test_csv_and_records_unchanged_by_rendering():
    from apse_uav_amd.synthetic import SyntheticSequence
    from apse_uav_amd.utils.track_visualizer import TrackVisualizer
    hw = (2160, 3840)
    seq = SyntheticSequence("dynamic", *hw)
    a, b = _tracker(hw), _tracker(hw)
    vis = TrackVisualizer({"thing_classes": ["car", "truck", "bus", "van"]})
    for t in range(16):
        f = seq.frame(t)
        oa = a.next_frame(f)
        vis.draw_instance_predictions(f, oa).get_image()
        ob = b.next_frame(f)
        assert a.log_line(oa, 1, t) == b.log_line(ob, 1, t)
        ra, rb = a._last_record, b._last_record
        assert set(ra) == set(rb)
        for k in ra:
            assert np.array_equal(np.asarray(ra[k]), np.asarray(rb[k])), (t, k)
