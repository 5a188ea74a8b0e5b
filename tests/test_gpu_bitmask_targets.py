"""-m gpu: ``apse_mots_remap_windows`` and ``apse_bitmask_targets`` (csrc/bitmask_targets.hip) through utils/COCO_utils.py, against
the numpy restatements of tests/bitmask_ref.py -- byte for byte.

1. remap: windows at the word-boundary placements under identity, Pillow and flipped maps equal the dense gather, every word;
2. targets on the exact lattice equal the reference on every byte (float32 and float64 agree there);
3. targets of 200 seeded boxes per case equal the FLOAT32 reference on every byte; the share of cells where the float32 and the
   float64 reference disagree is a property of the inputs, asserted here without a GPU;
4. rectangles as polygon and as RLE: the share of differing cells is printed, and cells well inside / outside are 1 / 0;
5. RLE dicts written by ``encode_masks``, the WindowMasks they came from and the dense arrays give the same bytes;
8. bad arguments are APSE_E_INVALID, n == 0 is a no-op."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import bitmask_ref as br                                     # noqa: E402
from test_bitmask_targets_host import lattice_cases          # noqa: E402

gpu = pytest.mark.gpu
DEV = "cuda:0"


def window_mask(dense, rect=None):
    """A WindowMask of ``dense`` over ``rect`` (default: its bounding box; an all-zero mask: the empty window)."""
    from apse_uav_amd.structures.window_mask import WindowMask
    from apse_uav_amd.utils.mots_evaluation import _repack
    if rect is None:
        ys, xs = np.nonzero(dense)
        if len(ys) == 0:
            return WindowMask(None, (0, 0, 0, 0), dense.shape, (-1, -1), 0)
        rect = (int(xs.min()), int(ys.min()), int(xs.max()) + 1, int(ys.max()) + 1)
    x0, y0, x1, y1 = rect
    return _repack(dense[y0:y1, x0:x1], rect, dense.shape, DEV)


def expected_words(dense, rect):
    """The words of the window ``rect`` of ``dense``: bit i of word c is pixel ((x0 >> 6) + c) * 64 + i inside the rect, else 0."""
    x0, y0, x1, y1 = rect
    words = ((x1 + 63) >> 6) - (x0 >> 6)
    base = (x0 >> 6) << 6
    px = np.zeros((y1 - y0, words * 64), bool)
    px[:, x0 - base:x1 - base] = dense[y0:y1, x0:x1]
    weights = np.uint64(1) << np.arange(64, dtype=np.uint64)
    return (px.reshape(y1 - y0, words, 64).astype(np.uint64) * weights).sum(axis=2, dtype=np.uint64)


# ---------------------------------------------------------------- 1. remap
def remap_sources(h, w):
    """(dense masks, window rects) with the placements that go wrong at word boundaries."""
    rng = np.random.default_rng(21)
    blob = br.blobs(rng, h, w, 3)
    out = []
    for x0 in (63, 64, 65):                                              # starts around a word boundary, ends on one
        m = np.zeros((h, w), bool)
        m[5:h - 7, x0:128] = blob[0][5:h - 7, x0:128] | (rng.random((h - 12, 128 - x0)) < 0.3)
        m[5, x0] = m[h - 8, 127] = True
        out.append((m, (x0, 5, 128, h - 7)))
    out.append((np.zeros((h, w), bool), None))                           # the empty window
    one = np.zeros((h, w), bool)
    one[h // 2, 64] = True
    out.append((one, None))                                              # one pixel
    full = blob[1].copy()
    full[0, :] = full[-1, :] = full[:, 0] = full[:, -1] = True
    out.append((full, (0, 0, w, h)))                                     # touches all four edges
    out.append((blob[2], None))
    rect = np.zeros((h, w), bool)
    rect[10:40, 20:150] = True
    out.append((rect, None))
    loose = np.zeros((h, w), bool)                                       # a window larger than its pixels
    loose[30:33, 70:75] = True
    out.append((loose, (3, 2, w - 1, h - 2)))
    return out


def remap_maps(h, w):
    from apse_uav_amd.utils.COCO_utils import nearest_maps
    maps = {"identity": ((h, w), np.arange(w), np.arange(h))}
    for oh, ow in ((60, 100), (150, 250)):
        maps["pillow %dx%d" % (oh, ow)] = ((oh, ow), nearest_maps(w, ow), nearest_maps(h, oh, vertical=True))
    maps["flip before"] = ((60, 100), nearest_maps(w, 100, flip_before=True), nearest_maps(h, 60, vertical=True))
    maps["flip after"] = ((150, 250), nearest_maps(w, 250, flip_after=True), nearest_maps(h, 150, vertical=True))
    maps["flip only"] = ((h, w), np.arange(w)[::-1].copy(), np.arange(h))
    return maps


@gpu
@pytest.mark.parametrize("name", ["identity", "pillow 60x100", "pillow 150x250", "flip before", "flip after", "flip only"])
def test_remap_equals_the_dense_gather_on_every_word(name):
    from apse_uav_amd.structures import device_windows as dw
    from apse_uav_amd.utils import coco as cocomod
    from apse_uav_amd.utils.COCO_utils import DeviceBitmasks
    H, W = 96, 160
    sources = remap_sources(H, W)
    (h, w), xmap, ymap = remap_maps(H, W)[name]
    src = DeviceBitmasks([window_mask(m, r) for m, r in sources], (H, W), DEV)
    assert np.array_equal(cocomod.windows_to_dense(src.windows, H, W), np.stack([m for m, _ in sources]))
    dst = src.transformed((h, w), xmap, ymap)
    torch.cuda.synchronize()
    want = np.stack([br.gather(m, xmap, ymap) for m, _ in sources])
    assert dst.frame_hw == (h, w) and dst.n_obj == len(sources)
    assert np.array_equal(cocomod.windows_to_dense(dst.windows, h, w), want)
    host = dw.read_back(dst.windows)
    assert np.array_equal(host["rect"], dst.host["rect"])
    _, off, total = dw.pool_layout(host["rect"])
    pool = dst.keep[0][:total].cpu().numpy().view(np.uint64)
    for k, rect in enumerate(host["rect"].tolist()):
        x0, y0, x1, y1 = rect
        inside = np.zeros((h, w), bool)
        inside[y0:y1, x0:x1] = True
        assert not (want[k] & ~inside).any(), (k, rect)                  # the host's rect holds every set pixel
        if x1 > x0 and y1 > y0:
            assert np.array_equal(pool[off[k]:off[k + 1]].reshape(y1 - y0, -1), expected_words(want[k], rect)), (k, rect)
        else:
            assert not want[k].any() and int(host["bits"][k]) == 0
    assert not want[3].any() and tuple(host["rect"][3]) == (0, 0, 0, 0)   # an empty source: an empty destination
    assert want[4].sum() >= 1 and want[5][0].all() and want[5][:, -1].all()


@gpu
def test_remap_of_a_kitti_frame():
    from apse_uav_amd.utils import coco as cocomod
    from apse_uav_amd.utils.COCO_utils import DeviceBitmasks, nearest_maps
    H, W, h, w = 375, 1242, 402, 1333
    masks = br.blobs(np.random.default_rng(5), H, W, 3)
    xmap, ymap = nearest_maps(W, w, flip_after=True), nearest_maps(H, h, vertical=True)
    dst = DeviceBitmasks([window_mask(masks[0]), masks[1], window_mask(masks[2])], (H, W), DEV).transformed((h, w), xmap, ymap)
    assert np.array_equal(cocomod.windows_to_dense(dst.windows, h, w), np.stack([br.gather(m, xmap, ymap) for m in masks]))


# ---------------------------------------------------------------- 2. targets, exact lattice
@gpu
@pytest.mark.parametrize("mask_size", [28, 14])
def test_targets_on_the_exact_lattice(mask_size):
    from apse_uav_amd.utils.COCO_utils import DeviceBitmasks, bitmask_targets_device
    masks, rois = lattice_cases()
    bm = DeviceBitmasks([m if k % 2 else window_mask(m) for k, m in enumerate(masks)], masks[0].shape, DEV)
    matched = np.repeat(np.arange(len(masks)), len(rois))
    all_rois = np.tile(rois, (len(masks), 1))
    got = bitmask_targets_device(bm, all_rois, matched, mask_size).cpu().numpy()
    want = br.ref_rows(masks, all_rois, matched, np.float32, mask_size)
    assert np.array_equal(want, br.ref_rows(masks, all_rois, matched, np.float64, mask_size))
    assert got.shape == want.shape and np.array_equal(got, want)
    assert 0 < want.sum() < want.size


# ---------------------------------------------------------------- 3. targets, random
CASES = {"96x160 m28": (96, 160, 28, 31), "96x160 m14": (96, 160, 14, 32), "61x83 m28": (61, 83, 28, 33), "375x1242 m28": (375, 1242, 28, 34)}
DISAGREE_CAP = 0.005


@functools.lru_cache(maxsize=None)
def random_case(name):
    """(dense masks, rois f32 [200][4], matched int32 [200], float32 reference): seeded inputs, computed once."""
    h, w, ms, seed = CASES[name]
    rng = np.random.default_rng(seed)
    masks = br.blobs(rng, h, w, 5, empty=(2,))
    rois = br.random_rois(rng, h, w, 200)
    rois[7] = (-2000.0, 10.0, 2150.0, 60.0)                              # 4150 px wide: a sample grid too wide for the kernel's x table
    rois[17] = (3.25, -3000.0, 40.5, 1200.0)                             # and a tall one: most rows outside (-1, size)
    matched = rng.integers(0, len(masks), 200).astype(np.int32)
    matched[11], matched[12] = -1, len(masks)
    matched[::10] = rng.integers(0, 2, 20)                               # the 0.9 x image boxes look at real blobs
    return masks, rois, matched, br.ref_rows(masks, rois, matched, np.float32, ms)


@pytest.mark.parametrize("name", list(CASES))
def test_float32_and_float64_references_disagree_on_few_cells(name):
    """Between the two references, no kernel: a cell flips when float32 rounding carries its average across 0.5, so the share
    depends on how many averages of the seeded inputs sit within a few ulps of 0.5.  Observed: no cell in any of the four cases."""
    masks, rois, matched, want32 = random_case(name)
    want64 = br.ref_rows(masks, rois, matched, np.float64, CASES[name][2])
    share = float((want32 != want64).mean())
    print("%s: float32 and float64 references disagree on %d of %d cells (%.4f %%)" % (name, int((want32 != want64).sum()), want32.size, 100 * share))
    assert share <= DISAGREE_CAP


@gpu
@pytest.mark.parametrize("name", list(CASES))
def test_targets_of_random_boxes_equal_the_float32_reference(name):
    from apse_uav_amd.utils.COCO_utils import DeviceBitmasks, bitmask_targets_device
    masks, rois, matched, want = random_case(name)
    h, w, ms, _ = CASES[name]
    bm = DeviceBitmasks([m if k % 2 else window_mask(m) for k, m in enumerate(masks)], (h, w), DEV)
    assert bm.has_mask.all() and int(bm.host["bits"][2]) == 0            # the blank mask: a segmentation with no pixels
    out = torch.full((203, ms, ms), 7, dtype=torch.uint8, device=DEV)
    got = bitmask_targets_device(bm, rois, matched, ms, out=out)
    assert got.data_ptr() == out.data_ptr() and bool((out[200:] == 7).all())
    got = got.cpu().numpy()
    bad = np.nonzero((got != want).reshape(200, -1).any(axis=1))[0]
    assert len(bad) == 0, (bad[:10], rois[bad[:10]], matched[bad[:10]])
    grids = br.samples_per_cell(rois, ms)
    assert (grids == 0).any() and (grids == 1).any() and (grids > 6).any()
    assert want[11].sum() == 0 and want[12].sum() == 0 and want[matched == 2].sum() == 0 and 0 < want.mean() < 1
    assert np.array_equal(bitmask_targets_device(bm, rois, matched, ms).cpu().numpy(), want)       # and again: the same bytes


# ---------------------------------------------------------------- 4. polygon path
@gpu
def test_rectangles_as_polygon_and_as_rle():
    """PolygonMasks.crop_and_resize rasterises the scaled polygon at 28 x 28; BitMasks.crop_and_resize samples the image-size
    bitmask bilinearly.  Different algorithms: the share of differing cells is an observation (printed), not a bar."""
    from apse_uav_amd.utils import rle
    from apse_uav_amd.utils.COCO_utils import DeviceBitmasks, DevicePolygons, bitmask_targets_device, mask_targets_device
    h, w = 96, 160
    rng = np.random.default_rng(41)
    rects = [(20, 10, 90, 70), (100, 30, 150, 90), (5, 40, 60, 80), (64, 0, 128, 96)]
    polys = [[[x0, y0, x1, y0, x1, y1, x0, y1]] for x0, y0, x1, y1 in rects]
    segs = []
    for x0, y0, x1, y1 in rects:
        m = np.zeros((h, w), np.uint8)
        m[y0:y1, x0:x1] = 1
        segs.append(rle.encode(m))
    n = 200
    matched = rng.integers(0, len(rects), n).astype(np.int32)
    rois = np.zeros((n, 4), np.float32)
    for r in range(n):                                                   # proposals around the matched rectangle
        x0, y0, x1, y1 = rects[matched[r]]
        jit = rng.uniform(-0.3, 0.3, 4) * np.array([x1 - x0, y1 - y0, x1 - x0, y1 - y0])
        rois[r] = np.array([x0, y0, x1, y1]) + jit
    a = mask_targets_device(DevicePolygons(polys, DEV), rois, matched).cpu().numpy()
    b = bitmask_targets_device(DeviceBitmasks(segs, (h, w), DEV), rois, matched).cpu().numpy()
    share = float((a != b).mean())
    print("polygon and bitmask targets differ on %.3f %% of the cells" % (100 * share))
    # a cell's footprint widened by a pixel and a cell: wholly inside the rectangle -> 1, wholly outside -> 0
    cells = np.arange(28)
    checked = 0
    for r in range(n):
        x0, y0, x1, y1 = rects[matched[r]]
        bw, bh = (rois[r, 2] - rois[r, 0]) / 28, (rois[r, 3] - rois[r, 1]) / 28
        cx0, cx1 = rois[r, 0] + cells * bw - bw - 1, rois[r, 0] + (cells + 1) * bw + bw + 1
        cy0, cy1 = rois[r, 1] + cells * bh - bh - 1, rois[r, 1] + (cells + 1) * bh + bh + 1
        inside = ((cy0 >= y0) & (cy1 <= y1))[:, None] & ((cx0 >= x0) & (cx1 <= x1))[None, :]
        outside = ((cy1 <= y0) | (cy0 >= y1))[:, None] | ((cx1 <= x0) | (cx0 >= x1))[None, :]
        agree = a[r] == b[r]
        assert (b[r][inside & agree] == 1).all() and (b[r][outside & agree] == 0).all(), r
        checked += int((inside & agree).sum() + (outside & agree).sum())
    assert checked > 0.3 * a.size


# ---------------------------------------------------------------- 5. round trip with the writers
@gpu
def test_rle_window_and_dense_inputs_give_the_same_bytes():
    from apse_uav_amd.utils.COCO_utils import bitmask_targets
    from apse_uav_amd.utils.rle_device import encode_masks
    h, w = 96, 160
    rng = np.random.default_rng(51)
    masks = br.blobs(rng, h, w, 6, empty=(2,))
    wins = [window_mask(m) for m in masks]
    dicts = encode_masks(wins, (h, w))
    plain = encode_masks(wins, (h, w), compressed=False)
    rois = br.random_rois(rng, h, w, 6)
    rois[0] = (2.0, 3.0, 150.0, 90.0)
    want = np.concatenate([br.ref_targets(m, rois[k:k + 1], np.float32) for k, m in enumerate(masks)])
    for segs in (dicts, wins, masks, [torch.from_numpy(m).to(DEV) for m in masks], [m.astype(np.uint8) * 255 for m in masks],
                 plain, [{"size": [h, w], "counts": d["counts"].decode()} for d in dicts]):
        assert np.array_equal(bitmask_targets(segs, rois, (h, w), DEV).cpu().numpy(), want)
    assert want[2].sum() == 0 and want.sum() > 0
    none = bitmask_targets([None, [], dicts[0]], rois[[0, 0, 0]], (h, w), DEV).cpu().numpy()
    assert none[:2].sum() == 0 and np.array_equal(none[2], want[0])
    assert tuple(bitmask_targets([], np.zeros((0, 4)), (h, w), DEV).shape) == (0, 28, 28)
    with pytest.raises(ValueError, match="size"):
        bitmask_targets([{"size": [h, w + 1], "counts": plain[0]["counts"]}], rois[:1], (h, w), DEV)


@gpu
def test_polygon_objects_are_rasterised_at_the_frame_size():
    from apse_uav_amd.utils import coco as cocomod
    from apse_uav_amd.utils.COCO_utils import DeviceBitmasks
    h, w = 61, 83
    polys = [[[10.0, 5.0, 70.0, 8.0, 60.0, 50.0, 12.0, 40.0]], [[1.5, 1.5, 20.5, 1.5, 20.5, 30.5]], []]
    bm = DeviceBitmasks(polys, (h, w), DEV)
    assert bm.has_mask.tolist() == [True, True, False]
    win, keep = cocomod.polygons_to_windows([(cocomod.polygon_parts(p), h, w) for p in polys[:2]], torch.device(DEV))
    assert np.array_equal(cocomod.windows_to_dense(bm.windows, h, w)[:2], cocomod.windows_to_dense(win, h, w))
    assert not cocomod.windows_to_dense(bm.windows, h, w)[2].any()


# ---------------------------------------------------------------- 8. the C ABI
@gpu
def test_bad_arguments_are_invalid_and_zero_rows_are_a_no_op():
    from apse_uav_amd import _lib
    from apse_uav_amd.structures import device_windows as dw
    from apse_uav_amd.utils.COCO_utils import DeviceBitmasks
    lib = _lib.load()
    assert "apse_mots_remap_windows" in _lib.EXPORTS and "apse_bitmask_targets" in _lib.EXPORTS
    assert hasattr(lib, "apse_mots_remap_windows") and hasattr(lib, "apse_bitmask_targets")
    INVALID, null, st = -1, C.c_void_p(0), _lib.stream_ptr()
    h, w = 40, 70
    dense = np.zeros((h, w), bool)
    dense[5:30, 10:60] = True
    bm = DeviceBitmasks([dense], (h, w), DEV)
    rois = torch.tensor([[8.0, 4.0, 62.0, 31.0]], device=DEV)
    matched = torch.zeros(1, dtype=torch.int32, device=DEV)
    out = torch.full((2, 28, 28), 9, dtype=torch.uint8, device=DEV)
    p = _lib.ptr

    def targets(win=p(bm.windows), n_obj=1, hh=h, ww=w, r=p(rois), m=p(matched), n=1, ms=28, o=p(out)):
        return lib.apse_bitmask_targets(win, n_obj, hh, ww, r, m, n, ms, o, st)
    assert targets(n=0, win=null, r=null, m=null, o=null) == 0
    torch.cuda.synchronize()
    assert bool((out == 9).all())
    for bad in (dict(n=-1), dict(n=1025), dict(n_obj=-1), dict(n_obj=1025), dict(ms=0), dict(ms=65), dict(hh=0), dict(ww=0),
                dict(ww=49153), dict(r=null), dict(m=null), dict(o=null), dict(win=null)):
        assert targets(**bad) == INVALID, bad
    assert targets(ms=1, o=p(out)) == 0 and targets(win=null, n_obj=0) == 0 and targets() == 0
    torch.cuda.synchronize()
    assert bool((out[1] == 9).all()) and int(out[0].sum()) > 0

    arr, pool = dw.pooled_windows(np.array([[10, 5, 60, 30]]), torch.device(DEV))
    dst = dw.upload(arr, DEV)
    xm = torch.arange(w, dtype=torch.int32, device=DEV)
    ym = torch.arange(h, dtype=torch.int32, device=DEV)

    def remap(src=p(bm.windows), n=1, H=h, W=w, x=p(xm), y=p(ym), hh=h, ww=w, d=p(dst), dh=p(arr)):
        return lib.apse_mots_remap_windows(src, n, H, W, x, y, hh, ww, d, dh, st)
    assert remap(n=0, src=null, x=null, y=null, d=null, dh=null) == 0
    for bad in (dict(n=-1), dict(n=1025), dict(H=0), dict(W=0), dict(hh=0), dict(ww=0), dict(src=null), dict(x=null), dict(y=null),
                dict(d=null), dict(dh=null), dict(ww=59), dict(hh=29)):       # (the last two: the rect leaves the image)
        assert remap(**bad) == INVALID, bad
    narrow = arr.copy()
    narrow["words_per_row"] = 0
    assert remap(dh=p(narrow)) == INVALID
    assert remap() == 0
    torch.cuda.synchronize()
    got = pool[:25].cpu().numpy().view(np.uint64).reshape(25, 1)
    assert np.array_equal(got, expected_words(dense, (10, 5, 60, 30)))
