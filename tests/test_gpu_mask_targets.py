"""-m gpu: apse_coco_mask_targets (csrc/coco_eval.hip mask_targets_kernel, utils/COCO_utils.py mask_targets_device) -- detectron2's
PolygonMasks.crop_and_resize(boxes, 28) for proposals that are new every step -- against two references, byte for byte and
without a tolerance:

* the host path ``COCO_utils.mask_targets`` (crop_and_resize_polygons + poly_layout + apse_coco_poly_to_bits + windows_to_dense),
  the arbiter;
* an independent CPU restatement: ``crop_and_resize_polygons`` followed by tests/coco_ref.py ``frPoly`` per part, ``merge`` and
  ``decode`` at 28 x 28.

The two references are compared with each other on every case first.  The case rows are every object (1 part, 3 parts, a part
with an odd coordinate count, no parts, degenerate 1- and 2-vertex parts) under every box kind (the ground-truth box, fractional
f32 corners, a square, a wide flat box, widths 0.05 and 0, boxes the polygon leaves to the left and to the top, a box off the
polygon, a box 20 x the polygon), followed by rows whose index is out of range.  Larger row counts cycle through the case rows, so
the references are computed once."""
import numpy as np
import pytest
import torch

import coco_ref

pytestmark = pytest.mark.gpu

DEV = "cuda"
S = 28

# The image's objects: flat x, y lists in resized-image pixels.
OBJECTS = [
    [[30.25, 40.5, 58.0, 36.75, 66.5, 55.0, 49.0, 71.25, 41.5, 52.0, 27.75, 60.5]],                       # 1 part, concave
    [[100.0, 20.0, 130.5, 22.0, 128.0, 48.5, 103.5, 44.0],                                                 # 3 parts: two overlap,
     [118.0, 30.0, 150.0, 34.0, 140.0, 60.0],                                                              # one stands apart
     [160.25, 18.5, 171.0, 18.5, 171.0, 29.75, 160.25, 29.75]],
    [[200.0, 100.0, 231.5, 104.0, 224.0, 131.0, 204.5, 126.5, 999.0],                                      # odd count: 999 is cut
     [210.0, 90.0, 216.0, 90.0, 213.0, 99.0]],
    [],                                                                                                    # no parts
    [[60.0, 120.0], [70.0, 121.0, 82.5, 133.0], [64.0, 124.0, 80.0, 126.5, 71.0, 140.0]],                  # 1 and 2 vertices, a triangle
]


def _extent(obj):
    pts = np.concatenate([np.asarray(p, np.float64)[:2 * (len(p) // 2)] for p in obj]) if obj else np.array([10.0, 10.0, 40.0, 30.0])
    return pts[0::2].min(), pts[1::2].min(), pts[0::2].max(), pts[1::2].max()


def _boxes(obj):
    """The box kinds for one object, as f32 rows."""
    x0, y0, x1, y1 = _extent(obj)
    w, h = x1 - x0, y1 - y0
    side = max(w, h)
    out = [
        (x0, y0, x1, y1),                                           # the ground-truth box
        (x0 - 1.37, y0 + 0.61, x1 + 2.213, y1 - 0.77),              # fractional f32 corners
        (x0, y0, x0 + side, y0 + side),                             # square: rh == rw
        (x0 - 0.5 * w, y0 + 0.4 * h, x1 + 0.5 * w, y0 + 0.4 * h + 0.07 * w),   # wide and flat
        (x0 + 0.5 * w, y0, x0 + 0.5 * w + 0.05, y1),                # width 0.05: max(., 0.1)
        (x0 + 0.25 * w, y0, x0 + 0.25 * w, y1),                     # width 0
        (x0 + 0.4 * w, y0 - 3.0, x1 + 0.4 * w, y1 + 1.0),           # the polygon crosses the left edge: negative x
        (x0 - 2.0, y0 + 0.45 * h, x1, y1 + 0.45 * h),               # ... the top edge: negative y
        (x1 + 25.0, y1 + 30.0, x1 + 60.0, y1 + 55.0),               # wholly off the polygon
        (x0 - 9.5 * w, y0 - 9.5 * h, x1 + 9.5 * w, y1 + 9.5 * h),   # 20 x the polygon: under one pixel
    ]
    return np.array(out, np.float64).astype(np.float32)


def _case_rows():
    boxes, matched = [], []
    for k, obj in enumerate(OBJECTS):
        b = _boxes(obj)
        boxes.append(b)
        matched += [k] * len(b)
    base = _boxes(OBJECTS[0])[:3]
    boxes.append(base)
    matched += [-1, len(OBJECTS), 2 ** 31 - 1]                       # out of range: all-zero rows
    return np.concatenate(boxes), np.array(matched, np.int64)


def _polys_of(m):
    return OBJECTS[m] if 0 <= m < len(OBJECTS) else []


def _restated(polys, box):
    """crop_and_resize_polygons + rleFrPoly per part + merge + decode at 28 x 28."""
    from apse_uav_amd.utils.COCO_utils import crop_and_resize_polygons
    rles = [coco_ref.frPoly(list(q), S, S) for q in crop_and_resize_polygons(polys, box, S)]
    if not rles:
        return np.zeros((S, S), np.uint8)
    return coco_ref.decode(coco_ref.merge(rles)).astype(np.uint8)


@pytest.fixture(scope="module")
def cases():
    """(boxes f32 [B][4], matched int64 [B], host-path targets u8 [B][28][28], restated targets u8 [B][28][28])."""
    from apse_uav_amd.utils.COCO_utils import mask_targets
    boxes, matched = _case_rows()
    host = mask_targets([_polys_of(int(m)) for m in matched], boxes, DEV).cpu().numpy()
    ref = np.stack([_restated(_polys_of(int(m)), b) for m, b in zip(matched, boxes)])
    return boxes, matched, host, ref


def _device(boxes, matched, out=None):
    from apse_uav_amd.utils.COCO_utils import DevicePolygons, mask_targets_device
    polys = DevicePolygons(OBJECTS, DEV)
    return mask_targets_device(polys, torch.from_numpy(boxes).to(DEV), torch.from_numpy(matched.astype(np.int32)).to(DEV), out=out)


def test_the_two_references_agree_on_every_case(cases):
    boxes, matched, host, ref = cases
    assert host.shape == ref.shape == (len(boxes), S, S) and host.dtype == ref.dtype == np.uint8
    bad = [i for i in range(len(boxes)) if not np.array_equal(host[i], ref[i])]
    assert not bad, bad
    assert set(np.unique(host)) <= {0, 1}
    # the cases are what they claim: full and empty rows, sub-pixel objects, every object seen
    per = host.reshape(len(boxes), -1).sum(1)
    kinds = per[:len(OBJECTS) * 10].reshape(len(OBJECTS), 10)
    assert (kinds[[0, 1, 2, 4], 0] > 100).all() and (kinds[:, 8] == 0).all() and (kinds[3] == 0).all()
    assert (kinds[[0, 1, 2, 4], 9] <= 4).all() and (per[-3:] == 0).all()
    assert (kinds[[0, 1, 2, 4], 4] > 0).all() and (kinds[[0, 1, 2, 4], 5] > 0).all()


@pytest.mark.parametrize("n", [0, 1, 65, 1024])
def test_device_targets_equal_both_references(cases, n):
    boxes, matched, host, ref = cases
    B = len(boxes)
    assert B < 65                                                   # 65 and 1024 rows wrap around: more than one pass of the cases
    idx = np.arange(n) % B
    got = _device(boxes[idx], matched[idx])
    assert got.dtype == torch.uint8 and tuple(got.shape) == (n, S, S) and got.is_cuda
    got = got.cpu().numpy()
    for name, want in (("host path", host), ("restatement", ref)):
        bad = [int(i) for i in range(n) if not np.array_equal(got[i], want[idx[i]])]
        assert not bad, (name, bad[:8])
    if n == 65:                                                     # the arbiter run on these very rows, not only tiled
        from apse_uav_amd.utils.COCO_utils import mask_targets
        again = mask_targets([_polys_of(int(m)) for m in matched[idx]], boxes[idx], DEV).cpu().numpy()
        assert np.array_equal(got, again)


def test_rows_past_n_stay_untouched_and_two_calls_agree(cases):
    boxes, matched, host, _ = cases
    n = len(boxes)
    buf = torch.full((n + 7, S, S), 0xA5, dtype=torch.uint8, device=DEV)
    a = _device(boxes, matched, out=buf).clone()
    assert a.shape[0] == n and bool((buf[n:] == 0xA5).all()) and np.array_equal(a.cpu().numpy(), host)
    buf.fill_(0x5A)                                                 # every byte of the n rows is written again
    b = _device(boxes, matched, out=buf)
    assert torch.equal(a, b) and bool((buf[n:] == 0x5A).all())


def test_limits_are_refused_before_any_launch():
    from apse_uav_amd import _lib
    from apse_uav_amd.utils.COCO_utils import DevicePolygons, mask_targets_device
    lib = _lib.load()
    polys = DevicePolygons(OBJECTS, DEV)
    rois = torch.zeros((1025, 4), device=DEV)
    matched = torch.zeros(1025, dtype=torch.int32, device=DEV)
    out = torch.full((1025, S, S), 7, dtype=torch.uint8, device=DEV)
    info = torch.zeros(1, dtype=torch.int32, device=DEV)

    def call(n, size):
        return lib.apse_coco_mask_targets(_lib.ptr(polys.xy), _lib.ptr(polys.part_vert_off), polys.n_parts, _lib.ptr(polys.obj_part_off),
                                     polys.n_obj, polys.n_verts, _lib.ptr(rois), _lib.ptr(matched), n, size, _lib.ptr(out),
                                     _lib.ptr(info), _lib.stream_ptr())
    assert call(1025, 28) == -1 and b"APSE_MASK_TRAIN_MAX_N" in lib.apse_last_error(None)
    assert call(-1, 28) == -1
    assert call(4, 27) == -1 and b"mask_size" in lib.apse_last_error(None)
    assert call(4, 14) == -1
    assert call(0, 28) == 0                                          # n = 0 enqueues nothing
    torch.cuda.synchronize()
    assert bool((out == 7).all()) and int(info.cpu()[0]) == 0
    with pytest.raises(_lib.ApseError):
        mask_targets_device(polys, rois, matched)
    with pytest.raises(_lib.ApseError):
        mask_targets_device(polys, rois[:2], matched[:2], mask_size=14)


def test_a_coordinate_past_the_range_raises_the_host_error():
    from apse_uav_amd.utils import coco
    from apse_uav_amd.utils.COCO_utils import DevicePolygons, mask_targets, mask_targets_device
    far = [[[10.0, 10.0, 2.0e6, 12.0, 15.0, 30.0]]]                 # x 280 (width 0): 5.6e8 > _COORD_MAX = 4.29e8
    boxes = np.array([[10.0, 10.0, 10.0, 30.0]], np.float32)
    assert 2.0e6 * 280 > coco._COORD_MAX
    with pytest.raises(ValueError) as host:
        mask_targets(far, boxes, DEV)
    with pytest.raises(ValueError) as dev:
        mask_targets_device(DevicePolygons(far, DEV), boxes, np.zeros(1, np.int32))
    assert str(host.value) == str(dev.value)
    ok = np.array([[10.0, 10.0, 30.0, 30.0]], np.float32)           # the same polygon under a sane box is accepted by both
    assert torch.equal(mask_targets(far, ok, DEV), mask_targets_device(DevicePolygons(far, DEV), ok, np.zeros(1, np.int32)))
