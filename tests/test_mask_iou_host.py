"""CPU (-m "not gpu"): the association metrics that need no association head -- the numpy restatement against the reference's
own translate_and_crop_mask outputs, and RcnnTracker's 'mask_iou' / 'bbox_center_dist' bookkeeping on scripted inputs."""
import os

import numpy as np
import pytest
import torch

import mask_iou_ref as ref

FRAME = (100, 200)


# ---------------------------------------------------------------- restatement against the golden
def load_translate_golden(golden_dir):
    z = np.load(os.path.join(golden_dir, "mask_translate_golden.npz"))
    H, W = (int(v) for v in z["shape"])
    unpack = lambda rows: np.unpackbits(rows, axis=1)[:, :H * W].reshape(-1, H, W).astype(bool)   # noqa: E731
    return unpack(z["masks"]), z["dx"], z["dy"], z["mask_index"], unpack(z["outputs"])


def test_restatement_equals_reference_translate_on_every_case(golden_dir):
    masks, dx, dy, which, outs = load_translate_golden(golden_dir)
    assert len(dx) == 16 * 8 and masks.shape[1:] == (37, 150)
    assert {int(v) for v in dx} == {0, 1, -1, 63, -63, 64, -64, 65, -65, 127, -128, 149, -149, 150, -150, 200}
    assert {int(v) for v in dy} == {0, 1, -1, 36, -36, 37, -37, 50}
    for k in range(len(dx)):
        got = ref.translate_and_crop(masks[which[k]], (int(dx[k]), int(dy[k])))
        assert np.array_equal(got, outs[k]), (int(dx[k]), int(dy[k]))
    assert np.array_equal(ref.translate_and_crop(masks[0], (2.9, -1.9)), ref.translate_and_crop(masks[0], (2, -1)))   # int()


def test_iou_division_is_f32_of_both_integers():
    for inter, union in ((7, 10), (1, 3), (16777217, 33554434), (599, 1080)):
        want = torch.true_divide(torch.tensor(inter), torch.tensor(union)).item()
        assert float(ref.iou_f32(inter, union, inter)) == want
    assert float(ref.iou_f32(0, 0, 0)) == 0.0


def test_scripted_sequence_outcomes():
    """The rectangles of the GPU test give the outcomes it names, by the restatement alone."""
    ids = ref.scripted_expected()
    assert all(f["mover"] == 1 for f in ids)                                  # aligned IoU 1.0 while moving
    assert ids[2]["returner"] == 2 and all("returner" not in ids[t] for t in (3, 4, 5)) and ids[6]["returner"] == 2
    assert ids[3]["grower"] == 3 and ids[4]["grower"] == 4                    # 20 -> 36 rows: IoU 20/36 < 0.7
    assert "late" not in ids[4] and ids[5]["late"] == 5
    a, b = ref.rect_mask((300, 150, 330, 170)), ref.rect_mask((300, 150, 330, 186))
    assert ref.masks_iou(b, a) == float(np.float32(600) / np.float32(1080))
    assert ref.masks_iou(ref.rect_mask((20, 30, 60, 60)), ref.rect_mask((34, 30, 74, 60))) == 1.0


# ---------------------------------------------------------------- tracker bookkeeping on scripted matrices
def _tracker(metric, weights=None, **kw):
    from apse_uav_amd.config import setup_cfg
    from apse_uav_amd.engines.rcnn_tracker import RcnnTracker
    from apse_uav_amd.weights import synthetic_detector_state
    return RcnnTracker(setup_cfg(device="cpu"), FRAME, weights, association_metric=metric,
                       detector_state=synthetic_detector_state(0, (1, 1, 1, 1)), **kw)


def _det(boxes):
    from apse_uav_amd.structures.instances import Boxes, Instances
    from apse_uav_amd.structures.window_mask import MaskList, WindowMask
    n = len(boxes)
    inst = Instances(FRAME)
    inst.pred_boxes = Boxes(torch.tensor(boxes, dtype=torch.float32).reshape(n, 4))
    inst.scores = torch.linspace(0.9, 0.6, n)
    inst.pred_classes = torch.arange(n) % 4
    inst.pred_masks = MaskList(WindowMask(None, (0, 0, 0, 0), FRAME, (k + 1, k + 2), 5) for k in range(n))
    return inst


def _ids(objects):
    return list(objects.ids) if len(objects) else []                             # an empty ObjectInstances has no fields


def _boxes(n, base=0):
    return [[base + 10.0 * k, 1.0, base + 10.0 * k + 4, 5.0] for k in range(n)]


class Script:
    """Stands in for mask_utils.masks_iou_matrix: hands out the scripted matrices in order and checks the shape asked for
    (rows: the frame's detections; columns: the stored objects, then -- with more than one detection -- the detections)."""

    def __init__(self, monkeypatch, *matrices):
        from apse_uav_amd.utils import mask_utils
        self.todo = [np.asarray(m) for m in matrices]
        self.calls = 0
        monkeypatch.setattr(mask_utils, "masks_iou_matrix", self)

    def __call__(self, det_masks, obj_masks):
        m = self.todo[self.calls]
        self.calls += 1
        assert m.shape == (len(det_masks), len(obj_masks)), (m.shape, len(det_masks), len(obj_masks))
        return m

    def done(self):
        return self.calls == len(self.todo)


def test_mask_iou_first_frame_all_new(monkeypatch):
    tr = _tracker("mask_iou")
    assert tr.association_head is None and tr.predictor.model._assoc is None
    s = Script(monkeypatch, np.zeros((3, 3), np.float32))
    out = tr._finish_frame(_det(_boxes(3)), None)
    assert out.ids == [1, 2, 3] and tr.objects.ids == [1, 2, 3] and s.done()
    assert not tr.objects.has("embeddings")


def test_mask_iou_single_first_detection_needs_no_matrix(monkeypatch):
    tr = _tracker("mask_iou")
    s = Script(monkeypatch)
    assert tr._finish_frame(_det(_boxes(1)), None).ids == [1] and s.calls == 0


def test_mask_iou_threshold_is_inclusive(monkeypatch):
    tr = _tracker("mask_iou")
    below = np.nextafter(0.7, 0.0)
    Script(monkeypatch, [[0.7]], [[below]])
    tr._finish_frame(_det(_boxes(1)), None)
    assert tr._finish_frame(_det(_boxes(1, 50)), None).ids == [1]                 # exactly 0.7 associates
    assert tr._finish_frame(_det(_boxes(1, 70)), None).ids == [2]                 # the next double below does not
    assert tr.objects.ids == [1, 2]


def test_mask_iou_f32_seven_tenths_is_below_the_threshold(monkeypatch):
    """The IoU is an f32 quotient read as a double (``.item()`` in the reference): f32(7) / f32(10) = 0.699999988 < 0.7."""
    tr = _tracker("mask_iou")
    Script(monkeypatch, np.asarray([[np.float32(7) / np.float32(10)]], np.float32))
    tr._finish_frame(_det(_boxes(1)), None)
    assert tr._finish_frame(_det(_boxes(1, 50)), None).ids == [2]


def test_mask_iou_tie_takes_the_first_object(monkeypatch):
    tr = _tracker("mask_iou")
    Script(monkeypatch, np.zeros((2, 2), np.float32), np.asarray([[0.8, 0.8]], np.float32))
    tr._finish_frame(_det(_boxes(2)), None)
    assert tr._finish_frame(_det(_boxes(1, 50)), None).ids == [1]


def test_mask_iou_two_detections_on_one_object_later_wins(monkeypatch):
    tr = _tracker("mask_iou")
    # columns: object 1, detection 0, detection 1.  Detection 0 takes object 1, which then holds detection 0's mask: detection
    # 1 is compared with THAT mask (column 1), not with the mask the object held before the frame (column 0)
    Script(monkeypatch, np.asarray([[0.9, 0.0, 0.0], [0.0, 0.95, 0.0]], np.float32))
    tr._finish_frame(_det(_boxes(1)), None)
    d = _det(_boxes(2, 50))
    out = tr._finish_frame(d, None)
    assert out.ids == [1] and tr.objects.ids == [1] and tr.objects.get_new_id() == 2
    assert torch.equal(tr.objects.pred_boxes[0].tensor, d.pred_boxes[1].tensor)
    assert tr._obj_det == {1: 1}


def test_mask_iou_object_born_in_the_frame_is_a_candidate(monkeypatch):
    tr = _tracker("mask_iou")
    Script(monkeypatch, np.asarray([[0.0, 0.0, 0.0], [0.9, 0.0, 0.0], [0.1, 0.0, 0.0]], np.float32))
    out = tr._finish_frame(_det(_boxes(3)), None)
    assert out.ids == [1, 2] and tr.objects.ids == [1, 2]                         # detection 1 joined the object of detection 0
    assert tr._obj_det == {1: 1, 2: 2}


def test_mask_iou_no_detections_changes_nothing_and_objects_age(monkeypatch):
    tr = _tracker("mask_iou")
    s = Script(monkeypatch, np.zeros((2, 2), np.float32), np.asarray([[0.0, 0.9]], np.float32), np.asarray([[0.0, 0.9]], np.float32))
    tr._finish_frame(_det(_boxes(2)), None)
    out = tr._finish_frame(_det([]), None)
    assert len(out) == 0 and tr.objects.ids == [1, 2] and tr.objects.frames_since_detected == [1, 1] and s.calls == 1
    assert tr._finish_frame(_det(_boxes(1)), None).ids == [2]                     # stale objects take part
    assert tr.objects.frames_since_detected == [2, 0]
    tr.objects._fields["frames_since_detected"] = [101, 0]
    assert tr._finish_frame(_det(_boxes(1)), None).ids == [2]                     # associated first, then the stale one is dropped
    assert tr.objects.ids == [2] and s.done()


def test_mask_iou_tracker_equals_restatement_on_random_scripts(monkeypatch):
    """Random IoU tables over 6 frames: the tracker's ids equal the restatement's greedy loop fed the same table."""
    rng = np.random.default_rng(5)
    from apse_uav_amd.utils import mask_utils
    table = {}

    def pair_iou(a, b):
        key = (id(a), id(b))
        if key not in table:
            table[key] = float(np.float32(rng.choice([0.0, 0.3, 0.69, 0.7, 0.75, 0.9, 0.9])))
        return table[key]
    monkeypatch.setattr(mask_utils, "masks_iou_matrix", lambda dm, om: np.asarray(
        [[pair_iou(a, b) for b in om] for a in dm], np.float32).reshape(len(dm), len(om)))
    tr = _tracker("mask_iou")
    store = ref.Store()
    for t in range(6):
        d = _det(_boxes(int(rng.integers(0, 5))))
        got = tr._finish_frame(d, None)
        want = ref.step_mask_iou(store, list(d.pred_masks), iou=lambda a, b: float(np.float32(pair_iou(a, b))))
        assert _ids(got) == want, t
    assert tr.objects.ids == store.ids


# ---------------------------------------------------------------- bbox_center_dist
def _record(boxes):
    n = len(boxes)
    return dict(boxes=np.asarray(boxes, np.float32).reshape(n, 4), scores=np.full(n, 0.9, np.float32),
                classes=np.zeros(n, np.int64), rects=np.zeros((n, 4), np.int32), centroids=np.ones((n, 2), np.int32),
                mass=np.ones(n, np.int32), closest=np.zeros((n, n, 2), np.int32))


def test_bbox_center_dist_needs_a_threshold():
    tr = _tracker("bbox_center_dist")
    assert tr.BBOX_CENTER_DIST_THRESHOLD is None
    with pytest.raises(ValueError, match="threshold"):
        tr._finish_frame(_det(_boxes(1)), None)


def test_bbox_center_dist_associates_every_object_under_the_threshold_through_records():
    tr = _tracker("bbox_center_dist", bbox_center_dist_threshold=25.0)
    store = ref.Store()
    frames = [[[8, 8, 12, 12], [14, 8, 18, 12], [100, 50, 110, 60]],             # centres (10, 10), (16, 10): 36 apart
              [[11, 8, 15, 12]],                                                  # centre (13, 10): 9 from both
              [[11, 8, 15, 12], [12, 9, 16, 13], [60, 60, 70, 70]],
              []]
    for boxes in frames:
        got = tr.next_record(_record(boxes))
        assert _ids(got) == ref.step_bbox_center_dist(store, boxes, 25.0)
    assert tr.objects.ids == [1, 2, 3, 4]
    tr2 = _tracker("bbox_center_dist", bbox_center_dist_threshold=25.0)
    tr2.next_record(_record(frames[0]))
    out = tr2.next_record(_record(frames[1]))
    assert out.ids == [1, 2] and tr2.objects.frames_since_detected == [0, 0, 1]
    for k in (0, 1):
        assert out.pred_boxes[k].tensor.tolist() == [[11.0, 8.0, 15.0, 12.0]]
    line, _ = tr2.log_line(out, 1, 1)
    assert line.startswith("1,")
    tr3 = _tracker("bbox_center_dist", bbox_center_dist_threshold=9.0)           # strictly below: 9 is not under 9
    tr3.next_record(_record(frames[0]))
    assert tr3.next_record(_record(frames[1])).ids == [4]


# ---------------------------------------------------------------- construction and refusals
def test_unknown_metric_is_refused_at_construction():
    with pytest.raises(ValueError, match="association_metric"):
        _tracker("iou")


def test_embeddings_metric_needs_weights():
    from apse_uav_amd.weights import synthetic_association_state
    with pytest.raises(ValueError, match="weights"):
        _tracker("embeddings")
    tr = _tracker("embeddings", synthetic_association_state(1))
    assert tr.association_metric == "embeddings" and tr.association_head is not None
    assert _tracker("mask_iou", synthetic_association_state(1)).association_head is not None     # weights given: still loaded


def test_record_paths_refuse_mask_iou():
    from apse_uav_amd.config import setup_cfg
    from apse_uav_amd.engines.pipelined_tracker import PipelinedRcnnTracker
    tr = _tracker("mask_iou")
    with pytest.raises(NotImplementedError, match="mask bits"):
        tr.next_record(_record(_boxes(1)))
    assert tr.frame_count == 0
    for metric in ("mask_iou", "bbox_center_dist"):
        with pytest.raises(NotImplementedError, match="embeddings"):
            PipelinedRcnnTracker(setup_cfg(device="cpu"), FRAME, None, association_metric=metric)


def test_translate_and_crop_needs_no_gpu_for_host_tensors(golden_dir):
    """The API-compatibility helper is plain tensor slicing: on host tensors it equals the golden too."""
    from apse_uav_amd.utils.mask_utils import translate_and_crop_mask
    masks, dx, dy, which, outs = load_translate_golden(golden_dir)
    for k in range(len(dx)):
        got = translate_and_crop_mask(torch.from_numpy(masks[which[k]]), (int(dx[k]), int(dy[k])))
        assert got.dtype == torch.bool and np.array_equal(got.numpy(), outs[k]), (int(dx[k]), int(dy[k]))
