"""CPU (-m "not gpu"): the COCO evaluation restatement (tests/coco_ref.py) on hand-derived cases, rleFrPoly on a rectangle,
and the host parts of utils/coco.py / utils/coco_eval.py: Params defaults, loadRes' field rules, the summarize() text,
instances_to_coco_json on host tensors."""
import numpy as np
import pytest
import torch

import coco_ref
from apse_uav_amd.structures.instances import Boxes, Instances
from apse_uav_amd.utils import coco as cocomod
from apse_uav_amd.utils import coco_eval as ce
from apse_uav_amd.utils import rle


def dataset(gts, h=600, w=600, cats=(1,)):
    """One image (id 1), categories ``cats``; gts: dicts with bbox (and optional area / iscrowd / segmentation)."""
    anns = []
    for k, g in enumerate(gts):
        b = g["bbox"]
        a = dict(id=g.get("id", k + 1), image_id=1, category_id=g.get("category_id", 1), bbox=list(b),
                 area=g.get("area", b[2] * b[3]), iscrowd=g.get("iscrowd", 0))
        a["segmentation"] = g.get("segmentation", [[b[0], b[1], b[0] + b[2], b[1], b[0] + b[2], b[1] + b[3], b[0], b[1] + b[3]]])
        anns.append(a)
    return dict(images=[dict(id=1, height=h, width=w)], annotations=anns, categories=[dict(id=c, name="c%d" % c) for c in cats])


def det(b, s, **kw):
    return dict(image_id=1, category_id=1, bbox=list(b), score=s, **kw)


def stats(gts, dts, iou_type="bbox", **kw):
    return coco_ref.run(dataset(gts, **kw), dts, iou_type).stats


HAND = {
    # name: (gts, dts, {stat index: expected})
    "A": ([dict(bbox=[0, 0, 50, 50]), dict(bbox=[100, 100, 50, 50])], [det([0, 0, 50, 50], .9)],
          {0: 51 / 101, 1: 51 / 101, 2: 51 / 101, 4: 51 / 101, 3: -1, 5: -1, 6: .5, 7: .5, 8: .5, 10: .5, 9: -1, 11: -1}),
    "B": ([dict(bbox=[0, 0, 50, 50])], [det([200, 200, 50, 50], .9), det([0, 0, 50, 50], .8)],
          {0: .5, 1: .5, 2: .5, 4: .5, 6: 0, 7: 1, 8: 1, 10: 1}),
    "C": ([dict(bbox=[0, 0, 50, 50]), dict(bbox=[300, 300, 200, 200], iscrowd=1)],
          [det([320, 320, 50, 50], .9), det([0, 0, 50, 50], .8)], {0: 1, 4: 1, 6: 0, 7: 1}),
    "D": ([dict(bbox=[0, 0, 50, 50], area=500)], [det([0, 0, 50, 50], .9)], {3: 1, 4: -1, 9: 1, 10: -1}),
    "E": ([dict(bbox=[0, 0, 100, 100])], [det([0, 0, 100, 50], .9)], {0: .1, 1: 1, 2: 0, 5: .1, 4: -1, 8: .1}),
}


@pytest.mark.parametrize("name", sorted(HAND))
def test_hand_cases_on_reference(name):
    gts, dts, want = HAND[name]
    got = stats(gts, dts)
    for i, v in want.items():
        assert got[i] == pytest.approx(v, abs=1e-12), (name, i, got)      # pr = tp / (tp + fp + 2^-52): 1 is 1 - 2^-52


def test_hand_case_c_crowd_matters():
    gts, dts, _ = HAND["C"]
    assert stats(gts[:1], dts)[0] == 0.5                 # without the crowd region, detection 1 is a false positive
    assert stats(gts, dts)[0] == pytest.approx(1, abs=1e-12)


def square(x, y, s, h=200, w=200):
    m = np.zeros((h, w), np.uint8)
    m[y:y + s, x:x + s] = 1
    e = rle.encode(m)
    e["counts"] = e["counts"].decode()
    return e


def test_hand_case_f_box_area_filters_segm():
    gts = [dict(bbox=[10, 10, 20, 20], area=400, segmentation=[[10, 10, 30, 10, 30, 30, 10, 30]])]
    dts = [det([100, 100, 40, 40], .9, segmentation=square(100, 100, 30)), det([10, 10, 20, 20], .8, segmentation=square(10, 10, 20))]
    got = stats(gts, dts, "segm", h=200, w=200)
    assert got[3] == pytest.approx(1, abs=1e-12)        # detection 1 (box area 1600) is ignored in 'small'
    seg_only = [dict(image_id=1, category_id=1, score=d["score"], segmentation=d["segmentation"]) for d in dts]
    assert stats(gts, seg_only, "segm", h=200, w=200)[3] == pytest.approx(0.5, abs=1e-12)     # by its mask area (900) it would count


@pytest.mark.parametrize("rect", [(10, 10, 20, 20), (3, 5, 17, 9), (0, 0, 7, 4), (2, 1, 3, 2), (0, 0, 40, 30)])
def test_polygon_rectangle_is_its_pixels(rect):
    x0, y0, x1, y1 = rect
    h, w = 30, 40
    m = coco_ref.decode(coco_ref.frPoly([x0, y0, x1, y0, x1, y1, x0, y1], h, w))
    want = np.zeros((h, w), bool)
    want[y0:y1, x0:x1] = True
    assert np.array_equal(m, want)


def test_params_defaults():
    p = ce.Params("bbox")
    assert np.array_equal(p.iouThrs, np.linspace(.5, .95, 10))
    assert p.iouThrs[8] == 0.8999999999999999
    assert np.array_equal(p.recThrs, np.linspace(0, 1, 101))
    assert p.maxDets == [1, 10, 100]
    assert p.areaRng == [[0, 1e10], [0, 1024], [1024, 9216], [9216, 1e10]]
    assert p.areaRngLbl == ["all", "small", "medium", "large"]
    assert p.useCats == 1 and p.iouType == "bbox" and ce.Params().iouType == "segm"
    with pytest.raises(NotImplementedError):
        ce.Params("keypoints")


def test_loadres_field_rules(capsys):
    gt = cocomod.COCO.from_dataset(dataset([dict(bbox=[0, 0, 10, 10])], h=20, w=30), verbose=False)
    seg = square(2, 3, 4, h=20, w=30)
    res = gt.loadRes([dict(image_id=1, category_id=1, bbox=[1.5, 2, 3, 4], score=.5, segmentation=seg),
                      dict(image_id=1, category_id=1, bbox=[0, 0, 2, 2], score=.4)])
    a, b = res.loadAnns([1, 2])
    assert a["area"] == 12.0 and a["id"] == 1 and a["iscrowd"] == 0 and a["segmentation"] is seg     # box area, not 16
    assert b["segmentation"] == [[0, 0, 0, 2, 2, 2, 2, 0]] and b["id"] == 2
    res2 = gt.loadRes([dict(image_id=1, category_id=1, score=.5, segmentation=seg)])
    c = res2.loadAnns([1])[0]
    assert c["area"] == 16 and list(c["bbox"]) == [2.0, 3.0, 4.0, 4.0]
    ref = coco_ref.COCO(dataset([dict(bbox=[0, 0, 10, 10])], h=20, w=30)).loadRes([dict(image_id=1, category_id=1, score=.5,
                                                                                         segmentation=seg)])
    assert ref.anns[1]["area"] == c["area"] and list(ref.anns[1]["bbox"]) == list(c["bbox"])
    with pytest.raises(AssertionError):
        gt.loadRes([dict(image_id=7, category_id=1, bbox=[0, 0, 1, 1], score=.1)])
    out = capsys.readouterr().out
    assert "Loading and preparing results..." in out


def test_tobbox_and_area_match_reference():
    g = np.random.default_rng(3)
    for _ in range(20):
        h, w = int(g.integers(1, 30)), int(g.integers(1, 30))
        m = g.random((h, w)) < g.random()
        e = rle.encode(m.astype(np.uint8))
        r = coco_ref.encode(m)
        assert cocomod.area(e) == coco_ref.area(r)
        assert list(cocomod.toBbox(e)) == coco_ref.toBbox(r)


def test_summarize_text(capsys):
    g = np.random.default_rng(0)
    T, R, K, A, M = 10, 101, 3, 4, 3
    prec = np.where(g.random((T, R, K, A, M)) < .2, -1.0, g.random((T, R, K, A, M)))
    rec = np.where(g.random((T, K, A, M)) < .2, -1.0, g.random((T, K, A, M)))
    ev = ce.COCOeval(None, None, "bbox")
    ev.eval = dict(precision=prec, recall=rec, scores=prec)
    ev.summarize()
    lines = capsys.readouterr().out.splitlines()
    ref = coco_ref.COCOeval.__new__(coco_ref.COCOeval)
    ref.params, ref.lines, ref.eval = coco_ref.Params(), [], dict(precision=prec, recall=rec)
    want = ref.summarize()
    assert lines == ref.lines and np.array_equal(ev.stats, want)
    assert lines[0] == " Average Precision  (AP) @[ IoU=0.50:0.95 | area=   all | maxDets=100 ] = %0.3f" % want[0]
    ev.params.maxDets = [1, 5, 50]                       # stats[0] asks for maxDets=100, which is not there: -1
    ev.summarize()
    assert ev.stats[0] == -1 and capsys.readouterr().out.splitlines()[0].endswith("= -1.000")


def test_instances_to_coco_json_host():
    g = np.random.default_rng(5)
    H, W = 20, 33
    n = 4
    xy = g.random((n, 2)) * 10
    boxes = np.concatenate([xy, xy + 1 + g.random((n, 2)) * 9], 1).astype(np.float32)
    inst = Instances((H, W))
    inst.pred_boxes = Boxes(torch.from_numpy(boxes))
    inst.scores = torch.from_numpy(g.random(n).astype(np.float32))
    inst.pred_classes = torch.from_numpy(np.array([0, 2, 1, 0], np.int64))
    masks = torch.from_numpy(g.random((n, H, W)) < .3)
    inst.pred_masks = masks
    got = ce.instances_to_coco_json(inst, 7)
    want = coco_ref.instances_to_coco_json(boxes, inst.scores.numpy(), [0, 2, 1, 0], masks.numpy(), 7)
    assert got == want
    assert got[0]["bbox"][2] == float(np.float32(boxes[0, 2]) - np.float32(boxes[0, 0]))
    assert isinstance(got[0]["segmentation"]["counts"], str)
    assert np.array_equal(rle.decode(got[1]["segmentation"]).astype(bool), masks[1].numpy())
    empty = Instances((H, W))
    empty.pred_boxes = Boxes(torch.zeros((0, 4)))
    empty.scores = torch.zeros(0)
    empty.pred_classes = torch.zeros(0, dtype=torch.int64)
    assert ce.instances_to_coco_json(empty, 1) == []


def test_refusals():
    ev = ce.COCOeval(None, None, "bbox")
    ev.params.useCats = 0
    with pytest.raises(NotImplementedError):
        ev.evaluate()
    with pytest.raises(NotImplementedError):
        ce.COCOeval(None, None, "keypoints")
