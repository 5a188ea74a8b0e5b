"""The host parts of the joint loop's mask rows (no GPU): the row selection, the row bound, the polygon layout that is uploaded,
``--mask`` and the results header, and the declaration of apse_coco_mask_targets."""
import os
import re
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def test_select_mask_rows():
    from apse_uav_amd.utils.COCO_utils import select_mask_rows
    K = 3
    #                  fg    fg    fg    fg   ignored  bg  bg   fg
    labels = np.array([0,    2,    1,    0,   -1,      3,  3,   2], np.int32)
    matched = np.array([0,   1,    2,    1,   0,       0,  2,   -1], np.int32)
    parts = [1, 0, 3]                                       # ground truth 1 has no polygon
    rows, skipped = select_mask_rows(labels, matched, parts, K)
    assert rows.dtype == np.int64 and rows.tolist() == [0, 2] and skipped == 3       # rows 1, 3 (no parts) and 7 (no ground truth)
    rows, skipped = select_mask_rows(labels, matched, [2, 2, 2], K)
    assert rows.tolist() == [0, 1, 2, 3] and skipped == 1   # sampling order kept
    rows, skipped = select_mask_rows(labels[5:7], matched[5:7], parts, K)
    assert rows.tolist() == [] and rows.dtype == np.int64 and skipped == 0
    rows, skipped = select_mask_rows(np.zeros(0, np.int32), np.zeros(0, np.int32), [], K)
    assert rows.tolist() == [] and skipped == 0
    rows, skipped = select_mask_rows(labels, matched, [], K)               # an image without ground truth: index -1 everywhere
    assert rows.tolist() == [] and skipped == 5


def test_row_bound():
    from apse_uav_amd.utils.joint_train import JointTrainLoader, check_mask_rows

    class Model:
        c4 = False
    assert check_mask_rows(4, 512, 0.25) == 512 and check_mask_rows(2, 1024, 0.5) == 1024
    assert check_mask_rows(3, 100, 0.26) == 78                             # floor(100 x 0.26) = 26 per image
    with pytest.raises(ValueError) as e:
        check_mask_rows(4, 1024, 0.3)                                      # 4 x 307 = 1228
    assert "1024" in str(e.value) and "APSE_MASK_TRAIN_MAX_N" in str(e.value)
    with pytest.raises(ValueError) as e:                                   # the constructor refuses before it touches the model
        JointTrainLoader([], Model(), 4, box_batch_size_per_image=1024, box_positive_fraction=0.3, mask=True)
    assert "mask rows" in str(e.value)


def test_device_polygons_layout():
    import torch
    from apse_uav_amd.utils.COCO_utils import DevicePolygons
    objs = [[[0.0, 1.0, 2.0, 3.0, 4.0, 5.0]], [], [[1.0, 1.0, 2.0, 2.0, 3.0, 3.0, 9.0], [5.0, 6.0]]]
    p = DevicePolygons(objs, "cpu")
    assert (p.n_obj, p.n_parts, p.n_verts) == (3, 3, 7) and p.parts.tolist() == [1, 0, 2]
    assert p.obj_part_off.tolist() == [0, 1, 1, 3] and p.part_vert_off.tolist() == [0, 3, 6, 7]
    assert p.obj_part_off.dtype == torch.int32 and p.part_vert_off.dtype == torch.int32 and p.xy.dtype == torch.float64
    assert p.xy.tolist() == [0.0, 1.0, 2.0, 3.0, 4.0, 5.0, 1.0, 1.0, 2.0, 2.0, 3.0, 3.0, 5.0, 6.0]      # the odd 9.0 is cut
    e = DevicePolygons([], "cpu")
    assert (e.n_obj, e.n_parts, e.n_verts) == (0, 0, 0) and e.obj_part_off.tolist() == [0] and e.xy.numel() == 0


def test_label_and_sample_proposals_keeps_its_signature():
    import inspect
    from apse_uav_amd.utils.box_train import label_and_sample_proposals
    sig = inspect.signature(label_and_sample_proposals)
    assert sig.parameters["return_index"].default is False and list(sig.parameters)[-1] == "return_index"


def test_mask_argument_and_header():
    import finetune_uav as tool
    from apse_uav_amd.utils import finetune as ft
    ap = tool.parser()
    assert ap.parse_args(["--out", "x"]).mask is False and ap.parse_args(["--out", "x", "--mask"]).mask is True
    plain = tool.results_header(False)
    assert plain == ft.AP_COLUMNS + "\tprop_AR@100\tprop_AR@1000\n" == tool.JointTask().header
    full = tool.results_header(True)
    assert full == tool.JointTask(True).header and full.startswith(plain[:-1]) and full.endswith("\n")
    cols = full.split()
    assert len(cols) == 26 and cols[14:] == ["segm_" + c for c in cols[:12]]
    task = tool.JointTask(True)
    assert (task.precision_index, task.recall_index) == (0, 12) and task.keep_box_only and not tool.JointTask().keep_box_only


def test_box_only_annotations_are_kept_on_request(tmp_path):
    import json
    from apse_uav_amd.utils import COCO_utils
    data = {"images": [{"id": 1, "file_name": "a.png", "height": 10, "width": 10}, {"id": 2, "file_name": "b.png", "height": 10, "width": 10}],
            "categories": [{"id": 7, "name": "car"}],
            "annotations": [{"id": 1, "image_id": 1, "category_id": 7, "bbox": [1, 1, 4, 4], "segmentation": [[1, 1, 5, 1, 5, 5]]},
                            {"id": 2, "image_id": 1, "category_id": 7, "bbox": [2, 2, 3, 3]},
                            {"id": 3, "image_id": 2, "category_id": 7, "bbox": [0, 0, 3, 3], "segmentation": []}]}
    path = tmp_path / "ann.json"
    path.write_text(json.dumps(data))
    today = COCO_utils.generate_coco_dataset_dictionaries(str(path), "x", None, None, False)
    assert [len(d["annotations"]) for d in today] == [1]
    kept = COCO_utils.generate_coco_dataset_dictionaries(str(path), "x", None, None, False, keep_box_only=True)
    assert [len(d["annotations"]) for d in kept] == [2, 1]
    assert [a["segmentation"] for d in kept for a in d["annotations"]] == [[[1.0, 1.0, 5.0, 1.0, 5.0, 5.0]], [], []]
    assert tool_has_polygons(kept[:1]) and not tool_has_polygons(kept[1:])


def tool_has_polygons(dicts):
    import finetune_uav as tool
    return tool.has_polygons(dicts)


def test_entry_is_declared_and_bound():
    from apse_uav_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "apse_hip.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+apse_coco_mask_targets\s*\(", text) and "apse_coco_mask_targets" in _lib.EXPORTS
    assert len(_lib.SIGNATURES["apse_coco_mask_targets"][0]) == 13
    kernels = open(os.path.join(ROOT, "apse_uav_amd", "csrc", "apse_kernels.h")).read()
    assert "apse_k_mask_targets" in kernels
