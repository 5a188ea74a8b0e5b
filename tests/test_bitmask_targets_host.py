"""Host side of bitmask ground truth (no GPU): the numpy reference of ``apse_bitmask_targets`` (tests/bitmask_ref.py) against the
oracle's ROIAlign and against itself in float64 on an exact lattice, ``nearest_maps`` against Pillow, the MOTS dataset
dictionaries, the dataset's mask_format switch and the declarations of the two entries."""
import json
import os
import re
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)

import bitmask_ref as br                                     # noqa: E402


# ---------------------------------------------------------------- the reference
def test_reference_averages_equal_the_oracle_roi_align_within_its_summation_error():
    """oracle.ops.roi_align_v2 computes the same samples and weights in float32 and differs only in the ORDER of the sum over a
    cell's samples (torch.sum over the two grid axes against one accumulator).  Two float32 sums of the same n terms in [0, 1]
    differ by at most 2 (n - 1) u times the sum, u = 2^-24, and the average of a 0 / 1 mask is at most 1.  Measured on these
    cases: at most 1.79e-7 (three ulps of 0.5 .. 1, grids up to 24 samples), and 0 for every box with one sample per cell."""
    from oracle.ops import roi_align_v2
    rng = np.random.default_rng(11)
    h, w = 40, 56
    worst = 0.0
    for dense in br.blobs(rng, h, w, 3):
        rois = br.random_rois(rng, h, w, 30)
        for ms in (28, 14):
            mine = br.ref_averages(dense, rois, np.float32, ms)
            want = roi_align_v2(torch.from_numpy(dense.astype(np.float32))[None], torch.from_numpy(rois), 1.0, ms)[:, 0].numpy()
            n = np.maximum(br.samples_per_cell(rois, ms), 1)
            diff = np.abs(mine - want).reshape(len(rois), -1).max(axis=1)
            worst = max(worst, float(diff.max()))
            assert (diff <= 2.0 * (n - 1) * 2.0 ** -24).all(), (ms, diff.max())
            assert (n > 1).any() and (n == 1).any()
    print("largest difference from oracle.ops.roi_align_v2: %.3g" % worst)


def lattice_cases():
    """Boxes with corners at integer + 0.5 and extents 28 * 2^j (j = 0, 1, 2) and 14 over 96 x 160 masks: every coordinate is a
    multiple of 1/4, every weight a multiple of 1/16 and every sum a multiple of 1/16 below 2^8 -- all exact in float32.  The
    half-plane masks put whole rows (and columns) of cells at exactly 0.5."""
    h, w = 96, 160
    yy, xx = np.mgrid[0:h, 0:w]
    masks = [yy < 40, xx >= 77, (yy >= 20) & (yy < 61) & (xx >= 30) & (xx < 130), ((yy // 3 + xx // 5) % 2) == 0,
             (yy + xx) % 2 == 0]
    rois = []
    for ext_w, ext_h in ((28, 28), (56, 56), (112, 112), (14, 14), (28, 56), (112, 14), (14, 112)):
        for x1, y1 in ((10.5, 12.5), (63.5, 25.5), (-3.5, -5.5), (100.5, 70.5), (48.5, 11.5)):
            rois.append((x1, y1, x1 + ext_w, y1 + ext_h))
    return masks, np.array(rois, np.float32)


def test_exact_lattice_f32_and_f64_agree_on_every_cell_ties_included():
    masks, rois = lattice_cases()
    ties = 0
    for dense in masks:
        for ms in (28, 14):
            a32, a64 = br.ref_averages(dense, rois, np.float32, ms), br.ref_averages(dense, rois, np.float64, ms)
            assert np.array_equal(a32.astype(np.float64), a64)
            assert np.array_equal(br.ref_targets(dense, rois, np.float32, ms), br.ref_targets(dense, rois, np.float64, ms))
            ties += int((a64 == 0.5).sum())
    assert ties > 0
    # the half-plane y < 40 under the box (10.5, 12.5, 38.5, 40.5): cell row ph samples y = 12.5 + ph, so ph = 27 sits between
    # the last set row 39 and the first clear row 40: exactly 0.5 along the whole row, and a 1
    avg = br.ref_averages(masks[0], rois[:1], np.float32)[0]
    assert (avg[27] == 0.5).all() and (avg[:27] == 1.0).all()
    assert (br.ref_targets(masks[0], rois[:1], np.float32)[0][27] == 1).all()


def test_degenerate_boxes_and_unmatched_rows_are_zero():
    dense = np.ones((20, 30), bool)
    rois = np.array([[5, 5, 5, 12], [9, 9, 4, 12], [3, 3, 12, 3], [np.nan, 1, 5, 5], [2, 2, 20, 14]], np.float32)
    t = br.ref_targets(dense, rois, np.float32)
    assert t[:4].sum() == 0 and t[4].all()
    rows = br.ref_rows([dense], rois[[4, 4, 4]], [-1, 1, 0], np.float32)
    assert rows[0].sum() == 0 and rows[1].sum() == 0 and rows[2].all()


# ---------------------------------------------------------------- nearest_maps
SIZES = ((3840, 1333), (2160, 750), (375, 402), (1242, 1333), (7, 5), (5, 7))


@pytest.mark.parametrize("src,dst", SIZES)
def test_nearest_maps_is_pillows_resize_of_a_ramp(src, dst):
    from apse_uav_amd.utils.COCO_utils import nearest_maps
    for vertical in (False, True):
        m = nearest_maps(src, dst, vertical=vertical)
        assert m.dtype == np.int32 and m.shape == (dst,)
        assert np.array_equal(m, br.pillow_map(src, dst, vertical))
        assert (np.diff(m) >= 0).all() and m.min() >= 0 and m.max() < src


def test_nearest_maps_2160_to_750_is_not_the_floor_formula():
    from apse_uav_amd.utils.COCO_utils import nearest_maps
    m = nearest_maps(2160, 750)
    formula = np.floor((np.arange(750) + 0.5) * 2160 / 750).astype(np.int64)
    assert np.array_equal(m, br.pillow_map(2160, 750))
    print("2160 -> 750: %d of 750 positions differ from floor((x + 0.5) * src / dst)" % int((m != formula).sum()))


@pytest.mark.parametrize("hw,out", (((96, 160), (60, 100)), ((96, 160), (150, 250)), ((37, 41), (50, 33))))
def test_both_flip_orders_equal_flipping_the_dense_mask(hw, out):
    from PIL import Image
    from apse_uav_amd.utils.COCO_utils import nearest_maps
    (H, W), (h, w) = hw, out
    dense = br.blobs(np.random.default_rng(3), H, W, 1)[0].astype(np.uint8)
    ymap = nearest_maps(H, h, vertical=True)

    def resize(m):
        return np.asarray(Image.fromarray(m).resize((w, h), Image.NEAREST))
    assert np.array_equal(br.gather(dense, nearest_maps(W, w), ymap), resize(dense))
    assert np.array_equal(br.gather(dense, nearest_maps(W, w, flip_before=True), ymap), resize(dense[:, ::-1].copy()))
    assert np.array_equal(br.gather(dense, nearest_maps(W, w, flip_after=True), ymap), resize(dense)[:, ::-1])
    assert np.array_equal(br.gather(dense, nearest_maps(W, w, True, True), ymap), resize(dense[:, ::-1].copy())[:, ::-1])


# ---------------------------------------------------------------- datasets
def test_mots_dataset_dictionaries(tmp_path):
    from apse_uav_amd.synthetic import write_synthetic_mots
    from apse_uav_amd.utils import rle
    from apse_uav_amd.utils.MOT_utils import generate_mots_dataset_dictionaries, parse_mots_instances
    root = str(tmp_path / "mots")
    seqmap = write_synthetic_mots(root, frames=6)
    dicts = generate_mots_dataset_dictionaries(root, seqmap)
    want_frames, want_objects = 0, 0
    for seq in ("0000", "0001"):
        rows, _ = parse_mots_instances(os.path.join(root, "instances_txt", seq + ".txt"))        # (drops the ignore regions)
        want_frames += len(np.unique(rows[:, 0]))
        want_objects += len(rows)
    assert len(dicts) == want_frames and sum(len(d["annotations"]) for d in dicts) == want_objects and want_objects > 0
    assert len({d["image_id"] for d in dicts}) == len(dicts)
    assert {d["sequence"] for d in dicts} == {"0000", "0001"} and all(d["frame"] != 1 for d in dicts)
    classes = set()
    for d in dicts:
        assert os.path.exists(d["file_name"]) and (d["height"], d["width"]) == (160, 288)
        assert d["proposal_boxes"].shape == (len(d["annotations"]), 4)
        for a in d["annotations"]:
            assert a["track_id"] != 10000 and a["category_id"] == a["track_id"] // 1000 - 1 and a["category_id"] in (0, 1)
            classes.add(a["category_id"])
            m = rle.decode(a["segmentation"])
            ys, xs = np.nonzero(m)
            assert a["bbox"] == [float(xs.min()), float(ys.min()), float(xs.max() - xs.min() + 1), float(ys.max() - ys.min() + 1)]
            assert not m[:8, :16].all()                                  # (the ignore region's pixels)
    assert classes == {0, 1}
    os.remove(dicts[0]["file_name"])
    with pytest.raises(FileNotFoundError, match=os.path.basename(dicts[0]["file_name"])):
        generate_mots_dataset_dictionaries(root, seqmap)


def test_mots_dataset_dictionaries_from_id_map_pngs(tmp_path):
    from PIL import Image
    from apse_uav_amd.utils import rle
    from apse_uav_amd.utils.MOT_utils import generate_mots_dataset_dictionaries
    root = tmp_path / "mots"
    (root / "instances" / "0003").mkdir(parents=True)
    (root / "training" / "image_02" / "0003").mkdir(parents=True)
    idmap = np.zeros((24, 40), np.uint16)
    idmap[2:9, 3:11] = 1001
    idmap[10:20, 20:38] = 2004
    idmap[0:4, 30:40] = 10000
    Image.fromarray(idmap).save(str(root / "instances" / "0003" / "000005.png"))
    Image.fromarray(np.zeros((24, 40, 3), np.uint8)).save(str(root / "training" / "image_02" / "0003" / "000005.png"))
    (root / "s.seqmap").write_text("0003 empty 000000 000009\n")
    dicts = generate_mots_dataset_dictionaries(str(root), str(root / "s.seqmap"))
    assert len(dicts) == 1 and dicts[0]["frame"] == 5 and (dicts[0]["height"], dicts[0]["width"]) == (24, 40)
    anns = dicts[0]["annotations"]
    assert [a["category_id"] for a in anns] == [0, 1] and [a["bbox"] for a in anns] == [[3.0, 2.0, 8.0, 7.0], [20.0, 10.0, 18.0, 10.0]]
    assert np.array_equal(rle.decode(anns[1]["segmentation"]), idmap == 2004)


def _coco_file(tmp_path, seg):
    path = str(tmp_path / "a.json")
    data = dict(images=[dict(id=1, file_name="a.png", height=20, width=30)], categories=[dict(id=1, name="car")],
                annotations=[dict(id=1, image_id=1, category_id=1, bbox=[2, 3, 10, 8], area=80, iscrowd=0, segmentation=seg),
                             dict(id=2, image_id=1, category_id=1, bbox=[1, 1, 4, 4], area=16, iscrowd=0,
                                  segmentation=[[1, 1, 5, 1, 5, 5, 1, 5]])])
    with open(path, "w") as fh:
        json.dump(data, fh)
    return path


def test_dataset_format_switch(tmp_path):
    from apse_uav_amd.utils import rle
    from apse_uav_amd.utils.COCO_utils import detectron2_dataset_to_coco, generate_coco_dataset_dictionaries
    m = np.zeros((20, 30), np.uint8)
    m[3:11, 2:12] = 1
    seg = {"size": [20, 30], "counts": rle.encode(m)["counts"].decode("ascii")}
    path = _coco_file(tmp_path, seg)
    with pytest.raises(ValueError, match="RLE"):
        generate_coco_dataset_dictionaries(path, str(tmp_path))
    with pytest.raises(ValueError, match="RLE"):
        generate_coco_dataset_dictionaries(path, str(tmp_path), mask_format="polygon")
    with pytest.raises(ValueError, match="mask_format"):
        generate_coco_dataset_dictionaries(path, str(tmp_path), mask_format="rle")
    dicts = generate_coco_dataset_dictionaries(path, str(tmp_path), mask_format="bitmask")
    anns = dicts[0]["annotations"]
    assert anns[0]["segmentation"] == seg and anns[1]["segmentation"] == [[1.0, 1.0, 5.0, 1.0, 5.0, 5.0, 1.0, 5.0]]
    back = detectron2_dataset_to_coco(dicts)
    assert back["annotations"][0]["segmentation"] == seg
    # a polygon-only file gives the same dictionaries under either format
    poly = _coco_file(tmp_path, [[2, 3, 12, 3, 12, 11, 2, 11]])
    a, b = generate_coco_dataset_dictionaries(poly, str(tmp_path)), generate_coco_dataset_dictionaries(poly, str(tmp_path), mask_format="bitmask")
    assert json.dumps(a, default=lambda v: v.tolist()) == json.dumps(b, default=lambda v: v.tolist())


def test_select_mask_rows_takes_has_mask():
    from apse_uav_amd.utils.COCO_utils import select_mask_rows
    labels, matched = np.array([0, 4, 1, -1, 2, 1]), np.array([0, 1, 2, 0, 5, 1])
    rows, skipped = select_mask_rows(labels, matched, np.array([True, False, True]), 4)
    assert rows.tolist() == [0, 2] and skipped == 2
    assert select_mask_rows(labels, matched, np.array([3, 0, 1]), 4)[0].tolist() == [0, 2]


# ---------------------------------------------------------------- the C ABI's declarations and the command line
def test_the_two_entries_are_declared_everywhere():
    from apse_uav_amd import _lib
    header = open(os.path.join(ROOT, "include", "apse_hip.h")).read()
    kernels = open(os.path.join(ROOT, "apse_uav_amd", "csrc", "apse_kernels.h")).read()
    makefile = open(os.path.join(ROOT, "apse_uav_amd", "csrc", "Makefile")).read()
    assert re.search(r"\bint\s+apse_mots_remap_windows\s*\(", header) and re.search(r"\bint\s+apse_bitmask_targets\s*\(", header)
    assert "apse_k_remap_windows" in kernels and "apse_k_bitmask_targets" in kernels and "bitmask_targets.hip" in makefile
    assert len(_lib.SIGNATURES["apse_mots_remap_windows"][0]) == 11 and len(_lib.SIGNATURES["apse_bitmask_targets"][0]) == 10
    assert re.search(r"#define\s+APSE_BITMASK_MAX_SIZE\s+64\b", header)


def test_command_line_flags():
    import argparse
    from apse_uav_amd.utils import finetune as ft
    ap = argparse.ArgumentParser()
    ft.add_common_arguments(ap, "X")
    a = ap.parse_args(["--out", "o"])
    assert a.mask_format == "polygon" and a.mots == "" and ft.mask_format(a) == "polygon"
    assert ft.mask_format(ap.parse_args(["--out", "o", "--mask-format", "bitmask"])) == "bitmask"
    b = ap.parse_args(["--out", "o", "--mots", "D", "--seqmap", "S"])
    assert (b.mots, b.seqmap) == ("D", "S") and ft.mask_format(b) == "bitmask"
    assert ft.mask_format(ap.parse_args(["--out", "o", "--synthetic", "4", "--mots"])) == "bitmask"
