"""CPU: the numpy restatement of association-head training (tests/assoc_train_ref.py) against the golden the reference's
own losses.py / AssociationHead / torch.optim.SGD produced (tests/golden/make_triplet_golden.py); the rleToBbox restatement
on hand-computed cases; the MOTS / MOT ground-truth parsers and the batch bookkeeping of utils/MOT_utils.py."""
import os
import shutil
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
import assoc_train_ref as R  # noqa: E402

CASES = ["seed2", "seed7", "seed48", "seed300", "lonely", "one_label", "neg_is_rowmax", "n1", "dups"]


@pytest.fixture(scope="module")
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, "triplet_golden.npz"))


def _close_grad(got, ref):
    scale = max(float(np.abs(ref).max()), 1e-30)
    return float(np.abs(got - ref).max()) <= 1e-4 * scale + 1e-12


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("squared", [0, 1])
def test_restatement_matches_reference(gold, case, squared):
    lab, e = gold[case + "_labels"], gold[case + "_emb"]
    loss, de = R.batch_hard(lab, e, 0.2, squared)
    assert np.isclose(loss, gold["%s_hard_sq%d_loss" % (case, squared)], rtol=1e-5, atol=1e-7)
    assert _close_grad(de, gold["%s_hard_sq%d_dE" % (case, squared)])
    loss, frac, de = R.batch_all(lab, e, 0.2, squared)
    assert np.isclose(loss, gold["%s_all_sq%d_loss" % (case, squared)], rtol=1e-5, atol=1e-7)
    assert np.isclose(frac, gold["%s_all_sq%d_frac" % (case, squared)], rtol=1e-6, atol=0)
    assert _close_grad(de, gold["%s_all_sq%d_dE" % (case, squared)])


def test_structural_cases(gold):
    # n == 1: the loss is the margin and the gradient 0; one label: the hardest positive is the row maximum and cancels
    for case in ("n1", "one_label"):
        for sq in (0, 1):
            assert float(gold["%s_hard_sq%d_loss" % (case, sq)]) == pytest.approx(0.2)
            assert not gold["%s_hard_sq%d_dE" % (case, sq)].any()
    loss, de = R.batch_hard(np.zeros(0), np.zeros((0, 8), np.float32), 0.2)
    assert np.isnan(loss) and de.shape == (0, 8)


def test_trajectory_matches_reference(gold):
    from make_triplet_golden import traj_inputs
    w0, b0, xs, ids, proj = traj_inputs()
    w, b = w0.numpy().copy(), b0.numpy().copy()
    sw, sb = {}, {}
    losses = []
    for s in range(5):
        x = xs[s].numpy()
        e, inv = R.fc_forward(x, w, b)
        loss, de = R.batch_hard(ids[s].numpy(), e, 0.2)
        dw, db = R.fc_backward(x, e, inv, de)
        w = R.sgd_step(w, dw, sw, 0.01, 0.9)
        b = R.sgd_step(b, db, sb, 0.01, 0.9)
        losses.append(loss)
    np.testing.assert_allclose(losses, gold["traj_losses"], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(b, gold["traj_bias"], rtol=0, atol=1e-5)
    np.testing.assert_allclose(w @ proj.numpy(), gold["traj_wproj"], rtol=0, atol=1e-4)


# ---------------------------------------------------------------- rleToBbox (pycocotools maskApi.c)
@pytest.mark.parametrize("counts,h,w,box", [
    ([16], 4, 4, [0, 0, 0, 0]),                 # empty mask: one run, dropped
    ([], 4, 4, [0, 0, 0, 0]),
    ([5, 3, 2], 4, 4, [1, 1, 1, 3]),            # one column, rows 1..3; trailing zeros run dropped (odd count)
    ([5, 3], 4, 4, [1, 1, 1, 3]),
    ([3, 3, 10], 4, 4, [0, 0, 2, 4]),           # run crosses from column 0 into column 1: ys = 0, ye = h - 1
    ([0, 16], 4, 4, [0, 0, 4, 4]),              # full mask
    ([6, 1, 4, 1, 4], 4, 4, [1, 2, 2, 2]),      # two single pixels: (x 1, y 2) and (x 2, y 3)
    ([9, 2, 1], 3, 4, [3, 0, 1, 2]),            # last column, rows 0..1
])
def test_rle_to_bbox(counts, h, w, box):
    from apse_uav_amd.utils.MOT_utils import rle_to_bbox
    assert rle_to_bbox(counts, h, w) == [float(v) for v in box]


def test_rle_to_bbox_matches_mask_extent():
    from apse_uav_amd.utils import rle
    from apse_uav_amd.utils.MOT_utils import mask_to_bbox
    m = np.zeros((30, 40), np.uint8)
    m[4:9, 7:20] = 1
    m[12, 3] = 1
    assert mask_to_bbox(rle.encode(m)) == [3.0, 4.0, 17.0, 9.0]
    one = np.zeros((30, 40), np.uint8)
    one[10:13, 5] = 1                            # one column: no crossing
    assert mask_to_bbox(rle.encode(one)) == [5.0, 10.0, 1.0, 3.0]


# ---------------------------------------------------------------- MOTS / MOT parsers and batching
def test_mots_parser_and_batches(golden_dir, tmp_path):
    from apse_uav_amd.utils import MOT_utils as M
    from apse_uav_amd.utils import rle
    src = os.path.join(golden_dir, "mots", "gt_txt")
    inst = tmp_path / "instances_txt"
    shutil.copytree(src, inst)
    objs, masks = M.parse_mots_instances(str(inst / "0000.txt"))
    lines = [ln.split(" ") for ln in open(os.path.join(src, "0000.txt")).read().splitlines() if ln.strip()]
    kept = [ln for ln in lines if int(ln[1]) != 10000]
    assert objs.shape == (len(kept), 6) and len(masks) == len(kept)
    assert objs.dtype == np.int64
    for row, ln, mk in zip(objs, kept, masks):
        assert row[0] == int(ln[0]) and row[1] == int(ln[1])
        dense = rle.decode({"size": [int(ln[3]), int(ln[4])], "counts": ln[5]})
        ys, xs = np.nonzero(dense)
        if len(xs):
            x0, x1 = xs.min(), xs.max()
            assert row[2] == x0 and row[4] == x1 - x0 + 1
        assert mk["counts"] == ln[5].strip()
    classes = {int(ln[2]) for ln in kept}
    assert {1, 2} <= classes                     # cars and pedestrians both kept
    frames = M.frames_with_objects(objs)
    assert list(frames) == sorted({int(ln[0]) for ln in kept})
    nb = len(frames) // 3
    got = [M.batch_frames(frames, 3, b) for b in range(nb)]
    assert [f for fs in got for f in fs] == list(frames[:3 * nb])


def test_mots_parser_drops_ignore_regions(tmp_path):
    from apse_uav_amd.utils import MOT_utils as M
    from apse_uav_amd.utils import rle
    m = np.zeros((10, 12), np.uint8)
    m[2:5, 3:6] = 1
    s = rle.encode(m)["counts"].decode()
    p = tmp_path / "s.txt"
    p.write_text("0 1001 1 10 12 %s\n0 10000 10 10 12 %s\n2 2003 2 10 12 %s\n" % (s, s, s))
    objs, masks = M.parse_mots_instances(str(p))
    assert objs.tolist() == [[0, 1001, 3, 2, 3, 3], [2, 2003, 3, 2, 3, 3]]
    assert len(masks) == 2


def test_mot_parser(tmp_path):
    from apse_uav_amd.utils import MOT_utils as M
    seq = tmp_path / "MOT-01"
    (seq / "gt").mkdir(parents=True)
    (seq / "seqinfo.ini").write_text("[Sequence]\nname=MOT-01\nimDir=img1\nframeRate=25\nseqLength=17\nimWidth=64\nimHeight=48\n")
    (seq / "gt" / "gt.txt").write_text("1,1,10,12,20,30,1,1,1.0\n1,2,5,6,7,8,0,1,1.0\n2,1,11,12,20,30,1,1,0.5\n")
    info = M.read_seqinfo(str(seq))
    assert info["seqLength"] == "17" and info["imWidth"] == "64"
    gt = M.parse_mot_gt(str(seq / "gt" / "gt.txt"))
    assert gt.tolist() == [[1, 1, 10, 12, 20, 30, 1], [2, 1, 11, 12, 20, 30, 1]]


def test_object_rows_width():
    from apse_uav_amd.engines.roi_features_generator import _object_rows
    six = np.array([[0, 1005, 10, 20, 30, 40], [0, 2001, 1, 2, 3, 4]] * 7)       # 14 rows: a multiple of 7
    r = _object_rows(six)
    assert r.shape == (14, 6) and r[1].tolist() == [0, 2001, 1, 2, 3, 4]
    seven = [[3, 11, 40.0, 30.0, 120.5, 60.25, 1], [3, 7, 200.0, 100.0, 90.0, 150.0, 1]]
    assert _object_rows(seven).tolist() == seven
    assert _object_rows(np.array(seven).reshape(-1)).tolist() == seven            # flat 7-column input, as before
    assert _object_rows(np.zeros((0, 7))).shape == (0, 7) and _object_rows([]).shape == (0, 7)
