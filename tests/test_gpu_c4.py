"""-m gpu: C4 (Res5ROIHeads) checkpoints end to end in HIP against the CPU C4 reference (tests/c4_ref.py).

Small configuration (one bottleneck per stage, res5 included): 270x480 frames resized to 252x448, so res4 is 16 x 28 and the
RPN sees 6720 anchors -- the 6000 pre-NMS cut really happens.  Score threshold 0.05 with the box predictor's class logits
centred on the frame's proposals: every proposal yields candidates and the 100-detection cut is reached.  The mask predictor's
bias is lifted by 3 so no mask is empty.  Bars: those of test_single_frame_stages (f32).
"""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

BLOCKS = (1, 1, 1, 1)
FRAME = (270, 480)
THRESH = 0.05


def _cfg(k=4, batch=1, thresh=THRESH):
    from apse_uav_amd.config import setup_cfg
    cfg = setup_cfg(score_thresh=thresh, num_classes=k, arch="C4")
    cfg.INPUT.MIN_SIZE_TEST = 256
    cfg.INPUT.MAX_SIZE_TEST = 448
    cfg.APSE.MAX_BATCH = batch
    return cfg


def _log(logdir, name, obj):
    with open(os.path.join(logdir, "c4.log"), "a") as f:
        f.write(name + " " + json.dumps(obj) + "\n")


@pytest.fixture(scope="module")
def env():
    from PIL import Image
    from apse_uav_amd.synthetic import SyntheticSequence
    from apse_uav_amd.utils import resample
    from apse_uav_amd.weights import synthetic_association_state, synthetic_c4_state
    from c4_ref import C4Oracle
    from oracle import tracker as otr
    seq = SyntheticSequence("dynamic", *FRAME)
    asd = synthetic_association_state(1, depth=1024)
    ih, iw = resample.resize_shortest_edge(FRAME[0], FRAME[1], 256, 448)

    def image(frame):
        img = np.asarray(Image.fromarray(frame).resize((iw, ih), Image.BILINEAR))
        return torch.as_tensor(img.astype("float32").transpose(2, 0, 1))

    def oracle(sd, k, thresh=THRESH):
        return C4Oracle(sd, dict(depth_blocks=BLOCKS, num_classes=k, score_thresh=thresh))

    states = {}
    x0 = image(seq.frame(0))
    for k in (4, 80):
        sd = synthetic_c4_state(0, BLOCKS, num_classes=k, cls_gain=2.0)
        lp = oracle(sd, k).inference(x0, *FRAME)["box_det"]["probs"].clamp_min(1e-30).log()
        bias = -(lp - lp.mean(1, keepdim=True)).mean(0)
        bias[k] -= 10.0                                               # background down: every ROI has candidates
        if k > 8:
            quiet = torch.arange(k + 1) % 8 != 1                      # 80 classes: the mass on 10 of them, above 0.05
            quiet[k] = False
            bias[quiet] -= 10.0
        sd = synthetic_c4_state(0, BLOCKS, num_classes=k, cls_gain=2.0, cls_bias=tuple(float(v) for v in bias))
        sd["roi_heads.mask_head.predictor.bias"] += 3.0
        states[k] = sd

    def oracle_frame(k, frame, thresh=THRESH):
        post = oracle(states[k], k, thresh).inference(image(frame), *FRAME)
        if post["boxes"].shape[0] == 0:
            post["emb"] = torch.zeros((0, asd["fc.weight"].shape[0]))
            return post
        rois = otr.features_rois(post["features"]["res4"], post["boxes"], FRAME[1])
        post["emb"] = otr.association_head(rois, asd["fc.weight"], asd["fc.bias"])
        return post
    return dict(seq=seq, asd=asd, states=states, image=image, oracle=oracle, oracle_frame=oracle_frame, ih=ih, iw=iw)


def _tracker(env, k=4, **kw):
    from apse_uav_amd.engines.rcnn_tracker import RcnnTracker
    return RcnnTracker(_cfg(k, **kw), FRAME, env["asd"], detector_state=env["states"][k])


def _check_frame(env, logdir, tr, post, inst, feats, k, tag):
    from hip_helpers import explain_detection_sets, hip_box_side, oracle_box_side
    from oracle import mask_utils as omu
    model = tr.predictor.model
    res = model.last_results
    # ---- res4
    assert list(feats.keys()) == ["res4"]
    got4, ref4 = feats["res4"].cpu(), post["features"]["res4"]
    assert got4.shape == ref4.shape, (got4.shape, ref4.shape)
    d4 = float((got4 - ref4).abs().max() / ref4.abs().max())
    # ---- proposals: same count, same order
    pr = post["proposals"]
    npro = int(res.prop_count[0])
    props = model.debug_tensor("proposals")[: npro * 4].view(npro, 4).cpu()
    dprop = float((props - pr["boxes"]).abs().max()) if npro else 0.0
    _log(logdir, tag + "/coverage", dict(anchors=pr["n_anchors"], valid=pr["n_valid"], nms_kept=pr["n_nms_kept"], proposals=npro,
                                         dets=int(post["boxes"].shape[0]), res4_rel=d4, prop_max_abs_px=dprop))
    # near-tied objectness logits (f32 noise of the 3x3 / 1x1 head, ~1e-6) may swap neighbouring proposals: such a swap is
    # accepted, and logged, when both boxes are the reference's at the other position with a logit within 1e-5
    psc = model.debug_tensor("proposal_scores").cpu()[:npro]
    perm = list(range(npro))
    swaps = []
    for i in range(npro):
        if float((props[i] - pr["boxes"][i]).abs().max()) <= 1.3e-4:
            continue
        cand = [j for j in range(max(0, i - 3), min(npro, i + 4))
                if float((props[i] - pr["boxes"][j]).abs().max()) <= 1.3e-4 and abs(float(psc[i] - pr["logits"][j])) <= 1e-5]
        assert cand, ("unexplained proposal", i, props[i].tolist(), pr["boxes"][i].tolist())
        perm[i] = cand[0]
        swaps.append((i, cand[0], float(psc[i]), float(pr["logits"][cand[0]])))
    assert sorted(perm) == list(range(npro))
    dprop = max((float((props[i] - pr["boxes"][perm[i]]).abs().max()) for i in range(npro)), default=0.0)
    _log(logdir, tag + "/proposal_swaps", dict(swaps=swaps, prop_max_abs_px=dprop))
    assert pr["n_anchors"] > 6000 and pr["n_nms_kept"] < pr["n_valid"]          # the 6000 cut and NMS suppression happen
    assert npro == pr["boxes"].shape[0]
    assert d4 < 1e-5, d4
    assert dprop <= 1.3e-4, dprop
    # ---- detections
    rep, unexplained = explain_detection_sets(hip_box_side(model), oracle_box_side(post), score_thr=THRESH, nms_thr=0.5,
                                              rank_limit=100)
    assert not unexplained, unexplained
    n = len(inst)
    assert n == post["boxes"].shape[0] and n > 0
    assert torch.equal(inst.pred_classes, post["classes"])
    got_roi = res.roi[res.record(0)["packed_index"]].astype(np.int64)
    assert np.array_equal(np.asarray(perm, np.int64)[got_roi], post["box_det"]["roi_index"][post["keep"]].numpy())
    dbox = float((inst.pred_boxes.tensor - post["boxes"]).abs().max())
    dscore = float((inst.scores - post["scores"]).abs().max())
    # ---- masks and embeddings
    bad_px = 0
    for i in range(n):
        m = inst.pred_masks[i]
        assert tuple(m.rect) == tuple(post["mask_rects"][i])
        bad_px += int((m.window().cpu() != post["mask_windows"][i]).sum())
        rc = omu.window_centroid(post["mask_windows"][i], post["mask_rects"][i])
        if m.mass and not np.isnan(rc[0]):
            assert abs(m.centroid[0] - rc[0]) <= 1 and abs(m.centroid[1] - rc[1]) <= 1
    de = float((torch.from_numpy(inst._record["embeddings"]) - post["emb"]).abs().max())
    _log(logdir, tag + "/dets", dict(n=n, box_max_abs_px=dbox, score_max_abs=dscore, mismatched_pixels=bad_px, emb_max_abs=de))
    assert dbox < 1.3e-4, dbox
    assert dscore < 2e-6, dscore
    assert bad_px <= 2, bad_px
    assert de < 1e-6, de


@pytest.mark.parametrize("k", [4, 80])
def test_c4_single_frame_vs_reference(env, logdir, k):
    tr = _tracker(env, k)
    frame = env["seq"].frame(0)
    pred, feats = tr.predictor(frame)
    post = env["oracle_frame"](k, frame)
    assert post["boxes"].shape[0] == 100                  # the full detection list
    _check_frame(env, logdir, tr, post, pred["instances"], feats, k, "k%d" % k)


def test_c4_given_boxes(env, logdir):
    from apse_uav_amd.engines.track_predictor import TrackPredictor
    from apse_uav_amd.structures.instances import Boxes, Instances
    pr = TrackPredictor(_cfg(4), state_dict=env["states"][4])
    x = env["image"](env["seq"].frame(0))
    boxes = torch.tensor([[40.0, 30.0, 120.0, 90.0], [200.5, 100.25, 260.0, 180.75], [300.0, 20.0, 440.0, 160.0]])
    classes = torch.tensor([0, 3, 2])
    det = Instances((env["ih"], env["iw"]))
    det.pred_boxes = Boxes(boxes)
    det.pred_classes = classes
    out, feats = pr.model.inference([{"image": x, "height": FRAME[0], "width": FRAME[1]}], detected_instances=[det])
    inst = out[0]["instances"]
    post = env["oracle"](env["states"][4], 4).inference(x, *FRAME, given_boxes=boxes, given_classes=classes)
    assert len(inst) == 3 == post["boxes"].shape[0]
    bad = tot = 0
    for i in range(3):
        m = inst.pred_masks[i]
        assert tuple(m.rect) == tuple(post["mask_rects"][i])
        bad += int((m.window().cpu() != post["mask_windows"][i]).sum())
        tot += int(post["mask_windows"][i].sum())
    _log(logdir, "given", dict(mask_px_mismatch=bad, mask_px=tot))
    assert tot > 0 and bad <= 2


def test_c4_no_detection_above_threshold(env, logdir):
    """Score threshold 0.999: no candidate; the forward gives an empty list, masks and embeddings included."""
    from apse_uav_amd.engines.rcnn_tracker import RcnnTracker
    tr = RcnnTracker(_cfg(4, thresh=0.999), FRAME, env["asd"], detector_state=env["states"][4])
    pred, _ = tr.predictor(env["seq"].frame(0))
    post = env["oracle_frame"](4, env["seq"].frame(0), thresh=0.999)
    assert len(pred["instances"]) == 0 == post["boxes"].shape[0]
    assert int(tr.predictor.model.last_results.prop_count[0]) == post["proposals"]["boxes"].shape[0]


def _image_bytes(model, res, b):
    rec = res.record(b)
    parts = [np.ascontiguousarray(rec[key]).tobytes() for key in
             ("boxes", "scores", "classes", "centroids", "mass", "rects", "closest", "embeddings")]
    for m in model.instances_from(res, b, want_masks=True).pred_masks:
        if m.bits is not None:
            parts.append(m.bits.cpu().numpy().tobytes())
    return len(rec["scores"]), b"".join(parts)


def test_c4_batch2_equals_batch1(env, logdir):
    frames = [env["seq"].frame(t) for t in (0, 7)]
    pr = _tracker(env, 4, batch=2).predictor
    one = []
    for fr in frames:
        pr.predict_batch([fr])
        one.append(_image_bytes(pr.model, pr.model.last_results, 0))
    pr.predict_batch(frames)
    got = [_image_bytes(pr.model, pr.model.last_results, b) for b in range(2)]
    assert all(o[0] > 0 for o in one)
    for b in range(2):
        assert got[b][0] == one[b][0] and got[b][1] == one[b][1], b


def test_c4_results_independent_of_history(env, logdir):
    from hip_helpers import history_independence
    outs = history_independence(_tracker(env, 4), env["seq"].frame(0), (env["ih"], env["iw"]))
    assert outs[0][0] > 0
    assert outs[0][1] == outs[1][1] == outs[2][1]


def test_c4_tracker_sequence_ids_and_csv(env, logdir):
    from apse_uav_amd.engines.pipelined_tracker import PipelinedRcnnTracker
    from oracle import tracker as otr
    tr = _tracker(env, 4)
    otk = otr.TrackerOracle()
    same, ids = 0, []
    for t in range(16):
        frame = env["seq"].frame(t)
        rec = tr.next_frame(frame)
        post = env["oracle_frame"](4, frame)
        det = dict(boxes=post["boxes"], scores=post["scores"], classes=post["classes"],
                   masks=list(zip(post["mask_windows"], post["mask_rects"])), emb=post["emb"])
        orec = otk.next_frame(det)
        got = list(rec.ids) if len(rec) else []
        assert got == orec["ids"], t
        ids.append(got)
        same += tr.log_line(rec, 1, t)[0] == otr.log_oneline(orec, 1, t)[0]
    _log(logdir, "tracker", dict(same_lines=same))
    assert same == 16
    drv = PipelinedRcnnTracker(_cfg(4), FRAME, env["asd"], depth=2, detector_state=env["states"][4])
    got = [list(r.ids) if len(r) else [] for _, r in drv.run([env["seq"].frame(t) for t in range(16)])]
    assert got == ids
