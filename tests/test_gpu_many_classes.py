"""-m gpu: wide box inference (7..80 classes, COCO's score threshold 0.05) against the CPU oracle.

Small configuration of test_gpu_detector.py (one bottleneck per stage, 270x480 frames resized to 252x448).  The synthetic box
predictor's per-class logit means are centred on the frame's proposals (an oracle run of the uncentred state gives the bias) and
the background, and at 80 classes two of every three classes, are pushed down by 10: the probability mass then sits on 27
classes (1, 4, .., 79), so that at a low gain (small logits, so the f32 bars hold) the frame still has thousands of candidates,
more than 20 classes survive NMS and the 100-detection cut is reached -- asserted below, so a weight change cannot quietly make
the test trivial.  The mask predictor's bias is lifted by 3 so that no detection has an empty mask (the reference's closest-point
step raises on one).
Bars: those of test_single_frame_stages (f32) and test_bf16_mode_vs_bf16_oracle (16-bit modes).
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
GAIN = {80: 2.0, 7: 2.0}             # cls_gain per class count (with the centring bias: see the module docstring)
STEP = {80: 3, 7: 1}                 # classes k with k % STEP == 1 % STEP carry the probability mass


def _cfg(k, dtype=None, batch=1):
    from apse_uav_amd.config import setup_cfg
    cfg = setup_cfg(score_thresh=THRESH, num_classes=k)
    cfg.INPUT.MIN_SIZE_TEST = 256
    cfg.INPUT.MAX_SIZE_TEST = 448
    if dtype:
        cfg.APSE.DTYPE = dtype
        cfg.APSE.STORAGE16 = True
    cfg.APSE.MAX_BATCH = batch
    return cfg


def _log(logdir, name, obj):
    with open(os.path.join(logdir, "many_classes.log"), "a") as f:
        f.write(name + " " + json.dumps(obj) + "\n")


@pytest.fixture(scope="module")
def env():
    from PIL import Image
    from apse_uav_amd.synthetic import SyntheticSequence
    from apse_uav_amd.utils import resample
    from apse_uav_amd.weights import synthetic_association_state, synthetic_detector_state
    from oracle import tracker as otr
    from oracle.detector import DetectorOracle
    seq = SyntheticSequence("dynamic", *FRAME)
    asd = synthetic_association_state(1)
    ih, iw = resample.resize_shortest_edge(FRAME[0], FRAME[1], 256, 448)

    def image(frame):
        img = np.asarray(Image.fromarray(frame).resize((iw, ih), Image.BILINEAR))
        return torch.as_tensor(img.astype("float32").transpose(2, 0, 1))

    def oracle(sd, k, **kw):
        return DetectorOracle(sd, dict(depth_blocks=BLOCKS, min_size=256, max_size=448, num_classes=k, score_thresh=THRESH, **kw))

    states = {}
    x0 = image(seq.frame(0))
    for k, gain in GAIN.items():
        sd = synthetic_detector_state(0, BLOCKS, num_classes=k, cls_gain=gain)
        lp = oracle(sd, k).inference(x0, *FRAME)["box_det"]["probs"].clamp_min(1e-30).log()
        bias = -(lp - lp.mean(1, keepdim=True)).mean(0)          # centre every class's mean logit over the proposals
        quiet = torch.tensor([c % STEP[k] != 1 % STEP[k] or c == k for c in range(k + 1)])
        bias[quiet] -= 10.0
        sd = synthetic_detector_state(0, BLOCKS, num_classes=k, cls_gain=gain, cls_bias=tuple(float(v) for v in bias))
        sd["roi_heads.mask_head.predictor.bias"] += 3.0
        states[k] = sd

    def oracle_frame(k, frame, **kw):
        post = oracle(states[k], k, **kw).inference(image(frame), *FRAME)
        rois = otr.features_rois(post["features"]["p2"], post["boxes"], FRAME[1])
        post["emb"] = otr.association_head(rois, asd["fc.weight"], asd["fc.bias"])
        return post
    return dict(seq=seq, asd=asd, states=states, image=image, oracle=oracle, oracle_frame=oracle_frame, ih=ih, iw=iw)


def _tracker(env, k, **kw):
    from apse_uav_amd.engines.rcnn_tracker import RcnnTracker
    return RcnnTracker(_cfg(k, **kw), FRAME, env["asd"], detector_state=env["states"][k])


@pytest.mark.parametrize("k", [80, 7])
def test_wide_box_inference_f32_vs_oracle(env, logdir, k):
    from hip_helpers import explain_detection_sets, hip_box_side, oracle_box_side
    from oracle import mask_utils as omu
    tr = _tracker(env, k)
    frame = env["seq"].frame(0)
    post = env["oracle_frame"](k, frame)
    pred, _ = tr.predictor(frame)
    inst = pred["instances"]
    model = tr.predictor.model
    # ---- coverage: the configuration exercises what the wide kernels are for
    ncand = int((post["box_det"]["probs"][:, :-1] > THRESH).sum())
    ncls = len(set(post["classes"].tolist()))
    _log(logdir, "f32/k%d/coverage" % k, dict(candidates=ncand, classes=ncls, dets=int(post["boxes"].shape[0])))
    assert ncand >= 1000 and post["boxes"].shape[0] == 100
    assert ncls >= (20 if k == 80 else k)
    # ---- near-threshold flips would have to be explained by the measured noise (none is expected in f32)
    rep, unexplained = explain_detection_sets(hip_box_side(model), oracle_box_side(post), score_thr=THRESH, nms_thr=0.5,
                                              rank_limit=100)
    _log(logdir, "f32/k%d/explain" % k, dict(matched=rep["matched"], only=rep["only"], unexplained=unexplained))
    assert not unexplained, unexplained
    # ---- detections: count, classes and ROI exact; boxes / scores at the f32 bars
    n = len(inst)
    assert n == post["boxes"].shape[0]
    assert torch.equal(inst.pred_classes, post["classes"])
    res = model.last_results
    got_roi = res.roi[res.record(0)["packed_index"]].astype(np.int64)
    assert np.array_equal(got_roi, post["box_det"]["roi_index"][post["keep"]].numpy())
    dbox = float((inst.pred_boxes.tensor - post["boxes"]).abs().max())
    dscore = float((inst.scores - post["scores"]).abs().max())
    _log(logdir, "f32/k%d/dets" % k, dict(n=n, box_max_abs_px=dbox, score_max_abs=dscore))
    assert dbox < 1.3e-4, dbox
    assert dscore < 2e-6, dscore
    # ---- masks (class channel up to 79) and embeddings
    bad_px = 0
    for i in range(n):
        m = inst.pred_masks[i]
        ref_win, ref_rect = post["mask_windows"][i], post["mask_rects"][i]
        assert tuple(m.rect) == tuple(ref_rect)
        bad_px += int((m.window().cpu() != ref_win).sum())
        rc = omu.window_centroid(ref_win, ref_rect)
        if m.mass and not np.isnan(rc[0]):
            assert abs(m.centroid[0] - rc[0]) <= 1 and abs(m.centroid[1] - rc[1]) <= 1
    de = float((torch.from_numpy(inst._record["embeddings"]) - post["emb"]).abs().max())
    _log(logdir, "f32/k%d/masks_emb" % k, dict(mismatched_pixels=bad_px, emb_max_abs=de))
    assert bad_px <= 2
    assert de < 1e-6


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_wide_box_inference_16bit_vs_16bit_oracle(env, logdir, dtype):
    from hip_helpers import explain_frame
    tr = _tracker(env, 80, dtype=dtype)
    frame = env["seq"].frame(0)
    pred, feats = tr.predictor(frame)
    inst = pred["instances"]
    post = env["oracle_frame"](80, frame, bf16=("f16" if dtype == "f16" else True), storage16=True)
    for key in ("p2", "p4", "p6"):
        got, ref = feats[key].cpu(), post["features"][key]
        d = float((got - ref).abs().max() / ref.abs().max())
        mean = float((got - ref).abs().mean() / ref.abs().mean())
        assert d < 3e-2 and mean < 1e-2, (key, d, mean)
    n, rn = len(inst), int(post["boxes"].shape[0])
    rep, unexplained = explain_frame(tr.predictor.model, post)
    _log(logdir, dtype + "/dets", dict(n=n, ref_n=rn, matched=rep["box"]["matched"], only=rep["box"]["only"],
                                       unexplained=unexplained, score_max_abs=rep["box"]["matched_score_max_abs"]))
    assert not unexplained, unexplained
    assert rep["box"]["matched"] >= 1 and rep["box"]["matched"] >= min(n, rn) - len(rep["box"]["only"])
    assert rep["box"]["matched_score_max_abs"] < (5e-3 if dtype == "bf16" else 1e-3)


def test_given_boxes_with_high_class_ids(env, logdir):
    """detected_instances with classes 0, 41 and 79: each mask is the oracle mask head's mask of that class channel."""
    from apse_uav_amd.engines.track_predictor import TrackPredictor
    from apse_uav_amd.structures.instances import Boxes, Instances
    pr = TrackPredictor(_cfg(80), state_dict=env["states"][80])
    x = env["image"](env["seq"].frame(0))
    boxes = torch.tensor([[40.0, 30.0, 120.0, 90.0], [200.5, 100.25, 260.0, 180.75], [300.0, 20.0, 440.0, 160.0]])
    classes = torch.tensor([0, 41, 79])
    det = Instances((env["ih"], env["iw"]))
    det.pred_boxes = Boxes(boxes)
    det.pred_classes = classes
    out, _ = pr.model.inference([{"image": x, "height": FRAME[0], "width": FRAME[1]}], detected_instances=[det])
    inst = out[0]["instances"]
    post = env["oracle"](env["states"][80], 80).inference(x, *FRAME, given_boxes=boxes, given_classes=classes)
    assert len(inst) == 3 == post["boxes"].shape[0]
    assert torch.equal(inst.pred_classes, post["classes"]) and post["classes"].tolist() == [0, 41, 79]
    bad = tot = 0
    for i in range(3):
        m = inst.pred_masks[i]
        assert tuple(m.rect) == tuple(post["mask_rects"][i])
        bad += int((m.window().cpu() != post["mask_windows"][i]).sum())
        tot += int(post["mask_windows"][i].sum())
    _log(logdir, "given", dict(mask_px_mismatch=bad, mask_px=tot))
    assert tot > 0 and bad <= 3


def _image_bytes(model, res, b):
    rec = res.record(b)
    parts = [np.ascontiguousarray(rec[key]).tobytes() for key in
             ("boxes", "scores", "classes", "centroids", "mass", "rects", "closest", "embeddings")]
    for m in model.instances_from(res, b, want_masks=True).pred_masks:
        if m.bits is not None:
            parts.append(m.bits.cpu().numpy().tobytes())
    return len(rec["scores"]), b"".join(parts)


def test_batch4_equals_batch1(env, logdir):
    """One context of max_batch 4 (the GEMM tile shapes are plan constants of the context): each frame of a batch-4 forward
    gives the bytes of its own batch-1 forward."""
    frames = [env["seq"].frame(t) for t in (0, 5, 10, 15)]
    pr = _tracker(env, 80, batch=4).predictor
    one = []
    for fr in frames:
        pr.predict_batch([fr])
        one.append(_image_bytes(pr.model, pr.model.last_results, 0))
    pr.predict_batch(frames)
    got = [_image_bytes(pr.model, pr.model.last_results, b) for b in range(4)]
    _log(logdir, "batch4", dict(n=[g[0] for g in got], n1=[o[0] for o in one]))
    assert all(o[0] > 0 for o in one)
    for b in range(4):
        assert got[b][0] == one[b][0] and got[b][1] == one[b][1], b


def test_tracker_sequence_ids_and_csv(env, logdir):
    from oracle import tracker as otr
    tr = _tracker(env, 80)
    otk = otr.TrackerOracle()
    same = 0
    for t in range(16):
        frame = env["seq"].frame(t)
        rec = tr.next_frame(frame)
        post = env["oracle_frame"](80, frame)
        det = dict(boxes=post["boxes"], scores=post["scores"], classes=post["classes"],
                   masks=list(zip(post["mask_windows"], post["mask_rects"])), emb=post["emb"])
        orec = otk.next_frame(det)
        assert (list(rec.ids) if len(rec) else []) == orec["ids"], t
        same += tr.log_line(rec, 1, t)[0] == otr.log_oneline(orec, 1, t)[0]
    _log(logdir, "tracker", dict(same_lines=same))
    assert same == 16


def test_results_independent_of_history(env, logdir):
    from hip_helpers import history_independence
    outs = history_independence(_tracker(env, 80), env["seq"].frame(0), (env["ih"], env["iw"]))
    _log(logdir, "history", dict(n=[o[0] for o in outs]))
    assert outs[0][0] > 0
    assert outs[0][1] == outs[1][1] == outs[2][1]
