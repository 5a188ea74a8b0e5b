"""-m gpu: frames whose width is not a multiple of 4, end to end.

Sizes: 375 x 1242 (KITTI MOTS, W % 4 = 2), 721 x 1283 (3), 1080 x 1918 (2), 217 x 389 (1).  The rows of such frames start at
every byte alignment, so the horizontal resize pass stages them with its unaligned-row branch (csrc/elementwise.hip,
pil_stage_row).  The default MIN/MAX_SIZE_TEST 800 / 1333 are kept: three of the sizes are UPSCALED by the shortest-edge
resize (375 x 1242 -> 402 x 1333, three-tap filters).  Small trunk (one bottleneck per stage) and synthetic weights, as in
test_gpu_detector.py, so that the CPU oracle finishes in seconds.  Bars and tolerances are those of test_gpu_detector.py
unless a check says otherwise.
"""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

BLOCKS = (1, 1, 1, 1)
KITTI = (375, 1242)
SIZES = [KITTI, (721, 1283), (1080, 1918), (217, 389)]
MEAN = (103.530, 116.280, 123.675)


def _cfg(batch=1, dtype="f32"):
    from apse_uav_amd.config import setup_cfg
    cfg = setup_cfg()
    cfg.APSE.MAX_BATCH = batch
    cfg.APSE.DTYPE = dtype
    return cfg


def _log(logdir, name, obj):
    with open(os.path.join(logdir, "frame_sizes.log"), "a") as f:
        f.write(name + " " + json.dumps(obj) + "\n")


def _pillow(frame, oh, ow):
    from PIL import Image
    return np.asarray(Image.fromarray(frame).resize((ow, oh), Image.BILINEAR))


@pytest.fixture(scope="module")
def env():
    from apse_uav_amd.weights import synthetic_association_state, synthetic_detector_state
    return dict(sd=synthetic_detector_state(0, BLOCKS), asd=synthetic_association_state(1))


def _oracle_frame(env, frame, hw, bf16=False):
    from oracle import tracker as otr
    from oracle.detector import DetectorOracle
    from apse_uav_amd.utils import resample
    opts = dict(depth_blocks=BLOCKS, min_size=800, max_size=1333)
    if bf16:
        opts.update(bf16=True, storage16=True)
    ih, iw = resample.resize_shortest_edge(hw[0], hw[1], 800, 1333)
    img = _pillow(frame, ih, iw)
    post = DetectorOracle(env["sd"], opts).inference(torch.as_tensor(img.astype("float32").transpose(2, 0, 1)), hw[0], hw[1])
    rois = otr.features_rois(post["features"]["p2"], post["boxes"], hw[1])
    post["emb"] = otr.association_head(rois, env["asd"]["fc.weight"], env["asd"]["fc.bias"])
    return post


# ---------------------------------------------------------------------------------------------------- 1. stateless resize
def _resize_case(H, W, oh, ow, seed):
    from apse_uav_amd import _lib
    from apse_uav_amd.utils import resample
    img = np.random.default_rng(seed).integers(0, 256, (H, W, 3), dtype=np.uint8)
    ref = _pillow(img, oh, ow)
    hb, hc, hk = resample.precompute_coeffs(W, ow)
    vb, vc, vk = resample.precompute_coeffs(H, oh)
    ph, pw = (oh + 31) // 32 * 32, (ow + 31) // 32 * 32
    src = torch.from_numpy(img).cuda()
    tmp = torch.empty((H, ow, 3), dtype=torch.uint8, device="cuda")
    out = torch.zeros((1, ph, pw, 4), device="cuda")
    rs = torch.empty((oh, ow, 3), dtype=torch.uint8, device="cuda")
    t = [torch.from_numpy(a).cuda() for a in (hb, hc, vb, vc)]
    mean = (C.c_float * 3)(*MEAN)
    rc = _lib.load().apse_resize_normalize(_lib.ptr(src), _lib.ptr(tmp), _lib.ptr(out), _lib.ptr(rs), _lib.ptr(t[0]), _lib.ptr(t[1]), hk,
                                           _lib.ptr(t[2]), _lib.ptr(t[3]), vk, 1, H, W, oh, ow, ph, pw, C.byref(mean), _lib.stream_ptr())
    assert rc == 0
    torch.cuda.synchronize()
    got = rs.cpu().numpy()
    o = out.cpu()[0]
    exp = torch.from_numpy(ref.astype(np.float32)) - torch.tensor(MEAN)
    return hk, int((got != ref).sum()), o, exp


RESIZE_CASES = [
    # (H, W, output (oh, ow) or None = shortest edge 800 / 1333, expected taps)
    (375, 1242, None, 3),            # upscale to 402 x 1333
    (721, 1283, None, 3),
    (1080, 1918, None, 5),           # downscale 1918 -> 1333
    (217, 389, None, 3),
    (1080, 1918, (114, 203), 21),    # > 8 taps: the per-sample form (pil_resize_h)
    (5, 7, (3, 4), None),            # tiny frame, explicit output size
    (5, 7, (11, 13), None),
]


@pytest.mark.parametrize("case", RESIZE_CASES, ids=["%dx%d%s" % (c[0], c[1], "" if c[2] is None else "_to_%dx%d" % c[2]) for c in RESIZE_CASES])
def test_resize_normalize_equals_pillow(case, logdir):
    from apse_uav_amd.utils import resample
    H, W, osz, want_k = case
    oh, ow = osz if osz is not None else resample.resize_shortest_edge(H, W, 800, 1333)
    hk, nd, o, exp = _resize_case(H, W, oh, ow, seed=H * 31 + W)
    _log(logdir, "resize/%dx%d->%dx%d" % (H, W, oh, ow), dict(hk=hk, mismatch=nd))
    if want_k is not None:
        assert hk == want_k
    assert nd == 0
    assert torch.equal(o[:oh, :ow, :3], exp)
    assert float(o[oh:].abs().sum()) == 0.0 and float(o[:, ow:].abs().sum()) == 0.0 and float(o[..., 3].abs().sum()) == 0.0


def test_resize_normalize_limits(logdir):
    """Frames at the documented width bound resize like Pillow (a few rows: no network at that width); sizes past the
    bounds are refused with APSE_E_INVALID before anything is launched."""
    from apse_uav_amd import _lib
    for H, W in ((2, 49152), (3, 49151)):
        hk, nd, o, exp = _resize_case(H, W, 1, 1333, seed=W)
        _log(logdir, "resize_bound/%dx%d" % (H, W), dict(hk=hk, mismatch=nd))
        assert nd == 0 and torch.equal(o[:1, :1333, :3], exp)
    lib = _lib.load()
    mean = (C.c_float * 3)(*MEAN)
    for H, W in ((2, 49153), (0, 16), (16, 0), (32769, 1)):
        rc = lib.apse_resize_normalize(None, None, None, None, None, None, 2, None, None, 2, 1, H, W, 1, 1, 32, 32, C.byref(mean),
                                       _lib.stream_ptr())
        assert rc == -1, (H, W, rc)


# ---------------------------------------------------------------------------------------------------- 2. in-context resize
@pytest.mark.parametrize("hw", [KITTI, (1080, 1918)])
def test_context_resize_equals_pillow(env, hw):
    """apse_preprocess_frames (tap-major coefficient table, dword vertical pass: pil_resize_h8<false> with the unaligned-row
    branch), batch 2 with two different frames: the network input is Pillow's bytes minus the mean, zero padded."""
    from apse_uav_amd.engines.track_predictor import TrackPredictor
    from apse_uav_amd.synthetic import SyntheticSequence
    from apse_uav_amd.utils import resample
    pr = TrackPredictor(_cfg(batch=2), state_dict=env["sd"])
    seq = SyntheticSequence("dynamic", *hw)
    frames = [seq.frame(2), seq.frame(13)]
    pr.model.preprocess_frames(torch.from_numpy(np.stack(frames)).cuda())
    ih, iw = resample.resize_shortest_edge(hw[0], hw[1], 800, 1333)
    ph, pw = (ih + 31) // 32 * 32, (iw + 31) // 32 * 32
    got = pr.model.debug_tensor("input").cpu()[:2 * ph * pw * 4].view(2, ph, pw, 4)
    mean = torch.tensor(list(pr.cfg.MODEL.PIXEL_MEAN), dtype=torch.float32)
    for b, f in enumerate(frames):
        ref = torch.from_numpy(_pillow(f, ih, iw).astype(np.float32)) - mean
        assert torch.equal(got[b, :ih, :iw, :3], ref), b
        assert float(got[b, ih:].abs().sum()) == 0.0 and float(got[b, :, iw:].abs().sum()) == 0.0 and float(got[b, ..., 3].abs().sum()) == 0.0


# ---------------------------------------------------------------------------------------------------- 3. one frame vs the oracle
def test_kitti_frame_vs_oracle(env, logdir):
    from apse_uav_amd.engines.rcnn_tracker import RcnnTracker
    from apse_uav_amd.synthetic import SyntheticSequence
    from oracle import mask_utils as omu
    tr = RcnnTracker(_cfg(), KITTI, env["asd"], detector_state=env["sd"])
    frame = SyntheticSequence("dynamic", *KITTI).frame(0)
    objs = tr.next_frame(frame)
    model = tr.predictor.model
    post = _oracle_frame(env, frame, KITTI)
    rec = tr._last_record
    # ---- proposals: same count, same rows.  Coordinates reach 1333 in the 402 x 1333 input (448 in test_gpu_detector.py):
    # the same 2 f32 ulps there are 2.4e-4 px
    P = int(model.last_results.prop_count[0])
    props = model.debug_tensor("proposals").cpu().view(-1, 4)[:P]
    ref_props = post["proposals"]["boxes"]
    assert P == ref_props.shape[0]
    dprop = float((props - ref_props).abs().max())
    # ---- detections: same list, same classes
    n = len(rec["scores"])
    assert n == post["boxes"].shape[0] and n > 0
    assert np.array_equal(rec["classes"], post["classes"].numpy())
    dbox = float(np.abs(rec["boxes"] - post["boxes"].numpy()).max())
    dscore = float(np.abs(rec["scores"] - post["scores"].numpy()).max())
    de = float((torch.from_numpy(rec["embeddings"]) - post["emb"]).abs().max())
    _log(logdir, "kitti/f32", dict(P=P, n=n, prop_max_abs=dprop, box_max_abs_px=dbox, score_max_abs=dscore, emb_max_abs=de))
    assert dprop < 2.5e-4, dprop              # [observed 1.2e-4 px: 1 ulp at x >= 1024]
    assert dbox < 2.5e-4, dbox                 # [observed 1.8e-4] frame pixels up to 1242: the same 2 ulps at x >= 1024
    assert dscore < 2e-6, dscore
    assert de < 1e-6, de
    # ---- ids: every detection of the first frame is a new object, numbered in detection order like the oracle's
    from oracle import tracker as otr
    orec = otr.TrackerOracle().next_frame(dict(boxes=post["boxes"], scores=post["scores"], classes=post["classes"],
                                              masks=list(zip(post["mask_windows"], post["mask_rects"])), emb=post["emb"]))
    assert (list(objs.ids) if len(objs) else []) == orec["ids"]
    # ---- masks (windows) within the 4K test's pixel tolerance
    pred = model.instances_from(model.last_results, 0)
    bad = 0
    for k in range(n):
        m = pred.pred_masks[k]
        assert tuple(m.rect) == tuple(post["mask_rects"][k])
        bad += int((m.window().cpu() != post["mask_windows"][k]).sum())
        rc = omu.window_centroid(post["mask_windows"][k], post["mask_rects"][k])
        if m.mass and not np.isnan(rc[0]):
            assert abs(m.centroid[0] - rc[0]) <= 1 and abs(m.centroid[1] - rc[1]) <= 1
    assert bad <= 8, bad


def test_kitti_bf16_batch4_vs_bf16_oracle(env, logdir):
    """bf16 matrix cores, batch 4 of four different frames, each against the oracle run with the same quantisation points;
    detections matched as in test_gpu_detector.py::test_bf16_mode_vs_bf16_oracle."""
    from apse_uav_amd.engines.rcnn_tracker import RcnnTracker
    from apse_uav_amd.synthetic import SyntheticSequence
    from hip_helpers import explain_frame
    tr = RcnnTracker(_cfg(batch=4, dtype="bf16"), KITTI, env["asd"], detector_state=env["sd"])
    seq = SyntheticSequence("dynamic", *KITTI)
    frames = [seq.frame(t) for t in (0, 3, 7, 12)]
    out = tr.predictor.predict_batch(frames, want_masks=False)[0]
    tot = 0
    for b in range(4):
        post = _oracle_frame(env, frames[b], KITTI, bf16=True)
        inst = out[b]["instances"]
        n, rn = len(inst), int(post["boxes"].shape[0])
        rep, unexplained = explain_frame(tr.predictor.model, post, b=b)
        _log(logdir, "kitti/bf16/img%d" % b, dict(n=n, ref_n=rn, matched=rep["box"]["matched"], only=rep["box"]["only"],
                                                  unexplained=unexplained, score_max_abs=rep["box"]["matched_score_max_abs"]))
        assert not unexplained, (b, unexplained)
        assert rep["box"]["matched"] >= 1 and rep["box"]["matched"] >= min(n, rn) - len(rep["box"]["only"])
        assert rep["box"]["matched_score_max_abs"] < 5e-3
        tot += n
    assert tot > 0


# ---------------------------------------------------------------------------------------------------- 4. masks, bit planes, closest points
@pytest.mark.parametrize("hw", [KITTI, (721, 1283)])
def test_masks_bits_and_closest_points(env, logdir, hw):
    from apse_uav_amd.engines.rcnn_tracker import RcnnTracker
    from apse_uav_amd.synthetic import SyntheticSequence
    from oracle import mask_utils as omu
    H, W = hw
    tr = RcnnTracker(_cfg(), hw, env["asd"], detector_state=env["sd"])
    frame = SyntheticSequence("dynamic", *hw).frame(5)
    tr.next_frame(frame)
    model = tr.predictor.model
    rec = tr._last_record
    pred = model.instances_from(model.last_results, 0)
    post = _oracle_frame(env, frame, hw)
    n = len(rec["scores"])
    assert n == post["boxes"].shape[0] and n > 0
    dense, bad, edge = [], 0, 0
    for k in range(n):
        m = pred.pred_masks[k]
        x0, y0, x1, y1 = m.rect
        assert 0 <= x0 <= x1 <= W and 0 <= y0 <= y1 <= H
        d = m.dense().cpu().numpy()
        ref = np.zeros((H, W), bool)
        rx0, ry0, rx1, ry1 = post["mask_rects"][k]
        ref[ry0:ry1, rx0:rx1] = np.asarray(post["mask_windows"][k], bool)
        bad += int((d != ref).sum())
        # no bit at x >= W in any row's last word of the window
        if m.bits is not None:
            bits = m.bits.cpu().numpy().view(np.uint64)
            xs = ((x0 >> 6) << 6) + np.arange(bits.shape[1] * 64)
            px = ((bits[:, :, None] >> np.arange(64, dtype=np.uint64)) & np.uint64(1)).reshape(bits.shape[0], -1)
            assert not px[:, xs >= W].any(), k
            edge += int(x1 == W)
        # centroid and mass on the HIP dense mask
        assert m.mass == int(d.sum())
        c = omu.get_mask_centroid(d)
        if m.mass:
            assert (float(rec["centroids"][k][0]), float(rec["centroids"][k][1])) == c, (k, rec["centroids"][k], c)
        dense.append(d)
    # closest pixel of mask i to the centroid of detection j (the CSV's positions), on the HIP dense masks
    checked = 0
    for i in range(n):
        for j in range(n):
            got = tuple(float(v) for v in rec["closest"][i][j])
            cj = rec["centroids"][j]
            if not dense[i].any() or cj[0] < 0:
                assert got == (-1.0, -1.0), (i, j, got)
                continue
            assert got == omu.compute_closest_point(dense[i], (float(cj[0]), float(cj[1]))), (i, j)
            checked += 1
    _log(logdir, "masks/%dx%d" % hw, dict(n=n, mismatched=bad, windows_at_right_edge=edge, closest_checked=checked))
    assert bad <= 8, bad


# ---------------------------------------------------------------------------------------------------- 5. sequence and CSV
def test_kitti_sequence_ids_and_csv(env, logdir):
    from apse_uav_amd.engines.rcnn_tracker import RcnnTracker
    from apse_uav_amd.synthetic import SyntheticSequence
    from oracle import tracker as otr
    tr = RcnnTracker(_cfg(), KITTI, env["asd"], detector_state=env["sd"])
    otk = otr.TrackerOracle()
    seq = SyntheticSequence("dynamic", *KITTI)
    lines, olines, ids = [], [], []
    for t in range(6):
        frame = seq.frame(t)
        rec = tr.next_frame(frame)
        post = _oracle_frame(env, frame, KITTI)
        orec = otk.next_frame(dict(boxes=post["boxes"], scores=post["scores"], classes=post["classes"],
                                   masks=list(zip(post["mask_windows"], post["mask_rects"])), emb=post["emb"]))
        got_ids = list(rec.ids) if len(rec) else []
        ids.append(got_ids)
        assert got_ids == orec["ids"], t
        lines.append(tr.log_line(rec, 1, t)[0])
        olines.append(otr.log_oneline(orec, 1, t)[0])
    _log(logdir, "kitti/seq", dict(ids=ids, sample=lines[-1][:160]))
    assert lines == olines


def _pipelined_equals_sequential(env, hw, nframes):
    from apse_uav_amd.engines.pipelined_tracker import PipelinedRcnnTracker
    from apse_uav_amd.engines.rcnn_tracker import RcnnTracker
    from apse_uav_amd.synthetic import SyntheticSequence
    seq = SyntheticSequence("dynamic", *hw)
    frames = [seq.frame(t) for t in range(nframes)]
    ref_tr = RcnnTracker(_cfg(), hw, env["asd"], detector_state=env["sd"])
    ref = []
    for t, f in enumerate(frames):
        rec = ref_tr.next_frame(f)
        ref.append((list(rec.ids) if len(rec) else [], ref_tr.log_line(rec, 1, t)[0], [m.dense().cpu().numpy() for m in rec.pred_masks]))
    drv = PipelinedRcnnTracker(_cfg(), hw, env["asd"], depth=2, want_masks=True, detector_state=env["sd"])
    n = 0
    for (t, rec), (ids, line, masks) in zip(drv.run(frames), ref):
        assert t == n
        n += 1
        assert (list(rec.ids) if len(rec) else []) == ids
        assert drv.tracker.log_line(rec, 1, t)[0] == line
        for a, b in zip(rec.pred_masks, masks):
            assert np.array_equal(a.dense().cpu().numpy(), b)
    assert n == len(frames)


def test_kitti_pipelined_equals_sequential(env):
    _pipelined_equals_sequential(env, KITTI, 4)


# ---------------------------------------------------------------------------------------------------- 6. MOTS
def test_kitti_mots_lines(env, logdir):
    """utils/mots_evaluation.file_lines_from_instances on the tracker's ObjectInstances == oracle/mots.file_lines on the same
    dense masks.  The MOTS writer keeps classes 0 and 2 only and the synthetic detector predicts class 1, so both sides are
    given the same relabelled classes; what is checked is the masks of a 1242-wide frame through the RLE."""
    from apse_uav_amd.engines.rcnn_tracker import RcnnTracker
    from apse_uav_amd.synthetic import SyntheticSequence
    from apse_uav_amd.utils import mots_evaluation, rle
    from oracle import mots as omots
    tr = RcnnTracker(_cfg(), KITTI, env["asd"], detector_state=env["sd"])
    objs = tr.next_frame(SyntheticSequence("dynamic", *KITTI).frame(1))
    n = len(objs)
    assert n > 0
    objs.pred_classes = torch.tensor([(0, 2)[k % 2] for k in range(n)], dtype=torch.int64)
    dense = [m.dense().cpu().numpy() for m in objs.pred_masks]
    got = mots_evaluation.file_lines_from_instances(objs, 3, KITTI)
    want = omots.file_lines(dict(ids=list(objs.ids), classes=[int(c) for c in objs.pred_classes], masks=dense), 3, KITTI)
    _log(logdir, "kitti/mots", dict(lines=got.count("\n"), sample=got.split("\n")[0][:120]))
    assert got == want and got.count("\n") == n
    for line, d in zip(got.strip().split("\n"), dense):
        f = line.split(" ")
        assert (int(f[3]), int(f[4])) == KITTI
        back = rle.decode({"size": [int(f[3]), int(f[4])], "counts": f[5].encode("ascii")})
        assert np.array_equal(back.astype(bool), d)


# ---------------------------------------------------------------------------------------------------- 7. fused undistort + gamma
def test_fused_preproc_721x1283_batch2(env, golden_dir):
    """undistort + gamma fused into the resize staging at 721 x 1283 (W % 4 = 3), batch 2: the network input equals the
    two-kernel form (apse_undistort_gamma, then the resize with the unaligned-row branch) and oracle/preproc + Pillow."""
    from apse_uav_amd.engines.track_predictor import TrackPredictor
    from apse_uav_amd.synthetic import SyntheticSequence
    from apse_uav_amd.utils import resample
    from oracle import preproc as op
    hw = (721, 1283)
    with open(os.path.join(golden_dir, "cam_params.json")) as f:
        cam = json.load(f)
    s = hw[1] / 3840.0
    mtx = np.asarray(cam["mtx"], np.float64)
    mtx[0] *= s
    mtx[1] *= s
    cam_s = dict(mtx=mtx.tolist(), dist=cam["dist"])
    seq = SyntheticSequence("dynamic", *hw)
    frames = [seq.frame(4), seq.frame(11)]
    got = []
    for fused in (True, False):
        pr = TrackPredictor(_cfg(batch=2), state_dict=env["sd"])
        pr.set_camera(cam_s, fused=fused)
        assert (pr.frame_preprocessor is None) == fused
        pr.model.preprocess_frames(pr._upload(frames))
        got.append(pr.model.debug_tensor("input").cpu())
    assert torch.equal(got[0], got[1])
    ih, iw = resample.resize_shortest_edge(hw[0], hw[1], 800, 1333)
    ph, pw = (ih + 31) // 32 * 32, (iw + 31) // 32 * 32
    x = got[0][:2 * ph * pw * 4].view(2, ph, pw, 4)
    mean = torch.tensor(MEAN, dtype=torch.float32)
    for b, f in enumerate(frames):
        pre = op.preprocess_img(f, cam_s["mtx"], cam_s["dist"])
        ref = torch.from_numpy(_pillow(pre, ih, iw).astype(np.float32)) - mean
        assert torch.equal(x[b, :ih, :iw, :3], ref), b


# ---------------------------------------------------------------------------------------------------- 8. limits
def test_create_limits():
    from apse_uav_amd import _lib
    from apse_uav_amd.utils import resample
    lib = _lib.load()

    def create(h, w):
        cfg = _lib.Config()
        cfg.struct_size = C.sizeof(_lib.Config)
        cfg.max_batch, cfg.frame_h, cfg.frame_w, cfg.num_classes, cfg.dets_per_image = 1, h, w, 4, 100
        cfg.image_h, cfg.image_w = resample.resize_shortest_edge(h, w, 800, 1333) if h > 0 and w > 0 else (800, 1333)
        cfg.rpn_pre_topk = cfg.rpn_post_topk = 1000
        cfg.assoc_roi, cfg.embed_dim = 10, 128
        ctx = C.c_void_p()
        rc = lib.apse_create(C.byref(cfg), C.byref(ctx))
        if ctx.value:
            lib.apse_destroy(ctx)
        return rc
    for hw in SIZES + [(2, 49152), (32768, 16)]:
        assert create(*hw) == 0, hw
    for hw in [(375, 0), (0, 1242), (-1, 1242), (375, -2), (375, 49153), (32769, 1242)]:
        assert create(*hw) == -1, hw


# ---------------------------------------------------------------------------------------------------- 9. frames above 4096 px
# Wider or taller than 4096 px: the closest points take the every-pixel kernel (csrc/mask_tail.hip closest_points<false>; the
# word search's exactness argument needs both bounds).  20 MP stills (5472 x 3648 -> 800 x 1200) and a portrait frame
# (2592 x 4608 -> 1333 x 750), detected path, against the oracle with the bars of the KITTI case (the mask-pixel bar
# scaled by the upscale, below).
LARGE = [(3648, 5472), (4608, 2592)]


@pytest.mark.parametrize("hw", LARGE, ids=["%dx%d" % hw for hw in LARGE])
def test_large_frame_vs_oracle(env, logdir, hw):
    from apse_uav_amd.engines.rcnn_tracker import RcnnTracker
    from apse_uav_amd.synthetic import SyntheticSequence
    from oracle import mask_utils as omu
    H, W = hw
    tr = RcnnTracker(_cfg(), hw, env["asd"], detector_state=env["sd"])
    frame = SyntheticSequence("dynamic", *hw).frame(2)
    tr.next_frame(frame)
    model = tr.predictor.model
    rec = tr._last_record
    post = _oracle_frame(env, frame, hw)
    # ---- detections: same list, same classes; boxes within 2 f32 ulps of the frame's largest coordinate (the KITTI bar,
    # 2.5e-4 at 1242, is the same 2 ulps at x >= 1024)
    n = len(rec["scores"])
    assert n == post["boxes"].shape[0] and n > 0
    assert np.array_equal(rec["classes"], post["classes"].numpy())
    dbox = float(np.abs(rec["boxes"] - post["boxes"].numpy()).max())
    bar = 2 * float(np.spacing(np.float32(max(H, W))))
    dscore = float(np.abs(rec["scores"] - post["scores"].numpy()).max())
    # ---- masks: windows within the 4K pixel bar, no bit at x >= W, mass / centroid / every closest point == oracle/mask_utils on
    # the HIP dense masks
    # The 4K tests' bar is 8 pixels at an upscale of 8.3 frame pixels per network-input pixel (3840 x 2160 from 1333 x 750); a
    # mask logit that moves a threshold crossing moves it by the upscale, so the bar here is the same 8 pixels per 8.3 of
    # this frame's upscale: 21 at 5472 x 3648 (800 x 1200 input), 12 at 2592 x 4608 (750 x 1333).
    from apse_uav_amd.utils import resample
    ih, iw = resample.resize_shortest_edge(H, W, 800, 1333)
    bar_px = max(8, int(np.ceil(8 * (H * W) / (ih * iw) / (2160 * 3840 / (750 * 1333)))))
    pred = model.instances_from(model.last_results, 0)
    dense, bad, edge = [], 0, 0
    for k in range(n):
        m = pred.pred_masks[k]
        assert tuple(m.rect) == tuple(post["mask_rects"][k])
        x0, y0, x1, y1 = m.rect
        bad += int((m.window().cpu() != post["mask_windows"][k]).sum())
        if m.bits is not None:
            bits = m.bits.cpu().numpy().view(np.uint64)
            xs = ((x0 >> 6) << 6) + np.arange(bits.shape[1] * 64)
            px = ((bits[:, :, None] >> np.arange(64, dtype=np.uint64)) & np.uint64(1)).reshape(bits.shape[0], -1)
            assert not px[:, xs >= W].any(), k
            edge += int(x1 == W)
        d = m.dense().cpu().numpy()
        assert m.mass == int(d.sum())
        if m.mass:
            assert (float(rec["centroids"][k][0]), float(rec["centroids"][k][1])) == omu.get_mask_centroid(d), k
        else:
            assert tuple(rec["centroids"][k]) == (-1, -1)
        dense.append(d)
    checked = 0
    for i in range(n):
        for j in range(n):
            got = tuple(float(v) for v in rec["closest"][i][j])
            cj = rec["centroids"][j]
            if not dense[i].any() or cj[0] < 0:
                assert got == (-1.0, -1.0), (i, j, got)
                continue
            assert got == omu.compute_closest_point(dense[i], (float(cj[0]), float(cj[1]))), (i, j)
            checked += 1
    _log(logdir, "large/%dx%d" % hw, dict(n=n, box_max_abs_px=dbox, box_bar=bar, score_max_abs=dscore, mismatched=bad, mismatch_bar=bar_px,
                                           windows_at_right_edge=edge, closest_checked=checked))
    assert dbox < bar, (dbox, bar)
    assert dscore < 2e-6, dscore
    assert bad <= bar_px, (bad, bar_px)
    assert checked > 0


def test_large_frame_pipelined_equals_sequential(env):
    _pipelined_equals_sequential(env, (4608, 2592), 3)
