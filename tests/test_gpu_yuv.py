"""-m gpu: NV12 / I420 frames.  The stand-alone converter (apse_yuv_to_bgr) against the numpy oracle (tests/yuv_ref.py), the
conversion fused into the resize's row staging against the BGR path on the oracle-converted frame, the camera path, and the
engines end to end.  Every comparison is byte for byte: the conversion is integer arithmetic.

Shapes: the smallest at which the addressing can go wrong (1 x 1 .. 17 x 33: odd sizes, a last column / row without a partner,
widths below and above the four pixels a thread converts), KITTI's 375 x 1242, pitches that leave rows at every byte
alignment, and the 4096 x 4096 frame whose 2 x 2 blocks enumerate all 2^24 (Y, U, V) triples.
"""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import yuv_ref

pytestmark = pytest.mark.gpu

BLOCKS = (1, 1, 1, 1)
FRAME = (270, 480)
MEAN = (103.530, 116.280, 123.675)
FMT = {"NV12": 0, "I420": 1}
GUARD = 64


def _cfg(fmt="BGR", batch=1, dtype="f32", matrix="cv601", arch=None):
    from apse_uav_amd.config import setup_cfg
    cfg = setup_cfg(score_thresh=0.05, num_classes=4, arch="C4") if arch else setup_cfg()
    cfg.INPUT.MIN_SIZE_TEST, cfg.INPUT.MAX_SIZE_TEST = 256, 448
    cfg.INPUT.FORMAT = fmt
    cfg.APSE.MAX_BATCH = batch
    cfg.APSE.DTYPE = dtype
    cfg.APSE.YUV_MATRIX = matrix
    return cfg


def _frame_bytes(H, W, pitch, fmt):
    CH, CW = (H + 1) // 2, (W + 1) // 2
    return (H + CH) * pitch if fmt == "NV12" else H * W + 2 * CH * CW


def _random_frames(B, H, W, pitch, fmt, seed):
    """B frames of random bytes, padding included: (B, rows, pitch) uint8."""
    rows = _frame_bytes(H, W, pitch, fmt) // pitch
    return np.random.default_rng(seed).integers(0, 256, (B, rows, pitch), dtype=np.uint8)


def _convert(data, H, W, fmt, matrix, offset=0):
    """apse_yuv_to_bgr on ``data`` (B, rows, pitch) placed ``offset`` bytes into an allocation that ends with the batch's last
    byte; the destination sits between guard bytes.  Returns the BGR frames (numpy)."""
    from apse_uav_amd import _lib
    B, rows, pitch = data.shape
    assert data.size == B * _frame_bytes(H, W, pitch, fmt)
    src = torch.empty(offset + data.size, dtype=torch.uint8, device="cuda")
    src[offset:] = torch.from_numpy(data.reshape(-1)).cuda()
    n = B * H * W * 3
    dst = torch.full((GUARD + n + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    rc = _lib.load().apse_yuv_to_bgr(C.c_void_p(src.data_ptr() + offset), C.c_void_p(dst.data_ptr() + GUARD), B, H, W, pitch,
                                     FMT[fmt], yuv_ref.ORDER.index(matrix), _lib.stream_ptr())
    assert rc == 0, _lib.load().apse_last_error(None)
    torch.cuda.synchronize()
    out = dst.cpu().numpy()
    assert (out[:GUARD] == 0xA5).all() and (out[GUARD + n:] == 0xA5).all(), "guard bytes around the destination changed"
    return out[GUARD:GUARD + n].reshape(B, H, W, 3)


def _oracle(data, H, W, fmt, matrix):
    return np.stack([yuv_ref.yuv_to_bgr(d, H, W, fmt, matrix) for d in data])


# ---------------------------------------------------------------------------------------------------- 1. stand-alone operator
@pytest.fixture(scope="module")
def all_triples():
    """A 4096 x 4096 NV12 frame whose 2 x 2 blocks enumerate every (Y, U, V): block k = by * 2048 + bx has (U, V) = k >> 6 and
    the four luma values 4 (k & 63) + (2 dy + dx)."""
    k = np.arange(2048 * 2048, dtype=np.int64).reshape(2048, 2048)
    uv = k >> 6
    Y = np.empty((4096, 4096), np.uint8)
    for dy in range(2):
        for dx in range(2):
            Y[dy::2, dx::2] = ((k & 63) * 4 + 2 * dy + dx).astype(np.uint8)
    data = np.empty((6144, 4096), np.uint8)
    data[:4096] = Y
    data[4096:, 0::2] = (uv >> 8).astype(np.uint8)
    data[4096:, 1::2] = (uv & 255).astype(np.uint8)
    trip = (Y.astype(np.int64) << 16) | (np.repeat(np.repeat(uv, 2, 0), 2, 1))
    assert np.unique(trip).size == 1 << 24
    return data


@pytest.mark.parametrize("matrix", ["cv601", "bt709-full"])
def test_every_triple(all_triples, matrix):
    got = torch.from_numpy(_convert(all_triples[None], 4096, 4096, "NV12", matrix)[0]).cuda()
    ref = torch.from_numpy(yuv_ref.yuv_to_bgr(all_triples, 4096, 4096, "NV12", matrix)).cuda()
    assert int((got != ref).sum()) == 0


@pytest.mark.parametrize("matrix", ["bt601", "bt709", "bt601-full"])
def test_random_frame_other_matrices(matrix):
    data = _random_frames(1, 256, 256, 256, "NV12", 7)
    assert np.array_equal(_convert(data, 256, 256, "NV12", matrix), _oracle(data, 256, 256, "NV12", matrix))


SHAPES = [(1, 1), (2, 2), (3, 5), (5, 3), (17, 33), (375, 1242)]


def _pitches(W):
    """W (the smallest legal pitch: an odd width needs W + 1 for its last chroma pair), W + 1, W + 13 and 256-aligned."""
    lo = max(W, 2 * ((W + 1) // 2))
    return sorted({lo, W + 1, W + 13, (W + 255) // 256 * 256})


@pytest.mark.parametrize("hw", SHAPES, ids=["%dx%d" % s for s in SHAPES])
def test_nv12_shapes_and_pitches(hw):
    H, W = hw
    for pitch in _pitches(W):
        data = _random_frames(1, H, W, pitch, "NV12", H * 131 + W + pitch)
        got = _convert(data, H, W, "NV12", "cv601")
        assert np.array_equal(got, _oracle(data, H, W, "NV12", "cv601")), (hw, pitch)


@pytest.mark.parametrize("offset", [1, 2, 3])
def test_offset_source_pointer(offset):
    """The source starts 1, 2, 3 bytes into its allocation (rows at every alignment, with an even and an odd pitch) and the
    allocation ends with the last chroma byte."""
    for (H, W), pitch in (((17, 33), 34), ((17, 33), 47), ((375, 1242), 1242), ((16, 18), 18)):
        fmt = "I420" if (H, W) == (16, 18) else "NV12"
        data = _random_frames(1, H, W, pitch, fmt, offset * 1000 + pitch)
        assert np.array_equal(_convert(data, H, W, fmt, "bt709", offset), _oracle(data, H, W, fmt, "bt709")), (H, W, pitch)


def test_batch_of_two():
    for (H, W), pitch, fmt in (((17, 33), 47, "NV12"), ((375, 1242), 1280, "NV12"), ((16, 18), 18, "I420")):
        data = _random_frames(2, H, W, pitch, fmt, 99 + W)
        got = _convert(data, H, W, fmt, "cv601")
        assert np.array_equal(got, _oracle(data, H, W, fmt, "cv601")), (H, W, fmt)
        assert not np.array_equal(got[0], got[1])


@pytest.mark.parametrize("hw", [(2, 2), (16, 18), (374, 1242)], ids=["2x2", "16x18", "374x1242"])
def test_i420(hw):
    H, W = hw
    data = _random_frames(1, H, W, W, "I420", H + W)
    assert np.array_equal(_convert(data, H, W, "I420", "cv601"), _oracle(data, H, W, "I420", "cv601"))


def test_python_yuv_to_bgr():
    """utils.preprocess.yuv_to_bgr: host and device YuvFrame, with a pitch."""
    from apse_uav_amd.structures.yuv_frame import YuvFrame
    from apse_uav_amd.utils.preprocess import yuv_to_bgr
    data = _random_frames(1, 53, 95, 101, "NV12", 5)[0]
    ref = yuv_ref.yuv_to_bgr(data, 53, 95, "NV12", "bt709")
    assert np.array_equal(yuv_to_bgr(YuvFrame(data, 95), "bt709").cpu().numpy(), ref)
    assert np.array_equal(yuv_to_bgr(YuvFrame(torch.from_numpy(data).cuda(), 95), "bt709").cpu().numpy(), ref)


# ---------------------------------------------------------------------------------------------------- 2. fused staging
def _resize(frames, H, W, oh, ow, yuv=None):
    """apse_resize_normalize on BGR ``frames`` (B, H, W, 3), or apse_resize_normalize_yuv on ``frames`` (B, rows, pitch) with
    yuv = (fmt, matrix, offset) -> (taps, resized u8 (B, oh, ow, 3), network input (B, ph, pw, 4) f32)."""
    from apse_uav_amd import _lib
    from apse_uav_amd.utils import resample
    B = frames.shape[0]
    hb, hc, hk = resample.precompute_coeffs(W, ow)
    vb, vc, vk = resample.precompute_coeffs(H, oh)
    ph, pw = (oh + 31) // 32 * 32, (ow + 31) // 32 * 32
    tmp = torch.empty((B, H, ow, 3), dtype=torch.uint8, device="cuda")
    out = torch.zeros((B, ph, pw, 4), device="cuda")
    rs = torch.empty((B, oh, ow, 3), dtype=torch.uint8, device="cuda")
    t = [torch.from_numpy(a).cuda() for a in (hb, hc, vb, vc)]
    mean = (C.c_float * 3)(*MEAN)
    lib = _lib.load()
    if yuv is None:
        src = torch.from_numpy(frames).cuda()
        rc = lib.apse_resize_normalize(_lib.ptr(src), _lib.ptr(tmp), _lib.ptr(out), _lib.ptr(rs), _lib.ptr(t[0]), _lib.ptr(t[1]), hk,
                                       _lib.ptr(t[2]), _lib.ptr(t[3]), vk, B, H, W, oh, ow, ph, pw, C.byref(mean), _lib.stream_ptr())
    else:
        fmt, matrix, offset = yuv
        src = torch.empty(offset + frames.size, dtype=torch.uint8, device="cuda")          # ends with the batch's last byte
        src[offset:] = torch.from_numpy(frames.reshape(-1)).cuda()
        rc = lib.apse_resize_normalize_yuv(C.c_void_p(src.data_ptr() + offset), frames.shape[2], FMT[fmt], yuv_ref.ORDER.index(matrix),
                                           _lib.ptr(tmp), _lib.ptr(out), _lib.ptr(rs), _lib.ptr(t[0]), _lib.ptr(t[1]), hk, _lib.ptr(t[2]),
                                           _lib.ptr(t[3]), vk, B, H, W, oh, ow, ph, pw, C.byref(mean), _lib.stream_ptr())
    assert rc == 0, lib.apse_last_error(None)
    torch.cuda.synchronize()
    return hk, rs.cpu(), out.cpu()


STAGING = [
    # (H, W, pitch, fmt, B, offset, (oh, ow), horizontal kernel)
    (270, 480, 480, "NV12", 1, 0, (135, 240), "h8"),        # downscale, 5 taps, aligned rows
    (135, 241, 255, "NV12", 2, 0, (68, 121), "h8"),         # odd W and H, odd pitch, batch 2
    (37, 1283, 1296, "NV12", 2, 3, (5, 129), "h"),          # 21+ taps: the per-sample kernel; offset pointer
    (375, 1242, 1242, "NV12", 1, 0, (402, 1333), "h8"),     # KITTI, upscale (3 taps)
    (375, 1242, 1255, "NV12", 1, 1, (402, 1333), "h8"),     # ... odd pitch, offset pointer
    (54, 98, 98, "I420", 2, 0, (27, 49), "h8"),             # I420, W % 4 = 2
    (40, 1284, 1284, "I420", 1, 2, (5, 129), "h"),
]


@pytest.mark.parametrize("case", STAGING, ids=["%dx%d_p%d_%s_b%d_o%d" % c[:6] for c in STAGING])
def test_fused_staging_equals_bgr_path(case):
    H, W, pitch, fmt, B, offset, (oh, ow), kern = case
    data = _random_frames(B, H, W, pitch, fmt, H + W + pitch)
    bgr = _oracle(data, H, W, fmt, "bt709")
    hk, rs_ref, out_ref = _resize(bgr, H, W, oh, ow)
    assert (hk <= 8) == (kern == "h8"), hk
    _, rs, out = _resize(data, H, W, oh, ow, (fmt, "bt709", offset))
    assert torch.equal(rs, rs_ref)
    assert torch.equal(out, out_ref)


@pytest.fixture(scope="module")
def env():
    from apse_uav_amd.synthetic import SyntheticSequence, bgr_to_nv12
    from apse_uav_amd.weights import synthetic_association_state, synthetic_detector_state
    seq = SyntheticSequence("dynamic", *FRAME)
    bgr = [seq.frame(t) for t in range(4)]
    nv12 = [bgr_to_nv12(f, "cv601", pitch=512) for f in bgr]                 # a padded surface: pitch 512 for 480 pixels
    back = [yuv_ref.yuv_to_bgr(y.data, FRAME[0], FRAME[1], "NV12", "cv601") for y in nv12]
    return dict(sd=synthetic_detector_state(0, BLOCKS), asd=synthetic_association_state(1), nv12=nv12, back=back)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_context_input_equals_bgr_path(env, dtype):
    """apse_preprocess_frames_yuv, batch 2, f32 and bf16 storage of the network input: the bytes of apse_preprocess_frames on the
    oracle-converted frames."""
    from apse_uav_amd.engines.track_predictor import TrackPredictor
    a = TrackPredictor(_cfg("NV12", 2, dtype), state_dict=env["sd"])
    a.model.preprocess_frames(a._upload(env["nv12"][:2]))
    b = TrackPredictor(_cfg("BGR", 2, dtype), state_dict=env["sd"])
    b.model.preprocess_frames(b._upload(env["back"][:2]))
    t = torch.float32 if dtype == "f32" else torch.int16
    ga, gb = a.model.debug_tensor("input", t).cpu(), b.model.debug_tensor("input", t).cpu()
    assert ga.numel() > 0 and int((ga != 0).sum()) > 0
    assert torch.equal(ga, gb)


# ---------------------------------------------------------------------------------------------------- 3. camera
@pytest.mark.parametrize("fused", [True, False], ids=["fused", "unfused"])
def test_camera_path_equals_bgr_path(env, golden_dir, fused):
    """set_camera (undistort + gamma) on NV12 frames = convert, then preprocess_img: the BGR path on the converted frame."""
    from apse_uav_amd.engines.track_predictor import TrackPredictor
    with open(os.path.join(golden_dir, "cam_params.json")) as f:
        cam = json.load(f)
    mtx = np.asarray(cam["mtx"], np.float64)
    mtx[0] *= FRAME[1] / 3840.0
    mtx[1] *= FRAME[1] / 3840.0
    cam_s = dict(mtx=mtx.tolist(), dist=cam["dist"])
    got = []
    for fmt, frames in (("NV12", env["nv12"][:1]), ("BGR", env["back"][:1])):
        pr = TrackPredictor(_cfg(fmt), state_dict=env["sd"])
        pr.set_camera(cam_s, fused=fused)
        pr.model.preprocess_frames(pr._upload(frames))
        got.append(pr.model.debug_tensor("input").cpu())
    plain = TrackPredictor(_cfg("NV12"), state_dict=env["sd"])
    plain.model.preprocess_frames(plain._upload(env["nv12"][:1]))
    assert torch.equal(got[0], got[1])
    assert not torch.equal(got[0], plain.model.debug_tensor("input").cpu())


# ---------------------------------------------------------------------------------------------------- 4. end to end
def _result_bytes(pr, pred):
    """The results block of the last forward and the mask windows of the returned instances."""
    inst = pred["instances"]
    wins = [m.window().cpu().numpy().tobytes() + bytes(str(tuple(m.rect)), "ascii") for m in inst.pred_masks]
    return len(inst), bytes(pr.model.last_results.raw), wins


def test_predictor_nv12_equals_bgr(env):
    from apse_uav_amd.engines.track_predictor import TrackPredictor
    from apse_uav_amd.structures.yuv_frame import YuvFrame
    ref_pr = TrackPredictor(_cfg("BGR"), state_dict=env["sd"])
    ref = _result_bytes(ref_pr, ref_pr(env["back"][0])[0])
    assert ref[0] > 0
    pr = TrackPredictor(_cfg("NV12"), state_dict=env["sd"])
    assert _result_bytes(pr, pr(env["nv12"][0])[0]) == ref                   # a host YuvFrame
    y = env["nv12"][0]
    surface = YuvFrame(torch.from_numpy(y.data).cuda(), y.width, "NV12")     # a decoder surface on the device, read in place
    assert _result_bytes(pr, pr(surface)[0]) == ref
    assert _result_bytes(pr, pr(np.ascontiguousarray(y.data[:, :480]))[0]) == ref          # a bare 2-D array: width = pitch (480)


def test_predictor_history(env):
    """BGR, NV12, BGR on ONE model: the scratch and the slot reshaping leave nothing behind."""
    from apse_uav_amd.engines.track_predictor import TrackPredictor
    from apse_uav_amd.structures.yuv_frame import YuvBatch
    pr = TrackPredictor(_cfg("BGR"), state_dict=env["sd"])
    first = _result_bytes(pr, pr(env["back"][1])[0])
    y = env["nv12"][0]
    m = pr.model
    B = m.preprocess_frames(YuvBatch(torch.from_numpy(y.data).cuda()[None], y.height, y.width, y.pitch, "NV12"))
    m.run(B)
    assert m.read(B).total >= 0
    again = _result_bytes(pr, pr(env["back"][1])[0])
    assert first[0] > 0 and again == first


def test_tracker_sequence_nv12_equals_bgr(env):
    """RcnnTracker.next_frame(frame, upcoming=next) over 4 frames: same ids, same CSV lines, same masks as the BGR tracker on the
    converted frames."""
    from apse_uav_amd.engines.rcnn_tracker import RcnnTracker

    def run(fmt, frames):
        tr = RcnnTracker(_cfg(fmt), FRAME, env["asd"], detector_state=env["sd"])
        out = []
        for t, f in enumerate(frames):
            rec = tr.next_frame(f, upcoming=frames[t + 1] if t + 1 < len(frames) else None)
            out.append((list(rec.ids) if len(rec) else [], tr.log_line(rec, 1, t)[0],
                        [m.dense().cpu().numpy().tobytes() for m in rec.pred_masks]))
        return out
    from apse_uav_amd.structures.yuv_frame import YuvFrame
    ref = run("BGR", env["back"])
    assert sum(len(r[0]) for r in ref) > 0
    assert run("NV12", env["nv12"]) == ref
    surfaces = [YuvFrame(torch.from_numpy(y.data).cuda(), y.width, "NV12") for y in env["nv12"]]
    assert run("NV12", surfaces) == ref                                      # announced device frames are pre-staged in place


def test_pipelined_tracker_nv12(env):
    from apse_uav_amd.engines.pipelined_tracker import PipelinedRcnnTracker

    def run(fmt, frames):
        drv = PipelinedRcnnTracker(_cfg(fmt), FRAME, env["asd"], depth=2, want_masks=True, detector_state=env["sd"])
        return [(t, list(r.ids) if len(r) else [], drv.tracker.log_line(r, 1, t)[0]) for t, r in drv.run(frames)]
    assert run("NV12", env["nv12"]) == run("BGR", env["back"])


def test_c4_nv12_equals_bgr(env):
    """The same under arch = C4 (Res5ROIHeads)."""
    from apse_uav_amd.engines.track_predictor import TrackPredictor
    from apse_uav_amd.weights import synthetic_c4_state
    sd = synthetic_c4_state(0, BLOCKS, num_classes=4, cls_gain=2.0)
    out = []
    for fmt, frame in (("NV12", env["nv12"][0]), ("BGR", env["back"][0])):
        pr = TrackPredictor(_cfg(fmt, arch="C4"), state_dict=sd)
        pred = pr(frame)[0]
        out.append((pr.model.debug_tensor("input").cpu(), _result_bytes(pr, pred)))
    assert torch.equal(out[0][0], out[1][0])
    assert out[0][1] == out[1][1]


# ---------------------------------------------------------------------------------------------------- 5. the other consumers
def test_selective_predictor_and_roi_features(env):
    from apse_uav_amd.engines.roi_features_generator import RoiFeaturesGenerator
    from apse_uav_amd.engines.selective_predictor import SelectivePredictor
    out = []
    for fmt, frame in (("NV12", env["nv12"][0]), ("BGR", env["back"][0])):
        pr = SelectivePredictor(_cfg(fmt), state_dict=env["sd"])
        inst = pr(frame)["instances"]
        out.append((len(inst), bytes(pr.model.last_results.raw)))
    assert out[0] == out[1]
    objects = [[0, 1, 40, 30, 120, 60, 1], [0, 2, 301, 155, 77, 93, 1]]
    feats = []
    for fmt, frame in (("NV12", env["nv12"][0]), ("BGR", env["back"][0])):
        gen = RoiFeaturesGenerator(_cfg(fmt), roi_size=8, state_dict=env["sd"])
        ids, rois = gen.get_rois_features(frame, objects)
        feats.append(rois.cpu())
    assert float(feats[0].abs().sum()) > 0 and torch.equal(feats[0], feats[1])


def test_visualizer_draws_on_yuv_frame(env):
    """visualize_tracks / draw_instance_predictions on a YuvFrame = on its conversion."""
    from apse_uav_amd.engines.rcnn_tracker import RcnnTracker
    from apse_uav_amd.utils.track_visualizer import TrackVisualizer, visualize_tracks
    tr = RcnnTracker(_cfg("NV12"), FRAME, env["asd"], detector_state=env["sd"])
    objs = tr.next_frame(env["nv12"][0])
    assert len(objs) > 0
    vis = TrackVisualizer({"thing_classes": ["car", "truck", "bus", "van"]})
    a = visualize_tracks(env["nv12"][0], objs, vis)
    b = visualize_tracks(env["back"][0], objs, vis)
    assert a.shape == FRAME + (3,) and np.array_equal(a, b)
    assert not np.array_equal(a, env["back"][0])
