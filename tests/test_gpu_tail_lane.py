"""-m gpu: the tail lane against the same library with the lane switched off, byte for byte.

With the lane the proposal selection, heads and results copy of a forward that RUNS AHEAD (one enqueued between the two halves
of a read, as the announced loop does) go to a second stream of the context while the caller's stream already carries the
next frame's trunk; two event edges order them (fork behind the RPN convolutions, join in front of
the next trunk's first FPN step).  Every test runs one call sequence on a default context and on a twin created under
APSE_TAIL_LANE=0 and compares results blocks, mask windows and debug tensors.  The shapes are the smallest at which the
ordering can go wrong: with BLOCKS = (1, 1, 1, 1) at the 256 / 448 test size and 1000 proposals the lane is still busy when
the next trunk reaches its first FPN step, so the wait really binds (the third counter of apse_lane_stats, asserted below;
tools/lane_probe.py prints it next to both durations) -- at 4K it is long satisfied.  The "dynamic" sequence
moves, so a frame computed from its neighbour's maps cannot pass.
"""
import ctypes as C
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
BLOCKS = (1, 1, 1, 1)
SMALL, WIDE = (270, 480), (375, 1242)
NCFG = 14


@pytest.fixture(scope="module")
def env():
    from apse_uav_amd.networks.association_head import AssociationHead
    from apse_uav_amd.synthetic import SyntheticSequence
    from apse_uav_amd.weights import synthetic_association_state, synthetic_detector_state
    head = AssociationHead(roi_size=10, input_depth=256)
    head.load_state_dict(synthetic_association_state(1))
    frames = {}
    for hw in (SMALL, WIDE):
        seq = SyntheticSequence("dynamic", *hw)
        frames[hw] = torch.stack([torch.from_numpy(seq.frame(5 * t)) for t in range(10)]).cuda()
        assert len({frames[hw][t].cpu().numpy().tobytes() for t in range(10)}) == 10          # consecutive frames differ
    return dict(sd=synthetic_detector_state(0, BLOCKS), head=head, frames=frames)


def _model(env, hw, lane, dtype="f32", batch=1):
    """A TrackRCNN whose context exists (it is created by the first preprocess_frames): default, or under APSE_TAIL_LANE=0."""
    from apse_uav_amd.config import setup_cfg
    from apse_uav_amd.networks.track_rcnn import TrackRCNN
    cfg = setup_cfg()
    cfg.INPUT.MIN_SIZE_TEST, cfg.INPUT.MAX_SIZE_TEST = 256, 448
    cfg.APSE.MAX_BATCH, cfg.APSE.DTYPE = batch, dtype
    m = TrackRCNN(cfg)
    m.to("cuda")
    m.load_state_dict(env["sd"])
    m.attach_association_head(env["head"])
    old = os.environ.pop("APSE_TAIL_LANE", None)
    if not lane:
        os.environ["APSE_TAIL_LANE"] = "0"            # read once, when the context is created
    try:
        m.preprocess_frames(env["frames"][hw][0:batch])
    finally:
        os.environ.pop("APSE_TAIL_LANE", None)
        if old is not None:
            os.environ["APSE_TAIL_LANE"] = old
    return m


def _windows(m, res, batch):
    """Bytes of every detection's mask window, copied out of the bit planes (apse_copy_mask_windows) on the current stream."""
    out = b""
    for b in range(batch):
        inst = m.instances_from(res, b)
        for k in range(len(inst)):
            mk = inst.pred_masks[k]
            out += repr(tuple(mk.rect)).encode() + (mk.bits.cpu().numpy().tobytes() if mk.bits is not None else b"-")
    return out


def _announced(m, fr, batch, n):
    """bench.py's call order: run, then per frame read_begin, the NEXT frame's preprocess_frames and run, read_end -- and the mask
    windows of the frame just read, copied with the next forward already enqueued."""
    out = []
    m.preprocess_frames(fr[0:batch])
    m.run(batch)
    for j in range(n):
        m.read_begin(batch)
        if j + 1 < n:
            m.preprocess_frames(fr[j + 1:j + 1 + batch])
            m.run(batch)
        res = m.read_end(batch)
        out.append((res.raw, _windows(m, res, batch)))
    torch.cuda.synchronize()
    return out


def _ahead(m, frames, batch=1, given=None):
    """A forward enqueued between the two halves of a read (of whatever the context computed last), as the announced loop
    enqueues every forward but its first: its tail goes to the lane."""
    m.read_begin(batch)
    m.preprocess_frames(frames)
    m.run(batch, given)
    m.read_end(batch)


def _plain(m, fr, batch, n):
    out = []
    for j in range(n):
        m.preprocess_frames(fr[j:j + batch])
        m.run(batch)
        res = m.read(batch)
        out.append((res.raw, _windows(m, res, batch)))
    return out


def _same(got, ref):
    assert [g[0] == r[0] for g, r in zip(got, ref)] == [True] * len(ref), "results blocks differ"
    assert [g[1] == r[1] for g, r in zip(got, ref)] == [True] * len(ref), "mask windows differ"
    assert len({r[0] for r in ref}) == len(ref)               # the frames really differ ...
    assert any(r[1] for r in ref)                             # ... and carry masks


@pytest.fixture(scope="module")
def announced_ref(env):
    """The lane-off twin's announced loop, once per (shape, dtype, batch); shared, never modified."""
    cache = {}

    def get(hw, dtype, batch):
        key = (hw, dtype, batch)
        if key not in cache:
            m = _model(env, hw, False, dtype, batch)
            cache[key] = _announced(m, env["frames"][hw], batch, 8)
            assert m.lane_stats() == (0, 0, 0, 0)
        return cache[key]
    return get


@pytest.mark.parametrize("own_stream", [False, True], ids=["legacy-stream", "torch-stream"])
@pytest.mark.parametrize("hw,dtype,batch", [(SMALL, "f32", 1), (WIDE, "f32", 1), (SMALL, "f32", 2), (SMALL, "bf16", 2)],
                         ids=["270x480-f32-b1", "375x1242-f32-b1", "270x480-f32-b2", "270x480-bf16-b2"])
def test_announced_loop(env, announced_ref, hw, dtype, batch, own_stream):
    ref = announced_ref(hw, dtype, batch)
    m = _model(env, hw, True, dtype, batch)
    torch.cuda.synchronize()
    if own_stream:
        with torch.cuda.stream(torch.cuda.Stream()):
            got = _announced(m, env["frames"][hw], batch, 8)
    else:
        got = _announced(m, env["frames"][hw], batch, 8)
    _same(got, ref)
    fwd, joins, fpn_waits, drains = m.lane_stats()
    print("lane stats %s %s b%d: forwards %d joins %d fpn waits not ready %d drains %d" % (hw, dtype, batch, fwd, joins, fpn_waits, drains))
    assert fwd == 7                                           # every forward enqueued ahead of a read ran its tail on the lane
    # (whether the FPN wait binds in THIS loop depends on how long the host spends copying mask windows between two forwards:
    # test_back_to_back_forwards_find_the_lane_busy asserts it, at both shapes, where nothing is copied in between)


def _back_to_back(env, m, hw):
    """Three forwards enqueued ahead of reads with nothing copied out in between, then everything of the last one."""
    fr = env["frames"][hw]
    for j in range(3):
        _ahead(m, fr[j:j + 1])
    res = m.read(1)
    return [(res.raw, _windows(m, res, 1))]


@pytest.mark.parametrize("hw", [SMALL, WIDE], ids=["270x480", "375x1242"])
def test_back_to_back_forwards_find_the_lane_busy(env, hw):
    """The edge these shapes were chosen for, at both of them: a trunk's first FPN step is enqueued microseconds after the
    previous forward's tail (0.8 ms of kernels behind a 0.5 ms trunk), so its wait must find the lane busy -- and hold."""
    ref = _back_to_back(env, _model(env, hw, False), hw)
    m = _model(env, hw, True)
    got = _back_to_back(env, m, hw)
    assert got[0][0] == ref[0][0] and got[0][1] == ref[0][1] and ref[0][1]
    fwd, _, fpn_waits, _ = m.lane_stats()
    assert fwd == 3 and fpn_waits > 0


def test_plain_loop(env):
    for hw in (SMALL, WIDE):
        ref = _plain(_model(env, hw, False), env["frames"][hw], 1, 4)
        m = _model(env, hw, True)
        _same(_plain(m, env["frames"][hw], 1, 4), ref)
        assert m.lane_stats() == (0, 0, 0, 0)                 # nothing runs ahead: the lane is never used


def _interleavings(env, m):
    """Entries that read lane-owned buffers or the FPN maps on the caller's stream, right behind or between forwards whose tail is
    on the lane."""
    from apse_uav_amd import _lib
    lib = _lib.load()
    fr = env["frames"][SMALL]
    s = _lib.stream_ptr()
    out = []
    # debug_tensor / export_feature directly after run
    _ahead(m, fr[0:1])
    for name in ("proposals", "det_boxes", "box_pooled", "mask_logits", "embedding_raw"):
        out.append(m.debug_tensor(name).cpu().numpy().tobytes())
    out.append(m.export_feature("p2", 1).cpu().numpy().tobytes())
    out.append(m.read(1).raw)
    # a given-boxes forward behind a detecting one, and the reverse, nothing read in between
    given = (np.array([[40.0, 30.0, 120.0, 90.0], [200.5, 100.25, 260.0, 180.75]], np.float32), np.array([0, 2], np.int32),
             np.array([2], np.int32))
    _ahead(m, fr[1:2])
    _ahead(m, fr[2:3], given=given)
    res = m.read(1)
    out += [res.raw, _windows(m, res, 1)]
    _ahead(m, fr[3:4], given=given)
    _ahead(m, fr[4:5])
    res = m.read(1)
    out += [res.raw, _windows(m, res, 1)]
    # apse_mask_tail twice on one detection list
    for _ in range(2):
        _lib.check(lib.apse_mask_tail(m._ctx, 1, s), m._ctx, "apse_mask_tail")
    _lib.check(lib.apse_embed(m._ctx, 1, s), m._ctx, "apse_embed")
    res = m.read(1)
    out += [res.raw, _windows(m, res, 1)]
    # roi_features / mask_roi_features between two forwards (they read the maps of the forward in front of them)
    _ahead(m, fr[5:6])
    rois = torch.tensor([[30.0, 20.0, 200.0, 150.0], [100.0, 50.0, 400.0, 260.0]], device="cuda")
    feat = torch.empty((2, 256, 10, 10), dtype=torch.float32, device="cuda")
    _lib.check(lib.apse_roi_features(m._ctx, 0, _lib.ptr(rois), None, 2, 10, _lib.ptr(feat), s), m._ctx, "apse_roi_features")
    mf = m.mask_roi_features(rois.cpu().numpy() * 0.9)
    _ahead(m, fr[6:7])
    out += [feat.cpu().numpy().tobytes(), mf.cpu().numpy().tobytes(), m.read(1).raw]
    return out


def test_interleavings(env):
    ref = _interleavings(env, _model(env, SMALL, False))
    m = _model(env, SMALL, True)
    got = _interleavings(env, m)
    assert [g == r for g, r in zip(got, ref)] == [True] * len(ref) and len(got) == len(ref)
    assert m.lane_stats()[0] == 7                             # one per forward: the repeated mask tails start none
    # forwards enqueued back to back with nothing read in between: the second trunk's first FPN step is enqueued microseconds
    # after the first forward's tail (0.8 ms of kernels behind a 0.5 ms trunk), so its wait must have found the lane busy
    assert m.lane_stats()[2] > 0


def _profiled(m, fr):
    from apse_uav_amd import _lib
    lib = _lib.load()
    m.preprocess_frames(fr[0:1]); m.run(1)
    _ahead(m, fr[5:6])                                        # runs ahead: on the lane
    first = m.read(1).raw
    before = m.lane_stats()[0]
    lib.apse_profile(m._ctx, 1)
    raws = []
    for j in range(1, 4):
        _ahead(m, fr[j:j + 1])                                # runs ahead, but profiling is on
        raws.append(m.read(1).raw)
    during = m.lane_stats()[0]
    pr = (C.c_double * (3 * NCFG))()
    lib.apse_profile_read(m._ctx, C.byref(pr), 1)
    lib.apse_profile(m._ctx, 0)
    _ahead(m, fr[4:5])
    raws.append(m.read(1).raw)
    return first, raws, np.array(list(pr)).reshape(NCFG, 3)[:, 2], before, during, m.lane_stats()[0]


def test_profiling_switches_the_lane_off(env):
    fr = env["frames"][SMALL]
    f0, r0, cnt0, *_ = _profiled(_model(env, SMALL, False), fr)
    f1, r1, cnt1, before, during, after = _profiled(_model(env, SMALL, True), fr)
    assert (before, during, after) == (1, 1, 2)               # no lane forward while profiling; the lane comes back afterwards
    assert cnt0.sum() > 10 and np.array_equal(cnt0, cnt1)     # the same launches timed per slot
    assert f0 == f1 and r0 == r1


def test_two_contexts_on_two_streams(env):
    fr = env["frames"][SMALL]
    ref = _plain(_model(env, SMALL, False), fr, 1, 6)
    ms = [_model(env, SMALL, True), _model(env, SMALL, True)]
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    got = [[], []]
    for k in range(2):
        with torch.cuda.stream(streams[k]):
            ms[k].preprocess_frames(fr[0:1]); ms[k].run(1)
    for j in range(6):                                        # alternating: each context has a forward in flight while the other is read
        for k in range(2):
            with torch.cuda.stream(streams[k]):
                ms[k].read_begin(1)
                if j + 1 < 6:
                    ms[k].preprocess_frames(fr[j + 1:j + 2]); ms[k].run(1)
                res = ms[k].read_end(1)
                got[k].append((res.raw, _windows(ms[k], res, 1)))
    torch.cuda.synchronize()
    for k in range(2):
        _same(got[k], ref)
        assert ms[k].lane_stats()[0] == 5                     # all but each context's first forward


def test_destroy_with_lane_work_pending(env):
    fr = env["frames"][SMALL]
    ref = _plain(_model(env, SMALL, False), fr, 1, 2)
    m = _model(env, SMALL, True)
    m.preprocess_frames(fr[2:3]); m.run(1)
    _ahead(m, fr[3:4])                                        # its tail is on the lane and is never read
    m._drop_ctx()                                             # apse_destroy: waits for the lane, then frees
    _same(_plain(_model(env, SMALL, True), fr, 1, 2), ref)
