"""-m gpu: what joint RPN / box-head training needs from a live context: TrackRCNN.train_proposals (apse_rpn_train_proposals)
and TrackRCNN.set_rpn_head (apse_set_rpn_head).  Seeded synthetic weights.

* the training selection at the test-time limits returns the test-time proposals, bit for bit;
* at (2000, 1000) it returns what apse_rpn_select_train returns on the context's own rpn_head2 .. rpn_head6 tensors, bit for bit,
  and that result is judged against tests/select_train_ref.py by the rules of tests/test_gpu_select_train.py;
* an inference forward gives the same result bytes before and after it;
* after set_rpn_head the RPN maps and the proposals are those of a fresh model loaded with the merged state, bit for bit, at a
  frame size whose RPN convolutions all run the direct kernel and at one where p2's runs as Winograd; a cached context that was
  idle during the refresh is current when it is used again;
* C4 and 16-bit contexts are refused by both entries.
"""
import numpy as np
import pytest
import torch

import select_ref as R
import test_gpu_select_train as G

pytestmark = pytest.mark.gpu

DEV = "cuda"
SMALL = (128, 224)           # p2 is 32 x 56: 1 x 7 x 4 = 28 Winograd blocks, far below APSE_WINO_MIN_BLOCKS: the direct kernel
# The plan gives a 3 x 3 layer its Winograd filters from APSE_WINO_MIN_BLOCKS = 128 blocks per image on
# (apse_conv_winograd_blocks: ceil(H / 32) x ceil(W / 8) x Cout / 64).  At a 160 x 512 image p2 is 40 x 128: 2 x 16 x 4 = 128;
# 32 pixels less on either side (128 x 512: 1 x 16 x 4, 160 x 480: 2 x 15 x 4) falls below it.  p3 (20 x 64: 32 blocks) stays direct.
WINO = (160, 512)


def wino_blocks(image_h, image_w, level=0):
    ph, pw = (image_h + 31) // 32 * 32, (image_w + 31) // 32 * 32
    h, w = ph >> (2 + level), pw >> (2 + level)
    return ((h + 31) // 32) * ((w + 7) // 8) * (256 // 64)


def test_winograd_threshold_sizes():
    assert wino_blocks(*WINO) == 128 and wino_blocks(WINO[0] - 32, WINO[1]) < 128 and wino_blocks(WINO[0], WINO[1] - 32) < 128
    assert wino_blocks(*WINO, level=1) < 128 and wino_blocks(*SMALL) < 128


def _model(size, batch=1, dtype="f32", arch=None, cache=1, state=None):
    from apse_uav_amd.config import setup_cfg
    from apse_uav_amd.engines.track_predictor import TrackPredictor
    from apse_uav_amd.weights import synthetic_c4_state, synthetic_detector_state
    cfg = setup_cfg(num_classes=4, arch=arch) if arch else setup_cfg(num_classes=4)
    cfg.INPUT.MIN_SIZE_TEST, cfg.INPUT.MAX_SIZE_TEST = size
    cfg.APSE.MAX_BATCH = batch
    cfg.APSE.DTYPE = dtype
    cfg.APSE.CONTEXT_CACHE = cache
    if state is None:
        state = synthetic_c4_state(0, (1, 1, 1, 1)) if arch else synthetic_detector_state(0, (1, 1, 1, 1))
    return TrackPredictor(cfg, state_dict=state).model


def _frames(h, w, n=1):
    from apse_uav_amd.synthetic import SyntheticSequence
    seq = SyntheticSequence("dynamic", h, w)
    return torch.from_numpy(np.stack([seq.frame(5 * i) for i in range(n)])).cuda()


def _heads(model, batch):
    """rpn_head2 .. rpn_head6 of the context as numpy [max_batch][H*W][16], and the level shapes."""
    shapes = model.rpn_level_shapes()
    out = [model.debug_tensor("rpn_head%d" % (l + 2)).reshape(-1, shapes[l][0] * shapes[l][1], 16)[:batch].cpu().numpy() for l in range(5)]
    return out, shapes


def _bytes(t):
    return t.detach().cpu().contiguous().numpy().view(np.uint8)


# ------------------------------------------------------------------------------------------------ training selection
def test_train_proposals_at_test_limits_equal_inference_proposals():
    model = _model(SMALL, batch=2)
    B = model.backbone_frames(_frames(*SMALL, n=2))
    old = model.proposals_after_backbone(B)
    new = model.train_proposals(B, 1000, 1000)
    assert len(new) == 2
    for b in range(2):
        assert old[b].shape[0] > 0 and np.array_equal(_bytes(old[b]), _bytes(new[b][0])), b
        s = new[b][1].cpu().numpy()
        assert s.shape[0] == old[b].shape[0] and (np.diff(s) <= 0).all()
    # the context's own proposals are where the inference selection left them
    again = [model.debug_tensor("proposals").reshape(2, -1, 4)[b, :old[b].shape[0]] for b in range(2)]
    for b in range(2):
        assert np.array_equal(_bytes(old[b]), _bytes(again[b])), b


def test_train_proposals_equal_the_injected_entry_and_the_reference(logdir, monkeypatch):
    model = _model(SMALL, batch=2)
    ih, iw = SMALL
    B = model.backbone_frames(_frames(*SMALL, n=2))
    got = model.train_proposals(B)                                 # cfg: 2000 per level, 1000
    assert int(model.cfg.MODEL.RPN.PRE_NMS_TOPK_TRAIN) == 2000 and int(model.cfg.MODEL.RPN.POST_NMS_TOPK_TRAIN) == 1000
    heads, shapes = _heads(model, B)
    assert 3 * shapes[0][0] * shapes[0][1] > 2048 > 3 * shapes[2][0] * shapes[2][1]      # lists on both sides of 1024 and 2048
    # the injected entry and its judge work on select_ref.FPN_HW: point them at this image
    monkeypatch.setattr(R, "FPN_HW", tuple(shapes))
    monkeypatch.setattr(G, "WS", [w for _, w in shapes])
    monkeypatch.setattr(G, "IMG_H", ih)
    monkeypatch.setattr(G, "IMG_W", iw)
    images = [[np.ascontiguousarray(heads[l][b]) for l in range(5)] for b in range(B)]
    rc, outs, _ = G.run_train(images, 2000, 1000, thr=float(model.cfg.MODEL.RPN.NMS_THRESH))
    assert rc == 0
    for b in range(B):
        n = outs[b]["count"]
        assert n == got[b][0].shape[0] and n > 0
        assert np.array_equal(_bytes(got[b][0]), outs[b]["props"][:n].view(np.uint8)), b
        assert np.array_equal(_bytes(got[b][1]), outs[b]["prop_scores"][:n].view(np.uint8)), b
        G.judge_train("context/%d" % b, logdir, outs[b], images[b], 2000, 1000, thr=float(model.cfg.MODEL.RPN.NMS_THRESH),
                      near_cap=None)


def test_inference_is_undisturbed_by_train_proposals():
    model = _model(SMALL)
    frames = _frames(*SMALL)

    def forward():
        model.preprocess_frames(frames)
        model.run(1)
        model.read(1)
        return bytes(model.last_results.raw)
    forward()
    before = forward()
    B = model.backbone_frames(frames)
    model.train_proposals(B)
    after = forward()
    assert model.last_results.total >= 0 and before == after


# ------------------------------------------------------------------------------------------------ weight refresh
def _perturbed_head(state, seed):
    from apse_uav_amd.networks import rpn_head as rh
    head = rh.RPNHead(DEV)
    head.load_state_dict(state)
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for _, p in head.named_parameters():
            p.add_((torch.randn(p.shape, generator=g) * 0.01).to(DEV))
    return head


def _rpn_outputs(model, frames):
    B = model.backbone_frames(frames)
    props = model.proposals_after_backbone(B)
    heads, _ = _heads(model, B)
    return [h.view(np.uint8) for h in heads] + [_bytes(p) for p in props]


def _same(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("size", [SMALL, WINO])
def test_set_rpn_head_equals_a_fresh_model(size, monkeypatch):
    from apse_uav_amd.networks import rpn_head as rh
    from apse_uav_amd.weights import synthetic_detector_state
    state = synthetic_detector_state(0, (1, 1, 1, 1))
    frames = _frames(*size)
    model = _model(size, state=state)
    first = _rpn_outputs(model, frames)
    head = _perturbed_head(state, 3)
    model.set_rpn_head(head)
    got = _rpn_outputs(model, frames)
    assert model.contexts_built == 1 and not _same(first, got)
    merged = rh.merge_rpn_head(state, head.state_dict())
    for k, v in head.state_dict(rh.PREFIX).items():                # _state follows the head
        assert torch.equal(model._state[k], v.cpu()) and torch.equal(merged[k], v.cpu())
    fresh = _model(size, state=merged)
    want = _rpn_outputs(fresh, frames)
    assert _same(got, want)
    tp = model.train_proposals(1)
    tf = fresh.train_proposals(1)
    assert np.array_equal(_bytes(tp[0][0]), _bytes(tf[0][0])) and np.array_equal(_bytes(tp[0][1]), _bytes(tf[0][1]))
    # which kernel p2's RPN convolution ran: with the Winograd layers switched off (read at apse_create) the bits of rpn_head2
    # change exactly where the plan had given it Winograd filters
    monkeypatch.setenv("APSE_F32_WINOGRAD", "0")
    direct = _rpn_outputs(_model(size, state=merged), frames)
    assert np.array_equal(direct[0], want[0]) == (size == SMALL)


def test_set_rpn_head_reaches_an_idle_cached_context():
    from apse_uav_amd.networks import rpn_head as rh
    from apse_uav_amd.weights import synthetic_detector_state
    state = synthetic_detector_state(0, (1, 1, 1, 1))
    other = (96, 160)
    fa, fb = _frames(*SMALL), _frames(*other)
    model = _model((96, 224), cache=2, state=state)          # two frame sizes: two contexts
    a0 = _rpn_outputs(model, fa)                             # the context of size A ...
    _rpn_outputs(model, fb)                                  # ... is idle while B's is current
    assert model.contexts_built == 2
    head = _perturbed_head(state, 4)
    model.set_rpn_head(head)
    b1 = _rpn_outputs(model, fb)
    a1 = _rpn_outputs(model, fa)                             # used again: refreshed first
    assert model.contexts_built == 2 and not _same(a0, a1)
    fresh = _model((96, 224), cache=2, state=rh.merge_rpn_head(state, head.state_dict()))
    assert _same(a1, _rpn_outputs(fresh, fa)) and _same(b1, _rpn_outputs(fresh, fb))
    # a second refresh while A is current reaches B when it comes back
    head2 = _perturbed_head(state, 5)
    model.set_rpn_head(head2)
    fresh2 = _model((96, 224), cache=2, state=rh.merge_rpn_head(state, head2.state_dict()))
    assert _same(_rpn_outputs(model, fb), _rpn_outputs(fresh2, fb)) and model.contexts_built == 2


# ------------------------------------------------------------------------------------------------ refusals
@pytest.mark.parametrize("kind", ["C4", "bf16"])
def test_refusals(kind):
    from apse_uav_amd import _lib
    lib = _lib.load()
    model = _model((256, 448), arch="C4") if kind == "C4" else _model(SMALL, dtype="bf16")
    model.backbone_frames(_frames(270, 480) if kind == "C4" else _frames(*SMALL))
    t = torch.full((1 << 16,), 7.0, device=DEV)
    ti = torch.full((4,), 7, dtype=torch.int32, device=DEV)
    ws = torch.empty(int(lib.apse_rpn_train_proposals_workspace_bytes(1, 2000)), dtype=torch.uint8, device=DEV)
    p, s = _lib.ptr(t), _lib.stream_ptr()
    assert lib.apse_rpn_train_proposals(model._ctx, 1, 2000, 1000, p, p, _lib.ptr(ti), _lib.ptr(ws), ws.numel(), s) == -1
    err = lib.apse_last_error(model._ctx)
    assert b"apse_rpn_train_proposals" in err and (b"C4" in err if kind == "C4" else b"f32" in err)
    assert lib.apse_set_rpn_head(model._ctx, p, p, p, p, p, p, s) == -1
    err = lib.apse_last_error(model._ctx)
    assert b"apse_set_rpn_head" in err and (b"C4" in err if kind == "C4" else b"f32" in err)
    torch.cuda.synchronize()
    assert float((t - 7.0).abs().max()) == 0.0 and int((ti - 7).abs().max()) == 0          # nothing was launched
    if kind == "C4":
        with pytest.raises(NotImplementedError):
            model.train_proposals(1)
        with pytest.raises(NotImplementedError):
            model.set_rpn_head({})


def test_limits_of_the_context_entry():
    from apse_uav_amd import _lib
    lib = _lib.load()
    model = _model(SMALL)
    model.backbone_frames(_frames(*SMALL))
    t = torch.full((1 << 16,), 7.0, device=DEV)
    ti = torch.full((4,), 7, dtype=torch.int32, device=DEV)
    need = int(lib.apse_rpn_train_proposals_workspace_bytes(1, 2048))
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    p, ip, s = _lib.ptr(t), _lib.ptr(ti), _lib.stream_ptr()
    assert need > 0 and lib.apse_rpn_train_proposals_workspace_bytes(1, 2049) == 0 and lib.apse_rpn_train_proposals_workspace_bytes(0, 2000) == 0
    for (batch, pre, post, nbytes) in [(2, 2000, 1000, need), (1, 0, 1000, need), (1, 2049, 1000, need), (1, 2000, 0, need),
                                       (1, 2000, 2049, need), (1, 2048, 1000, need - 1)]:
        assert lib.apse_rpn_train_proposals(model._ctx, batch, pre, post, p, p, ip, _lib.ptr(ws), nbytes, s) == -1, (batch, pre, post)
        assert b"apse_rpn_train_proposals" in lib.apse_last_error(model._ctx)
    assert lib.apse_rpn_train_proposals(model._ctx, 1, 2000, 1000, None, p, ip, _lib.ptr(ws), need, s) == -1
    assert lib.apse_set_rpn_head(model._ctx, p, p, None, p, p, p, s) == -1
    torch.cuda.synchronize()
    assert float((t - 7.0).abs().max()) == 0.0 and int((ti - 7).abs().max()) == 0
