"""Host side of box-head training: hand-derived cases that pin the restatement (tests/box_train_ref.py), the sampling invariants,
checkpoint merging and the refused limits of the ABI -- no GPU needed."""
import math

import numpy as np
import pytest
import torch

import box_train_ref as R


# ------------------------------------------------------------------------------------------------ the restatement, by hand
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_matcher_hand_cases(dtype):
    gts = torch.tensor([[0, 0, 1, 1], [10, 10, 14, 14]], dtype=dtype)
    cls = torch.tensor([2, 0])
    props = torch.tensor([[0, 0, 2, 1],          # IoU exactly 0.5 with ground truth 0: 1 / (1 + 2 - 1) -> foreground
                          [10, 10, 14, 12],      # half of ground truth 1: 8 / 16 = 0.5 -> foreground
                          [20, 20, 30, 30]], dtype=dtype)          # touches nothing
    idx, iou, lab = R.match(props, gts, cls, 3)
    assert idx.tolist() == [0, 1, 0] and iou.tolist() == [0.5, 0.5, 0.0] and lab.tolist() == [2, 0, 3]
    # a proposal equidistant from two ground truths: the lowest index
    gts = torch.tensor([[0, 0, 4, 4], [4, 0, 8, 4]], dtype=dtype)
    idx, iou, lab = R.match(torch.tensor([[2, 0, 6, 4]], dtype=dtype), gts, torch.tensor([1, 0]), 2, thresh=0.3)
    assert idx.tolist() == [0] and iou.tolist() == [float(torch.tensor(8.0, dtype=dtype) / 24)] and lab.tolist() == [1]
    # boxes that only touch: zero-area overlap, IoU 0
    idx, iou, lab = R.match(torch.tensor([[4, 0, 8, 4]], dtype=dtype), gts[:1], torch.tensor([1]), 2)
    assert iou.tolist() == [0.0] and lab.tolist() == [2]
    # no ground truth
    idx, iou, lab = R.match(props, torch.zeros(0, 4, dtype=dtype), torch.zeros(0, dtype=torch.int64), 3)
    assert idx.tolist() == [0, 0, 0] and iou.tolist() == [0.0] * 3 and lab.tolist() == [3, 3, 3]


def test_get_deltas_hand_cases():
    b = torch.tensor([[3.0, 5.0, 11.0, 9.0]], dtype=torch.float64)
    assert R.get_deltas(b, b).tolist() == [[0.0, 0.0, 0.0, 0.0]]
    wide = torch.tensor([[-1.0, 5.0, 15.0, 9.0]], dtype=torch.float64)          # same centre, doubled width
    d = R.get_deltas(b, wide)[0].tolist()
    assert d[0] == 0.0 and d[1] == 0.0 and d[3] == 0.0 and d[2] == pytest.approx(5 * math.log(2), rel=1e-15)
    moved = torch.tensor([[5.0, 6.0, 13.0, 10.0]], dtype=torch.float64)         # + (2, 1): dx = 10 * 2 / 8, dy = 10 * 1 / 4
    assert R.get_deltas(b, moved)[0].tolist() == [2.5, 2.5, 0.0, 0.0]


@pytest.mark.parametrize("beta", [0.0, 0.5])
def test_two_row_loss_by_hand(beta):
    K = 2
    logits = torch.tensor([[0.0, math.log(3.0), 0.0], [1.0, 1.0, 1.0]], dtype=torch.float64)
    labels = torch.tensor([1, 2])                       # row 0 foreground class 1, row 1 background
    props = torch.tensor([[0.0, 0.0, 8.0, 4.0], [0.0, 0.0, 1.0, 1.0]], dtype=torch.float64)
    gts = torch.tensor([[2.0, 1.0, 10.0, 5.0], [0.0, 0.0, 1.0, 1.0]], dtype=torch.float64)       # target (2.5, 2.5, 0, 0)
    deltas = torch.zeros(2, 8, dtype=torch.float64)
    deltas[0, 4:8] = torch.tensor([2.75, 1.5, 0.0, -2.0])                       # |d| = 0.25, 1.0, 0, 2.0
    deltas[0, 0:4] = 99.0                                                       # another class: not compared
    deltas[1] = 7.0                                                             # background row: not compared
    lc, lb = R.box_losses(logits, deltas, labels, props, gts, beta)
    # row 0: softmax = (1, 3, 1) / 5 -> -ln(3/5); row 1: -ln(1/3); mean over the 2 rows
    assert float(lc) == pytest.approx(0.5 * (math.log(5 / 3) + math.log(3)), rel=1e-14)
    if beta == 0.0:
        want = (0.25 + 1.0 + 0.0 + 2.0) / 2                                     # divided by n = 2, not by the foreground count
    else:
        want = (0.5 * 0.25 ** 2 / 0.5 + (1.0 - 0.25) + 0.0 + (2.0 - 0.25)) / 2
    assert float(lb) == pytest.approx(want, rel=1e-14)
    acc, fg_acc, fn, nfg, nbg = R.box_stats(logits, labels)
    assert (acc, fg_acc, fn, nfg, nbg) == (0.5, 1.0, 0.0, 1, 1)                 # row 1: a three-way tie -> class 0, not background
    # no foreground row -> 0
    assert float(R.box_losses(logits, deltas, torch.tensor([2, 2]), props, gts, beta)[1]) == 0.0


# ------------------------------------------------------------------------------------------------ sampling
@pytest.mark.parametrize("nfg,nbg", [(0, 700), (5, 700), (128, 700), (129, 700), (600, 700), (40, 200), (600, 100)])
def test_subsample_invariants(nfg, nbg):
    from apse_uav_amd.utils import box_train as bt
    K = 4
    g = torch.Generator().manual_seed(nfg * 1000 + nbg)
    labels = torch.cat([torch.randint(0, K, (nfg,), generator=g), torch.full((nbg,), K)])[torch.randperm(nfg + nbg, generator=g)]
    want_fg = min(nfg, 128)
    want_bg = min(nbg, 512 - want_fg)
    for fn in (bt.subsample_labels, R.subsample_labels):
        pos, neg = fn(labels, 512, 0.25, K, torch.Generator().manual_seed(7))
        assert pos.numel() == want_fg and neg.numel() == want_bg
        both = torch.cat([pos, neg])
        assert both.unique().numel() == both.numel()
        assert bool((labels[pos] != K).all()) and bool((labels[neg] == K).all())
        pos2, neg2 = fn(labels, 512, 0.25, K, torch.Generator().manual_seed(7))
        assert torch.equal(pos, pos2) and torch.equal(neg, neg2)
    # the project's draw is the restatement's draw
    a = bt.subsample_labels(labels, 512, 0.25, K, torch.Generator().manual_seed(11))
    b = R.subsample_labels(labels, 512, 0.25, K, torch.Generator().manual_seed(11))
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


# ------------------------------------------------------------------------------------------------ head object and ABI
def test_merge_box_head_and_state():
    from apse_uav_amd.networks.box_head import PREFIX, BoxHead, merge_box_head
    torch.manual_seed(0)
    head = BoxHead(2, "cpu")
    hs = head.state_dict()
    assert list(hs) == R.param_names()
    assert hs["box_head.fc1.weight"].shape == (1024, 12544) and hs["box_predictor.cls_score.weight"].shape == (3, 1024)
    assert hs["box_predictor.bbox_pred.weight"].shape == (8, 1024)
    assert all(float(hs[n + ".bias"].abs().max()) == 0.0 for n in R.NAMES)
    bound = math.sqrt(3.0 / 12544)                                       # kaiming_uniform_(a=1): sqrt(6 / (2 fan_in))
    assert float(hs["box_head.fc1.weight"].abs().max()) <= bound and float(hs["box_head.fc1.weight"].abs().max()) > 0.99 * bound
    assert 0.008 < float(hs["box_predictor.cls_score.weight"].std()) < 0.012
    assert 0.0008 < float(hs["box_predictor.bbox_pred.weight"].std()) < 0.0012
    det = {"backbone.x": torch.ones(1), "model.roi_heads.mask_head.deconv.bias": torch.ones(2),
           PREFIX + "box_head.fc2.bias": torch.full((1024,), 9.0)}
    m = merge_box_head(det, hs)
    assert "roi_heads.mask_head.deconv.bias" in m and "backbone.x" in m and len(m) == 2 + 8
    assert torch.equal(m[PREFIX + "box_head.fc2.bias"], hs["box_head.fc2.bias"])          # the trained head wins
    m2 = merge_box_head(det, head.state_dict(PREFIX))
    assert all(torch.equal(m[k], m2[k]) for k in m)
    with pytest.raises(KeyError):
        merge_box_head(det, {k: v for k, v in hs.items() if k != "box_predictor.bbox_pred.bias"})
    with pytest.raises(KeyError):
        merge_box_head(det, dict(hs, stray=torch.ones(1)))
    h2 = BoxHead(2, "cpu")
    h2.load_state_dict(m)
    assert all(torch.equal(a, b) for a, b in zip(h2.state_dict().values(), hs.values()))
    with pytest.raises(RuntimeError):
        BoxHead(3, "cpu").load_state_dict(hs)
    h3 = BoxHead(3, "cpu")                                                # another class count: fc1 / fc2 only
    h3.load_state_dict(hs, keep_predictor=True)
    assert torch.equal(h3.state_dict()["box_head.fc1.weight"], hs["box_head.fc1.weight"])
    assert h3.state_dict()["box_predictor.cls_score.weight"].shape == (4, 1024)
    assert all(p.requires_grad and p.is_leaf and p.dtype == torch.float32 for p in head.parameters())


def test_limits_refused():
    import ctypes as C
    from apse_uav_amd import _lib
    from apse_uav_amd.config import setup_cfg
    from apse_uav_amd.networks import box_head as bh
    lib = _lib.load()
    assert bh.MAX_ROIS == 1024 and bh.MAX_CLASSES == 80
    wsb = lib.apse_box_train_workspace_bytes
    assert wsb(1024, 80) > 0 and wsb(1, 1) > 0
    assert wsb(1025, 4) == 0 and wsb(0, 4) == 0 and wsb(4, 81) == 0 and wsb(4, 0) == 0
    one = np.zeros(16, np.float32)
    ione = np.zeros(16, np.int32)
    p, ip = _lib.ptr(one), _lib.ptr(ione)
    w4 = (C.c_float * 4)(10, 10, 5, 5)

    def refused(rc, text):
        assert rc == -1 and text in lib.apse_last_error(None), (rc, lib.apse_last_error(None))

    # n = 1025
    refused(lib.apse_box_fc_wgrad(p, p, 1025, 4, 4, p, None), b"APSE_BOX_TRAIN_MAX_N")
    refused(lib.apse_box_fc_forward(p, p, p, 1025, 4, 4, 0, p, p, 1 << 20, None), b"APSE_BOX_TRAIN_MAX_N")
    refused(lib.apse_box_fc_dgrad(p, p, 1025, 4, 4, 0, p, None), b"APSE_BOX_TRAIN_MAX_N")
    refused(lib.apse_box_bias_grad(p, 1025, 4, p, p, 1 << 20, None), b"APSE_BOX_TRAIN_MAX_N")
    refused(lib.apse_box_permute_features(p, 1025, p, None), b"APSE_BOX_TRAIN_MAX_N")
    refused(lib.apse_box_loss_forward(p, p, ip, p, p, 1025, 1, w4, 0.0, p, p, 1 << 20, None), b"APSE_BOX_TRAIN_MAX_N")
    refused(lib.apse_box_loss_backward(p, p, ip, p, p, 1025, 1, w4, 0.0, None, None, p, p, None), b"APSE_BOX_TRAIN_MAX_N")
    # K = 0 and 81
    for K in (0, 81):
        refused(lib.apse_box_loss_forward(p, p, ip, p, p, 1, K, w4, 0.0, p, p, 1 << 20, None), b"APSE_MAX_CLASSES")
        refused(lib.apse_box_loss_backward(p, p, ip, p, p, 1, K, w4, 0.0, None, None, p, p, None), b"APSE_MAX_CLASSES")
        refused(lib.apse_box_match(p, 1, p, ip, 1, K, 0.5, ip, p, ip, None), b"APSE_MAX_CLASSES")
    # G = 4097
    refused(lib.apse_box_match(p, 1, p, ip, 4097, 4, 0.5, ip, p, ip, None), b"4096")
    # layer shapes
    refused(lib.apse_box_fc_wgrad(p, p, 1, 1025, 4, p, None), b"1024")
    refused(lib.apse_box_fc_wgrad(p, p, 1, 4, 0, p, None), b"1024")
    # null pointers
    refused(lib.apse_box_match(None, 1, p, ip, 1, 4, 0.5, ip, p, ip, None), b"null")
    refused(lib.apse_box_match(p, 1, None, ip, 1, 4, 0.5, ip, p, ip, None), b"null")
    refused(lib.apse_box_fc_forward(None, p, p, 1, 4, 4, 0, p, p, 1 << 20, None), b"null")
    refused(lib.apse_box_fc_dgrad(p, None, 1, 4, 4, 0, p, None), b"null")
    refused(lib.apse_box_fc_wgrad(p, p, 1, 4, 4, None, None), b"null")
    refused(lib.apse_box_bias_grad(p, 1, 4, None, p, 1 << 20, None), b"null")
    refused(lib.apse_box_permute_features(p, 1, None, None), b"null")
    refused(lib.apse_box_loss_forward(p, p, None, p, p, 1, 1, w4, 0.0, p, p, 1 << 20, None), b"null")
    refused(lib.apse_box_loss_forward(p, p, ip, p, p, 1, 1, None, 0.0, p, p, 1 << 20, None), b"null")
    refused(lib.apse_box_loss_backward(p, p, ip, p, p, 1, 1, w4, 0.0, None, None, None, p, None), b"null")
    # a workspace too small
    refused(lib.apse_box_loss_forward(p, p, ip, p, p, 2, 1, w4, 0.0, p, p, 2 * 6 * 8 - 1, None), b"workspace")
    refused(lib.apse_box_bias_grad(p, 65, 4, p, p, 2 * 4 * 8 - 1, None), b"workspace")
    refused(lib.apse_box_fc_forward(p, p, p, 2, 4, 12544, 0, p, p, 8 * 2 * 4 * 4 - 1, None), b"workspace")
    refused(lib.apse_box_fc_forward(p, p, p, 2, 4, 12544, 0, p, None, 0, None), b"workspace")
    # n = 0 and N = 0 enqueue nothing and succeed without touching a pointer
    assert lib.apse_box_loss_forward(None, None, None, None, None, 0, 4, w4, 0.0, None, None, 0, None) == 0
    assert lib.apse_box_loss_backward(None, None, None, None, None, 0, 4, w4, 0.0, None, None, None, None, None) == 0
    assert lib.apse_box_match(None, 0, None, None, 0, 4, 0.5, None, None, None, None) == 0
    # the context entries
    assert lib.apse_box_roi_features(None, 0, p, 1, p, None) != 0 and lib.apse_proposals(None, 0, p, ip, None) != 0
    # Python surface
    with pytest.raises(_lib.ApseError):
        bh._workspace(bh.MAX_ROIS + 1, 4, "cpu")
    with pytest.raises(ValueError):
        bh.BoxHead(81)
    with pytest.raises(ValueError):
        bh.BoxHead(0)
    with pytest.raises(NotImplementedError):
        bh.BoxHead.from_cfg(setup_cfg(num_classes=4, arch="C4"))
    assert bh.BoxHead.from_cfg(setup_cfg(num_classes=7), "cpu").num_classes == 7
    head = bh.BoxHead(2, "cpu")
    with pytest.raises(_lib.ApseError):
        head(torch.zeros(1, 7, 7, 256), torch.zeros(1), torch.zeros(1, 4), torch.zeros(1, 4))
    with pytest.raises(_lib.ApseError):
        head.predict(torch.zeros(1, 7, 7, 256))


def test_header_names():
    import os
    import re
    from apse_uav_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "apse_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(apse_[a-z0-9_]+)\s*\(", text))
    new = {"apse_box_roi_features", "apse_proposals", "apse_box_train_workspace_bytes", "apse_box_match", "apse_box_permute_features",
           "apse_box_fc_forward", "apse_box_fc_dgrad", "apse_box_fc_wgrad", "apse_box_bias_grad", "apse_box_loss_forward",
           "apse_box_loss_backward"}
    assert new <= declared and new <= set(_lib.EXPORTS)
    assert "#define APSE_BOX_TRAIN_MAX_N 1024" in open(os.path.join(root, "include", "apse_hip.h")).read()
