"""RPN-head training on the GPU (csrc/rpn_train.hip, networks/rpn_head.py): the anchor labelling bit for bit against the f32
restatement (tests/rpn_train_ref.py), the patch gather bit for bit against unfold-style indexing of the exported FPN maps, the loss
and its gradient under the float64 arbiter of tests/mask_train_ref.py and exactly on a lattice, the whole head against torch-CPU
autograd, determinism, agreement with the inference path, and the refused limits.

Observed errors (normalised by max|f64|) are printed per output and logged to rpn_train.log in the log directory; DESIGN.md
"RPN-head training" records them.
"""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import rpn_train_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NAN = float("nan")
PNAMES = ("p2", "p3", "p4", "p5", "p6")


def _log(logdir, name, obj):
    print(name, json.dumps(obj))
    with open(os.path.join(logdir, "rpn_train.log"), "a") as f:
        f.write(name + " " + json.dumps(obj) + "\n")


def _judge(logdir, tag, outputs, factor=2.0):
    """outputs: {name: (hip, f64, f32)}; logs every pair of errors, then asserts the arbiter rule on each."""
    rows, bad = {}, []
    for name, (hip, f64, f32) in outputs.items():
        eh, ef, bound, ok = R.arbiter(hip, f64, f32, factor)
        rows[name] = {"hip": eh, "torch_f32": ef, "bound": bound}
        if not ok:
            bad.append(name)
    _log(logdir, tag, rows)
    assert not bad, (tag, {k: rows[k] for k in bad})


def _rh():
    from apse_uav_amd.networks import rpn_head
    return rpn_head


# ------------------------------------------------------------------------------------------------ labelling
LABEL_IMAGES = {"256x448": (256, 448), "40x72": (40, 72)}          # levels 64x112 .. 4x7, and 16x24 .. a 1-row p6 (1x2)
_ANCHORS = {}


def _anchors(image):
    if image not in _ANCHORS:
        _ANCHORS[image] = R.anchors(R.level_shapes(*LABEL_IMAGES[image]))[0]
    return _ANCHORS[image]


def draw_ground_truth(image, j, seed):
    """Box j of a case: every second one a randomly chosen anchor with each side moved by up to a tenth of its width (its best
    anchor is that one, with an IoU near or above 0.7), the others anywhere in the image with sides of 24 px to 60 % of it."""
    g = torch.Generator().manual_seed(seed)
    anc = _anchors(image)
    ih, iw = LABEL_IMAGES[image]
    if j % 2 == 0:
        a = anc[int(torch.randint(0, anc.shape[0], (1,), generator=g))]
        return (a + (torch.rand(4, generator=g) - 0.5) * 0.2 * (a[2] - a[0])).float()
    wh = 24 + torch.rand(2, generator=g) * 0.6 * torch.tensor([iw - 24.0, ih - 24.0]).clamp(min=1)
    xy = torch.rand(2, generator=g) * torch.tensor([float(iw), float(ih)]) - 0.25 * wh
    return torch.cat([xy, xy + wh]).float()


def label_case_is_clean(anc, gts):
    """In float64: no anchor / ground-truth IoU within 1e-5 of 0.3 or of 0.7, and none within 1e-5 of its ground truth's maximum
    without being that maximum.  Without it a label would be a rounding question."""
    if gts.shape[0] == 0:
        return True
    q = R.pairwise_iou(gts.double(), anc.double())
    if bool((((q - 0.3).abs() < 1e-5) | ((q - 0.7).abs() < 1e-5)).any()):
        return False
    best = q.max(dim=1, keepdim=True).values
    return not bool((((best - q) < 1e-5) & (q != best)).any())


def clean_ground_truths(image, G, seed):
    """G boxes drawn on the CPU, each re-seeded until it is clean (the condition reads one ground truth's row of IoUs, so a box is
    clean or not on its own; at most 50 tries each).  -> (boxes f32 [G][4], tries)."""
    anc = _anchors(image)
    out, tries = [], 0
    for j in range(G):
        for k in range(50):
            tries += 1
            box = draw_ground_truth(image, j, (seed * 100 + j) * 50 + k)
            if label_case_is_clean(anc, box[None]):
                out.append(box)
                break
        else:
            raise AssertionError("no clean box in 50 seeds for %s G = %d, box %d" % (image, G, j))
    return (torch.stack(out) if out else torch.zeros(0, 4)), tries


def _label_on_gpu(image, gts):
    rh = _rh()
    shapes = R.level_shapes(*LABEL_IMAGES[image])
    lab, idx, iou = rh.anchor_labels(shapes, gts, device=DEV)
    torch.cuda.synchronize()
    return lab.cpu().numpy(), idx.cpu().numpy(), iou.cpu().numpy()


def _check_labels(image, gts):
    anc = _anchors(image)
    assert label_case_is_clean(anc, gts)                               # before the GPU is touched
    labels, idx, iou = R.label_anchors(anc, gts)                       # the f32 restatement
    l64, i64, _ = R.label_anchors(anc.double(), gts.double())
    assert torch.equal(l64, labels) and torch.equal(i64, idx)          # the condition above at work
    got = _label_on_gpu(image, gts)
    again = _label_on_gpu(image, gts)
    assert got[0].dtype == np.int32 and got[0].shape == (anc.shape[0],)
    assert np.array_equal(got[0], labels.numpy().astype(np.int32))
    assert np.array_equal(got[1], idx.numpy().astype(np.int32))
    assert np.array_equal(got[2], iou.numpy())
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got, again))
    return labels


@pytest.mark.parametrize("G", [0, 1, 7, 65])
@pytest.mark.parametrize("image", sorted(LABEL_IMAGES))
def test_labelling_bit_exact(image, G):
    gts, _ = clean_ground_truths(image, G, 100 * G + len(image))
    labels = _check_labels(image, gts)
    if G == 0:
        assert int(labels.abs().max()) == 0
    else:
        assert int((labels == 1).sum()) >= 1 and int((labels == 0).sum()) >= 1


def test_labelling_second_chunk_of_ground_truths():
    """G = 1025 on the small grid: the kernels stage the ground truths in LDS 1024 at a time, so box 1024 is alone in a second
    chunk -- its block maxima, its place in the argmax (an index >= 1024) and the low-quality rule across chunks.  Box 1024 is an
    anchor's own box, so that anchor's best ground truth is in the second chunk."""
    image = "40x72"
    gts, _ = clean_ground_truths(image, 1025, 7)
    anc = _anchors(image)
    for i in range(anc.shape[0] - 1, -1, -1):                       # the last anchor that no earlier box already equals
        gts[1024] = anc[i]
        if label_case_is_clean(anc, gts[1024:]) and float(R.pairwise_iou(gts[:1024], anc[i:i + 1]).max()) < 0.99:
            break
    labels = _check_labels(image, gts)
    _, idx, iou = R.label_anchors(anc, gts)
    assert int(idx[i]) == 1024 and float(iou[i]) == 1.0 and int(labels[i]) == 1


@pytest.mark.parametrize("name", sorted(R.hand_cases()))
def test_labelling_hand_cases(name):
    gts = R.hand_cases()[name]
    labels = _check_labels("256x448", gts)
    if name == "two_anchor_tie":
        assert int((labels == 1).sum()) == 2
    if name == "no_overlap":
        assert bool((labels == 1).all())


# ------------------------------------------------------------------------------------------------ patch gather
def _predictor(size, arch=None):
    from apse_uav_amd.config import setup_cfg
    from apse_uav_amd.engines.track_predictor import TrackPredictor
    from apse_uav_amd.weights import synthetic_c4_state, synthetic_detector_state
    cfg = setup_cfg(num_classes=4, arch=arch) if arch else setup_cfg(num_classes=4)
    cfg.INPUT.MIN_SIZE_TEST, cfg.INPUT.MAX_SIZE_TEST = size
    cfg.APSE.MAX_BATCH = 1
    cfg.APSE.DTYPE = "f32"
    sd = synthetic_c4_state(0, (1, 1, 1, 1)) if arch else synthetic_detector_state(0, (1, 1, 1, 1))
    return TrackPredictor(cfg, state_dict=sd)


@pytest.fixture(scope="module")
def predictor():
    return _predictor((256, 448))


def _frames(h, w):
    from apse_uav_amd.synthetic import SyntheticSequence
    return torch.from_numpy(SyntheticSequence("dynamic", h, w).frame(0)[None]).cuda()


def _unfolded(model):
    """Per level the exported map as unfold columns [2304][H W] ((c, kh, kw) rows, zero padding 1), and the level shapes."""
    cols, shapes = [], []
    for name in PNAMES:
        m = model.export_feature(name, 1).cpu()                        # [1][256][H][W]
        shapes.append((m.shape[2], m.shape[3]))
        cols.append(F.unfold(m, 3, padding=1)[0])
    return cols, shapes


def _gather_list(shapes, seed):
    """256 global anchor indices: the four corners of every level (slots cycling through 0, 1, 2), a duplicated anchor, the same
    position under another slot, then seeded random ones."""
    off, out, k = 0, [], 0
    for (H, W) in shapes:
        for (y, x) in ((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)):
            out.append(off + 3 * (y * W + x) + k % 3)
            k += 1
        off += 3 * H * W
    out += [out[5], out[5], out[5] - out[5] % 3 + (out[5] + 1) % 3]
    g = torch.Generator().manual_seed(seed)
    out += torch.randint(0, off, (256 - len(out),), generator=g).tolist()
    return torch.tensor(out, dtype=torch.int64), off


def _check_gather(model, sizes):
    cols, shapes = _unfolded(model)
    assert shapes == model.rpn_level_shapes()
    anc, level, ys, xs, slot = R.anchors(shapes)
    idx_all, A = _gather_list(shapes, 5)
    assert A == anc.shape[0]
    for S in sizes:
        idx = idx_all[:S]
        x, sl, boxes, lv = model.rpn_patches(idx.to(DEV))
        torch.cuda.synchronize()
        want = torch.stack([cols[int(level[i])][:, int(ys[i]) * shapes[int(level[i])][1] + int(xs[i])] for i in idx])
        assert tuple(x.shape) == (S, 2304) and np.array_equal(x.cpu().numpy(), want.numpy()), S
        assert np.array_equal(sl.cpu().numpy(), slot[idx].numpy().astype(np.int32))
        assert np.array_equal(lv.cpu().numpy(), level[idx].numpy().astype(np.int32))
        assert np.array_equal(boxes.cpu().numpy(), anc[idx].numpy())
    return anc, A


def test_gather_bit_exact(predictor):
    model = predictor.model
    model.backbone_frames(_frames(256, 448))
    anc, A = _check_gather(model, (1, 127, 128, 129, 256))
    # an index outside 0 .. A - 1: a zero row, slot 0, a zero box, level -1; S = 0: nothing
    x, sl, boxes, lv = model.rpn_patches(torch.tensor([-1, A, A - 1]))
    torch.cuda.synchronize()
    assert float(x[:2].abs().max()) == 0.0 and float(boxes[:2].abs().max()) == 0.0
    assert sl.cpu().tolist() == [0, 0, 2] and lv.cpu().tolist() == [-1, -1, 4]
    assert np.array_equal(boxes[2].cpu().numpy(), anc[A - 1].numpy())
    assert tuple(model.rpn_patches(torch.zeros(0, dtype=torch.int64))[0].shape) == (0, 2304)


def test_gather_second_image_of_a_batch():
    """A context of two images: the rows of image 1 come from image 1's maps (and those of image 0 from image 0's)."""
    from apse_uav_amd.config import setup_cfg
    from apse_uav_amd.engines.track_predictor import TrackPredictor
    from apse_uav_amd.synthetic import SyntheticSequence
    from apse_uav_amd.weights import synthetic_detector_state
    cfg = setup_cfg(num_classes=4)
    cfg.INPUT.MIN_SIZE_TEST, cfg.INPUT.MAX_SIZE_TEST = 128, 224
    cfg.APSE.MAX_BATCH = 2
    cfg.APSE.DTYPE = "f32"
    model = TrackPredictor(cfg, state_dict=synthetic_detector_state(0, (1, 1, 1, 1))).model
    seq = SyntheticSequence("dynamic", 128, 224)
    model.backbone_frames(torch.from_numpy(np.stack([seq.frame(0), seq.frame(5)])).cuda())
    maps = [model.export_feature(name, 2).cpu() for name in PNAMES]             # [2][256][H][W]
    shapes = [(m.shape[2], m.shape[3]) for m in maps]
    assert shapes == model.rpn_level_shapes() and not torch.equal(maps[0][0], maps[0][1])
    anc, level, ys, xs, slot = R.anchors(shapes)
    idx = _gather_list(shapes, 9)[0][:64]
    for image in (0, 1):
        cols = [F.unfold(m[image:image + 1], 3, padding=1)[0] for m in maps]
        x, sl, boxes, lv = model.rpn_patches(idx.to(DEV), image=image)
        torch.cuda.synchronize()
        want = torch.stack([cols[int(level[i])][:, int(ys[i]) * shapes[int(level[i])][1] + int(xs[i])] for i in idx])
        assert np.array_equal(x.cpu().numpy(), want.numpy()), image
        assert np.array_equal(boxes.cpu().numpy(), anc[idx].numpy()) and sl.cpu().tolist() == slot[idx].tolist()
    labels, _, _ = model.rpn_anchor_targets(anc[:1], image=1)
    assert int(labels[0]) == 1
    with pytest.raises(ValueError):
        model.rpn_anchor_targets(anc[:1], image=2)


def test_gather_one_row_p6():
    """A 40 x 72 image: p6 is 1 x 2, so every p6 row reads zero padding above and below."""
    model = _predictor((40, 72)).model
    model.backbone_frames(_frames(40, 72))
    _check_gather(model, (256,))
    assert model.rpn_level_shapes()[4] == (1, 2)


# ------------------------------------------------------------------------------------------------ loss
def loss_case(S, seed, kind):
    g = torch.Generator().manual_seed(seed)
    slots, labels, anc, gts = R.sample_rows(S, seed + 1)
    if kind == "negative":
        labels[:] = 0
    elif kind == "positive":
        labels[:] = 1
    logits = torch.randn(S, 3, generator=g) * 3
    deltas = torch.randn(S, 12, generator=g)
    if S >= 4:
        logits[S - 1] = torch.tensor([80.0, -80.0, 80.0])
        logits[S - 2] = torch.tensor([-80.0, 80.0, -80.0])
        logits[S - 3] = 0.0
    return logits, deltas, slots, labels, anc, gts


def loss_case_is_clean(deltas, slots, labels, anc, gts, beta):
    """beta 0: smooth_l1 is |d| and its gradient jumps at d = 0; no compared difference may lie within 1e-4 of 0 (float64)."""
    if beta >= 1e-5 or not bool((labels > 0).any()):
        return True
    _, d = R.own_columns(torch.zeros(deltas.shape[0], 3, dtype=torch.float64), deltas.double(), slots)
    diff = (d - R.get_deltas(anc.double(), gts.double()))[labels > 0]
    return bool((diff.abs() > 1e-4).all())


@pytest.mark.parametrize("kind", ["mixed", "negative", "positive"])
@pytest.mark.parametrize("beta", [0.0, 1.0 / 9])
@pytest.mark.parametrize("S", [1, 64, 257])
def test_loss_and_gradient(logdir, S, beta, kind):
    rh = _rh()
    logits, deltas, slots, labels, anc, gts = loss_case(S, 10 * S + 3, kind)
    assert loss_case_is_clean(deltas, slots, labels, anc, gts, beta)
    norm = 256 * ((S + 255) // 256)
    gcls, gloc = 0.5, 2.0
    ref = {}
    for dt in (torch.float64, torch.float32):
        lg, dl = logits.to(dt).requires_grad_(True), deltas.to(dt).requires_grad_(True)
        lc, ll = R.rpn_losses(lg, dl, slots, labels, anc.to(dt), gts.to(dt), norm, beta)
        (gcls * lc + gloc * ll).backward()
        ref[dt] = (torch.stack([lc.detach(), ll.detach()]), lg.grad, dl.grad)
    ws = rh.train_workspace(0, 0, S, DEV)
    ld, dd = logits.to(DEV), deltas.to(DEV)
    sd_, lab = slots.to(DEV, torch.int32), labels.to(DEV, torch.int32)
    ad, gd = anc.to(DEV), gts.to(DEV)
    out8 = rh.loss_forward(ld, dd, sd_, lab, ad, gd, norm, ws, beta)
    dlg, ddl = rh.loss_backward(ld, dd, sd_, lab, ad, gd, norm, torch.tensor([gcls], device=DEV), torch.tensor([gloc], device=DEV), beta)
    dlg1, ddl1 = rh.loss_backward(ld, dd, sd_, lab, ad, gd, norm, None, None, beta)
    torch.cuda.synchronize()
    out8, dlg, ddl = out8.cpu(), dlg.cpu(), ddl.cpu()
    assert bool(torch.isfinite(out8).all()) and bool(torch.isfinite(dlg).all()) and bool(torch.isfinite(ddl).all())
    a, f = ref[torch.float64], ref[torch.float32]
    tag = "loss S=%d beta=%g %s" % (S, beta, kind)
    _judge(logdir, tag, {"loss_rpn_cls": (out8[0], a[0][0], f[0][0]), "loss_rpn_loc": (out8[1], a[0][1], f[0][1]),
                         "dlogits": (dlg, a[1], f[1]), "ddeltas": (ddl, a[2], f[2])})
    # NULL gradient scalars mean 1
    _judge(logdir, tag + " unit", {"dlogits": (dlg1.cpu() * gcls, a[1], f[1]), "ddeltas": (ddl1.cpu() * gloc, a[2], f[2])})
    want = np.array(R.rpn_stats(logits, slots, labels), np.float64).astype(np.float32)
    assert np.array_equal(out8[2:6].numpy(), want), (out8, want)
    assert out8[6:].tolist() == [0.0, 0.0]
    # exactly zero outside the row's own columns (and on every delta column of a negative row)
    rows = torch.arange(S)
    lmask = torch.zeros(S, 3, dtype=torch.bool)
    lmask[rows, slots] = True
    dmask = torch.zeros(S, 3, 4, dtype=torch.bool)
    dmask[rows[labels > 0], slots[labels > 0]] = True
    dmask = dmask.reshape(S, 12)
    for grad, mask in ((dlg, lmask), (ddl, dmask), (dlg1.cpu(), lmask), (ddl1.cpu(), dmask)):
        if bool((~mask).any()):
            assert float(grad[~mask].abs().max()) == 0.0
    if kind == "negative":
        assert float(out8[1]) == 0.0


def test_loss_exact_on_lattice():
    """Anchors with power-of-two sides, ground truths that are the anchor moved by eighths of its side (targets k / 8, 0, 0 exactly),
    deltas on a 1/4 grid, logits 0, norm 256: every L1 term is a multiple of 1/8 and their sum is exact in f32, so loss_rpn_loc and
    both gradients equal float64 exactly; loss_rpn_cls is S log(2) / 256, rounded once."""
    rh = _rh()
    S, norm = 257, 256
    g = torch.Generator().manual_seed(4)
    side = 2.0 ** torch.randint(4, 8, (S, 2), generator=g).float()
    xy = torch.randint(0, 64, (S, 2), generator=g).float() * 8
    anc = torch.cat([xy, xy + side], dim=1)
    shift = torch.randint(-4, 5, (S, 2), generator=g).float() * side / 8
    gts = anc + torch.cat([shift, shift], dim=1)
    deltas = torch.randint(-8, 9, (S, 12), generator=g).float() / 4 + 0.0625          # never equal to a target: no |d| = 0
    logits = torch.zeros(S, 3)
    slots = torch.randint(0, 3, (S,), generator=g)
    labels = (torch.rand(S, generator=g) < 0.5).long()
    lg, dl = logits.double().requires_grad_(True), deltas.double().requires_grad_(True)
    lc, ll = R.rpn_losses(lg, dl, slots, labels, anc.double(), gts.double(), norm)
    (lc + ll).backward()
    ws = rh.train_workspace(0, 0, S, DEV)
    args = (logits.to(DEV), deltas.to(DEV), slots.to(DEV, torch.int32), labels.to(DEV, torch.int32), anc.to(DEV), gts.to(DEV), norm)
    out8 = rh.loss_forward(*args, ws).cpu()
    dlg, ddl = rh.loss_backward(*args)
    torch.cuda.synchronize()
    assert float(out8[1].double()) == float(ll.detach())
    assert float(out8[0]) == float(lc.detach().float())
    assert np.array_equal(dlg.cpu().numpy().astype(np.float64), lg.grad.numpy())
    assert np.array_equal(ddl.cpu().numpy().astype(np.float64), dl.grad.numpy())


def test_zero_rows():
    """S = 0 launches nothing and leaves the outputs untouched; RPNHead.forward returns zeros whose gradients reach all six
    parameters."""
    rh = _rh()
    lib = rh._lib.load()
    out = torch.full((8,), 7.0, device=DEV)
    s = rh._lib.stream_ptr()
    assert lib.apse_rpn_loss_forward(None, None, None, None, None, None, 0, 256, 0.0, rh._lib.ptr(out), None, 0, s) == 0
    assert lib.apse_rpn_loss_backward(None, None, None, None, None, None, 0, 256, 0.0, None, None, None, None, s) == 0
    torch.cuda.synchronize()
    assert out.cpu().tolist() == [7.0] * 8
    head = rh.RPNHead(DEV)
    losses = head(torch.zeros(0, 2304, device=DEV), torch.zeros(0), torch.zeros(0), torch.zeros(0, 4), torch.zeros(0, 4), 1)
    assert float(losses["loss_rpn_cls"].detach()) == 0.0 and float(losses["loss_rpn_loc"].detach()) == 0.0
    (losses["loss_rpn_cls"] + losses["loss_rpn_loc"]).backward()
    ps = list(head.parameters())
    assert len(ps) == 6 and all(p.grad is not None and float(p.grad.abs().max()) == 0.0 for p in ps)
    lg, dl = head.predict(torch.zeros(0, 2304, device=DEV))
    assert tuple(lg.shape) == (0, 3) and tuple(dl.shape) == (0, 12)


# ------------------------------------------------------------------------------------------------ whole head
@pytest.mark.parametrize("S", [129, 512])
def test_whole_head_one_step(logdir, S):
    """All six gradients of loss_rpn_cls + loss_rpn_loc on an exact-forward state: f32 and f64 see the same ReLU mask, so the
    comparison is not decided by sign flips at rounding distance from 0."""
    rh = _rh()
    sd = R.exact_forward_state(5)
    x = R.exact_patches(S, 6)
    slots, labels, anc, gts = R.sample_rows(S, 7)
    images = (S + 255) // 256
    norm = 256 * images
    l64, g64 = R.head_step(x, sd, slots, labels, anc, gts, norm, torch.float64)
    l32, g32 = R.head_step(x, sd, slots, labels, anc, gts, norm, torch.float32)
    head = rh.RPNHead(DEV)
    head.load_state_dict(sd)
    losses = head(x.to(DEV), slots, labels, anc, gts, images)
    (losses["loss_rpn_cls"] + losses["loss_rpn_loc"]).backward()
    torch.cuda.synchronize()
    lg, dl = head.predict(x.to(DEV))
    o64 = R.head_outputs(x.double(), {k: v.double() for k, v in sd.items()})
    o32 = R.head_outputs(x, sd)
    outputs = {"loss_rpn_cls": (losses["loss_rpn_cls"], l64[0], l32[0]), "loss_rpn_loc": (losses["loss_rpn_loc"], l64[1], l32[1]),
               "logits": (lg, o64[0], o32[0]), "deltas": (dl, o64[1], o32[1])}
    for k, p in head.named_parameters():
        assert tuple(p.grad.shape) == tuple(p.shape), k
        outputs[k] = (p.grad, g64[k], g32[k])
    _judge(logdir, "whole head S=%d" % S, outputs)
    stats = head.last_stats.cpu()
    assert float(stats[2]) == float((labels > 0).sum()) and float(stats[2] + stats[3]) == S


def _three_steps(S, opt_kind):
    from apse_uav_amd import optim
    rh = _rh()
    g = torch.Generator().manual_seed(S)
    x = torch.relu(torch.randn(S, 2304, generator=g)).to(DEV)
    slots, labels, anc, gts = R.sample_rows(S, S + 1)
    head = rh.RPNHead(DEV)
    head.load_state_dict(R.seeded_state(31))
    params = list(head.parameters())
    opt = (optim.SGD if opt_kind == "apse" else torch.optim.SGD)(params, lr=0.02, momentum=0.9)
    blob = []
    for _ in range(3):
        opt.zero_grad()
        losses = head(x, slots, labels, anc, gts, (S + 255) // 256)
        loss = losses["loss_rpn_cls"] + losses["loss_rpn_loc"]
        loss.backward()
        blob.append(loss.detach().cpu().numpy().tobytes())
        opt.step()
    torch.cuda.synchronize()
    blob += [p.detach().cpu().numpy().tobytes() for p in params]
    return b"".join(blob), float(loss.detach())


@pytest.mark.parametrize("S,opt_kind", [(129, "apse"), (512, "apse"), (129, "torch")])
def test_determinism(S, opt_kind):
    a, la = _three_steps(S, opt_kind)
    b, lb = _three_steps(S, opt_kind)
    assert np.isfinite(la) and a == b


# ------------------------------------------------------------------------------------------------ agreement with inference
def test_agreement_with_inference(predictor, logdir):
    """The training forward at 200 sampled anchors (40 per level) and the same channels of the running detector's rpn_head2 ..
    rpn_head6 tensors, both against float64 computed from the exported p-maps: this pins level, position, slot and channel order.
    p2 / p3 run as Winograd in the detector, so the two are not asked to be the same bits."""
    rh = _rh()
    model = predictor.model
    model.inference_frames(_frames(270, 480))
    torch.cuda.synchronize()
    cols, shapes = _unfolded(model)
    assert shapes == R.level_shapes(252, 448)
    anc, level, ys, xs, slot = R.anchors(shapes)
    g = torch.Generator().manual_seed(11)
    idx, off = [], 0
    for (H, W) in shapes:
        idx.append(off + torch.randperm(3 * H * W, generator=g)[:40])
        off += 3 * H * W
    idx = torch.cat(idx)
    taps = [model.debug_tensor("rpn_head%d" % (l + 2)).reshape(shapes[l][0], shapes[l][1], 16).cpu() for l in range(5)]
    patches, sl, boxes, lv = model.rpn_patches(idx.to(DEV))
    head = rh.RPNHead(DEV)
    head.load_state_dict(model._state)
    logits, deltas = head.predict(patches)
    torch.cuda.synchronize()
    assert lv.cpu().tolist() == level[idx].tolist() and sl.cpu().tolist() == slot[idx].tolist()
    got = R.own_columns(logits.cpu(), deltas.cpu(), slot[idx])
    tap_l = torch.stack([taps[int(level[i])][int(ys[i]), int(xs[i]), int(slot[i])] for i in idx])
    tap_d = torch.stack([taps[int(level[i])][int(ys[i]), int(xs[i]), 3 + 4 * int(slot[i]):7 + 4 * int(slot[i])] for i in idx])
    x32 = torch.stack([cols[int(level[i])][:, int(ys[i]) * shapes[int(level[i])][1] + int(xs[i])] for i in idx])
    sd = {k: v.cpu() for k, v in head.state_dict().items()}
    p64 = R.own_columns(*R.head_outputs(x32.double(), {k: v.double() for k, v in sd.items()}), slot[idx])
    p32 = R.own_columns(*R.head_outputs(x32, sd), slot[idx])
    rows = {}
    for j, (nm, tap) in enumerate((("logits", tap_l), ("deltas", tap_d))):
        for name, (a, b) in {"train_vs_torch": (got[j], p32[j]), "train_vs_inference": (got[j], tap),
                             "inference_vs_torch": (tap, p32[j])}.items():
            eh, ef, bound, ok = R.arbiter(a, p64[j], b)
            rows[nm + " " + name] = {"first": eh, "second": ef, "bound": bound, "ok": ok}
    _log(logdir, "train / inference rpn head n=%d" % idx.numel(), rows)
    for nm in ("logits", "deltas"):
        assert rows[nm + " train_vs_torch"]["ok"] and rows[nm + " train_vs_inference"]["ok"], rows


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_on_the_device(predictor):
    from apse_uav_amd import _lib
    rh = _rh()
    lib = _lib.load()
    t = torch.zeros(4096, device=DEV)
    ti = torch.zeros(4096, dtype=torch.int32, device=DEV)
    p, ip, s = _lib.ptr(t), _lib.ptr(ti), _lib.stream_ptr()
    H5, W5 = (C.c_int * 5)(4, 2, 1, 1, 1), (C.c_int * 5)(4, 2, 1, 1, 1)           # A = 63 anchors
    need = int(lib.apse_rpn_train_workspace_bytes(63, 5, 0))

    def err():
        return lib.apse_last_error(None)
    assert lib.apse_rpn_anchor_labels(C.byref(H5), C.byref(W5), p, 4097, 0.3, 0.7, ip, ip, p, p, 1 << 30, s) == -1
    assert b"apse_rpn_anchor_labels" in err() and b"4096" in err()
    assert lib.apse_rpn_anchor_labels(C.byref(H5), C.byref(W5), p, 5, 0.3, 0.7, ip, ip, p, None, 1 << 20, s) == -1
    assert b"apse_rpn_anchor_labels" in err() and b"workspace" in err()
    assert lib.apse_rpn_anchor_labels(C.byref(H5), C.byref(W5), p, 5, 0.3, 0.7, ip, ip, p, p, 5 * 2 * 4 - 1, s) == -1
    assert b"apse_rpn_anchor_labels" in err() and b"workspace too small" in err()
    assert need >= 5 * 2 * 4
    big = (C.c_int * 5)(2048, 1, 1, 1, 1)
    assert lib.apse_rpn_anchor_labels(C.byref(big), C.byref(big), p, 1, 0.3, 0.7, ip, ip, p, p, 1 << 30, s) == -1 and b"2^22" in err()
    assert lib.apse_rpn_loss_forward(p, p, ip, ip, p, p, 2, 256, 0.0, p, None, 1 << 10, s) == -1 and b"apse_rpn_loss_forward" in err()
    assert lib.apse_rpn_loss_forward(p, p, ip, ip, p, p, 2, 256, 0.0, p, p, 95, s) == -1 and b"workspace too small" in err()
    assert lib.apse_rpn_loss_forward(p, p, ip, ip, p, p, 2, 0, 0.0, p, p, 1 << 10, s) == -1
    assert lib.apse_rpn_loss_backward(p, p, ip, ip, p, p, (1 << 20) + 1, 256, 0.0, None, None, p, p, s) == -1
    assert b"apse_rpn_loss_backward" in err()
    # the gather: a C4 context, and its own limits on an FPN one
    model = predictor.model
    model.backbone_frames(_frames(256, 448))
    assert lib.apse_rpn_patches(model._ctx, 0, ip, (1 << 20) + 1, p, ip, p, ip, s) == -1
    assert b"apse_rpn_patches" in lib.apse_last_error(model._ctx)
    assert lib.apse_rpn_patches(model._ctx, 1, ip, 1, p, ip, p, ip, s) == -1
    c4 = _predictor((256, 448), arch="C4").model
    c4.backbone_frames(_frames(270, 480))
    assert lib.apse_rpn_patches(c4._ctx, 0, ip, 1, p, ip, p, ip, s) == -1
    assert b"apse_rpn_patches" in lib.apse_last_error(c4._ctx) and b"C4" in lib.apse_last_error(c4._ctx)
    torch.cuda.synchronize()
    assert float(t.abs().max()) == 0.0 and int(ti.abs().max()) == 0          # nothing was launched
    with pytest.raises(_lib.ApseError):
        rh.RPNHead(DEV)(torch.zeros(1025, 2304, device=DEV), torch.zeros(1025), torch.zeros(1025), torch.zeros(1025, 4),
                        torch.zeros(1025, 4), 4)
    with pytest.raises(NotImplementedError):
        c4.rpn_patches(np.zeros(1, np.int32))
