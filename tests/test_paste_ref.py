"""CPU (-m "not gpu"): tests/paste_ref.py (the f64 paste reference of test_gpu_mask_tail.py) against the detectron2 restatement,
oracle.detector.DetectorOracle.postprocess (Boxes.scale / clip / nonempty, then oracle.ops.paste_mask per kept box).

Random logit maps (M = 28 and 14) on the edge-case boxes of paste_ref.edge_boxes plus random fractional boxes, at the frame sizes
of the GPU test.  Scaled boxes equal bit for bit, the kept set and the windows equal, and the masks equal outside the reference's
ambiguous pixels.  The oracle's sigmoid and blend are f32, so this also bounds how far an f32 paste lands from the f64 value: a
pixel the two decide differently must lie inside the 2^-20 band.
"""
import numpy as np
import pytest
import torch

import paste_ref

CASES = [  # (frame (H, W), network input (h, w), M)
    ((270, 480), (252, 448), 28),
    ((375, 1242), (402, 1333), 28),
    ((1600, 2666), (800, 1333), 28),
    ((1600, 2666), (800, 1333), 14),
    ((2160, 3840), (750, 1333), 14),
    ((3648, 5472), (800, 1200), 28),
    ((4608, 2592), (1333, 750), 28),
]


def _oracle_post(boxes, probs, image_hw, frame_hw):
    from oracle.detector import DetectorOracle
    n = boxes.shape[0]
    o = DetectorOracle({}, dict(mask_thresh=0.5))
    return o.postprocess(torch.from_numpy(boxes), torch.ones(n), torch.zeros(n, dtype=torch.int64), probs, image_hw, *frame_hw)


def _random_boxes(rng, n, image_hw, big):
    h, w = image_hw
    x0 = rng.uniform(-0.05 * w, w, n)
    y0 = rng.uniform(-0.05 * h, h, n)
    side = rng.uniform(0.2, 60.0 if not big else 0.3 * min(h, w), (n, 2))
    return np.stack([x0, y0, x0 + side[:, 0], y0 + side[:, 1]], 1).astype(np.float32)


@pytest.mark.parametrize("case", CASES, ids=["%dx%d_M%d" % (c[0][0], c[0][1], c[2]) for c in CASES])
def test_paste_reference_equals_oracle(case):
    from apse_uav_amd.utils import resample
    frame_hw, image_hw, M = case
    assert resample.resize_shortest_edge(frame_hw[0], frame_hw[1], 800, 1333) == image_hw or frame_hw == (270, 480)
    rng = np.random.default_rng(frame_hw[0] * 7 + frame_hw[1] + M)
    large = frame_hw[0] * frame_hw[1] > 4e6
    edge = paste_ref.edge_boxes(frame_hw, image_hw)
    if large:                      # at most two frame-sized windows per case (the oracle's grid_sample is not cheap there)
        keep = [k for k, b in enumerate(edge) if (b[2] - b[0]) * (b[3] - b[1]) < 0.5 * image_hw[0] * image_hw[1]]
        edge = np.concatenate([edge[keep], edge[[13]]])
    boxes = np.concatenate([edge, _random_boxes(rng, 30, image_hw, False), _random_boxes(rng, 4 if large else 10, image_hw, True)])
    n = boxes.shape[0]
    # logits: smooth blobs plus noise, so windows hold both decisions and long threshold crossings
    yy, xx = np.mgrid[0:M, 0:M] / (M - 1.0)
    cx, cy, r = rng.uniform(0.2, 0.8, (3, n, 1, 1))
    logits = (4.0 * (0.35 - np.hypot(xx - cx, yy - cy) * r * 3) + rng.normal(0, 1.0, (n, M, M))).astype(np.float32)
    probs = torch.sigmoid(torch.from_numpy(logits))
    post = _oracle_post(boxes, probs, image_hw, frame_hw)
    refs = [paste_ref.paste(logits[k], boxes[k], frame_hw, image_hw) for k in range(n)]
    keep = np.nonzero([r["valid"] for r in refs])[0]
    assert np.array_equal(post["keep"].numpy(), np.array([r["valid"] for r in refs]))
    assert len(keep) < n                                   # the edge list holds invalid boxes
    assert np.array_equal(post["boxes"].numpy().view(np.uint32), np.stack([refs[k]["box"] for k in keep]).view(np.uint32))
    ambig = differ = px = on = 0
    for j, k in enumerate(keep):
        r = refs[k]
        assert tuple(post["mask_rects"][j]) == r["rect"], k
        got = post["mask_windows"][j].numpy()
        assert got.shape == r["mask"].shape
        d = got != r["mask"]
        assert not (d & ~r["ambiguous"]).any(), (k, int((d & ~r["ambiguous"]).sum()))
        ambig += int(r["ambiguous"].sum())
        differ += int(d.sum())
        px += got.size
        on += int(got.sum())
    print("pixels %d on %d ambiguous %d decided differently %d" % (px, on, ambig, differ))
    assert 0 < on < px                                      # both decisions occur
    assert ambig <= max(8, px // 100000), (ambig, px)       # the band is narrow: a handful of pixels per case


def test_paste_reference_detects_a_shift():
    """The comparison above has teeth: a reference whose grid moves by 1/64 px disagrees with the oracle outside the band."""
    frame_hw, image_hw, M = (1600, 2666), (800, 1333), 28
    rng = np.random.default_rng(5)
    logits = rng.normal(0, 3.0, (M, M)).astype(np.float32)
    box = np.array([100.25, 80.5, 400.75, 350.125], np.float32)
    post = _oracle_post(box[None], torch.sigmoid(torch.from_numpy(logits))[None], image_hw, frame_hw)
    good = paste_ref.paste(logits, box, frame_hw, image_hw)
    assert not ((post["mask_windows"][0].numpy() != good["mask"]) & ~good["ambiguous"]).any()
    orig = paste_ref.grid_index
    try:
        paste_ref.grid_index = lambda c, lo, hi, m: orig(np.asarray(c) + 1.0 / 64, lo, hi, m)
        bad = paste_ref.paste(logits, box, frame_hw, image_hw)
    finally:
        paste_ref.grid_index = orig
    assert ((post["mask_windows"][0].numpy() != bad["mask"]) & ~bad["ambiguous"]).any()
