"""-m gpu: the mask tail (csrc/mask_tail.hip: det_post, paste_masks, closest_points, driven by apse_mask_tail) stage-exact against
the f64 paste reference (tests/paste_ref.py, pinned to the detectron2 restatement by tests/test_paste_ref.py).

Boxes are given (apse_set_detections), so the test chooses them; the inputs of the paste are then read back from the context:
the mask logits that were pasted (debug tensor ``mask_logits``, f32 NHWC [max_batch * dets_per_image, M, M, ldc], channel =
class) and the packed boxes / classes of the results block.  On exactly those inputs:
  * scaled box bit for bit, ``valid``, ``rect`` and the packed -> record mapping exactly;
  * every window pixel equal to the reference except the reference's ambiguous pixels (f64 value within 2^-20 of the
    threshold: counted, logged and bounded), and no set bit outside [rx0, rx1) in the window's words (so none at x >= W);
  * ``mass`` = popcount, ``centroid`` = floor of the 1-based integer sums (Python integers), or (-1, -1) for an empty mask;
  * every closest point = oracle/mask_utils.compute_closest_point's arithmetic on the mask's bits with the other detection's
    centroid as target ((-1, -1) for an empty mask or target), on the record's sub-matrix of valid detections.
Each case runs five forwards in one context: A, B, C, A, D.  Bit planes alternate per forward and rows outside a window are
never cleared, so the second A lands on the plane B wrote; it must equal the first A byte for byte.  The sets are built so
that every case reaches all three paste bands, more work items than PASTE_BLOCKS, 1, 2 and >= 3 target groups per image and,
at 2160 x 3840, both layouts of closest_points<true> (row range in LDS / in global memory); frames above 4096 px take
closest_points<false>.  The regimes are recomputed from the rects and asserted.  Small synthetic trunk (one bottleneck per stage).
"""
import json
import os
import re
import time

import numpy as np
import pytest
import torch

import paste_ref

pytestmark = pytest.mark.gpu

BLOCKS = (1, 1, 1, 1)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIGS = {
    "fpn_f32_k4": dict(arch="FPN", k=4, dtype="f32", batch=3),
    "fpn_f32_k80": dict(arch="FPN", k=80, dtype="f32", batch=3),
    "fpn_bf16_k4": dict(arch="FPN", k=4, dtype="bf16", batch=3),
    "c4_f32_k4": dict(arch="C4", k=4, dtype="f32", batch=2),           # C4: at most 2 frames per forward
}
CASES = [
    ("fpn_f32_k4", (270, 480)), ("fpn_f32_k4", (1600, 2666)), ("fpn_f32_k4", (2160, 3840)),
    ("fpn_f32_k4", (3648, 5472)), ("fpn_f32_k4", (4608, 2592)),
    ("fpn_f32_k80", (375, 1242)), ("fpn_f32_k80", (2160, 3840)),
    ("fpn_bf16_k4", (375, 1242)), ("fpn_bf16_k4", (2160, 3840)),
    ("c4_f32_k4", (1600, 2666)), ("c4_f32_k4", (2160, 3840)),
]
AMBIG_SHIFT = 14              # ambiguous pixels per case: at most one in 2^14 of the window pixels checked


def _kernel_constants():
    """The launch constants the regimes depend on, read from the kernel source so the test follows them."""
    with open(os.path.join(ROOT, "apse_uav_amd", "csrc", "mask_tail.hip")) as f:
        src = f.read()
    out = {}
    for name in ("PASTE_BLOCKS", "PASTE_BAND_MAX", "PASTE_BAND_MIN", "PASTE_ITEMS_MIN", "CP_PARTS", "CP_ROWS_MIN", "CP_LDS_WORDS"):
        out[name] = int(re.search(r"#define %s (\d+)" % name, src).group(1))
    return out


KC = _kernel_constants()


def _log(logdir, name, obj):
    with open(os.path.join(logdir, "mask_tail.log"), "a") as f:
        f.write(name + " " + json.dumps(obj) + "\n")


@pytest.fixture(scope="module")
def states():
    from apse_uav_amd.weights import synthetic_c4_state, synthetic_detector_state
    return {"fpn4": synthetic_detector_state(0, BLOCKS), "fpn80": synthetic_detector_state(0, BLOCKS, num_classes=80),
            "c4": synthetic_c4_state(0, BLOCKS)}


def _predictor(name, states):
    from apse_uav_amd.config import setup_cfg
    from apse_uav_amd.engines.track_predictor import TrackPredictor
    c = CONFIGS[name]
    cfg = setup_cfg(num_classes=c["k"], arch=c["arch"])
    cfg.APSE.MAX_BATCH = c["batch"]
    cfg.APSE.DTYPE = c["dtype"]
    sd = states["c4"] if c["arch"] == "C4" else states["fpn%d" % c["k"]]
    return TrackPredictor(cfg, state_dict=sd)


# ---------------------------------------------------------------------------------------------------- detection sets
def _small_boxes(rng, n, frame_hw, image_hw, most=120.0):
    """Fractional interior boxes of at most ``most`` frame pixels a side, in network-input pixels."""
    H, W = frame_hw
    sx, sy = W / image_hw[1], H / image_hw[0]
    x0 = rng.uniform(0.0, W - most, n)
    y0 = rng.uniform(0.0, H - most, n)
    s = rng.uniform(0.7, most, (n, 2))
    return np.stack([x0 / sx, y0 / sy, (x0 + s[:, 0]) / sx, (y0 + s[:, 1]) / sy], 1).astype(np.float32)


def _columns(rng, n, frame_hw, image_hw):
    """1-px wide boxes over the full height (in frame pixels) at random columns: many window rows for little work."""
    H, W = frame_hw
    sx, sy = W / image_hw[1], H / image_hw[0]
    x = rng.integers(0, W - 1, n).astype(np.float64) + rng.choice([0.0, 0.5], n)
    return np.stack([x / sx, np.zeros(n), (x + 1.0) / sx, np.full(n, H / sy)], 1).astype(np.float32)


def _invalid(n, image_hw):
    h, w = image_hw
    return np.array([[w + 3.0, 5.0, w + 30.0, 40.0], [10.0, -50.0, 40.0, -3.0], [30.0, 20.0, 30.0, 60.0], [15.0, 25.0, 45.0, 25.0]]
                    * ((n + 3) // 4), np.float32)[:n]


def _classes(rng, n, k):
    return rng.integers(k - 16 if k > 64 else 0, k, n).astype(np.int32)      # K = 80: channels >= 64 of the ldc stride


def _sets(frame_hw, image_hw, k, batch, seed):
    """Detection sets A (edge cases), B (>= 48 000 window rows: band 16), C (few small boxes: band 4, 1 and 2 target groups,
    the frame-sized windows) and D (24 000 .. 48 000 rows: band 8).  Returns name -> (boxes [n, 4], classes [n], counts)."""
    rng = np.random.default_rng(seed)
    H = frame_hw[0]
    edge = paste_ref.edge_boxes(frame_hw, image_hw)
    full = [13, 14]
    rest = np.delete(edge, full, axis=0)
    # A: (17, 0, 100) -- FPN; (0, 100) -- C4.  The 100 interleave invalid boxes between valid ones and hold identical boxes
    # with different classes.
    a0 = rest[:17]
    dup = _small_boxes(rng, 3, frame_hw, image_hw)
    cd = _classes(rng, 3, k)
    cd2 = np.where(cd + 1 < k, cd + 1, k - 2).astype(np.int32)
    good = (list(zip(rest[17:], _classes(rng, len(rest) - 17, k))) + list(zip(dup, cd)) + list(zip(dup, cd2))
            + list(zip(_columns(rng, 12, frame_hw, image_hw), _classes(rng, 12, k))))
    bad = list(zip(_invalid(8, image_hw), _classes(rng, 8, k)))
    pairs = [] if batch >= 3 else list(zip(a0, _classes(rng, 17, k)))
    for j, g in enumerate(good):
        if j and j % 4 == 0 and bad:
            pairs.append(bad.pop())
        pairs.append(g)
    pairs += bad
    nf = 100 - len(pairs)
    a_long = np.concatenate([np.stack([p[0] for p in pairs]), _small_boxes(rng, nf, frame_hw, image_hw)]).astype(np.float32)
    cls_long = np.concatenate([np.array([p[1] for p in pairs], np.int32), _classes(rng, nf, k)])
    if batch >= 3:
        A = (np.concatenate([a0, a_long]), np.concatenate([_classes(rng, 17, k), cls_long]), [17, 0, 100])
    else:
        A = (a_long, cls_long, [0, 100])
    # B: columns until >= 52 000 rows (band 16; more items than PASTE_BLOCKS), two or three images of >= 17
    nb = min(100 * batch, -(-52000 // H))
    nb = max(nb, 17 * batch)
    bb = _columns(rng, nb, frame_hw, image_hw)
    cnt_b = [nb // batch + (1 if j < nb % batch else 0) for j in range(batch)]
    B = (bb, _classes(rng, nb, k), cnt_b)
    # C: 5 and 12 boxes (1 and 2 target groups), the two frame-sized windows among them
    cb = np.concatenate([edge[full], _small_boxes(rng, 15, frame_hw, image_hw)])
    C = (cb, _classes(rng, 17, k), [5, 12] + [0] * (batch - 2))
    # D: columns of a height that gives 24 000 .. 48 000 rows (band 8)
    hd = min(H, 600)
    nd_ = min(100 * batch, -(-36000 // hd))
    dd = _columns(rng, nd_, frame_hw, image_hw)
    dd[:, 3] = dd[:, 1] + np.float32(hd * image_hw[0] / H)
    cnt_d = [nd_ // batch + (1 if j < nd_ % batch else 0) for j in range(batch)]
    D = (dd, _classes(rng, nd_, k), cnt_d)
    return dict(A=A, B=B, C=C, D=D)


# ---------------------------------------------------------------------------------------------------- checks
def _unpack(bits):
    """int64 [rows, nw] words -> bool [rows, nw * 64] (bit j of word w = column 64 w + j)."""
    a = np.ascontiguousarray(bits).view(np.uint8).reshape(bits.shape[0], -1)
    return np.unpackbits(a, axis=1, bitorder="little").astype(bool)


def _closest(ys, xs, targets):
    """compute_closest_point's arithmetic (1-based f32 coordinates, f32 squared distance, first row-major argmin) for many targets
    of one mask given by its pixels in row-major order."""
    fx = (xs + 1).astype(np.float32)
    fy = (ys + 1).astype(np.float32)
    out = []
    step = max(1, (1 << 23) // max(1, len(xs)))
    for s in range(0, len(targets), step):
        t = np.asarray(targets[s:s + step], np.float32)
        dx = fx[None, :] - t[:, 0:1]
        dy = fy[None, :] - t[:, 1:2]
        d = dx * dx + dy * dy
        i = np.argmin(d, axis=1)
        out += [(float(fx[v]), float(fy[v])) for v in i]
    return out


def _regimes(res, frame_hw, batch):
    """Which launch regimes the forward's rects select (csrc/mask_tail.hip: mt_pick_band, the item count, closest_points)."""
    H, W = frame_hw
    n = res.total
    rect = res.rect[:n].astype(np.int64)
    rows = np.where(res.valid[:n] != 0, rect[:, 3] - rect[:, 1], 0)
    tot = int(rows.sum())
    band = KC["PASTE_BAND_MAX"]
    while band > KC["PASTE_BAND_MIN"] and tot // band < KC["PASTE_ITEMS_MIN"]:
        band //= 2
    items = int(((rows + band - 1) // band).sum())
    layouts = set()
    wordwise = H <= 4096 and W <= 4096
    for i in range(n):
        r = int(rows[i])
        if r <= 0:
            continue
        if not wordwise:
            layouts.add("every_pixel")
            continue
        P = min(max(1, -(-r // KC["CP_ROWS_MIN"])), KC["CP_PARTS"])
        rpp = -(-r // P)
        nw = ((rect[i, 2] + 63) >> 6) - (rect[i, 0] >> 6)
        for p in range(P):
            pr = min(rpp, r - p * rpp)
            if pr > 0:
                layouts.add("lds" if pr * nw <= KC["CP_LDS_WORDS"] else "global")
    groups = set()
    for b in range(batch):
        nt = int(res.offset[b + 1] - res.offset[b])
        if nt:
            groups.add(min(3, -(-nt // 8)))
    return dict(rows=tot, band=band, items=items, layouts=sorted(layouts), groups=sorted(groups))


def _check_forward(model, res, insts, given, frame_hw, image_hw, M, k):
    """Every check of the module docstring on one forward; returns (stats, the forward's bytes)."""
    H, W = frame_hw
    boxes, classes, counts = given
    batch = len(insts)
    n = res.total
    assert n == sum(counts)
    assert list(res.offset[:batch + 1]) == list(np.concatenate([[0], np.cumsum(counts)]))
    KD = res.lay.dets_per_image
    lg = model.debug_tensor("mask_logits").cpu().numpy()
    assert lg.size % (res.lay.max_batch * KD * M * M) == 0
    ldc = lg.size // (res.lay.max_batch * KD * M * M)
    assert lg.size == res.lay.max_batch * KD * M * M * ldc and ldc >= k
    lg = lg.reshape(res.lay.max_batch * KD, M, M, ldc)
    # packed inputs == the given list, in order
    assert np.array_equal(res.box_resized[:n].view(np.uint32), np.asarray(boxes, np.float32).view(np.uint32))
    assert np.array_equal(res.cls[:n], classes)
    assert np.array_equal(res.img[:n], np.repeat(np.arange(batch), counts))
    refs = [paste_ref.paste(lg[i, :, :, res.cls[i]], res.box_resized[i], frame_hw, image_hw) for i in range(n)]
    assert np.array_equal(res.box[:n].view(np.uint32), np.stack([r["box"] for r in refs]).view(np.uint32))
    assert np.array_equal(res.valid[:n] != 0, np.array([r["valid"] for r in refs]))
    st = dict(ambiguous=0, ambiguous_differ=0, pixels=0, on=0, empty=0, invalid=int(n - (res.valid[:n] != 0).sum()), closest=0)
    blob = [res.box[:n].tobytes(), res.valid[:n].tobytes(), res.rect[:n].tobytes()]
    for i in range(n):
        if refs[i]["valid"]:
            assert tuple(int(v) for v in res.rect[i]) == refs[i]["rect"], (i, res.rect[i], refs[i]["rect"])
        else:
            assert res.rect[i][2] == res.rect[i][0] and res.rect[i][3] == res.rect[i][1], i
    for b in range(batch):
        lo, hi = res.image_slice(b)
        rec = res.record(b)
        keep = [i for i in range(lo, hi) if refs[i]["valid"]]
        assert list(rec["packed_index"]) == keep
        inst = insts[b]
        assert len(inst) == len(keep)
        pix, cents = [], []
        for kk, i in enumerate(keep):
            r = refs[i]
            x0, y0, x1, y1 = r["rect"]
            m = inst.pred_masks[kk]
            assert m.rect == r["rect"]
            words = m.bits.cpu().numpy()
            blob.append(words.tobytes())
            px = _unpack(words)
            base = (x0 >> 6) << 6
            assert px.shape == (y1 - y0, (((x1 + 63) >> 6) - (x0 >> 6)) * 64)
            cols = base + np.arange(px.shape[1])
            assert not px[:, (cols < x0) | (cols >= x1)].any(), i          # includes every column >= W
            win = px[:, x0 - base:x1 - base]
            d = win != r["mask"]
            assert not (d & ~r["ambiguous"]).any(), (i, int((d & ~r["ambiguous"]).sum()), r["rect"])
            st["ambiguous"] += int(r["ambiguous"].sum())
            st["ambiguous_differ"] += int(d.sum())
            st["pixels"] += win.size
            ys, xs = np.nonzero(win)
            ys, xs = ys + y0, xs + x0
            mass = len(xs)
            st["on"] += mass
            assert int(rec["mass"][kk]) == mass == m.mass, i
            c = (int(np.sum(xs + 1, dtype=np.int64)) // mass, int(np.sum(ys + 1, dtype=np.int64)) // mass) if mass else (-1, -1)
            assert tuple(int(v) for v in rec["centroids"][kk]) == c, (i, rec["centroids"][kk], c)
            st["empty"] += int(mass == 0)
            pix.append((ys, xs))
            cents.append(c)
        nk = len(keep)
        assert rec["closest"].shape == (nk, nk, 2)
        for kk in range(nk):
            ys, xs = pix[kk]
            live = [j for j in range(nk) if cents[j][0] >= 0]
            want = {j: (-1.0, -1.0) for j in range(nk)}
            if len(xs):
                for j, p in zip(live, _closest(ys, xs, [cents[j] for j in live])):
                    want[j] = p
            got = {j: tuple(float(v) for v in rec["closest"][kk][j]) for j in range(nk)}
            assert got == want, (b, kk, [(j, got[j], want[j]) for j in range(nk) if got[j] != want[j]][:4])
            st["closest"] += len(live) if len(xs) else 0
        blob.append(np.ascontiguousarray(rec["closest"]).tobytes() + rec["mass"].tobytes() + rec["centroids"].tobytes())
    # the batched closest-point helper against oracle/mask_utils itself on a dense mask
    from oracle import mask_utils as omu
    for b in range(batch):
        inst = insts[b]
        rec = res.record(b)
        if len(inst) and inst.pred_masks[0].mass and rec["centroids"][-1][0] >= 0:
            dense = inst.pred_masks[0].dense().cpu().numpy()
            t = (float(rec["centroids"][-1][0]), float(rec["centroids"][-1][1]))
            assert omu.compute_closest_point(dense, t) == tuple(float(v) for v in rec["closest"][0][len(inst) - 1])
            break
    return st, b"".join(bytes(x) for x in blob)


@pytest.mark.parametrize("case", CASES, ids=["%s-%dx%d" % (c[0], c[1][0], c[1][1]) for c in CASES])
def test_mask_tail_stage_exact(states, logdir, case):
    from apse_uav_amd.synthetic import SyntheticSequence
    from apse_uav_amd.utils import resample
    name, frame_hw = case
    c = CONFIGS[name]
    t0 = time.time()
    pr = _predictor(name, states)
    model = pr.model
    H, W = frame_hw
    image_hw = resample.resize_shortest_edge(H, W, pr.cfg.INPUT.MIN_SIZE_TEST, pr.cfg.INPUT.MAX_SIZE_TEST)
    M = 14 if c["arch"] == "C4" else 28
    seq = SyntheticSequence("dynamic", H, W)
    frames = torch.from_numpy(np.stack([seq.frame(3 * t) for t in range(c["batch"])])).cuda()
    sets = _sets(frame_hw, image_hw, c["k"], c["batch"], seed=H * 13 + W + c["k"])
    stats, regimes, blobs = [], [], {}
    for step, key in enumerate("ABCAD"):
        boxes, classes, counts = sets[key]
        insts, _ = model.inference_frames(frames, given=(boxes, classes, np.asarray(counts, np.int32)))
        res = model.last_results
        rg = _regimes(res, frame_hw, c["batch"])
        st, blob = _check_forward(model, res, insts, (boxes, classes, counts), frame_hw, image_hw, M, c["k"])
        if key == "A":
            blobs.setdefault(key, []).append(blob)
        stats.append(st)
        regimes.append(rg)
    assert blobs["A"][0] == blobs["A"][1]                    # the second A ran on the plane B left behind
    amb = sum(s["ambiguous"] for s in stats)
    info = dict(ambiguous=amb, ambiguous_decided_differently=sum(s["ambiguous_differ"] for s in stats),
                pixels=sum(s["pixels"] for s in stats), on=sum(s["on"] for s in stats), empty_masks=sum(s["empty"] for s in stats),
                invalid=sum(s["invalid"] for s in stats), closest_checked=sum(s["closest"] for s in stats),
                bands=sorted({r["band"] for r in regimes}), max_items=max(r["items"] for r in regimes),
                layouts=sorted(set().union(*[r["layouts"] for r in regimes])), groups=sorted(set().union(*[r["groups"] for r in regimes])),
                per_forward=[dict(set=k, rows=r["rows"], band=r["band"], items=r["items"]) for k, r in zip("ABCAD", regimes)],
                image=list(image_hw), wall_s=round(time.time() - t0, 1))
    _log(logdir, "%s/%dx%d" % (name, H, W), info)
    assert amb <= info["pixels"] >> AMBIG_SHIFT, (amb, info["pixels"])
    assert 0 < info["on"] < info["pixels"]
    assert info["bands"] == [4, 8, 16], info["per_forward"]
    assert info["max_items"] > KC["PASTE_BLOCKS"]
    assert info["groups"] == [1, 2, 3]
    if H > 4096 or W > 4096:
        assert info["layouts"] == ["every_pixel"]
    elif frame_hw == (2160, 3840):
        assert info["layouts"] == ["global", "lds"]
    else:
        assert "lds" in info["layouts"]


def test_every_configuration_covered():
    """Each configuration runs at two sizes or more, one of them 2160 x 3840 (both closest-point layouts); the frames above
    4096 px run in f32 FPN."""
    for name in CONFIGS:
        sizes = [hw for n, hw in CASES if n == name]
        assert len(sizes) >= 2 and (2160, 3840) in sizes, name
    big = [n for n, hw in CASES if max(hw) > 4096]
    assert {(3648, 5472), (4608, 2592)} <= {hw for n, hw in CASES if n == "fpn_f32_k4"} and big
