"""Training augmentation on the GPU (csrc/augment.hip, utils/augment.py, the context cache of TrackRCNN, MaskTrainLoader's
device path, tools/finetune_segmentation.py --augment): every uint8 against the numpy oracle tests/augment_ref.py, exactly."""
import ctypes as C
import itertools
import os
import sys

import numpy as np
import pytest
import torch

import augment_ref as A

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tools"))
DEV = "cuda:0"

# widths not divisible by 4, rows shorter than a run of 4 pixels, one row, several blocks per image with a ragged end
SHAPES = [(1, 1), (1, 256), (3, 5), (37, 61), (64, 256), (130, 517)]
CONTENTS = ["random", "const0", "const1", "const77", "const128", "const200", "const255", "half_grey", "ramp"]


def _content(kind, h, w, seed):
    g = np.random.default_rng(seed)
    if kind == "random":
        return g.integers(0, 256, (h, w, 3), dtype=np.uint8)
    if kind.startswith("const"):
        return np.full((h, w, 3), int(kind[5:]), np.uint8)
    if kind == "half_grey":
        img = g.integers(0, 256, (h, w, 3), dtype=np.uint8)
        img[:, :w // 2] = int(g.integers(0, 256))
        return img
    ramp = (np.arange(w)[None, :] + np.arange(h)[:, None]) % 256           # "ramp": grey, every level at 1 x 256
    return np.repeat(ramp.astype(np.uint8)[:, :, None], 3, axis=2)


def _param_sets():
    """(wb, ws, wc, lw): seeded draws, the 27 corners, lighting all negative / all positive, the identity."""
    from apse_uav_amd.utils import augment
    g = np.random.default_rng(11)
    sets = []
    for _ in range(3):
        p = augment.draw_params(g, False, True)
        sets.append((p.brightness, p.saturation, p.contrast, tuple(p.lighting.tolist())))
    for wb, ws, wc in itertools.product((0.9, 1.0, 1.1), repeat=3):
        sets.append((wb, ws, wc, (0.0, 0.0, 0.0)))
    sets.append((1.0, 1.0, 1.0, (-0.3, -0.2, -0.25)))
    sets.append((1.03, 0.97, 1.02, (0.3, 0.2, 0.25)))
    sets.append((1.0, 1.0, 1.0, (0.0, 0.0, 0.0)))
    return sets


def _run(imgs, flips, sets):
    """imgs: list of uint8 [h][w][3]; one flip and one parameter set per image -> (u8, chw, sums) as numpy / python ints."""
    from apse_uav_amd.utils import augment
    src = torch.from_numpy(np.stack(imgs)).to(DEV)
    params = [augment.AugmentParams(f, s[0], s[1], s[2], s[3]) for f, s in zip(flips, sets)]
    u8, chw, sums = augment.augment_images(src, params)
    torch.cuda.synchronize()
    assert torch.equal(src.cpu(), torch.from_numpy(np.stack(imgs)))           # the source is read, never written
    return u8.cpu().numpy(), chw.cpu().numpy(), [int(v) & (2 ** 64 - 1) for v in sums.cpu().tolist()]


def _check(imgs, flips, sets):
    u8, chw, sums = _run(imgs, flips, sets)
    for k, (img, f, s) in enumerate(zip(imgs, flips, sets)):
        want, S = A.augment(img, f, s[0], s[1], s[2], s[3])
        bad = np.argwhere(u8[k] != want)
        assert bad.size == 0, (img.shape, f, s, len(bad), bad[:4].tolist(), u8[k][tuple(bad[0])], want[tuple(bad[0])])
        assert chw[k].dtype == np.float32 and np.array_equal(chw[k], want.transpose(2, 0, 1).astype(np.float32)), (img.shape, f, s)
        assert sums[k] == S, (img.shape, f, s, sums[k], S)
        if s == (1.0, 1.0, 1.0, (0.0, 0.0, 0.0)):
            assert np.array_equal(u8[k], img[:, ::-1] if f else img)          # all-identity: the input, mirrored when flipped


@pytest.mark.parametrize("content", CONTENTS)
@pytest.mark.parametrize("hw", SHAPES, ids=["%dx%d" % s for s in SHAPES])
def test_kernel_equals_oracle(hw, content):
    h, w = hw
    sets = _param_sets()
    assert len(sets) == 33
    for flip in (False, True):
        # B = 3: three images (different bytes where the content is random), a different parameter set each
        for i in range(0, len(sets), 3):
            imgs = [_content(content, h, w, seed=100 + i + k) for k in range(3)]
            _check(imgs, [flip] * 3, sets[i:i + 3])
        # B = 1: a seeded draw, a corner, both lighting signs, the identity
        for s in (sets[0], sets[5], sets[-3], sets[-2], sets[-1]):
            _check([_content(content, h, w, seed=7)], [flip], [s])
    # one batch with both flip states in it
    imgs = [_content(content, h, w, seed=3 + k) for k in range(3)]
    _check(imgs, [True, False, True], [sets[1], sets[2], sets[3]])


def test_sum_above_32_bits():
    """2400 x 2400 of 255: S = 4 406 400 000 > 2^32 catches a 32-bit accumulator; the mean stays 255.0."""
    img = np.full((2400, 2400, 3), 255, np.uint8)
    s = (1.0, 1.0, 1.1, (0.1, -0.1, 0.1))
    u8, chw, sums = _run([img], [False], [s])
    want, S = A.augment(img, False, *s)
    assert S == 4406400000 and sums[0] == S
    assert np.array_equal(u8[0], want)
    assert np.array_equal(chw[0], want.transpose(2, 0, 1).astype(np.float32))


def test_refused_arguments():
    """Each refused combination returns APSE_E_INVALID with a text and launches nothing (the outputs keep their fill)."""
    from apse_uav_amd import _lib
    from apse_uav_amd.utils import augment
    lib = _lib.load()
    B, h, w = 2, 6, 10
    src = torch.full((B, h, w, 3), 9, dtype=torch.uint8, device=DEV)
    out = torch.full((B, h, w, 3), 201, dtype=torch.uint8, device=DEV)
    chw = torch.full((B, 3, h, w), -7.0, device=DEV)
    sums = torch.full((B,), 12345, dtype=torch.int64, device=DEV)
    big = torch.full((2 * B * h * w * 3,), 9, dtype=torch.uint8, device=DEV)
    cp = (augment._CParams * augment.MAX_BATCH)()
    for k in range(augment.MAX_BATCH):
        cp[k].brightness = cp[k].saturation = cp[k].contrast = 1.1
    p = _lib.ptr

    def call(s_, B_, h_, w_, cp_, o_, c_, m_):
        return lib.apse_augment_u8(s_, B_, h_, w_, cp_, o_, c_, m_, _lib.stream_ptr())

    cases = {
        "H = 0": (p(src), B, 0, w, cp, p(out), p(chw), p(sums)),
        "W = 0": (p(src), B, h, 0, cp, p(out), p(chw), p(sums)),
        "H above the bound": (p(src), 1, 32769, 1, cp, p(out), p(chw), p(sums)),
        "W above the bound": (p(src), 1, 1, 49153, cp, p(out), p(chw), p(sums)),
        "B = 0": (p(src), 0, h, w, cp, p(out), p(chw), p(sums)),
        "B above the bound": (p(src), augment.MAX_BATCH + 1, h, w, cp, p(out), p(chw), p(sums)),
        "src NULL": (None, B, h, w, cp, p(out), p(chw), p(sums)),
        "sums NULL": (p(src), B, h, w, cp, p(out), p(chw), None),
        "params NULL": (p(src), B, h, w, None, p(out), p(chw), p(sums)),
        "both outputs NULL": (p(src), B, h, w, cp, None, None, p(sums)),
        "out_u8 == src": (p(src), B, h, w, cp, p(src), p(chw), p(sums)),
        "out_u8 overlaps the end of src": (C.c_void_p(big.data_ptr()), B, h, w, cp, C.c_void_p(big.data_ptr() + B * h * w * 3 - 1),
                                           p(chw), p(sums)),
        "out_u8 overlaps the start of src": (C.c_void_p(big.data_ptr() + 5), B, h, w, cp, C.c_void_p(big.data_ptr()), p(chw), p(sums)),
    }
    for name, args in cases.items():
        assert call(*args) == -1, name
        assert b"apse_augment_u8" in lib.apse_last_error(None), name
    torch.cuda.synchronize()
    assert bool((src == 9).all()) and bool((out == 201).all()) and bool((chw == -7.0).all()) and bool((sums == 12345).all())
    assert bool((big == 9).all())
    # adjacent, not overlapping, is accepted; so is either output alone
    assert call(C.c_void_p(big.data_ptr()), B, h, w, cp, C.c_void_p(big.data_ptr() + B * h * w * 3), None, p(sums)) == 0
    assert call(p(src), B, h, w, cp, None, p(chw), p(sums)) == 0
    torch.cuda.synchronize()
    assert bool((chw != -7.0).all())
    with pytest.raises(ValueError):
        augment.augment_images(src.float(), augment.AugmentParams())


# ------------------------------------------------------------------------------------------------ model, loader, tool
K = 4
FRAME_HW = (240, 320)


@pytest.fixture(scope="module")
def predictor():
    from apse_uav_amd.config import setup_cfg
    from apse_uav_amd.engines.track_predictor import TrackPredictor
    from apse_uav_amd.weights import synthetic_detector_state
    cfg = setup_cfg(num_classes=K)
    cfg.APSE.MAX_BATCH = 1
    cfg.INPUT.MIN_SIZE_TEST, cfg.INPUT.MAX_SIZE_TEST = 256, 448
    return TrackPredictor(cfg, state_dict=synthetic_detector_state(0, (1, 1, 1, 1), num_classes=K))


def _frame(i=0, hw=FRAME_HW):
    from apse_uav_amd.synthetic import SyntheticSequence
    return SyntheticSequence("dynamic", *hw).frame(i)


BOXES = np.array([[10.0, 12.0, 90.0, 70.0], [100.5, 40.25, 180.0, 160.0], [0.0, 0.0, 255.0, 191.0], [200.0, 100.0, 230.0, 130.0]],
                 np.float32)


def test_path_equivalence(predictor):
    """Identity parameters at the test size, no flip: resize_frames -> augment_images -> preprocess_images -> backbone gives the
    RoI features of backbone_frames, bit for bit."""
    from apse_uav_amd.utils import augment, resample
    model = predictor.model
    frame = torch.from_numpy(_frame()[None]).to(DEV)
    model.backbone_frames(frame)
    want = model.mask_roi_features(BOXES).clone()
    ih, iw = resample.resize_shortest_edge(FRAME_HW[0], FRAME_HW[1], 256, 448)
    resized = augment.resize_frames(frame, ih, iw)
    u8, chw, _ = augment.augment_images(resized, augment.AugmentParams())
    assert torch.equal(u8, resized)
    model.backbone_images(chw, FRAME_HW)
    got = model.mask_roi_features(BOXES)
    assert want.abs().max() > 0 and torch.equal(got, want)


def _dataset(root, n):
    """n synthetic images of ONE frame size with polygon ground truth -> dataset dictionaries."""
    import json
    from PIL import Image
    from apse_uav_amd.utils import COCO_utils
    H, W = FRAME_HW
    g = np.random.default_rng(2)
    os.makedirs(root, exist_ok=True)
    images, anns = [], []
    for i in range(n):
        name = "%03d.png" % i
        Image.fromarray(_frame(i)[:, :, ::-1].copy()).save(os.path.join(root, name))
        images.append(dict(id=i + 1, file_name=name, height=H, width=W))
        for _ in range(int(g.integers(1, 4))):
            bw, bh = float(g.integers(12, W // 3)), float(g.integers(12, H // 3))
            x, y = float(g.integers(0, W - int(bw))), float(g.integers(0, H - int(bh)))
            anns.append(dict(id=len(anns) + 1, image_id=i + 1, category_id=int(g.integers(0, K)), bbox=[x, y, bw, bh], area=bw * bh,
                             iscrowd=0, segmentation=[[x, y, x + bw, y + bh / 3, x + bw / 2, y + bh, x, y + bh / 2]]))
    path = os.path.join(root, "annotations.json")
    with open(path, "w") as fh:
        json.dump(dict(images=images, annotations=anns, categories=[dict(id=c, name="c%d" % c) for c in range(K)]), fh)
    return COCO_utils.generate_coco_dataset_dictionaries(path, root)


def test_loader_equals_cpu_made_images(predictor, tmp_path):
    """8 draws of an augmenting multi-scale loader: the features equal those of the CPU-made image (the numpy restatement of the
    Pillow resize, then the oracle, with parameters drawn from a generator in the same state) fed through preprocess_images;
    classes and targets equal those of transform_annotations' output."""
    from PIL import Image
    from apse_uav_amd.utils import COCO_utils, augment, resample
    model = predictor.model
    dicts = _dataset(str(tmp_path / "img"), 4)
    sizes = (224, 256, 288)
    loader = COCO_utils.MaskTrainLoader(dicts, model, ims_per_batch=1, seed=21, flip=True, cache_features=True, augment=True,
                                        min_sizes=sizes)
    assert loader.cache is None and int(model.cfg.APSE.CONTEXT_CACHE) >= 3
    rng = np.random.default_rng(21)
    order, seen, flips = [], set(), 0
    H, W = FRAME_HW
    for _ in range(8):
        feats, classes, targets = next(loader)
        feats, targets = feats.clone(), targets.clone()
        if not order:
            order = [int(i) for i in rng.permutation(len(dicts))]
        d = dicts[order.pop(0)]
        size = augment.draw_size(rng, sizes, "choice")
        p = augment.draw_params(rng, True, True)
        seen.add(size)
        flips += p.flip
        ih, iw = resample.resize_shortest_edge(H, W, size, loader.max_size)
        frame = np.asarray(Image.open(d["file_name"]).convert("RGB"))[:, :, ::-1].copy()
        img, _ = A.augment(resample.resize_reference_numpy(frame, ih, iw), p.flip, p.brightness, p.saturation, p.contrast, p.lighting)
        boxes = np.array([[a["bbox"][0], a["bbox"][1], a["bbox"][0] + a["bbox"][2], a["bbox"][1] + a["bbox"][3]]
                          for a in d["annotations"]], np.float64)
        boxes, polys = augment.transform_annotations(boxes, [a["segmentation"] for a in d["annotations"]], (H, W), (ih, iw), p.flip)
        model.backbone_images(torch.from_numpy(img.transpose(2, 0, 1).astype(np.float32)[None]).to(DEV), (H, W))
        want = model.mask_roi_features(boxes.astype(np.float32))
        assert torch.equal(feats, want), (size, p)
        assert classes.tolist() == [a["category_id"] for a in d["annotations"]]
        assert torch.equal(targets, COCO_utils.mask_targets(polys, boxes, model.device))
        assert int(targets.sum()) > 0
    assert rng.bit_generator.state == loader.rng.bit_generator.state
    assert len(seen) > 1 and 0 < flips < 8                     # the 8 draws did exercise several sizes and both flip states


def test_loader_options_off_keep_the_draws(predictor, tmp_path):
    """augment false and min_sizes None: the host path, with the draws of before (order, then one flip draw per image)."""
    from apse_uav_amd.utils import COCO_utils
    dicts = _dataset(str(tmp_path / "img"), 3)
    loader = COCO_utils.MaskTrainLoader(dicts, predictor.model, ims_per_batch=2, seed=4, flip=True)
    assert not loader.device_path
    rng = np.random.default_rng(4)
    order = []
    for _ in range(3):
        feats, classes, targets = next(loader)
        want = []
        for _ in range(2):
            if not order:
                order = [int(i) for i in rng.permutation(len(dicts))]
            d = dicts[order.pop(0)]
            want.append(loader.image_item(d, bool(rng.random() < 0.5)))
        assert torch.equal(feats, torch.cat([w[0] for w in want])) and torch.equal(targets, torch.cat([w[2] for w in want]))
    assert rng.bit_generator.state == loader.rng.bit_generator.state


def _model(cache):
    from apse_uav_amd.config import setup_cfg
    from apse_uav_amd.networks.track_rcnn import TrackRCNN
    from apse_uav_amd.weights import synthetic_detector_state
    cfg = setup_cfg(num_classes=K)
    cfg.APSE.MAX_BATCH = 1
    if cache is not None:
        cfg.APSE.CONTEXT_CACHE = cache
    m = TrackRCNN(cfg)
    m.load_state_dict(synthetic_detector_state(0, (1, 1, 1, 1), num_classes=K))
    return m


def _visit(model, hw, seed):
    img = torch.from_numpy(np.random.default_rng(seed).integers(0, 256, (1, 3) + hw).astype(np.float32)).to(DEV)
    model.backbone_images(img, FRAME_HW)
    boxes = BOXES * np.float32(hw[0] / 192.0)
    return model.mask_roi_features(boxes).clone()


def test_context_cache():
    Asz, Bsz, Csz = (192, 256), (224, 288), (160, 224)
    sd = None
    m = _model(4)
    first = {}
    for k, hw in enumerate((Asz, Bsz, Asz, Bsz, Csz, Asz)):
        f = _visit(m, hw, seed=hw[0])
        if hw in first:
            assert torch.equal(f, first[hw]), (k, hw)                  # a revisited context computes the same bits
        first.setdefault(hw, f)
    assert m.contexts_built == 3 and len(m._cache) == 3
    sd = dict(m._state)
    m.load_state_dict(sd)
    assert len(m._cache) == 0 and m._ctx is None
    assert torch.equal(_visit(m, Asz, seed=Asz[0]), first[Asz]) and m.contexts_built == 4
    m = _model(None)                                                   # the default: one context, rebuilt at every change
    assert int(m.cfg.APSE.CONTEXT_CACHE) == 1
    for hw in (Asz, Bsz, Asz, Bsz, Csz, Asz):
        assert torch.equal(_visit(m, hw, seed=hw[0]), first[hw])
        assert len(m._cache) == 1
    assert m.contexts_built == 6
    m = _model(2)
    for hw in (Asz, Bsz, Csz, Asz):                                    # C evicts A, the least recently used
        _visit(m, hw, seed=hw[0])
    assert m.contexts_built == 4 and len(m._cache) == 2 and list(m._cache) == [(FRAME_HW, Csz), (FRAME_HW, Asz)]


ITERS = 20


def _tool(out, *extra):
    import finetune_segmentation as ft
    return ft.main(["--synthetic", "12", "--iters", str(ITERS), "--out", out, "--k-folds", "4", "--warmup-iters", "10", "--flip",
                    "--augment", "--min-sizes", "224,256,288"] + list(extra))


def test_tool_augmented_run_and_resume(tmp_path):
    a = _tool(str(tmp_path / "a"))
    assert len(a["losses"]) == ITERS and all(np.isfinite(a["losses"]))
    b_dir = str(tmp_path / "b")
    _tool(b_dir, "--stop-at", "10")
    b = _tool(b_dir, "--resume")
    for k, v in a["state"].items():
        assert torch.equal(v, b["state"][k]), k
