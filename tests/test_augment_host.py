"""The augmentation oracle (tests/augment_ref.py) pinned by numbers worked outside it: every value below was obtained when the
rules of DESIGN.md "Training augmentation" were written down, from a separate evaluation of them.  The grey pixels, the constant
images and the ramp are the inputs where a blend lands within rounding distance of an integer, so that the float32 / float64
mix of the rules -- and nothing else -- decides the truncated grey level."""
import numpy as np
import pytest

import augment_ref as A


def _const(v, h=4, w=4):
    return np.full((h, w, 3), v, np.uint8)


def _ramp():
    return np.repeat(np.arange(256, dtype=np.uint8)[None, :, None], 3, axis=2)


def test_lighting_is_a_truncation():
    out, _ = A.augment(_const(100), lw=(0.2, -0.2, 0.2))
    assert (out == 99).all()
    px = np.array([[[0, 100, 255]]], np.uint8)
    assert A.augment(px, lw=(-0.2, 0, 0))[0].tolist() == [[[0, 100, 255]]]
    assert A.augment(px, lw=(0.2, 0, 0))[0].tolist() == [[[0, 99, 254]]]
    assert np.abs(A.lighting_vec((0.2, -0.2, 0.2))).max() < 0.05           # never scaled to 0..255


def test_brightness():
    assert (A.augment(_const(250), wb=1.1)[0] == 255).all()
    assert (A.augment(_const(10), wb=0.9)[0] == 9).all()


@pytest.mark.parametrize("wc,v,want", [(1.05, 128, 127), (1.05, 200, 199), (1.05, 1, 0), (1.05, 77, 77), (0.9, 77, 76),
                                       (1.1, 255, 255), (1.1, 128, 128)])
def test_contrast_on_constant_images(wc, v, want):
    assert (A.augment(_const(v), wc=wc)[0] == want).all()


def test_contrast_all_float64_differs():
    assert (A.augment_all_f64(_const(255), wc=1.1) == 254).all()


def test_saturation_on_the_grey_ramp():
    ramp = _ramp()
    assert np.array_equal(A.augment(ramp, ws=1.0)[0], ramp)
    out = A.augment(ramp, ws=0.93)[0]
    changed = np.nonzero((out != ramp).any(axis=2)[0])[0]
    assert len(changed) == 94 and changed[:6].tolist() == [3, 6, 9, 12, 15, 18]
    out = A.augment(ramp, ws=1.07)[0]
    assert np.nonzero((out != ramp).any(axis=2)[0])[0].tolist() == [127, 254]
    for ws, n in ((0.93, 95), (1.07, 6), (0.9, 188)):
        diff = (A.augment(ramp, ws=ws)[0] != A.augment_all_f64(ramp, ws=ws)).any(axis=2)
        assert int(diff.sum()) == n, (ws, int(diff.sum()))


def test_whole_chain_on_one_pixel():
    px = np.array([[[10, 200, 90]]], np.uint8)
    out, S = A.augment(px, wb=1.05, ws=0.92, wc=1.08, lw=(0.3, -0.1, 0.25))
    assert out.tolist() == [[[12, 209, 95]]] and S == 320


def test_sum_above_32_bits():
    img = np.full((2400, 2400, 3), 255, np.uint8)
    S = A.image_sum(img)
    assert S == 4406400000 and S > 2 ** 32
    assert np.float64(S) / np.float64(img.size) == 255.0


def test_identity_and_flip():
    img = np.random.default_rng(0).integers(0, 256, (7, 9, 3), dtype=np.uint8)
    assert np.array_equal(A.augment(img)[0], img)
    assert np.array_equal(A.augment(img, flip=True)[0], img[:, ::-1])


def test_transform_annotations():
    """ResizeTransform then HFlipTransform on XYXY boxes and polygons, in float64."""
    from apse_uav_amd.utils import augment
    boxes = np.array([[10.0, 20.0, 110.0, 70.0]])
    polys = [[[10.0, 20.0, 110.0, 20.0, 60.0, 70.0]]]
    b, p = augment.transform_annotations(boxes, polys, (100, 200), (50, 150), False)
    assert b.tolist() == [[7.5, 10.0, 82.5, 35.0]] and p[0][0].tolist() == [7.5, 10.0, 82.5, 10.0, 45.0, 35.0]
    b, p = augment.transform_annotations(boxes, polys, (100, 200), (50, 150), True)
    assert b.tolist() == [[67.5, 10.0, 142.5, 35.0]] and p[0][0].tolist() == [142.5, 10.0, 67.5, 10.0, 105.0, 35.0]
    assert b.dtype == np.float64 and p[0][0].dtype == np.float64


def test_draw_order():
    """size (only with several), flip (only when on), wb, ws, wc, lw -- and nothing is drawn for a step that is off."""
    from apse_uav_amd.utils import augment
    g, r = np.random.default_rng(5), np.random.default_rng(5)
    size = augment.draw_size(g, (640, 672, 704), "choice")
    p = augment.draw_params(g, True, True)
    assert size == (640, 672, 704)[int(r.integers(0, 3))]
    assert p.flip == bool(r.random() < 0.5)
    assert (p.brightness, p.saturation, p.contrast) == tuple(float(r.uniform(0.9, 1.1)) for _ in range(3))
    assert all(type(v) is float for v in (p.brightness, p.saturation, p.contrast))
    assert np.array_equal(p.lighting, r.normal(0, 0.2, 3))
    assert g.bit_generator.state == r.bit_generator.state
    # one size: no draw; everything off: no draw, the identity parameters
    before = g.bit_generator.state
    assert augment.draw_size(g, (800,), "choice") == 800
    q = augment.draw_params(g, False, False)
    assert g.bit_generator.state == before
    assert (q.flip, q.brightness, q.saturation, q.contrast, q.lighting.tolist()) == (False, 1.0, 1.0, 1.0, [0.0, 0.0, 0.0])
    lo = augment.draw_size(g, (640, 800), "range")
    assert 640 <= lo <= 800


def test_config_keys():
    """detectron2's defaults; the reference's Base-RCNN-FPN.yaml, when merged, gives the six sizes; the cache is off by default."""
    from apse_uav_amd.config import get_cfg
    cfg = get_cfg()
    assert (cfg.INPUT.MIN_SIZE_TRAIN, cfg.INPUT.MAX_SIZE_TRAIN, cfg.INPUT.MIN_SIZE_TRAIN_SAMPLING) == ((800,), 1333, "choice")
    assert cfg.APSE.CONTEXT_CACHE == 1
    cfg._merge({"INPUT": {"MIN_SIZE_TRAIN": [640, 672, 704, 736, 768, 800]}})
    assert cfg.INPUT.MIN_SIZE_TRAIN == (640, 672, 704, 736, 768, 800) and cfg.INPUT.MAX_SIZE_TRAIN == 1333
