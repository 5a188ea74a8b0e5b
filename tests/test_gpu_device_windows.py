"""GPU test (-m gpu): one mixed mask list through every consumer of structures/device_windows.py, each compared exactly with the
host references of tests/ (mask_iou_ref, rle_ref and utils/rle.py) and a numpy statement of the owner rule of DESIGN.md "MOTS
evaluation".  The list: a one-word window, a window at x 63..129 (two word boundaries), a WindowMask without bits, one with an
empty rect, one whose word rows are longer than its rect needs (garbage in the spare words and outside the rect's columns), and
the second mask again as a dense bool tensor for the functions that take one."""
import math

import numpy as np
import pytest
import torch

import mask_iou_ref
import rle_ref
from apse_uav_amd import _lib
from apse_uav_amd.structures.instances import Instances
from apse_uav_amd.structures.window_mask import MaskList, WindowMask
from apse_uav_amd.utils import coco as cocomod
from apse_uav_amd.utils import mask_utils, rle, rle_device
from apse_uav_amd.utils import mots_eval as me

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
H, W = 70, 130
SCORES = [0.5, 0.9, 0.7, 0.9, 0.9, 0.95]                    # ties: the highest index keeps the pixel
CLASSES = [0, 2, 0, 2, 7, 2]                                 # 0 -> pedestrian (2), 2 -> car (1), 7 is not scored
IDS = [1, 2, 3, 4, 5, 6]
VALUES = [2001, 1002, 2003, 1004, 0, 1006]


def _window_mask(win, rect, garbage=None, extra_words=0):
    dense = rle_ref.dense(win, rect, H, W)
    cx, cy = mask_iou_ref.centroid(dense)
    bits = None
    if win is not None:
        words = rle_ref.pack_words(win, rect, garbage, extra_words)
        bits = torch.from_numpy(words.view(np.int64)).to(DEV)
    return WindowMask(bits, rect, (H, W), (cx, cy) if dense.any() else (-1, -1), int(dense.sum())), dense


@pytest.fixture(scope="module")
def case():
    """(masks: five WindowMasks and the dense twin of the second, the dense host frame of each)."""
    g = np.random.default_rng(21)
    rnd = lambda rect: g.random((rect[3] - rect[1], rect[2] - rect[0])) < 0.7          # noqa: E731
    one_word, across, wide = (5, 3, 40, 20), (63, 10, 129, 60), (20, 30, 100, 65)
    pairs = [_window_mask(rnd(one_word), one_word),
             _window_mask(rnd(across), across, garbage=g),
             _window_mask(None, (10, 10, 30, 20)),
             (WindowMask(torch.zeros((4, 1), dtype=torch.int64, device=DEV), (70, 5, 70, 9), (H, W), (-1, -1), 0),
              np.zeros((H, W), bool)),
             _window_mask(rnd(wide), wide, garbage=g, extra_words=2)]
    masks, dense = [m for m, _ in pairs], [d for _, d in pairs]
    assert tuple(masks[1].bits.shape) == (50, 3) and tuple(masks[4].bits.shape) == (35, 2 + 2)
    return masks + [torch.from_numpy(dense[1]).to(DEV)], dense + [dense[1]]


def _instances(masks):
    inst = Instances((H, W))
    n = len(masks)
    inst.pred_classes = torch.as_tensor(CLASSES[:n], dtype=torch.int64)
    inst.scores = list(torch.as_tensor(np.asarray(SCORES[:n], np.float64)))
    inst.ids = IDS[:n]
    inst.pred_masks = MaskList(masks)
    return inst


def _owners(dense, n):
    """int [H, W]: the object of highest (score, index) among the first ``n`` that hold the pixel, -1 where none does."""
    owner = np.full((H, W), -1)
    best = np.full((H, W), -np.inf)
    for k in range(n):
        take = dense[k] & (SCORES[k] >= best)
        owner[take], best[take] = k, SCORES[k]
    return owner


def test_masks_iou_matrix(case):
    masks, dense = case
    want = np.array([[mask_iou_ref.masks_iou(a, b) for b in dense] for a in dense], np.float32)
    got = mask_utils.masks_iou_matrix(masks, masks)
    assert got.dtype == np.float32 and np.array_equal(got, want)
    assert np.array_equal(got[5], got[1]) and np.array_equal(got[:, 5], got[:, 1])       # the dense copy and its twin
    assert got[1, 1] == 1.0 and not got[2].any() and not got[3].any() and got[0, 4] > 0


def test_mask_utils_refuses_host_bits(case):
    masks, _ = case
    with pytest.raises(_lib.ApseError):
        mask_utils.masks_iou_matrix([masks[0]], [masks[1].to("cpu")])


def test_render_idmap(case):
    masks, dense = case
    owner = _owners(dense, 6)
    want = np.where(owner >= 0, np.asarray(VALUES)[owner], 0).astype(np.uint16)
    got = me.render_idmap(_instances(masks), (H, W), DEV).cpu().numpy()
    assert np.array_equal(got, want)
    twin = me.render_idmap(_instances(masks[:5] + [masks[1]]), (H, W), DEV).cpu().numpy()
    assert np.array_equal(twin, want)
    # the twin outranks the mask it copies, the masks without pixels write nothing
    assert (got == 2001).any() and (got == 1006).any() and not np.isin(got, (1002, 2003, 1004)).any()


def test_encode_masks(case):
    masks, dense = case
    got = rle_device.encode_masks(masks[:5], (H, W))
    assert got == [rle.encode(d) for d in dense[:5]]
    runs = rle_device.encode_masks(masks[:5], (H, W), compressed=False)
    for k, m in enumerate(masks[:5]):
        win = None if m.bits is None else rle_ref.unpack_words(m.bits.cpu().numpy().view(np.uint64), m.rect)
        ends = rle_ref.ends_from_window(win, m.rect, H, W)
        assert runs[k] == {"size": [H, W], "counts": np.diff(ends, prepend=0).tolist()}
        assert runs[k]["counts"] == [int(c) for c in rle.counts_from_mask(dense[k])]


def test_crop_overlaps(case):
    masks, dense = case
    owner = _owners(dense, 5)
    got, changed = rle_device.crop_overlaps(_instances(masks[:5]), with_changed=True)
    for k, m in enumerate(got):
        want = dense[k] & (owner == k)
        assert m.rect == masks[k].rect and np.array_equal(m.dense().cpu().numpy(), want)
        assert m.mass == int(want.sum()) and changed[k] == bool((want != dense[k]).any())
        for u, v in zip(m.centroid, mask_iou_ref.centroid(want)):
            assert u == v or (math.isnan(u) and math.isnan(v))
    assert got[2].bits is None and got[3].bits is None
    assert tuple(got[4].bits.shape) == tuple(masks[4].bits.shape) and changed[1] and not changed[0]


def test_segm_to_windows_and_back(case):
    masks, dense = case
    windows, sizes, keep = cocomod.segm_to_windows([(m, H, W) for m in masks[:5]], DEV)
    assert sizes == [(H, W)] * 5 and tuple(windows.shape) == (5, 32)
    assert np.array_equal(cocomod.windows_to_dense(windows, H, W), np.stack(dense[:5]))
