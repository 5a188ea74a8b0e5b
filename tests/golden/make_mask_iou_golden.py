"""Writes tests/golden/mask_translate_golden.npz: inputs and outputs of the reference's own translate_and_crop_mask
(dcnn/utils/mask_utils.py:57-77), bit-packed.  Needs the reference checkout (its path as the only argument); its module imports
cv2 for show_mask only, so an empty placeholder module stands in for it.

    python tests/golden/make_mask_iou_golden.py /path/to/reference

Seeded 37 x 150 masks at density 0.4, every (dx, dy) of the grids below (whole-frame shifts and beyond included)."""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

H, W = 37, 150
DX = [0, 1, -1, 63, -63, 64, -64, 65, -65, 127, -128, 149, -149, 150, -150, 200]
DY = [0, 1, -1, 36, -36, 37, -37, 50]
N_MASKS = 2


def main():
    ref_root = sys.argv[1]
    sys.modules.setdefault("cv2", types.ModuleType("cv2"))
    spec = importlib.util.spec_from_file_location("ref_mask_utils", os.path.join(ref_root, "dcnn", "utils", "mask_utils.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    rng = np.random.default_rng(20240607)
    masks = rng.random((N_MASKS, H, W)) < 0.4
    dx, dy, which, outs = [], [], [], []
    for i, x in enumerate(DX):
        for j, y in enumerate(DY):
            k = (i * len(DY) + j) % N_MASKS
            got = mod.translate_and_crop_mask(torch.from_numpy(masks[k]), (x, y)).numpy()
            assert got.shape == (H, W) and got.dtype == bool
            dx.append(x); dy.append(y); which.append(k); outs.append(np.packbits(got.reshape(-1)))
    here = os.path.dirname(os.path.abspath(__file__))
    np.savez_compressed(os.path.join(here, "mask_translate_golden.npz"), shape=np.asarray([H, W], np.int32),
                        masks=np.stack([np.packbits(m.reshape(-1)) for m in masks]), dx=np.asarray(dx, np.int32),
                        dy=np.asarray(dy, np.int32), mask_index=np.asarray(which, np.int32), outputs=np.stack(outs))


if __name__ == "__main__":
    main()
