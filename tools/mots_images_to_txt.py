#!/usr/bin/env python3
"""MOTS id-map PNGs -> MOTS .txt files on the GPU, the counterpart of mots_tools/mots_common/images_to_txt.py: same arguments,
same files.

    python tools/mots_images_to_txt.py IMG_DIR OUT_DIR SEQMAP

IMG_DIR holds one folder of id-map PNGs (000000.png, ...) per sequence of the seqmap; OUT_DIR/SEQ.txt gets one line
``t track_id class_id h w counts`` per non-zero value of every frame (class_id = value // 1000, values ascending, frames in
sorted file order).  Each frame is split into one bit window per value (apse_mots_split_idmap) and the windows are run-length
encoded on the device (utils/rle_device.encode_masks): no per-object dense mask is built.
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def sequence_lines(folder, dev):
    import numpy as np
    import torch
    from PIL import Image
    from apse_uav_amd.utils import mots_eval as me
    from apse_uav_amd.utils import rle_device
    lines = []
    for t, path in me.png_frames(folder).items():
        img = np.array(Image.open(path))
        if img.dtype != np.uint16:
            img = img.astype(np.uint16)
        idmap = torch.from_numpy(np.ascontiguousarray(img)).to(dev)
        values, windows, pool = me.split_idmap(idmap)
        h, w = img.shape
        for v, r in zip(values, rle_device.encode_masks(windows, (h, w), count=len(values))):
            lines.append("%d %d %d %d %d %s\n" % (t, v, v // 1000, h, w, r["counts"].decode("utf-8")))
        del pool
    return lines


def main(argv):
    if len(argv) != 4:
        print("Usage: python images_to_txt.py gt_img_folder gt_txt_output_folder seqmap")
        sys.exit(1)
    import torch
    if not torch.cuda.is_available():
        sys.exit("mots_images_to_txt.py: no GPU visible (the encoder has no CPU fallback)")
    from apse_uav_amd.utils import mots_metrics as mm
    dev = torch.device("cuda", torch.cuda.current_device())
    seqs, _ = mm.load_seqmap(argv[3], out=None)
    os.makedirs(argv[2], exist_ok=True)
    for seq in seqs:
        print("Converting sequence", seq)
        with open(os.path.join(argv[2], seq + ".txt"), "w") as fh:
            fh.write("".join(sequence_lines(os.path.join(argv[1], seq), dev)))


if __name__ == "__main__":
    main(sys.argv)
