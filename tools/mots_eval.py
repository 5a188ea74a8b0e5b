#!/usr/bin/env python3
"""KITTI MOTS evaluation on the GPU, a drop-in for mots_tools/mots_eval/eval.py: same arguments, same stdout.

    python tools/mots_eval.py RESULTS_FOLDER GT_FOLDER SEQMAP

Either folder holds, per sequence of the seqmap, a folder of id-map PNGs (000000.png, ...) or a MOTS .txt file.  The mask
arithmetic runs in HIP (utils/mots_eval.py); the metrics are utils/mots_metrics.py.
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main(argv):
    if len(argv) != 4:
        print("Usage: python eval.py results_folder gt_folder seqmap")
        sys.exit(1)
    from apse_uav_amd.utils.mots_eval import evaluate_mots
    evaluate_mots(argv[1], argv[2], argv[3])


if __name__ == "__main__":
    main(sys.argv)
