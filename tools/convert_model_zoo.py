"""Converts a detectron2 model-zoo checkpoint (.pkl of numpy arrays) into the .pth form the package loads.

    python tools/convert_model_zoo.py model_final_f10217.pkl model_final_f10217.pth

The pickle is read through an allow-list of numpy / container globals (apse_uav_amd.weights.convert_model_zoo_pickle);
a file that names anything else is refused.  The result holds {"model": {name: f32 tensor}}."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from apse_uav_amd.weights import convert_model_zoo_pickle  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("src", help="model-zoo .pkl")
    ap.add_argument("dst", help="output .pth")
    a = ap.parse_args()
    sd = convert_model_zoo_pickle(a.src, a.dst)
    ncls = sd["roi_heads.box_predictor.cls_score.weight"].shape[0] - 1 if "roi_heads.box_predictor.cls_score.weight" in sd else None
    print("wrote %s: %d tensors%s" % (a.dst, len(sd), ", %d classes" % ncls if ncls is not None else ""))


if __name__ == "__main__":
    main()
