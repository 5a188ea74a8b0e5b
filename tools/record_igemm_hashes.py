#!/usr/bin/env python3
"""Records tests/golden/igemm_step_seam_sha256.json, the fixture of tests/test_gpu_igemm_step_seam.py: the sha256 of every case's
output, computed with the library that APSE_HIP_LIB names.  To pin a change of conv_igemm_f32's loop to the bits of the commit
before it, build that commit's csrc/ into a second .so and run (on the GPU)
    APSE_HIP_LIB=/path/to/parent/libapse_hip.so python tools/record_igemm_hashes.py [out.json]
The file holds names and hashes only, and the recording library's apse_version() so that a reader can tell what it pins."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import test_gpu_igemm_step_seam as T   # noqa: E402
from apse_uav_amd import _lib          # noqa: E402


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else T.GOLDEN
    doc = {"recorded_with": _lib.load().apse_version().decode(), "cases": {}}
    for name in sorted(T.CASES):
        doc["cases"][name] = T.sha(T.run_case(T.CASES[name]))
        print(name, doc["cases"][name], flush=True)
    with open(out, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")


main()
