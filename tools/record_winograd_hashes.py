#!/usr/bin/env python3
"""Records tests/golden/winograd_layer_sha256.json, the fixture of tests/test_gpu_winograd_bits.py: the sha256 of inner2 / inner3 /
p2 / p3 / rpn_t2 / rpn_t3 for the test's seeded frames, computed with the library that APSE_HIP_LIB names.  To pin a kernel
change to the bits of the commit before it, build that commit's csrc/ into a second .so and run (on the GPU)
    APSE_HIP_LIB=/path/to/parent/libapse_hip.so python tools/record_winograd_hashes.py [out.json]
The file keeps the recording library's apse_version() so that a reader can tell what it pins.
A section argument records one section and keeps the other as the file has it:
    ... python tools/record_winograd_hashes.py out.json layers     "cases": the Winograd layers (test_winograd_layers_keep_their_bits)
    ... python tools/record_winograd_hashes.py out.json plans      "plans": every plan variant (test_plans_keep_their_bits)
Record the plans twice and compare the two files before trusting them: an entry that differs between two recordings with one
library is not deterministic and goes into PLAN_NOT_DETERMINISTIC of the test."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import test_gpu_winograd_bits as T   # noqa: E402
from apse_uav_amd import _lib        # noqa: E402


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else T.GOLDEN
    section = sys.argv[2] if len(sys.argv) > 2 else "all"
    doc = json.load(open(T.GOLDEN)) if section != "all" else {}
    version = _lib.load().apse_version().decode()
    if section in ("all", "layers"):
        doc["recorded_with"], doc["cases"] = version, {}
        for frame_hw, batch in T.CASES:
            doc["cases"][T.case_key(frame_hw, batch)] = T.layer_hashes(frame_hw, batch)
            print(T.case_key(frame_hw, batch), doc["cases"][T.case_key(frame_hw, batch)], flush=True)
    if section in ("all", "plans"):
        doc["plans_recorded_with"], doc["plans"] = version, {}
        for name in sorted(T.PLAN_CASES):
            doc["plans"][name] = T.plan_hashes(name)
            print(name, doc["plans"][name], flush=True)
    with open(out, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")


main()
