#!/usr/bin/env python3
"""Times the fused f32 Winograd kernel on ONE layer shape in isolation (HIP events around `iters` back-to-back launches on the
launch stream, outputs on a ring larger than the Infinity Cache) and prints the sha256 of the output, so that two builds
(APSE_HIP_LIB) can be compared bit for bit and by time on the same box:  python tools/winograd_probe.py <out2|rpn_t2|out3|p4|odd>[,<layer>...] [iters]
Shapes are the f32 batch-1 layers of the 4K frame.  The network run stays the judge of a kernel change; this is the quick look."""
import ctypes as C
import hashlib
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from apse_uav_amd import _lib

# name: (B, H, W, Cin, Cout, relu)
SH = {"out2": (1, 192, 336, 256, 256, 0), "rpn_t2": (1, 192, 336, 256, 256, 1), "out3": (1, 96, 168, 256, 256, 0),
      "p4": (1, 48, 84, 256, 256, 0), "odd": (2, 75, 125, 256, 256, 1)}


def probe(name, iters):
    B, H, W, Cin, Cout, relu = SH[name]
    lib = _lib.load()
    dev = torch.device("cuda:0")
    d = _lib.ConvDesc()
    d.B, d.H, d.W, d.Cin, d.Cout, d.KH, d.KW, d.stride, d.pad, d.relu = B, H, W, Cin, Cout, 3, 3, 1, 1, relu
    g = torch.Generator().manual_seed(11)
    w = (torch.randn(Cout, Cin, 3, 3, generator=g) / (Cin * 9) ** 0.5).numpy()
    packed = np.zeros(16 * Cout * Cin, np.float32)
    _lib.check(lib.apse_winograd_pack_filter(_lib.ptr(np.ascontiguousarray(w)), Cout, Cin, _lib.ptr(packed)), None, "pack")
    x = torch.randn(B, H, W, Cin, generator=g).to(dev)
    wd = torch.from_numpy(packed).to(dev)
    bd = torch.randn(Cout, generator=g).to(dev)
    n_ring = max(2, int(320e6 // (B * H * W * Cout * 4)) + 1)
    ring = [torch.empty(B, H, W, Cout, device=dev) for _ in range(n_ring)]

    def launch(y):
        rc = lib.apse_winograd_conv2d(C.byref(d), _lib.ptr(x), _lib.ptr(wd), _lib.ptr(bd), _lib.ptr(y), _lib.stream_ptr())
        assert rc == 0, rc

    for i in range(5):
        launch(ring[i % n_ring])
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(iters):
        launch(ring[i % n_ring])
    e1.record()
    torch.cuda.synchronize()
    us = e0.elapsed_time(e1) * 1e3 / iters
    digest = hashlib.sha256(ring[0].cpu().numpy().tobytes()).hexdigest()[:16]
    flop = 2.0 * B * H * W * Cout * Cin * 9
    print("%-7s %8.2f us  %6.1f TFLOP/s algorithmic  %5.1f TFLOP/s on the matrix pipe  sha %s  %s"
          % (name, us, flop / us / 1e6, flop * 16 / 36 / us / 1e6, digest, os.environ.get("APSE_HIP_LIB", "tree")))


for layer in sys.argv[1].split(","):
    probe(layer, int(sys.argv[2]) if len(sys.argv) > 2 else 50)
