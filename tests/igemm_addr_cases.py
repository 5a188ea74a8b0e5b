"""Cases and the child-process worker of tests/test_gpu_igemm_pointwise.py.

conv_igemm_f32 picks the address code of its k loop per launch (csrc/conv_igemm.hip: the pointwise kernel, or the general
per-step code) unless APSE_IGEMM_ADDR=0, which is read once per process.  The worker runs every case through the stateless
apse_conv2d in THIS process, under whatever the environment says, and writes each output's raw bytes to an .npz; the test starts
it twice.  Under LAUNCHES the file also holds, per case in the order of CASES, how many launches of the pointwise kernel the case
made (apse_conv_pointwise_launches before and after it), so that the test sees which address form really ran.

    python tests/igemm_addr_cases.py OUT.npz

Every operand sits between NaN guard bands, y and the split-K workspace are NaN-filled, and the worker itself asserts that no
guard word changed and that no NaN reached y.
"""
import ctypes as C
import os
import sys

import numpy as np

GUARD = 1024                     # floats in front of and behind x, y and the workspace
CFGS = (0, 1, 3, 6)              # the tile configs the plans use: 128x128, 64x64, 128x64, 64x64 with two k groups
LAUNCHES = "__pointwise_launches__"


def cin_stored(c):
    """Cin as stored: the next power of two, at least 4."""
    p = 4
    while p < c["cin"]:
        p *= 2
    return p


def takes_pointwise(c):
    """pointwise_ok of csrc/conv_igemm.hip: 1x1 / pad 0 whose filter row (padded to 32 floats) is exactly the pixel's Cin run."""
    return c["k"] == 1 and c["pad"] == 0 and -(-c["k"] * cin_stored(c) // 32) * 32 == cin_stored(c)


def _case(group, name, **kw):
    c = dict(group=group, name=name, B=1, H=7, W=9, cin=64, cout=80, k=1, stride=1, pad=0, cfg=1, splitk=0, relu=0, res_mode=0,
             bias=False, prec=0)
    c.update(kw)
    return c


def cases():
    out = []
    # ---- pointwise f32: rows past M in the first (M = 1, 63) and in the last tile (65, 129), every tile config
    for (h, w) in ((1, 1), (7, 9), (5, 13), (3, 43)):
        for cfg in CFGS:
            out.append(_case("pw", "pw_m%d_cfg%d" % (h * w, cfg), H=h, W=w, cfg=cfg))
    # Cin 32 / 64 / 96 (stored padded to 128): 1, 2 and 4 sub-steps -- one live half of a KS = 2 step, a whole step, two steps;
    # Cout 80 (columns past the tile) and 64
    for cin in (32, 64, 96):
        for cfg in CFGS:
            out.append(_case("pw", "pw_cin%d_cfg%d" % (cin, cfg), cin=cin, cfg=cfg))
        for cfg in (0, 1):
            out.append(_case("pw", "pw_cin%d_cout64_cfg%d" % (cin, cfg), cin=cin, cout=64, cfg=cfg))
    for cin in (64, 128):
        for cfg in CFGS:
            out.append(_case("pw", "pw_s2_cin%d_cfg%d" % (cin, cfg), H=9, W=11, cin=cin, stride=2, cfg=cfg))
    # split K over 4 sub-steps: 2 slices, and 3 slices of which the last is EMPTY (2 + 2 + 0 sub-steps, 1 + 1 + 0 steps at KS = 2)
    for sk in (2, 3):
        for cfg in CFGS:
            out.append(_case("pw", "pw_splitk%d_cfg%d" % (sk, cfg), H=5, W=13, cin=128, cfg=cfg, splitk=sk))
    # a dead part INSIDE a split of two: Cin 32 is one sub-step, so the second slice is empty at every tile config and at KS = 2
    # (configs 1, 6) the first holds a live and a dead half step; Cin 64 is two sub-steps: one whole step and an empty slice at
    # KS = 2, one step per slice at KS = 1
    for cin in (32, 64):
        for cfg in CFGS:
            out.append(_case("pw", "pw_cin%d_splitk2_cfg%d" % (cin, cfg), H=5, W=13, cin=cin, cfg=cfg, splitk=2))
    for cfg in (1, 3):
        out.append(_case("pw", "pw_b3_cfg%d" % cfg, B=3, H=5, W=13, cfg=cfg))
    for res_mode in (0, 1, 2):
        for relu in (0, 1):
            for cfg in (3, 6):
                out.append(_case("pw", "pw_res%d_relu%d_cfg%d" % (res_mode, relu, cfg), H=6, W=8, cfg=cfg, res_mode=res_mode, relu=relu, bias=True))
    # ---- the same loop with bf16 / f16 operands and storage
    for prec in (1, 2):
        for cfg in CFGS:
            out.append(_case("pw16", "pw16_p%d_cin64_m65_cfg%d" % (prec, cfg), H=5, W=13, cfg=cfg, prec=prec))
            out.append(_case("pw16", "pw16_p%d_cin128_m129_cfg%d" % (prec, cfg), H=3, W=43, cin=128, cfg=cfg, prec=prec))
            out.append(_case("pw16", "pw16_p%d_k3_cfg%d" % (prec, cfg), H=5, W=5, k=3, pad=1, cfg=cfg, prec=prec))
        out.append(_case("pw16", "pw16_p%d_res1_relu" % prec, H=6, W=8, cfg=6, prec=prec, res_mode=1, relu=1, bias=True))
        out.append(_case("pw16", "pw16_p%d_s2_splitk2" % prec, H=9, W=11, cin=256, stride=2, cfg=1, prec=prec, splitk=2))
    # ---- filters with padding taps: every pattern of taps inside / outside the map occurs on maps of 1, 2 and 5 pixels a side
    # and at 9 x 11.  (k, cin): 3x3 over whole sub-steps; 3x3 / Cin 8 = 3 sub-steps and 5x5 / Cin 4 = 5 sub-steps (a dead half
    # step; filter rows padded to 32 floats); 5x5 / Cin 32 (25 taps); 7x7 (49 taps).  All of them keep the general code under
    # either setting: the cases pin that the switch leaves them alone
    maps = [(h, w) for h in (1, 2, 5) for w in (1, 2, 5)] + [(9, 11)]
    n = 0
    for (k, cin) in ((3, 32), (3, 8), (5, 4), (5, 32), (7, 4), (7, 32)):
        for stride in (1, 2):
            for (h, w) in maps:
                cfgs = CFGS if (h, w) in ((5, 5), (9, 11)) and cin == 32 and k == 3 else (CFGS[n % 4],)
                n += 1
                for cfg in cfgs:
                    out.append(_case("general", "k%d_cin%d_s%d_%dx%d_cfg%d" % (k, cin, stride, h, w, cfg), H=h, W=w, cin=cin, cout=72,
                                     k=k, stride=stride, pad=k // 2, cfg=cfg))
    for sk in (2, 4):
        for cfg in (1, 6):
            out.append(_case("general", "k3_cin32_splitk%d_cfg%d" % (sk, cfg), H=9, W=11, cin=32, cout=72, k=3, pad=1, cfg=cfg, splitk=sk))
    out.append(_case("general", "k3_cin64_b3_res1_relu", B=3, H=5, W=5, cin=64, cout=72, k=3, pad=1, cfg=6, res_mode=1, relu=1, bias=True))
    assert len({c["name"] for c in out}) == len(out)
    return out


CASES = cases()
GROUPS = ("pw", "pw16", "general")


def _operands(c):
    """Seeded operands of a case (the same in both processes): x NCHW, w OIHW, bias, residual NCHW (or None)."""
    rng = np.random.RandomState((c["cin"] * 1000003 + c["k"] * 10007 + c["H"] * 101 + c["W"] * 13 + c["B"] * 7 + c["cout"]) % (2 ** 31))
    oh = (c["H"] + 2 * c["pad"] - c["k"]) // c["stride"] + 1
    ow = (c["W"] + 2 * c["pad"] - c["k"]) // c["stride"] + 1
    x = rng.standard_normal((c["B"], c["cin"], c["H"], c["W"])).astype(np.float32)
    w = rng.standard_normal((c["cout"], c["cin"], c["k"], c["k"])).astype(np.float32)
    bias = rng.standard_normal(c["cout"]).astype(np.float32) if c["bias"] else None
    res = None
    if c["res_mode"] == 1:
        res = rng.standard_normal((c["B"], c["cout"], oh, ow)).astype(np.float32)
    elif c["res_mode"] == 2:
        res = rng.standard_normal((c["B"], c["cout"], oh // 2, ow // 2)).astype(np.float32)
    return x, w, bias, res, oh, ow


def run_case(c):
    """The case's output as raw bytes (uint8 array) in its storage type, NHWC, from apse_conv2d on cuda:0."""
    import torch
    from apse_uav_amd import _lib
    from hip_helpers import pack_filter, to_nhwc
    tdt = {0: torch.float32, 1: torch.bfloat16, 2: torch.float16}[c["prec"]]
    esz = 4 if c["prec"] == 0 else 2
    x, w, bias, res, oh, ow = _operands(c)
    packed, cin_p = pack_filter(torch.from_numpy(w))

    def guarded(n, dtype, payload=None):
        buf = torch.full((n + 2 * GUARD,), float("nan"), device="cuda", dtype=dtype)
        view = buf[GUARD:GUARD + n]
        if payload is not None:
            view.copy_(payload.reshape(-1).to(dtype))
        return buf, view

    xn = to_nhwc(torch.from_numpy(x), cin_p)
    xbuf, xv = guarded(xn.numel(), tdt, xn)
    ybuf, yv = guarded(c["B"] * oh * ow * c["cout"], tdt)
    sk = max(c["splitk"], 1)
    wsbuf, wsv = guarded(sk * c["B"] * oh * ow * c["cout"] + 16, torch.float32)
    wd = torch.from_numpy(packed).cuda()
    bp = torch.zeros(((c["cout"] + 127) // 128) * 128)
    if bias is not None:
        bp[:c["cout"]] = torch.from_numpy(bias)
    bd = bp.cuda()
    rd = None if res is None else to_nhwc(torch.from_numpy(res)).to(tdt).cuda().contiguous()
    d = _lib.ConvDesc()
    d.B, d.H, d.W, d.Cin, d.Cout, d.KH, d.KW, d.stride, d.pad = c["B"], c["H"], c["W"], cin_p, c["cout"], c["k"], c["k"], c["stride"], c["pad"]
    d.relu, d.res_mode, d.cfg, d.splitk, d.prec, d.fuse_reduce = c["relu"], c["res_mode"], c["cfg"], c["splitk"], c["prec"], 0
    d.x_st = d.res_st = d.y_st = c["prec"]
    rc = _lib.load().apse_conv2d(C.byref(d), _lib.ptr(xv), _lib.ptr(wd), _lib.ptr(bd), _lib.ptr(rd), _lib.ptr(yv), _lib.ptr(wsv),
                                 wsv.numel() * 4, _lib.stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0, (c["name"], rc)
    for buf, v, what in ((xbuf, xv, "x"), (ybuf, yv, "y"), (wsbuf, wsv, "ws")):
        assert bool(torch.isnan(buf[:GUARD]).all()) and bool(torch.isnan(buf[GUARD + v.numel():]).all()), (c["name"], "guard band of " + what)
    assert not bool(torch.isnan(yv).any()), (c["name"], "NaN in y: elements never written, or a read outside x")
    out = yv.contiguous().view(torch.uint8).cpu().numpy()
    assert out.size == yv.numel() * esz
    return out


def main(path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for p in (root, os.path.dirname(os.path.abspath(__file__))):
        if p not in sys.path:
            sys.path.insert(0, p)
    from apse_uav_amd import _lib
    outs, launches = {}, []
    for c in CASES:
        before = _lib.load().apse_conv_pointwise_launches()
        outs[c["name"]] = run_case(c)
        launches.append(_lib.load().apse_conv_pointwise_launches() - before)
    outs[LAUNCHES] = np.asarray(launches, dtype=np.int64)
    np.savez(path, **outs)


if __name__ == "__main__":
    main(sys.argv[1])
