"""-m gpu: every launcher of csrc/roi.hip against the float64 references of tests/roi_ref.py, called directly through ctypes
(tests/hip_helpers.py: ROI_KERNEL_SIG, FpnMaps) at the shapes, types and edges where the kernels change behaviour.

Tolerances are derived, not fitted (roi_ref.py states each derivation): max and integer outputs are exact; an f32 output
satisfies |got - ref64| <= n_ops * 2^-24 * mag element by element; a 16-bit output lies between round16(ref - b) and
round16(ref + b).  No case and no element is exempt.  Every output is prefilled with NaN; rows documented as untouched carry a
second bit pattern and are compared bit for bit.  The worst err / bound of each test goes to ops_parity.log.
"""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import roi_cases as rc
import roi_ref as rr

pytestmark = pytest.mark.gpu

TDT = {0: torch.float32, 1: torch.bfloat16, 2: torch.float16}
ST = pytest.mark.parametrize("st", [0, 1, 2], ids=["f32", "bf16", "f16"])
SENT32, SENT16 = 0x7fc0beef, 0x7fee          # NaN payloads no kernel writes: "this row was not touched"
E_INVALID = -1


def _log(logdir, name, obj):
    with open(os.path.join(logdir, "ops_parity.log"), "a") as f:
        f.write("roi_ops/" + name + " " + json.dumps(obj) + "\n")


def _lib():
    from hip_helpers import roi_kernels
    return roi_kernels()


def _p(t):
    from apse_uav_amd import _lib as L
    return L.ptr(t)


def _s():
    from apse_uav_amd import _lib as L
    return L.stream_ptr()


def _dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).cuda().contiguous()


def _ints(v):
    return None if v is None else torch.tensor(np.asarray(v).reshape(-1).tolist(), dtype=torch.int32, device="cuda")


def _nan(shape, st=0):
    return torch.full(tuple(shape), float("nan"), dtype=TDT[st], device="cuda")


def _iv(t):
    return t.view(torch.int32 if t.element_size() == 4 else torch.int16)


def _mark(t, lo):
    """rows [lo:] of ``t`` get the untouched pattern"""
    _iv(t)[lo:] = SENT32 if t.element_size() == 4 else SENT16


def _untouched(t, lo):
    return bool((_iv(t)[lo:] == (SENT32 if t.element_size() == 4 else SENT16)).all())


def _maps(dims, n_img, st, seed, const=None):
    """(device maps in storage type st, the same values widened to f32 on the host)"""
    rng = np.random.RandomState(seed)
    dev, host = [], []
    for k, (h, w) in enumerate(dims):
        a = rng.standard_normal((n_img, h, w, 256)).astype(np.float32) if const is None else np.full((n_img, h, w, 256), const[k], np.float32)
        t = torch.from_numpy(a).to(TDT[st])
        dev.append(t.cuda().contiguous())
        host.append(t.float().numpy())
    return dev, host


_PLANS = {}


def _plan(key, boxes, dims, R):
    """roi_align_plan does not depend on the storage type: built once per (case, R)"""
    if (key, R) not in _PLANS:
        _PLANS[(key, R)] = rr.roi_align_plan(boxes, dims, rr.FPN_SCALES, R)
    return _PLANS[(key, R)]


def _window(host):
    return lambda lv, img, y0, y1, x0, x1: host[lv][img, y0:y1, x0:x1]


def _run_align(lib, dev, dims, st, boxes, R, n_max, roi_img=None, total=None, per_img=0, cnt=None, out=None):
    from hip_helpers import fpn_maps
    F = fpn_maps(dev, dims, st)
    bd = _dev(np.asarray(boxes, np.float32))
    assert bd.shape[0] >= n_max
    out = _nan((n_max, R, R, 256), st) if out is None else out
    ri, cn, tt = _ints(roi_img), _ints(cnt), _ints(total)
    assert ri is None or ri.numel() >= n_max
    code = lib.apse_k_roi_align(C.byref(F), _p(bd), _p(ri), _p(cn), _p(tt), per_img, n_max, R, _p(out), st, _s())
    torch.cuda.synchronize()
    return code, out


def _describe(p, names, i):
    return dict(roi=i, name=names[i] if names and i < len(names) else None, level=p["level"] + 2, form=p["form"], gh=p["gh"], gw=p["gw"],
                win_y=p["win_y"].tolist(), win_x=p["win_x"].tolist())


def _compare_align(out, plan, imgs, window, R, st, rows, C_=256, names=None, chunk=256):
    """err / bound of the rows ``rows`` of ``out`` [n][R][R][C]; the first offending roi is reported with the reference's per-roi
    report (level, form, windows)."""
    worst = 0.0
    rows = list(rows)
    for lo in range(0, len(rows), chunk):
        idx = rows[lo:lo + chunk]
        res = rr.roi_align_apply([plan[i] for i in idx], [imgs[i] for i in idx], window, R, C=C_)
        got = out[torch.tensor(idx, device=out.device)].float().cpu().numpy()
        for j, i in enumerate(idx):
            ok, w = rr.check(got[j], dict(ref=res["ref"][j], mag=res["mag"][j], n_ops=res["n_ops"][j]), st)
            assert ok, _describe(plan[i], names, i)
            worst = max(worst, w)
    return worst


# ====================================================================================================== roi_align_nhwc
@ST
def test_roi_align_edge_boxes_and_locality(st, logdir):
    """Packed-list mode on the edge list (16 / 17-cell windows per axis, level thresholds, empty grids, boxes outside the map,
    the per-sample form on level 5) plus random boxes, R = 1, 7 and 14, two images; 64 rois, so a roi's bins are split over the
    largest number of blocks.

    Locality: the run is repeated on maps whose every cell OUTSIDE the union of the reference's tap windows is overwritten with a
    large finite value of alternating sign, and must give the same bits.  NaN / Inf poison is deliberately not used: the 16-bit
    form loads the cell past an odd window's last column (and padding cells) and multiplies it by a zero weight, which a
    finite value survives and a NaN would not; what is asserted is that a bin depends only on the cells its samples touch."""
    lib = _lib()
    boxes, names = rc.align_edge_boxes()
    boxes = np.concatenate([boxes, rc.random_boxes(21, 64 - len(boxes), 640., 640.)])
    n = len(boxes)
    imgs = np.arange(n) % 2
    dev, host = _maps(rc.PYR_E, 2, st, 100 + st)
    big = 6.0e4 if st == 2 else 1.0e30
    for R in (1, 7, 14):
        plan = rr.roi_align_plan(boxes, rc.PYR_E, rr.FPN_SCALES, R)
        if R == 7:
            assert {p["form"] for p in plan} == {"sep", "direct"}
        code, out = _run_align(lib, dev, rc.PYR_E, st, boxes, R, n, roi_img=imgs, total=[n])
        assert code == 0
        worst = _compare_align(out, plan, imgs, _window(host), R, st, range(n), names=names)
        _log(logdir, "roi_align_edges/%s/R%d" % (TDT[st], R), dict(worst_err_over_bound=worst))
        used = rr.roi_align_used_cells(plan, imgs, rc.PYR_E, 2)
        dev2 = []
        for k in range(4):
            alt = np.where(np.indices(used[k].shape).sum(axis=0) & 1, -big, big).astype(np.float32)
            dev2.append(_dev(np.where(used[k][..., None], host[k], alt[..., None]).astype(np.float32), TDT[st]))
        assert sum(int((~u).sum()) for u in used) > 10000               # there is something to overwrite
        code, out2 = _run_align(lib, dev2, rc.PYR_E, st, boxes, R, n, roi_img=imgs, total=[n])
        assert code == 0
        assert torch.equal(_iv(out), _iv(out2)), "a bin read a cell outside its tap window"


@ST
def test_roi_align_per_image_mode(st, logdir):
    """Per-image mode as the box head runs it: image = r / per_img, live rois from cnt = [per_img, 0, 3, per_img - 1]; dead rois
    are zero-filled.  1000 rois: an intermediate number of blocks per roi."""
    lib = _lib()
    per = 250
    n = 4 * per
    cnt = [per, 0, 3, per - 1]
    boxes = rc.random_boxes(31, n)
    imgs = np.arange(n) // per
    live = [r for r in range(n) if r % per < cnt[r // per]]
    dead = [r for r in range(n) if r % per >= cnt[r // per]]
    dev, host = _maps(rc.PYR_A, 4, st, 200 + st)
    for R in (7, 14):
        plan = _plan("per_image", boxes, rc.PYR_A, R)
        code, out = _run_align(lib, dev, rc.PYR_A, st, boxes, R, n, per_img=per, cnt=cnt)
        assert code == 0
        worst = _compare_align(out, plan, imgs, _window(host), R, st, live)
        assert bool((_iv(out)[torch.tensor(dead, device="cuda")] == 0).all()), "dead rois must be +0"
        _log(logdir, "roi_align_per_image/%s/R%d" % (TDT[st], R), dict(worst_err_over_bound=worst, live=len(live)))


@ST
@pytest.mark.parametrize("total", [40, 64, 100])
def test_roi_align_packed_total(st, total, logdir):
    """Packed list with *total below, equal to and above n_max = 64: rows at or past min(*total, n_max) are never written."""
    lib = _lib()
    n_max = 64
    nl = min(total, n_max)
    boxes = rc.random_boxes(41, n_max)
    imgs = (np.arange(n_max) * 7) % 3
    dev, host = _maps(rc.PYR_A, 3, st, 300 + st)
    plan = rr.roi_align_plan(boxes, rc.PYR_A, rr.FPN_SCALES, 7)
    out = _nan((n_max, 7, 7, 256), st)
    _mark(out, nl)
    code, out = _run_align(lib, dev, rc.PYR_A, st, boxes, 7, n_max, roi_img=imgs, total=[total], out=out)
    assert code == 0 and _untouched(out, nl)
    worst = _compare_align(out, plan, imgs, _window(host), 7, st, range(nl))
    _log(logdir, "roi_align_total/%s/%d" % (TDT[st], total), dict(worst_err_over_bound=worst))


@ST
def test_roi_align_many_rois(st, logdir):
    """8200 rois on a small pyramid: the packed list runs 2048 blocks (grid-stride over the rois), per-image mode one block per
    roi with all its bins in that block."""
    lib = _lib()
    per = 2050
    n = 4 * per
    boxes = np.concatenate([rc.random_boxes(51, n // 2, 84., 48.), rc.random_boxes(52, n - n // 2)])
    dev, host = _maps(rc.PYR_SMALL, 4, st, 400 + st)
    plan = _plan("many", boxes, rc.PYR_SMALL, 7)
    imgs = (np.arange(n) * 5) % 4
    total = n - 100
    out = _nan((n, 7, 7, 256), st)
    _mark(out, total)
    code, out = _run_align(lib, dev, rc.PYR_SMALL, st, boxes, 7, n, roi_img=imgs, total=[total], out=out)
    assert code == 0 and _untouched(out, total)
    w1 = _compare_align(out, plan, imgs, _window(host), 7, st, range(total), chunk=1024)
    del out
    cnt = [per, per - 1, 0, 7]
    imgs2 = np.arange(n) // per
    live = [r for r in range(n) if r % per < cnt[r // per]]
    dead = [r for r in range(n) if r % per >= cnt[r // per]]
    code, out = _run_align(lib, dev, rc.PYR_SMALL, st, boxes, 7, n, per_img=per, cnt=cnt)
    assert code == 0
    w2 = _compare_align(out, plan, imgs2, _window(host), 7, st, live, chunk=1024)
    assert bool((_iv(out)[torch.tensor(dead, device="cuda")] == 0).all())
    _log(logdir, "roi_align_many/%s" % TDT[st], dict(worst_err_over_bound_packed=w1, worst_err_over_bound_per_image=w2))


@ST
def test_roi_align_level_choice_is_exact(st, logdir):
    """The four maps are the constants 2, 3, 4, 5: a roi with a sample grid whose samples all lie inside its map returns its
    level -- the nearest integer of every output element is the reference's level, and the element is inside its bound."""
    lib = _lib()
    boxes, names = rc.align_edge_boxes()
    boxes = np.concatenate([boxes, rc.random_boxes(61, 400, 640., 640.)])
    n = len(boxes)
    dev, host = _maps(rc.PYR_E, 1, st, 0, const=(2., 3., 4., 5.))
    imgs = np.zeros(n, np.int64)
    for R in (7, 14):
        plan = rr.roi_align_plan(boxes, rc.PYR_E, rr.FPN_SCALES, R)
        code, out = _run_align(lib, dev, rc.PYR_E, st, boxes, R, n, roi_img=imgs, total=[n])
        assert code == 0
        worst = _compare_align(out, plan, imgs, _window(host), R, st, range(n), names=names)
        got = out.float().cpu().numpy()
        sure = [i for i, p in enumerate(plan) if p["inside"] and p["gh"] > 0 and p["gw"] > 0]
        assert len(sure) > 100 and all(names.index("thr%d_%s" % (t, k)) in sure for t in rc.LEVEL_THRESHOLDS for k in ("lo", "hi", "at"))
        for i in sure:
            assert (np.rint(got[i]) == plan[i]["level"] + 2).all(), _describe(plan[i], names, i)
        _log(logdir, "roi_align_levels/%s/R%d" % (TDT[st], R), dict(worst_err_over_bound=worst, rois_with_exact_level=len(sure)))


@ST
def test_roi_align_frame_boxes_and_unit_extent_maps(st, logdir):
    """A frame-sized box on every level (a pyramid whose level-l map is exactly that box), and coarsest maps of H = 1 and W = 1."""
    lib = _lib()
    edge, _ = rc.align_edge_boxes()
    worst = 0.0
    for dims, boxes in ((rc.PYR_F, np.array([b for b, _ in rc.FRAME_BOXES], np.float32)),
                        (rc.PYR_H1, np.concatenate([edge, [[0., 0., 512., 512.], [0., 0., 288., 32.], [-40., -8., 2000., 400.]]]).astype(np.float32)),
                        (rc.PYR_W1, np.concatenate([edge, [[0., 0., 512., 512.], [0., 0., 32., 288.], [-8., -40., 400., 2000.]]]).astype(np.float32))):
        dev, host = _maps(dims, 1, st, 500 + st)
        imgs = np.zeros(len(boxes), np.int64)
        for R in (7, 14):
            plan = rr.roi_align_plan(boxes, dims, rr.FPN_SCALES, R)
            if dims is rc.PYR_F:
                assert [p["level"] for p in plan] == [lv for _, lv in rc.FRAME_BOXES]
            code, out = _run_align(lib, dev, dims, st, boxes, R, len(boxes), roi_img=imgs, total=[len(boxes)])
            assert code == 0
            worst = max(worst, _compare_align(out, plan, imgs, _window(host), R, st, range(len(boxes))))
    _log(logdir, "roi_align_frames_unit_maps/%s" % TDT[st], dict(worst_err_over_bound=worst))


def test_roi_align_refuses_a_resolution_above_14():
    lib = _lib()
    dev, _ = _maps(rc.PYR_SMALL, 1, 0, 1)
    out = _nan((2, 15, 15, 256))
    _mark(out, 0)
    code, out = _run_align(lib, dev, rc.PYR_SMALL, 0, np.array([[0., 0., 40., 40.], [4., 4., 30., 20.]], np.float32), 15, 2,
                           roi_img=[0, 0], total=[2], out=out)
    assert code == E_INVALID and _untouched(out, 0)


def _big_case(st, n_img, logdir):
    lib = _lib()
    H, W = 1024, 2048                                    # x 256 channels: 2^29 elements per image
    try:
        base = torch.randn((H, W, 256), device="cuda", dtype=torch.float32)
        big = torch.empty((n_img, H, W, 256), device="cuda", dtype=TDT[st])
        for b in range(n_img):
            big[b].copy_(base)
        del base
    except torch.OutOfMemoryError as e:
        pytest.skip("cannot allocate a %d-image %s map of 2^29 elements per image on this device: %s" % (n_img, TDT[st], str(e)[:80]))
    dims = [(H, W), (8, 8), (8, 8), (8, 8)]
    rng = np.random.RandomState(7)
    bx = [[0., 0., 60., 60.], [8100., 4000., 8192., 4096.], [8000., 4040., 8400., 4070.], [4000., 2000., 4100., 2100.],
          [3., 3000., 423., 3024.], [3., 3100., 424., 3124.], [8150., 4090., 8192., 4096.], [7700., 4066., 8124., 4090.],
          [5000., 3., 5024., 427.], [100., 100., 400., 300.], [0., 0., 64., 64.]]
    for _ in range(21):
        x, y, w, h = rng.uniform(0, 8100), rng.uniform(0, 4000), rng.uniform(2, 100), rng.uniform(2, 100)
        bx.append([x, y, x + w, y + h])
    m = len(bx)
    boxes = np.array(bx * n_img, np.float32)
    imgs = np.repeat(np.arange(n_img), m)
    small = [torch.randn((1, 8, 8, 256), dtype=torch.float32).to(TDT[st]).repeat(n_img, 1, 1, 1).contiguous() for _ in range(3)]
    dev = [big] + [t.cuda() for t in small]
    host = [None] + [t.float().numpy() for t in small]

    def window(lv, img, y0, y1, x0, x1):
        if lv == 0:
            return big[img, y0:y1, x0:x1].float().cpu().numpy()          # only the window cells leave the device
        return host[lv][img, y0:y1, x0:x1]
    worst = 0.0
    for R in (7, 14):
        plan = rr.roi_align_plan(boxes, dims, rr.FPN_SCALES, R)
        assert sum(p["level"] == 0 for p in plan) >= 30 * n_img
        if R == 7:
            assert {p["form"] for p in plan} == {"sep", "direct"}
        code, out = _run_align(lib, dev, dims, st, boxes, R, len(boxes), roi_img=imgs, total=[len(boxes)])
        assert code == 0
        for b in range(1, n_img):
            diff = (_iv(out)[:m] != _iv(out)[b * m:(b + 1) * m]).flatten(1).any(dim=1).nonzero().flatten().tolist()
            assert not diff, ("image %d differs from image 0 on the same map and rois" % b, [_describe(plan[i], None, i) for i in diff[:4]])
        worst = max(worst, _compare_align(out, plan, imgs, window, R, st, range(len(boxes))))
    _log(logdir, "roi_align_above_2gib/%s" % TDT[st], dict(worst_err_over_bound=worst, images=n_img))


@pytest.mark.parametrize("st", [1, 2], ids=["bf16", "f16"])
def test_roi_align_16bit_map_above_2gib(st, logdir):
    """Two images of exactly 1 GiB each, the second a copy of the first: image 0 ends below 2 GiB and takes the buffer-descriptor
    branch, image 1 the pointer branch.  The same rois must give the same bits on both, and both must match the reference."""
    _big_case(st, 2, logdir)


def test_roi_align_f32_map_above_4gib(logdir):
    """Three f32 images of 2 GiB each; image 2 starts 4 GiB into the map."""
    _big_case(0, 3, logdir)


# ====================================================================================================== roi_align_c4
def _c4_boxes():
    """the edge boxes with the geometry they have on their FPN level, moved to a stride-16 map"""
    boxes, names = rc.align_edge_boxes()
    lv = rr.assign_levels(boxes)
    k = np.array([rr.FPN_SCALES[i] for i in lv], np.float32) * np.float32(16)
    return boxes * k[:, None], names


def _run_align_c4(lib, fd, H, W, Cc, boxes, R, n_max, roi_img=None, total=None, per_img=0, cnt=None, out=None, scale=0.0625):
    bd = _dev(np.asarray(boxes, np.float32))
    out = _nan((n_max, R, R, Cc)) if out is None else out
    ri, cn, tt = _ints(roi_img), _ints(cnt), _ints(total)
    code = lib.apse_k_roi_align_c4(_p(fd), H, W, Cc, scale, _p(bd), _p(ri), _p(cn), _p(tt), per_img, n_max, R, _p(out), _s())
    torch.cuda.synchronize()
    return code, out


@pytest.mark.parametrize("Cc", [256, 1024])
def test_roi_align_c4(Cc, logdir):
    lib = _lib()
    rng = np.random.RandomState(600 + Cc)
    # (a) the edge boxes, packed list with a short count, two images
    H, W = (160, 160) if Cc == 256 else (112, 112)
    feat = rng.standard_normal((2, H, W, Cc)).astype(np.float32)
    fd = _dev(feat)
    boxes, names = _c4_boxes()
    boxes = np.concatenate([boxes, rc.random_boxes(71, 12, W * 16., H * 16.)])
    n = len(boxes)
    imgs = np.arange(n) % 2
    win = lambda lv, img, y0, y1, x0, x1: feat[img, y0:y1, x0:x1]
    worst = 0.0
    for R in (7, 14):
        plan = rr.roi_align_plan(boxes, [(H, W)], [0.0625], R, levels=np.zeros(n, np.int64))
        if R == 7:
            assert {p["form"] for p in plan} == {"sep", "direct"}
        out = _nan((n, R, R, Cc))
        _mark(out, n - 2)
        code, out = _run_align_c4(lib, fd, H, W, Cc, boxes, R, n, roi_img=imgs, total=[n - 2], out=out)
        assert code == 0 and _untouched(out, n - 2)
        worst = max(worst, _compare_align(out, plan, imgs, win, R, 0, range(n - 2), C_=Cc, names=names, chunk=16))
    # (b) per-image mode on a small map
    h2, w2, per = 12, 21, 20
    feat2 = rng.standard_normal((4, h2, w2, Cc)).astype(np.float32)
    fd2 = _dev(feat2)
    cnt = [per, 0, 3, per - 1]
    b2 = rc.random_boxes(72, 4 * per)
    imgs2 = np.arange(4 * per) // per
    live = [r for r in range(4 * per) if r % per < cnt[r // per]]
    dead = [r for r in range(4 * per) if r % per >= cnt[r // per]]
    win2 = lambda lv, img, y0, y1, x0, x1: feat2[img, y0:y1, x0:x1]
    for R in (7, 14):
        plan = rr.roi_align_plan(b2, [(h2, w2)], [0.0625], R, levels=np.zeros(len(b2), np.int64))
        code, out = _run_align_c4(lib, fd2, h2, w2, Cc, b2, R, 4 * per, per_img=per, cnt=cnt)
        assert code == 0
        worst = max(worst, _compare_align(out, plan, imgs2, win2, R, 0, live, C_=Cc, chunk=16))
        assert bool((_iv(out)[torch.tensor(dead, device="cuda")] == 0).all())
    _log(logdir, "roi_align_c4/C%d" % Cc, dict(worst_err_over_bound=worst))


def test_roi_align_c4_many_rois_and_refusals(logdir):
    lib = _lib()
    rng = np.random.RandomState(610)
    H, W, n = 12, 21, 4200                                   # more rois than the 4096 blocks of the grid
    feat = rng.standard_normal((3, H, W, 256)).astype(np.float32)
    fd = _dev(feat)
    boxes = rc.random_boxes(73, n)
    imgs = (np.arange(n) * 2) % 3
    plan = rr.roi_align_plan(boxes, [(H, W)], [0.0625], 7, levels=np.zeros(n, np.int64))
    code, out = _run_align_c4(lib, fd, H, W, 256, boxes, 7, n, roi_img=imgs, total=[n])
    assert code == 0
    worst = _compare_align(out, plan, imgs, lambda lv, img, y0, y1, x0, x1: feat[img, y0:y1, x0:x1], 7, 0, range(n), chunk=1024)
    _log(logdir, "roi_align_c4_many", dict(worst_err_over_bound=worst))
    for Cc, R in ((128, 7), (384, 7), (256, 0), (256, 15)):
        out = _nan((2, max(R, 1), max(R, 1), 512))
        _mark(out, 0)
        code, out = _run_align_c4(lib, fd, H, W, Cc, boxes[:2], R, 2, roi_img=[0, 0], total=[2], out=out)
        assert code == E_INVALID and _untouched(out, 0), (Cc, R)


# ====================================================================================================== roi_pool
def _pool_boxes(scale, H, W, n_random, seed):
    boxes, names = rc.pool_edge_boxes(scale, H, W)
    rng = np.random.RandomState(seed)
    fw, fh = W / scale, H / scale
    x1, y1 = rng.uniform(-0.1 * fw, fw, n_random), rng.uniform(-0.1 * fh, fh, n_random)
    rnd = np.stack([x1, y1, x1 + rng.uniform(0, 0.6 * fw, n_random), y1 + rng.uniform(0, 0.6 * fh, n_random)], 1)
    return np.concatenate([boxes, rnd.astype(np.float32)]), names


@ST
@pytest.mark.parametrize("nchw", [0, 1])
@pytest.mark.parametrize("mode", ["list", "img0"])
def test_roi_pool_bit_exact(st, nchw, mode, logdir):
    """The max of the same cells (16-bit maps: of the widened values) is exact.  mode list: roi_img + *total (rows past it
    untouched); mode img0: roi_img == nullptr with image 1 of two and total == nullptr.  53 rois x R = 10: 5300 bins on a grid
    of 2048 blocks."""
    lib = _lib()
    H, W, scale = 48, 84, 0.25
    rng = np.random.RandomState(700 + st)
    t = torch.from_numpy(rng.standard_normal((2, H, W, 256)).astype(np.float32)).to(TDT[st])
    fd, feat = t.cuda(), t.float().numpy()
    boxes, _ = _pool_boxes(scale, H, W, 40, 701)
    n = len(boxes)
    bd = _dev(boxes)
    for R in (1, 7, 10):
        imgs = np.arange(n) % 2 if mode == "list" else np.ones(n, np.int64)
        nl = n - 3 if mode == "list" else n
        ref, empty = rr.roi_pool(feat, boxes, imgs, scale, R)
        assert empty.any() and not empty.all()
        out = _nan((n, 256, R, R) if nchw else (n, R, R, 256))
        _mark(out, nl)
        ri, tt = (_ints(imgs), _ints([nl])) if mode == "list" else (None, None)
        code = lib.apse_k_roi_pool(_p(fd), st, H, W, _p(bd), _p(ri), _p(tt), n, R, scale, _p(out), 1, nchw, _s())
        torch.cuda.synchronize()
        assert code == 0 and _untouched(out, nl)
        got = out[:nl].cpu().numpy().astype(np.float64)
        if nchw:
            got = got.transpose(0, 2, 3, 1)
        assert np.array_equal(got, ref[:nl])
    _log(logdir, "roi_pool/%s/nchw%d/%s" % (TDT[st], nchw, mode), dict(exact=True, rois=n))


@pytest.mark.parametrize("Cc", [256, 1024])
def test_roi_pool_c4_bit_exact(Cc, logdir):
    """90 rois x R = 10: 9000 bins on a grid of 8192 blocks."""
    lib = _lib()
    H, W, scale = 24, 40, 0.0625
    rng = np.random.RandomState(710 + Cc)
    feat = rng.standard_normal((2, H, W, Cc)).astype(np.float32)
    fd = _dev(feat)
    boxes, _ = _pool_boxes(scale, H, W, 77, 711)
    n = len(boxes)
    assert n * 100 > 8192
    imgs = np.arange(n) % 2
    bd, ri = _dev(boxes), _ints(imgs)
    for R, total in ((1, n), (7, n - 5), (10, n), (10, n + 9)):
        nl = min(total, n)
        ref, _ = rr.roi_pool(feat, boxes, imgs, scale, R)
        out = _nan((n, R, R, Cc))
        _mark(out, nl)
        tt = _ints([total])
        code = lib.apse_k_roi_pool_c4(_p(fd), H, W, Cc, _p(bd), _p(ri), _p(tt), n, R, scale, _p(out), _s())
        torch.cuda.synchronize()
        assert code == 0 and _untouched(out, nl)
        assert np.array_equal(out[:nl].cpu().numpy().astype(np.float64), ref[:nl])
    out = _nan((n, 7, 7, 384))
    _mark(out, 0)
    tt = _ints([n])
    assert lib.apse_k_roi_pool_c4(_p(fd), H, W, 384, _p(bd), _p(ri), _p(tt), n, 7, scale, _p(out), _s()) == E_INVALID
    torch.cuda.synchronize()
    assert _untouched(out, 0)
    _log(logdir, "roi_pool_c4/C%d" % Cc, dict(exact=True, rois=n))


# ====================================================================================================== mean_cells
@pytest.mark.parametrize("n", [1, 1000])
@pytest.mark.parametrize("Cc", [4, 1024, 2048])
@pytest.mark.parametrize("cells", [1, 49, 196])
def test_mean_cells(cells, Cc, n, logdir):
    """Bit-equal to the sequential ascending f32 sum, and inside the f64 bound."""
    lib = _lib()
    g = torch.Generator(device="cuda").manual_seed(800 + cells + Cc + n)
    xd = torch.randn((n, cells, Cc), device="cuda", generator=g)
    y = _nan((n, Cc))
    assert lib.apse_k_mean_cells(_p(xd), n, cells, Cc, _p(y), _s()) == 0
    torch.cuda.synchronize()
    x = xd.cpu().numpy()
    got = y.cpu().numpy()
    acc32 = np.zeros((n, Cc), np.float32)
    acc64, mag = np.zeros((n, Cc)), np.zeros((n, Cc))
    for k in range(cells):
        acc32 = acc32 + x[:, k]
        acc64 += x[:, k]
        mag += np.abs(x[:, k])
    assert acc32.dtype == np.float32
    assert np.array_equal(got.view(np.int32), (acc32 / np.float32(cells)).view(np.int32))
    ok, worst = rr.check(got, dict(ref=acc64 / cells, mag=mag / cells, n_ops=float(cells + 1)))
    assert ok, worst
    _log(logdir, "mean_cells/%d/%d/%d" % (cells, Cc, n), dict(worst_err_over_bound=worst, bit_equal_to_f32_order=True))


def test_mean_cells_refuses_a_channel_count_not_a_multiple_of_4():
    lib = _lib()
    xd = torch.zeros((2, 3, 8), device="cuda")
    y = _nan((2, 8))
    _mark(y, 0)
    assert lib.apse_k_mean_cells(_p(xd), 2, 4, 6, _p(y), _s()) == E_INVALID
    torch.cuda.synchronize()
    assert _untouched(y, 0)


# ====================================================================================================== mask_resize_bilinear
@pytest.mark.parametrize("shape", [((28, 28), (48, 84)), ((48, 84), (28, 28)), ((17, 23), (5, 40)), ((9, 9), (1, 7)), ((1, 1), (6, 5)),
                                   ((30, 40), (30, 40)), ((540, 960), (135, 240)), ((7, 5), (300, 301))], ids=str)
def test_mask_resize(shape, logdir):
    """Up- and down-scaling, non-integer ratios, OH = 1, a single-pixel mask, n = 3; values other than 0 / 1 count as 1."""
    lib = _lib()
    (H, W), (OH, OW) = shape
    rng = np.random.RandomState(900 + H + OW)
    m = ((rng.rand(3, H, W) < 0.5) * rng.randint(1, 256, (3, H, W))).astype(np.uint8)
    if H * W == 1:
        m[:] = [[[255]], [[0]], [[2]]]
    assert m.max() > 1
    out = _nan((3, OH, OW))
    md = _dev(m)                                            # every device input stays bound until after the synchronize
    assert lib.apse_k_mask_resize(_p(md), 3, H, W, OH, OW, _p(out), _s()) == 0
    torch.cuda.synchronize()
    ok, worst = rr.check(out.cpu().numpy(), rr.mask_resize(m, OH, OW))
    assert ok, worst
    _log(logdir, "mask_resize/%dx%d_to_%dx%d" % (H, W, OH, OW), dict(worst_err_over_bound=worst))


# ====================================================================================================== roi_align_masked
@ST
@pytest.mark.parametrize("SR", [1, 4])
def test_roi_align_masked(st, SR, logdir):
    """torchvision roi_align(aligned = False) of feat * mask on image 1 of two: boxes smaller than a cell (roi size clamped to 1),
    samples outside the map on every side, the whole map."""
    lib = _lib()
    H, W, scale = 48, 84, 0.25
    rng = np.random.RandomState(1000 + st)
    t = torch.from_numpy(rng.standard_normal((2, H, W, 256)).astype(np.float32)).to(TDT[st])
    fd, feat = t.cuda(), t.float().numpy()
    boxes = np.array([[8., 8., 60., 70.], [10., 10., 10.5, 10.2], [100.3, 40.7, 101.1, 44.], [-20., -12., 30., 40.], [300., 150., 400., 260.],
                      [0., 0., 336., 192.], [-60., 20., -8., 60.], [340., 20., 420., 90.], [33.3, 171.9, 290.1, 191.9], [50., 50., 50., 50.],
                      [120., -30., 200., -6.], [64., 64., 32., 32.]], np.float32)
    n = len(boxes)
    mask = (rng.rand(n, H, W) < 0.7).astype(np.float32) * rng.rand(n, H, W).astype(np.float32)
    worst = 0.0
    for R in (7, 10):
        res = rr.roi_align_masked(feat[1], mask, boxes, scale, R, SR)
        assert (res["mag"].reshape(n, -1).max(axis=1) == 0).any() and (res["mag"].reshape(n, -1).max(axis=1) > 0).any()
        out = _nan((n, 256, R, R))
        bd, mk = _dev(boxes), _dev(mask)                    # bound until after the synchronize
        assert lib.apse_k_roi_align_masked(_p(fd), st, H, W, 1, _p(bd), _p(mk), n, R, SR, scale, _p(out), _s()) == 0
        torch.cuda.synchronize()
        ok, w = rr.check(out.cpu().numpy(), res)
        assert ok, w
        worst = max(worst, w)
    _log(logdir, "roi_align_masked/%s/SR%d" % (TDT[st], SR), dict(worst_err_over_bound=worst))


# ====================================================================================================== l2_normalize, sqdist
@pytest.mark.parametrize("D", [64, 100, 128, 256])
def test_l2_normalize_rows(D, logdir):
    lib = _lib()
    rng = np.random.RandomState(1100 + D)
    n_max, total = 37, 29
    x = (rng.standard_normal((n_max, D)) * rng.uniform(0.01, 30, (n_max, 1))).astype(np.float32)
    x[5] = 0
    res = rr.l2_normalize(x)
    xd = _dev(x)
    worst = 0.0
    for tt, nl in ((_ints([total]), total), (None, n_max), (_ints([n_max + 4]), n_max)):
        y = _nan((n_max, D))
        _mark(y, nl)
        assert lib.apse_k_l2_normalize(_p(xd), _p(y), D, _p(tt), n_max, _s()) == 0
        torch.cuda.synchronize()
        got = y[:nl].cpu().numpy()
        assert _untouched(y, nl) and not np.isnan(got).any() and (got[5] == 0).all()
        ok, w = rr.check(got, dict(ref=res["ref"][:nl], mag=res["mag"][:nl], n_ops=res["n_ops"]))
        assert ok, w
        worst = max(worst, w)
    _log(logdir, "l2_normalize/D%d" % D, dict(worst_err_over_bound=worst))


@pytest.mark.parametrize("D", [64, 100, 128, 256])
@pytest.mark.parametrize("ON", [(1, 1), (7, 100), (300, 5)], ids=str)
def test_sqdist_matrix(ON, D, logdir):
    lib = _lib()
    O, N = ON
    rng = np.random.RandomState(1200 + D + O)
    a, b = rng.standard_normal((O, D)).astype(np.float32), rng.standard_normal((N, D)).astype(np.float32)
    if N > 1:
        b[0] = a[0]                                       # a zero distance (not in the 1 x 1 case: a and b must differ there)
    out = _nan((O, N))
    ad, bd = _dev(a), _dev(b)                               # bound until after the synchronize
    assert lib.apse_k_sqdist(_p(ad), _p(bd), O, N, D, _p(out), _s()) == 0
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    ok, worst = rr.check(got, rr.sqdist(a, b))
    assert ok and (N == 1 or got[0, 0] == 0), worst
    _log(logdir, "sqdist/%dx%d/D%d" % (O, N, D), dict(worst_err_over_bound=worst))


# ====================================================================================================== assoc_fc
@pytest.mark.parametrize("K", [128, 1280, 25600])
@pytest.mark.parametrize("N", [64, 128, 256])
def test_assoc_fc(N, K, logdir):
    """Linear(K -> N) + F.normalize over live rows in {0, 1, 15, 16, 17, 100} of n_max = 100 (around the 16-row matrix chunk), with
    and without bias: raw and y inside their bounds, rows of raw / y / the slice workspace past the count untouched, two calls
    bit-identical."""
    lib = _lib()
    rng = np.random.RandomState(1300 + N + K)
    n_max, slices = 100, K // 128
    x = rng.standard_normal((n_max, K)).astype(np.float32)
    w = (rng.standard_normal((N, K)) / np.sqrt(K)).astype(np.float32)
    bias = rng.standard_normal(N).astype(np.float32)
    assert lib.apse_assoc_fc_ok(K, N)
    xd, wd, bd = _dev(x), _dev(w), _dev(bias)
    worst_raw = worst_y = 0.0
    for use_bias in (True, False):
        res = rr.assoc_fc(x, w, bias if use_bias else None)
        assert np.isfinite(res["y_bound"]).all()
        for live in (0, 1, 15, 16, 17, 100):
            outs = []
            for _ in range(2):
                ws = _nan((slices, n_max, N))
                _iv(ws)[:, live:] = SENT32
                raw, y = _nan((n_max, N)), _nan((n_max, N))
                _mark(raw, live)
                _mark(y, live)
                tt = _ints([live])
                code = lib.apse_k_assoc_fc(_p(xd), _p(wd), _p(bd if use_bias else None), _p(ws), _p(tt), n_max, K, N, _p(raw),
                                           _p(y), _s())
                torch.cuda.synchronize()
                assert code == 0 and _untouched(raw, live) and _untouched(y, live)
                assert bool((_iv(ws)[:, live:] == SENT32).all()) and not bool(torch.isnan(ws[:, :live]).any())
                outs.append((raw, y))
            assert torch.equal(_iv(outs[0][0]), _iv(outs[1][0])) and torch.equal(_iv(outs[0][1]), _iv(outs[1][1]))
            ok, wr = rr.check(raw[:live].cpu().numpy(), dict(ref=res["ref"][:live], mag=res["mag"][:live], n_ops=res["n_ops"]))
            assert ok, (live, use_bias, wr)
            ok, wy = rr.check(y[:live].cpu().numpy(), dict(ref=res["y"][:live]), b=res["y_bound"][:live])
            assert ok, (live, use_bias, wy)
            worst_raw, worst_y = max(worst_raw, wr), max(worst_y, wy)
    _log(logdir, "assoc_fc/N%d/K%d" % (N, K), dict(worst_err_over_bound_raw=worst_raw, worst_err_over_bound_y=worst_y))


def test_assoc_fc_refuses_ineligible_shapes():
    lib = _lib()
    for K, N in ((130, 128), (1280, 96)):
        assert not lib.apse_assoc_fc_ok(K, N)
        xd, wd = torch.zeros((4, 1280), device="cuda"), torch.zeros((128, 1280), device="cuda")
        ws, raw, y = _nan((10, 4, 128)), _nan((4, 128)), _nan((4, 128))
        for t in (ws, raw, y):
            _mark(t, 0)
        tt = _ints([4])
        assert lib.apse_k_assoc_fc(_p(xd), _p(wd), None, _p(ws), _p(tt), 4, K, N, _p(raw), _p(y), _s()) == E_INVALID
        torch.cuda.synchronize()
        assert _untouched(ws, 0) and _untouched(raw, 0) and _untouched(y, 0)
