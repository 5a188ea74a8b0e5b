"""GPU tests (-m gpu): the RLE encoder of csrc/rle_encode.hip (apse_mots_bits_to_rle, apse_mots_rle_pack) and
utils/rle_device.encode_masks against the host codec utils/rle.py.  Every case checks the run ends, the counts, the compressed
string and chars_off exactly, and that apse_mots_rle_to_bits of the emitted ends gives the input pixels back.  Frames too large
to make dense use tests/rle_ref.ends_from_window, which tests/test_rle_ref.py pins to the codec."""
import ctypes as C

import numpy as np
import pytest
import torch

import rle_ref
from apse_uav_amd import _lib
from apse_uav_amd.structures.window_mask import WindowMask
from apse_uav_amd.utils import mots_eval as me
from apse_uav_amd.utils import rle, rle_device

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
SEG = rle_device.SEG_ROWS
GUARD = 16
SENTINEL = -7
FRAMES = [(30, 150), (375, 1242), (2160, 3840)]
INVALID = -1


class Obj:
    """One test window: bool pixels (None: NULL bits), rect, and how its words are laid out."""

    def __init__(self, win, rect, garbage=None, extra_words=0):
        self.win, self.rect, self.garbage, self.extra = win, tuple(int(v) for v in rect), garbage, extra_words
        self.words = None
        if win is not None and rect[2] > rect[0] and rect[3] > rect[1]:
            self.words = rle_ref.pack_words(win, self.rect, garbage, extra_words)


def upload(objs):
    """-> (host MotsWindow array, device struct tensor, pool tensor, word offsets)."""
    n = len(objs)
    arr = (_lib.MotsWindow * max(n, 1))()
    chunks, offs, off = [], [], 0
    for o in objs:
        offs.append(off)
        if o.words is not None:
            chunks.append(o.words.reshape(-1))
            off += o.words.size
    flat = np.concatenate(chunks) if chunks else np.zeros(1, np.uint64)
    pool = torch.from_numpy(flat.view(np.int64).copy()).to(DEV)
    for k, o in enumerate(objs):
        x0, y0, x1, y1 = o.rect
        arr[k].rect[:] = list(o.rect)
        arr[k].words_per_row = o.words.shape[1] if o.words is not None else \
            ((((x1 + 63) >> 6) - (x0 >> 6)) if x1 > x0 and y1 > y0 else 0)
        arr[k].area = 0
        arr[k].bits = pool.data_ptr() + 8 * offs[k] if o.words is not None else None
    host = np.frombuffer(bytes(arr), np.uint8).reshape(-1, C.sizeof(_lib.MotsWindow))[:n]
    return arr, torch.from_numpy(host.copy()).to(DEV), pool, offs


def run_rle(objs, h, w, cap, chars_cap):
    """The two entry points with guarded outputs -> dict of host arrays (ends and chars include their guard words)."""
    lib = _lib.load()
    n = len(objs)
    arr, windows, pool, _ = upload(objs)
    ws_bytes = lib.apse_mots_rle_workspace_bytes(arr, n, h, w)
    assert ws_bytes > 0
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=DEV)
    ends = torch.full((cap + GUARD,), SENTINEL, dtype=torch.int32, device=DEV)
    ends_off = torch.full((n + 1,), SENTINEL, dtype=torch.int32, device=DEV)
    info = torch.full((4,), SENTINEL, dtype=torch.int32, device=DEV)
    chars = torch.full((chars_cap + GUARD,), 255, dtype=torch.uint8, device=DEV)
    chars_off = torch.full((n + 1,), SENTINEL, dtype=torch.int32, device=DEV)
    st = _lib.stream_ptr()
    rc = lib.apse_mots_bits_to_rle(_lib.ptr(windows), arr, n, h, w, _lib.ptr(ends), cap, _lib.ptr(ends_off), _lib.ptr(info),
                                   _lib.ptr(ws), ws_bytes, st)
    assert rc == 0
    pws_bytes = lib.apse_mots_rle_pack_workspace_bytes(cap)
    pws = torch.empty(pws_bytes, dtype=torch.uint8, device=DEV)
    rc = lib.apse_mots_rle_pack(_lib.ptr(ends), _lib.ptr(ends_off), n, cap, _lib.ptr(chars), chars_cap, _lib.ptr(chars_off),
                                _lib.ptr(info[2:]), _lib.ptr(pws), pws_bytes, st)
    assert rc == 0
    torch.cuda.synchronize()
    return dict(ends=ends.cpu().numpy(), ends_off=ends_off.cpu().numpy(), info=info.cpu().numpy(),
                chars=chars.cpu().numpy(), chars_off=chars_off.cpu().numpy(), ends_dev=ends, ends_off_dev=ends_off,
                keep=(pool, windows))


def expected(objs, h, w, dense_check):
    """Per object: run ends (int64), counts, string.  ``dense_check``: also prove the ends against the codec on the dense frame."""
    out = []
    for o in objs:
        e = rle_ref.ends_from_window(o.win if o.words is not None else None, o.rect, h, w)
        counts = np.diff(e, prepend=0).tolist()
        if dense_check:
            assert counts == rle.counts_from_mask(rle_ref.dense(o.win if o.words is not None else None, o.rect, h, w))
        out.append((e, counts, rle.counts_to_string(counts)))
    return out


def round_trip(objs, h, w, res):
    """apse_mots_rle_to_bits of the emitted ends, into fresh windows of the same rects == the input pixels."""
    lib = _lib.load()
    n = len(objs)
    clean = [Obj(o.win if o.words is not None else None, o.rect) for o in objs]
    arr, windows, pool, offs = upload(clean)
    pool.fill_(0x5555555555555555)
    rc = lib.apse_mots_rle_to_bits(_lib.ptr(res["ends_dev"]), _lib.ptr(res["ends_off_dev"]), n, h, w, _lib.ptr(windows),
                                   _lib.stream_ptr())
    assert rc == 0
    back = pool.cpu().numpy().view(np.uint64)
    for k, o in enumerate(clean):
        if o.words is None:
            continue
        words = back[offs[k]:offs[k] + o.words.size].reshape(o.words.shape)
        assert np.array_equal(rle_ref.unpack_words(words, o.rect), o.win), (k, o.rect)


def check(objs, h, w, dense_check=True, trip=True):
    want = expected(objs, h, w, dense_check)
    need = sum(len(e) for e, _, _ in want)
    nbytes = sum(len(s) for _, _, s in want)
    res = run_rle(objs, h, w, need, nbytes)                  # exact capacities: the guards prove nothing runs past them
    assert res["info"].tolist() == [need, 1, nbytes, 1]
    assert res["ends_off"].tolist() == np.cumsum([0] + [len(e) for e, _, _ in want]).tolist()
    assert res["chars_off"].tolist() == np.cumsum([0] + [len(s) for _, _, s in want]).tolist()
    assert (res["ends"][need:] == SENTINEL).all() and (res["chars"][nbytes:] == 255).all()
    for k, (e, counts, s) in enumerate(want):
        a, b = res["ends_off"][k], res["ends_off"][k + 1]
        got = res["ends"][a:b].astype(np.int64)
        assert got.tolist() == e.tolist(), (k, objs[k].rect)
        assert np.diff(got, prepend=0).tolist() == counts
        ca, cb = res["chars_off"][k], res["chars_off"][k + 1]
        assert res["chars"][ca:cb].tobytes().decode("ascii") == s, (k, objs[k].rect)
    if trip:
        round_trip(objs, h, w, res)
    return res


def blob(g, rows, cols, p=0.8):
    """A blob-like window: a filled ellipse with noise at density p."""
    yy, xx = np.mgrid[0:rows, 0:cols]
    inside = ((yy - (rows - 1) / 2) / max(rows / 2, 1)) ** 2 + ((xx - (cols - 1) / 2) / max(cols / 2, 1)) ** 2 <= 1.0
    return inside & (g.random((rows, cols)) < p)


def frame_cases(h, w, g):
    """The named widths and heights are clipped to the frame: at 30 x 150 the 129 px windows at phases 1 and 63 end at the right
    edge and every height above 30 collapses to 30 rows.  The two larger frames hold all of them as named."""
    one = np.ones((1, 1), bool)
    objs = [Obj(None, (0, 0, 0, 0)), Obj(None, (3, 2, min(w, 9), min(h, 7))),          # empty rect, NULL bits
            Obj(np.zeros((min(h, 5), 4), bool), (1, 0, 5, min(h, 5)))]                  # bits without a set pixel
    objs += [Obj(one, (x, y, x + 1, y + 1)) for x, y in ((0, 0), (w - 1, h - 1), (0, h - 1), (w - 1, 0))]
    objs.append(Obj(np.ones((h, w), bool), (0, 0, w, h)))                                 # whole frame: ends [0, h * w]
    for wd in (1, 63, 64, 65, 129):                                                       # widths x word phases, garbage outside
        for phase in (0, 1, 63):
            x0 = phase + (64 if phase + 64 + wd <= w else 0)
            x1 = min(x0 + wd, w)
            y0 = int(g.integers(0, h - 1))
            y1 = min(h, y0 + int(g.integers(1, 40)))
            objs.append(Obj(g.random((y1 - y0, x1 - x0)) < 0.6, (x0, y0, x1, y1), garbage=g, extra_words=int(phase == 1)))
    for x0 in (5, w - 2):                                                                 # full-height windows over the seam
        for bottom, top in ((1, 1), (1, 0), (0, 1)):
            win = np.zeros((h, 2), bool)
            win[h - 1, 0], win[0, 1] = bottom, top
            win[h // 2, :] = True
            objs.append(Obj(win, (x0, 0, x0 + 2, h), garbage=g))
    for hh in (1, SEG - 1, SEG, SEG + 1, 3 * SEG + 5):                                    # heights around the row segment
        hh = min(hh, h)
        for y0 in (0, h - hh, (h - hh) // 2):
            x0 = int(g.integers(0, w - 1))
            x1 = min(w, x0 + int(g.integers(1, 70)))
            objs.append(Obj(g.random((hh, x1 - x0)) < 0.5, (x0, y0, x1, y0 + hh), garbage=g))
    return objs


@pytest.mark.parametrize("hw", FRAMES)
def test_windows_equal_codec(hw):
    h, w = hw
    g = np.random.default_rng(h * 7 + w)
    objs = frame_cases(h, w, g)
    if h * w <= 375 * 1242:
        res = check(objs, h, w, dense_check=True)
    else:                                                    # dense codec on a few, the window-only helper on all
        expected([objs[3], objs[4], objs[7], objs[12]], h, w, True)
        res = check(objs, h, w, dense_check=False)
    k = 7                                                    # the whole-frame mask
    assert res["ends"][res["ends_off"][k]:res["ends_off"][k + 1]].tolist() == [0, h * w]
    again = run_rle(objs, h, w, int(res["info"][0]), int(res["info"][2]))
    assert np.array_equal(again["ends"], res["ends"]) and np.array_equal(again["chars"], res["chars"])   # run to run


def test_checkerboard_capacity_protocol():
    h, w = 64, 70
    yy, xx = np.mgrid[0:h, 0:w]
    objs = [Obj((yy + xx) % 2 == 0, (0, 0, w, h)), Obj((yy + xx) % 2 == 1, (0, 0, w, h))]
    res = check(objs, h, w)
    need, nbytes = int(res["info"][0]), int(res["info"][2])
    # every pixel is a run, except that h is even: the bottom pixel of a column and the top pixel of the next are equal and
    # share a run (w - 1 seams per board); one board starts with the empty zeros run
    assert need == 2 * (h * w - (w - 1)) + 1
    short = run_rle(objs, h, w, need - 1, nbytes)            # one end short: nothing written, the need reported
    assert short["info"].tolist() == [need, 0, -1, 0]
    assert (short["ends"] == SENTINEL).all() and (short["chars"] == 255).all()
    assert short["ends_off"].tolist() == res["ends_off"].tolist()
    short = run_rle(objs, h, w, need, nbytes - 1)            # one byte short
    assert short["info"].tolist() == [need, 1, nbytes, 0]
    assert np.array_equal(short["ends"], res["ends"]) and (short["chars"] == 255).all()
    assert short["chars_off"].tolist() == res["chars_off"].tolist()
    retry = run_rle(objs, h, w, int(short["info"][0]), int(short["info"][2]))
    assert np.array_equal(retry["ends"], res["ends"]) and np.array_equal(retry["chars"], res["chars"])


@pytest.mark.parametrize("n", [1, 7, 100])
def test_many_objects_in_one_call(n):
    h, w = 375, 1242
    g = np.random.default_rng(n)
    objs = []
    for k in range(n):
        if n > 1 and k % 5 == 3:
            objs.append(Obj(None, (0, 0, 0, 0)) if k % 2 else Obj(None, (10, 10, 40, 30)))
            continue
        rows, cols = int(g.integers(1, 120)), int(g.integers(1, 200))
        x0, y0 = int(g.integers(0, w - cols + 1)), int(g.integers(0, h - rows + 1))
        objs.append(Obj(blob(g, rows, cols, 0.95), (x0, y0, x0 + cols, y0 + rows)))
    check(objs, h, w, dense_check=n <= 7)


def test_largest_frame_corners():
    h, w = 32768, 49152
    g = np.random.default_rng(9)
    far = g.random((70, 5)) < 0.6
    far[-1, -1] = True                                       # the last pixel of the frame
    near = g.random((70, 5)) < 0.6
    near[0, 0] = True
    wide = g.random((5, 70)) < 0.6
    objs = [Obj(far, (w - 5, h - 70, w, h)), Obj(near, (0, 0, 5, 70)), Obj(wide, (w - 70, h - 5, w, h), garbage=g)]
    res = check(objs, h, w, dense_check=False)
    want = expected(objs, h, w, False)
    counts = want[0][1]
    assert want[0][0][0] > 1.6e9 and len(rle.counts_to_string(counts[:1])) == 7         # ends near 1.6e9, a 7-byte value
    assert any(counts[i] - counts[i - 2] < 0 for i in range(3, len(counts)))            # negative differences occur
    assert res["info"][1] == 1


def test_invalid_arguments_launch_nothing():
    lib = _lib.load()
    h, w = 30, 150
    st = _lib.stream_ptr()
    ends = torch.full((64,), SENTINEL, dtype=torch.int32, device=DEV)
    off = torch.full((4,), SENTINEL, dtype=torch.int32, device=DEV)
    info = torch.full((2,), SENTINEL, dtype=torch.int32, device=DEV)
    ws = torch.empty(1 << 16, dtype=torch.uint8, device=DEV)
    good = [Obj(np.ones((3, 3), bool), (1, 1, 4, 4))]
    arr, windows, pool, _ = upload(good)

    def call(arr_, windows_, n, hh, ww, ends_=ends, off_=off, info_=info, ws_=ws):
        return lib.apse_mots_bits_to_rle(_lib.ptr(windows_), arr_, n, hh, ww, _lib.ptr(ends_), 64, _lib.ptr(off_),
                                         _lib.ptr(info_), _lib.ptr(ws_), ws.numel() if ws_ is not None else 0, st)

    for rect in ((148, 1, 151, 4), (1, 28, 4, 31), (-1, 1, 4, 4), (1, -2, 4, 4)):      # a rect outside the frame
        bad = [Obj(np.ones((rect[3] - rect[1], rect[2] - rect[0]), bool), rect)]
        barr, bwin, bpool, _ = upload(bad)
        assert call(barr, bwin, 1, h, w) == INVALID
        assert lib.apse_mots_rle_workspace_bytes(barr, 1, h, w) == 0
    narrow, nwin, npool, _ = upload([Obj(np.ones((2, 70), bool), (60, 1, 130, 3))])
    narrow[0].words_per_row = 2                              # the rect needs three words
    assert call(narrow, nwin, 1, h, w) == INVALID
    assert call(arr, windows, rle_device.MAX_OBJECTS + 1, h, w) == INVALID
    assert call(arr, windows, -1, h, w) == INVALID
    assert call(arr, windows, 1, 0, w) == INVALID and call(arr, windows, 1, 32769, w) == INVALID
    assert call(arr, None, 1, h, w) == INVALID and call(None, windows, 1, h, w) == INVALID
    assert call(arr, windows, 1, h, w, off_=None) == INVALID and call(arr, windows, 1, h, w, info_=None) == INVALID
    assert call(arr, windows, 1, h, w, ends_=None) == INVALID and call(arr, windows, 1, h, w, ws_=None) == INVALID
    assert lib.apse_mots_bits_to_rle(_lib.ptr(windows), arr, 1, h, w, _lib.ptr(ends), 64, _lib.ptr(off), _lib.ptr(info),
                                     _lib.ptr(ws), 8, st) == INVALID                     # a workspace below the query
    assert call(arr, windows, 0, h, w) == 0                  # n == 0: a no-op
    pws = torch.empty(lib.apse_mots_rle_pack_workspace_bytes(64), dtype=torch.uint8, device=DEV)
    chars = torch.full((64,), 255, dtype=torch.uint8, device=DEV)
    for n_, ends_, off_ in ((rle_device.MAX_OBJECTS + 1, ends, off), (-1, ends, off), (1, None, off), (1, ends, None)):
        assert lib.apse_mots_rle_pack(_lib.ptr(ends_), _lib.ptr(off_), n_, 64, _lib.ptr(chars), 64, _lib.ptr(off),
                                      _lib.ptr(info), _lib.ptr(pws), pws.numel(), st) == INVALID
    assert lib.apse_mots_rle_pack(_lib.ptr(ends), _lib.ptr(off), 1, 64, _lib.ptr(chars), 64, _lib.ptr(off), _lib.ptr(info),
                                  _lib.ptr(pws), 8, st) == INVALID
    torch.cuda.synchronize()
    assert (ends.cpu() == SENTINEL).all() and (off.cpu() == SENTINEL).all() and (info.cpu() == SENTINEL).all()
    assert (chars.cpu() == 255).all()


def _window_mask(o, h, w):
    bits = torch.from_numpy(o.words.view(np.int64).copy()).to(DEV) if o.words is not None else None
    return WindowMask(bits, o.rect, (h, w), (-1, -1), int(o.win.sum()) if o.words is not None else 0)


@pytest.mark.parametrize("hw", FRAMES[:2])
def test_encode_masks_equals_rle_encode(hw):
    h, w = hw
    g = np.random.default_rng(w)
    objs = frame_cases(h, w, g)
    masks = [_window_mask(o, h, w) for o in objs]
    want = [rle.encode(rle_ref.dense(o.win if o.words is not None else None, o.rect, h, w)) for o in objs]
    assert rle_device.encode_masks(masks, (h, w)) == want
    plain = rle_device.encode_masks(masks, (h, w), compressed=False)
    assert [r["counts"] for r in plain] == [rle.string_to_counts(r["counts"]) for r in want]
    assert all(r["size"] == [h, w] for r in plain)
    assert rle_device.encode_masks([], (h, w)) == []
    yy, xx = np.mgrid[0:h, 0:w]                              # far more runs than the first capacity guess: the second round
    board = Obj((yy + xx) % 2 == 0, (0, 0, w, h))
    assert rle_device.encode_masks([_window_mask(board, h, w)], (h, w)) == [rle.encode(board.win)]


def test_encode_masks_takes_split_idmap_windows():
    h, w = 37, 131
    g = np.random.default_rng(3)
    img = np.zeros((h, w), np.uint16)
    for v in (1001, 1002, 2001, 10000):
        x0, y0 = int(g.integers(0, w - 20)), int(g.integers(0, h - 10))
        img[y0:y0 + 10, x0:x0 + 20] = np.where(g.random((10, 20)) < 0.7, v, img[y0:y0 + 10, x0:x0 + 20])
    values, windows, pool = me.split_idmap(torch.from_numpy(img).to(DEV))
    got = rle_device.encode_masks(windows, (h, w), count=len(values))
    assert got == [rle.encode(img == v) for v in values]
