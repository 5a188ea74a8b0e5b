"""numpy restatement of the association metrics that need no association head (DESIGN.md "Association metrics"): the mask
translate / crop and centroid-aligned IoU of dcnn/utils/mask_utils.py:41-77 on dense masks, and the two greedy loops of
dcnn/engines/rcnn_tracker.py:91-120 over plain lists, with the track store's ageing and deletion."""
import numpy as np

MASKS_IOU_THRESHOLD = 0.7
UNDETECTED_FRAMES_TH = 100


def translate_and_crop(mask, vec):
    """Pixel (x, y) moves to (x + int(dx), y + int(dy)); zero fill; cropped to the frame."""
    H, W = mask.shape
    dx, dy = int(vec[0]), int(vec[1])
    out = np.zeros_like(mask)
    ys, xs = np.nonzero(mask)
    ys, xs = ys + dy, xs + dx
    ok = (ys >= 0) & (ys < H) & (xs >= 0) & (xs < W)
    out[ys[ok], xs[ok]] = True
    return out


def centroid(mask):
    """get_mask_centroid: 1-based, floor of the mean of the set coordinates; (nan, nan) for an empty mask."""
    ys, xs = np.nonzero(mask)
    if len(xs) == 0:
        return (float("nan"), float("nan"))
    return (float(int((xs + 1).sum()) // len(xs)), float(int((ys + 1).sum()) // len(ys)))


def shift_counts(a, b, dx, dy):
    """(|T(a) & b|, |T(a)|, |b|)"""
    t = translate_and_crop(a, (dx, dy))
    return int((t & b).sum()), int(t.sum()), int(b.sum())


def iou_f32(inter, area_t, area_b):
    union = area_t + area_b - inter
    if union <= 0:
        return np.float32(0.0)
    return np.float32(inter) / np.float32(union)


def masks_iou(det, obj, det_centroid=None):
    """compute_masks_iou as a Python float; 0.0 when either mask is empty."""
    oc = centroid(obj)
    dc = centroid(det) if det_centroid is None else det_centroid
    dx, dy = oc[0] - dc[0], oc[1] - dc[1]
    if dx != dx or dy != dy:
        return 0.0
    return float(iou_f32(*shift_counts(det, obj, int(dx), int(dy))))


class Store:
    """ObjectInstances reduced to what the id bookkeeping reads: per object its id, the frames since it was seen, whether it
    was seen this frame, and the payload (mask or box) the metric compares against."""

    def __init__(self):
        self.ids, self.since, self.seen, self.payload = [], [], [], []
        self.next_id = 1

    def add(self, payload):
        self.ids.append(self.next_id)
        self.next_id += 1
        self.since.append(0)
        self.seen.append(True)
        self.payload.append(payload)

    def associate(self, k, payload):
        self.since[k] = 0
        self.seen[k] = True
        self.payload[k] = payload

    def finish(self):
        """delete_undetected_objects, get_recent_objects, finish_association -> ids seen this frame in store order."""
        keep = [k for k in range(len(self.ids)) if not self.since[k] > UNDETECTED_FRAMES_TH]
        for name in ("ids", "since", "seen", "payload"):
            setattr(self, name, [getattr(self, name)[k] for k in keep])
        recent = [i for i, s in zip(self.ids, self.seen) if s]
        self.since = [0 if s else n + 1 for s, n in zip(self.seen, self.since)]
        self.seen = [False] * len(self.ids)
        return recent


def assign_mask_iou(store, det_masks, iou=masks_iou):
    """The 'mask_iou' branch (rcnn_tracker.py:108-120) -> the id each detection ends up with."""
    ids = []
    for m in det_masks:
        k = -1
        if len(store.ids) > 0:
            ious = [iou(m, o) for o in store.payload]
            k = int(np.argmax(ious))
            if not ious[k] >= MASKS_IOU_THRESHOLD:
                k = -1
        if k >= 0:
            store.associate(k, m)
        else:
            store.add(m)
        ids.append(store.ids[k])
    return ids


def step_mask_iou(store, det_masks, iou=masks_iou):
    """One frame -> ids seen this frame, in store order."""
    assign_mask_iou(store, det_masks, iou)
    return store.finish()


def box_center(box):
    b = np.asarray(box, np.float32)
    return (b[:2] + b[2:]) / np.float32(2)


def step_bbox_center_dist(store, det_boxes, threshold):
    """One frame of the 'bbox_center_dist' branch (rcnn_tracker.py:91-106) -> ids seen this frame."""
    for box in det_boxes:
        c = box_center(box)
        hit = False
        for k in range(len(store.ids)):
            d = c - box_center(store.payload[k])
            if float((d * d).sum(dtype=np.float32)) < threshold:
                hit = True
                store.associate(k, box)
        if not hit:
            store.add(box)
    return store.finish()


# ---------------------------------------------------------------- the scripted sequence of the GPU test
SCRIPT_FRAME = (270, 480)
SCRIPT_FRAMES = 8


def scripted_rects(t):
    """Rectangles (x0, y0, x1, y1) detected in frame t, in detection order, each with its name."""
    out = [("mover", (20 + 2 * t, 30, 60 + 2 * t, 60))]                       # 40 x 30, 2 px per frame
    if t not in (3, 4, 5):
        out.append(("returner", (200, 100, 250, 140)))                        # 50 x 40, absent for three frames
    out.append(("grower", (300, 150, 330, 170 if t < 4 else 186)))            # 30 wide, 20 rows -> 36 rows at frame 4
    if t >= 5:
        out.append(("late", (100, 200, 120, 250)))                            # 20 x 50, from frame 5
    return out


def rect_mask(rect, frame=SCRIPT_FRAME):
    m = np.zeros(frame, bool)
    m[rect[1]:rect[3], rect[0]:rect[2]] = True
    return m


def scripted_expected():
    """[{name: id} per frame] from the restatement."""
    store = Store()
    out = []
    for t in range(SCRIPT_FRAMES):
        rects = scripted_rects(t)
        ids = assign_mask_iou(store, [rect_mask(r) for _, r in rects])
        store.finish()
        out.append({name: i for (name, _), i in zip(rects, ids)})
    return out
