"""RPNHead -- the trainable counterpart of detectron2's StandardRPNHead (FPN models: one 3 x 3 convolution + ReLU shared by p2 .. p6,
then the 1 x 1 ``objectness_logits`` (3 anchors) and ``anchor_deltas`` (12) layers), with ``loss_rpn_cls`` and ``loss_rpn_loc`` of
RPNOutputs.losses (detectron2 0.1.2), as dcnn/scripts/train/finetune_uav.py fine-tunes them on a frozen backbone.

RPNOutputs.losses reads the head's outputs only at the anchors that ``subsample_labels`` kept (at most 256 per image), so the loss
and every parameter gradient are functions of the 3 x 3 x 256 input patches at those positions.  With the patches gathered as rows
``X [S][2304]`` in the checkpoint's (c, kh, kw) order (``apse_rpn_patches`` / ``TrackRCNN.rpn_patches``) the head is three FC layers:

    X -> conv [256][2304] + ReLU -> objectness_logits [3][256] | anchor_deltas [12][256]

They run on the box trainer's MFMA GEMM entries (csrc/box_train.hip) with the checkpoint's tensors as they are; the loss and its
gradient are csrc/rpn_train.hip.  This is the dense five-level loss itself, not an approximation of it.  The parameters are f32
leaf tensors on the device under detectron2's names and shapes (``conv.weight`` [256][256][3][3], ``objectness_logits.weight``
[3][256][1][1], ``anchor_deltas.weight`` [12][256][1][1]); ``torch.optim.SGD`` and ``apse_uav_amd.optim.SGD`` both update them in
place.  There is no CPU path and no gradient for the patches: the FPN maps are frozen.
"""
import ctypes as C

import torch

from .. import _lib
from . import box_head as bh
from .head_base import TrainableHead, _check, workspace_tensor

PREFIX = "proposal_generator.rpn_head."
CONV_DIM = 256
PATCH = CONV_DIM * 9
NUM_ANCHORS = 3
MAX_ROWS = bh.MAX_ROIS     # APSE_BOX_TRAIN_MAX_N: rows of one step (256 per image x at most 4 images)
NAMES = ["conv", "objectness_logits", "anchor_deltas"]
SHAPES = {
    "conv.weight": (CONV_DIM, CONV_DIM, 3, 3), "conv.bias": (CONV_DIM,),
    "objectness_logits.weight": (NUM_ANCHORS, CONV_DIM, 1, 1), "objectness_logits.bias": (NUM_ANCHORS,),
    "anchor_deltas.weight": (4 * NUM_ANCHORS, CONV_DIM, 1, 1), "anchor_deltas.bias": (4 * NUM_ANCHORS,),
}


def _names():
    return [n + s for n in NAMES for s in (".weight", ".bias")]


def train_workspace(A, G, S, device):
    """The workspace of the labelling of A anchors against G ground truths / the loss of S rows (f32 elements)."""
    nbytes = int(_lib.load().apse_rpn_train_workspace_bytes(int(A), int(G), int(S)))
    if nbytes == 0:
        raise _lib.ApseError("RPN-head training needs A <= 2^22 anchors, G <= 4096 ground truths and S <= 2^20 rows "
                             "(got A = %d, G = %d, S = %d)" % (A, G, S))
    return workspace_tensor(nbytes, device)


# ---- thin operator wrappers (also the surface the layer tests drive)
def anchor_labels(level_shapes, gt_boxes, iou_lo=0.3, iou_hi=0.7, device=None):
    """level_shapes: five (H, W) of p2 .. p6; gt_boxes f32 [G][4] in resized-image pixels -> (labels int32 [A] in {1, 0, -1},
    matched_idx int32 [A], matched_iou f32 [A]) on the device, A = 3 sum(H W), anchors in (level, y, x, a) order."""
    gt = torch.as_tensor(gt_boxes, dtype=torch.float32).reshape(-1, 4)
    dev = torch.device(device) if device is not None else gt.device
    if dev.type != "cuda":
        raise _lib.ApseError("anchor_labels needs a GPU device (no CPU fallback)")
    gt = gt.to(dev).contiguous()
    if len(level_shapes) != 5:
        raise ValueError("anchor_labels takes the five (H, W) of p2 .. p6")
    H5 = (C.c_int * 5)(*[int(h) for h, _ in level_shapes])
    W5 = (C.c_int * 5)(*[int(w) for _, w in level_shapes])
    A = 3 * sum(int(h) * int(w) for h, w in level_shapes)
    G = gt.shape[0]
    labels = torch.empty(max(A, 0), dtype=torch.int32, device=dev)
    idx = torch.empty(max(A, 0), dtype=torch.int32, device=dev)
    iou = torch.empty(max(A, 0), dtype=torch.float32, device=dev)
    ws = train_workspace(A, G, 0, dev) if 0 <= A <= (1 << 22) and 0 <= G <= 4096 else torch.empty(64, device=dev)
    _check(_lib.load().apse_rpn_anchor_labels(C.byref(H5), C.byref(W5), _lib.ptr(gt) if G else None, G, float(iou_lo), float(iou_hi),
                                              _lib.ptr(labels), _lib.ptr(idx), _lib.ptr(iou), _lib.ptr(ws), ws.numel() * 4,
                                              _lib.stream_ptr()), "apse_rpn_anchor_labels")
    return labels, idx, iou


def loss_forward(logits, deltas, slots, labels, anchor_boxes, gt_boxes, norm, ws, beta=0.0):
    """-> f32 [8]: loss_rpn_cls, loss_rpn_loc, num_pos, num_neg, share of positives with logit > 0, of negatives with logit < 0, 0, 0."""
    S = logits.shape[0]
    out = torch.zeros(8, dtype=torch.float32, device=logits.device)
    _check(_lib.load().apse_rpn_loss_forward(_lib.ptr(logits), _lib.ptr(deltas), _lib.ptr(slots), _lib.ptr(labels),
                                             _lib.ptr(anchor_boxes), _lib.ptr(gt_boxes), S, int(norm), float(beta), _lib.ptr(out),
                                             _lib.ptr(ws), ws.numel() * 4, _lib.stream_ptr()), "apse_rpn_loss_forward")
    return out


def loss_backward(logits, deltas, slots, labels, anchor_boxes, gt_boxes, norm, grad_cls=None, grad_loc=None, beta=0.0):
    S = logits.shape[0]
    dl, dd = torch.empty_like(logits), torch.empty_like(deltas)
    _check(_lib.load().apse_rpn_loss_backward(_lib.ptr(logits), _lib.ptr(deltas), _lib.ptr(slots), _lib.ptr(labels),
                                              _lib.ptr(anchor_boxes), _lib.ptr(gt_boxes), S, int(norm), float(beta),
                                              _lib.ptr(grad_cls), _lib.ptr(grad_loc), _lib.ptr(dl), _lib.ptr(dd), _lib.stream_ptr()),
           "apse_rpn_loss_backward")
    return dl, dd


def _flat(params):
    """The six tensors in named_parameters() order with the weights viewed as [O][K] (the same memory)."""
    return [p.reshape(p.shape[0], -1) if p.dim() == 4 else p for p in params]


def head_outputs(x, params, keep=False):
    """The three layers on patches [S][2304].  params: the 6 tensors in named_parameters() order -> (logits [S][3], deltas [S][12]);
    keep: also the hidden activation."""
    w = _flat(params)
    ws = torch.empty(64, dtype=torch.float32, device=x.device)       # K = 2304 < 4096: single-pass forwards, the workspace is not read
    h = bh.fc_forward(x, w[0], w[1], True, ws)
    logits = bh.fc_forward(h, w[2], w[3], False, ws)
    deltas = bh.fc_forward(h, w[4], w[5], False, ws)
    return (logits, deltas, h) if keep else (logits, deltas)


class _RpnLoss(torch.autograd.Function):
    """(loss_rpn_cls, loss_rpn_loc) = RPNOutputs.losses(head(x)) on the sampled rows; backward gives the 6 parameter gradients (the
    patches are frozen: no dx).  It follows box_head._BoxLoss."""

    @staticmethod
    def forward(ctx, x, slots, labels, anchor_boxes, gt_boxes, stats, beta, norm, *params):
        S = x.shape[0]
        det = [p.detach() for p in params]
        ws = train_workspace(0, 0, S, x.device)
        logits, deltas, h = head_outputs(x, det, keep=True)
        out = loss_forward(logits, deltas, slots, labels, anchor_boxes, gt_boxes, norm, ws, beta)
        stats.copy_(out)
        ctx.beta, ctx.norm = beta, norm
        ctx.save_for_backward(x, slots, labels, anchor_boxes, gt_boxes, logits, deltas, h, *det)
        return out[0].clone(), out[1].clone()

    @staticmethod
    def backward(ctx, grad_cls, grad_loc):
        x, slots, labels, anchor_boxes, gt_boxes, logits, deltas, h = ctx.saved_tensors[:8]
        params = ctx.saved_tensors[8:]
        w = _flat(params)
        ws = bh._workspace(x.shape[0], 1, x.device)
        gc = grad_cls.detach().to(torch.float32).reshape(1).contiguous()
        gl = grad_loc.detach().to(torch.float32).reshape(1).contiguous()
        grads = [None] * 6
        dl, dd = loss_backward(logits, deltas, slots, labels, anchor_boxes, gt_boxes, ctx.norm, gc, gl, ctx.beta)
        grads[2], grads[3] = bh.fc_wgrad(dl, h).reshape(params[2].shape), bh.bias_grad(dl, ws)
        grads[4], grads[5] = bh.fc_wgrad(dd, h).reshape(params[4].shape), bh.bias_grad(dd, ws)
        dh = bh.fc_dgrad(dl, w[2])                           # objectness first, then the deltas: a fixed order
        dh = bh.fc_dgrad(dd, w[4], into=dh)
        g1 = bh.relu_grad(h, dh)
        grads[0], grads[1] = bh.fc_wgrad(g1, x).reshape(params[0].shape), bh.bias_grad(g1, ws)
        return (None,) * 8 + tuple(grads)


class RPNHead(TrainableHead):
    prefix = PREFIX
    names = _names()
    noun = "RPN-head"
    a_noun = "an RPN-head"

    def __init__(self, device="cuda", smooth_l1_beta=0.0, batch_size_per_image=256):
        self.smooth_l1_beta = float(smooth_l1_beta)
        self.batch_size_per_image = int(batch_size_per_image)
        super().__init__(dict(SHAPES), device)          # last_stats: f32 [8], apse_rpn_loss_forward's out8

    @classmethod
    def from_cfg(cls, cfg, device="cuda"):
        """Head for a detector configuration; C4 (one stride-16 map, 15 anchors, 1024 channels) is refused."""
        from ..config import is_c4
        if is_c4(cfg):
            raise NotImplementedError("RPN-head training covers FPN models (p2 .. p6, 3 anchors per position, 256 channels); "
                                      "the C4 head (res4, 15 anchors, 1024 channels) is not covered")
        return cls(device)

    def _init_tensor(self, name, t):
        """detectron2's initialisation: normal(std = 0.01) on the three weights."""
        torch.nn.init.normal_(t, std=0.01)

    # ---- compute
    def _rows(self, patches):
        if not patches.is_cuda:
            raise _lib.ApseError("RPNHead needs GPU tensors (no CPU fallback)")
        if patches.dim() != 2 or patches.shape[1] != PATCH:
            raise ValueError("patches must be [S][2304] in (c, kh, kw) order, got %s" % (tuple(patches.shape),))
        if patches.shape[0] > MAX_ROWS:
            raise _lib.ApseError("RPNHead: %d rows in one step, the limit is %d (APSE_BOX_TRAIN_MAX_N)" % (patches.shape[0], MAX_ROWS))
        return patches.to(torch.float32).contiguous()

    def predict(self, patches):
        """(logits [S][3], deltas [S][12]) of the current weights at the patches' positions (no graph)."""
        x = self._rows(patches)
        if x.shape[0] == 0:
            return torch.zeros((0, NUM_ANCHORS), device=x.device), torch.zeros((0, 4 * NUM_ANCHORS), device=x.device)
        with torch.no_grad():
            return head_outputs(x, [p.detach() for p in self.parameters()])

    def forward(self, patches, slots, labels, anchor_boxes, gt_boxes, num_images):
        """patches [S][2304]; slots [S] in 0 .. 2; labels [S] (1 positive, 0 negative); anchor_boxes and gt_boxes [S][4] (the sampled
        anchors and their matched ground truths, read on positive rows); the sums are divided by ``batch_size_per_image x
        num_images`` -> {"loss_rpn_cls", "loss_rpn_loc"}.  ``last_stats`` holds apse_rpn_loss_forward's out8."""
        x = self._rows(patches)
        S = x.shape[0]
        params = list(self.parameters())
        if S == 0:
            # a zero that still reaches every parameter
            self.last_stats = torch.zeros(8, device=x.device)
            zero = sum((p.sum() for p in params)) * 0
            return {"loss_rpn_cls": zero, "loss_rpn_loc": zero * 1}
        dev = x.device
        sl = torch.as_tensor(slots).detach().reshape(-1).to(dev, torch.int32).contiguous()
        lab = torch.as_tensor(labels).detach().reshape(-1).to(dev, torch.int32).contiguous()
        ab = torch.as_tensor(anchor_boxes).detach().to(dev, torch.float32).reshape(-1, 4).contiguous()
        gb = torch.as_tensor(gt_boxes).detach().to(dev, torch.float32).reshape(-1, 4).contiguous()
        if sl.numel() != S or lab.numel() != S or ab.shape[0] != S or gb.shape[0] != S:
            raise ValueError("slots and labels must be [S], anchor_boxes and gt_boxes [S][4] for S = %d rows" % S)
        norm = self.batch_size_per_image * int(num_images)
        if norm < 1:
            raise ValueError("num_images must be at least 1")
        stats = torch.zeros(8, dtype=torch.float32, device=dev)
        loss_cls, loss_loc = _RpnLoss.apply(x, sl, lab, ab, gb, stats, self.smooth_l1_beta, norm, *params)
        self.last_stats = stats
        return {"loss_rpn_cls": loss_cls, "loss_rpn_loc": loss_loc}

    __call__ = forward


def merge_rpn_head(detector_state, rpn_state):
    """A full detector checkpoint with the six RPN-head tensors taken from ``rpn_state`` (bare names or
    ``proposal_generator.rpn_head.`` prefixed; an optional leading ``model.`` is dropped): the counterpart of merge_box_head."""
    return RPNHead.merge_into(detector_state, rpn_state, "merge_rpn_head")
