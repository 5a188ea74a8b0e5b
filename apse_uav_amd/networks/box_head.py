"""BoxHead -- the trainable counterpart of detectron2's box branch of StandardROIHeads (FPN models): FastRCNNConvFCHead with two
1024-wide FC layers and FastRCNNOutputLayers, with ``loss_cls`` and ``loss_box_reg`` of FastRCNNOutputs.losses (detectron2 0.1.2),
as dcnn/scripts/train/finetune_uav.py fine-tunes them on a frozen backbone.

    ROIAlign 7 (given) -> flatten (c, h, w) -> fc1 + ReLU -> fc2 + ReLU -> cls_score (K + 1) | bbox_pred (4 K)

The parameters are f32 leaf tensors on the device in the checkpoint's own layouts (``box_head.fc1.weight`` [1024][12544] with the
input index (c, h, w)-major, ``box_head.fc2.weight`` [1024][1024], ``box_predictor.cls_score.weight`` [K + 1][1024],
``box_predictor.bbox_pred.weight`` [4 K][1024]); ``torch.optim.SGD`` and ``apse_uav_amd.optim.SGD`` both update them in place.
``forward`` runs under one ``torch.autograd.Function`` that only ties the HIP kernels of csrc/box_train.hip together: the feature
permutation, the MFMA GEMM (forward, data gradient, weight gradient), the bias sums, the loss and its gradient.  There is no CPU
path.

RoI features are NHWC ``[n][7][7][256]`` (``apse_box_roi_features`` / ``TrackRCNN.box_roi_features``); an NCHW tensor
``[n][256][7][7]`` is accepted and permuted.
"""
import ctypes as C

import torch

from .. import _lib
from .head_base import TrainableHead, _check, relu_grad, roi_nhwc, workspace_tensor

PREFIX = "roi_heads."
FC_DIM = 1024
CONV_DIM = 256
POOL = 7
FEAT = CONV_DIM * POOL * POOL
MAX_ROIS = 1024            # APSE_BOX_TRAIN_MAX_N
MAX_CLASSES = 80           # APSE_MAX_CLASSES
BBOX_REG_WEIGHTS = (10.0, 10.0, 5.0, 5.0)
NAMES = ["box_head.fc1", "box_head.fc2", "box_predictor.cls_score", "box_predictor.bbox_pred"]


def _names():
    return [n + s for n in NAMES for s in (".weight", ".bias")]


def _workspace(n, K, device):
    nbytes = int(_lib.load().apse_box_train_workspace_bytes(int(n), int(K)))
    if nbytes == 0:
        raise _lib.ApseError("box-head training needs 1 <= n <= %d RoIs and 1 <= K <= %d classes (got n = %d, K = %d)"
                             % (MAX_ROIS, MAX_CLASSES, n, K))
    return workspace_tensor(nbytes, device)


def _w4(weights):
    return (C.c_float * 4)(*[float(v) for v in weights])


# ---- thin operator wrappers (also the surface the layer tests drive)
def box_match(proposals, gt_boxes, gt_classes, num_classes, iou_thresh=0.5):
    """proposals f32 [N][4], gt_boxes f32 [G][4], gt_classes int32 [G] on the device -> (matched_idx int32 [N], matched_iou f32 [N],
    labels int32 [N]; num_classes = background)."""
    N, G = proposals.shape[0], gt_boxes.shape[0]
    dev = proposals.device
    idx = torch.zeros(N, dtype=torch.int32, device=dev)
    iou = torch.zeros(N, dtype=torch.float32, device=dev)
    lab = torch.full((N,), int(num_classes), dtype=torch.int32, device=dev)
    _check(_lib.load().apse_box_match(_lib.ptr(proposals), N, _lib.ptr(gt_boxes) if G else None, _lib.ptr(gt_classes) if G else None,
                                      G, int(num_classes), float(iou_thresh), _lib.ptr(idx), _lib.ptr(iou), _lib.ptr(lab),
                                      _lib.stream_ptr()), "apse_box_match")
    return idx, iou, lab


def permute_features(x):
    """[n][7][7][256] -> [n][12544] in fc1's (c, h, w) order."""
    out = torch.empty((x.shape[0], FEAT), dtype=torch.float32, device=x.device)
    _check(_lib.load().apse_box_permute_features(_lib.ptr(x), x.shape[0], _lib.ptr(out), _lib.stream_ptr()),
           "apse_box_permute_features")
    return out


def fc_forward(x, w, bias, relu, ws=None):
    """y = x w^T + bias (+ ReLU); ws: the step's workspace (fc1's forward keeps its chunk sums there), allocated when None."""
    n, (O, K) = x.shape[0], w.shape
    if ws is None:
        ws = _workspace(n, 1, x.device)
    y = torch.empty((n, O), dtype=torch.float32, device=x.device)
    _check(_lib.load().apse_box_fc_forward(_lib.ptr(x), _lib.ptr(w), _lib.ptr(bias), n, O, K, int(relu), _lib.ptr(y), _lib.ptr(ws),
                                           ws.numel() * 4, _lib.stream_ptr()), "apse_box_fc_forward")
    return y


def fc_dgrad(dy, w, into=None):
    """dx = dy w; ``into``: an earlier dx that this one is added to (in place)."""
    n, (O, K) = dy.shape[0], w.shape
    dx = into if into is not None else torch.empty((n, K), dtype=torch.float32, device=dy.device)
    _check(_lib.load().apse_box_fc_dgrad(_lib.ptr(dy), _lib.ptr(w), n, O, K, int(into is not None), _lib.ptr(dx), _lib.stream_ptr()),
           "apse_box_fc_dgrad")
    return dx


def fc_wgrad(dy, x):
    n, O, K = dy.shape[0], dy.shape[1], x.shape[1]
    dw = torch.empty((O, K), dtype=torch.float32, device=dy.device)
    _check(_lib.load().apse_box_fc_wgrad(_lib.ptr(dy), _lib.ptr(x), n, O, K, _lib.ptr(dw), _lib.stream_ptr()), "apse_box_fc_wgrad")
    return dw


def bias_grad(dy, ws):
    n, O = dy.shape
    db = torch.empty(O, dtype=torch.float32, device=dy.device)
    _check(_lib.load().apse_box_bias_grad(_lib.ptr(dy), n, O, _lib.ptr(db), _lib.ptr(ws), ws.numel() * 4, _lib.stream_ptr()),
           "apse_box_bias_grad")
    return db


def loss_forward(logits, deltas, labels, prop_boxes, gt_boxes, ws, weights=BBOX_REG_WEIGHTS, beta=0.0):
    """-> f32 [8]: loss_cls, loss_box_reg, cls_accuracy, fg_cls_accuracy, false_negative, num_fg, num_bg, 0."""
    n, K = logits.shape[0], logits.shape[1] - 1
    out = torch.zeros(8, dtype=torch.float32, device=logits.device)
    _check(_lib.load().apse_box_loss_forward(_lib.ptr(logits), _lib.ptr(deltas), _lib.ptr(labels), _lib.ptr(prop_boxes),
                                             _lib.ptr(gt_boxes), n, K, _w4(weights), float(beta), _lib.ptr(out), _lib.ptr(ws),
                                             ws.numel() * 4, _lib.stream_ptr()), "apse_box_loss_forward")
    return out


def loss_backward(logits, deltas, labels, prop_boxes, gt_boxes, grad_cls=None, grad_box=None, weights=BBOX_REG_WEIGHTS, beta=0.0):
    n, K = logits.shape[0], logits.shape[1] - 1
    dl, dd = torch.empty_like(logits), torch.empty_like(deltas)
    _check(_lib.load().apse_box_loss_backward(_lib.ptr(logits), _lib.ptr(deltas), _lib.ptr(labels), _lib.ptr(prop_boxes),
                                              _lib.ptr(gt_boxes), n, K, _w4(weights), float(beta), _lib.ptr(grad_cls),
                                              _lib.ptr(grad_box), _lib.ptr(dl), _lib.ptr(dd), _lib.stream_ptr()),
           "apse_box_loss_backward")
    return dl, dd


def head_outputs(x, params, ws=None, keep=False):
    """The four layers on NHWC RoI features [n][7][7][256].  params: the 8 tensors in named_parameters() order -> (logits
    [n][K + 1], deltas [n][4 K]); keep: also the saved activations [x permuted, a1, a2]."""
    if ws is None:
        ws = _workspace(x.shape[0], 1, x.device)
    xp = permute_features(x)
    a1 = fc_forward(xp, params[0], params[1], True, ws)
    a2 = fc_forward(a1, params[2], params[3], True, ws)
    logits = fc_forward(a2, params[4], params[5], False, ws)
    deltas = fc_forward(a2, params[6], params[7], False, ws)
    return (logits, deltas, [xp, a1, a2]) if keep else (logits, deltas)


class _BoxLoss(torch.autograd.Function):
    """(loss_cls, loss_box_reg) = FastRCNNOutputs.losses(head(x)); backward gives the 8 parameter gradients (the RoI features are
    frozen: no dx)."""

    @staticmethod
    def forward(ctx, x, labels, prop_boxes, gt_boxes, stats, beta, *params):
        n, K = x.shape[0], params[4].shape[0] - 1
        det = [p.detach() for p in params]
        ws = _workspace(n, K, x.device)
        logits, deltas, acts = head_outputs(x, det, ws, keep=True)
        out = loss_forward(logits, deltas, labels, prop_boxes, gt_boxes, ws, beta=beta)
        stats.copy_(out)
        ctx.beta = beta
        ctx.save_for_backward(labels, prop_boxes, gt_boxes, logits, deltas, *acts, *det)
        return out[0].clone(), out[1].clone()

    @staticmethod
    def backward(ctx, grad_cls, grad_box):
        labels, prop_boxes, gt_boxes, logits, deltas, xp, a1, a2 = ctx.saved_tensors[:8]
        params = ctx.saved_tensors[8:]
        n, K = logits.shape[0], logits.shape[1] - 1
        ws = _workspace(n, K, logits.device)
        gc = grad_cls.detach().to(torch.float32).reshape(1).contiguous()
        gb = grad_box.detach().to(torch.float32).reshape(1).contiguous()
        grads = [None] * 8
        dl, dd = loss_backward(logits, deltas, labels, prop_boxes, gt_boxes, gc, gb, beta=ctx.beta)
        grads[4], grads[5] = fc_wgrad(dl, a2), bias_grad(dl, ws)
        grads[6], grads[7] = fc_wgrad(dd, a2), bias_grad(dd, ws)
        da2 = fc_dgrad(dl, params[4])                        # cls first, then bbox: a fixed order
        da2 = fc_dgrad(dd, params[6], into=da2)
        g2 = relu_grad(a2, da2)
        grads[2], grads[3] = fc_wgrad(g2, a1), bias_grad(g2, ws)
        g1 = relu_grad(a1, fc_dgrad(g2, params[2]))
        grads[0], grads[1] = fc_wgrad(g1, xp), bias_grad(g1, ws)
        return (None,) * 6 + tuple(grads)


class BoxHead(TrainableHead):
    prefix = PREFIX
    names = _names()
    noun = "box-head"

    def __init__(self, num_classes, device="cuda", smooth_l1_beta=0.0):
        if not 1 <= int(num_classes) <= MAX_CLASSES:
            raise ValueError("BoxHead: num_classes must be in 1..%d (APSE_MAX_CLASSES), got %d" % (MAX_CLASSES, num_classes))
        self.num_classes = K = int(num_classes)
        self.smooth_l1_beta = float(smooth_l1_beta)
        super().__init__({                    # last_stats: f32 [8], apse_box_loss_forward's out8
            "box_head.fc1.weight": (FC_DIM, FEAT), "box_head.fc1.bias": (FC_DIM,),
            "box_head.fc2.weight": (FC_DIM, FC_DIM), "box_head.fc2.bias": (FC_DIM,),
            "box_predictor.cls_score.weight": (K + 1, FC_DIM), "box_predictor.cls_score.bias": (K + 1,),
            "box_predictor.bbox_pred.weight": (4 * K, FC_DIM), "box_predictor.bbox_pred.bias": (4 * K,),
        }, device)

    @classmethod
    def from_cfg(cls, cfg, device="cuda"):
        """Head for a detector configuration; C4 (Res5ROIHeads: the box branch is res5 + a mean) is refused."""
        from ..config import is_c4
        if is_c4(cfg):
            raise NotImplementedError("box-head training covers FPN models (StandardROIHeads / FastRCNNConvFCHead); "
                                      "under C4 (Res5ROIHeads) the box branch is the res5 stage")
        return cls(int(cfg.MODEL.ROI_HEADS.NUM_CLASSES), device)

    def _init_tensor(self, name, t):
        """detectron2's initialisation: c2_xavier_fill (kaiming_uniform_(a = 1), bias 0) on fc1 / fc2, normal(std = 0.01) on
        cls_score, normal(std = 0.001) on bbox_pred."""
        if name.startswith("box_head"):
            torch.nn.init.kaiming_uniform_(t, a=1)
        else:
            torch.nn.init.normal_(t, std=0.01 if "cls_score" in name else 0.001)

    def load_state_dict(self, sd, strict=True, keep_predictor=False):
        """TrainableHead.load_state_dict.  ``keep_predictor``: load fc1 / fc2 only and leave ``box_predictor.*`` as initialised
        (a checkpoint of another class count)."""
        return super().load_state_dict(sd, strict, ("box_predictor",) if keep_predictor else ())

    # ---- compute
    def _check_input(self, x):
        if not x.is_cuda:
            raise _lib.ApseError("BoxHead needs GPU tensors (no CPU fallback)")
        if x.shape[0] > MAX_ROIS:
            raise _lib.ApseError("BoxHead: %d RoIs in one step, the limit is %d (APSE_BOX_TRAIN_MAX_N)" % (x.shape[0], MAX_ROIS))

    def predict(self, roi_features):
        """(logits [n][K + 1], deltas [n][4 K]) of the current weights (no graph)."""
        self._check_input(roi_features)
        x = roi_nhwc(roi_features, POOL)
        K = self.num_classes
        if x.shape[0] == 0:
            return torch.zeros((0, K + 1), device=x.device), torch.zeros((0, 4 * K), device=x.device)
        with torch.no_grad():
            return head_outputs(x, [p.detach() for p in self.parameters()])

    def forward(self, roi_features, labels, proposal_boxes, gt_boxes):
        """roi_features [n][7][7][256]; labels [n] integers in 0..K (K = background); proposal_boxes and gt_boxes [n][4] (the
        sampled boxes and their matched ground truths, read on foreground rows) -> {"loss_cls", "loss_box_reg"}.
        ``last_stats`` holds apse_box_loss_forward's out8."""
        self._check_input(roi_features)
        x = roi_nhwc(roi_features, POOL)
        n = x.shape[0]
        params = list(self.parameters())
        if n == 0:
            # a zero that still reaches every parameter
            self.last_stats = torch.zeros(8, device=x.device)
            zero = sum((p.sum() for p in params)) * 0
            return {"loss_cls": zero, "loss_box_reg": zero * 1}
        lab = torch.as_tensor(labels).detach().reshape(-1).to(x.device, torch.int32).contiguous()
        pb = torch.as_tensor(proposal_boxes).detach().to(x.device, torch.float32).reshape(-1, 4).contiguous()
        gb = torch.as_tensor(gt_boxes).detach().to(x.device, torch.float32).reshape(-1, 4).contiguous()
        if lab.numel() != n or pb.shape[0] != n or gb.shape[0] != n:
            raise ValueError("labels must be [n], proposal_boxes and gt_boxes [n][4] for n = %d RoIs" % n)
        stats = torch.zeros(8, dtype=torch.float32, device=x.device)
        loss_cls, loss_box = _BoxLoss.apply(x, lab, pb, gb, stats, self.smooth_l1_beta, *params)
        self.last_stats = stats
        return {"loss_cls": loss_cls, "loss_box_reg": loss_box}

    __call__ = forward


def merge_box_head(detector_state, box_head_state):
    """A full detector checkpoint with the eight box-branch tensors taken from ``box_head_state`` (bare names or ``roi_heads.``
    prefixed; an optional leading ``model.`` is dropped): the counterpart of merge_full_mask_rcnn."""
    return BoxHead.merge_into(detector_state, box_head_state, "merge_box_head")
