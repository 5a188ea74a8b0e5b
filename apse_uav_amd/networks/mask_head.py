"""MaskHead -- the trainable counterpart of detectron2's MaskRCNNConvUpsampleHead (FPN models) with mask_rcnn_loss, as
dcnn/scripts/train/finetune_segmentation.py fine-tunes it: everything frozen except ``roi_heads.mask_head.*``, ground-truth
boxes as proposals, ``loss_mask`` as the only loss.

    ROIAlign 14 (given) -> 4 x (conv3x3 256 + ReLU) -> deconv 2x2 stride 2 + ReLU -> 1x1 predictor (K class channels)

The parameters are f32 leaf tensors on the device in the checkpoint's own layouts (``mask_fcnN.weight`` OIHW,
``deconv.weight`` [Cin][Cout][2][2], ``predictor.weight`` [K][256][1][1]); ``torch.optim.SGD`` and ``apse_uav_amd.optim.SGD``
both update them in place.  ``forward`` runs under one ``torch.autograd.Function`` that only ties the HIP kernels of
csrc/mask_train.hip together: device-side filter packing, the MFMA 3x3 convolution (forward and data gradient), the inference
convolution kernel for the deconvolution and the predictor, the MFMA weight-gradient kernel, the loss and its gradient.  There is
no CPU path.

RoI features are NHWC ``[n][14][14][256]`` (``apse_mask_roi_features`` / ``TrackRCNN.mask_roi_features``); an NCHW tensor
``[n][256][14][14]`` is accepted and permuted.
"""
import torch

from .. import _lib
from .head_base import TrainableHead, _check, relu_grad, roi_nhwc, workspace_tensor

PREFIX = "roi_heads.mask_head."
CONV_DIM = 256
NUM_CONV = 4
POOL = 14
MAX_ROIS = 1024            # APSE_MASK_TRAIN_MAX_N
MAX_CLASSES = 80           # APSE_MAX_CLASSES


def _workspace(n, K, device):
    nbytes = int(_lib.load().apse_mask_train_workspace_bytes(int(n), int(K)))
    if nbytes == 0:
        raise _lib.ApseError("mask-head training needs 1 <= n <= %d RoIs and 1 <= K <= %d classes (got n = %d, K = %d)"
                             % (MAX_ROIS, MAX_CLASSES, n, K))
    return workspace_tensor(nbytes, device)


# ---- thin operator wrappers (also the surface the layer tests drive)
def pack_weight(w, bias, kind, cout, cin, kh, kw):
    """Device-side packing (apse_mask_pack_weight): returns (packed filter, padded bias)."""
    lib = _lib.load()
    packed = torch.empty(int(lib.apse_mask_pack_elems(cout, cin, kh, kw)), dtype=torch.float32, device=w.device)
    bias_p = torch.empty(((cout + 127) // 128) * 128, dtype=torch.float32, device=w.device)
    _check(lib.apse_mask_pack_weight(_lib.ptr(w), _lib.ptr(bias), kind, cout, cin, kh, kw, _lib.ptr(packed), _lib.ptr(bias_p),
                                     _lib.stream_ptr()), "apse_mask_pack_weight")
    return packed, bias_p


def conv_forward(x, packed, bias_p, cout, kh, kw, stride, pad, relu, deconv, ws):
    """x NHWC [n][H][W][Cin] -> y NHWC (deconv: [n][2H][2W][cout / 4])."""
    n, H, W, cin = x.shape
    oh, ow = (H + 2 * pad - kh) // stride + 1, (W + 2 * pad - kw) // stride + 1
    shape = (n, 2 * oh, 2 * ow, cout // 4) if deconv else (n, oh, ow, cout)
    y = torch.empty(shape, dtype=torch.float32, device=x.device)
    _check(_lib.load().apse_mask_conv_forward(_lib.ptr(x), _lib.ptr(packed), _lib.ptr(bias_p), n, H, W, cin, cout, kh, kw, stride,
                                              pad, int(relu), int(deconv), _lib.ptr(y), _lib.ptr(ws), ws.numel() * 4,
                                              _lib.stream_ptr()), "apse_mask_conv_forward")
    return y


def conv3x3(x, packed, bias_p, relu):
    """The 256 -> 256 3x3 layers on [n][14][14][256] (apse_mask_conv3x3): forward from a kind 0 pack, data gradient from kind 1."""
    y = torch.empty_like(x)
    _check(_lib.load().apse_mask_conv3x3(_lib.ptr(x), _lib.ptr(packed), _lib.ptr(bias_p), x.shape[0], int(relu), _lib.ptr(y),
                                         _lib.stream_ptr()), "apse_mask_conv3x3")
    return y


def bias_grad(g, ws):
    db = torch.empty(CONV_DIM, dtype=torch.float32, device=g.device)
    _check(_lib.load().apse_mask_bias_grad(_lib.ptr(g), g.numel() // CONV_DIM, _lib.ptr(db), _lib.ptr(ws), ws.numel() * 4,
                                           _lib.stream_ptr()), "apse_mask_bias_grad")
    return db


def weight_grad(a, b, kind, ws):
    """kind 0: a = dY, b = X of a 3x3 layer -> [256][256][3][3]; kind 1: a = X, b = dY of the deconvolution -> [256][256][2][2]."""
    k = 3 if kind == 0 else 2
    dw = torch.empty((CONV_DIM, CONV_DIM, k, k), dtype=torch.float32, device=a.device)
    _check(_lib.load().apse_mask_wgrad(_lib.ptr(a), _lib.ptr(b), a.shape[0], kind, _lib.ptr(dw), _lib.ptr(ws), ws.numel() * 4,
                                       _lib.stream_ptr()), "apse_mask_wgrad")
    return dw


def loss_forward(logits, classes, targets, ws):
    """logits [n][28][28][K], classes int32 [n], targets uint8 [n][28][28] -> f32 [4]: loss, accuracy, false positive, false negative."""
    n, K = logits.shape[0], logits.shape[3]
    out = torch.zeros(4, dtype=torch.float32, device=logits.device)
    _check(_lib.load().apse_mask_loss_forward(_lib.ptr(logits), K, _lib.ptr(classes), _lib.ptr(targets), n, _lib.ptr(out),
                                              _lib.ptr(ws), ws.numel() * 4, _lib.stream_ptr()), "apse_mask_loss_forward")
    return out


def loss_backward(logits, classes, targets, grad_loss=None):
    n, K = logits.shape[0], logits.shape[3]
    d = torch.empty((n, 28, 28), dtype=torch.float32, device=logits.device)
    _check(_lib.load().apse_mask_loss_backward(_lib.ptr(logits), K, _lib.ptr(classes), _lib.ptr(targets), n, _lib.ptr(grad_loss),
                                               _lib.ptr(d), _lib.stream_ptr()), "apse_mask_loss_backward")
    return d


def predictor_backward(d, a5, classes, w_pred, ws):
    """-> (g5 = a5 > 0 ? dX : 0, dW [K][256][1][1], db [K])."""
    n, K = a5.shape[0], w_pred.shape[0]
    g5 = torch.empty_like(a5)
    dw = torch.empty((K, CONV_DIM, 1, 1), dtype=torch.float32, device=a5.device)
    db = torch.empty(K, dtype=torch.float32, device=a5.device)
    _check(_lib.load().apse_mask_predictor_backward(_lib.ptr(d), _lib.ptr(a5), _lib.ptr(classes), _lib.ptr(w_pred), n, K,
                                                    _lib.ptr(g5), _lib.ptr(dw), _lib.ptr(db), _lib.ptr(ws), ws.numel() * 4,
                                                    _lib.stream_ptr()), "apse_mask_predictor_backward")
    return g5, dw, db


def head_logits(x, params, ws, keep=False):
    """The six layers on NHWC RoI features.  params: the 12 tensors in named_parameters() order.  keep: also return the saved
    activations [x, a1, a2, a3, a4, a5]."""
    acts = [x]
    for i in range(NUM_CONV):
        w, b = params[2 * i], params[2 * i + 1]
        pk, bp = pack_weight(w, b, 0, CONV_DIM, CONV_DIM, 3, 3)
        acts.append(conv3x3(acts[-1], pk, bp, True))
    pk, bp = pack_weight(params[8], params[9], 2, 4 * CONV_DIM, CONV_DIM, 1, 1)
    acts.append(conv_forward(acts[-1], pk, bp, 4 * CONV_DIM, 1, 1, 1, 0, True, True, ws))
    K = params[10].shape[0]
    pk, bp = pack_weight(params[10], params[11], 0, K, CONV_DIM, 1, 1)
    logits = conv_forward(acts[-1], pk, bp, K, 1, 1, 1, 0, False, False, ws)
    return (logits, acts) if keep else logits


class _MaskLoss(torch.autograd.Function):
    """loss_mask = mask_rcnn_loss(head(x)); backward gives the 12 parameter gradients (the RoI features are frozen: no dx)."""

    @staticmethod
    def forward(ctx, x, classes, targets, stats, *params):
        n, K = x.shape[0], params[10].shape[0]
        det = [p.detach() for p in params]
        ws = _workspace(n, K, x.device)
        logits, acts = head_logits(x, det, ws, keep=True)
        out = loss_forward(logits, classes, targets, ws)
        stats.copy_(out)
        ctx.save_for_backward(classes, targets, logits, *acts, *det)
        return out[0].clone()

    @staticmethod
    def backward(ctx, grad_loss):
        saved = ctx.saved_tensors
        classes, targets, logits = saved[:3]
        acts, params = saved[3:9], saved[9:]
        n, K = logits.shape[0], logits.shape[3]
        ws = _workspace(n, K, logits.device)
        go = grad_loss.detach().to(torch.float32).reshape(1).contiguous()
        grads = [None] * 12
        d = loss_backward(logits, classes, targets, go)
        g, grads[10], grads[11] = predictor_backward(d, acts[5], classes, params[10].reshape(K, CONV_DIM), ws)
        # deconvolution: db, dW = X^T dY per tap, dX = the 2x2 stride-2 convolution of dY with deconv.weight read as OIHW
        grads[9] = bias_grad(g, ws)
        grads[8] = weight_grad(acts[4], g, 1, ws)
        pk, _ = pack_weight(params[8], None, 0, CONV_DIM, CONV_DIM, 2, 2)
        dx = conv_forward(g, pk, None, CONV_DIM, 2, 2, 2, 0, False, False, ws)
        g = relu_grad(acts[4], dx)
        for i in range(NUM_CONV - 1, -1, -1):
            grads[2 * i + 1] = bias_grad(g, ws)
            grads[2 * i] = weight_grad(g, acts[i], 0, ws)
            if i > 0:
                pk, _ = pack_weight(params[2 * i], None, 1, CONV_DIM, CONV_DIM, 3, 3)
                dx = conv3x3(g, pk, None, False)
                g = relu_grad(acts[i], dx)
        return (None, None, None, None) + tuple(grads)


def _names():
    names = []
    for i in range(1, NUM_CONV + 1):
        names += ["mask_fcn%d.weight" % i, "mask_fcn%d.bias" % i]
    return names + ["deconv.weight", "deconv.bias", "predictor.weight", "predictor.bias"]


class MaskHead(TrainableHead):
    prefix = PREFIX
    names = _names()
    noun = "mask-head"
    stray_under_prefix = True

    def __init__(self, num_classes, device="cuda"):
        if not 1 <= int(num_classes) <= MAX_CLASSES:
            raise ValueError("MaskHead: num_classes must be in 1..%d (APSE_MAX_CLASSES), got %d" % (MAX_CLASSES, num_classes))
        self.num_classes = int(num_classes)
        shapes = {}
        for i in range(1, NUM_CONV + 1):
            shapes["mask_fcn%d.weight" % i] = (CONV_DIM, CONV_DIM, 3, 3)
            shapes["mask_fcn%d.bias" % i] = (CONV_DIM,)
        shapes["deconv.weight"] = (CONV_DIM, CONV_DIM, 2, 2)
        shapes["deconv.bias"] = (CONV_DIM,)
        shapes["predictor.weight"] = (self.num_classes, CONV_DIM, 1, 1)
        shapes["predictor.bias"] = (self.num_classes,)
        super().__init__(shapes, device)      # last_stats: f32 [4], loss, accuracy, false positive, false negative

    @classmethod
    def from_cfg(cls, cfg, device="cuda"):
        """Head for a detector configuration; C4 (Res5ROIHeads: the mask branch shares res5) is refused."""
        from ..config import is_c4
        if is_c4(cfg):
            raise NotImplementedError("mask-head training covers FPN models (StandardROIHeads / MaskRCNNConvUpsampleHead); "
                                      "under C4 (Res5ROIHeads) the mask branch shares res5 with the box branch")
        return cls(int(cfg.MODEL.ROI_HEADS.NUM_CLASSES), device)

    def _init_tensor(self, name, t):
        """detectron2's initialisation: c2_msra_fill (kaiming_normal_, fan_out, relu; bias 0) on the convolutions and the
        deconvolution, normal(std = 0.001) on the predictor."""
        if name.startswith("predictor"):
            torch.nn.init.normal_(t, std=0.001)
        else:
            torch.nn.init.kaiming_normal_(t, mode="fan_out", nonlinearity="relu")

    # ---- compute
    def _check_input(self, x):
        if not x.is_cuda:
            raise _lib.ApseError("MaskHead needs GPU tensors (no CPU fallback)")
        if x.shape[0] > MAX_ROIS:
            raise _lib.ApseError("MaskHead: %d RoIs in one step, the limit is %d (APSE_MASK_TRAIN_MAX_N)" % (x.shape[0], MAX_ROIS))

    def logits(self, roi_features):
        """Mask logits [n][28][28][K] of the current weights (no graph)."""
        self._check_input(roi_features)
        x = roi_nhwc(roi_features, POOL)
        n = x.shape[0]
        if n == 0:
            return torch.zeros((0, 28, 28, self.num_classes), device=x.device)
        with torch.no_grad():
            return head_logits(x, [p.detach() for p in self.parameters()], _workspace(n, self.num_classes, x.device))

    def forward(self, roi_features, gt_classes, targets):
        """roi_features [n][14][14][256]; gt_classes [n] integer class indices; targets [n][28][28] (non-zero = inside) ->
        {"loss_mask": scalar tensor}.  ``last_stats`` holds the loss and detectron2's three logged ratios."""
        self._check_input(roi_features)
        x = roi_nhwc(roi_features, POOL)
        n = x.shape[0]
        params = list(self.parameters())
        if n == 0:
            # detectron2: pred_mask_logits.sum() * 0 -- a zero that still reaches every parameter
            self.last_stats = torch.zeros(4, device=x.device)
            return {"loss_mask": sum((p.sum() for p in params)) * 0}
        cls_host = torch.as_tensor(gt_classes).detach().to("cpu", torch.int64).reshape(-1)
        if cls_host.numel() != n or tuple(targets.shape) != (n, 28, 28):
            raise ValueError("gt_classes must be [n] and targets [n][28][28] for n = %d RoIs" % n)
        if self.num_classes > 1 and (int(cls_host.min()) < 0 or int(cls_host.max()) >= self.num_classes):
            raise ValueError("gt_classes outside 0..%d" % (self.num_classes - 1))
        classes = cls_host.to(torch.int32).to(x.device)
        tg = (targets != 0).to(torch.uint8).to(x.device).contiguous()
        stats = torch.zeros(4, dtype=torch.float32, device=x.device)
        loss = _MaskLoss.apply(x, classes, tg, stats, *params)
        self.last_stats = stats
        return {"loss_mask": loss}

    __call__ = forward


def merge_full_mask_rcnn(detector_state, mask_head_state):
    """The merged checkpoint of add_mask_head_to_frcnn.py / finetune_segmentation.py: every key of the detector, with
    ``roi_heads.mask_head.*`` taken from ``mask_head_state`` (bare names or prefixed; an optional leading ``model.`` is dropped)."""
    return MaskHead.merge_into(detector_state, mask_head_state, "merge_full_mask_rcnn")
