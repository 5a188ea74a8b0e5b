"""torch CPU restatement of the mask head and mask_rcnn_loss (detectron2 0.1.2: MaskRCNNConvUpsampleHead, mask_rcnn_loss), and the
float64 arbiter the mask-head training tests judge by.

The arbiter: a reference is computed twice with torch's CPU operators, in float64 and in float32.  Two correct f32 implementations
with different summation orders land at errors of the same size, not at the same error, so the HIP result passes when

    max|HIP - f64| <= factor * max|torch_f32 - f64| + eps_floor          (both sides divided by max|f64|)

with factor 2 (4 where errors compound through weight updates) and eps_floor one f32 ulp of max|f64|, for outputs torch happens to
get exactly.
"""
import numpy as np
import torch
import torch.nn.functional as F

NAMES = ["mask_fcn1", "mask_fcn2", "mask_fcn3", "mask_fcn4", "deconv", "predictor"]


def param_names():
    return [n + s for n in NAMES for s in (".weight", ".bias")]


def seeded_state(K, seed, scale=1.0):
    """Weights that keep activations O(1) through the head (He-like), biases O(0.1), on the CPU in f32."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for i in range(1, 5):
        sd["mask_fcn%d.weight" % i] = torch.randn(256, 256, 3, 3, generator=g) * (scale * (2.0 / 2304) ** 0.5)
        sd["mask_fcn%d.bias" % i] = torch.randn(256, generator=g) * 0.1
    sd["deconv.weight"] = torch.randn(256, 256, 2, 2, generator=g) * (scale * (2.0 / 256) ** 0.5)
    sd["deconv.bias"] = torch.randn(256, generator=g) * 0.1
    sd["predictor.weight"] = torch.randn(K, 256, 1, 1, generator=g) * (scale * (1.0 / 256) ** 0.5)
    sd["predictor.bias"] = torch.randn(K, generator=g) * 0.1
    return sd


def exact_forward_state(K, seed):
    """Weights whose forward pass is exact in f32 up to the predictor: mask_fcnN and deconv weights are 0 or +-1/4 (sparse, so the
    activations stay O(1)), their biases multiples of 1/4.  With RoI features that are multiples of 1/2 (exact_features) every
    product and every partial sum through the deconvolution's ReLU is a multiple of 2^-11 below 2^5: representable, whatever the
    summation order.  f32 and f64 then see the SAME ReLU masks, exact zeros included, and a gradient comparison is not decided by
    which pre-activations within rounding distance of 0 happen to change sign (each such flip moves a gradient by ~1e-4 of its
    scale, in torch's own f32 run as much as in ours).  The predictor is dense and random."""
    g = torch.Generator().manual_seed(seed)
    sd = {}

    def sparse(shape, fan_in):
        keep = torch.rand(shape, generator=g) < 32.0 / fan_in
        sign = (torch.rand(shape, generator=g) < 0.5).float() * 2 - 1
        return keep.float() * sign * 0.25

    for i in range(1, 5):
        sd["mask_fcn%d.weight" % i] = sparse((256, 256, 3, 3), 2304)
        sd["mask_fcn%d.bias" % i] = torch.randint(-2, 3, (256,), generator=g).float() * 0.25
    sd["deconv.weight"] = sparse((256, 256, 2, 2), 256)
    sd["deconv.bias"] = torch.randint(-2, 3, (256,), generator=g).float() * 0.25
    sd["predictor.weight"] = torch.randn(K, 256, 1, 1, generator=g) * (1.0 / 256) ** 0.5
    sd["predictor.bias"] = torch.randn(K, generator=g) * 0.1
    return sd


def exact_features(n, seed):
    """RoI features [n][256][14][14] that are non-negative multiples of 1/2 (see exact_forward_state)."""
    g = torch.Generator().manual_seed(seed)
    return torch.relu(torch.round(torch.randn(n, 256, 14, 14, generator=g) * 2) / 2)


def quiet_band(z64, dy, rel=1e-5):
    """dy with zeros where the float64 pre-activation z64 lies within rel * max|z| of 0 without being 0: ReLU's gradient is
    discontinuous there, and whether an f32 implementation lands on the same side as float64 is chance (its rounding error is ~1e-6
    of the scale), not correctness.  Exact zeros keep their upstream gradient: the tie rule (gradient 0) is checked."""
    band = (z64.abs() < rel * float(z64.abs().max())) & (z64 != 0)
    out = dy.clone()
    out[band] = 0
    return out, int(band.sum())


def head_logits(x, p):
    """x NCHW [n][256][14][14]; p: dict of the 12 parameters -> logits [n][K][28][28]."""
    for i in range(1, 5):
        x = F.relu(F.conv2d(x, p["mask_fcn%d.weight" % i], p["mask_fcn%d.bias" % i], padding=1))
    x = F.relu(F.conv_transpose2d(x, p["deconv.weight"], p["deconv.bias"], stride=2))
    return F.conv2d(x, p["predictor.weight"], p["predictor.bias"])


def mask_loss(logits, classes, targets):
    """mask_rcnn_loss: logits [n][K][28][28], classes int64 [n], targets bool [n][28][28]."""
    n, K = logits.shape[0], logits.shape[1]
    if n == 0:
        return logits.sum() * 0
    sel = logits[:, 0] if K == 1 else logits[torch.arange(n), classes]
    return F.binary_cross_entropy_with_logits(sel, targets.to(logits.dtype), reduction="mean")


def mask_stats(logits, classes, targets):
    """accuracy, false_positive, false_negative as mask_rcnn_loss logs them."""
    n, K = logits.shape[0], logits.shape[1]
    sel = logits[:, 0] if K == 1 else logits[torch.arange(n), classes]
    gt = targets.bool()
    wrong = (sel > 0.0) != gt
    pos = int(gt.sum())
    return (1 - int(wrong.sum()) / max(wrong.numel(), 1.0), int((wrong & ~gt).sum()) / max(gt.numel() - pos, 1.0),
            int((wrong & gt).sum()) / max(pos, 1.0))


def head_step(x, sd, classes, targets, dtype):
    """loss and the 12 parameter gradients of one forward + backward in `dtype` on the CPU."""
    p = {k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in sd.items()}
    loss = mask_loss(head_logits(x.to(dtype), p), classes, targets)
    loss.backward()
    return loss.detach(), {k: v.grad for k, v in p.items()}


def arbiter(hip, f64, f32, factor=2.0):
    """-> (err_hip, err_f32, bound, ok), errors normalised by max|f64|."""
    f64 = torch.as_tensor(f64).detach().cpu().double().reshape(-1)
    hip = torch.as_tensor(hip).detach().cpu().double().reshape(-1)
    f32 = torch.as_tensor(f32).detach().cpu().double().reshape(-1)
    assert hip.shape == f64.shape == f32.shape, (hip.shape, f64.shape, f32.shape)
    scale = float(f64.abs().max())
    if scale == 0.0:
        e = float(hip.abs().max())
        return e, float(f32.abs().max()), 0.0, e == 0.0
    floor = float(np.spacing(np.float32(scale))) / scale
    eh = float((hip - f64).abs().max()) / scale
    ef = float((f32 - f64).abs().max()) / scale
    bound = factor * ef + floor
    return eh, ef, bound, bool(np.isfinite(eh) and eh <= bound)


def nhwc(x):
    return x.permute(0, 2, 3, 1).contiguous()


def nchw(x):
    return x.permute(0, 3, 1, 2).contiguous()
