"""Online triplet losses -- counterpart of dcnn/online_triplet_loss/losses.py (batch_hard_triplet_loss :102-146,
batch_all_triplet_loss :149-197).

Same names and call contracts; the forward pass and the gradient in the embeddings are the HIP kernels of
csrc/assoc_train.hip (include/apse_hip.h "Association-head training"), tied to autograd by ``torch.autograd.Function``.
The reference's expression is kept, quirks included (DESIGN.md "Association-head training"): Gram-form distances clamped at 0,
the ``eq(0)`` mask of the non-squared form (zero gradient at zero distance), the row maximum added to invalid negatives, the
strict hinge ``tl[tl < 0] = 0`` and the ``1e-16`` guards of batch-all.  Labels are compared as values.
"""
import torch

from .. import _lib


def _check(rc, what):
    if rc != _lib.APSE_OK:
        raise _lib.ApseError("%s failed (code %d) %s" % (what, rc, _lib.load().apse_last_error(None).decode()))


def _prepare(labels, embeddings):
    if not embeddings.is_cuda:
        raise _lib.ApseError("triplet losses need GPU embeddings (no CPU fallback)")
    if embeddings.dim() != 2:
        raise ValueError("embeddings must be (batch_size, embed_dim), got %s" % (tuple(embeddings.shape),))
    labels = torch.as_tensor(labels).reshape(-1).to(device=embeddings.device, dtype=torch.float64).contiguous()
    if labels.shape[0] != embeddings.shape[0]:
        raise ValueError("%d labels for %d embeddings" % (labels.shape[0], embeddings.shape[0]))
    return labels


class _TripletLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, embeddings, labels, margin, squared, batch_all):
        lib = _lib.load()
        e = embeddings.detach().to(torch.float32).contiguous()
        n, d = e.shape
        ctx.squared, ctx.batch_all, ctx.n = int(bool(squared)), batch_all, n
        out = torch.zeros(2, device=e.device, dtype=torch.float32)
        if n == 0:
            # mean() of an empty tensor is NaN (batch-hard); batch-all divides an empty sum by 1e-16
            if not batch_all:
                out[0] = float("nan")
            ctx.save_for_backward(e)
            ctx.ws = None
            return out
        ws = torch.empty(max(int(lib.apse_triplet_workspace_bytes(n)), 1), device=e.device, dtype=torch.uint8)
        fn = lib.apse_triplet_all_forward if batch_all else lib.apse_triplet_hard_forward
        _check(fn(_lib.ptr(labels), _lib.ptr(e), n, d, float(margin), ctx.squared, _lib.ptr(out), _lib.ptr(ws), ws.numel(),
                  _lib.stream_ptr()), "apse_triplet_%s_forward" % ("all" if batch_all else "hard"))
        ctx.save_for_backward(e)
        ctx.ws = ws
        return out

    @staticmethod
    def backward(ctx, grad_out):
        (e,) = ctx.saved_tensors
        n, d = e.shape
        de = torch.zeros_like(e)
        if n == 0:
            return de, None, None, None, None
        lib = _lib.load()
        g = grad_out[0:1].to(torch.float32).contiguous()
        fn = lib.apse_triplet_all_backward if ctx.batch_all else lib.apse_triplet_hard_backward
        _check(fn(_lib.ptr(e), n, d, ctx.squared, _lib.ptr(ctx.ws), _lib.ptr(g), _lib.ptr(de), _lib.stream_ptr()),
               "apse_triplet_%s_backward" % ("all" if ctx.batch_all else "hard"))
        return de, None, None, None, None


def batch_hard_triplet_loss(labels, embeddings, margin, squared=False, device='cpu'):
    """For each anchor the hardest positive and the hardest negative; mean over all anchors (losses.py:102-146).
    Returns a scalar device tensor.  ``device`` is accepted for the reference's signature (its masks live there); the
    computation runs on the embeddings' GPU."""
    labels = _prepare(labels, embeddings)
    out = _TripletLoss.apply(embeddings, labels, margin, squared, False)
    return out[0]


def batch_all_triplet_loss(labels, embeddings, margin, squared=False):
    """Mean over the positive valid triplets; returns ``(triplet_loss, fraction_positive_triplets)`` (losses.py:149-197).
    The reference's debug print is not ported."""
    labels = _prepare(labels, embeddings)
    out = _TripletLoss.apply(embeddings, labels, margin, squared, True)
    return out[0], out[1].detach()
