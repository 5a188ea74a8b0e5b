"""AssociationHead -- counterpart of /root/reference/dcnn/networks/association_head.py:5-35.

Same constructor and ``forward`` contract (``(N, C, roi, roi)`` -> ``(N, embedding_dim)`` unit
vectors: flatten, ``Linear``, ``F.normalize(p=2, dim=1)``), computed by the HIP library: the
``Linear`` runs as an ``roi x roi`` valid convolution on the MFMA implicit-GEMM kernel and
the normalisation as a wave reduction.  On the tracker's per-frame path the head is fused
into the detector context instead (``TrackRCNN.attach_association_head``), so ``forward``
here serves stand-alone use and the parity tests.

Training (dcnn/scripts/train/train_association_head.py): ``parameters()`` returns ``fc.weight`` and ``fc.bias`` as leaf
tensors on the head's device, and after ``train()`` the forward pass runs the training kernels of csrc/assoc_train.hip
(x W^T + b and F.normalize, then on ``backward()`` dW and db) under an autograd Function, so ``.grad`` accumulates as it
does on an ``nn.Module``.  The head is in inference mode by default, and inference keeps the implicit-GEMM route above.
"""
import ctypes as C
import math

import numpy as np
import torch

from .. import _lib


class _FC:
    def __init__(self, out_f, in_f):
        self.weight = torch.zeros(out_f, in_f)
        self.bias = torch.zeros(out_f)
        self.initialized = False        # zeros until load_state_dict, or nn.Linear's init when parameters() needs them

    def reset_parameters(self):
        """nn.Linear.reset_parameters: kaiming_uniform_(a=sqrt(5)) on the weight, U(-1/sqrt(in), 1/sqrt(in)) on the bias, from
        torch's global generator.  Deferred to the first parameters() call of a head that loaded no weights, so building a
        head for inference (the tracker) draws nothing."""
        torch.nn.init.kaiming_uniform_(self.weight, a=math.sqrt(5))
        bound = 1.0 / math.sqrt(self.weight.shape[1]) if self.weight.shape[1] > 0 else 0.0
        torch.nn.init.uniform_(self.bias, -bound, bound)
        self.initialized = True


def _check(rc, what):
    if rc != _lib.APSE_OK:
        raise _lib.ApseError("%s failed (code %d) %s" % (what, rc, _lib.load().apse_last_error(None).decode()))


class _FCNormalize(torch.autograd.Function):
    """E = F.normalize(x.view(n, -1) @ W^T + b) on apse_assoc_fc_forward; backward = apse_assoc_fc_backward (dW, db; no dx)."""

    @staticmethod
    def forward(ctx, x, weight, bias):
        lib = _lib.load()
        n = x.shape[0]
        D, K = weight.shape
        xf = x.detach().reshape(n, -1).to(torch.float32).contiguous()          # (C, H, W) order, as x.view(-1, K)
        if xf.shape[1] != K:
            raise ValueError("input has %d features per row, fc expects %d" % (xf.shape[1], K))
        w = weight.detach().contiguous()
        b = bias.detach().contiguous()
        e = torch.empty((n, D), device=x.device, dtype=torch.float32)
        inv = torch.empty((n,), device=x.device, dtype=torch.float32)
        ws = torch.empty((max(int(lib.apse_assoc_fc_workspace_bytes(n, K, D)), 4) // 4,), device=x.device, dtype=torch.float32)
        _check(lib.apse_assoc_fc_forward(_lib.ptr(xf), _lib.ptr(w), _lib.ptr(b), n, K, D, _lib.ptr(e), _lib.ptr(inv),
                                         _lib.ptr(ws), ws.numel() * 4, _lib.stream_ptr()), "apse_assoc_fc_forward")
        ctx.save_for_backward(xf, e, inv)
        return e

    @staticmethod
    def backward(ctx, grad_e):
        lib = _lib.load()
        xf, e, inv = ctx.saved_tensors
        n, K = xf.shape
        D = e.shape[1]
        ge = grad_e.to(torch.float32).contiguous()
        dw = torch.empty((D, K), device=xf.device, dtype=torch.float32)
        db = torch.empty((D,), device=xf.device, dtype=torch.float32)
        ws = torch.empty((max(int(lib.apse_assoc_fc_workspace_bytes(n, K, D)), 4) // 4,), device=xf.device, dtype=torch.float32)
        _check(lib.apse_assoc_fc_backward(_lib.ptr(xf), _lib.ptr(e), _lib.ptr(inv), _lib.ptr(ge), n, K, D, _lib.ptr(dw),
                                          _lib.ptr(db), _lib.ptr(ws), ws.numel() * 4, _lib.stream_ptr()),
               "apse_assoc_fc_backward")
        return None, dw, db


class AssociationHead:
    def __init__(self, roi_size, input_depth, embedding_dim=128):
        self.embedding_dim = embedding_dim
        self.roi_size = roi_size
        self.input_depth = input_depth
        self.fc = _FC(embedding_dim, input_depth * roi_size * roi_size)
        self._packed = None
        self._packed_key = None
        self._device = torch.device("cpu")
        self.training = False

    # nn.Module-like surface used by the reference (rcnn_tracker.py:55-57, train_association_head.py:88-95)
    def state_dict(self):
        return {"fc.weight": self.fc.weight.detach(), "fc.bias": self.fc.bias.detach()}

    def load_state_dict(self, sd):
        w, b = sd["fc.weight"], sd["fc.bias"]
        if tuple(w.shape) != tuple(self.fc.weight.shape) or tuple(b.shape) != tuple(self.fc.bias.shape):
            raise RuntimeError("size mismatch for fc: %s vs %s" % (tuple(w.shape), tuple(self.fc.weight.shape)))
        if self.fc.weight.requires_grad:
            # parameters already handed out (an optimizer may hold them): copy in place, as nn.Module does
            with torch.no_grad():
                self.fc.weight.copy_(w.to(torch.float32))
                self.fc.bias.copy_(b.to(torch.float32))
        else:
            self.fc.weight = w.detach().to(torch.float32).cpu().contiguous()
            self.fc.bias = b.detach().to(torch.float32).cpu().contiguous()
        self.fc.initialized = True
        self._packed = None

    def to(self, device):
        self._device = torch.device(device)
        if self.fc.weight.requires_grad and self.fc.weight.device != self._device:
            # move the leaves in place (their identity, and an optimizer's references, survive), as nn.Module.to does
            for p in (self.fc.weight, self.fc.bias):
                p.data = p.data.to(self._device)
                if p.grad is not None:
                    p.grad = p.grad.to(self._device)
            self._packed = None
        return self

    def parameters(self, recurse=True):
        """fc.weight and fc.bias as f32 leaf tensors that require grad, on the head's device (the same objects on every
        call, so torch.optim.SGD and apse_uav_amd.optim.SGD may hold them)."""
        if not self.fc.initialized:
            self.fc.reset_parameters()
        for name in ("weight", "bias"):
            p = getattr(self.fc, name)
            if not p.requires_grad:
                p = p.detach().to(device=self._device, dtype=torch.float32).contiguous().requires_grad_(True)
                setattr(self.fc, name, p)
        return iter([self.fc.weight, self.fc.bias])

    def named_parameters(self):
        self.parameters()
        return iter([("fc.weight", self.fc.weight), ("fc.bias", self.fc.bias)])

    def zero_grad(self, set_to_none=True):
        for p in (self.fc.weight, self.fc.bias):
            if p.grad is not None:
                if set_to_none:
                    p.grad = None
                else:
                    p.grad.detach_()
                    p.grad.zero_()

    def train(self, mode=True):
        """Training mode: forward runs the training kernels (autograd-recorded when grad is enabled)."""
        self.training = bool(mode)
        self._packed = None
        return self

    def eval(self):
        return self.train(False)

    def num_flat_features(self, x):
        n = 1
        for s in x.size()[1:]:
            n *= s
        return n

    def _desc(self, n):
        d = _lib.ConvDesc()
        d.B, d.H, d.W, d.Cin = n, self.roi_size, self.roi_size, self.input_depth
        d.Cout, d.KH, d.KW, d.stride, d.pad = self.embedding_dim, self.roi_size, self.roi_size, 1, 0
        d.relu, d.res_mode, d.cfg, d.splitk = 0, 0, -1, 0
        return d

    def forward(self, x):
        lib = _lib.load()
        if not x.is_cuda:
            raise _lib.ApseError("AssociationHead.forward needs a GPU tensor (no CPU fallback)")
        n = x.shape[0]
        if n == 0:
            return torch.zeros((0, self.embedding_dim), device=x.device)
        if self.training:
            w, b = self.parameters()
            if w.device != x.device:
                raise _lib.ApseError("AssociationHead in training mode: input on %s, parameters on %s (call .to(device) and "
                                     ".parameters() first)" % (x.device, w.device))
            return _FCNormalize.apply(x, w, b)
        d = self._desc(n)
        key = (x.device, self.fc.weight.data_ptr(), self.fc.weight._version, self.fc.bias._version)
        if self._packed is None or self._packed_key != key:
            self._packed_key = key
            packed = np.zeros(lib.apse_conv_packed_elems(C.byref(d)), np.float32)
            w = np.ascontiguousarray(self.fc.weight.detach().cpu().numpy())       # [out][c*h*w] == OIHW
            _lib.check(lib.apse_conv_pack_weight(C.byref(d), _lib.ptr(w), self.input_depth, None, _lib.ptr(packed)), None,
                       "apse_conv_pack_weight")
            bias = np.zeros(((self.embedding_dim + 127) // 128) * 128, np.float32)
            bias[: self.embedding_dim] = self.fc.bias.detach().cpu().numpy()
            self._packed = (torch.from_numpy(packed).to(x.device), torch.from_numpy(bias).to(x.device))
        xn = x.to(torch.float32).permute(0, 2, 3, 1).contiguous()            # NCHW -> NHWC (plumbing)
        y = torch.empty((n, self.embedding_dim), device=x.device, dtype=torch.float32)
        steps = self.roi_size * ((self.roi_size * self.input_depth + 31) // 32)
        ws = torch.empty((64 * n * self.embedding_dim,), device=x.device, dtype=torch.float32)
        _lib.check(lib.apse_conv2d(C.byref(d), _lib.ptr(xn), _lib.ptr(self._packed[0]), _lib.ptr(self._packed[1]), None,
                                   _lib.ptr(y), _lib.ptr(ws), ws.numel() * 4, _lib.stream_ptr()), None, "apse_conv2d")
        out = torch.empty_like(y)
        _lib.check(lib.apse_l2_normalize(_lib.ptr(y), _lib.ptr(out), n, self.embedding_dim, _lib.stream_ptr()), None,
                   "apse_l2_normalize")
        return out

    __call__ = forward
