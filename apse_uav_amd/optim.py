"""Momentum SGD on the HIP kernel apse_sgd_step (include/apse_hip.h) -- the update rule of torch.optim.SGD, which
dcnn/scripts/train/train_association_head.py:88 builds with lr=0.01, momentum=0.9.

Same constructor and methods as torch.optim.SGD for one parameter group: ``step()`` launches one kernel per parameter that
has a ``.grad``; the first step of a parameter sets its momentum buffer to the gradient, later ones apply
``buf = momentum * buf + (1 - dampening) * grad``; ``nesterov`` and ``weight_decay`` as torch defines them.
``torch.optim.SGD`` works on the same parameters too.
"""
import torch
from torch.autograd.graph import increment_version

from . import _lib


class SGD:
    def __init__(self, params, lr, momentum=0, dampening=0, weight_decay=0, nesterov=False):
        if lr < 0.0:
            raise ValueError("Invalid learning rate: {}".format(lr))
        if momentum < 0.0:
            raise ValueError("Invalid momentum value: {}".format(momentum))
        if weight_decay < 0.0:
            raise ValueError("Invalid weight_decay value: {}".format(weight_decay))
        if nesterov and (momentum <= 0 or dampening != 0):
            raise ValueError("Nesterov momentum requires a momentum and zero dampening")
        self.params = list(params)
        for p in self.params:
            if not p.is_cuda or p.dtype != torch.float32 or not p.is_contiguous():
                raise _lib.ApseError("apse_uav_amd.optim.SGD needs contiguous f32 GPU parameters (no CPU fallback)")
        self.defaults = dict(lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay, nesterov=nesterov)
        self.param_groups = [dict(self.defaults, params=self.params)]
        self.state = {}

    def zero_grad(self, set_to_none=True):
        for p in self.params:
            if p.grad is not None:
                if set_to_none:
                    p.grad = None
                else:
                    p.grad.detach_()
                    p.grad.zero_()

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        lib = _lib.load()
        g = self.param_groups[0]
        momentum = float(g["momentum"])
        for p in g["params"]:
            if p.grad is None:
                continue
            grad = p.grad.contiguous()
            st = self.state.setdefault(p, {})
            buf = st.get("momentum_buffer")
            first = 0
            if momentum != 0 and buf is None:
                buf = torch.empty_like(p)
                st["momentum_buffer"] = buf
                first = 1
            rc = lib.apse_sgd_step(_lib.ptr(p), _lib.ptr(grad), _lib.ptr(buf) if buf is not None else None, p.numel(),
                                   float(g["lr"]), momentum, float(g["dampening"]), float(g["weight_decay"]),
                                   int(bool(g["nesterov"])), first, _lib.stream_ptr())
            if rc != _lib.APSE_OK:
                raise _lib.ApseError("apse_sgd_step failed (code %d) %s" % (rc, lib.apse_last_error(None).decode()))
            increment_version(p)       # an in-place update, as torch's p.add_ would record it
        return loss

    def state_dict(self):
        return {"state": {i: dict(self.state[p]) for i, p in enumerate(self.params) if p in self.state},
                "param_groups": [{k: v for k, v in self.param_groups[0].items() if k != "params"}]}

    def load_state_dict(self, sd):
        """Restores what ``state_dict`` wrote (hyper-parameters and momentum buffers, matched to the parameters by position)."""
        for k, v in sd["param_groups"][0].items():
            if k != "params":
                self.param_groups[0][k] = v
        self.state = {}
        for i, st in sd["state"].items():
            p = self.params[int(i)]
            self.state[p] = {k: (v.detach().to(device=p.device, dtype=p.dtype).clone() if torch.is_tensor(v) else v)
                             for k, v in st.items()}


class WarmupMultiStepLR:
    """detectron2's ``build_lr_scheduler`` default (solver/lr_scheduler.py WarmupMultiStepLR), as
    dcnn/scripts/train/finetune_segmentation.py steps it once per iteration:

        lr(it) = base_lr * warmup(it) * gamma ** (number of milestones <= it)
        warmup(it) = 1 for it >= warmup_iters, else warmup_factor * (1 - it / warmup_iters) + it / warmup_iters   ("linear")
                     ("constant": warmup_factor)

    Works on any optimizer with ``param_groups`` (``torch.optim.SGD``, ``apse_uav_amd.optim.SGD``).  Like torch's schedulers the
    constructor sets the learning rate of iteration 0 and ``step()`` moves to the next iteration.
    """

    def __init__(self, optimizer, milestones, gamma=0.1, warmup_factor=0.001, warmup_iters=1000, warmup_method="linear",
                 last_epoch=-1):
        milestones = [int(m) for m in milestones]
        if milestones != sorted(milestones):
            raise ValueError("Milestones should be a list of increasing integers. Got {}".format(milestones))
        if warmup_method not in ("linear", "constant"):
            raise ValueError("Unknown warmup method: {}".format(warmup_method))
        self.optimizer = optimizer
        self.milestones = milestones
        self.gamma = float(gamma)
        self.warmup_factor = float(warmup_factor)
        self.warmup_iters = int(warmup_iters)
        self.warmup_method = warmup_method
        for g in optimizer.param_groups:
            g.setdefault("initial_lr", g["lr"])
        self.base_lrs = [g["initial_lr"] for g in optimizer.param_groups]
        self.last_epoch = int(last_epoch)
        self.step()

    def factor(self, it):
        """lr(it) / base_lr."""
        if it >= self.warmup_iters:
            warm = 1.0
        elif self.warmup_method == "constant":
            warm = self.warmup_factor
        else:
            alpha = it / self.warmup_iters
            warm = self.warmup_factor * (1 - alpha) + alpha
        return warm * self.gamma ** sum(1 for m in self.milestones if m <= it)

    def get_lr(self):
        f = self.factor(self.last_epoch)
        return [b * f for b in self.base_lrs]

    def get_last_lr(self):
        return [g["lr"] for g in self.optimizer.param_groups]

    def step(self):
        self.last_epoch += 1
        for g, lr in zip(self.optimizer.param_groups, self.get_lr()):
            g["lr"] = lr

    def state_dict(self):
        return {k: v for k, v in self.__dict__.items() if k != "optimizer"}

    def load_state_dict(self, sd):
        self.__dict__.update(sd)
        for g, lr in zip(self.optimizer.param_groups, self.get_lr()):
            g["lr"] = lr
