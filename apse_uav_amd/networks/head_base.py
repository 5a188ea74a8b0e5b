"""What MaskHead, BoxHead and RPNHead share: the parameter bookkeeping of a trainable head whose parameters are f32 leaf tensors
under the checkpoint's own names, and the few helpers their operator wrappers have in common.  A head declares ``prefix`` (its
keys' prefix in a detector state), ``names`` (the parameter names in order), ``noun`` (for messages), its shape table (to
``__init__``) and ``_init_tensor``; the kernels, the ``autograd.Function`` and ``forward`` stay in the head's own file.
"""
import torch

from .. import _lib

CONV_DIM = 256
DETECTOR_ROOTS = ("backbone.", "proposal_generator.", "roi_heads.", "pixel_")


def _check(rc, what):
    if rc != _lib.APSE_OK:
        raise _lib.ApseError("%s failed (code %d) %s" % (what, rc, _lib.load().apse_last_error(None).decode()))


def workspace_tensor(nbytes, device):
    """A workspace of ``nbytes`` bytes as an f32 tensor (the entries take its pointer and ``numel() * 4``)."""
    return torch.empty((nbytes + 3) // 4, dtype=torch.float32, device=device)


def relu_grad(y, dy):
    g = torch.empty_like(dy)
    _check(_lib.load().apse_mask_relu_grad(_lib.ptr(y), _lib.ptr(dy), dy.numel(), _lib.ptr(g), _lib.stream_ptr()),
           "apse_mask_relu_grad")
    return g


def roi_nhwc(x, pool):
    """RoI features as contiguous f32 NHWC [n][pool][pool][256]; an NCHW tensor [n][256][pool][pool] is permuted."""
    want = "RoI features must be [n][%d][%d][%d] (NHWC) or [n][%d][%d][%d]" % (pool, pool, CONV_DIM, CONV_DIM, pool, pool)
    if x.dim() != 4:
        raise ValueError(want)
    if tuple(x.shape[1:]) == (pool, pool, CONV_DIM):
        return x.to(torch.float32).contiguous()
    if tuple(x.shape[1:]) == (CONV_DIM, pool, pool):
        return x.to(torch.float32).permute(0, 2, 3, 1).contiguous()
    raise ValueError("%s, got %s" % (want, tuple(x.shape)))


class TrainableHead:
    prefix = None               # the parameters' prefix in a detector state
    names = ()                  # parameter names in named_parameters() order
    noun = None                 # "box-head": what the messages call the head
    a_noun = None               # the noun with its article where "a" is wrong
    stray_under_prefix = False  # merge_into: an unknown key under ``prefix`` is an error (MaskHead; the others let it pass)

    def __init__(self, shapes, device):
        self._shapes = shapes
        self._device = torch.device(device)
        self.training = True
        self.last_stats = None                # the loss kernel's statistics on the device after a forward
        self._params = None

    # ---- parameters
    def _init_tensor(self, name, t):
        """detectron2's initialisation of one weight, in place on a zeroed CPU tensor (biases stay 0)."""
        raise NotImplementedError

    def _init(self):
        """Every parameter in order: zeros on the CPU, ``_init_tensor`` on the weights (drawn from torch's global generator), then
        the move to the device."""
        ps = {}
        for name in self.names:
            t = torch.zeros(self._shapes[name])
            if name.endswith(".weight"):
                self._init_tensor(name, t)
            ps[name] = t.to(self._device).requires_grad_(True)
        self._params = ps

    def named_parameters(self):
        if self._params is None:
            self._init()
        return iter([(k, self._params[k]) for k in self.names])

    def parameters(self, recurse=True):
        return iter([p for _, p in self.named_parameters()])

    def to(self, device):
        self._device = torch.device(device)
        if self._params is not None:
            for p in self._params.values():
                p.data = p.data.to(self._device)
                if p.grad is not None:
                    p.grad = p.grad.to(self._device)
        return self

    def state_dict(self, prefix=""):
        return {prefix + k: p.detach().clone() for k, p in self.named_parameters()}

    def load_state_dict(self, sd, strict=True, skip=()):
        """Accepts the bare names or the detector's (under ``prefix``; other keys of a full detector are ignored).  ``skip``: name
        prefixes that are not loaded and stay as initialised.  -> the missing names; raises on them only when ``strict``."""
        if self._params is None:
            if skip:
                self._init()
            else:
                self._params = {k: torch.zeros(self._shapes[k], device=self._device).requires_grad_(True) for k in self.names}
        missing = []
        with torch.no_grad():
            for k in self.names:
                if skip and k.startswith(tuple(skip)):
                    continue
                src = sd.get(k, sd.get(self.prefix + k))
                if src is None:
                    missing.append(k)
                    continue
                src = torch.as_tensor(src)
                if tuple(src.shape) != tuple(self._shapes[k]):
                    raise RuntimeError("size mismatch for %s: %s vs %s" % (k, tuple(src.shape), tuple(self._shapes[k])))
                self._params[k].copy_(src.to(torch.float32))
        if missing and strict:
            raise RuntimeError("missing %s keys: %s" % (self.noun, ", ".join(missing)))
        return missing

    def zero_grad(self, set_to_none=True):
        for p in self.parameters():
            if p.grad is not None:
                if set_to_none:
                    p.grad = None
                else:
                    p.grad.detach_()
                    p.grad.zero_()

    def train(self, mode=True):
        self.training = bool(mode)
        return self

    def eval(self):
        return self.train(False)

    def push_into(self, model):
        """Loads the current head weights into a TrackRCNN (or a TrackPredictor's ``model``): its state gets the head's entries
        under ``prefix`` replaced and its context is rebuilt on the next frame."""
        target = getattr(model, "model", model)
        if target._state is None:
            raise _lib.ApseError("push_into: the detector has no weights loaded")
        sd = dict(target._state)
        sd.update({k: v.cpu() for k, v in self.state_dict(self.prefix).items()})
        target.load_state_dict(sd)
        return model

    @classmethod
    def merge_into(cls, detector_state, head_state, caller="merge_into"):
        """Every key of ``detector_state`` with the head's tensors taken from ``head_state`` (bare names or under ``prefix``; an
        optional leading ``model.`` is dropped from both).  A key of ``head_state`` that is neither a parameter of the head nor
        under one of a detector's roots, or an incomplete head, is a KeyError in ``caller``'s name."""
        out = {}
        for k, v in detector_state.items():
            out[k[6:] if k.startswith("model.") else k] = v
        found = 0
        for k, v in head_state.items():
            k = k[6:] if k.startswith("model.") else k
            bare = k[len(cls.prefix):] if k.startswith(cls.prefix) else k
            if bare in cls.names:
                out[cls.prefix + bare] = torch.as_tensor(v).detach().cpu()
                found += 1
                continue
            stray = bare if cls.stray_under_prefix else k
            if not stray.startswith(DETECTOR_ROOTS):
                raise KeyError("%s: %r is not %s parameter" % (caller, stray, cls.a_noun or "a " + cls.noun))
        if found != len(cls.names):
            raise KeyError("%s: the %s state has %d of %d parameters" % (caller, cls.noun, found, len(cls.names)))
        return out
