"""YUV 4:2:0 frames as video decoders hand them out (include/apse_hip.h, "YUV 4:2:0 frames").

``YuvFrame(data, width=None, format="NV12")`` wraps one frame without copying it:

* NV12: ``data`` is a 2-D uint8 array (host) or CUDA tensor (a decoder surface) of shape ``(H + CH, pitch)`` -- ``H`` luma rows,
  then ``CH = (H + 1) // 2`` rows of interleaved (U, V) pairs; ``width`` defaults to the pitch;
* I420: ``(3 H / 2, W)``: the packed luma plane, then the U and the V plane (``W`` and ``H`` even).

``H`` is recovered as ``2 * rows // 3``.  ``.shape`` is ``(H, W, 3)``, what the frame converts to, so code that asks a frame for
its size keeps working.  Everything that takes a BGR frame takes a ``YuvFrame``; a bare 2-D array is wrapped when
``cfg.INPUT.FORMAT`` is "NV12" or "I420".  Nothing here touches the GPU.
"""
import numpy as np

FORMATS = {"NV12": 0, "I420": 1}                                                           # APSE_FMT_*
MATRICES = {"cv601": 0, "bt601": 1, "bt709": 2, "bt601-full": 3, "bt709-full": 4}          # APSE_YUV_*


def matrix_index(name):
    try:
        return MATRICES[str(name)]
    except KeyError:
        raise ValueError("unknown YUV matrix %r (one of %s)" % (name, ", ".join(MATRICES))) from None


def _is_tensor(a):
    return hasattr(a, "is_cuda")


class YuvFrame:
    __slots__ = ("data", "height", "width", "pitch", "format")

    def __init__(self, data, width=None, format="NV12"):
        fmt = str(format).upper()
        if fmt not in FORMATS:
            raise ValueError("unknown YUV format %r (NV12 or I420)" % (format,))
        if _is_tensor(data):
            ok = data.dim() == 2 and str(data.dtype) == "torch.uint8" and data.is_contiguous()
            if ok and not data.is_cuda:
                data, ok = data.numpy(), True
        else:
            data = np.asarray(data)
            ok = data.ndim == 2 and data.dtype == np.uint8
        if not ok:
            raise ValueError("a %s frame is a contiguous 2-D uint8 array of shape (rows, pitch), got %s %s"
                             % (fmt, getattr(data, "dtype", None), tuple(getattr(data, "shape", ()))))
        rows, pitch = int(data.shape[0]), int(data.shape[1])
        W = pitch if width is None else int(width)
        H = 2 * rows // 3
        CH, CW = (H + 1) // 2, (W + 1) // 2
        if H < 1 or W < 1:
            raise ValueError("empty %s frame: %d rows, width %d" % (fmt, rows, W))
        if fmt == "NV12":
            if H + CH != rows:
                raise ValueError("NV12: %d rows are no H + (H + 1) // 2" % rows)
            if pitch < max(W, 2 * CW):
                raise ValueError("NV12: pitch %d below max(W, 2 * ((W + 1) // 2)) = %d" % (pitch, max(W, 2 * CW)))
        else:
            if W != pitch:
                raise ValueError("I420 is packed: width %d must equal the row length %d" % (W, pitch))
            if (W & 1) or (H & 1) or 3 * H != 2 * rows:
                raise ValueError("I420 needs an even width and height (got %d rows of %d)" % (rows, W))
        if not _is_tensor(data) and not data.flags["C_CONTIGUOUS"]:
            data = np.ascontiguousarray(data)
        self.data, self.height, self.width, self.pitch, self.format = data, H, W, pitch, fmt

    @property
    def shape(self):
        return (self.height, self.width, 3)

    @property
    def rows(self):
        return int(self.data.shape[0])

    @property
    def is_cuda(self):
        return _is_tensor(self.data)

    @property
    def geometry(self):
        """What two frames must share to travel in one batch."""
        return (self.rows, self.pitch, self.width, self.format)

    def __repr__(self):
        return "YuvFrame(%s %dx%d, pitch %d, %s)" % (self.format, self.width, self.height, self.pitch, "cuda" if self.is_cuda else "host")


class YuvBatch:
    """``B`` contiguous frames of one geometry on the device: a uint8 CUDA tensor ``(B, rows, pitch)`` and what the library needs
    to read it.  What ``FrameUploader`` hands to ``TrackRCNN.preprocess_frames`` for YUV input; a device ``YuvFrame`` becomes one
    without a copy."""
    __slots__ = ("dev", "height", "width", "pitch", "format")

    def __init__(self, dev, height, width, pitch, format):
        self.dev, self.height, self.width, self.pitch, self.format = dev, int(height), int(width), int(pitch), format

    @classmethod
    def of(cls, frames):
        """From device ``YuvFrame``s: one frame is viewed in place, several are gathered into one tensor."""
        import torch
        f0 = frames[0]
        for f in frames:
            if f.geometry != f0.geometry:
                raise ValueError("frames of one batch must have the same size, pitch and format")
        dev = f0.data[None] if len(frames) == 1 else torch.stack([f.data for f in frames])
        return cls(dev, f0.height, f0.width, f0.pitch, f0.format)

    @property
    def shape(self):
        return (int(self.dev.shape[0]), self.height, self.width, 3)


def as_yuv(frame, input_format):
    """The frame as a ``YuvFrame`` under ``cfg.INPUT.FORMAT`` "NV12" / "I420": a ``YuvFrame`` as it is, a bare 2-D array wrapped
    (its width is its pitch)."""
    if isinstance(frame, YuvFrame):
        return frame
    if getattr(frame, "ndim", None) != 2 and not (_is_tensor(frame) and frame.dim() == 2):
        raise ValueError("INPUT.FORMAT = %s takes YuvFrame objects or 2-D uint8 arrays (rows, pitch), got shape %s"
                         % (input_format, tuple(getattr(frame, "shape", ()))))
    return YuvFrame(frame, None, input_format)
