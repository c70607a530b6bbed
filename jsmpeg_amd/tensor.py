"""Decoded pictures as resized RGB torch tensors on the device: the Python side of C ABI part 7 (include/jsmpeg_hip.h,
jsmpeg_hip_*_render_tensor).  Batch.tensor, Live.tensor and Live.latest_tensor come here.  torch is imported when a
tensor is asked for, not before: jsmpeg_amd.batch and jsmpeg_amd.live import without it."""
import ctypes

import numpy as np

U8, F16, BF16, F32 = 0, 1, 2, 3
NCHW, NHWC = 0, 1
RGB, BGR = 0, 1
MAX_SIDE = 4096


class TensorDesc(ctypes.Structure):
    _fields_ = [(n, ctypes.c_uint32) for n in ("width", "height", "crop_x", "crop_y", "crop_width", "crop_height",
                                                "dtype", "layout", "order", "antialias")] + \
               [("mean", ctypes.c_float * 3), ("std", ctypes.c_float * 3)]


SYMBOLS = ("jsmpeg_hip_batch_render_tensor", "jsmpeg_hip_live_render_tensor", "jsmpeg_hip_live_render_tensor_latest")
ROI_SYMBOLS = ("jsmpeg_hip_batch_render_tensor_rois", "jsmpeg_hip_live_render_tensor_rois",
               "jsmpeg_hip_live_render_tensor_rois_latest")
ROI_EMPTY, ROI_INSIDE, ROI_CLIPPED = 0, 1, 2          # a row's status (include/jsmpeg_hip.h, jsmpeg_hip_roi_t)


def bind(L):
    """argtypes of the three part-7 functions on a loaded libjsmpeg_hip"""
    vp, u32 = ctypes.c_void_p, ctypes.c_uint32
    for name in SYMBOLS[:2]:
        fn = getattr(L, name)
        fn.restype = ctypes.c_int
        fn.argtypes = [vp, vp, u32, ctypes.POINTER(TensorDesc), vp, vp]
    L.jsmpeg_hip_live_render_tensor_latest.restype = ctypes.c_int
    L.jsmpeg_hip_live_render_tensor_latest.argtypes = [vp, vp, u32, ctypes.POINTER(TensorDesc), vp, vp, vp]
    for name in ROI_SYMBOLS:
        fn = getattr(L, name)
        fn.restype = ctypes.c_int
        fn.argtypes = [vp, vp, u32, ctypes.POINTER(TensorDesc), vp, u32, vp, vp, vp] + ([vp] if name.endswith("latest") else [])
    return L


def current_device():
    """the HIP device current in this thread (what a handle created with device=-1 decodes on), or None when the HIP runtime
    cannot be asked here (torch's current device is taken then)"""
    try:
        hip = ctypes.CDLL("libamdhip64.so")
    except OSError:
        return None
    d = ctypes.c_int(-1)
    return d.value if hip.hipGetDevice(ctypes.byref(d)) == 0 else None


def _dtype(torch, dtype):
    table = {torch.uint8: U8, torch.float16: F16, torch.bfloat16: BF16, torch.float32: F32}
    names = {"uint8": torch.uint8, "u8": torch.uint8, "float16": torch.float16, "half": torch.float16, "f16": torch.float16,
             "bfloat16": torch.bfloat16, "bf16": torch.bfloat16, "float32": torch.float32, "float": torch.float32,
             "f32": torch.float32}
    if dtype is None:
        dtype = torch.float32
    if isinstance(dtype, str):
        if dtype.lower() not in names:
            raise ValueError("dtype %r: one of uint8, float16, bfloat16, float32" % dtype)
        dtype = names[dtype.lower()]
    if dtype not in table:
        raise ValueError("dtype %r: one of torch.uint8, float16, bfloat16, float32" % (dtype,))
    return dtype, table[dtype]


def _choice(value, options, what):
    v = str(value).lower()
    if v not in options:
        raise ValueError("%s %r: one of %s" % (what, value, ", ".join(options)))
    return options[v]


def indices(items, default_count):
    """None -> (None, default_count); a range, list or integer array -> (uint32 array, its length)"""
    if items is None:
        return None, int(default_count)
    a = np.asarray(list(items) if isinstance(items, range) else items)
    if a.ndim != 1 or (a.size and not np.issubdtype(a.dtype, np.integer)):
        raise ValueError("pictures / streams: a 1-D list of integers")
    if a.size and (a.min() < 0 or a.max() >= 1 << 32):
        raise ValueError("pictures / streams: indices must be 0 .. 2^32 - 1")
    return np.ascontiguousarray(a, dtype=np.uint32), int(a.size)


def render(call, device, width, height, count, size=None, crop=None, dtype=None, layout="nchw", order="rgb", antialias=True,
           mean=None, std=None, out=None):
    """Checks and allocates the output of `count` pictures, then call(desc, out_ptr, stream) on torch's current stream of
    `device` (the C function's return code: < 0 raises RuntimeError in the caller's _ok).  Returns the tensor."""
    import torch
    dev = torch.device("cuda", torch.cuda.current_device() if device is None or device < 0 else device)
    tdtype, code = _dtype(torch, dtype)
    lay = _choice(layout, {"nchw": NCHW, "nhwc": NHWC}, "layout")
    ordr = _choice(order, {"rgb": RGB, "bgr": BGR}, "order")
    if crop is None:
        cx, cy, cw, ch = 0, 0, 0, 0
    else:
        cx, cy, cw, ch = (int(v) for v in crop)
        if min(cx, cy, cw, ch) < 0:
            raise ValueError("crop %r: (x, y, width, height), none negative" % (crop,))
    if size is None:
        oh, ow = (ch, cw) if cw or ch else (height, width)
    else:
        oh, ow = (int(v) for v in size)
    if not (1 <= ow <= MAX_SIDE and 1 <= oh <= MAX_SIDE):
        raise ValueError("size %r: (height, width), each 1 .. %d" % ((oh, ow), MAX_SIDE))
    m = [0.0, 0.0, 0.0] if mean is None else [float(v) for v in mean]
    s = [1.0, 1.0, 1.0] if std is None else [float(v) for v in std]
    if len(m) != 3 or len(s) != 3:
        raise ValueError("mean / std: three values, in the tensor's channel order")
    shape = (count, 3, oh, ow) if lay == NCHW else (count, oh, ow, 3)
    if out is None:
        out = torch.empty(shape, dtype=tdtype, device=dev)
    elif not isinstance(out, torch.Tensor) or tuple(out.shape) != shape or out.dtype != tdtype or out.device != dev \
            or not out.is_contiguous():
        raise ValueError("out: a contiguous %s tensor of shape %r on %s is needed, got %s" % (
            tdtype, shape, dev, ("%s %r on %s%s" % (out.dtype, tuple(out.shape), out.device, "" if out.is_contiguous() else ", not contiguous"))
            if isinstance(out, torch.Tensor) else type(out).__name__))
    desc = TensorDesc(ow, oh, cx, cy, cw, ch, code, lay, ordr, 1 if antialias else 0, (ctypes.c_float * 3)(*m), (ctypes.c_float * 3)(*s))
    stream = torch.cuda.current_stream(dev).cuda_stream
    call(ctypes.byref(desc), out.data_ptr() if count else None, stream)
    return out


def render_rois(call, device, width, height, rois, size, dtype=None, layout="nchw", order="rgb", antialias=True, mean=None,
                std=None, out=None):
    """A row per region of interest: `rois` goes to the handle's device as int32 [R, 5] (row, x, y, width, height) -- an int32
    CUDA tensor of that shape there is used in place, anything else array-like is copied -- then render() with
    call(desc, rois_ptr, R, out_ptr, status_ptr, stream).  Returns (tensor, status); no host wait."""
    import torch
    if size is None:
        raise ValueError("size: (height, width) is required with rois (every row has a box of its own)")
    dev = torch.device("cuda", torch.cuda.current_device() if device is None or device < 0 else device)
    if isinstance(rois, torch.Tensor):
        if rois.is_floating_point() or rois.is_complex() or rois.dtype == torch.bool:
            raise ValueError("rois: integers (row, x, y, width, height) are needed, got %s (rois_from_xyxy makes them of float boxes)" % rois.dtype)
        r = rois
    else:
        a = np.asarray(rois)
        if a.size and not np.issubdtype(a.dtype, np.integer):
            raise ValueError("rois: integers (row, x, y, width, height) are needed, got %s" % a.dtype)
        a = a.reshape(0, 5) if a.size == 0 else a
        if a.size and (a.min() < -(1 << 31) or a.max() >= 1 << 31):
            raise ValueError("rois: values must be int32")
        r = torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32))
    if r.dim() != 2 or r.shape[1] != 5:
        raise ValueError("rois: shape [R, 5] (row, x, y, width, height) is needed, got %r" % (tuple(r.shape),))
    if r.dtype != torch.int32 and r.numel() and (int(r.min()) < -(1 << 31) or int(r.max()) >= 1 << 31):      # (a host wait: pass int32)
        raise ValueError("rois: values must be int32")
    r = r.to(device=dev, dtype=torch.int32).contiguous()          # (itself when it is int32, contiguous and there)
    n = int(r.shape[0])
    status = torch.empty((n,), dtype=torch.uint8, device=dev)
    t = render(lambda d, o, st: call(d, r.data_ptr() if n else None, n, o, status.data_ptr() if n else None, st),
               device, width, height, n, size, None, dtype, layout, order, antialias, mean, std, out)
    return t, status


def rois_from_xyxy(boxes, rows, scale=(1, 1), pad=0):
    """Float boxes [R, 4] (x1, y1, x2, y2), as a detector gives them, and the picture index `rows` [R] of each -> int32 [R, 5]
    (row, x, y, width, height) for tensor_rois, in torch ops on the boxes' device (no host step): the coordinates times
    scale = (sx, sy) -- the detector's input to display pixels -- grown by `pad` pixels on every side, then the smallest
    pixel rectangle that covers them (floor of the near edges, ceil of the far ones).  A box with a NaN gets width 0 (status
    0); values beyond int32 are clamped.  The box is NOT clipped to the picture: the render does that and reports it."""
    import torch
    b = torch.as_tensor(boxes)
    if b.dim() != 2 or b.shape[1] != 4:
        raise ValueError("boxes: shape [R, 4] (x1, y1, x2, y2) is needed, got %r" % (tuple(b.shape),))
    rows = torch.as_tensor(rows, device=b.device)
    if rows.dim() != 1 or rows.shape[0] != b.shape[0] or rows.is_floating_point():
        raise ValueError("rows: %d integers are needed, one per box" % b.shape[0])
    sx, sy = (float(scale), float(scale)) if isinstance(scale, (int, float)) else (float(v) for v in scale)
    lim = (-float(1 << 31), float((1 << 31) - 1))
    b = b.to(torch.float64)
    bad = torch.isnan(b).any(dim=1)
    b = torch.nan_to_num(b, nan=0.0) * torch.tensor([sx, sy, sx, sy], dtype=torch.float64, device=b.device)
    lo = torch.floor(b[:, :2] - float(pad)).clamp(*lim).to(torch.int64)
    hi = torch.ceil(b[:, 2:] + float(pad)).clamp(*lim).to(torch.int64)
    wh = (hi - lo).clamp(int(lim[0]), int(lim[1]))
    wh = torch.where(bad[:, None], torch.zeros_like(wh), wh)
    return torch.cat([rows.to(torch.int64).clamp(int(lim[0]), int(lim[1]))[:, None], lo, wh], dim=1).to(torch.int32)
