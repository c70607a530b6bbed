"""Log-mel features on the device: the Python side of C ABI part 12 (include/jsmpeg_hip.h, jsmpeg_hip_logmel_*).  Float32 mono
PCM in HBM -- a Resampler's waveform read in place, a torch tensor, raw pointers -- -> log-mel spectrograms
[stream][n_mels][row] (layout="mel_major", what Whisper reads) or [stream][row][n_mels] ("time_major") in float32 / float16 /
bfloat16.  The rule: jsmpeg_amd/csrc/logmel.h.  A call is a pure enqueue; sync() or a reader of device results settles it.
torch is imported only when a tensor is handed in or asked for."""
import ctypes

import numpy as np

from . import _pass
from . import batch as _batch
from ._pass import c_int, p_f32, p_u64, u32, u64, vp

END = 1
CHAIN = 2        # continue the call's streams where their last chained call left them (JSMPEG_HIP_LOGMEL_CHAIN)

SCALES = {"power": 0, "log": 1, "log10": 2, "db": 3, "whisper": 4}
LAYOUTS = {"mel_major": 0, "time_major": 1}
MEL_SCALES = {"htk": 0, "slaney": 1}
MEL_NORMS = {"none": 0, None: 0, "slaney": 1}
DTYPES = _pass.DTYPES


class LogMelConfig(ctypes.Structure):
    _fields_ = [("sample_rate", ctypes.c_uint32), ("n_fft", ctypes.c_uint32), ("hop", ctypes.c_uint32), ("n_mels", ctypes.c_uint32),
                ("f_min", ctypes.c_float), ("f_max", ctypes.c_float), ("mel_scale", ctypes.c_uint32), ("mel_norm", ctypes.c_uint32),
                ("window", ctypes.c_void_p), ("floor", ctypes.c_float), ("scale", ctypes.c_uint32), ("layout", ctypes.c_uint32),
                ("dtype", ctypes.c_uint32), ("max_streams", ctypes.c_uint32), ("max_samples", ctypes.c_uint32), ("row", ctypes.c_uint32),
                ("device", ctypes.c_int32)]


_cfg = ctypes.POINTER(LogMelConfig)
SIGNATURES = {
    "jsmpeg_hip_logmel_create": (vp, [_cfg]),
    "jsmpeg_hip_logmel_destroy": (None, [vp]),
    "jsmpeg_hip_logmel_features": (c_int, [vp, vp, vp, vp, u32, u32, vp]),
    "jsmpeg_hip_logmel_sync": (c_int, [vp]),
    "jsmpeg_hip_logmel_query": (c_int, [vp]),
    "jsmpeg_hip_logmel_out": (vp, [vp, p_u64]),
    "jsmpeg_hip_logmel_stream_out": (c_int, [vp, u32, p_u64, p_u64]),
    "jsmpeg_hip_logmel_chain_reset": (c_int, [vp, u32]),
    "jsmpeg_hip_logmel_chain_info": (c_int, [vp, u32, p_u64]),
    "jsmpeg_hip_logmel_timings": (c_int, [vp, p_f32]),
    "jsmpeg_hip_logmel_plan": (c_int, [_cfg, u64, p_u64]),
    "jsmpeg_hip_logmel_basis": (c_int, [_cfg, vp]),
    "jsmpeg_hip_logmel_filters": (c_int, [_cfg, vp, vp]),
}
SYMBOLS = tuple(SIGNATURES)

_bound = None


def lib():
    """libjsmpeg_hip with the part-12 argtypes set"""
    global _bound
    if _bound is None:
        _bound = _pass.bind(_pass.lib(), SIGNATURES)
    return _bound


def _config(sample_rate=16000, n_fft=400, hop=160, n_mels=80, f_min=0.0, f_max=0.0, mel_scale="slaney", mel_norm="slaney", window=None, floor=1e-10,
            scale="log10", layout="mel_major", dtype="float32", max_streams=1, max_samples=1, row=None, device=-1):
    """(LogMelConfig, what keeps its window alive)"""
    for name, value, table in (("scale", scale, SCALES), ("layout", layout, LAYOUTS), ("mel_scale", mel_scale, MEL_SCALES), ("mel_norm", mel_norm, MEL_NORMS),
                               ("dtype", dtype, DTYPES)):
        if value not in table:
            raise ValueError("%s: one of %s" % (name, ", ".join(repr(k) for k in table if k is not None)))
    w = None
    if window is not None:
        w = np.ascontiguousarray(window, dtype=np.float32)
        if w.shape != (n_fft,):
            raise ValueError("window: n_fft floats")
    cfg = LogMelConfig(sample_rate, n_fft, hop, n_mels, f_min, f_max, MEL_SCALES[mel_scale], MEL_NORMS[mel_norm], None if w is None else w.ctypes.data, floor,
                       SCALES[scale], LAYOUTS[layout], DTYPES[dtype], max_streams, max_samples, row or 0, device)
    return cfg, w


def plan(n=0, **config):
    """dict(bins, cols, frames_open, frames_end, frames_per_workgroup, lds_bytes, carry, row) of a config and n samples; no device
    needed"""
    cfg, _w = _config(**config)
    out = (ctypes.c_uint64 * 8)()
    if lib().jsmpeg_hip_logmel_plan(ctypes.byref(cfg), n, out) < 0:
        raise ValueError(_batch.last_error())
    return dict(zip(("bins", "cols", "frames_open", "frames_end", "frames_per_workgroup", "lds_bytes", "carry", "row"), (int(v) for v in out)))


def frames(n, end, n_fft=400, hop=160):
    """frames of a stream that has taken n samples in all: the closed form, from the library"""
    return plan(n, n_fft=n_fft, hop=hop, n_mels=1, mel_scale="htk", mel_norm="none")["frames_end" if end else "frames_open"]


def basis(**config):
    """the basis with the window folded in, float32 [n_fft][padded columns]: column 2 b = w cos, 2 b + 1 = -w sin; no device needed"""
    cfg, _w = _config(**config)
    out = np.zeros((cfg.n_fft, plan(**config)["cols"]), np.float32)
    if lib().jsmpeg_hip_logmel_basis(ctypes.byref(cfg), out.ctypes.data) < 0:
        raise ValueError(_batch.last_error())
    return out


def filters(**config):
    """(the filterbank float32 [n_mels][bins], the ranges int32 [n_mels][2] = lo, hi of each row's nonzero span); no device needed"""
    cfg, _w = _config(**config)
    fb = np.zeros((cfg.n_mels, plan(**config)["bins"]), np.float32)
    rg = np.zeros((cfg.n_mels, 2), np.int32)
    if lib().jsmpeg_hip_logmel_filters(ctypes.byref(cfg), fb.ctypes.data, rg.ctypes.data) < 0:
        raise ValueError(_batch.last_error())
    return fb, rg


class LogMel(_pass.RowPass):
    """Float32 mono PCM on the device -> log-mel features on the device.  chain=True on a call continues its streams -- the
    stream NUMBER is a stream's identity from call to call -- and the pieces concatenated are bit for bit the frames of one
    call.  end=True ends the streams: the reflection at the end and the last frames come out.  stream_out and counts: the
    element index of a stream's first row and its frames."""
    PREFIX = "jsmpeg_hip_logmel_"

    def __init__(self, sample_rate=16000, n_fft=400, hop=160, n_mels=80, f_min=0.0, f_max=0.0, mel_scale="slaney", mel_norm="slaney", window=None,
                 floor=1e-10, scale="log10", layout="mel_major", dtype="float32", max_streams=1, max_samples=1, row=None, device=-1):
        self.config = dict(sample_rate=sample_rate, n_fft=n_fft, hop=hop, n_mels=n_mels, f_min=f_min, f_max=f_max, mel_scale=mel_scale, mel_norm=mel_norm,
                           window=window, floor=floor, scale=scale, layout=layout, dtype=dtype, max_streams=max_streams, max_samples=max_samples, row=row,
                           device=device)
        cfg, _w = _config(**self.config)
        self._open(lib(), SIGNATURES, cfg)
        self.n_fft, self.hop, self.n_mels, self.scale, self.layout, self.dtype = n_fft, hop, n_mels, scale, layout, dtype
        self.max_streams, self.max_samples = max_streams, max_samples
        self.row = plan(**self.config)["row"]
        self._numbers = []
        self._keep = None

    def _enqueue(self, ptrs, samples, streams, chain, end, stream):
        self._submit("features", "counts: one sample count per stream", ptrs, samples, streams, chain, end, stream)

    def features(self, source, counts=None, streams=None, chain=False, end=None, stream=None, channel=0):
        """source: a Resampler whose last call was form="waveform", dtype="float32" -- read in place on the device, nothing is
        waited for, the call is enqueued on the HIP stream `stream` (the one the resampler ran on); channel picks the row of a
        two-channel resampler; counts=None takes each stream's valid count, counts="row" the whole zero-padded row (Whisper's
        "pad to 30 s").  Or a contiguous float32 CUDA tensor [S, N] with optional counts (None: N each), on torch's current
        stream of its device.  Or a list of device addresses with counts, on `stream`.
        streams: ascending stream numbers (None: 0, 1, ..); chain: continue the streams; end: the streams end with this call
        (None: True for an unchained call, False for a chained one)."""
        end = (not chain) if end is None else end
        if hasattr(source, "device_out") and hasattr(source, "stream_out"):
            if getattr(source, "form", None) != "waveform" or getattr(source, "dtype", None) != "float32":
                raise ValueError("features: the Resampler must have form='waveform' and dtype='float32' (it has %r, %r)" % (getattr(source, "form", None), getattr(source, "dtype", None)))
            if not 0 <= channel < source.channels:
                raise ValueError("features: channel %d of a %d-channel resampler" % (channel, source.channels))
            if counts is not None and counts != "row":
                raise ValueError("features: counts is None or 'row' for a Resampler")
            base = source.device_out()[0]
            outs = [source.stream_out(s) for s in source.numbers()]
            ptrs = [base + (o + channel * source.row) * 4 for o, _ in outs]
            self._enqueue(ptrs, [source.row if counts == "row" else c for _, c in outs], streams, chain, end, stream)
            self._keep = source
            return
        if isinstance(source, (list, tuple)):
            if counts is None:
                raise ValueError("features: device addresses need counts")
            self._enqueue(list(source), counts, streams, chain, end, stream)
            return
        import torch
        x = source
        if not isinstance(x, torch.Tensor) or x.dtype != torch.float32 or not x.is_cuda or x.dim() != 2 or not x.is_contiguous():
            raise ValueError("features: a Resampler, a contiguous float32 CUDA tensor [S, N] or a list of device addresses is needed")
        s, n = int(x.shape[0]), int(x.shape[1])
        cnt = [n] * s if counts is None else [int(c) for c in counts]
        if len(cnt) != s or any(c < 0 or c > n for c in cnt):
            raise ValueError("features: one count in 0 .. N per stream")
        self._enqueue([x.data_ptr() + i * n * 4 if n else 0 for i in range(s)], cnt, streams, chain, end, torch.cuda.current_stream(x.device).cuda_stream)
        self._keep = x          # the tensor stays alive until the next call

    def shape(self):
        n = len(self._numbers)
        return (n, self.n_mels, self.row) if self.layout == "mel_major" else (n, self.row, self.n_mels)

    def tensor(self):
        """the last call's features as a torch tensor OVER the device buffer: no copy, valid until the handle's next call.
        Settles the pass, so the tensor is safe on any torch stream."""
        return self._tensor(self.shape())

    def read(self):
        """the last call's features on the host (bfloat16 as its uint16 bits)"""
        return self._host(self.shape())
