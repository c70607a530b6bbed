"""The PCM resampler on the device: the Python side of C ABI part 11 (include/jsmpeg_hip.h, jsmpeg_hip_resampler_*).  PCM in
HBM -- float32 [frame][2][1152], as Mp2Batch and Mp2Live leave it, or a torch tensor -- -> a padded batch of waveforms for
models (form="waveform": [stream][channels][row] in float32 / float16 / bfloat16) or frames at another rate that Mp2Encoder
takes as they are (form="frames").  The rule: jsmpeg_amd/csrc/pcm_resample.h.  A call is a pure enqueue; sync() or a reader
of device results settles it.  torch is imported only when a tensor is handed in or asked for."""
import ctypes
import math

import numpy as np

from . import _pass
from . import batch as _batch
from ._pass import c_int, p_f32, p_u32, p_u64, u32, vp

END = 1
CHAIN = 2        # continue the call's streams where their last chained call left them (JSMPEG_HIP_RESAMPLE_CHAIN)

IN_RATES = (32000, 44100, 48000)
OUT_RATES = (8000, 16000, 22050, 24000, 32000, 44100, 48000)
FORMS = {"waveform": 0, "frames": 1}
DTYPES = _pass.DTYPES
SAMPLES_PER_FRAME = 1152


class ResamplerConfig(ctypes.Structure):
    _fields_ = [("in_rate", ctypes.c_uint32), ("out_rate", ctypes.c_uint32), ("channels_out", ctypes.c_uint32), ("form", ctypes.c_uint32),
                ("dtype", ctypes.c_uint32), ("gain", ctypes.c_float), ("max_streams", ctypes.c_uint32), ("max_frames", ctypes.c_uint32),
                ("row", ctypes.c_uint32), ("device", ctypes.c_int32)]


SIGNATURES = {
    "jsmpeg_hip_resampler_create": (vp, [ctypes.POINTER(ResamplerConfig)]),
    "jsmpeg_hip_resampler_destroy": (None, [vp]),
    "jsmpeg_hip_resampler_resample": (c_int, [vp, vp, vp, vp, u32, u32, vp]),
    "jsmpeg_hip_resampler_sync": (c_int, [vp]),
    "jsmpeg_hip_resampler_query": (c_int, [vp]),
    "jsmpeg_hip_resampler_out": (vp, [vp, p_u64]),
    "jsmpeg_hip_resampler_stream_out": (c_int, [vp, u32, p_u64, p_u64]),
    "jsmpeg_hip_resampler_chain_reset": (c_int, [vp, u32]),
    "jsmpeg_hip_resampler_chain_info": (c_int, [vp, u32, p_u64]),
    "jsmpeg_hip_resampler_timings": (c_int, [vp, p_f32]),
    "jsmpeg_hip_resample_plan": (c_int, [u32, u32, p_u32, p_u32, p_u32]),
    "jsmpeg_hip_resample_taps": (c_int, [u32, u32, vp]),
}
SYMBOLS = tuple(SIGNATURES)

_bound = None


def lib():
    """libjsmpeg_hip with the part-11 argtypes set"""
    global _bound
    if _bound is None:
        _bound = _pass.bind(_pass.lib(), SIGNATURES)
    return _bound


def plan(in_rate, out_rate):
    """(L, M, H) of a pair: out / gcd, in / gcd, the half width in input samples; no device needed"""
    l, m, h = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_uint32()
    if lib().jsmpeg_hip_resample_plan(in_rate, out_rate, ctypes.byref(l), ctypes.byref(m), ctypes.byref(h)) < 0:
        raise ValueError(_batch.last_error())
    return int(l.value), int(m.value), int(h.value)


def taps(in_rate, out_rate):
    """the pair's table, float32 [L][2 H]; no device needed"""
    l, _, h = plan(in_rate, out_rate)
    out = np.zeros((l, 2 * h), np.float32)
    if lib().jsmpeg_hip_resample_taps(in_rate, out_rate, out.ctypes.data) < 0:
        raise ValueError(_batch.last_error())
    return out


def outputs(in_rate, out_rate, n):
    """outputs of a stream after n input samples: ceil(n L / M)"""
    g = math.gcd(in_rate, out_rate)
    return -((-n * (out_rate // g)) // (in_rate // g))


class Resampler(_pass.RowPass):
    """PCM on the device -> PCM at another rate on the device.  chain=True on a call continues its streams -- the stream
    NUMBER is a stream's identity from call to call -- where their last chained call left them, and the pieces concatenated
    are bit for bit what one call over all the frames writes.  end=True lets the filter's tail (delay_seconds of it) come
    out.  gain multiplies every sample once: 2.0 undoes the decoders' half level in front of Mp2Encoder.  stream_out and
    counts: waveform -- the element index of a stream's first row and its samples per channel; frames -- its first frame and
    its whole frames."""
    PREFIX = "jsmpeg_hip_resampler_"

    def __init__(self, in_rate, out_rate, channels=2, form="waveform", dtype="float32", gain=1.0, max_streams=1, max_frames=1, row=None, device=-1):
        if form not in FORMS:
            raise ValueError("form: 'waveform' or 'frames'")
        if dtype not in DTYPES:
            raise ValueError("dtype: 'float32', 'float16' or 'bfloat16'")
        self.in_rate, self.out_rate, self.channels, self.form, self.dtype, self.gain = in_rate, out_rate, channels, form, dtype, float(gain)
        self.max_streams, self.max_frames = max_streams, max_frames
        cfg = ResamplerConfig(in_rate, out_rate, channels, FORMS[form], DTYPES[dtype], gain, max_streams, max_frames, row or 0, device)
        self._open(lib(), SIGNATURES, cfg)
        self.plan = plan(in_rate, out_rate)
        self.row = (row or outputs(in_rate, out_rate, max_frames * SAMPLES_PER_FRAME + self.plan[2])) if form == "waveform" else 0
        self.delay_seconds = self.plan[2] / in_rate
        self._numbers = []

    def resample(self, ptrs, frames, streams=None, chain=False, end=False, stream=None):
        """ptrs: one device address per stream, of its first frame ([frames][2][1152] float32, contiguous); frames: the count
        per stream (0 allowed); streams: ascending stream numbers (None: 0, 1, ..); chain: continue the streams; end: let the
        tail come out (with chain, the chains end behind this call); stream: the HIP stream to enqueue on -- the one the PCM
        was produced on."""
        self._submit("resample", "frames: one count per stream", ptrs, frames, streams, chain, end, stream)

    def resample_tensor(self, x, streams=None, chain=False, end=False):
        """x: a contiguous float32 CUDA tensor [S, F, 2, 1152] -- S streams of F frames; runs on torch's current stream of the
        tensor's device, right behind whatever produced the tensor there"""
        ptrs, frames, stream = _pass.frames_tensor(x, "resample_tensor")
        self.resample(ptrs, frames, streams, chain, end, stream)
        self._keep = x          # the tensor stays alive until the next call

    def resample_batch(self, mp2batch, streams=None, chain=False, end=False, stream=None):
        """every frame of an Mp2Batch's last decode, straight from its PCM in HBM (the batch's streams in order; streams:
        their stream numbers here).  A batch whose sampling rate is not in_rate is refused."""
        ptrs, counts = _pass.batch_frames(mp2batch, self.in_rate, "resample_batch", "the resampler takes")
        self.resample(ptrs, counts, streams, chain, end, stream)

    def resample_live(self, mp2live, chain=True, end=False, stream=None):
        """the frames of an Mp2Live's last tick from their device_pcm pointers (they lie stream after stream, a stream's frames
        contiguous).  chain=True: the live stream id IS the stream number (an id at or above max_streams is refused);
        otherwise the streams are numbered 0, 1, .. in the order of their ids.  Returns the tick's frames in that order."""
        frames, ptrs, counts, numbers = _pass.live_frames(mp2live, self.in_rate, self.max_streams, chain, "resample_live", "the resampler takes")
        self.resample(ptrs, counts, numbers, chain, end, stream)
        return frames

    def waveform(self):
        """the last call's padded batch as a torch tensor [streams of the call][channels][row] OVER the device buffer: no copy,
        valid until the handle's next call.  Settles the pass, so the tensor is safe on any torch stream."""
        if self.form != "waveform":
            raise ValueError("waveform(): the handle was made with form='frames'")
        return self._tensor((len(self._numbers), self.channels, self.row))

    def read(self):
        """the last call's buffer on the host: waveform -- [streams][channels][row] (bfloat16 as its uint16 bits); frames --
        float32 [frames][2][1152], the streams' whole frames one after the other"""
        return self._host(None if self.form == "frames" else (len(self._numbers), self.channels, self.row))

    def frames(self):
        """(ptrs, counts, stream numbers) of the last call's whole frames, ready for Mp2Encoder.encode(ptrs, counts, numbers,
        chain=True, stream=...) on the same HIP stream: closed form, nothing is waited for"""
        if self.form != "frames":
            raise ValueError("frames(): the handle was made with form='waveform'")
        base = self.device_out()[0]
        outs = [self.stream_out(s) for s in self._numbers]
        return [base + o * 2 * SAMPLES_PER_FRAME * 4 if c else 0 for o, c in outs], [c for _, c in outs], list(self._numbers)
