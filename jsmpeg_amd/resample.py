"""The PCM resampler on the device: the Python side of C ABI part 11 (include/jsmpeg_hip.h, jsmpeg_hip_resampler_*).  PCM in
HBM -- float32 [frame][2][1152], as Mp2Batch and Mp2Live leave it, or a torch tensor -- -> a padded batch of waveforms for
models (form="waveform": [stream][channels][row] in float32 / float16 / bfloat16) or frames at another rate that Mp2Encoder
takes as they are (form="frames").  The rule: jsmpeg_amd/csrc/pcm_resample.h.  A call is a pure enqueue; sync() or a reader
of device results settles it.  torch is imported only when a tensor is handed in or asked for."""
import ctypes
import math

import numpy as np

from . import batch as _batch

END = 1
CHAIN = 2        # continue the call's streams where their last chained call left them (JSMPEG_HIP_RESAMPLE_CHAIN)

SYMBOLS = ("jsmpeg_hip_resampler_create", "jsmpeg_hip_resampler_destroy", "jsmpeg_hip_resampler_resample", "jsmpeg_hip_resampler_sync",
           "jsmpeg_hip_resampler_query", "jsmpeg_hip_resampler_out", "jsmpeg_hip_resampler_stream_out", "jsmpeg_hip_resampler_chain_reset",
           "jsmpeg_hip_resampler_chain_info", "jsmpeg_hip_resampler_timings", "jsmpeg_hip_resample_plan", "jsmpeg_hip_resample_taps")

IN_RATES = (32000, 44100, 48000)
OUT_RATES = (8000, 16000, 22050, 24000, 32000, 44100, 48000)
FORMS = {"waveform": 0, "frames": 1}
DTYPES = {"float32": 0, "float16": 1, "bfloat16": 2}
SAMPLES_PER_FRAME = 1152


class ResamplerConfig(ctypes.Structure):
    _fields_ = [("in_rate", ctypes.c_uint32), ("out_rate", ctypes.c_uint32), ("channels_out", ctypes.c_uint32), ("form", ctypes.c_uint32),
                ("dtype", ctypes.c_uint32), ("gain", ctypes.c_float), ("max_streams", ctypes.c_uint32), ("max_frames", ctypes.c_uint32),
                ("row", ctypes.c_uint32), ("device", ctypes.c_int32)]


_bound = None


def lib():
    """libjsmpeg_hip with the part-11 argtypes set"""
    global _bound
    if _bound is None:
        L = _batch.lib()
        vp, u32, u64 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64
        L.jsmpeg_hip_resampler_create.restype = vp
        L.jsmpeg_hip_resampler_create.argtypes = [ctypes.POINTER(ResamplerConfig)]
        L.jsmpeg_hip_resampler_destroy.restype = None
        L.jsmpeg_hip_resampler_destroy.argtypes = [vp]
        L.jsmpeg_hip_resampler_resample.restype = ctypes.c_int
        L.jsmpeg_hip_resampler_resample.argtypes = [vp, vp, vp, vp, u32, u32, vp]
        for name in ("jsmpeg_hip_resampler_sync", "jsmpeg_hip_resampler_query"):
            getattr(L, name).restype = ctypes.c_int
            getattr(L, name).argtypes = [vp]
        L.jsmpeg_hip_resampler_out.restype = vp
        L.jsmpeg_hip_resampler_out.argtypes = [vp, ctypes.POINTER(u64)]
        L.jsmpeg_hip_resampler_stream_out.restype = ctypes.c_int
        L.jsmpeg_hip_resampler_stream_out.argtypes = [vp, u32, ctypes.POINTER(u64), ctypes.POINTER(u64)]
        L.jsmpeg_hip_resampler_chain_reset.restype = ctypes.c_int
        L.jsmpeg_hip_resampler_chain_reset.argtypes = [vp, u32]
        L.jsmpeg_hip_resampler_chain_info.restype = ctypes.c_int
        L.jsmpeg_hip_resampler_chain_info.argtypes = [vp, u32, ctypes.POINTER(u64)]
        L.jsmpeg_hip_resampler_timings.restype = ctypes.c_int
        L.jsmpeg_hip_resampler_timings.argtypes = [vp, ctypes.POINTER(ctypes.c_float)]
        L.jsmpeg_hip_resample_plan.restype = ctypes.c_int
        L.jsmpeg_hip_resample_plan.argtypes = [u32, u32, ctypes.POINTER(u32), ctypes.POINTER(u32), ctypes.POINTER(u32)]
        L.jsmpeg_hip_resample_taps.restype = ctypes.c_int
        L.jsmpeg_hip_resample_taps.argtypes = [u32, u32, vp]
        L.jsmpeg_hip_device_read.restype = ctypes.c_int
        L.jsmpeg_hip_device_read.argtypes = [vp, vp, u64]
        _bound = L
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


class Resampler:
    """PCM on the device -> PCM at another rate on the device.  chain=True on a call continues its streams -- the stream
    NUMBER is a stream's identity from call to call -- where their last chained call left them, and the pieces concatenated
    are bit for bit what one call over all the frames writes.  end=True lets the filter's tail (delay_seconds of it) come
    out.  gain multiplies every sample once: 2.0 undoes the decoders' half level in front of Mp2Encoder."""

    def __init__(self, in_rate, out_rate, channels=2, form="waveform", dtype="float32", gain=1.0, max_streams=1, max_frames=1, row=None, device=-1):
        if form not in FORMS:
            raise ValueError("form: 'waveform' or 'frames'")
        if dtype not in DTYPES:
            raise ValueError("dtype: 'float32', 'float16' or 'bfloat16'")
        self.L = lib()
        self.in_rate, self.out_rate, self.channels, self.form, self.dtype, self.gain = in_rate, out_rate, channels, form, dtype, float(gain)
        self.max_streams, self.max_frames = max_streams, max_frames
        cfg = ResamplerConfig(in_rate, out_rate, channels, FORMS[form], DTYPES[dtype], gain, max_streams, max_frames, row or 0, device)
        self.h = self.L.jsmpeg_hip_resampler_create(ctypes.byref(cfg))
        if not self.h:
            raise RuntimeError("jsmpeg_hip_resampler_create: " + _batch.last_error())
        self.plan = plan(in_rate, out_rate)
        self.row = (row or outputs(in_rate, out_rate, max_frames * SAMPLES_PER_FRAME + self.plan[2])) if form == "waveform" else 0
        self.delay_seconds = self.plan[2] / in_rate
        self._numbers = []

    def _ok(self, rc):
        if rc < 0:
            raise RuntimeError(_batch.last_error())
        return rc

    def close(self):
        if self.h:
            self.L.jsmpeg_hip_resampler_destroy(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def resample(self, ptrs, frames, streams=None, chain=False, end=False, stream=None):
        """ptrs: one device address per stream, of its first frame ([frames][2][1152] float32, contiguous); frames: the count
        per stream (0 allowed); streams: ascending stream numbers (None: 0, 1, ..); chain: continue the streams; end: let the
        tail come out (with chain, the chains end behind this call); stream: the HIP stream to enqueue on -- the one the PCM
        was produced on."""
        n = len(ptrs)
        fr = np.ascontiguousarray(frames, dtype=np.uint32)
        if fr.shape != (n,):
            raise ValueError("frames: one count per stream")
        st = None if streams is None else np.ascontiguousarray(streams, dtype=np.uint32)
        if st is not None and st.shape != (n,):
            raise ValueError("streams: one stream number per stream")
        arr = (ctypes.c_void_p * max(1, n))(*[int(p) if p else None for p in ptrs])
        self._ok(self.L.jsmpeg_hip_resampler_resample(self.h, arr, fr.ctypes.data, None if st is None else st.ctypes.data, n,
                                                      (END if end else 0) | (CHAIN if chain else 0), stream))
        self._numbers = list(range(n)) if st is None else [int(v) for v in st]

    def resample_tensor(self, x, streams=None, chain=False, end=False):
        """x: a contiguous float32 CUDA tensor [S, F, 2, 1152] -- S streams of F frames; runs on torch's current stream of the
        tensor's device, right behind whatever produced the tensor there"""
        import torch
        if not isinstance(x, torch.Tensor) or x.dtype != torch.float32 or not x.is_cuda or x.dim() != 4 or not x.is_contiguous() or \
                tuple(x.shape[2:]) != (2, SAMPLES_PER_FRAME):
            raise ValueError("resample_tensor: a contiguous float32 CUDA tensor [S, F, 2, 1152] is needed")
        s, f = int(x.shape[0]), int(x.shape[1])
        step = f * 2 * SAMPLES_PER_FRAME * 4
        self.resample([x.data_ptr() + i * step if f else 0 for i in range(s)], [f] * s, streams, chain, end,
                      torch.cuda.current_stream(x.device).cuda_stream)
        self._keep = x          # the tensor stays alive until the next call

    def resample_batch(self, mp2batch, streams=None, chain=False, end=False, stream=None):
        """every frame of an Mp2Batch's last decode, straight from its PCM in HBM (the batch's streams in order; streams:
        their stream numbers here).  A batch whose sampling rate is not in_rate is refused."""
        n = mp2batch.n_streams
        counts = [mp2batch.frame_count(s) for s in range(n)]
        for s in range(n):
            if counts[s] and mp2batch.frame_info(s, 0)[2] != self.in_rate:
                raise ValueError("resample_batch: stream %d is sampled at %d Hz, the resampler takes %d" % (s, mp2batch.frame_info(s, 0)[2], self.in_rate))
        base, before = mp2batch.pcm_device_pointer(), 0
        ptrs = []
        for c in counts:
            ptrs.append(base + before * 2 * SAMPLES_PER_FRAME * 4)
            before += c
        self.resample(ptrs, counts, streams, chain, end, stream)

    def resample_live(self, mp2live, chain=True, end=False, stream=None):
        """the frames of an Mp2Live's last tick from their device_pcm pointers (they lie stream after stream, a stream's frames
        contiguous).  chain=True: the live stream id IS the stream number (an id at or above max_streams is refused);
        otherwise the streams are numbered 0, 1, .. in the order of their ids.  Returns the tick's frames in that order."""
        frames = sorted(mp2live.frames(), key=lambda f: f["stream"])
        ids = sorted({f["stream"] for f in frames})
        for f in frames:
            if f["sample_rate"] != self.in_rate:
                raise ValueError("resample_live: stream %d is sampled at %d Hz, the resampler takes %d" % (f["stream"], f["sample_rate"], self.in_rate))
        if chain and ids and ids[-1] >= self.max_streams:
            raise ValueError("resample_live: live stream id %d >= max_streams %d" % (ids[-1], self.max_streams))
        ptrs = [next(f["device_pcm"] for f in frames if f["stream"] == i) for i in ids]
        counts = [sum(1 for f in frames if f["stream"] == i) for i in ids]
        self.resample(ptrs, counts, ids if chain else None, chain, end, stream)
        return frames

    def sync(self):
        self._ok(self.L.jsmpeg_hip_resampler_sync(self.h))

    def query(self):
        """True once the pass in flight has finished on the device; never waits"""
        return bool(self._ok(self.L.jsmpeg_hip_resampler_query(self.h)))

    def stream_out(self, stream):
        """(offset, count) of stream NUMBER `stream` in the last call's buffer: waveform -- the element index of its first row
        and its samples per channel; frames -- its first frame and its whole frames.  Answered without waiting."""
        o, c = ctypes.c_uint64(), ctypes.c_uint64()
        self._ok(self.L.jsmpeg_hip_resampler_stream_out(self.h, stream, ctypes.byref(o), ctypes.byref(c)))
        return int(o.value), int(c.value)

    def counts(self):
        """samples per channel (waveform) or whole frames (frames) of every stream of the last call, in call order"""
        return [self.stream_out(s)[1] for s in self._numbers]

    def device_out(self):
        """(device address, bytes) of the last call's buffer: closed form, nothing is waited for -- the contents are there for
        work enqueued behind the call on its HIP stream, or after sync()"""
        total = ctypes.c_uint64()
        p = self.L.jsmpeg_hip_resampler_out(self.h, ctypes.byref(total))
        if not p:
            raise RuntimeError(_batch.last_error())
        return p, int(total.value)

    def waveform(self):
        """the last call's padded batch as a torch tensor [streams of the call][channels][row] OVER the device buffer: no copy,
        valid until the handle's next call.  Settles the pass, so the tensor is safe on any torch stream."""
        import torch
        if self.form != "waveform":
            raise ValueError("waveform(): the handle was made with form='frames'")
        self.sync()
        p, total = self.device_out()
        n = len(self._numbers)
        dt = {"float32": torch.float32, "float16": torch.float16, "bfloat16": torch.bfloat16}[self.dtype]
        if not n:
            return torch.empty((0, self.channels, self.row), dtype=dt, device="cuda")
        size = 4 if self.dtype == "float32" else 2
        typestr = "<f4" if self.dtype == "float32" else ("<f2" if self.dtype == "float16" else "<i2")

        class _Span:
            __cuda_array_interface__ = {"shape": (n, self.channels, self.row), "typestr": typestr, "data": (p, False), "version": 2}
        assert total == n * self.channels * self.row * size
        t = torch.as_tensor(_Span(), device="cuda")
        return t.view(torch.bfloat16) if self.dtype == "bfloat16" else t

    def read(self):
        """the last call's buffer on the host: waveform -- [streams][channels][row] (bfloat16 as its uint16 bits); frames --
        float32 [frames][2][1152], the streams' whole frames one after the other"""
        self.sync()
        p, total = self.device_out()
        if self.form == "frames":
            out = np.zeros((total // (2 * SAMPLES_PER_FRAME * 4), 2, SAMPLES_PER_FRAME), np.float32)
        else:
            out = np.zeros((len(self._numbers), self.channels, self.row), {"float32": np.float32, "float16": np.float16, "bfloat16": np.uint16}[self.dtype])
        if total:
            self._ok(self.L.jsmpeg_hip_device_read(out.ctypes.data, p, total))
        return out

    def frames(self):
        """(ptrs, counts, stream numbers) of the last call's whole frames, ready for Mp2Encoder.encode(ptrs, counts, numbers,
        chain=True, stream=...) on the same HIP stream: closed form, nothing is waited for"""
        if self.form != "frames":
            raise ValueError("frames(): the handle was made with form='waveform'")
        base = self.device_out()[0]
        outs = [self.stream_out(s) for s in self._numbers]
        return [base + o * 2 * SAMPLES_PER_FRAME * 4 if c else 0 for o, c in outs], [c for _, c in outs], list(self._numbers)

    def chain_reset(self, stream=None):
        """ends the chain of `stream` (None: of every stream): its next chained call starts from zeros"""
        self._ok(self.L.jsmpeg_hip_resampler_chain_reset(self.h, 0xffffffff if stream is None else stream))

    def chain_info(self, stream):
        """(whether `stream` has chain state, input samples per channel it has taken, outputs it has made)"""
        out = (ctypes.c_uint64 * 3)()
        self._ok(self.L.jsmpeg_hip_resampler_chain_info(self.h, stream, out))
        return bool(out[0]), int(out[1]), int(out[2])

    def timings(self):
        ms = (ctypes.c_float * 2)()
        self._ok(self.L.jsmpeg_hip_resampler_timings(self.h, ms))
        return dict(kernel_ms=float(ms[0]), total_ms=float(ms[1]))
