"""The MP2 (MPEG-1 Audio Layer II) encoder on the device: the Python side of C ABI part 9 (include/jsmpeg_hip.h,
jsmpeg_hip_mp2_encoder_*).  PCM in HBM -- float32 [frame][2][1152], as Mp2Batch and Mp2Live leave it, or a torch tensor --
-> constant-bit-rate Layer II frames in a device buffer that Mp2Batch.upload_device and encode.ts_mux_device take as it is.
The rule: jsmpeg_amd/csrc/mp2_enc.h.  A call is a pure enqueue; sync() or a reader of device results settles it.  torch is
imported only when a tensor is handed in."""
import ctypes

import numpy as np

from . import batch as _batch

END = 1
CHAIN = 2        # continue the call's streams where their last chained call left them (JSMPEG_HIP_MP2_ENC_CHAIN)

SYMBOLS = ("jsmpeg_hip_mp2_encoder_create", "jsmpeg_hip_mp2_encoder_destroy", "jsmpeg_hip_mp2_encoder_encode", "jsmpeg_hip_mp2_encoder_sync",
           "jsmpeg_hip_mp2_encoder_query", "jsmpeg_hip_mp2_encoder_es", "jsmpeg_hip_mp2_encoder_stream_range", "jsmpeg_hip_mp2_encoder_frame_range",
           "jsmpeg_hip_mp2_encoder_read_es", "jsmpeg_hip_mp2_encoder_frame_stats", "jsmpeg_hip_mp2_encoder_chain_reset",
           "jsmpeg_hip_mp2_encoder_chain_info", "jsmpeg_hip_mp2_encoder_timings")

SAMPLE_RATES = (44100, 48000, 32000)
KBPS = (32, 48, 56, 64, 80, 96, 112, 128, 160, 192, 224, 256, 320, 384)
SAMPLES_PER_FRAME = 1152


def frame_offset(n, sample_rate_index, bitrate_index):
    """where frame n (the stream's ordinal) begins, in bytes behind ordinal 0: n b + floor(n r / fs)"""
    N, fs = 144000 * KBPS[bitrate_index - 1], SAMPLE_RATES[sample_rate_index]
    return n * (N // fs) + n * (N % fs) // fs


def frame_bytes(n, sample_rate_index, bitrate_index):
    """bytes of frame n: b + pad(n)"""
    return frame_offset(n + 1, sample_rate_index, bitrate_index) - frame_offset(n, sample_rate_index, bitrate_index)


def default_pts(n, rate):
    """the default PTS of frame n in 90 kHz ticks: floor(n 1152 90000 / fs)"""
    return n * SAMPLES_PER_FRAME * 90000 // rate


def es_bytes(frames, sample_rate_index, bitrate_index, first=None):
    """the bytes a call needs (a safe max_es_bytes): frames per stream, first = each stream's first ordinal (None: 0)"""
    total = 0
    for i, f in enumerate(frames):
        n0 = 0 if first is None else first[i]
        total += frame_offset(n0 + f, sample_rate_index, bitrate_index) - frame_offset(n0, sample_rate_index, bitrate_index)
        total = (total + 15) & ~15
    return total


class Mp2EncoderConfig(ctypes.Structure):
    _fields_ = [("sample_rate_index", ctypes.c_uint32), ("channels", ctypes.c_uint32), ("bitrate_index", ctypes.c_uint32),
                ("max_streams", ctypes.c_uint32), ("max_frames", ctypes.c_uint32), ("max_es_bytes", ctypes.c_uint64), ("device", ctypes.c_int32)]


_bound = None


def lib():
    """libjsmpeg_hip with the part-9 argtypes set"""
    global _bound
    if _bound is None:
        L = _batch.lib()
        vp, u32, u64 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64
        L.jsmpeg_hip_mp2_encoder_create.restype = vp
        L.jsmpeg_hip_mp2_encoder_create.argtypes = [ctypes.POINTER(Mp2EncoderConfig)]
        L.jsmpeg_hip_mp2_encoder_destroy.restype = None
        L.jsmpeg_hip_mp2_encoder_destroy.argtypes = [vp]
        L.jsmpeg_hip_mp2_encoder_encode.restype = ctypes.c_int
        L.jsmpeg_hip_mp2_encoder_encode.argtypes = [vp, vp, vp, vp, u32, u32, vp]
        for name in ("jsmpeg_hip_mp2_encoder_sync", "jsmpeg_hip_mp2_encoder_query"):
            getattr(L, name).restype = ctypes.c_int
            getattr(L, name).argtypes = [vp]
        L.jsmpeg_hip_mp2_encoder_es.restype = vp
        L.jsmpeg_hip_mp2_encoder_es.argtypes = [vp, ctypes.POINTER(u64)]
        L.jsmpeg_hip_mp2_encoder_stream_range.restype = ctypes.c_int
        L.jsmpeg_hip_mp2_encoder_stream_range.argtypes = [vp, u32, ctypes.POINTER(u64), ctypes.POINTER(u64)]
        L.jsmpeg_hip_mp2_encoder_frame_range.restype = ctypes.c_int
        L.jsmpeg_hip_mp2_encoder_frame_range.argtypes = [vp, u32, ctypes.POINTER(u64), ctypes.POINTER(u32)]
        L.jsmpeg_hip_mp2_encoder_read_es.restype = ctypes.c_int64
        L.jsmpeg_hip_mp2_encoder_read_es.argtypes = [vp, u32, vp, u64]
        L.jsmpeg_hip_mp2_encoder_frame_stats.restype = ctypes.c_int
        L.jsmpeg_hip_mp2_encoder_frame_stats.argtypes = [vp, u32, ctypes.POINTER(u32)]
        L.jsmpeg_hip_mp2_encoder_chain_reset.restype = ctypes.c_int
        L.jsmpeg_hip_mp2_encoder_chain_reset.argtypes = [vp, u32]
        L.jsmpeg_hip_mp2_encoder_chain_info.restype = ctypes.c_int
        L.jsmpeg_hip_mp2_encoder_chain_info.argtypes = [vp, u32, ctypes.POINTER(u64)]
        L.jsmpeg_hip_mp2_encoder_timings.restype = ctypes.c_int
        L.jsmpeg_hip_mp2_encoder_timings.argtypes = [vp, ctypes.POINTER(ctypes.c_float)]
        _bound = L
    return _bound


class Mp2Encoder:
    """PCM on the device -> Layer II streams on the device.  chain=True on a call continues its streams -- the stream NUMBER
    is a stream's identity from call to call -- where their last chained call left them: ordinal (padding, PTS) and filter
    history go on, and the pieces concatenated are byte for byte the stream one call over all the frames writes."""

    def __init__(self, sample_rate_index, channels, bitrate_index, max_streams, max_frames, max_es_bytes, device=-1):
        self.L = lib()
        cfg = Mp2EncoderConfig(sample_rate_index, channels, bitrate_index, max_streams, max_frames, max_es_bytes, device)
        self.sample_rate_index, self.channels, self.bitrate_index = sample_rate_index, channels, bitrate_index
        self.max_streams, self.max_frames = max_streams, max_frames
        self.h = self.L.jsmpeg_hip_mp2_encoder_create(ctypes.byref(cfg))
        if not self.h:
            raise RuntimeError("jsmpeg_hip_mp2_encoder_create: " + _batch.last_error())
        self.sample_rate = SAMPLE_RATES[sample_rate_index]
        self.count = 0
        self._streams, self._first = [], []

    def _ok(self, rc):
        if rc < 0:
            raise RuntimeError(_batch.last_error())
        return rc

    def close(self):
        if self.h:
            self.L.jsmpeg_hip_mp2_encoder_destroy(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def encode(self, ptrs, frames, streams=None, end=False, chain=False, stream=None):
        """ptrs: one device address per stream, of its first frame ([frames][2][1152] float32, contiguous); frames: the count
        per stream (0 allowed); streams: ascending stream numbers (None: 0, 1, ..); chain: continue the streams; end: with
        chain, their chains end behind this call; stream: the HIP stream to enqueue on -- the one the PCM was produced on."""
        n = len(ptrs)
        fr = np.ascontiguousarray(frames, dtype=np.uint32)
        if fr.shape != (n,):
            raise ValueError("frames: one count per stream")
        st = None if streams is None else np.ascontiguousarray(streams, dtype=np.uint32)
        if st is not None and st.shape != (n,):
            raise ValueError("streams: one stream number per stream")
        numbers = list(range(n)) if st is None else [int(v) for v in st]
        first = [self.chain_info(s)[1] if chain and s < self.max_streams else 0 for s in numbers]
        arr = (ctypes.c_void_p * max(1, n))(*[int(p) if p else None for p in ptrs])
        self._ok(self.L.jsmpeg_hip_mp2_encoder_encode(self.h, arr, fr.ctypes.data, None if st is None else st.ctypes.data, n,
                                                      (END if end else 0) | (CHAIN if chain else 0), stream))
        self.count = int(fr.sum())
        self._streams = [s for s, f in zip(numbers, fr) for _ in range(int(f))]       # per frame of the call: its stream number
        self._first = [n0 + k for n0, f in zip(first, fr) for k in range(int(f))]     # ... and its ordinal in that stream

    def encode_tensor(self, x, streams=None, end=False, chain=False):
        """x: a contiguous float32 CUDA tensor [S, F, 2, 1152] -- S streams of F frames; runs on torch's current stream of the
        tensor's device, right behind whatever produced the tensor there"""
        import torch
        if not isinstance(x, torch.Tensor) or x.dtype != torch.float32 or not x.is_cuda or x.dim() != 4 or not x.is_contiguous() or \
                tuple(x.shape[2:]) != (2, SAMPLES_PER_FRAME):
            raise ValueError("encode_tensor: a contiguous float32 CUDA tensor [S, F, 2, 1152] is needed")
        s, f = int(x.shape[0]), int(x.shape[1])
        step = f * 2 * SAMPLES_PER_FRAME * 4
        self.encode([x.data_ptr() + i * step if f else 0 for i in range(s)], [f] * s, streams, end, chain,
                    torch.cuda.current_stream(x.device).cuda_stream)
        self._keep = x          # the tensor stays alive until the next call

    def encode_batch(self, mp2batch, streams=None, end=False, chain=False, stream=None):
        """every frame of an Mp2Batch's last decode, straight from its PCM in HBM (the batch's streams in order; streams:
        their stream numbers here).  A batch whose sampling rate is not the encoder's is refused."""
        n = mp2batch.n_streams
        counts = [mp2batch.frame_count(s) for s in range(n)]
        for s in range(n):
            if counts[s] and mp2batch.frame_info(s, 0)[2] != self.sample_rate:
                raise ValueError("encode_batch: stream %d is sampled at %d Hz, the encoder at %d" % (s, mp2batch.frame_info(s, 0)[2], self.sample_rate))
        base, before = mp2batch.pcm_device_pointer(), 0
        ptrs = []
        for c in counts:
            ptrs.append(base + before * 2 * SAMPLES_PER_FRAME * 4)
            before += c
        self.encode(ptrs, counts, streams, end, chain, stream)

    def encode_live(self, mp2live, chain=True, end=False, stream=None):
        """the frames of an Mp2Live's last tick from their device_pcm pointers (they lie stream after stream, a stream's frames
        contiguous).  chain=True: the live stream id IS the stream number (an id at or above max_streams is refused);
        otherwise the streams are numbered 0, 1, .. in the order of their ids.  Returns the tick's frames in encoded order."""
        frames = sorted(mp2live.frames(), key=lambda f: f["stream"])
        ids = sorted({f["stream"] for f in frames})
        for f in frames:
            if f["sample_rate"] != self.sample_rate:
                raise ValueError("encode_live: stream %d is sampled at %d Hz, the encoder at %d" % (f["stream"], f["sample_rate"], self.sample_rate))
        if chain and ids and ids[-1] >= self.max_streams:
            raise ValueError("encode_live: live stream id %d >= max_streams %d" % (ids[-1], self.max_streams))
        ptrs = [next(f["device_pcm"] for f in frames if f["stream"] == i) for i in ids]
        counts = [sum(1 for f in frames if f["stream"] == i) for i in ids]
        self.encode(ptrs, counts, ids if chain else None, end, chain, stream)
        return frames

    def sync(self):
        self._ok(self.L.jsmpeg_hip_mp2_encoder_sync(self.h))

    def query(self):
        """True once the pass in flight has finished on the device; never waits"""
        return bool(self._ok(self.L.jsmpeg_hip_mp2_encoder_query(self.h)))

    def device_es(self):
        """(device address, total bytes) of the last call's buffer: 16-byte aligned stream begins, zeros behind each stream"""
        total = ctypes.c_uint64()
        p = self.L.jsmpeg_hip_mp2_encoder_es(self.h, ctypes.byref(total))
        if not p:
            raise RuntimeError(_batch.last_error())
        return p, int(total.value)

    def stream_range(self, stream):
        b, e = ctypes.c_uint64(), ctypes.c_uint64()
        self._ok(self.L.jsmpeg_hip_mp2_encoder_stream_range(self.h, stream, ctypes.byref(b), ctypes.byref(e)))
        return int(b.value), int(e.value)

    def frame_ranges(self):
        """[(offset in the device buffer, bytes)] per frame of the last call; answered without waiting"""
        out = []
        for k in range(self.count):
            o, b = ctypes.c_uint64(), ctypes.c_uint32()
            self._ok(self.L.jsmpeg_hip_mp2_encoder_frame_range(self.h, k, ctypes.byref(o), ctypes.byref(b)))
            out.append((int(o.value), int(b.value)))
        return out

    def es(self, stream=0):
        """the stream's bytes, copied to the host"""
        n = self._ok(self.L.jsmpeg_hip_mp2_encoder_read_es(self.h, stream, None, 0))
        out = np.empty(max(1, n), dtype=np.uint8)
        self._ok(self.L.jsmpeg_hip_mp2_encoder_read_es(self.h, stream, out.ctypes.data, n))
        return out[:n].tobytes()

    def frame_stats(self, k):
        out = (ctypes.c_uint32 * 4)()
        self._ok(self.L.jsmpeg_hip_mp2_encoder_frame_stats(self.h, k, out))
        return dict(coded_pairs=int(out[0]), bits_used=int(out[1]), bits_left=int(out[2]), top_code=int(out[3]))

    def chain_reset(self, stream=None):
        """ends the chain of `stream` (None: of every stream): its next chained frame has ordinal 0 and a silent history"""
        self._ok(self.L.jsmpeg_hip_mp2_encoder_chain_reset(self.h, 0xffffffff if stream is None else stream))

    def chain_info(self, stream):
        """(whether `stream` has chain state, the frames it has coded = the ordinal of its next chained frame)"""
        out = (ctypes.c_uint64 * 2)()
        self._ok(self.L.jsmpeg_hip_mp2_encoder_chain_info(self.h, stream, out))
        return bool(out[0]), int(out[1])

    def timings(self):
        ms = (ctypes.c_float * 2)()
        self._ok(self.L.jsmpeg_hip_mp2_encoder_timings(self.h, ms))
        return dict(kernel_ms=float(ms[0]), total_ms=float(ms[1]))

    def ts_units(self):
        """(ranges, pts in seconds, stream numbers) of the last call's frames, ready for encode.ts_mux_device(..., stream_id=0xC0,
        pid=0x101): one PES per frame with the default PTS of its ordinal"""
        pts = [default_pts(n, self.sample_rate) / 90000.0 for n in self._first]
        return self.frame_ranges(), pts, list(self._streams)
