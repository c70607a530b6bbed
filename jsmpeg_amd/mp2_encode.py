"""The MP2 (MPEG-1 Audio Layer II) encoder on the device: the Python side of C ABI part 9 (include/jsmpeg_hip.h,
jsmpeg_hip_mp2_encoder_*).  PCM in HBM -- float32 [frame][2][1152], as Mp2Batch and Mp2Live leave it, or a torch tensor --
-> constant-bit-rate Layer II frames in a device buffer that Mp2Batch.upload_device and encode.ts_mux_device take as it is.
The rule: jsmpeg_amd/csrc/mp2_enc.h.  A call is a pure enqueue; sync() or a reader of device results settles it.  torch is
imported only when a tensor is handed in."""
import ctypes

import numpy as np

from . import _pass
from ._pass import c_int, i64, p_f32, p_u32, p_u64, u32, u64, vp

END = 1
CHAIN = 2        # continue the call's streams where their last chained call left them (JSMPEG_HIP_MP2_ENC_CHAIN)

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


SIGNATURES = {
    "jsmpeg_hip_mp2_encoder_create": (vp, [ctypes.POINTER(Mp2EncoderConfig)]),
    "jsmpeg_hip_mp2_encoder_destroy": (None, [vp]),
    "jsmpeg_hip_mp2_encoder_encode": (c_int, [vp, vp, vp, vp, u32, u32, vp]),
    "jsmpeg_hip_mp2_encoder_sync": (c_int, [vp]),
    "jsmpeg_hip_mp2_encoder_query": (c_int, [vp]),
    "jsmpeg_hip_mp2_encoder_es": (vp, [vp, p_u64]),
    "jsmpeg_hip_mp2_encoder_stream_range": (c_int, [vp, u32, p_u64, p_u64]),
    "jsmpeg_hip_mp2_encoder_frame_range": (c_int, [vp, u32, p_u64, p_u32]),
    "jsmpeg_hip_mp2_encoder_read_es": (i64, [vp, u32, vp, u64]),
    "jsmpeg_hip_mp2_encoder_frame_stats": (c_int, [vp, u32, p_u32]),
    "jsmpeg_hip_mp2_encoder_chain_reset": (c_int, [vp, u32]),
    "jsmpeg_hip_mp2_encoder_chain_info": (c_int, [vp, u32, p_u64]),
    "jsmpeg_hip_mp2_encoder_timings": (c_int, [vp, p_f32]),
}
SYMBOLS = tuple(SIGNATURES)

_bound = None


def lib():
    """libjsmpeg_hip with the part-9 argtypes set"""
    global _bound
    if _bound is None:
        _bound = _pass.bind(_pass.lib(), SIGNATURES)
    return _bound


class Mp2Encoder(_pass.Pass):
    """PCM on the device -> Layer II streams on the device.  chain=True on a call continues its streams -- the stream NUMBER
    is a stream's identity from call to call -- where their last chained call left them: ordinal (padding, PTS) and filter
    history go on, and the pieces concatenated are byte for byte the stream one call over all the frames writes."""
    PREFIX = "jsmpeg_hip_mp2_encoder_"

    def __init__(self, sample_rate_index, channels, bitrate_index, max_streams, max_frames, max_es_bytes, device=-1):
        cfg = Mp2EncoderConfig(sample_rate_index, channels, bitrate_index, max_streams, max_frames, max_es_bytes, device)
        self.sample_rate_index, self.channels, self.bitrate_index = sample_rate_index, channels, bitrate_index
        self.max_streams, self.max_frames = max_streams, max_frames
        self._open(lib(), SIGNATURES, cfg)
        self.sample_rate = SAMPLE_RATES[sample_rate_index]
        self.count = 0
        self._streams, self._first = [], []

    def encode(self, ptrs, frames, streams=None, end=False, chain=False, stream=None):
        """ptrs: one device address per stream, of its first frame ([frames][2][1152] float32, contiguous); frames: the count
        per stream (0 allowed); streams: ascending stream numbers (None: 0, 1, ..); chain: continue the streams; end: with
        chain, their chains end behind this call; stream: the HIP stream to enqueue on -- the one the PCM was produced on."""
        arr, fr, st, numbers = _pass.marshal(ptrs, frames, streams, "frames: one count per stream")
        first = [self.chain_info(s)[1] if chain and s < self.max_streams else 0 for s in numbers]
        self._call("encode", arr, fr.ctypes.data, None if st is None else st.ctypes.data, len(ptrs), (END if end else 0) | (CHAIN if chain else 0), stream)
        self.count = int(fr.sum())
        self._streams = [s for s, f in zip(numbers, fr) for _ in range(int(f))]       # per frame of the call: its stream number
        self._first = [n0 + k for n0, f in zip(first, fr) for k in range(int(f))]     # ... and its ordinal in that stream

    def encode_tensor(self, x, streams=None, end=False, chain=False):
        """x: a contiguous float32 CUDA tensor [S, F, 2, 1152] -- S streams of F frames; runs on torch's current stream of the
        tensor's device, right behind whatever produced the tensor there"""
        ptrs, frames, stream = _pass.frames_tensor(x, "encode_tensor")
        self.encode(ptrs, frames, streams, end, chain, stream)
        self._keep = x          # the tensor stays alive until the next call

    def encode_batch(self, mp2batch, streams=None, end=False, chain=False, stream=None):
        """every frame of an Mp2Batch's last decode, straight from its PCM in HBM (the batch's streams in order; streams:
        their stream numbers here).  A batch whose sampling rate is not the encoder's is refused."""
        ptrs, counts = _pass.batch_frames(mp2batch, self.sample_rate, "encode_batch", "the encoder at")
        self.encode(ptrs, counts, streams, end, chain, stream)

    def encode_live(self, mp2live, chain=True, end=False, stream=None):
        """the frames of an Mp2Live's last tick from their device_pcm pointers (they lie stream after stream, a stream's frames
        contiguous).  chain=True: the live stream id IS the stream number (an id at or above max_streams is refused);
        otherwise the streams are numbered 0, 1, .. in the order of their ids.  Returns the tick's frames in encoded order."""
        frames, ptrs, counts, numbers = _pass.live_frames(mp2live, self.sample_rate, self.max_streams, chain, "encode_live", "the encoder at")
        self.encode(ptrs, counts, numbers, end, chain, stream)
        return frames

    def device_es(self):
        """(device address, total bytes) of the last call's buffer: 16-byte aligned stream begins, zeros behind each stream"""
        return self._buffer("es")

    def stream_range(self, stream):
        return self._pair("stream_range", stream)

    def frame_ranges(self):
        """[(offset in the device buffer, bytes)] per frame of the last call; answered without waiting"""
        out = []
        for k in range(self.count):
            o, b = ctypes.c_uint64(), ctypes.c_uint32()
            self._call("frame_range", k, ctypes.byref(o), ctypes.byref(b))
            out.append((int(o.value), int(b.value)))
        return out

    def es(self, stream=0):
        """the stream's bytes, copied to the host"""
        n = self._call("read_es", stream, None, 0)
        out = np.empty(max(1, n), dtype=np.uint8)
        self._call("read_es", stream, out.ctypes.data, n)
        return out[:n].tobytes()

    def frame_stats(self, k):
        out = (ctypes.c_uint32 * 4)()
        self._call("frame_stats", k, out)
        return dict(coded_pairs=int(out[0]), bits_used=int(out[1]), bits_left=int(out[2]), top_code=int(out[3]))

    def chain_reset(self, stream=None):
        """ends the chain of `stream` (None: of every stream): its next chained frame has ordinal 0 and a silent history"""
        self._call("chain_reset", 0xffffffff if stream is None else stream)

    def chain_info(self, stream):
        """(whether `stream` has chain state, the frames it has coded = the ordinal of its next chained frame)"""
        out = (ctypes.c_uint64 * 2)()
        self._ok(self._fn["chain_info"](self.h, stream, out))          # (not _call: asked per stream by every chained encode)
        return bool(out[0]), int(out[1])

    def ts_units(self):
        """(ranges, pts in seconds, stream numbers) of the last call's frames, ready for encode.ts_mux_device(..., stream_id=0xC0,
        pid=0x101): one PES per frame with the default PTS of its ordinal"""
        pts = [default_pts(n, self.sample_rate) / 90000.0 for n in self._first]
        return self.frame_ranges(), pts, list(self._streams)
