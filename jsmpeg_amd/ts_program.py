"""The TS program mux: the Python side of C ABI part 10 (include/jsmpeg_hip.h, jsmpeg_hip_ts_program_*).  Video units over one
device buffer and audio units over another -> ONE transport stream per stream number, merged by PTS, with PAT / PMT in front
of entry points and a PCR on the carrier's PES on request -- in one enqueue, read back in one copy.  TsProgram.mux takes host
tables, TsProgram.mux_encoders the last calls of an Encoder and an Mp2Encoder (which may still be in flight on the same
stream).  program_mux_host writes the same bytes without a device.  The rule: jsmpeg_amd/csrc/ts_prog.h."""
import ctypes

import numpy as np

from . import _pass
from . import batch as _batch
from ._pass import c_int, i64, p_f32, p_u32, p_u64, u32, u64, vp

PSI = 1
PCR = 2
NO_PID = 0x1fff
VIDEO, AUDIO = 0, 1
ALL = 0xffffffff

class TsProgramConfig(ctypes.Structure):
    _fields_ = [("max_streams", ctypes.c_uint32), ("max_video_units", ctypes.c_uint32), ("max_audio_units", ctypes.c_uint32),
                ("max_ts_bytes", ctypes.c_uint64), ("video_pid", ctypes.c_uint32), ("audio_pid", ctypes.c_uint32), ("pmt_pid", ctypes.c_uint32),
                ("video_stream_id", ctypes.c_uint32), ("audio_stream_id", ctypes.c_uint32), ("program_number", ctypes.c_uint32),
                ("transport_stream_id", ctypes.c_uint32), ("flags", ctypes.c_uint32), ("pcr_lead_90k", ctypes.c_uint64), ("device", ctypes.c_int32)]


def config(max_streams=1, max_video_units=1, max_audio_units=1, max_ts_bytes=188, video_pid=0x100, audio_pid=0x101, pmt_pid=0x1000,
           video_stream_id=0xE0, audio_stream_id=0xC0, program_number=1, transport_stream_id=1, psi=True, pcr=True, pcr_lead_90k=0, device=-1):
    """a TsProgramConfig; video_pid / audio_pid NO_PID: that kind is absent"""
    return TsProgramConfig(max_streams, max_video_units, max_audio_units, max_ts_bytes, video_pid, audio_pid, pmt_pid, video_stream_id,
                           audio_stream_id, program_number, transport_stream_id, (PSI if psi else 0) | (PCR if pcr else 0), pcr_lead_90k, device)


_cfg = ctypes.POINTER(TsProgramConfig)
SIGNATURES = {
    "jsmpeg_hip_ts_program_create": (vp, [_cfg]),
    "jsmpeg_hip_ts_program_destroy": (None, [vp]),
    "jsmpeg_hip_ts_program_set_output": (c_int, [vp, vp, u64]),
    "jsmpeg_hip_ts_program_mux": (c_int, [vp, vp, vp, vp, vp, vp, u32, vp, vp, vp, vp, vp, u32, vp]),
    "jsmpeg_hip_ts_program_mux_encoders": (c_int, [vp, vp, vp, vp, vp, vp]),
    "jsmpeg_hip_ts_program_sync": (c_int, [vp]),
    "jsmpeg_hip_ts_program_query": (c_int, [vp]),
    "jsmpeg_hip_ts_program_ts": (vp, [vp, p_u64]),
    "jsmpeg_hip_ts_program_stream_range": (c_int, [vp, u32, p_u64, p_u64]),
    "jsmpeg_hip_ts_program_unit_range": (c_int, [vp, u32, u32, p_u64, p_u32, p_u32]),
    "jsmpeg_hip_ts_program_read": (i64, [vp, u32, vp, u64]),
    "jsmpeg_hip_ts_program_state": (c_int, [vp, u32, p_u32]),
    "jsmpeg_hip_ts_program_reset": (c_int, [vp, u32]),
    "jsmpeg_hip_ts_program_timings": (c_int, [vp, p_f32]),
    "jsmpeg_hip_ts_program_mux_host": (i64, [_cfg, vp, vp, vp, vp, vp, u32, vp, vp, vp, vp, vp, u32, vp, vp, u64, vp, vp]),
    "jsmpeg_hip_ts_program_bound": (u64, [u64, u32, u64, u32, u32]),
    "jsmpeg_hip_ts_program_psi": (c_int, [_cfg, vp]),
    "jsmpeg_hip_ts_program_set_state": (c_int, [vp, u32, p_u32]),
}
SYMBOLS = tuple(SIGNATURES)

_bound = None


def lib():
    """libjsmpeg_hip with the part-10 argtypes set"""
    global _bound
    if _bound is None:
        _bound = _pass.bind(_pass.lib(), SIGNATURES)
    return _bound


def program_bound(v_bytes, n_v, a_bytes, n_a, streams=1):
    """a safe max_ts_bytes for v_bytes of payload in n_v video units and a_bytes in n_a audio units over `streams` streams"""
    return int(lib().jsmpeg_hip_ts_program_bound(int(v_bytes), int(n_v), int(a_bytes), int(n_a), int(streams)))


def psi_packets(cfg):
    """(the PAT packet, the PMT packet) of a config, 188 bytes each, continuity 0"""
    out = np.zeros(376, np.uint8)
    if lib().jsmpeg_hip_ts_program_psi(ctypes.byref(cfg), out.ctypes.data) < 0:
        raise RuntimeError(_batch.last_error())
    return out[:188].tobytes(), out[188:].tobytes()


class _Table:
    """one kind's host table as the C ABI takes it: ranges = [(offset, bytes)], pts = 90 kHz integers, streams = a number per unit"""

    def __init__(self, ranges, pts, streams, what):
        n = len(ranges)
        if len(pts) != n or (streams is not None and len(streams) != n):
            raise ValueError("%s: one pts and one stream number per range" % what)
        self.n = n
        self.off = np.ascontiguousarray([r[0] for r in ranges], dtype=np.uint64)
        self.len = np.ascontiguousarray([r[1] for r in ranges], dtype=np.uint32)
        self.pts = np.ascontiguousarray([int(p) for p in pts], dtype=np.uint64)
        self.st = np.zeros(n, np.uint32) if streams is None else np.ascontiguousarray(streams, dtype=np.uint32)

    def args(self, base):
        return [base, self.off.ctypes.data, self.len.ctypes.data, self.st.ctypes.data, self.pts.ctypes.data, self.n]


def _host_bytes(x):
    return np.ascontiguousarray(np.frombuffer(x, dtype=np.uint8) if isinstance(x, (bytes, bytearray)) else x, dtype=np.uint8)


def program_mux_host(cfg, video=None, v_ranges=(), v_pts=(), v_streams=None, audio=None, a_ranges=(), a_pts=(), a_streams=None, state=None, cap=None):
    """jsmpeg_hip_ts_program_mux_host: the program mux without a device.  video / audio: host bytes; the tables as
    TsProgram.mux takes them; state: [max_streams][5] (None: zeros); cap: the capacity (None: what the call needs).
    Returns (the buffer as a uint8 array, {stream: (begin, end)}, the state behind the call as [[5 words]])."""
    L = lib()
    v, a = _Table(v_ranges, v_pts, v_streams, "video"), _Table(a_ranges, a_pts, a_streams, "audio")
    vb = _host_bytes(video) if video is not None else np.zeros(1, np.uint8)
    ab = _host_bytes(audio) if audio is not None else np.zeros(1, np.uint8)
    for t, b, what in ((v, vb, "video"), (a, ab, "audio")):
        if t.n and int((t.off + t.len).max()) > b.size:
            raise ValueError("program_mux_host: a %s range ends behind the bytes" % what)
    ns = cfg.max_streams
    st = np.zeros((ns, 5), np.uint32)
    if state is not None:
        st[:] = np.asarray(state, dtype=np.uint32).reshape(ns, 5)
    sb, se = np.zeros(ns, np.uint64), np.zeros(ns, np.uint64)
    args = [ctypes.byref(cfg)] + v.args(vb.ctypes.data) + a.args(ab.ctypes.data)
    need = L.jsmpeg_hip_ts_program_mux_host(*(args + [st.ctypes.data, None, 0, None, None]))
    if need < 0:
        raise RuntimeError(_batch.last_error())
    cap = need if cap is None else cap
    out = np.full(max(1, cap), 0xA5, np.uint8)
    got = L.jsmpeg_hip_ts_program_mux_host(*(args + [st.ctypes.data, out.ctypes.data, cap, sb.ctypes.data, se.ctypes.data]))
    if got < 0:
        raise RuntimeError(_batch.last_error())
    present = sorted(set(int(s) for s in v.st) | set(int(s) for s in a.st))
    return out[:got], {s: (int(sb[s]), int(se[s])) for s in present}, [[int(w) for w in row] for row in st]


class TsProgram(_pass.Pass):
    """One program per stream number out of two unit tables, on the device.  A call is a pure enqueue; sync() or any reader
    settles it.  The continuity counters of PAT, PMT, video and audio and the `started` word of every stream number live on
    the device and go on from call to call: the pieces of a stream, concatenated in call order, are one valid stream."""
    PREFIX = "jsmpeg_hip_ts_program_"
    TIMINGS = ("mux_ms", "total_ms")

    def __init__(self, cfg):
        self.cfg = cfg
        self._open(lib(), SIGNATURES, cfg)
        self.n_v = self.n_a = 0

    def set_output(self, dev_ts, cap):
        """the calls write into the caller's device buffer (4-byte aligned, cap bytes); None: the handle's own again"""
        self._call("set_output", dev_ts, int(cap))

    def mux(self, dev_video=None, v_ranges=(), v_pts=(), v_streams=None, dev_audio=None, a_ranges=(), a_pts=(), a_streams=None, stream=None):
        """dev_video / dev_audio: device addresses; v_ranges / a_ranges = [(offset, bytes)], one PES per range; v_pts / a_pts:
        90 kHz integers, unwrapped, non-decreasing within a stream; v_streams / a_streams: ascending stream numbers (None: all
        0); stream: the HIP stream to enqueue on -- the one the bytes were produced on"""
        v, a = _Table(v_ranges, v_pts, v_streams, "video"), _Table(a_ranges, a_pts, a_streams, "audio")
        self._call("mux", *(v.args(dev_video) + a.args(dev_audio) + [stream]))
        self.n_v, self.n_a = v.n, a.n

    def mux_encoders(self, encoder=None, mp2_encoder=None, v_pts=None, a_pts=None, stream=None):
        """the relay form: the video units are the pictures of encoder's last call, the audio units the frames of mp2_encoder's
        -- both may still be in flight on `stream`; v_pts / a_pts: 90 kHz integers per picture / frame (None: the default of
        the chain ordinal).  Either encoder may be None."""
        vp = None if v_pts is None else np.ascontiguousarray([int(p) for p in v_pts], dtype=np.uint64)
        ap = None if a_pts is None else np.ascontiguousarray([int(p) for p in a_pts], dtype=np.uint64)
        n_v, n_a = (encoder.count if encoder is not None else 0), (mp2_encoder.count if mp2_encoder is not None else 0)
        if (vp is not None and vp.shape != (n_v,)) or (ap is not None and ap.shape != (n_a,)):
            raise ValueError("mux_encoders: one pts per picture / frame of the encoders' last calls")
        self._call("mux_encoders", encoder.h if encoder is not None else None, None if vp is None else vp.ctypes.data,
                   mp2_encoder.h if mp2_encoder is not None else None, None if ap is None else ap.ctypes.data, stream)
        self.n_v, self.n_a = n_v, n_a

    def device_ts(self):
        """(device address, total bytes) of the last call's buffer"""
        return self._buffer("ts")

    def stream_range(self, stream):
        return self._pair("stream_range", stream)

    def _read(self, stream):
        n = self._call("read", stream, None, 0)
        out = np.empty(max(1, n), dtype=np.uint8)
        self._call("read", stream, out.ctypes.data, n)
        return out[:n]

    def ts(self, stream=0):
        """the stream's program, copied to the host"""
        return self._read(stream).tobytes()

    def ts_all(self, streams=None):
        """every stream's program in ONE copy: {stream: bytes} for `streams` (None: every stream number that has packets)"""
        buf = self._read(ALL)
        out = {}
        for s in (range(self.cfg.max_streams) if streams is None else streams):
            b, e = self.stream_range(s)
            if e > b or streams is not None:
                out[s] = buf[b:e].tobytes()
        return out

    def unit_ranges(self, kind):
        """[(offset, bytes, psi_bytes)] per unit of `kind` (VIDEO / AUDIO) of the last call: offset at the PAT if PSI lies in front"""
        out = []
        for k in range(self.n_a if kind else self.n_v):
            o, b, p = ctypes.c_uint64(), ctypes.c_uint32(), ctypes.c_uint32()
            self._call("unit_range", kind, k, ctypes.byref(o), ctypes.byref(b), ctypes.byref(p))
            out.append((int(o.value), int(b.value), int(p.value)))
        return out

    def state(self, stream):
        """[PAT, PMT, video, audio counters, started] of a stream number behind the last call"""
        out = (ctypes.c_uint32 * 5)()
        self._call("state", stream, out)
        return [int(v) for v in out]

    def set_state(self, stream, words):
        """sets the five words of a stream number: a relay that restarts goes on where its streams were"""
        self._call("set_state", stream, (ctypes.c_uint32 * 5)(*[int(w) for w in words]))

    def reset(self, stream=None):
        """zeroes the five words of `stream` (None: of every stream): its next unit gets PSI in front again"""
        self._call("reset", ALL if stream is None else stream)
