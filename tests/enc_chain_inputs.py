"""TEST INFRASTRUCTURE ONLY -- what the tests of the encoder's chains across calls (JSMPEG_HIP_ENC_CHAIN) share, beside
tests/enc_p_inputs.py and tests/enc_rate_inputs.py: the CPU simulator of a handle that is called again and again
(sim_chain_* of tests/sim/sim_encode_pass.cpp, built on demand), the ways of cutting n pictures into calls, and the ledger that gathers what
the calls leave per stream, segment by segment, to be held against ONE unchained call over the segment's pictures."""
import ctypes

import numpy as np

import enc_inputs as ei
import enc_p_inputs as ep
import enc_rate_inputs as er
import enc_ref

ROOT = ei.ROOT
SIM_DIR, SIM_SRC, CXXFLAGS = ei.SIM_DIR, ei.PASS_SRC, ei.CXXFLAGS      # what the stand-alone sanitizer build of the tests uses
ALL = 0xffffffff
_sim = None


def sim_deps():
    return ei.sim_deps(SIM_SRC)


def sim():
    global _sim
    if _sim is None:
        lib = ei.pass_sim()
        vp, u32, u64 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64
        lib.sim_chain_create.restype = vp
        lib.sim_chain_create.argtypes = [u32, u32, u32, u32]
        lib.sim_chain_destroy.restype = None
        lib.sim_chain_destroy.argtypes = [vp]
        lib.sim_chain_set_gop.restype = None
        lib.sim_chain_set_gop.argtypes = [vp, u32, u32]
        lib.sim_chain_set_rate.restype = None
        lib.sim_chain_set_rate.argtypes = [vp, u32, u32, u32, u32]
        lib.sim_chain_reset.restype = ctypes.c_int
        lib.sim_chain_reset.argtypes = [vp, u32]
        lib.sim_chain_info.restype = ctypes.c_int
        lib.sim_chain_info.argtypes = [vp, u32, vp]
        lib.sim_chain_record.restype = None
        lib.sim_chain_record.argtypes = [vp, u32, vp]
        lib.sim_chain_set_record.restype = None
        lib.sim_chain_set_record.argtypes = [vp, u32, vp]
        lib.sim_chain_next.restype = u32
        lib.sim_chain_next.argtypes = [u32, u32]
        lib.sim_chain_encode.restype = ctypes.c_int64
        lib.sim_chain_encode.argtypes = [vp, vp, u32, vp, vp, u32, vp, u64, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
        _sim = lib
    return _sim


class Chain:
    """the simulator's handle: Encoder's calls that matter here, with the same names"""

    def __init__(self, width, height, max_streams=1, frame_rate_code=5):
        self.L = sim()
        self.width, self.height, self.max_streams = width, height, max_streams
        self.h = self.L.sim_chain_create(width, height, frame_rate_code, max_streams)
        self.rate = False

    def close(self):
        if self.h:
            self.L.sim_chain_destroy(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def set_gop(self, gop, search=7):
        self.L.sim_chain_set_gop(self.h, gop, search)

    def set_rate(self, T, q_min=1, q_max=31, W=4):
        self.L.sim_chain_set_rate(self.h, T, q_min, q_max, W)
        self.rate = T != 0

    def chain_reset(self, stream=None):
        if self.L.sim_chain_reset(self.h, ALL if stream is None else stream) < 0:
            raise RuntimeError("stream %r >= max_streams" % (stream,))

    def chain_info(self, stream):
        out = np.zeros(2, np.uint32)
        if self.L.sim_chain_info(self.h, stream, out.ctypes.data) < 0:
            raise RuntimeError("stream %r >= max_streams" % (stream,))
        return bool(out[0]), int(out[1])

    def record(self, stream):
        out = np.zeros(4, np.uint32)
        self.L.sim_chain_record(self.h, stream, out.ctypes.data)
        return dict(have=int(out[0]), n=int(out[1]), parity=int(out[2]), rated=int(out[3]))

    def set_record(self, stream, have, n, parity=0, rated=0):
        v = np.ascontiguousarray([have, n, parity, rated], dtype=np.uint32)
        self.L.sim_chain_set_record(self.h, stream, v.ctypes.data)

    def encode(self, frames, streams=None, qscale=8, end=False, chain=True, cap=None):
        """a call: ep.Result with .ordinals and, with rate control, .rate = [(q, budget, bytes)]; None on overflow"""
        n = len(frames)
        fr = np.ascontiguousarray(np.stack(frames), dtype=np.uint8)
        q = np.ascontiguousarray([qscale] * n if np.isscalar(qscale) else qscale, dtype=np.uint8).copy()
        s = None if streams is None else np.ascontiguousarray(streams, dtype=np.uint32)
        ms, fb = self.max_streams, fr.shape[1]
        cap = cap if cap is not None else 64 + n * (fb * 4 + 4096)
        out = np.zeros(cap + 256 + 16, dtype=np.uint8)
        po, pb = np.zeros(n, np.uint64), np.zeros(n, np.uint32)
        sb, se = np.zeros(ms, np.uint64), np.zeros(ms, np.uint64)
        cw, ch = enc_ref.coded(self.width, self.height)
        mbs = (cw // 16) * (ch // 16)
        recon = np.zeros(n * fb + 16, dtype=np.uint8)
        info, stats, ordinal = np.zeros(n * mbs, np.uint32), np.zeros(n * 4, np.uint32), np.zeros(n, np.uint32)
        budget, size = np.zeros(n, np.uint64), np.zeros(n, np.uint32)
        total = self.L.sim_chain_encode(self.h, fr.ctypes.data, n, None if s is None else s.ctypes.data, q.ctypes.data, (1 if end else 0) | (2 if chain else 0),
                                        out.ctypes.data, cap, po.ctypes.data, pb.ctypes.data, sb.ctypes.data, se.ctypes.data, recon.ctypes.data,
                                        info.ctypes.data, stats.ctypes.data, ordinal.ctypes.data, budget.ctypes.data, size.ctypes.data)
        assert total != -2, "the simulator covers the level loop only (gop > 1, or rate control)"
        if total < 0:
            return None
        assert np.all(out[total:total + 256] == 0xff)
        present = sorted(set([0] * n if streams is None else [int(v) for v in streams]))
        vectors = [[None if (v & 3) == 0 else (ep._s8(v >> 16), ep._s8(v >> 24)) for v in info[k * mbs:(k + 1) * mbs].tolist()] for k in range(n)]
        r = ep.Result(out[:total].tobytes(), [(int(po[k]), int(pb[k])) for k in range(n)], {i: (int(sb[i]), int(se[i])) for i in present},
                      [recon[k * fb:(k + 1) * fb].copy() for k in range(n)], vectors, [tuple(int(v) for v in stats[4 * k:4 * k + 4]) for k in range(n)],
                      [(int(sb[i]), int(se[i])) for i in range(ms)])
        r.ordinals = [int(v) for v in ordinal]
        r.rate = [(int(q[k]), int(budget[k]), int(size[k])) for k in range(n)] if self.rate else None
        return r


def next_ordinal(ordinal, gop):
    return int(sim().sim_chain_next(ordinal, gop))


def splits(n):
    """all 2 ** (n - 1) ways of cutting n pictures into consecutive calls: lists of call lengths"""
    out = []
    for mask in range(1 << (n - 1)):
        cuts, run = [], 1
        for i in range(n - 1):
            if mask >> i & 1:
                cuts.append(run)
                run = 1
            else:
                run += 1
        out.append(cuts + [run])
    return out


class Segment:
    """what the calls left of one stream between two ends of its chain"""

    def __init__(self):
        self.frames, self.pieces, self.recon, self.stats, self.sizes, self.rate, self.ended = [], [], [], [], [], [], False


class Ledger:
    """gathers every call's result per stream; cut(stream) where the test ends a chain by other means than END"""

    def __init__(self):
        self.segments = {}

    def _open(self, s):
        segs = self.segments.setdefault(s, [])
        if not segs or segs[-1].ended:
            segs.append(Segment())
        return segs[-1]

    def cut(self, stream):
        if self.segments.get(stream):
            self.segments[stream][-1].ended = True

    def add(self, frames, streams, r, end):
        streams = [0] * len(frames) if streams is None else [int(s) for s in streams]
        for s in sorted(set(streams)):
            seg = self._open(s)
            b, e = r.streams[s]
            seg.pieces.append(r.buf[b:e])
            at = b
            for k in [k for k in range(len(frames)) if streams[k] == s]:
                assert r.ranges[k][0] == at, "a stream's pictures lie back to back from the stream's begin"
                at += r.ranges[k][1]
                seg.frames.append(frames[k])
                seg.recon.append(r.recon[k])
                seg.stats.append(r.stats[k])
                seg.sizes.append(r.ranges[k][1])
                seg.rate.append(r.rate[k] if getattr(r, "rate", None) else None)
            assert e - at == (4 if end else 0)
            if end:
                seg.ended = True


def one_call(seg, width, height, gop, search, qscale=8, rule=None, closed=None):
    """today's encoder on a segment's pictures in ONE unchained call (the yardstick)"""
    end = seg.ended if closed is None else closed
    if rule:
        return er.sim_encode_rate(seg.frames, width, height, gop, search, end=end, **rule)
    return ep.sim_encode_p(seg.frames, width, height, gop, search, qscale=qscale, end=end)


def assert_segment(seg, one, where, rate=True):
    """pieces concatenated, every picture's reconstruction, kinds, bytes and -- with rate control -- choice"""
    assert b"".join(seg.pieces) == one.stream(0).tobytes(), where
    assert seg.sizes == [b for _, b in one.ranges], where
    assert seg.stats == one.stats, where
    for k in range(len(seg.frames)):
        assert np.array_equal(seg.recon[k], one.recon[k]), (where, k)
    if rate and getattr(one, "rate", None):
        assert seg.rate == one.rate, where


def run_split(frames, width, height, gop, search, cuts, qscale=8, rule=None, encoder=None):
    """one stream cut into calls of `cuts` pictures on a fresh chain (or `encoder`, anything with Chain's encode), END on the last:
    the Segment"""
    led = Ledger()
    own = encoder is None
    c = Chain(width, height) if own else encoder
    try:
        if own:
            c.set_gop(gop, search)
            if rule:
                c.set_rate(rule["T"], rule.get("q_min", 1), rule.get("q_max", 31), rule.get("W", 4))
        at = 0
        for i, n in enumerate(cuts):
            end = i + 1 == len(cuts)
            r = c.encode(frames[at:at + n], None, qscale, end=end, chain=True)
            assert r is not None
            led.add(frames[at:at + n], None, r, end)
            at += n
    finally:
        if own:
            c.close()
    assert len(led.segments[0]) == 1
    return led.segments[0][0]
