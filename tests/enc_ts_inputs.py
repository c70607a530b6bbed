"""TEST INFRASTRUCTURE ONLY -- what the tests of the TS mux on the device share: the CPU simulator (tests/sim/sim_enc_ts.cpp,
built on demand), the host mux with raw 90 kHz values, and the cases: test_ts_mux.py's SIZES, every payload size 1 .. 400 with
each unit at source offset size % 16, a three-stream case and the seeded random cases."""
import ctypes
import os

import numpy as np

import enc_inputs as ei
from test_ts_mux import SIZES

ROOT = ei.ROOT
SIM_SRC = os.path.join(ei.SIM_DIR, "sim_enc_ts.cpp")
PTS_MASK = (1 << 33) - 1
_sim = None


def sim():
    global _sim
    if _sim is None:
        lib = ei.build_sim(SIM_SRC, "jsmpeg_sim_enc_ts")
        vp, u32, u64 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64
        lib.sim_ts_mux.restype = ctypes.c_int64
        lib.sim_ts_mux.argtypes = [vp, vp, vp, vp, vp, u32, u32, u32, vp, u32, vp, u64, vp, vp, vp, vp, vp, ctypes.c_int]
        lib.sim_ts_mux_serial.restype = ctypes.c_int64
        lib.sim_ts_mux_serial.argtypes = [vp, vp, vp, vp, u32, u32, u32, vp, vp]
        lib.sim_ts_packets.restype = u32
        lib.sim_ts_packets.argtypes = [u32]
        lib.sim_ts_bound.restype = u64
        lib.sim_ts_bound.argtypes = [u64, u32, u32]
        lib.sim_ts_default_pts.restype = u64
        lib.sim_ts_default_pts.argtypes = [u32, u32]
        _sim = lib
    return _sim


class Case:
    """es: the source bytes; ranges: [(offset, bytes)]; pts: 90 kHz integers; streams: ascending stream numbers, a stream's
    units contiguous; cc: {stream: start counter}"""

    def __init__(self, es, ranges, pts, streams=None, cc=None, n_streams=None):
        self.es, self.ranges, self.pts = es, list(ranges), [int(p) for p in pts]
        self.streams = [0] * len(self.ranges) if streams is None else [int(s) for s in streams]
        self.n_streams = n_streams or (max(self.streams) + 1 if self.streams else 1)
        self.cc = {s: 0 for s in set(self.streams)}
        self.cc.update(cc or {})
        self.payload = sum(b for _, b in self.ranges)

    def present(self):
        return sorted(set(self.streams))

    def of(self, s):
        """the indices of stream s's units"""
        return [i for i, v in enumerate(self.streams) if v == s]

    def counters(self):
        out = [0] * self.n_streams
        for s, c in self.cc.items():
            out[s] = c
        return out

    def bound(self):
        return int(sim().sim_ts_bound(self.payload, len(self.ranges), len(self.present())))

    def pick(self, idx, cc=None):
        """the case of the units idx alone"""
        return Case(self.es, [self.ranges[i] for i in idx], [self.pts[i] for i in idx], [self.streams[i] for i in idx],
                    dict(self.cc) if cc is None else cc, self.n_streams)


def host_mux(es, ranges, pts, cc=0, stream_id=0xE0, pid=0x100):
    """jsmpeg_hip_ts_mux_host over one stream's units with raw 90 kHz values: (bytes, counter out)"""
    from jsmpeg_amd import encode
    L = encode.lib()
    n = len(ranges)
    off = np.ascontiguousarray([r[0] for r in ranges], dtype=np.uint64)
    ln = np.ascontiguousarray([r[1] for r in ranges], dtype=np.uint32)
    p90 = np.ascontiguousarray(pts, dtype=np.uint64)
    c = ctypes.c_uint8(cc)
    need = L.jsmpeg_hip_ts_mux_host(es.ctypes.data, off.ctypes.data, ln.ctypes.data, p90.ctypes.data, n, stream_id, pid, ctypes.byref(c), None, 0)
    assert need >= 0
    out = np.zeros(max(1, need), np.uint8)
    assert L.jsmpeg_hip_ts_mux_host(es.ctypes.data, off.ctypes.data, ln.ctypes.data, p90.ctypes.data, n, stream_id, pid, ctypes.byref(c), out.ctypes.data, need) == need
    return out[:need].tobytes(), int(c.value)


def host_want(case, stream_id=0xE0, pid=0x100):
    """{stream: (the host mux's bytes over the stream's units, its counter out)}"""
    out = {}
    for s in case.present():
        idx = case.of(s)
        out[s] = host_mux(case.es, [case.ranges[i] for i in idx], [case.pts[i] for i in idx], case.cc[s], stream_id, pid)
    return out


class SimResult:
    pass


def sim_mux(case, cap=None, aligned=False, stream_id=0xE0, pid=0x100):
    """the simulator's call: .total, .buf (uint8 [cap]), .ranges {stream: (begin, end)}, .cc [n_streams] out, .units [(at,
    packets, cc)]; on overflow .total is -1 and .cc what the call left"""
    n, ns = len(case.ranges), case.n_streams
    es = case.es
    if aligned:                                               # the dwords around a unit's ends are read: keep them inside
        es = np.zeros((case.es.size + 3) // 4 * 4 + 16, np.uint8)[:(case.es.size + 3) // 4 * 4]
        es[:case.es.size] = case.es
    off = np.ascontiguousarray([r[0] for r in case.ranges], dtype=np.uint64)
    ln = np.ascontiguousarray([r[1] for r in case.ranges], dtype=np.uint32)
    st = np.ascontiguousarray(case.streams, dtype=np.uint32)
    p90 = np.ascontiguousarray(case.pts, dtype=np.uint64)
    cc = np.ascontiguousarray(case.counters(), dtype=np.uint32)
    cap = case.bound() if cap is None else cap
    ts = np.full(cap + 8, 0xA5, np.uint8)
    sb, se = np.zeros(ns, np.uint64), np.zeros(ns, np.uint64)
    ua, up, uc = np.zeros(max(1, n), np.uint64), np.zeros(max(1, n), np.uint32), np.zeros(max(1, n), np.uint32)
    r = SimResult()
    r.total = int(sim().sim_ts_mux(es.ctypes.data, off.ctypes.data, ln.ctypes.data, st.ctypes.data, p90.ctypes.data, n, stream_id, pid,
                                   cc.ctypes.data, ns, ts.ctypes.data, cap, sb.ctypes.data, se.ctypes.data, ua.ctypes.data, up.ctypes.data,
                                   uc.ctypes.data, 1 if aligned else 0))
    assert np.all(ts[cap:] == 0xA5)
    r.buf, r.cc = ts[:cap], [int(c) for c in cc]
    r.ranges = {s: (int(sb[s]), int(se[s])) for s in case.present()}
    r.units = [(int(ua[i]), int(up[i]), int(uc[i])) for i in range(n)]
    return r


def assert_equals_host(case, got_buf, got_ranges, got_cc, where, want=None):
    """per stream the host mux's bytes and counter; begins multiples of 16, ranges in stream order without overlap"""
    want = host_want(case) if want is None else want
    at = 0
    for s in case.present():
        b, e = got_ranges[s]
        assert b % 16 == 0 and b >= at and b - at < 16, (where, s, b, at)
        assert bytes(got_buf[b:e]) == want[s][0], (where, s)
        assert got_cc[s] == want[s][1], (where, s)
        at = e
    return at


# ---------------------------------------------------------------------------------------------------- cases

def sizes_case(seed=1, lead=5, sizes=SIZES):
    """`sizes` units back to back, the first at byte `lead` of the buffer; the first PTS needs bit 32"""
    rng = np.random.default_rng(seed)
    es = rng.integers(0, 256, lead + sum(sizes), dtype=np.uint8)
    ranges, at = [], lead
    for n in sizes:
        ranges.append((at, n))
        at += n
    pts = [PTS_MASK - 90000 if i == 0 else 45000 + 3000 * i for i in range(len(sizes))]
    return Case(es, ranges, pts)


def sweep_case(seed=7):
    """every payload size 1 .. 400, the unit of size n at a source offset that is n % 16 modulo 16: all stuffing lengths, all
    alignments"""
    ranges, at = [], 0
    for n in range(1, 401):
        at += (n % 16 - at) % 16
        ranges.append((at, n))
        at += n
    es = np.random.default_rng(seed).integers(0, 256, at, dtype=np.uint8)
    return Case(es, ranges, [1000 * i for i in range(400)], cc={0: 9})


def three_stream_case(seed=3):
    """streams 0, 2 and 5; sizes around the packet and PES-length edges"""
    sizes = {0: [170, 174, 4000], 2: [65528, 1, 184 * 3 - 14], 5: [184 * 400 - 14, 300, 65527, 2000]}
    rng = np.random.default_rng(seed)
    ranges, streams, at = [], [], 3
    for s in sorted(sizes):
        for n in sizes[s]:
            ranges.append((at, n))
            streams.append(s)
            at += n + int(rng.integers(0, 7))
    es = rng.integers(0, 256, at, dtype=np.uint8)
    pts = [int(rng.integers(0, 1 << 33)) for _ in ranges]
    return Case(es, ranges, pts, streams, cc={0: 15, 2: 7, 5: 12}, n_streams=7)


def random_cases(n=300, seed=2025):
    """1 to 5 streams with gaps in their numbers, random start counters, a few units above 65527 bytes"""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        ranges, streams, cc, at, s = [], [], {}, int(rng.integers(0, 16)), int(rng.integers(0, 3))
        for _ in range(int(rng.integers(1, 6))):
            cc[s] = int(rng.integers(0, 16))
            for _ in range(int(rng.integers(1, 5))):
                b = int(rng.integers(65528, 75000)) if rng.integers(0, 12) == 0 else int(rng.integers(1, 3000))
                at += int(rng.integers(0, 5))
                ranges.append((at, b))
                streams.append(s)
                at += b
            s += int(rng.integers(1, 4))
        es = rng.integers(0, 256, at, dtype=np.uint8)
        out.append(Case(es, ranges, [int(v) for v in rng.integers(0, 1 << 34, len(ranges))], streams, cc, s + int(rng.integers(0, 3))))
    return out
