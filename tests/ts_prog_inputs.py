"""TEST INFRASTRUCTURE ONLY -- what the tests of the TS program mux (C ABI part 10) share: the CPU simulator
(tests/sim/sim_ts_prog.cpp, built on demand), the host program mux, and the cases -- two unit tables over two source
buffers, the state the call enters with, and the configuration."""
import ctypes
import os

import numpy as np

import enc_inputs as ei

ROOT = ei.ROOT
SIM_SRC = os.path.join(ei.SIM_DIR, "sim_ts_prog.cpp")
PTS_MASK = (1 << 33) - 1
VIDEO, AUDIO = 0, 1
KEY = bytes([0, 0, 1, 0xB3])
_sim = None


def sim():
    global _sim
    if _sim is None:
        lib = ei.build_sim(SIM_SRC, "jsmpeg_sim_ts_prog")
        vp, u32, u64 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64
        lib.sim_tsp_mux.restype = ctypes.c_int64
        lib.sim_tsp_mux.argtypes = [vp, u64, vp, vp, vp, vp, vp, u32, vp, vp, vp, vp, vp, u32, vp, u32, vp, u64, vp, vp, vp, vp, vp, vp, ctypes.c_int]
        lib.sim_tsp_packets.restype = u32
        lib.sim_tsp_packets.argtypes = [u32, u32]
        lib.sim_tsp_bound.restype = u64
        lib.sim_tsp_bound.argtypes = [u64, u32, u64, u32, u32]
        lib.sim_tsp_rank.restype = u32
        lib.sim_tsp_rank.argtypes = [vp, vp, u32, vp, vp, u32, u32, u32]
        _sim = lib
    return _sim


class Table:
    """one kind's units: src (uint8 array), ranges [(offset, bytes)], pts (90 kHz integers), streams (ascending)"""

    def __init__(self, src=None, ranges=(), pts=(), streams=None):
        self.src = np.zeros(0, np.uint8) if src is None else src
        self.ranges, self.pts = list(ranges), [int(p) for p in pts]
        self.streams = [0] * len(self.ranges) if streams is None else [int(s) for s in streams]
        self.payload = sum(b for _, b in self.ranges)

    def __len__(self):
        return len(self.ranges)

    def pick(self, idx):
        return Table(self.src, [self.ranges[i] for i in idx], [self.pts[i] for i in idx], [self.streams[i] for i in idx])

    def arrays(self):
        n = len(self)
        return (np.ascontiguousarray([r[0] for r in self.ranges], dtype=np.uint64), np.ascontiguousarray([r[1] for r in self.ranges], dtype=np.uint32),
                np.ascontiguousarray(self.streams, dtype=np.uint32), np.ascontiguousarray(self.pts, dtype=np.uint64), n)


class Case:
    """video / audio: Tables; state: {stream: [PAT, PMT, video, audio, started]} the call enters with; the rest: the config"""

    def __init__(self, video=None, audio=None, n_streams=None, state=None, psi=False, pcr=False, pcr_lead=0, video_pid=0x100, audio_pid=0x101,
                 pmt_pid=0x1000, program_number=1, transport_stream_id=1):
        self.video, self.audio = video or Table(), audio or Table()
        top = max(self.video.streams + self.audio.streams + [0])
        self.n_streams = n_streams or top + 1
        self.state = {s: list(w) for s, w in (state or {}).items()}
        self.psi, self.pcr, self.pcr_lead = psi, pcr, pcr_lead
        self.video_pid, self.audio_pid, self.pmt_pid = video_pid, audio_pid, pmt_pid
        self.program_number, self.transport_stream_id = program_number, transport_stream_id

    def tables(self):
        return (self.video, self.audio)

    def present(self):
        return sorted(set(self.video.streams) | set(self.audio.streams))

    def words(self):
        out = [[0] * 5 for _ in range(self.n_streams)]
        for s, w in self.state.items():
            out[s] = list(w)
        return out

    def cfg(self, max_ts_bytes=188):
        from jsmpeg_amd import ts_program
        return ts_program.config(self.n_streams, max(1, len(self.video)), max(1, len(self.audio)), max(188, max_ts_bytes), self.video_pid, self.audio_pid,
                                 self.pmt_pid, 0xE0, 0xC0, self.program_number, self.transport_stream_id, self.psi, self.pcr, self.pcr_lead)

    def bound(self):
        return int(sim().sim_tsp_bound(self.video.payload, len(self.video), self.audio.payload, len(self.audio), len(self.present())))

    def lead0(self, kind):
        carrier = VIDEO if self.video_pid != 0x1fff else AUDIO
        return 8 if self.pcr and kind == carrier else 0

    def is_key(self, i):
        o, b = self.video.ranges[i]
        return b >= 4 and self.video.src[o:o + 4].tobytes() == KEY

    def merged(self, s):
        """the units of stream s in the order the rule asks for: a stable sort by (pts, kind) -> [(kind, index)]"""
        units = [(t.pts[i], kind, i) for kind, t in enumerate(self.tables()) for i in range(len(t)) if t.streams[i] == s]
        return [(kind, i) for _, kind, i in sorted(units, key=lambda u: (u[0], u[1]))]

    def split(self, T):
        """(the case of all units with pts < T, the case of the rest); the second enters with whatever state it is given"""
        a = [[i for i in range(len(t)) if t.pts[i] < T] for t in self.tables()]
        b = [[i for i in range(len(t)) if t.pts[i] >= T] for t in self.tables()]
        return self.with_tables(self.video.pick(a[0]), self.audio.pick(a[1])), self.with_tables(self.video.pick(b[0]), self.audio.pick(b[1]))

    def with_tables(self, video, audio, state=None):
        return Case(video, audio, self.n_streams, self.state if state is None else state, self.psi, self.pcr, self.pcr_lead, self.video_pid,
                    self.audio_pid, self.pmt_pid, self.program_number, self.transport_stream_id)


class Result:
    pass


def sim_mux(case, cap=None, aligned=False):
    """the simulator's call: .total (-1 on overflow), .buf (uint8 [cap]), .ranges {stream: (begin, end)}, .state [[5]] behind
    the call, .units = ([(at, bytes, psi_bytes, cc word)] per video unit, the same per audio unit)"""
    ns = case.n_streams
    srcs = []
    for t in case.tables():
        src = t.src
        if aligned:                                           # the dwords around a unit's ends are read: keep them inside
            src = np.zeros((t.src.size + 3) // 4 * 4 + 16, np.uint8)[:(t.src.size + 3) // 4 * 4]
            src[:t.src.size] = t.src
        srcs.append(np.ascontiguousarray(src) if src.size else np.zeros(4, np.uint8))
    cfg = np.ascontiguousarray([case.video_pid, case.audio_pid, case.pmt_pid, 0xE0, 0xC0, (1 if case.psi else 0) | (2 if case.pcr else 0),
                                case.program_number, case.transport_stream_id], dtype=np.uint32)
    (vo, vb, vs, vp, nv), (ao, ab, as_, ap, na) = case.video.arrays(), case.audio.arrays()
    st = np.ascontiguousarray(case.words(), dtype=np.uint32)
    cap = case.bound() if cap is None else cap
    ts = np.full(cap + 8, 0xA5, np.uint8)
    sb, se = np.zeros(ns, np.uint64), np.zeros(ns, np.uint64)
    n = max(1, nv + na)
    ua, ub, up, uc = np.zeros(n, np.uint64), np.zeros(n, np.uint32), np.zeros(n, np.uint32), np.zeros(n, np.uint32)
    r = Result()
    r.total = int(sim().sim_tsp_mux(cfg.ctypes.data, case.pcr_lead, srcs[0].ctypes.data, vo.ctypes.data, vb.ctypes.data, vs.ctypes.data, vp.ctypes.data, nv,
                                    srcs[1].ctypes.data, ao.ctypes.data, ab.ctypes.data, as_.ctypes.data, ap.ctypes.data, na,
                                    st.ctypes.data, ns, ts.ctypes.data, cap, sb.ctypes.data, se.ctypes.data,
                                    ua.ctypes.data, ub.ctypes.data, up.ctypes.data, uc.ctypes.data, 1 if aligned else 0))
    assert np.all(ts[cap:] == 0xA5)
    r.buf, r.state = ts[:cap], [[int(w) for w in row] for row in st]
    r.ranges = {s: (int(sb[s]), int(se[s])) for s in case.present()}
    units = [(int(ua[i]), int(ub[i]), int(up[i]), int(uc[i])) for i in range(nv + na)]
    r.units = (units[:nv], units[nv:])
    return r


def host_mux(case, cap=None):
    """jsmpeg_hip_ts_program_mux_host over the case: .total, .buf, .ranges, .state; RuntimeError when it refuses"""
    from jsmpeg_amd import ts_program
    v, a = case.video, case.audio
    r = Result()
    r.buf, r.ranges, r.state = ts_program.program_mux_host(case.cfg(), v.src, v.ranges, v.pts, v.streams, a.src, a.ranges, a.pts, a.streams, case.words(), cap)
    r.total = len(r.buf)
    return r


def assert_equal(case, got, want, where):
    """two results of one case: the total, every stream's range and bytes, all five words of every stream number"""
    assert got.total == want.total, (where, got.total, want.total)
    assert got.state == want.state, where
    at = 0
    for s in case.present():
        b, e = got.ranges[s]
        assert (b, e) == want.ranges[s] and b % 16 == 0 and 0 <= b - at < 16, (where, s)
        assert bytes(got.buf[b:e]) == bytes(want.buf[b:e]), (where, s)
        at = e
    assert at == got.total, where


def sim_equals_host(case, where, aligned=False):
    got, want = sim_mux(case, aligned=aligned), host_mux(case)
    assert 0 <= got.total <= case.bound(), where
    assert_equal(case, got, want, where)
    return got


# ---------------------------------------------------------------------------------------------------- cases

def from_enc_ts(c, kind=VIDEO):
    """a case of enc_ts_inputs as a one-table program case, PSI and PCR off: the units as they are, the PTS of every stream
    sorted (the program mux refuses a PTS that goes back), the entry counter on the kind's PID"""
    pts = list(c.pts)
    for s in c.present():
        idx = c.of(s)
        for i, p in zip(idx, sorted(pts[i] for i in idx)):
            pts[i] = p
    t = Table(c.es, c.ranges, pts, c.streams)
    state = {s: [0, 0, cc if kind == VIDEO else 0, cc if kind == AUDIO else 0, 0] for s, cc in c.cc.items()}
    return Case(t if kind == VIDEO else None, t if kind == AUDIO else None, c.n_streams, state), pts


def back_to_back(sizes, seed=11, keys=()):
    """(src, ranges): units of `sizes` back to back from byte 3 of random bytes; those in `keys` begin with a sequence header"""
    rng = np.random.default_rng(seed)
    src = rng.integers(0, 256, 3 + sum(sizes), dtype=np.uint8)
    ranges, at = [], 3
    for k, n in enumerate(sizes):
        ranges.append((at, n))
        if k in keys and n >= 4:
            src[at:at + 4] = list(KEY)
        elif n >= 4 and src[at:at + 4].tobytes() == KEY:
            src[at + 3] = 0
        at += n
    return src, ranges


def pcr_sweep_case():
    """every payload size 1 .. 400 as PCR units of one stream, audio frames of 417 / 418 bytes in between"""
    src, ranges = back_to_back(list(range(1, 401)), 21, keys=range(0, 400, 12))
    a_src, a_ranges = back_to_back([417 + (k % 2) for k in range(150)], 22)
    return Case(Table(src, ranges, [3000 * i for i in range(400)]), Table(a_src, a_ranges, [8000 * i for i in range(150)]),
                state={0: [3, 9, 14, 15, 0]}, psi=True, pcr=True, pcr_lead=9000)


def one_unit_case(size, kind=VIDEO, pcr=True, psi=False, state=None, pts=100, seed=5):
    src, ranges = back_to_back([size], seed + size)
    t = Table(src, ranges, [pts])
    return Case(t if kind == VIDEO else None, t if kind == AUDIO else None, 1, state, psi=psi, pcr=pcr, pcr_lead=9000,
                video_pid=0x100 if kind == VIDEO else 0x1fff)


EDGE_ONE_PACKET = (161, 162, 163)                              # 14 + bytes + 8 around 184
EDGE_UNSIZED = (184 * 400 - 22, 184 * 400 - 14)                # above 65527; (14 + bytes + 8) % 184 == 0, (14 + bytes) % 184 == 0


def counters_at_15_case():
    """all four counters enter at 15; PSI in front of the first unit (not started) and of the key pictures"""
    src, ranges = back_to_back([500, 170, 163, 2000, 162], 31, keys=(0, 3))
    a_src, a_ranges = back_to_back([418] * 4, 32)
    return Case(Table(src, ranges, [0, 3000, 6000, 9000, 12000]), Table(a_src, a_ranges, [0, 2351, 4702, 7053]),
                state={0: [15, 15, 15, 15, 0]}, psi=True, pcr=True, pcr_lead=4500)


def random_cases(n=300, seed=2026):
    """up to 5 present streams out of 8: audio-only and video-only streams among them, PTS ties inside a list and across the
    two, key pictures, started and unstarted streams, PSI / PCR on and off, now and then a kind that is absent altogether"""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        absent = int(rng.integers(0, 8))                      # 0: no video at all, 1: no audio at all
        tabs, state = [[], []], {}
        present = sorted(rng.choice(8, int(rng.integers(1, 6)), replace=False).tolist())
        for s in present:
            state[s] = [int(v) for v in rng.integers(0, 16, 4)] + [int(rng.integers(0, 2))]
            shape = int(rng.integers(0, 4))                   # 0: video only, 1: audio only, else both
            for kind in (VIDEO, AUDIO):
                if kind == absent or (shape == 0 and kind == AUDIO and absent != VIDEO) or (shape == 1 and kind == VIDEO and absent != AUDIO):
                    continue
                pts = int(rng.integers(0, 5)) * 1500
                for _ in range(int(rng.integers(1, 6))):
                    big = rng.integers(0, 14) == 0
                    tabs[kind].append((int(rng.integers(65528, 75000)) if big else int(rng.integers(1, 2500)), s, pts, bool(rng.integers(0, 3) == 0)))
                    pts += int(rng.integers(0, 3)) * 1500
        tables = []
        for kind in (VIDEO, AUDIO):
            units = tabs[kind]
            src, ranges = back_to_back([u[0] for u in units], int(rng.integers(0, 1 << 30)), keys=[k for k, u in enumerate(units) if u[3] and kind == VIDEO])
            tables.append(Table(src, ranges, [u[2] for u in units], [u[1] for u in units]))
        out.append(Case(tables[0], tables[1], 8, state, psi=bool(rng.integers(0, 2)), pcr=bool(rng.integers(0, 2)), pcr_lead=int(rng.integers(0, 20000)),
                        video_pid=0x1fff if absent == VIDEO else 0x100, audio_pid=0x1fff if absent == AUDIO else 0x101))
    return out


def count_case(n_v, n_a, n_streams=1, seed=41, per_stream=None):
    """n_v video and n_a audio units of small sizes spread over n_streams streams (per_stream: units of each kind per stream)"""
    rng = np.random.default_rng(seed)
    v_sizes = [int(v) for v in rng.integers(1, 420, n_v)]
    a_sizes = [int(v) for v in rng.integers(100, 420, n_a)]
    src, ranges = back_to_back(v_sizes, seed + 1, keys=range(0, n_v, 7))
    a_src, a_ranges = back_to_back(a_sizes, seed + 2)

    def spread(n):
        return sorted(i % n_streams for i in range(n)) if per_stream is None else [i // per_stream for i in range(n)]

    def pts_of(streams, step):
        out, before, k = [], None, 0
        for s in streams:
            k = 0 if s != before else k + 1
            before = s
            out.append(step * (k // 2 if step == 3000 else k))    # pairs of video units tie
        return out
    vs, as_ = spread(n_v), spread(n_a)
    return Case(Table(src, ranges, pts_of(vs, 3000), vs), Table(a_src, a_ranges, pts_of(as_, 2351), as_), max(n_streams, 1),
                {s: [s & 15, (s + 5) & 15, (s + 9) & 15, (s + 13) & 15, s & 1] for s in range(n_streams)}, psi=True, pcr=True, pcr_lead=1234)


def three_stream_program(seed=51):
    """streams 0, 2 and 5 with video and audio, PSI and PCR on: what the reference's demuxer is run over"""
    rng = np.random.default_rng(seed)
    v_sizes = {0: [170, 174, 4000, 66000], 2: [65528, 1, 184 * 3 - 14, 900], 5: [184 * 400 - 22, 300, 65527, 2000]}
    sizes, streams, pts = [], [], []
    for s in sorted(v_sizes):
        for k, n in enumerate(v_sizes[s]):
            sizes.append(n); streams.append(s); pts.append(90000 + 3000 * k + (PTS_MASK - 95000 if s == 5 else 0))
    src, ranges = back_to_back(sizes, seed, keys=(0, 4, 8, 10))
    a_sizes, a_streams, a_pts = [], [], []
    for s in (0, 2, 5):
        for k in range(5):
            a_sizes.append(626 + int(rng.integers(0, 2))); a_streams.append(s); a_pts.append(90000 + 2351 * k + (PTS_MASK - 95000 if s == 5 else 0))
    a_src, a_ranges = back_to_back(a_sizes, seed + 1)
    return Case(Table(src, ranges, pts, streams), Table(a_src, a_ranges, a_pts, a_streams), 7,
                {0: [15, 3, 7, 12, 0], 2: [1, 2, 3, 4, 1], 5: [0, 0, 15, 15, 0]}, psi=True, pcr=True, pcr_lead=45000)

