"""TEST INFRASTRUCTURE ONLY -- what the tests of the encoder's rate control share, beside tests/enc_p_inputs.py: the CPU
simulator of its kernels (sim_encode_rate of tests/sim/sim_encode_pass.cpp, built on demand), the cases of the issue's list, and
the properties of rule RATE (jsmpeg_amd/csrc/enc_rate.h) that hold for every picture."""
import ctypes

import numpy as np

import enc_inputs as ei
import enc_p_inputs as ep
import enc_ref

ROOT = ei.ROOT
_sim = None


def sim():
    global _sim
    if _sim is None:
        lib = ei.pass_sim()
        vp, u32, u64 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64
        lib.sim_encode_rate.restype = ctypes.c_int64
        lib.sim_encode_rate.argtypes = [vp, u32, u32, u32, vp, u32, u32, u32, u32, u32, u32, u32, u32, u32, vp, u64, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
        _sim = lib
    return _sim


def sim_encode_rate(frames, width, height, gop, search, T, q_min=1, q_max=31, W=4, streams=None, frame_rate_code=5, end=True, max_streams=None, cap=None):
    """the simulator's call with rate control: ep.Result with .rate = [(q, budget, bytes)] per picture, or None on overflow"""
    n = len(frames)
    fr = np.ascontiguousarray(np.stack(frames), dtype=np.uint8)
    s = None if streams is None else np.ascontiguousarray(streams, dtype=np.uint32)
    ms = max_streams or (int(max(streams)) + 1 if streams is not None else 1)
    fb = fr.shape[1]
    cap = cap if cap is not None else 64 + n * (fb * 4 + 4096)
    out = np.zeros(cap + 256 + 16, dtype=np.uint8)
    po, pb = np.zeros(n, np.uint64), np.zeros(n, np.uint32)
    sb, se = np.zeros(ms, np.uint64), np.zeros(ms, np.uint64)
    cw, ch = enc_ref.coded(width, height)
    mbs = (cw // 16) * (ch // 16)
    recon = np.zeros(n * fb + 16, dtype=np.uint8)
    info, stats = np.zeros(n * mbs, np.uint32), np.zeros(n * 4, np.uint32)
    q, budget, size = np.zeros(n, np.uint8), np.zeros(n, np.uint64), np.zeros(n, np.uint32)
    total = sim().sim_encode_rate(fr.ctypes.data, width, height, n, None if s is None else s.ctypes.data, frame_rate_code, 1 if end else 0, ms,
                                  gop, search, T, q_min, q_max, W, out.ctypes.data, cap, po.ctypes.data, pb.ctypes.data, sb.ctypes.data,
                                  se.ctypes.data, recon.ctypes.data, info.ctypes.data, stats.ctypes.data, q.ctypes.data, budget.ctypes.data, size.ctypes.data)
    if total < 0:
        return None
    assert np.all(out[total:total + 256] == 0xff)
    present = sorted(set([0] * n if streams is None else [int(v) for v in streams]))
    vectors = [[None if (v & 3) == 0 else (ep._s8(v >> 16), ep._s8(v >> 24)) for v in info[k * mbs:(k + 1) * mbs].tolist()] for k in range(n)]
    r = ep.Result(out[:total].tobytes(), [(int(po[k]), int(pb[k])) for k in range(n)], {i: (int(sb[i]), int(se[i])) for i in present},
                  [recon[k * fb:(k + 1) * fb].copy() for k in range(n)], vectors, [tuple(int(v) for v in stats[4 * k:4 * k + 4]) for k in range(n)],
                  [(int(sb[i]), int(se[i])) for i in range(ms)])
    r.rate = [(int(q[k]), int(budget[k]), int(size[k])) for k in range(n)]
    return r


# ---------------------------------------------------------------------------------------------------- the cases

class Case:
    def __init__(self, frames, width, height, gop, search, T, q_min=1, q_max=31, W=4, streams=None, max_streams=None, small=True):
        self.frames, self.width, self.height, self.gop, self.search, self.T = frames, width, height, gop, search, T
        self.q_min, self.q_max, self.W, self.streams, self.max_streams = q_min, q_max, W, streams, max_streams
        self.small = small              # 64 x 48 or smaller: the restatement is quick enough to judge the device as well

    def rule(self):
        return dict(T=self.T, q_min=self.q_min, q_max=self.q_max, W=self.W)

    def sim(self):
        return sim_encode_rate(self.frames, self.width, self.height, self.gop, self.search, streams=self.streams, max_streams=self.max_streams, **self.rule())


PAN_STREAMS = [0] * 4 + [2] * 3 + [5] * 2     # numbers with gaps; with gop 3: a GOP of one, a whole GOP, a short one


def rate_cases(libs, base=None):
    """name -> Case: each the smallest input at which something in particular can go wrong"""
    base = base if base is not None else ep.p_cases(libs)
    pan = ep.pan_frames(64, 48, 7, (3, -2))
    out = {}
    out["pan_gop3_T150"] = Case(pan, 64, 48, 3, 7, 150)         # a short last GOP: a GOP of one that fits at no scale
    out["pan_gop4_T100"] = Case(pan, 64, 48, 4, 7, 100)         # pictures that are exactly their budget
    out["pan_T20"] = Case(pan, 64, 48, 3, 7, 20)                # q_max everywhere, budgets of 0
    out["pan_T1500"] = Case(pan, 64, 48, 4, 7, 1500)            # q_min everywhere
    out["pan_gop1"] = Case(pan, 64, 48, 1, 7, 250)              # every picture a GOP of its own, level 0
    f, w, h = base["noise"]
    out["noise_T1500"] = Case(f, w, h, 4, 7, 1500)              # intra macroblocks in P pictures, escapes, sizes far above any budget
    out["noise_T4000"] = Case(f, w, h, 4, 7, 4000)
    f, w, h = base["flat_grey"]
    out["flat_grey"] = Case(f, w, h, 3, 7, 40)                  # skipped runs
    f, w, h = base["flat_wide"]
    out["flat_wide"] = Case(f, w, h, 3, 7, 120, small=False)    # the escape increment
    f, w, h = base["content_177x145"]
    out["content_177x145"] = Case(f, w, h, 3, 7, 3000, small=False)          # not a multiple of 16; q_max 31 in the range
    out["content_177x145_R0"] = Case(f, w, h, 3, 0, 1500, small=False)       # search 0
    f, w, h = base["one_macroblock"]
    out["one_macroblock"] = Case(f, w, h, 3, 7, 60)             # first and last of its slice at once
    f, w, h = base["content_176x144"]
    out["range_4_16"] = Case(f, w, h, 4, 7, 1500, q_min=4, q_max=16, small=False)
    out["range_8_8"] = Case(f, w, h, 4, 7, 1500, q_min=8, q_max=8, small=False)
    pan9 = ep.pan_frames(64, 48, 9, (2, 1))
    out["streams_W1"] = Case(pan9, 64, 48, 3, 7, 120, W=1, streams=PAN_STREAMS, max_streams=7)
    out["streams_W16"] = Case(pan9, 64, 48, 3, 7, 120, W=16, streams=PAN_STREAMS, max_streams=7)
    return out


LONG_RULE = dict(T=65, q_min=6, q_max=10, W=4)
LONG_GOP, LONG_SEARCH = 7, 1


def sim_long(long_call, n=None):
    frames, w, h, streams, _ = long_call
    return sim_encode_rate(frames[:n], w, h, LONG_GOP, LONG_SEARCH, streams=streams[:n], max_streams=ep.LONG_MAX_STREAMS, **LONG_RULE)


# ---------------------------------------------------------------------------------------------------- the properties

def gop_members(streams, gop):
    """the GOPs of a call: lists of picture numbers"""
    out = []
    for k, o in enumerate(ep.ordinals(streams)):
        if o % gop == 0:
            out.append([])
        out[-1].append(k)
    return out


def check_properties(rate, ranges, table, streams, gop, T, q_min, q_max, where):
    """rate: [(q, budget, bytes)], ranges: [(offset, bytes)] of the call, table: [{q: bytes}] (the restatement's)"""
    for k, (q, budget, size) in enumerate(rate):
        assert q_min <= q <= q_max, (where, k)
        assert size == ranges[k][1] == table[k][q], (where, k)
        assert size <= budget or q == q_max, (where, k)
        assert all(table[k][v] > budget for v in range(q_min, q)), (where, k)
    for members in gop_members(streams, gop):
        if all(rate[k][2] <= rate[k][1] for k in members):                 # no picture fell to q_max above its budget
            assert sum(rate[k][2] for k in members) <= len(members) * T, (where, members)
