"""Shared helpers of the MP2 encoder tests: the simulator (tests/sim/sim_mp2_enc.cpp, TEST ONLY) and the oracle's decode."""
import ctypes
import glob
import os
import struct
import subprocess

import numpy as np

from conftest import ROOT
from jsmpeg_amd import cabi

CSRC = os.path.join(ROOT, "jsmpeg_amd", "csrc")
SIM_SRC = os.path.join(ROOT, "tests", "sim", "sim_mp2_enc.cpp")
CHAIN = 2

_sim = None


def _stale(target, deps):
    return not os.path.exists(target) or any(os.path.getmtime(d) > os.path.getmtime(target) for d in deps)


def _deps():
    return [SIM_SRC] + glob.glob(os.path.join(CSRC, "mp2_*.h"))


def sim_lib():
    global _sim
    if _sim is None:
        so = os.path.join(ROOT, "tests", "sim", "libjsmpeg_sim_mp2_enc.so")
        if _stale(so, _deps()):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-Wall", "-Wno-unknown-pragmas",
                                   "-Wno-unused-function", "-I", CSRC, "-o", so, SIM_SRC])
        L = ctypes.CDLL(so)
        L.sim_mp2_enc_chain.restype = ctypes.c_int64
        L.sim_mp2_enc_chain.argtypes = [ctypes.c_void_p] * 4 + [ctypes.c_uint32, ctypes.c_uint32] + [ctypes.c_void_p] * 3 + [ctypes.c_uint64] + [ctypes.c_void_p] * 5
        for name in ("sim_mp2_enc_frame_offset", "sim_mp2_enc_default_pts"):
            getattr(L, name).restype = ctypes.c_uint64
            getattr(L, name).argtypes = [ctypes.c_int] * 3 + [ctypes.c_uint64]
        L.sim_mp2_enc_frame_bytes.restype = ctypes.c_uint32
        L.sim_mp2_enc_frame_bytes.argtypes = [ctypes.c_int] * 3 + [ctypes.c_uint64]
        L.sim_mp2_enc_pcm_s16.argtypes = [ctypes.c_float]
        L.sim_mp2_enc_analysis.restype = None
        L.sim_mp2_enc_analysis.argtypes = [ctypes.c_void_p] * 5
        _sim = L
    return _sim


def sim_analysis(samples):
    """int16 [480 + 1152] of one channel (history first) -> (Y [36][64], Z [36][32], halves [36][32][2], S [36][32]) of the
    kernel's own mp2e_window_sum, mp2e_window_fold, mp2e_y_lo / _hi and mp2e_matrix_sum"""
    x = np.ascontiguousarray(samples, dtype=np.int16)
    assert x.shape == (480 + 1152,)
    Y, Z = np.zeros((36, 64), np.int64), np.zeros((36, 32), np.int64)
    halves, S = np.zeros((36, 32, 2), np.int32), np.zeros((36, 32), np.int32)
    sim_lib().sim_mp2_enc_analysis(x.ctypes.data, Y.ctypes.data, Z.ctypes.data, halves.ctypes.data, S.ctypes.data)
    return Y, Z, halves, S


def sim_main():
    """the stand-alone program of the simulator under the sanitizers"""
    exe = os.path.join(ROOT, "tests", "sim", "_asan", "sim_mp2_enc_asan")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    if _stale(exe, _deps()):
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                               "-Wno-unknown-pragmas", "-DSIM_MP2_ENC_MAIN", "-I", CSRC, "-o", exe, SIM_SRC])
    return exe


class SimState:
    """the chain state a handle keeps: records and carries per stream number"""

    def __init__(self, max_streams):
        self.rec = np.zeros((max_streams, 2), np.uint64)          # {have, parity} (two u32), n (u64)
        self.carry = np.zeros((max_streams, 2, 2, 480), np.int16)

    def reset(self, stream=None):
        if stream is None:
            self.rec[:] = 0
        else:
            self.rec[stream] = 0

    def info(self, stream):
        have = int(self.rec[stream, 0]) & 0xffffffff
        return bool(have), int(self.rec[stream, 1]) if have else 0


def sim_encode(cfg, streams, numbers=None, chain=False, state=None, want_debug=False):
    """streams: float32 [frames][2][1152] per stream -> ([bytes per stream], stats [frame][4]) or, with want_debug,
    (.., S [frame][2][36][32], dbg [frame][64][8])"""
    L = sim_lib()
    streams = [np.ascontiguousarray(s, dtype=np.float32).reshape(-1, 2, 1152) for s in streams]
    n = len(streams)
    frames = np.array([len(s) for s in streams], np.uint32)
    total_frames = int(frames.sum())
    ptrs = (ctypes.c_void_p * max(1, n))(*[s.ctypes.data if len(s) else None for s in streams])
    nums = None if numbers is None else np.ascontiguousarray(numbers, dtype=np.uint32)
    cap = total_frames * 1729 + 16 * n + 16
    out = np.full(cap, 0xAA, np.uint8)
    begin, end = np.zeros(max(1, n), np.uint64), np.zeros(max(1, n), np.uint64)
    stats = np.zeros((max(1, total_frames), 4), np.uint32)
    S = np.zeros((max(1, total_frames), 2, 36, 32), np.int32) if want_debug else None
    dbg = np.zeros((max(1, total_frames), 64, 8), np.uint8) if want_debug else None
    c = np.array(cfg, np.int32)
    total = L.sim_mp2_enc_chain(c.ctypes.data, ptrs, frames.ctypes.data, None if nums is None else nums.ctypes.data, n, CHAIN if chain else 0,
                                None if state is None else state.rec.ctypes.data, None if state is None else state.carry.ctypes.data,
                                out.ctypes.data, cap, begin.ctypes.data, end.ctypes.data, stats.ctypes.data,
                                None if S is None else S.ctypes.data, None if dbg is None else dbg.ctypes.data)
    assert total >= 0, total
    pieces = [out[int(begin[i]):int(end[i])].tobytes() for i in range(n)]
    for i in range(n):                                            # the zeros up to the next multiple of 16
        gap_end = (int(end[i]) + 15) & ~15
        assert not out[int(end[i]):gap_end].any() and int(begin[i]) % 16 == 0
    assert total == ((int(end[n - 1]) + 15) & ~15 if n else 0)
    assert (out[total:] == 0xAA).all()                            # nothing was written behind the call's bytes
    if want_debug:
        return pieces, stats[:total_frames], S[:total_frames], dbg[:total_frames]
    return pieces, stats[:total_frames]


def oracle_decode(libs, data):
    """(pcm [frames][2][1152], [frame sizes]) of the oracle decoder over the bytes"""
    pcm, _, sizes, _ = cabi.decode_mp2_stream(libs["oracle"], np.frombuffer(data, np.uint8))
    return pcm, sizes


def write_cases(path, cases):
    """the stand-alone program's input: cases = [(cfg, [calls: [frames per stream]], [pcm per stream])]"""
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(cases)))
        for cfg, calls, pcm in cases:
            f.write(struct.pack("<3iII", *cfg, len(pcm), len(calls)))
            for call in calls:
                f.write(np.asarray(call, "<u4").tobytes())
            for s, x in enumerate(pcm):
                x = np.ascontiguousarray(x, "<f4")
                assert len(x) == sum(call[s] for call in calls)
                f.write(x.tobytes())
