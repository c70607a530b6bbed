"""Shared helpers of the resampler tests: the simulator (tests/sim/sim_resample.cpp, TEST ONLY) behind ctypes, and its
stand-alone program under the sanitizers."""
import ctypes
import os
import struct
import subprocess

import numpy as np

from conftest import ROOT

CSRC = os.path.join(ROOT, "jsmpeg_amd", "csrc")
SIM_SRC = os.path.join(ROOT, "tests", "sim", "sim_resample.cpp")
END, CHAIN = 1, 2
FORMS = {"waveform": 0, "frames": 1}
DTYPES = {"float32": 0, "float16": 1, "bfloat16": 2}
NP_DTYPES = {"float32": np.float32, "float16": np.float16, "bfloat16": np.uint16}      # bfloat16 as its bits
FRAME = 1152

_sim = None


def _stale(target, deps):
    return not os.path.exists(target) or any(os.path.getmtime(d) > os.path.getmtime(target) for d in deps)


def _deps():
    return [SIM_SRC, os.path.join(CSRC, "pcm_resample.h")]


def sim_lib():
    global _sim
    if _sim is None:
        so = os.path.join(ROOT, "tests", "sim", "libjsmpeg_sim_resample.so")
        if _stale(so, _deps()):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-Wall", "-Wno-unknown-pragmas",
                                   "-Wno-unused-function", "-I", CSRC, "-o", so, SIM_SRC])
        L = ctypes.CDLL(so)
        vp = ctypes.c_void_p
        L.sim_resample_plan.argtypes = [ctypes.c_int, ctypes.c_int, vp]
        L.sim_resample_taps.argtypes = [ctypes.c_int, ctypes.c_int, vp]
        L.sim_resample_outputs.restype = ctypes.c_uint64
        L.sim_resample_outputs.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_uint64]
        L.sim_resample_f16.restype = L.sim_resample_bf16.restype = ctypes.c_uint32
        L.sim_resample_f16.argtypes = L.sim_resample_bf16.argtypes = [ctypes.c_float]
        L.sim_resample_state_floats.restype = ctypes.c_uint32
        L.sim_resample_state_floats.argtypes = [ctypes.c_int]
        L.sim_resample_call.restype = ctypes.c_int64
        L.sim_resample_call.argtypes = [vp, ctypes.c_float, vp, vp, vp, ctypes.c_uint32, ctypes.c_uint32, vp, vp, vp, vp, ctypes.c_uint64, vp, vp]
        _sim = L
    return _sim


def sim_main():
    """the stand-alone program of the simulator under the sanitizers"""
    exe = os.path.join(ROOT, "tests", "sim", "_asan", "sim_resample_asan")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    if _stale(exe, _deps()):
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                               "-Wno-unknown-pragmas", "-DSIM_RESAMPLE_MAIN", "-I", CSRC, "-o", exe, SIM_SRC])
    return exe


def sim_plan(in_rate, out_rate):
    out = np.zeros(3, np.int32)
    if sim_lib().sim_resample_plan(in_rate, out_rate, out.ctypes.data) != 0:
        return None
    return tuple(int(v) for v in out)


def sim_taps(in_rate, out_rate):
    L, _, H = sim_plan(in_rate, out_rate)
    out = np.zeros((L, 2 * H), np.float32)
    assert sim_lib().sim_resample_taps(in_rate, out_rate, out.ctypes.data) == 0
    return out


class SimState:
    """the chain state a handle keeps: records, input carries and partial frames per stream number"""

    def __init__(self, max_streams):
        L = sim_lib()
        self.rec = np.zeros((max_streams, 3), np.uint64)          # {have, parity} (two u32), n_in, n_out
        self.carry = np.zeros((max_streams, L.sim_resample_state_floats(0)), np.float32)
        self.part = np.zeros((max_streams, L.sim_resample_state_floats(1)), np.float32)

    def reset(self, stream=None):
        if stream is None:
            self.rec[:] = 0
        else:
            self.rec[stream] = 0

    def info(self, stream):
        have = int(self.rec[stream, 0]) & 0xffffffff
        return bool(have), int(self.rec[stream, 1]) if have else 0, int(self.rec[stream, 2]) if have else 0


def sim_resample(in_rate, out_rate, streams, channels=2, form="waveform", dtype="float32", gain=1.0, row=None, numbers=None, chain=False, end=False,
                 state=None):
    """streams: float32 [frames][2][1152] per stream.  waveform -> (array [streams][channels][row], counts); frames ->
    ([float32 [whole frames][2][1152] per stream], counts).  The output buffer has exactly the call's size and a guard behind
    it that must stay untouched."""
    L = sim_lib()
    streams = [np.ascontiguousarray(s, dtype=np.float32).reshape(-1, 2, FRAME) for s in streams]
    n = len(streams)
    frames = np.array([len(s) for s in streams], np.uint32)
    lmh = sim_plan(in_rate, out_rate)
    assert lmh is not None
    if row is None:
        row = -((-(int(frames.max(initial=0)) * FRAME + 2 * FRAME + lmh[2]) * lmh[0]) // lmh[1]) if form == "waveform" else 0
    cfg = np.array([in_rate, out_rate, channels, FORMS[form], DTYPES[dtype], row], np.int32)
    ptrs = (ctypes.c_void_p * max(1, n))(*[s.ctypes.data if len(s) else None for s in streams])
    nums = None if numbers is None else np.ascontiguousarray(numbers, dtype=np.uint32)
    elem = (2 * FRAME * 4) if form == "frames" else np.dtype(NP_DTYPES[dtype]).itemsize
    if form == "frames":
        cap = (int(frames.sum()) * FRAME * lmh[0] // lmh[1] // FRAME + 3 * n + 2) * elem
    else:
        cap = n * channels * row * elem
    guard = 64
    out = np.full(cap + guard, 0xA5, np.uint8)
    offset, count = np.zeros(max(1, n), np.uint64), np.zeros(max(1, n), np.uint64)
    total = L.sim_resample_call(cfg.ctypes.data, gain, ptrs, frames.ctypes.data, None if nums is None else nums.ctypes.data, n,
                                (CHAIN if chain else 0) | (END if end else 0),
                                None if state is None else state.rec.ctypes.data, None if state is None else state.carry.ctypes.data,
                                None if state is None else state.part.ctypes.data, out.ctypes.data, cap, offset.ctypes.data, count.ctypes.data)
    if total < 0:
        raise RuntimeError("sim_resample_call: %d" % total)
    assert (out[total * elem:] == 0xA5).all()                     # nothing was written behind the call's bytes
    counts = [int(c) for c in count[:n]]
    if form == "frames":
        fr = out[:total * elem].view(np.float32).reshape(-1, 2, FRAME)
        assert [int(o) for o in offset[:n]] == [sum(counts[:i]) for i in range(n)] and total == sum(counts)
        return [fr[int(offset[i]):int(offset[i]) + counts[i]].copy() for i in range(n)], counts
    wave = out[:total * elem].view(NP_DTYPES[dtype]).reshape(n, channels, row).copy()
    for i in range(n):
        assert int(offset[i]) == i * channels * row and not wave[i, :, counts[i]:].any()       # a padded batch
    return wave, counts


def write_cases(path, cases):
    """the stand-alone program's input: cases = [(cfg6, gain, end, [calls: [frames per stream]], [pcm per stream])]"""
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(cases)))
        for cfg, gain, end, calls, pcm in cases:
            f.write(struct.pack("<6ifIII", *cfg, gain, int(end), len(pcm), len(calls)))
            for call in calls:
                f.write(np.asarray(call, "<u4").tobytes())
            for s, x in enumerate(pcm):
                x = np.ascontiguousarray(x, "<f4")
                assert len(x) == sum(call[s] for call in calls)
                f.write(x.tobytes())
