"""Shared helpers of the log-mel tests: the simulator (tests/sim/sim_logmel.cpp, TEST ONLY) behind ctypes, its stand-alone
program under the sanitizers, and the configs and stream lengths both test files use."""
import ctypes
import os
import struct
import subprocess

import numpy as np

from conftest import ROOT

CSRC = os.path.join(ROOT, "jsmpeg_amd", "csrc")
SIM_SRC = os.path.join(ROOT, "tests", "sim", "sim_logmel.cpp")
END, CHAIN = 1, 2
SCALES = {"power": 0, "log": 1, "log10": 2, "db": 3, "whisper": 4}
LAYOUTS = {"mel_major": 0, "time_major": 1}
MEL_SCALES = {"htk": 0, "slaney": 1}
MEL_NORMS = {"none": 0, "slaney": 1}
DTYPES = {"float32": 0, "float16": 1, "bfloat16": 2}
NP_DTYPES = {"float32": np.float32, "float16": np.float16, "bfloat16": np.uint16}      # bfloat16 as its bits
F = 32                                                                                  # frames per workgroup (LM_F)

WHISPER = dict(sample_rate=16000, n_fft=400, hop=160, n_mels=80, f_min=0.0, f_max=8000.0, mel_scale="slaney", mel_norm="slaney")
CONFIGS = {
    (400, 160, 80): WHISPER,
    (512, 128, 128): dict(sample_rate=16000, n_fft=512, hop=128, n_mels=128, f_min=0.0, f_max=0.0, mel_scale="htk", mel_norm="none"),
    (32, 8, 8): dict(sample_rate=8000, n_fft=32, hop=8, n_mels=8, f_min=0.0, f_max=0.0, mel_scale="htk", mel_norm="none"),
    (1024, 256, 64): dict(sample_rate=48000, n_fft=1024, hop=256, n_mels=64, f_min=20.0, f_max=20000.0, mel_scale="slaney", mel_norm="slaney"),
}

_sim = None


def _stale(target, deps):
    return not os.path.exists(target) or any(os.path.getmtime(d) > os.path.getmtime(target) for d in deps)


def _deps():
    return [SIM_SRC, os.path.join(CSRC, "logmel.h"), os.path.join(CSRC, "pcm_resample.h")]


def sim_lib():
    global _sim
    if _sim is None:
        so = os.path.join(ROOT, "tests", "sim", "libjsmpeg_sim_logmel.so")
        if _stale(so, _deps()):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-Wall", "-Wno-unknown-pragmas",
                                   "-Wno-unused-function", "-I", CSRC, "-o", so, SIM_SRC])
        L = ctypes.CDLL(so)
        vp = ctypes.c_void_p
        L.sim_logmel_rule.argtypes = [vp, vp, vp]
        L.sim_logmel_frames.restype = ctypes.c_uint64
        L.sim_logmel_frames.argtypes = [vp, vp, ctypes.c_uint64, ctypes.c_int]
        L.sim_logmel_basis.argtypes = [vp, vp, vp, vp]
        L.sim_logmel_filters.argtypes = [vp, vp, vp, vp]
        L.sim_logmel_log2.restype = None
        L.sim_logmel_log2.argtypes = [vp, vp, ctypes.c_uint64]
        L.sim_logmel_scale.restype = None
        L.sim_logmel_scale.argtypes = [ctypes.c_int, ctypes.c_float, vp, vp, ctypes.c_uint64]
        L.sim_logmel_call.restype = ctypes.c_int64
        L.sim_logmel_call.argtypes = [vp, vp, vp, vp, vp, vp, ctypes.c_uint32, ctypes.c_uint32, vp, vp, vp, ctypes.c_uint64, vp, vp]
        _sim = L
    return _sim


def sim_main():
    """the stand-alone program of the simulator under the sanitizers"""
    exe = os.path.join(ROOT, "tests", "sim", "_asan", "sim_logmel_asan")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    if _stale(exe, _deps()):
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                               "-Wno-unknown-pragmas", "-DSIM_LOGMEL_MAIN", "-I", CSRC, "-o", exe, SIM_SRC])
    return exe


def cfg_arrays(sample_rate=16000, n_fft=400, hop=160, n_mels=80, f_min=0.0, f_max=0.0, mel_scale="slaney", mel_norm="slaney", floor=1e-10, scale="log10",
               layout="mel_major", dtype="float32", row=0, **_):
    icfg = np.array([sample_rate, n_fft, hop, n_mels, MEL_SCALES[mel_scale], MEL_NORMS[mel_norm], SCALES[scale], LAYOUTS[layout], DTYPES[dtype], row], np.int32)
    fcfg = np.array([f_min, f_max, floor], np.float32)
    return icfg, fcfg


def sim_rule(**cfg):
    """dict(bins, cols, F, lds_floats, carry, sh, fstride), or None when the settings are refused"""
    icfg, fcfg = cfg_arrays(**cfg)
    out = np.zeros(7, np.int32)
    if sim_lib().sim_logmel_rule(icfg.ctypes.data, fcfg.ctypes.data, out.ctypes.data) != 0:
        return None
    return dict(zip(("bins", "cols", "F", "lds_floats", "carry", "sh", "fstride"), (int(v) for v in out)))


def sim_frames(n, end, **cfg):
    icfg, fcfg = cfg_arrays(**cfg)
    return int(sim_lib().sim_logmel_frames(icfg.ctypes.data, fcfg.ctypes.data, n, int(end)))


def sim_basis(window=None, **cfg):
    icfg, fcfg = cfg_arrays(**cfg)
    out = np.zeros((cfg.get("n_fft", 400), sim_rule(**cfg)["cols"]), np.float32)
    w = None if window is None else np.ascontiguousarray(window, np.float32)
    assert sim_lib().sim_logmel_basis(icfg.ctypes.data, fcfg.ctypes.data, None if w is None else w.ctypes.data, out.ctypes.data) == 0
    return out


def sim_filters(**cfg):
    icfg, fcfg = cfg_arrays(**cfg)
    fb = np.zeros((cfg.get("n_mels", 80), sim_rule(**cfg)["bins"]), np.float32)
    rg = np.zeros((cfg.get("n_mels", 80), 2), np.int32)
    assert sim_lib().sim_logmel_filters(icfg.ctypes.data, fcfg.ctypes.data, fb.ctypes.data, rg.ctypes.data) == 0
    return fb, rg


def sim_log2(x):
    x = np.ascontiguousarray(x, np.float32)
    out = np.zeros_like(x)
    sim_lib().sim_logmel_log2(x.ctypes.data, out.ctypes.data, x.size)
    return out


def sim_scale(scale, floor, x):
    x = np.ascontiguousarray(x, np.float32)
    out = np.zeros_like(x)
    sim_lib().sim_logmel_scale(SCALES[scale], floor, x.ctypes.data, out.ctypes.data, x.size)
    return out


class SimState:
    """the chain state a handle keeps: records and carries per stream number"""

    def __init__(self, max_streams, **cfg):
        self.rec = np.zeros((max_streams, 2), np.uint64)          # {have, parity} (two u32), n
        self.carry = np.zeros((max_streams, 2 * sim_rule(**cfg)["carry"]), np.float32)

    def reset(self, stream=None):
        if stream is None:
            self.rec[:] = 0
        else:
            self.rec[stream] = 0


def default_row(streams, **cfg):
    return (max([len(s) for s in streams] + [0]) + cfg.get("n_fft", 400) // 2) // cfg.get("hop", 160) + 2


def sim_features(streams, numbers=None, chain=False, end=True, state=None, window=None, want_dft=False, **cfg):
    """streams: float32 samples per stream.  -> (array [streams][n_mels][row] or [streams][row][n_mels], counts[, dft
    [streams][row][bins][2]]).  The output buffer has exactly the call's size and a guard behind it that must stay untouched."""
    L = sim_lib()
    streams = [np.ascontiguousarray(s, dtype=np.float32).reshape(-1) for s in streams]
    n = len(streams)
    cfg = dict(cfg)
    if not cfg.get("row"):
        cfg["row"] = default_row(streams, **cfg)
    row, n_mels, dtype = cfg["row"], cfg.get("n_mels", 80), cfg.get("dtype", "float32")
    icfg, fcfg = cfg_arrays(**cfg)
    samples = np.array([len(s) for s in streams], np.uint32)
    ptrs = (ctypes.c_void_p * max(1, n))(*[s.ctypes.data if len(s) else None for s in streams])
    nums = None if numbers is None else np.ascontiguousarray(numbers, dtype=np.uint32)
    w = None if window is None else np.ascontiguousarray(window, np.float32)
    elem = np.dtype(NP_DTYPES[dtype]).itemsize
    cap = n * n_mels * row * elem
    guard = 64
    out = np.full(cap + guard, 0xA5, np.uint8)
    count = np.zeros(max(1, n), np.uint64)
    dft = np.zeros((n, row, sim_rule(**cfg)["bins"], 2), np.float32) if want_dft else None
    total = L.sim_logmel_call(icfg.ctypes.data, fcfg.ctypes.data, None if w is None else w.ctypes.data, ptrs, samples.ctypes.data,
                              None if nums is None else nums.ctypes.data, n, (CHAIN if chain else 0) | (END if end else 0),
                              None if state is None else state.rec.ctypes.data, None if state is None else state.carry.ctypes.data, out.ctypes.data, cap,
                              count.ctypes.data, None if dft is None else dft.ctypes.data)
    if total < 0:
        raise RuntimeError("sim_logmel_call: %d" % total)
    assert total * elem == cap and (out[cap:] == 0xA5).all()      # nothing was written behind the call's bytes
    shape = (n, n_mels, row) if cfg.get("layout", "mel_major") == "mel_major" else (n, row, n_mels)
    feats = out[:cap].view(NP_DTYPES[dtype]).reshape(shape).copy()
    counts = [int(c) for c in count[:n]]
    return (feats, counts, dft) if want_dft else (feats, counts)


def frames_axis(feats, layout):
    """[streams][row][n_mels] whatever the layout"""
    return feats.transpose(0, 2, 1) if layout == "mel_major" else feats


def chain_splits(n_fft, hop):
    """the split lists of one stream of 7 hop + n_fft samples: piece lengths per call (0: the stream has no samples in that call)"""
    n, h = 7 * hop + n_fft, n_fft // 2
    out = []
    for k in range(1, 8):
        for d in (-1, 0, 1):
            out.append([k * hop + d, n - k * hop - d])
    out.append([h, n - h])
    out.append([h + 1, n - h - 1])
    at = h + 2 * hop                      # the last sample of frame 2 is at - 1: singles across that boundary
    out.append([at - 2, 1, 1, 1, 1, n - at - 2])
    out.append([3 * hop, 0, n - 3 * hop])             # absent from a middle call
    out.append([n, 0])                                # with END: the last call has no new samples
    return n, out


def write_cases(path, cases):
    """the stand-alone program's input: cases = [(cfg dict, end, [calls: [samples per stream]], [pcm per stream])]"""
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(cases)))
        for cfg, end, calls, pcm in cases:
            icfg, fcfg = cfg_arrays(**cfg)
            f.write(icfg.astype("<i4").tobytes() + fcfg.astype("<f4").tobytes())
            f.write(struct.pack("<III", int(end), len(pcm), len(calls)))
            for call in calls:
                f.write(np.asarray(call, "<u4").tobytes())
            for s, x in enumerate(pcm):
                x = np.ascontiguousarray(x, "<f4")
                assert len(x) == sum(call[s] for call in calls)
                f.write(x.tobytes())
