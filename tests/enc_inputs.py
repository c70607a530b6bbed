"""TEST INFRASTRUCTURE ONLY -- what the encoder's tests and tools share: the builder of the CPU simulators (build_sim), the
simulator of the encoder's pass (tests/sim/sim_encode_pass.cpp, built on demand; its intra entry points are bound here, the
others in enc_p_inputs, enc_rate_inputs and enc_chain_inputs), the input pictures, and small stream helpers."""
import ctypes
import glob
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "enc"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import enc_ref  # noqa: E402
import mpeg1_enc  # noqa: E402

CSRC = os.path.join(ROOT, "jsmpeg_amd", "csrc")
SIM_DIR = os.path.join(ROOT, "tests", "sim")
PASS_SRC = os.path.join(SIM_DIR, "sim_encode_pass.cpp")
CXXFLAGS = ["-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-Wno-unused-function", "-I", CSRC, "-I", os.path.join(ROOT, "include")]
_libs = {}
_sim = None


def sim_deps(source, deps=()):
    """what a simulator is built from: its source, the headers it may include, and `deps`"""
    return [source] + list(deps) + glob.glob(os.path.join(CSRC, "*.h")) + [os.path.join(ROOT, "include", "jsmpeg_hip.h")]


def build_sim(source, name, deps=()):
    """tests/sim/lib<name>.so from `source`, rebuilt when anything of sim_deps is newer; the library, one object per name"""
    if name not in _libs:
        so = os.path.join(SIM_DIR, "lib%s.so" % name)
        if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in sim_deps(source, deps)):
            subprocess.check_call(["g++", "-O2", "-fPIC", "-shared"] + CXXFLAGS + ["-o", so, source])
        _libs[name] = ctypes.CDLL(so)
    return _libs[name]


def pass_sim():
    """the simulator of the encoder's pass: one library behind the sim() of this module, enc_p_inputs, enc_rate_inputs and
    enc_chain_inputs, each of which binds its own entry points"""
    return build_sim(PASS_SRC, "jsmpeg_sim_encode_pass")


def sim():
    global _sim
    if _sim is None:
        lib = pass_sim()
        vp, u32, u64 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64
        lib.sim_encode.restype = ctypes.c_int64
        lib.sim_encode.argtypes = [vp, u32, u32, u32, vp, vp, u32, u32, u32, vp, u64, vp, vp, vp, vp]
        lib.sim_enc_rgb.restype = None
        lib.sim_enc_rgb.argtypes = [vp, u32, u32, u32, u32, u32, vp]
        lib.sim_enc_levels.restype = None
        lib.sim_enc_levels.argtypes = [vp, u32, u32, u32, vp]
        lib.sim_enc_coeff_table.restype = ctypes.POINTER(ctypes.c_uint32)
        lib.sim_enc_dc_table.restype = ctypes.POINTER(ctypes.c_uint16)
        lib.sim_enc_dc_table.argtypes = [ctypes.c_int]
        _sim = lib
    return _sim


def sim_encode(frames, width, height, streams=None, qscale=8, frame_rate_code=5, end=True, max_streams=None, cap=None):
    """the simulator's call: (buffer bytes, [(offset, bytes)], {stream: (begin, end)}), or None on overflow"""
    n = len(frames)
    fr = np.ascontiguousarray(np.stack(frames) if n else np.zeros((0, 1), np.uint8), dtype=np.uint8)
    q = np.ascontiguousarray([qscale] * n if np.isscalar(qscale) else qscale, dtype=np.uint8)
    s = None if streams is None else np.ascontiguousarray(streams, dtype=np.uint32)
    ms = max_streams or (int(max(streams)) + 1 if streams is not None and n else 1)
    cap = cap if cap is not None else 64 + n * (fr.shape[1] * 4 + 4096)
    out = np.zeros(cap + 256 + 16, dtype=np.uint8)
    po, pb = np.zeros(max(1, n), np.uint64), np.zeros(max(1, n), np.uint32)
    sb, se = np.zeros(ms, np.uint64), np.zeros(ms, np.uint64)
    total = sim().sim_encode(fr.ctypes.data, width, height, n, None if s is None else s.ctypes.data, q.ctypes.data, frame_rate_code,
                             1 if end else 0, ms, out.ctypes.data, cap, po.ctypes.data, pb.ctypes.data, sb.ctypes.data, se.ctypes.data)
    if total < 0:
        return None
    assert np.all(out[total:total + 256] == 0xff)
    present = sorted(set([0] * n if streams is None else [int(v) for v in streams]))
    return out[:total].tobytes(), [(int(po[k]), int(pb[k])) for k in range(n)], {i: (int(sb[i]), int(se[i])) for i in present}


def sim_levels(frame, width, height, q):
    cw, ch = enc_ref.coded(width, height)
    out = np.zeros((cw // 16) * (ch // 16) * 6 * 64, dtype=np.int16)
    f = np.ascontiguousarray(frame, dtype=np.uint8)
    sim().sim_enc_levels(f.ctypes.data, width, height, q, out.ctypes.data)
    return out.reshape(-1, 6, 64).astype(np.int64)


def sim_rgb(rgb, layout, order):
    """rgb: uint8 [N, 3, H, W] (layout 0) or [N, H, W, 3] (layout 1) -> [N, frame_bytes]"""
    rgb = np.ascontiguousarray(rgb, dtype=np.uint8)
    n = rgb.shape[0]
    h, w = (rgb.shape[2], rgb.shape[3]) if layout == 0 else (rgb.shape[1], rgb.shape[2])
    cw, ch = enc_ref.coded(w, h)
    out = np.zeros((n, cw * ch * 3 // 2), dtype=np.uint8)
    sim().sim_enc_rgb(rgb.ctypes.data, layout, order, w, h, n, out.ctypes.data)
    return out


# ---------------------------------------------------------------------------------------------------- inputs

def frame_of(y, cr, cb):
    return np.concatenate([np.asarray(p, dtype=np.uint8).ravel() for p in (y, cr, cb)])


def content_frames(width, height, n, seed=11):
    cw, ch = enc_ref.coded(width, height)
    out = []
    for f in mpeg1_enc.content(width, height, n, seed):
        y, u, v = mpeg1_enc.pad_planes(f, cw, ch)
        out.append(frame_of(np.rint(y), np.rint(v), np.rint(u)))
    return out


def flat_frame(width, height, value):
    cw, ch = enc_ref.coded(width, height)
    return np.full(cw * ch * 3 // 2, value, dtype=np.uint8)


def stripe_frame(width, height):
    """vertical stripes 0 / 255, eight wide in luma and chroma: DC differentials of +-255; and a one-wide stripe region
    whose high frequencies take escape levels, and a four-wide one whose first horizontal coefficient exceeds every level"""
    cw, ch = enc_ref.coded(width, height)
    y = np.where((np.arange(cw) // 8) % 2, 255, 0).astype(np.uint8)[None, :].repeat(ch, 0)
    y[ch // 2:, :] = np.where(np.arange(cw) % 2, 255, 0).astype(np.uint8)[None, :]
    y[ch // 2:, cw // 2:] = np.where((np.arange(cw // 2) // 4) % 2, 0, 255).astype(np.uint8)[None, :]     # half a block wide: coefficient (0, 1) near 924, clamped at q = 1
    c = np.where((np.arange(cw // 2) // 8) % 2, 255, 0).astype(np.uint8)[None, :].repeat(ch // 2, 0)
    return frame_of(y, c, 255 - c)


def noise_frame(width, height, seed=3):
    cw, ch = enc_ref.coded(width, height)
    return np.random.default_rng(seed).integers(0, 256, cw * ch * 3 // 2, dtype=np.uint8)


def golden_frames(libs, name, n):
    """the first n decoded pictures of a golden stream (oracle planes), and its size"""
    from jsmpeg_amd import cabi
    es = np.fromfile(os.path.join(ROOT, "tests", "golden", name + ".m1v"), dtype=np.uint8)
    frames, _, info = cabi.decode_stream(libs["oracle"], es, keep="planes", max_frames=n)
    return [frame_of(*f) for f in frames], info["width"], info["height"]


def small_cases(libs):
    """name -> (frames, width, height): every input of the issue's list but the 1080p pair"""
    out = {}
    for name in ("enc_pan_176x144", "enc_wide_search_208x160"):
        out[name] = golden_frames(libs, name, 3)
    out["content_176x144"] = (content_frames(176, 144, 2), 176, 144)
    out["content_177x145"] = (content_frames(177, 145, 2), 177, 145)
    out["flat"] = ([flat_frame(48, 32, v) for v in (0, 128, 255)], 48, 32)
    out["stripes"] = ([stripe_frame(64, 48)], 64, 48)
    y, cr, cb = enc_ref.planes(out["content_176x144"][0][0], 176, 144)     # 16x16: that picture's macroblock (4, 3), and noise
    out["one_macroblock"] = ([frame_of(y[48:64, 64:80], cr[24:32, 32:40], cb[24:32, 32:40]), noise_frame(16, 16)], 16, 16)
    return out


def start_codes(buf):
    b = np.frombuffer(buf, dtype=np.uint8)
    return int(np.count_nonzero((b[:-3] == 0) & (b[1:-2] == 0) & (b[2:-1] == 1)))


def luma_sse(decoded_planes, frames, width, height):
    """sum of squared luma errors over the display area, and the sample count"""
    cw, ch = enc_ref.coded(width, height)
    sse = 0.0
    for d, f in zip(decoded_planes, frames):
        a = d[0].reshape(ch, cw)[:height, :width].astype(np.float64)
        b = np.asarray(f[:cw * ch]).reshape(ch, cw)[:height, :width].astype(np.float64)
        sse += float(((a - b) ** 2).sum())
    return sse, len(frames) * width * height


def psnr(sse, n):
    return float("inf") if sse == 0 else 10.0 * np.log10(255.0 ** 2 * n / sse)


# ---------------------------------------------------------------------------------------------------- quality

QUALITY_SCALES = (1, 2, 8, 31)


def stream_of(result, stream=0):
    buf, _, sr = result
    b, e = sr[stream]
    return np.frombuffer(buf[b:e], dtype=np.uint8)


def measure_quality(libs, cases, scales=QUALITY_SCALES):
    """The integer encoder (the simulator) against the restatement with a float64 DCT and np.rint in its place, over
    `cases` (name -> (frames, width, height)), per quantiser scale: the share of levels that differ, the largest
    difference, and the luma PSNR of decode(stream) against the source for both -- sums over all the cases' pictures."""
    from jsmpeg_amd import cabi
    out = {}
    for q in scales:
        differ = total = worst = 0
        sse_i = sse_f = n_px = 0
        for name, (frames, w, h) in sorted(cases.items()):
            for f in frames:
                a, b = sim_levels(f, w, h, q), enc_ref.frame_levels(f, w, h, q, exact_float=True)
                differ += int(np.count_nonzero(a != b))
                total += a.size
                worst = max(worst, int(np.abs(a - b).max()))
            dec_i, _, _ = cabi.decode_stream(libs["oracle"], stream_of(sim_encode(frames, w, h, qscale=q)), keep="planes")
            dec_f, _, _ = cabi.decode_stream(libs["oracle"], stream_of(enc_ref.encode(frames, w, h, qscale=q, exact_float=True)), keep="planes")
            assert len(dec_i) == len(dec_f) == len(frames)
            si, n = luma_sse(dec_i, frames, w, h)
            sf, _ = luma_sse(dec_f, frames, w, h)
            sse_i, sse_f, n_px = sse_i + si, sse_f + sf, n_px + n
        out[q] = dict(share=differ / total, worst=worst, psnr_int=psnr(sse_i, n_px), psnr_float=psnr(sse_f, n_px),
                      gap_db=psnr(sse_f, n_px) - psnr(sse_i, n_px), levels=total)
    return out


def quality_cases(libs):
    """the inputs the quality figures are taken over: the small cases and the two 1080p pictures (the q = 1 noise case is
    held to less: tests/test_enc_sim.py)"""
    cases = small_cases(libs)
    cases["content_1920x1080"] = (content_frames(1920, 1080, 2), 1920, 1080)
    return cases
