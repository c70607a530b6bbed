"""TEST INFRASTRUCTURE ONLY -- what the tests of the encoder's scaled input share: the CPU simulator
(tests/sim/sim_encode_scale.cpp, built on demand), the named cases, their content and the seeded sweep of geometries."""
import ctypes
import os

import numpy as np

import enc_inputs as ei
import enc_scale_ref as es

ROOT = ei.ROOT
_sim = None


class Source(ctypes.Structure):
    _fields_ = [(n, ctypes.c_uint32) for n in ("width", "height", "crop_x", "crop_y", "crop_width", "crop_height", "antialias")]


def source(width, height, crop=None, aa=1):
    return Source(width, height, *(crop or (0, 0, 0, 0)), int(aa))


def sim():
    global _sim
    if _sim is None:
        lib = ei.build_sim(os.path.join(ei.SIM_DIR, "sim_encode_scale.cpp"), "jsmpeg_sim_encode_scale")
        vp, u32 = ctypes.c_void_p, ctypes.c_uint32
        lib.sim_es_check.restype = ctypes.c_char_p
        lib.sim_es_check.argtypes = [ctypes.POINTER(Source)]
        lib.sim_es_taps.restype = None
        lib.sim_es_taps.argtypes = [u32, u32, u32, u32, vp, vp, u32]
        lib.sim_es_frame.restype = ctypes.c_int
        lib.sim_es_frame.argtypes = [vp, ctypes.POINTER(Source), u32, u32, vp]
        lib.sim_es_plan_check.restype = ctypes.c_int
        lib.sim_es_plan_check.argtypes = [ctypes.POINTER(Source), u32, u32, vp]
        _sim = lib
    return _sim


def sim_taps(n_in, n_out, aa, i):
    out, w = np.zeros(2, np.uint32), np.zeros(2 * n_in + 2, np.uint32)
    sim().sim_es_taps(n_in, n_out, aa, i, out.ctypes.data, w.ctypes.data, w.size)
    return int(out[0]), [int(v) for v in w[:out[1]]]


def sim_frame(frame, width, height, out_w, out_h, crop=None, aa=1):
    """the simulator's frame of the coded size of out_w x out_h, or None for a descriptor it refuses"""
    cw, ch = es.coded(out_w, out_h)
    f = np.ascontiguousarray(frame, dtype=np.uint8)
    assert f.size == np.prod(es.coded(width, height)) * 3 // 2
    out = np.zeros(cw * ch * 3 // 2, dtype=np.uint8)
    s = source(width, height, crop, aa)
    return out if sim().sim_es_frame(f.ctypes.data, ctypes.byref(s), out_w, out_h, out.ctypes.data) == 0 else None


def plan_check(width, height, out_w, out_h, crop=None, aa=1):
    """(0 or what is wrong, dict(words, bound, tiles, rows))"""
    out = np.zeros(4, np.uint32)
    s = source(width, height, crop, aa)
    rc = sim().sim_es_plan_check(ctypes.byref(s), out_w, out_h, out.ctypes.data)
    return rc, dict(words=int(out[0]), bound=int(out[1]), tiles=int(out[2]), rows=int(out[3]))


# name -> (source display w, h, crop or None, output w, h, antialias)
CASES = {
    "1_odd_177x145_to_65x33": (177, 145, None, 65, 33, 1),
    "2_cut_out_64x48": (176, 144, (16, 8, 64, 48), 64, 48, 1),
    "3_up_64x48_to_160x112": (64, 48, None, 160, 112, 1),
    "4_one_axis_64x48_to_64x24": (64, 48, None, 64, 24, 1),
    "5_many_taps_640x360_to_40x23": (640, 360, None, 40, 23, 1),
    "6_odd_crop_aa": (333, 251, (2, 2, 171, 141), 80, 64, 1),
    "6_odd_crop_plain": (333, 251, (2, 2, 171, 141), 80, 64, 0),
    "7_1080p_to_640x360": (1920, 1080, None, 640, 360, 1),
}
SMALL = [n for n in sorted(CASES) if not n.startswith("7")]


def smooth_frame(width, height, seed=5):
    """low frequencies only: a few sines per plane"""
    cw, ch = es.coded(width, height)
    rng = np.random.default_rng(seed)

    def plane(w, h):
        y, x = np.mgrid[0:h, 0:w]
        v = np.full((h, w), 128.0)
        for _ in range(3):
            fx, fy, ph = rng.uniform(0.5, 3.0), rng.uniform(0.5, 3.0), rng.uniform(0, 6.28)
            v += 40.0 * np.sin(6.2832 * (fx * x / w + fy * y / h) + ph)
        return np.clip(np.rint(v), 0, 255).astype(np.uint8)
    return ei.frame_of(plane(cw, ch), plane(cw // 2, ch // 2), plane(cw // 2, ch // 2))


_frames = {}


def case_frames(name):
    """the case's two source frames: noise and smooth; case 7: two content pictures"""
    if name not in _frames:
        w, h = CASES[name][:2]
        _frames[name] = ei.content_frames(1920, 1080, 1) + ei.content_frames(1920, 1080, 1, seed=12) if name.startswith("7") \
            else [ei.noise_frame(w, h, seed=len(name)), smooth_frame(w, h)]
    return _frames[name]


_want = {}


def case_want(name):
    """the restatement's frames of a case, computed once"""
    if name not in _want:
        w, h, crop, ow, oh, aa = CASES[name]
        _want[name] = [es.scale_frame(f, w, h, ow, oh, crop, bool(aa)) for f in case_frames(name)]
    return _want[name]


def sweep(n=240, seed=2024, side=96):
    """seeded geometries: (w, h, crop or None, ow, oh, aa) -- sides at most `side`, crops of even and odd sizes, both antialias
    values, up and down mixed per axis, every fourth with one axis unchanged"""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(n):
        w, h = int(rng.integers(1, side + 1)), int(rng.integers(1, side + 1))
        crop = None
        if k % 2:
            x, y = 2 * int(rng.integers(0, (w + 1) // 2)), 2 * int(rng.integers(0, (h + 1) // 2))
            crop = (x, y, int(rng.integers(1, w - x + 1)), int(rng.integers(1, h - y + 1)))
        cw, ch = (crop[2], crop[3]) if crop else (w, h)
        ow, oh = int(rng.integers(1, side + 1)), int(rng.integers(1, side + 1))
        if k % 4 == 2:
            ow = cw
        if k % 4 == 3:
            oh = ch
        out.append((w, h, crop, ow, oh, int(rng.integers(0, 2))))
    return out
