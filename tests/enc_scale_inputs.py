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
        lib.sim_es_axis_scan.restype = None
        lib.sim_es_axis_scan.argtypes = [u32, u32, u32, vp]
        lib.sim_es_axis.restype = u32
        lib.sim_es_axis.argtypes = [u32, u32, u32, vp, vp, u32]
        lib.sim_es_walk.restype = ctypes.c_int
        lib.sim_es_walk.argtypes = [ctypes.POINTER(Source), u32, u32, vp, u32]
        _sim = lib
    return _sim


def axis_scan(n_in, n_out, aa):
    """(smallest weight, largest weight, every sum is 16384, output indices on the rule's second form) over an axis"""
    out = np.zeros(4, np.int32)
    sim().sim_es_axis_scan(n_in, n_out, aa, out.ctypes.data)
    return int(out[0]), int(out[1]), bool(out[2]), int(out[3])


def sim_axis(n_in, n_out, aa):
    """the header's taps of a whole axis: (xmin[n_out], xsize[n_out], all the weights one index after the other, int64)"""
    ent = np.zeros(2 * n_out, np.uint32)
    w = np.zeros(2 * n_in + 3 * n_out + 8, np.int32)       # at most 2 n_in / n_out + 1 taps per index, or two (enc_scale.h)
    n = sim().sim_es_axis(n_in, n_out, aa, ent.ctypes.data, w.ctypes.data, w.size)
    assert n <= w.size
    return ent[0::2].astype(np.int64), ent[1::2].astype(np.int64), w[:n].astype(np.int64)


WALK_FIELDS = ("kind", "tx", "ty", "nw", "nh", "stride", "cr_max", "chunks", "last_rows", "straddle", "phase", "replicated")


def walk(width, height, out_w, out_h, crop=None, aa=1):
    """one dict per workgroup of one picture, as k_enc_scale walks them (sim_es_walk): WALK_FIELDS; replicated: bit 0 columns,
    bit 1 rows"""
    s = source(width, height, crop, aa)
    n = sim().sim_es_walk(ctypes.byref(s), out_w, out_h, None, 0)
    assert n > 0
    rec = np.zeros((n, len(WALK_FIELDS)), np.uint32)
    assert sim().sim_es_walk(ctypes.byref(s), out_w, out_h, rec.ctypes.data, n) == n
    return [dict(zip(WALK_FIELDS, (int(v) for v in row))) for row in rec]


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


# The edges of k_enc_scale's tile walk, each named for what sim_es_walk (walk() above) shows it to reach -- tests/
# test_enc_scale_edges.py holds every name to its class, so an input that falls out of it after a change of a tile constant
# is the thing to change.  Same tuples as CASES.
EDGES = {
    "stride_4096_cr_4": (4094, 40, None, 128, 20, 1),            # luma stride 4096, cr_max 4, ten chunks; chroma cr_max 8
    "identity_rows_cr_4": (4094, 33, None, 100, 33, 1),          # vertical identity at cr_max 4; a chunk of one source row
    "cr_7_last_chunk_6": (2050, 70, None, 64, 33, 1),            # cr_max 7, chroma cr_max 15; second luma tile row nh 16
    "cr_30_full_tile": (530, 100, None, 128, 48, 1),             # cr_max 30 under the cap of 32; a full-width tile, two rows
    "three_columns_aa": (900, 66, None, 260, 36, 1),             # luma tile columns 128 128 16, chroma 128 8; margin 260 -> 272
    "three_columns_plain": (900, 66, None, 260, 36, 0),          # the same with two plain taps
    "upscale_300x40": (150, 20, None, 300, 40, 1),               # luma columns 128 128 48, chroma 128 24; one chunk
    "tall_125_to_1": (16, 1000, None, 8, 70, 1),                 # 125:1 vertically, 15 chunks of 32 rows, three tile rows
}

# a 96 x 40 source to 40 x 16: origins 0, 2, 14 and 2 mod 16, ends 1, 15 and 0 mod 16 and flush with the right and bottom
# edges, crops 1 and 2 wide (a chroma plane of one sample); each is run with both antialias values
CROP_SOURCE, CROP_OUT = (96, 40), (40, 16)
CROPS = [(0, 0, 96, 40), (2, 0, 63, 40), (2, 2, 77, 37), (14, 0, 50, 40), (14, 4, 81, 35), (16, 0, 80, 40), (16, 6, 33, 21), (18, 0, 61, 40),
         (18, 2, 78, 38), (30, 0, 2, 40), (30, 8, 1, 1), (94, 38, 2, 2)]

# a 33 x 17 source to the smallest outputs, each with both antialias values
TINY_SOURCE = (33, 17)
TINY = [(1, 1), (2, 2), (1, 70), (70, 1)]

# The ratios at which the remainder tap of enc_scale.h's first weight form would go below 0, so that the rule's second form
# (cumulative rounding) is what runs -- from the scan of every n_in in 1 .. 4095 (profiles/enc_scale_edges_notes.md): n_out = 1
# fails first at n_in = 1280 and worst at 3120, n_out = 2 first at 2870 and worst at 3418.  The short side of each source is 2.
RATIOS = {
    "first_1280_to_1": (1280, 2, None, 1, 1, 1),
    "worst_3120_to_1": (3120, 2, None, 1, 1, 1),
    "first_2870_to_2": (2870, 2, None, 2, 2, 1),
    "worst_3418_to_2": (3418, 2, None, 2, 1, 1),
    "vertical_3120_to_1": (2, 3120, None, 1, 1, 1),
    "chroma_only_2560_to_2": (2560, 2, None, 2, 2, 1),           # luma 2560 -> 2 keeps the first form, chroma 1280 -> 1 does not
}


def named_geometries():
    """every named geometry beside CASES: [(name, (w, h, crop, ow, oh, aa))]"""
    out = [("edge:" + n, g) for n, g in sorted(EDGES.items())]
    out += [("crop:%d_%d_%d_%d:aa%d" % (c + (aa,)), CROP_SOURCE + (c,) + CROP_OUT + (aa,)) for c in CROPS for aa in (1, 0)]
    out += [("tiny:%dx%d:aa%d" % (ow, oh, aa), TINY_SOURCE + (None, ow, oh, aa)) for ow, oh in TINY for aa in (1, 0)]
    return out + [("ratio:" + n, g) for n, g in sorted(RATIOS.items())]


_noise = {}


def geometry_frames(w, h, seed=100):
    """the two source frames of a geometry beside CASES: noise, another seed per picture"""
    key = (w, h, seed)
    if key not in _noise:
        _noise[key] = [ei.noise_frame(w, h, seed=seed), ei.noise_frame(w, h, seed=seed + 1)]
    return _noise[key]


_scaled = {}


def geometry_want(geo, seed=100):
    """the restatement's two frames of a geometry over geometry_frames, computed once"""
    if (geo, seed) not in _scaled:
        w, h, crop, ow, oh, aa = geo
        _scaled[(geo, seed)] = [es.scale_frame(f, w, h, ow, oh, crop, bool(aa)) for f in geometry_frames(w, h, seed)]
    return _scaled[(geo, seed)]


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
