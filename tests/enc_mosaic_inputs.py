"""TEST INFRASTRUCTURE ONLY -- what the tests of the encoder's mosaic input share: the CPU simulator
(tests/sim/sim_encode_mosaic.cpp, built on demand), the named layouts, their content and the seeded sweep of layouts.
A cell is (source w, source h, crop or None, antialias, x, y, w, h), as tests/enc_mosaic_ref.py reads it."""
import ctypes
import os

import numpy as np

import enc_inputs as ei
import enc_mosaic_ref as em
import enc_scale_inputs as si
import enc_scale_ref as es

ROOT = ei.ROOT
FILL = (16, 128, 128)
_sim = None


class Cell(ctypes.Structure):
    _fields_ = [("source", si.Source)] + [(n, ctypes.c_uint32) for n in ("x", "y", "width", "height")]


def cell_array(cells):
    arr = (Cell * max(1, len(cells)))()
    for k, (sw, sh, crop, aa, x, y, w, h) in enumerate(cells):
        arr[k] = Cell(si.source(sw, sh, crop, aa), x, y, w, h)
    return arr


def fill_word(fill):
    return fill[0] | fill[1] << 8 | fill[2] << 16


def sim():
    global _sim
    if _sim is None:
        lib = ei.build_sim(os.path.join(ei.SIM_DIR, "sim_encode_mosaic.cpp"), "jsmpeg_sim_encode_mosaic")
        vp, u32 = ctypes.c_void_p, ctypes.c_uint32
        lib.sim_em_sizeof_cell.restype = u32
        lib.sim_em_check.restype = ctypes.c_int
        lib.sim_em_check.argtypes = [vp, u32, u32, u32, u32, ctypes.c_char_p, u32]
        lib.sim_em_frame.restype = ctypes.c_int
        lib.sim_em_frame.argtypes = [vp, vp, u32, u32, u32, u32, vp]
        lib.sim_em_plan_check.restype = ctypes.c_int
        lib.sim_em_plan_check.argtypes = [vp, u32, u32, u32, u32, vp]
        _sim = lib
    return _sim


def check(cells, width, height, fill=FILL, n=None, null=False):
    """"" or the layout check's message; n: the cell count handed over (None: len(cells)); null: NULL for the cells"""
    msg = ctypes.create_string_buffer(256)
    arr = cell_array(cells)
    sim().sim_em_check(None if null else arr, len(cells) if n is None else n, fill if isinstance(fill, int) else fill_word(fill), width, height, msg, 256)
    return msg.value.decode()


def sim_frame(cells, frames, width, height, fill=FILL):
    """the simulator's frame of the coded size of width x height (frames: one per cell, None = absent), or None for a layout
    it refuses"""
    cw, ch = es.coded(width, height)
    keep = [None if f is None else np.ascontiguousarray(f, dtype=np.uint8) for f in frames]
    for (sw, sh, *_), f in zip(cells, keep):
        assert f is None or not (1 <= sw <= 4095 and 1 <= sh <= 4095) or f.size == np.prod(es.coded(sw, sh)) * 3 // 2
    ptrs = (ctypes.c_void_p * max(1, len(cells)))(*[None if f is None else f.ctypes.data for f in keep])
    out = np.zeros(cw * ch * 3 // 2, dtype=np.uint8)
    arr = cell_array(cells)
    return out if sim().sim_em_frame(ptrs, arr, len(cells), fill_word(fill), width, height, out.ctypes.data) == 0 else None


def plan_check(cells, width, height, fill=FILL):
    """(0 or what is wrong, dict(words, bound, tiles, rows))"""
    out = np.zeros(4, np.uint32)
    arr = cell_array(cells)
    rc = sim().sim_em_plan_check(arr, len(cells), fill_word(fill), width, height, out.ctypes.data)
    return rc, dict(words=int(out[0]), bound=int(out[1]), tiles=int(out[2]), rows=int(out[3]))


# name -> (encoder w, h, fill, [cells], [present per picture])
A = (352, 288, None, 1, 0, 0, 130, 66)          # antialiased, more source rows per tile than a chunk holds, edges inside tiles
B = (64, 48, None, 0, 130, 0, 143, 70)          # plain bilinear up, flush with the odd right edge
C = (64, 48, None, 1, 8, 20, 64, 48)            # a copy over A: the one-tap path and the paste order
LAYOUTS = {
    # coded 288x80: luma tiles 3x3, chroma tiles 2x2; the rows below 70 stay fill
    "1_wall_273x71": (273, 71, FILL, [A, B, C], [(1, 1, 1), (1, 0, 1)]),
    # picture in picture: a whole-picture cell, a crop over its corner flush with right and bottom, one more over both
    "2_pip_177x145": (177, 145, (40, 90, 200), [(176, 144, None, 1, 0, 0, 177, 145), (64, 48, (16, 8, 31, 25), 1, 114, 96, 63, 49),
                                                (64, 48, None, 0, 100, 80, 40, 30)], [(1, 1, 1), (0, 1, 1)]),
    # a 2 x 2 wall of odd cell sizes with gaps of fill between and around
    "3_grid_gaps_150x100": (150, 100, (235, 16, 240), [(64, 48, None, 1, 0, 0, 71, 47), (176, 144, None, 1, 76, 0, 71, 47),
                                                       (64, 48, None, 0, 0, 52, 71, 47), (176, 144, (32, 16, 88, 72), 1, 76, 52, 71, 47)],
                            [(1, 1, 1, 1), (1, 0, 0, 1)]),
    # everything absent in the second picture
    "4_one_small_cell_33x17": (33, 17, (1, 2, 3), [(64, 48, None, 1, 2, 4, 1, 1)], [(1,), (0,)]),
    # the most cells a layout has: 8 x 8 cells of 18x14, each over its neighbours' edges; every third absent in the second picture
    "5_64_cells_130x100": (130, 100, (90, 100, 110), [(64, 48, None, k & 1, 16 * (k % 8), 12 * (k // 8), 18, 14) for k in range(64)],
                           [(1,) * 64, tuple(int(k % 3 != 0) for k in range(64))]),
}

# Beside LAYOUTS (same tuple): cells whose sources are enc_scale_inputs.RATIOS geometries -- a horizontal tap run whose weights
# take enc_scale.h's second form -- pasted 1 and 2 pixels wide at even x over a whole-picture cell
RATIO_LAYOUT = (64, 48, FILL, [(64, 48, None, 1, 0, 0, 64, 48), si.RATIOS["worst_3120_to_1"][:3] + (1, 22, 10, 1, 9),
                               si.RATIOS["worst_3418_to_2"][:3] + (1, 40, 20, 2, 6)], [(1, 1, 1), (0, 1, 1)])


def ratio_layout_frames():
    """[picture][cell] -> source frame or None, noise throughout"""
    _, _, _, cells, present = RATIO_LAYOUT
    return [[ei.noise_frame(c[0], c[1], seed=40 + 3 * p + k) if here else None for k, (c, here) in enumerate(zip(cells, pic))]
            for p, pic in enumerate(present)]


_frames = {}


def source_frame(sw, sh, seed):
    """a source frame of a size, content by seed: even seeds noise, odd seeds smooth"""
    key = (sw, sh, seed)
    if key not in _frames:
        _frames[key] = si.smooth_frame(sw, sh, seed) if seed & 1 else ei.noise_frame(sw, sh, seed)
    return _frames[key]


def layout_frames(name):
    """[picture][cell] -> source frame or None"""
    _, _, _, cells, present = LAYOUTS[name]
    return [[source_frame(c[0], c[1], 2 * k + p + len(name)) if here else None for k, (c, here) in enumerate(zip(cells, pic))]
            for p, pic in enumerate(present)]


_want = {}


def layout_want(name):
    """the restatement's frames of a layout, computed once"""
    if name not in _want:
        w, h, fill, cells, _ = LAYOUTS[name]
        _want[name] = [em.compose(cells, fr, w, h, fill) for fr in layout_frames(name)]
    return _want[name]


def sweep(n=160, seed=77, side=96):
    """seeded layouts: (w, h, fill, [cells], [present]) -- 1 to 6 cells, sides at most `side`, cells anywhere (so they overlap),
    every third flush with the right edge, every third with the bottom edge, one cell in five absent"""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(n):
        w, h = int(rng.integers(1, side + 1)), int(rng.integers(1, side + 1))
        cells, present = [], []
        for c in range(int(rng.integers(1, 7))):
            sw, sh = int(rng.integers(1, side + 1)), int(rng.integers(1, side + 1))
            crop = None
            if (k + c) % 2:
                cx, cy = 2 * int(rng.integers(0, (sw + 1) // 2)), 2 * int(rng.integers(0, (sh + 1) // 2))
                crop = (cx, cy, int(rng.integers(1, sw - cx + 1)), int(rng.integers(1, sh - cy + 1)))
            x, y = 2 * int(rng.integers(0, (w + 1) // 2)), 2 * int(rng.integers(0, (h + 1) // 2))
            cw = w - x if (k + c) % 3 == 0 else int(rng.integers(1, w - x + 1))
            ch = h - y if (k + c) % 3 == 1 else int(rng.integers(1, h - y + 1))
            cells.append((sw, sh, crop, int(rng.integers(0, 2)), x, y, cw, ch))
            present.append(int(rng.integers(0, 5)) != 0)
        out.append((w, h, tuple(int(v) for v in rng.integers(0, 256, 3)), cells, present))
    return out
