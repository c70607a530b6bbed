"""The encoder's mosaic input without a GPU: enc_mosaic.h -- the layout check, the plan, the table and the tile walk that
k_enc_mosaic (encode.hip) runs -- compiled by g++ into a TEST-ONLY simulator (tests/sim/sim_encode_mosaic.cpp) that pastes
pixel by pixel, held bit for bit against the numpy restatement (tests/enc_mosaic_ref.py), which pastes
enc_scale_ref.scaled_planes and shares nothing with the header."""
import ctypes

import numpy as np
import pytest

import enc_mosaic_inputs as mi
import enc_mosaic_ref as em
import enc_scale_inputs as si
import enc_scale_ref as es


def planes(frame, width, height):
    """the display parts of a frame: (luma, Cr, Cb)"""
    y, cr, cb = es.source_planes(frame, width, height)
    hw, hh = (width + 1) >> 1, (height + 1) >> 1
    return y[:height, :width], cr[:hh, :hw], cb[:hh, :hw]


@pytest.mark.parametrize("name", sorted(mi.LAYOUTS))
def test_named_layouts_simulator_equals_restatement(name):
    w, h, fill, cells, _ = mi.LAYOUTS[name]
    for k, (fr, want) in enumerate(zip(mi.layout_frames(name), mi.layout_want(name))):
        got = mi.sim_frame(cells, fr, w, h, fill)
        assert got is not None and np.array_equal(got, want), (name, k)
    rc, plan = mi.plan_check(cells, w, h, fill)
    assert rc == 0 and plan["words"] <= plan["bound"] and plan["rows"] >= 4, (rc, plan)


def test_cells_of_the_largest_ratios_simulator_equals_restatement():
    """cells 1 and 2 pixels wide from sources 3120 and 3418 wide: their horizontal weights take enc_scale.h's second form (the
    first form's remainder tap would be negative there); the device runs the same layout in tests/test_gpu_encode_scale_edges.py"""
    w, h, fill, cells, _ = mi.RATIO_LAYOUT
    assert all(c[4] % 2 == 0 and c[6] in (1, 2) for c in cells[1:])
    assert all(si.axis_scan(c[0], c[6], 1)[3] == c[6] for c in cells[1:]), "every output column of these cells is on the second form"
    for k, fr in enumerate(mi.ratio_layout_frames()):
        got, want = mi.sim_frame(cells, fr, w, h, fill), em.compose(cells, fr, w, h, fill)
        assert got is not None and np.array_equal(got, want), k
        y = planes(want, w, h)[0]
        assert k == 1 or not np.array_equal(y[10:19, 22], planes(em.compose(cells[:1], fr[:1], w, h, fill), w, h)[0][10:19, 22]), "the cell is seen"
    rc, plan = mi.plan_check(cells, w, h, fill)
    assert rc == 0 and plan["words"] <= plan["bound"] and plan["rows"] >= 4, (rc, plan)


def test_the_named_wall_is_what_the_kernel_test_counts_on():
    w, h, fill, cells, present = mi.LAYOUTS["1_wall_273x71"]
    rc, plan = mi.plan_check(cells, w, h, fill)
    assert es.coded(w, h) == (288, 80) and plan["tiles"] == 3 * 3 + 2 * 2 * 2 and plan["rows"] == 32
    assert plan["rows"] < 288 * 32 // 66, "cell A needs more source rows per tile than a chunk holds"
    y = planes(mi.layout_want("1_wall_273x71")[0], w, h)[0]
    assert np.all(y[70] == fill[0]) and not np.all(y[69] == fill[0])
    assert present[1] == (1, 0, 1)


def test_sweep_simulator_equals_restatement_and_the_table_stays_below_its_bound():
    layouts = mi.sweep()
    assert len(layouts) >= 150
    seen = dict(overlap=0, absent=0, right=0, bottom=0, cells=set())
    for n, (w, h, fill, cells, present) in enumerate(layouts):
        assert 1 <= len(cells) <= 6 and max(w, h) <= 96
        frames = [mi.source_frame(c[0], c[1], n + k) if here else None for k, (c, here) in enumerate(zip(cells, present))]
        got = mi.sim_frame(cells, frames, w, h, fill)
        assert got is not None and np.array_equal(got, em.compose(cells, frames, w, h, fill)), (n, layouts[n])
        rc, plan = mi.plan_check(cells, w, h, fill)
        assert rc == 0 and plan["words"] <= plan["bound"], (layouts[n], rc, plan)
        seen["cells"].add(len(cells))
        seen["absent"] += not all(present)
        seen["right"] += any(c[4] + c[6] == w for c in cells)
        seen["bottom"] += any(c[5] + c[7] == h for c in cells)
        seen["overlap"] += any(a[4] < b[4] + b[6] and b[4] < a[4] + a[6] and a[5] < b[5] + b[7] and b[5] < a[5] + a[7]
                               for i, a in enumerate(cells) for b in cells[:i])
    assert seen["cells"] == {1, 2, 3, 4, 5, 6} and min(seen["overlap"], seen["absent"], seen["right"], seen["bottom"]) >= 20, seen


@pytest.mark.parametrize("name", si.SMALL)
def test_one_whole_picture_cell_is_the_scaled_frame(name):
    w, h, crop, ow, oh, aa = si.CASES[name]
    for f, want in zip(si.case_frames(name), si.case_want(name)):
        cells = [(w, h, crop, aa, 0, 0, ow, oh)]
        assert np.array_equal(mi.sim_frame(cells, [f], ow, oh), want), name
        assert np.array_equal(em.compose(cells, [f], ow, oh), want), name


def test_swapping_two_overlapping_cells_changes_exactly_the_overlap():
    w, h = 90, 70
    a, b = (64, 48, None, 1, 10, 6, 51, 41), (176, 144, None, 1, 40, 30, 45, 37)
    fa, fb = mi.source_frame(64, 48, 2), mi.source_frame(176, 144, 4)            # noise both
    ab, ba = mi.sim_frame([a, b], [fa, fb], w, h), mi.sim_frame([b, a], [fb, fa], w, h)
    only_a, only_b = mi.sim_frame([a], [fa], w, h), mi.sim_frame([b], [fb], w, h)
    for i, (pab, pba, pa, pb) in enumerate(zip(planes(ab, w, h), planes(ba, w, h), planes(only_a, w, h), planes(only_b, w, h))):
        # the overlap in this plane: luma x 40 .. 60, y 30 .. 46; chroma x 20 .. 30 (a: 5 + 26, b from 20), y 15 .. 23
        x0, x1, y0, y1 = (40, 61, 30, 47) if i == 0 else (20, 31, 15, 24)
        inside = np.zeros(pab.shape, bool)
        inside[y0:y1, x0:x1] = True
        assert np.array_equal(pab[~inside], pba[~inside])
        assert np.array_equal(pab[inside], pb[inside]) and np.array_equal(pba[inside], pa[inside])
        assert np.count_nonzero(pab[inside] != pba[inside]) > inside.sum() * 0.5           # (two independent contents agree on few samples)


def test_an_absent_cell_shows_what_is_under_it_and_all_absent_is_the_fill():
    w, h, fill = 90, 70, (200, 30, 77)
    a, b = (64, 48, None, 1, 10, 6, 51, 41), (176, 144, None, 0, 40, 30, 45, 37)
    fa, fb = mi.source_frame(64, 48, 2), mi.source_frame(176, 144, 4)
    assert np.array_equal(mi.sim_frame([a, b], [fa, None], w, h, fill), mi.sim_frame([a], [fa], w, h, fill))
    assert np.array_equal(mi.sim_frame([a, b], [None, fb], w, h, fill), mi.sim_frame([b], [fb], w, h, fill))
    got = mi.sim_frame([a, b], [None, None], w, h, fill)
    cw, ch = es.coded(w, h)
    n = cw * ch
    assert got.size == n * 3 // 2 and np.all(got[:n] == 200) and np.all(got[n:n + n // 4] == 30) and np.all(got[n + n // 4:] == 77)
    assert np.array_equal(got, em.compose([a, b], [None, None], w, h, fill))


def test_table_bound_at_the_extremes():
    wall = [(4095, 4095 if c & 1 else 16, None, 1, (c % 8) * 64, (c // 8) * 36, 64, 36) for c in range(64)]
    rc, plan = mi.plan_check(wall, 512, 288)
    assert rc == 0 and plan["words"] <= plan["bound"] and plan["rows"] >= 4, (rc, plan)
    rc, plan = mi.plan_check([(4095, 4095, None, 1, 510, 286, 1, 1)], 512, 288)
    assert rc == 0 and plan["words"] <= plan["bound"] and plan["rows"] >= 4, (rc, plan)
    rc, plan = mi.plan_check([(4095, 4095, None, 1, 0, 0, 1, 1)], 1, 1)
    assert rc == 0 and plan["words"] <= plan["bound"], (rc, plan)
    rc, plan = mi.plan_check([(1, 1, None, 0, 0, 0, 4095, 2800)] * 2, 4095, 2800)
    assert rc == 0 and plan["words"] <= plan["bound"], (rc, plan)


GOOD = (64, 48, None, 1, 0, 0, 32, 24)
REFUSED = [
    (dict(cells=[GOOD] * 65), "a layout has 1 .. 64 cells"),
    (dict(cells=[GOOD], n=65), "a layout has 1 .. 64 cells"),
    (dict(cells=[GOOD, (64, 48, None, 1, 1, 0, 32, 24)]), "cell 1: cell x and y must be even"),
    (dict(cells=[(64, 48, None, 1, 0, 3, 32, 24)]), "cell 0: cell x and y must be even"),
    (dict(cells=[GOOD, GOOD, (64, 48, None, 1, 70, 0, 32, 24)]), "cell 2: cell rectangle outside"),
    (dict(cells=[(64, 48, None, 1, 0, 50, 32, 24)]), "cell 0: cell rectangle outside"),
    (dict(cells=[(64, 48, None, 1, 0xfffffffe, 0, 4, 4)]), "cell 0: cell rectangle outside"),
    (dict(cells=[GOOD, (64, 48, None, 1, 0, 0, 0, 24)]), "cell 1: cell width and height"),
    (dict(cells=[(64, 48, None, 1, 0, 0, 32, 0)]), "cell 0: cell width and height"),
    (dict(cells=[GOOD, GOOD, GOOD, (64, 48, (1, 0, 10, 10), 1, 0, 0, 32, 24)]), "cell 3: crop_x and crop_y must be even"),
    (dict(cells=[GOOD, (0, 48, None, 1, 0, 0, 32, 24)]), "cell 1: source width and height"),
    (dict(cells=[GOOD, (64, 48, None, 2, 0, 0, 32, 24)]), "cell 1: antialias"),
    (dict(cells=[(64, 48, (60, 0, 10, 10), 1, 0, 0, 32, 24)]), "cell 0: crop rectangle outside"),
    (dict(cells=[GOOD], null=True), "null cells"),
    (dict(cells=[GOOD], fill=0x1000000), "fill"),
]


@pytest.mark.parametrize("bad,why", REFUSED)
def test_layout_check_refuses(bad, why):
    msg = mi.check(bad["cells"], 100, 72, bad.get("fill", mi.FILL), bad.get("n"), bad.get("null", False))
    assert msg.startswith(why), msg
    if "n" not in bad and "null" not in bad and "fill" not in bad:
        frames = [mi.source_frame(64, 48, 2)] * len(bad["cells"])
        assert mi.sim_frame(bad["cells"], frames, 100, 72) is None


def test_layout_check_accepts_the_edges():
    for cells in ([GOOD] * 64, [(64, 48, None, 1, 98, 70, 2, 2)], [(64, 48, None, 0, 0, 0, 100, 72)], [(4095, 1, None, 1, 98, 0, 1, 72)]):
        assert mi.check(cells, 100, 72) == "", cells
    assert mi.check([GOOD], 100, 72, (255, 255, 255)) == ""


def test_library_exports_struct_size_and_kernel_resources():
    from jsmpeg_amd import build, encode, live
    lib = ctypes.CDLL(build.LIB_HIP)
    for name in ("jsmpeg_hip_encoder_set_mosaic", "jsmpeg_hip_encoder_encode_mosaic"):
        assert name in encode.SYMBOLS and hasattr(lib, name), name
    assert "jsmpeg_hip_live_latest_frames" in live.LIVE_SYMBOLS and hasattr(lib, "jsmpeg_hip_live_latest_frames")
    assert ctypes.sizeof(encode.EncCell) == ctypes.sizeof(mi.Cell) == mi.sim().sim_em_sizeof_cell() == 44
    usage = build.check_kernel_resources()
    mine = [v for k, v in usage.items() if "k_enc_mosaic" in k]
    assert len(mine) == 1 and mine[0]["ScratchSize"] == 0 and mine[0]["LDS Size"] <= 29 * 1024, mine
    # both kernels keep four wavefronts per SIMD: at most 128 VGPRs (what the compiler makes of that budget in k_enc_mosaic's
    # horizontal pass: profiles/enc_mosaic_notes.md)
    assert mine[0]["VGPRs"] <= 128 and mine[0]["Occupancy"] >= 4, mine
    # k_enc_scale beside it shares nothing with k_enc_mosaic: its LDS is what its own arrays add up to, as before (the notes
    # hold its register count against the parent's once; a compiler's choice is not pinned here)
    scale = [v for k, v in usage.items() if "k_enc_scale" in k]
    assert len(scale) == 1 and scale[0]["LDS Size"] == 24832 and scale[0]["ScratchSize"] == 0 and scale[0]["VGPRs"] <= 128, scale


def test_grid_is_a_regular_wall():
    from jsmpeg_amd import encode
    cells = encode.grid(4, 4, (1920, 1080), (1920, 1080))
    assert len(cells) == 16 and [(c.x, c.y, c.width, c.height) for c in cells[:5]] == [(0, 0, 480, 270), (480, 0, 480, 270), (960, 0, 480, 270),
                                                                                   (1440, 0, 480, 270), (0, 270, 480, 270)]
    assert all(c.source.width == 1920 and c.source.height == 1080 and c.source.antialias == 1 and c.source.crop_width == 0 for c in cells)
    cells = encode.grid(3, 2, (273, 71), (64, 48), gap=3, crop=(2, 4, 30, 20), antialias=False)
    as_tuples = [(c.source.width, c.source.height, (c.source.crop_x, c.source.crop_y, c.source.crop_width, c.source.crop_height),
                  c.source.antialias, c.x, c.y, c.width, c.height) for c in cells]
    assert [t[4:] for t in as_tuples] == [(0, 0, 88, 32), (92, 0, 88, 32), (184, 0, 88, 32), (0, 36, 88, 32), (92, 36, 88, 32), (184, 36, 88, 32)]
    assert as_tuples[0][:4] == (64, 48, (2, 4, 30, 20), 0) and mi.check(as_tuples, 273, 71) == ""
    for cols, rows in ((200, 1), (0, 1), (1, 0)):
        with pytest.raises(ValueError):
            encode.grid(cols, rows, (273, 71), (64, 48))


def test_sanitizers_on_the_rule_and_the_plan():
    """enc_mosaic.h's functions and the simulator around them as a stand-alone program (its own main, g++
    -fsanitize=address,undefined): a sweep of layouts with every frame in a buffer of exactly its size; nothing is loaded
    into python"""
    import glob
    import os
    import subprocess
    sim_dir = os.path.join(mi.ROOT, "tests", "sim")
    out_dir = os.path.join(sim_dir, "_asan")
    os.makedirs(out_dir, exist_ok=True)
    exe, src = os.path.join(out_dir, "sim_mosaic_main"), os.path.join(sim_dir, "sim_encode_mosaic.cpp")
    deps = [src, __file__] + glob.glob(os.path.join(mi.ei.CSRC, "*.h"))
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DSIM_EM_MAIN",
                               "-Wall", "-Wno-unknown-pragmas", "-I", mi.ei.CSRC, "-I", os.path.join(mi.ROOT, "include"), "-o", exe, src])
    r = subprocess.run([exe, "150"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-3000:]
    assert "150 layouts and the largest plans are clean" in r.stdout
