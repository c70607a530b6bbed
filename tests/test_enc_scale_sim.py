"""The encoder's scaled input without a GPU: enc_scale.h -- the taps, the weights, the roundings, the descriptor check and the
launch plan that k_enc_scale (encode.hip) runs -- compiled by g++ into a TEST-ONLY simulator (tests/sim/sim_encode_scale.cpp)
and held bit for bit against the numpy restatement (tests/enc_scale_ref.py), and the restatement against torch's CPU
F.interpolate."""
import ctypes

import numpy as np
import pytest

import enc_scale_inputs as si
import enc_scale_ref as es

# |restatement - torch's unrounded float| <= 0.5 + E on the named cases.  Measured worst excess over 0.5: 0.00620 (case
# 7; ties in the rounding plus the 14-bit weights); doubled and rounded up.  profiles/enc_scale_notes.md; the issue's ceiling is 0.05.
E = 0.0125


@pytest.mark.parametrize("name", sorted(si.CASES))
def test_named_cases_simulator_equals_restatement(name):
    w, h, crop, ow, oh, aa = si.CASES[name]
    for k, (f, want) in enumerate(zip(si.case_frames(name), si.case_want(name))):
        got = si.sim_frame(f, w, h, ow, oh, crop, aa)
        assert got is not None and np.array_equal(got, want), (name, k)


def test_sweep_simulator_equals_restatement_and_tap_properties():
    geos = si.sweep()
    assert len(geos) >= 200
    kinds = set()
    for n, (w, h, crop, ow, oh, aa) in enumerate(geos):
        f = si.ei.noise_frame(w, h, seed=n)
        got = si.sim_frame(f, w, h, ow, oh, crop, aa)
        assert got is not None and np.array_equal(got, es.scale_frame(f, w, h, ow, oh, crop, bool(aa))), geos[n]
        rc, plan = si.plan_check(w, h, ow, oh, crop, aa)
        assert rc == 0 and plan["words"] <= plan["bound"], (geos[n], rc, plan)
        cw, ch = (crop[2], crop[3]) if crop else (w, h)
        for n_in, n_out in ((cw, ow), (ch, oh), ((cw + 1) >> 1, (ow + 1) >> 1), ((ch + 1) >> 1, (oh + 1) >> 1)):
            kinds.add((n_in > n_out) - (n_in < n_out))
            want = es.axis_taps(n_in, n_out, aa)
            last_min = last_end = 0
            for i in range(n_out):
                xmin, wts = si.sim_taps(n_in, n_out, aa, i)
                assert (xmin, wts) == want[i], (n_in, n_out, aa, i)
                assert min(wts) >= 0 and sum(wts) == es.ONE
                assert 0 <= xmin and xmin + len(wts) <= n_in                     # contiguous by construction, inside the crop
                assert xmin >= last_min and xmin + len(wts) >= last_end
                last_min, last_end = xmin, xmin + len(wts)
    assert kinds == {-1, 0, 1}


def test_equal_size_is_a_copy_and_a_crop_a_cut_out():
    w, h = 177, 145
    f = si.ei.noise_frame(w, h, seed=4)
    Y, Cr, Cb = es.source_planes(f, w, h)
    for aa in (0, 1):
        y, cr, cb = es.source_planes(si.sim_frame(f, w, h, w, h, None, aa), w, h)
        assert np.array_equal(y[:h, :w], Y[:h, :w]) and np.array_equal(cr[:73, :89], Cr[:73, :89]) and np.array_equal(cb[:73, :89], Cb[:73, :89])
        assert np.all(y[:h, w:] == Y[:h, w - 1:w]) and np.all(y[h:, :w] == Y[h - 1:h, :w]) and np.all(cr[73:, 89:] == Cr[72, 88])
        x0, y0, cw, ch = 34, 6, 63, 41
        y, cr, cb = es.source_planes(si.sim_frame(f, w, h, cw, ch, (x0, y0, cw, ch), aa), cw, ch)
        assert np.array_equal(y[:ch, :cw], Y[y0:y0 + ch, x0:x0 + cw])
        assert np.array_equal(cr[:21, :32], Cr[3:24, 17:49]) and np.array_equal(cb[:21, :32], Cb[3:24, 17:49])


@pytest.mark.parametrize("name", sorted(si.CASES))
def test_restatement_is_close_to_torch(name):
    import torch
    import torch.nn.functional as F
    w, h, crop, ow, oh, aa = si.CASES[name]
    worst = 0.0
    for f in si.case_frames(name):
        ins = es.crops(f, w, h, crop)
        outs = es.scaled_planes(f, w, h, ow, oh, crop, bool(aa))
        for p, got in zip(ins, outs):
            if got.shape[1] == 1 and got.shape[0] != p.shape[0]:
                continue            # torch's 2-D antialiased CPU kernel is wrong for one output column and a changed height (tests/tensor_ref.py)
            x = torch.from_numpy(np.ascontiguousarray(p)).float()[None, None]
            if got.shape == p.shape:
                want = x[0, 0].numpy()
            else:
                want = F.interpolate(x, size=got.shape, mode="bilinear", align_corners=False, antialias=bool(aa))[0, 0].numpy()
            worst = max(worst, float(np.abs(got.astype(np.float64) - want.astype(np.float64)).max()))
    print("%s: worst |integer - torch float| = %.5f" % (name, worst))
    assert worst <= 0.5 + E, (name, worst)


REFUSED = [
    (dict(width=0), "width"), (dict(height=0), "width"), (dict(width=4096), "width"), (dict(height=4096), "width"),
    (dict(crop=(1900, 0, 100, 100)), "crop"), (dict(crop=(0, 1000, 100, 100)), "crop"), (dict(crop=(0, 0, 100, 0)), "crop"),
    (dict(crop=(0, 0, 0, 100)), "crop"), (dict(crop=(4, 4, 0, 0)), "crop"), (dict(crop=(0xfffffffe, 0, 4, 4)), "crop"),
    (dict(crop=(1, 0, 100, 100)), "even"), (dict(crop=(0, 3, 100, 100)), "even"), (dict(aa=2), "antialias"),
]


@pytest.mark.parametrize("bad,why", REFUSED)
def test_descriptor_check_refuses(bad, why):
    kw = dict(width=1920, height=1080, crop=None, aa=1)
    kw.update(bad)
    s = si.source(kw["width"], kw["height"], kw["crop"], kw["aa"])
    msg = si.sim().sim_es_check(ctypes.byref(s)).decode()
    assert msg and why in msg, msg
    out = np.zeros(16 * 16 * 3 // 2, np.uint8)
    assert si.sim().sim_es_frame(out.ctypes.data, ctypes.byref(s), 16, 16, out.ctypes.data) == -1
    assert si.sim().sim_es_check(None).decode()


def test_descriptor_check_accepts_the_edges():
    for kw in (dict(width=1920, height=1080, crop=(1918, 1078, 2, 2)), dict(width=1920, height=1080, crop=(100, 200, 1820, 880)),
               dict(width=4095, height=1), dict(width=1, height=4095), dict(width=1919, height=1079, crop=(0, 0, 1919, 1079), aa=0)):
        s = si.source(kw["width"], kw["height"], kw.get("crop"), kw.get("aa", 1))
        assert si.sim().sim_es_check(ctypes.byref(s)).decode() == "", kw
    # 4095-wide sources and output 1 x 1 run: the plan holds, the values are the restatement's
    f = si.ei.noise_frame(4095, 3, seed=9)
    assert np.array_equal(si.sim_frame(f, 4095, 3, 1, 1), es.scale_frame(f, 4095, 3, 1, 1))
    assert np.array_equal(si.sim_frame(f, 4095, 3, 70, 2, (2, 0, 4093, 3), 0), es.scale_frame(f, 4095, 3, 70, 2, (2, 0, 4093, 3), False))
    for geo in ((4095, 3, 1, 1), (4095, 4095, 1, 1), (1, 1, 4095, 2800), (4095, 4095, 4095, 2800), (4095, 16, 4094, 16)):
        rc, plan = si.plan_check(*geo)
        assert rc == 0 and plan["rows"] >= 4, (geo, rc, plan)


@pytest.mark.parametrize("name", sorted(si.CASES))
def test_launch_plan_of_the_named_cases(name):
    w, h, crop, ow, oh, aa = si.CASES[name]
    rc, plan = si.plan_check(w, h, ow, oh, crop, aa)
    assert rc == 0 and plan["words"] <= plan["bound"] and plan["rows"] >= 4, (rc, plan)
    if name.startswith("5"):
        assert plan["rows"] < 360, "more than one chunk of source rows per tile"


def test_library_exports_and_kernel_resources():
    from jsmpeg_amd import build, encode
    lib = ctypes.CDLL(build.LIB_HIP)
    for name in ("jsmpeg_hip_encoder_encode_scaled", "jsmpeg_hip_encoder_source"):
        assert name in encode.SYMBOLS and hasattr(lib, name), name
    assert ctypes.sizeof(encode.EncSource) == ctypes.sizeof(si.Source) == 28


def test_sanitizers_on_the_rule_and_the_plan():
    """enc_scale.h's functions and the simulator around them as a stand-alone program (its own main, g++
    -fsanitize=address,undefined): a sweep of geometries with the frames in buffers of exactly their size"""
    import glob
    import os
    import subprocess
    sim_dir = os.path.join(si.ROOT, "tests", "sim")
    out_dir = os.path.join(sim_dir, "_asan")
    os.makedirs(out_dir, exist_ok=True)
    exe, src = os.path.join(out_dir, "sim_scale_main"), os.path.join(sim_dir, "sim_encode_scale.cpp")
    deps = [src, __file__] + glob.glob(os.path.join(si.ei.CSRC, "*.h"))
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DSIM_ES_MAIN",
                               "-Wall", "-Wno-unknown-pragmas", "-I", si.ei.CSRC, "-I", os.path.join(si.ROOT, "include"), "-o", exe, src])
    r = subprocess.run([exe, "150"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-3000:]
    assert "150 geometries and the largest plans are clean" in r.stdout
