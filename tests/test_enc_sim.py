"""The intra encoder (C ABI part 8) without a GPU: enc_block.h's device functions compiled by g++ (tests/sim/sim_encode_pass.cpp)
and driven in the kernels' two-pass order.  Every stream is read by the reference's decoder (its restatement, and its own C
where present) and by tests/sim's decoder, equals tests/enc_ref.py's independent restatement byte for byte, and its
quantiser is held against a float64 transform with bounds measured by tools/enc_quality.py (profiles/enc_bounds.json)."""
import ctypes
import json
import os

import numpy as np
import pytest

import enc_inputs as ei
import enc_ref
from conftest import ROOT
from jsmpeg_amd import cabi, spec_tables

SCALES = (1, 2, 8, 31)


class GopUnit(ctypes.Structure):
    _fields_ = [("offset", ctypes.c_uint64), ("bytes", ctypes.c_uint64), ("pictures", ctypes.c_uint32), ("needs_header", ctypes.c_uint32)]


@pytest.fixture(scope="module")
def cases(libs):
    return ei.small_cases(libs)


@pytest.fixture(scope="module")
def hd(libs):
    return ei.content_frames(1920, 1080, 2)


def sim_decode(es, w, h, n):
    """tests/sim's decoder (the decode path's own device functions on the CPU)"""
    import glob
    import subprocess
    so = os.path.join(ROOT, "tests", "sim", "libjsmpeg_sim.so")
    src = os.path.join(ROOT, "tests", "sim", "sim_decode.cpp")
    csrc = os.path.join(ROOT, "jsmpeg_amd", "csrc")
    deps = [src] + glob.glob(os.path.join(csrc, "*.h"))
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-Wno-unknown-pragmas", "-I", csrc, "-o", so, src])
    lib = ctypes.CDLL(so)
    lib.sim_decode_stream.restype = ctypes.c_int
    lib.sim_decode_stream.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_int]
    cw, ch = enc_ref.coded(w, h)
    fb = cw * ch * 3 // 2
    out = np.zeros(n * fb, dtype=np.uint8)
    es = np.ascontiguousarray(es)
    assert lib.sim_decode_stream(es.ctypes.data, len(es), w, h, out.ctypes.data, n) == n
    return out.reshape(n, fb)


def check_stream(libs, hip_lib, result, frames, w, h, streams, end, rate=30.0, with_sim_decoder=True):
    """1. of the issue: the reference reads every stream of the call"""
    buf, ranges, sr = result
    cw, ch = enc_ref.coded(w, h)
    n = len(frames)
    streams = [0] * n if streams is None else list(streams)
    assert ei.start_codes(buf) == n * (3 + ch // 16) + (len(sr) if end else 0)         # nothing emulated inside a slice
    raw = np.frombuffer(buf, dtype=np.uint8)
    inside = np.zeros(len(raw), bool)
    for s, (b, e) in sr.items():
        assert b % 16 == 0 and b >= 16
        inside[b:e] = True
    assert np.all(raw[~inside] == 0xff)
    L = ctypes.CDLL(hip_lib)
    L.jsmpeg_hip_split_gops.restype = ctypes.c_int
    for s, (b, e) in sr.items():
        es = raw[b:e]
        mine = [k for k in range(n) if streams[k] == s]
        dec, _, info = cabi.decode_stream(libs["oracle"], es, keep="planes")
        assert len(dec) == len(mine)
        assert (info["width"], info["height"], info["frame_rate"]) == (w, h, rate)
        for k in mine:
            o = ranges[k][0]
            assert bytes(raw[o + 20:o + 24]) == b"\x00\x00\x01\x00" and (raw[o + 25] >> 3) & 7 == 1      # picture_coding_type I
        if libs.get("ref"):
            ref, _, _ = cabi.decode_stream(libs["ref"], es, keep="planes")
            assert len(ref) == len(dec)
            for a, c in zip(ref, dec):
                assert all(np.array_equal(x, y) for x, y in zip(a, c))
        if with_sim_decoder:
            got = sim_decode(es, w, h, len(mine))
            for a, c in zip(got, dec):
                assert np.array_equal(a, np.concatenate(c))
        units = (GopUnit * (len(mine) + 2))()
        ho, hb = ctypes.c_uint64(), ctypes.c_uint64()
        nu = L.jsmpeg_hip_split_gops(ctypes.c_void_p(es.ctypes.data), ctypes.c_uint64(len(es)), units, ctypes.c_uint32(len(mine) + 2),
                                     ctypes.byref(ho), ctypes.byref(hb))
        assert nu == len(mine)
        for u, k in zip(units, mine):
            tail = 4 if end and k == mine[-1] else 0
            assert (u.offset + b, u.bytes - tail, u.pictures) == (ranges[k][0], ranges[k][1], 1)
    return True


@pytest.mark.parametrize("q", SCALES)
def test_small_inputs(libs, hip_lib, cases, q):
    """decodes by the reference, byte-exact against the restatement"""
    for name, (frames, w, h) in cases.items():
        got = ei.sim_encode(frames, w, h, qscale=q)
        check_stream(libs, hip_lib, got, frames, w, h, None, True)
        assert got == enc_ref.encode(frames, w, h, qscale=q), name


def test_per_picture_scales_streams_and_flags(libs, hip_lib, cases):
    frames, w, h = cases["enc_pan_176x144"]
    frames = frames + cases["content_176x144"][0]
    streams, qs = [0, 0, 2, 3, 3], [1, 31, 8, 2, 5]
    for end in (True, False):
        for rate_code, rate in ((5, 30.0), (3, 25.0)):
            got = ei.sim_encode(frames, w, h, streams=streams, qscale=qs, frame_rate_code=rate_code, end=end, max_streams=5)
            assert got == enc_ref.encode(frames, w, h, streams=streams, qscale=qs, frame_rate_code=rate_code, end=end)
            check_stream(libs, hip_lib, got, frames, w, h, streams, end, rate)
    # the bytes of a picture do not depend on the call it is in: its range in a call of one
    got = ei.sim_encode(frames, w, h, streams=streams, qscale=qs, max_streams=5)
    for k in range(len(frames)):
        one = ei.sim_encode(frames[k:k + 1], w, h, qscale=qs[k])
        a, b = got[1][k], one[1][0]
        ordinal = 1 if k in (1, 4) else 0
        x, y = bytearray(got[0][a[0]:a[0] + a[1]]), bytearray(one[0][b[0]:b[0] + b[1]])
        assert x[:16] == y[:16] and x[20:] == y[20:]                  # all but the GOP header's time code
        bits = int.from_bytes(x[16:20], "big")
        assert ((bits >> 13) & 63, (bits >> 7) & 63) == (0, ordinal)


def test_time_code_counts_pictures_of_a_stream(libs):
    frames = [ei.flat_frame(16, 16, 7)] * 62
    buf, ranges, _ = ei.sim_encode(frames, 16, 16, qscale=4)
    for k, (o, _) in enumerate(ranges):
        bits = int.from_bytes(buf[o + 16:o + 20], "big")
        assert bits >> 31 == 0 and (bits >> 19) & 1 == 1 and (bits >> 6) & 1 == 1      # drop_frame 0, marker, closed_gop
        assert ((bits >> 13) & 63, (bits >> 7) & 63) == (k // 30, k % 30)


def test_1080p_pair(libs, hip_lib, hd):
    got = ei.sim_encode(hd, 1920, 1080, qscale=8)
    check_stream(libs, hip_lib, got, hd, 1920, 1080, None, True)
    assert got == enc_ref.encode(hd, 1920, 1080, qscale=8)


def test_noise_at_q1_worst_case_size(libs, hip_lib):
    """uniform noise at q = 1: clamped levels, the largest macroblocks there are; held to: decodes, byte-exact, no level off by more than 1"""
    w, h = 64, 48
    frames = [ei.noise_frame(w, h, 1), ei.noise_frame(w, h, 2)]
    got = ei.sim_encode(frames, w, h, qscale=1)
    check_stream(libs, hip_lib, got, frames, w, h, None, True)
    assert got == enc_ref.encode(frames, w, h, qscale=1)
    for f in frames:
        a, b = ei.sim_levels(f, w, h, 1), enc_ref.frame_levels(f, w, h, 1, exact_float=True)
        assert np.abs(a - b).max() <= 1
        assert a.min() >= -255 and a.max() <= 255
    assert len(got[0]) > 2 * w * h * 3 // 2                              # more bytes than the pictures themselves


def test_overflow_is_reported_not_written():
    frames = [ei.noise_frame(64, 48, 1)]
    need = len(ei.sim_encode(frames, 64, 48, qscale=1)[0])
    assert ei.sim_encode(frames, 64, 48, qscale=1, cap=need) is not None
    assert ei.sim_encode(frames, 64, 48, qscale=1, cap=need - 1) is None


def test_quantiser_against_a_float64_transform(libs, cases, hd):
    """3. of the issue.  Derived: no level differs by more than 1 (2 would need a transform error of a whole quantiser step;
    the integer transform's is below 1/16 of the smallest one -- three fractional bits, q W >= 8).  Measured
    (tools/enc_quality.py, profiles/enc_bounds.json, the figures in profiles/enc_notes.md): the share of differing levels,
    at most twice the measured one; the luma PSNR of decode(stream) short of the float64 encoder's by at most the
    measured gap plus a tenth of it.  Condition: a gap above 0.1 dB at any q >= 2 means the transform is too coarse."""
    bounds = json.load(open(os.path.join(ROOT, "profiles", "enc_bounds.json")))["scales"]
    all_cases = dict(cases)
    all_cases["content_1920x1080"] = (hd, 1920, 1080)
    m = ei.measure_quality(libs, all_cases, SCALES)
    for q in SCALES:
        v, b = m[q], bounds[str(q)]
        print("q %2d: share %.3e (measured %.3e), worst %d, PSNR %.4f against float64 %.4f: gap %+.5f dB (measured %+.5f)" % (
            q, v["share"], b["share"], v["worst"], v["psnr_int"], v["psnr_float"], v["gap_db"], b["gap_db"]))
    for q in SCALES:
        v, b = m[q], bounds[str(q)]
        assert v["worst"] <= 1
        assert v["share"] <= 2 * b["share"]
        assert v["gap_db"] <= b["gap_db"] + 0.1 * abs(b["gap_db"])
        if q >= 2:
            assert b["gap_db"] <= 0.1 and v["gap_db"] <= 0.1


def test_code_table_equals_the_spec_tables():
    """4. of the issue: the encoder's (run, level) table is spec_tables' DCT_COEFF inverted; every pair outside it has no code
    (takes an escape); the DC size tables likewise"""
    T = spec_tables.load()
    tab = np.ctypeslib.as_array(ei.sim().sim_enc_coeff_table(), shape=(32, 41))
    want = np.zeros((32, 41), dtype=np.uint32)
    for bits, (run, level) in T["DCT_COEFF"].items():
        want[run, level] = (len(bits) << 16) | int(bits, 2)
    assert np.array_equal(tab, want)
    assert np.count_nonzero(want) == len(T["DCT_COEFF"]) and not want[:, 0].any() and want[0, 1] == 0
    for chroma, name in ((0, "DCSIZE_LUMA"), (1, "DCSIZE_CHROMA")):
        dc = np.ctypeslib.as_array(ei.sim().sim_enc_dc_table(chroma), shape=(9,))
        assert [int(v) for v in dc] == [(len(b) << 8) | int(b, 2) for b, _ in sorted(T[name].items(), key=lambda kv: kv[1])]


def test_levels_are_in_range_and_escapes_round_trip(libs):
    """level 0 is never coded and |level| <= 255: a picture of every extreme decodes to what the restatement's levels say"""
    f = ei.stripe_frame(64, 48)
    for q in (1, 2):
        lv = ei.sim_levels(f, 64, 48, q)
        assert np.array_equal(lv, enc_ref.frame_levels(f, 64, 48, q))
        assert lv.min() >= -255 and lv.max() <= 255 and lv[:, :, 0].min() >= 0
        mags = np.abs(lv[:, :, 1:])
        assert np.any((mags > 127) & (mags < 255)) or q == 2              # the 16-bit escape forms are in the stream ...
        assert mags.max() == (255 if q == 1 else mags.max()) and np.any(mags > 40)     # ... and at q = 1 the clamp is reached
    dc = ei.sim_levels(f, 64, 48, 8)[:, :, 0]
    assert set(np.unique(dc)) == {0, 128, 255} or {0, 255} <= set(np.unique(dc))     # differentials of +-255


def test_forward_transform_table_and_bounds():
    """the header's cosines are round(2^14 c_k cos((2n + 1) k pi / 16)); the stated bounds hold for them"""
    import re
    text = open(os.path.join(ROOT, "jsmpeg_amd", "csrc", "enc_block.h")).read()
    body = text[text.index("JmEncConst c = {"):text.index("MPEG1_DEFAULT_INTRA_QUANT_INIT, {}")]
    vals = np.array([int(v) for v in re.findall(r"-?\d+", body)], dtype=np.int64).reshape(8, 8)
    assert np.array_equal(vals, enc_ref.COS)
    s = int(np.abs(vals).sum(axis=1).max())
    assert s == 46344 and 255 * s < 1 << 24 and 255 * s * s < 1 << 39


@pytest.mark.parametrize("layout", [0, 1], ids=["nchw", "nhwc"])
@pytest.mark.parametrize("order", [0, 1], ids=["rgb", "bgr"])
@pytest.mark.parametrize("size", [(176, 144), (177, 145), (16, 16), (1, 1)], ids=lambda s: "%dx%d" % s)
def test_rgb_conversion(size, layout, order):
    """k_enc_rgb's body: exactly the restatement's integer form, and within 1 LSB of a float64 JFIF conversion.  Derivation:
    the fixed point's coefficients are each within 2^-17 of the real ones, so before rounding the integer value is within
    3 * 255 * 2^-17 < 0.006 of the real one; both are then rounded to an integer, which can move them apart by at most 1."""
    w, h = size
    rng = np.random.default_rng(w * 7 + layout * 2 + order)
    rgb = rng.integers(0, 256, (3, h, w, 3), dtype=np.uint8)
    rgb[1] = np.where(rng.random((h, w, 3)) < 0.5, 0, 255)            # saturated colours: the chroma clamp
    src = rgb[..., ::-1] if order else rgb
    got = ei.sim_rgb(src.transpose(0, 3, 1, 2) if layout == 0 else src, layout, order)
    cw, ch = enc_ref.coded(w, h)
    for k in range(3):
        assert np.array_equal(got[k], enc_ref.rgb_to_frame(rgb[k]))
        y, cr, cb = enc_ref.rgb_to_frame_float(rgb[k])
        gy, gcr, gcb = enc_ref.planes(got[k], cw, ch)
        for a, b in ((gy, y), (gcr, cr), (gcb, cb)):
            assert np.abs(a.astype(np.float64) - np.clip(np.rint(b), 0, 255)).max() <= 1


def test_rgb_round_trip_through_the_renderer(libs):
    """the conversion is the inverse of the renderer the project matches (canvas2d.js): grey stays grey, primaries come back close"""
    from oracle import checkers
    rgb = np.zeros((16, 16, 3), np.uint8)
    rgb[:, :8] = (200, 30, 60)
    rgb[:, 8:] = (20, 180, 240)
    f = ei.sim_rgb(rgb[None], 1, 0)[0]
    y, cr, cb = enc_ref.planes(f, 16, 16)
    back = checkers.oracle_rgba(libs["oracle"], y.ravel(), cr.ravel(), cb.ravel(), 16, 16)[..., :3]
    assert np.abs(back.astype(int) - rgb.astype(int)).max() <= 3
    grey = np.full((16, 16, 3), 77, np.uint8)
    y, cr, cb = enc_ref.planes(ei.sim_rgb(grey[None], 1, 0)[0], 16, 16)
    assert np.all(y == 77) and np.all(cr == 128) and np.all(cb == 128)


def test_python_module_and_exports(hip_lib):
    from jsmpeg_amd import encode
    lib = ctypes.CDLL(hip_lib)
    for name in encode.SYMBOLS:
        assert hasattr(lib, name), name
    assert ctypes.sizeof(encode.EncoderConfig) == 32


def test_encoder_kernels_use_no_scratch():
    from jsmpeg_amd import build
    usage = build.check_kernel_resources()
    for k in ("k_enc_rgb", "k_enc_measure", "k_enc_scan_slices", "k_enc_scan_pictures", "k_enc_place", "k_enc_clear", "k_enc_write"):
        name = [n for n in usage if k in n]
        assert name, k
        assert usage[name[0]]["ScratchSize"] == 0 and usage[name[0]].get("LDS Size", 0) <= 64 * 1024
