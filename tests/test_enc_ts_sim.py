"""The TS mux's rule (jsmpeg_amd/csrc/enc_ts.h) without a GPU: jsmpeg_hip_ts_mux_host, rewritten on the rule, pinned to the bytes it
wrote before; the simulator of the device mux (tests/sim/sim_enc_ts.cpp: k_ts_plan's walk, then every output dword on its own,
in reverse order) against the host mux, byte for byte, per stream, counters included; the plan's properties; the default PTS
rule; the reference's own demuxer over the simulator's packets; and the simulator's driver under the sanitizers."""
import ctypes
import hashlib
import json
import os
import subprocess
import tempfile

import numpy as np
import pytest

import enc_inputs as ei
import enc_ts_inputs as et
from conftest import ROOT, have_reference
from test_ts_mux import SIZES, units_case


def test_host_mux_is_pinned(hip_lib):
    """(fails without the feature: the pin and enc_ts.h are new; the bytes are the parent commit's)"""
    from jsmpeg_amd import encode
    pin = json.load(open(os.path.join(ROOT, "tests", "golden", "enc_ts_mux_pin.json")))
    assert pin["start"] == 11 and sorted(pin["cases"]) == ["units_case_1", "units_case_4"]
    assert os.path.exists(os.path.join(ROOT, "jsmpeg_amd", "csrc", "enc_ts.h"))
    for seed in (1, 4):
        es, ranges, pts = units_case(seed, SIZES)
        ts, cc = encode.ts_mux(es, ranges, pts, continuity=pin["start"])
        want = pin["cases"]["units_case_%d" % seed]
        assert (hashlib.sha256(ts.tobytes()).hexdigest(), int(ts.size), cc) == (want["sha256"], want["bytes"], want["continuity_out"]), seed


def held(case, where, aligned=False):
    """the simulator's call equals the host mux; returns (the result, the host's bytes)"""
    want = et.host_want(case)
    got = et.sim_mux(case, aligned=aligned)
    assert got.total >= 0, where
    end = et.assert_equals_host(case, got.buf, got.ranges, got.cc, where, want)
    assert end == got.total <= case.bound(), where
    for s in range(case.n_streams):
        if s not in case.present():
            assert got.cc[s] == case.counters()[s], (where, s)         # a stream without units keeps its counter
    return got, want


@pytest.mark.parametrize("aligned", [False, True], ids=["bytes", "aligned_dwords"])
def test_sim_equals_host_on_the_edge_sizes(hip_lib, aligned):
    for seed, cc in ((1, 11), (4, 15)):
        c = et.sizes_case(seed)
        c.cc[0] = cc
        got, _ = held(c, ("sizes", seed), aligned)
        assert [n for _, n, _ in got.units] == [et.sim().sim_ts_packets(b) for b in SIZES]


@pytest.mark.parametrize("aligned", [False, True], ids=["bytes", "aligned_dwords"])
def test_sim_equals_host_on_every_size_1_to_400(hip_lib, aligned):
    c = et.sweep_case()
    assert [b for _, b in c.ranges] == list(range(1, 401)) and all(o % 16 == b % 16 for o, b in c.ranges)
    held(c, "sweep", aligned)
    held(et.three_stream_case(), "three streams", aligned)


def test_sim_equals_the_serial_loop_and_host_on_random_cases(hip_lib):
    cases = et.random_cases()
    assert len(cases) == 300 and any(b > 65527 for c in cases for _, b in c.ranges)
    assert any(len(c.present()) == 5 for c in cases) and any(c.present() != list(range(len(c.present()))) for c in cases)
    for i, c in enumerate(cases):
        got, want = held(c, ("random", i), aligned=bool(i & 1))
        if i % 10 == 0:                                        # and the byte loop the host mux was, kept in the simulator's file
            for s in c.present():
                idx = c.of(s)
                off = np.ascontiguousarray([c.ranges[k][0] for k in idx], dtype=np.uint64)
                ln = np.ascontiguousarray([c.ranges[k][1] for k in idx], dtype=np.uint32)
                p90 = np.ascontiguousarray([c.pts[k] for k in idx], dtype=np.uint64)
                cc = ctypes.c_uint32(c.cc[s])
                out = np.zeros(len(want[s][0]), np.uint8)
                n = et.sim().sim_ts_mux_serial(c.es.ctypes.data, off.ctypes.data, ln.ctypes.data, p90.ctypes.data, len(idx), 0xE0, 0x100,
                                               ctypes.byref(cc), out.ctypes.data)
                assert n == len(out) and out.tobytes() == want[s][0] and cc.value == want[s][1], (i, s)


def test_two_calls_with_carried_counters_equal_one(hip_lib):
    c = et.three_stream_case()
    one = et.sim_mux(c)
    first = [i for s in c.present() for i in c.of(s)[:1 if s != 5 else 2]]
    rest = [i for i in range(len(c.ranges)) if i not in first]
    a = et.sim_mux(c.pick(first))
    b = et.sim_mux(c.pick(rest, cc={s: a.cc[s] for s in c.present()}))
    assert b.cc == one.cc
    for s in c.present():
        (ab, ae), (bb, be), (ob, oe) = a.ranges[s], b.ranges[s], one.ranges[s]
        assert bytes(a.buf[ab:ae]) + bytes(b.buf[bb:be]) == bytes(one.buf[ob:oe]), s


def test_plan_properties(hip_lib):
    for i, c in enumerate([et.sizes_case(), et.sweep_case(), et.three_stream_case()] + et.random_cases(60, seed=77)):
        got = et.sim_mux(c)
        need, at = got.total, 0
        assert 0 < need <= c.bound(), i
        for s in c.present():
            b, e = got.ranges[s]
            assert b % 16 == 0 and b >= at and e > b and (e - b) % 188 == 0, (i, s)
            at = e
        # the units' packets tile their stream's range, the counters go on from unit to unit
        for s in c.present():
            pos, cc = got.ranges[s][0], c.cc[s]
            for k in c.of(s):
                u_at, packets, u_cc = got.units[k]
                assert (u_at, u_cc) == (pos, cc) and packets == et.sim().sim_ts_packets(c.ranges[k][1]), (i, k)
                pos, cc = pos + 188 * packets, (cc + packets) & 15
            assert pos == got.ranges[s][1] and cc == got.cc[s], (i, s)
        short = et.sim_mux(c, cap=need - 1)
        assert short.total == -1 and short.cc == c.counters(), i       # overflow: the counters stay
        assert np.all(short.buf == 0xA5), i                            # and nothing is written
        exact = et.sim_mux(c, cap=need)
        assert exact.total == need and bytes(exact.buf) == bytes(got.buf[:need]), i


def test_ts_bound_module_function(hip_lib):
    from jsmpeg_amd import encode
    for args in ((0, 0, 1), (1, 1, 1), (65528, 1, 1), (1 << 33, 4000, 64)):
        assert encode.ts_bound(*args) == et.sim().sim_ts_bound(*args) == 188 * (args[0] // 184 + 2 * args[1]) + 15 * args[2]


def test_default_pts_rule():
    from jsmpeg_amd import encode
    rng = np.random.default_rng(5)
    ordinals = [0, 1, 2, 29, 30, 1000, 1001, 95443, 95444, (1 << 31) - 1, 1 << 31, (1 << 32) - 2, (1 << 32) - 1] + [int(v) for v in rng.integers(0, 1 << 32, 200)]
    for code in range(1, 9):
        num, den = encode.FRAME_RATES[code]
        for o in ordinals:
            assert et.sim().sim_ts_default_pts(o, code) == (o * 90000 * den // num) & ((1 << 33) - 1), (code, o)
    assert et.sim().sim_ts_default_pts(1 << 31, 8) != ((1 << 31) * 90000 // 60)          # the mask is at work


@pytest.mark.reference
@pytest.mark.skipif(not have_reference(), reason="needs the reference tree")
def test_reference_ts_js_gives_back_every_unit_of_every_stream(hip_lib):
    c = et.three_stream_case()
    got = et.sim_mux(c)
    for s in c.present():
        b, e = got.ranges[s]
        with tempfile.NamedTemporaryFile(suffix=".ts", delete=False) as f:
            f.write(bytes(got.buf[b:e]))
        try:
            ref = json.loads(subprocess.check_output(["node", os.path.join(ROOT, "oracle", "ref_node_ts.js"), f.name, "224"]))
        finally:
            os.unlink(f.name)
        idx = c.of(s)
        assert len(ref["writes"]) == len(idx), s
        for w, k in zip(ref["writes"], idx):
            o, n = c.ranges[k]
            assert w["length"] == n and w["md5"] == hashlib.md5(c.es[o:o + n].tobytes()).hexdigest(), (s, k)
            assert w["pts"] == (c.pts[k] & et.PTS_MASK) / 90000.0, (s, k)


def test_python_module_and_exports(hip_lib):
    from jsmpeg_amd import encode
    lib = ctypes.CDLL(hip_lib)
    for name in ("jsmpeg_hip_encoder_set_ts", "jsmpeg_hip_encoder_ts_pts", "jsmpeg_hip_encoder_ts", "jsmpeg_hip_encoder_ts_range",
                 "jsmpeg_hip_encoder_ts_picture_range", "jsmpeg_hip_encoder_read_ts", "jsmpeg_hip_ts_bound", "jsmpeg_hip_ts_mux_device"):
        assert name in encode.SYMBOLS and hasattr(lib, name), name
    for name in ("set_ts", "ts", "ts_all", "ts_range", "ts_picture_ranges", "device_ts", "ts_mux"):
        assert hasattr(encode.Encoder, name), name
    assert callable(encode.ts_bound) and callable(encode.ts_mux_device)


def test_kernels_use_no_scratch():
    from jsmpeg_amd import build
    usage = build.check_kernel_resources()
    for k in ("k_ts_units", "k_ts_plan", "k_ts_write"):
        name = [n for n in usage if k in n]
        assert name, k
        assert usage[name[0]]["ScratchSize"] == 0, k


def test_sanitizers_on_the_rule_and_the_driver():
    """enc_ts.h's functions and the simulator's driver as a stand-alone program (its own main, g++
    -fsanitize=address,undefined): the edge sizes, 1 .. 400 in one call and one by one, random streams -- the source buffer
    exactly the units' size, so a fetch outside a unit at either end of the buffer is an error"""
    out_dir = os.path.join(ei.SIM_DIR, "_asan")
    os.makedirs(out_dir, exist_ok=True)
    exe = os.path.join(out_dir, "sim_ts_main")
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in ei.sim_deps(et.SIM_SRC) + [__file__]):
        subprocess.check_call(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DSIM_TS_MAIN"] + ei.CXXFLAGS +
                              ["-o", exe, et.SIM_SRC])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-3000:]
    assert "502 cases equal the serial mux" in r.stdout
