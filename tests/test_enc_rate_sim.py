"""The encoder's rate control (rule RATE, jsmpeg_amd/csrc/enc_rate.h) without a GPU: the CPU simulator of its kernels
(sim_encode_rate of tests/sim/sim_encode_pass.cpp) against the brute-force restatement (tests/enc_rate_ref.py) in chosen scale, budget, bytes,
buffer, ranges and reconstructions; the properties of the rule on every picture; the fixed-scale simulator (sim_encode_p,
unchanged) given the chosen scales; and the oracle as judge of every stream."""
import numpy as np
import pytest

import enc_inputs as ei
import enc_p_inputs as ep
import enc_rate_inputs as er
import enc_rate_ref
from jsmpeg_amd import encode


@pytest.fixture(scope="module")
def cases(libs):
    return er.rate_cases(libs)


_sim, _ref = {}, {}


def sim_of(cases, name):
    if name not in _sim:
        _sim[name] = cases[name].sim()
    return _sim[name]


def ref_of(cases, name):
    if name not in _ref:
        c = cases[name]
        _ref[name] = enc_rate_ref.encode(c.frames, c.width, c.height, c.gop, c.search, streams=c.streams, **c.rule())
    return _ref[name]


NAMES = ("pan_gop3_T150", "pan_gop4_T100", "pan_T20", "pan_T1500", "pan_gop1", "noise_T1500", "noise_T4000", "flat_grey", "flat_wide",
         "content_177x145", "content_177x145_R0", "one_macroblock", "range_4_16", "range_8_8", "streams_W1", "streams_W16")


def test_the_list_is_the_case_list(cases):
    assert sorted(NAMES) == sorted(cases)


def assert_same(got, want, where):
    assert [r[0] for r in got.rate] == want.rate.q, where
    assert [r[1] for r in got.rate] == want.rate.budget, where
    assert [r[2] for r in got.rate] == want.rate.bytes, where
    assert got.vectors == want.vectors and got.stats == want.stats, where
    assert all(np.array_equal(a, b) for a, b in zip(got.recon, want.recon)), where
    assert got.ranges == want.ranges and got.streams == want.streams, where
    assert got.buf == want.buf, where


@pytest.mark.parametrize("name", NAMES)
def test_simulator_equals_the_restatement(cases, name):
    assert_same(sim_of(cases, name), ref_of(cases, name), name)


@pytest.mark.parametrize("name", NAMES)
def test_properties_of_the_rule(cases, name):
    c, got = cases[name], sim_of(cases, name)
    streams = c.streams or [0] * len(c.frames)
    er.check_properties(got.rate, got.ranges, ref_of(cases, name).rate.table, streams, c.gop, c.T, c.q_min, c.q_max, name)
    fixed = ep.sim_encode_p(c.frames, c.width, c.height, c.gop, c.search, streams=c.streams, qscale=[r[0] for r in got.rate], max_streams=c.max_streams)
    assert fixed.buf == got.buf and fixed.ranges == got.ranges, name


@pytest.mark.parametrize("name", NAMES)
def test_the_oracle_decodes_every_stream_to_the_encoders_reconstruction(libs, cases, name):
    c, got = cases[name], sim_of(cases, name)
    streams = c.streams or [0] * len(c.frames)
    for s in sorted(set(streams)):
        ks = [k for k, v in enumerate(streams) if v == s]
        es = got.stream(s)
        assert ep.picture_types(es) == ep.expected_types(len(ks), c.gop), (name, s)
        dec = ep.oracle_frames(libs, es)
        assert len(dec) == len(ks) and all(np.array_equal(dec[i], got.recon[k]) for i, k in enumerate(ks)), (name, s)


def test_the_edges_show_on_the_inputs_meant_for_them(cases):
    """what each case is there for is really in it -- judged by the restatement, so that a change of an input is noticed"""
    r = ref_of(cases, "pan_gop3_T150").rate
    assert r.q[6] == 31 and r.bytes[6] > r.budget[6] == 150                         # a GOP of one that fits at no scale
    r = ref_of(cases, "pan_gop4_T100").rate
    assert any(b == g and q > 1 for q, g, b in zip(r.q, r.budget, r.bytes))         # exactly the budget is taken
    r = ref_of(cases, "pan_T20").rate
    assert set(r.q) == {31} and r.budget[1:3] == [0, 0]
    assert set(ref_of(cases, "pan_T1500").rate.q) == {1}
    r = ref_of(cases, "pan_gop1").rate
    assert len(set(r.budget)) == 1 and 1 < min(r.q) and max(r.q) < 31
    r = ref_of(cases, "noise_T1500").rate
    assert all(q == 31 and b > g for q, g, b in list(zip(r.q, r.budget, r.bytes))[1:])  # far above any budget
    assert 0 < sim_of(cases, "noise_T1500").stats[1][0] < 12                        # intra macroblocks inside a P picture
    assert all(1 < q < 31 for q in ref_of(cases, "noise_T4000").rate.q[1:3])
    assert sim_of(cases, "flat_grey").stats[1][3] and sim_of(cases, "flat_wide").stats[1] == (0, 0, 2, 46)
    a, b = ref_of(cases, "streams_W1").rate, ref_of(cases, "streams_W16").rate
    assert a.budget[0] < b.budget[0] and a.q != b.q
    assert a.budget[3] == 120                                                       # stream 0's fourth picture: a GOP of one


def test_a_range_of_one_scale_is_the_fixed_scale_call(cases):
    c, got = cases["range_8_8"], sim_of(cases, "range_8_8")
    assert [r[0] for r in got.rate] == [8] * len(c.frames)
    assert got.buf == ep.sim_encode_p(c.frames, c.width, c.height, c.gop, c.search, qscale=8).buf
    r = ref_of(cases, "range_4_16").rate
    assert all(4 <= q <= 16 for q in r.q) and len(set(r.q)) > 1


def test_gop_1_at_one_scale_is_the_intra_encoder(cases):
    c = cases["pan_gop1"]
    got = er.sim_encode_rate(c.frames, c.width, c.height, 1, 7, 250, q_min=9, q_max=9)
    assert got.triple() == ei.sim_encode(c.frames, c.width, c.height, qscale=9)


@pytest.fixture(scope="module")
def long_call():
    return ep.long_call()


def test_the_long_call(long_call):
    """1100 pictures in five streams with gaps over the range 6 .. 10: the simulator against the restatement on the first 300
    pictures (the cut falls on a GOP's end: 42 pictures of stream 4 are six GOPs of 7, so the prefix is chosen as in the whole
    call), the whole call against the properties and the fixed-scale simulator"""
    frames, w, h, streams, _ = long_call
    rule = er.LONG_RULE
    want = enc_rate_ref.encode(frames[:300], w, h, er.LONG_GOP, er.LONG_SEARCH, streams=streams[:300], **rule)
    assert_same(er.sim_long(long_call, 300), want, "first 300")
    got = er.sim_long(long_call)
    assert got.rate[:300] == list(zip(want.rate.q, want.rate.budget, want.rate.bytes))
    assert len(set(r[0] for r in got.rate)) == 5                                    # every scale of the range is in use
    table = enc_rate_ref.choose(frames, w, h, er.LONG_GOP, er.LONG_SEARCH, streams=streams, **rule)
    assert [r[0] for r in got.rate] == table.q
    er.check_properties(got.rate, got.ranges, table.table, streams, er.LONG_GOP, rule["T"], rule["q_min"], rule["q_max"], "long")
    fixed = ep.sim_encode_p(frames, w, h, er.LONG_GOP, er.LONG_SEARCH, streams=streams, qscale=[r[0] for r in got.rate], max_streams=ep.LONG_MAX_STREAMS)
    assert fixed.buf == got.buf and fixed.ranges == got.ranges and fixed.table == got.table


def test_bytes_per_picture():
    assert encode.bytes_per_picture(1_200_000, 5) == 5000 and encode.bytes_per_picture(1_200_000, 0) == 5000
    assert encode.bytes_per_picture(1_000_000, 3) == 5000
    assert encode.bytes_per_picture(1_200_000, 4) == 5005                           # 30000 / 1001 pictures per second
    assert encode.bytes_per_picture(1, 8) == 1
    assert "jsmpeg_hip_encoder_set_rate" in encode.SYMBOLS and "jsmpeg_hip_encoder_picture_rate" in encode.SYMBOLS
