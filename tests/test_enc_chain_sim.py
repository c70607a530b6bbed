"""The encoder's chains across calls (JSMPEG_HIP_ENC_CHAIN; the rule: jsmpeg_amd/csrc/enc_chain.h) without a GPU: the simulator of
a handle that is called again and again (sim_chain_* of tests/sim/sim_encode_pass.cpp) against the yardstick -- the one-call encoder as it
was (ep.sim_encode_p, er.sim_encode_rate) on the same pictures: the pieces concatenated, every picture's reconstruction, kinds,
bytes and rate choice.  Where a chain is ended the segments between the ends are the units."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import enc_chain_inputs as ec
import enc_inputs as ei
import enc_p_inputs as ep
import enc_rate_inputs as er

PAN = ep.pan_frames(64, 48, 8, (3, -2))        # its first seven: ep.pan_frames(64, 48, 7, (3, -2)), er.rate_cases' pan
CONFIGS = ((3, 7), (4, 0))                     # (gop, search range)
SCALES = (1, 8)


@pytest.fixture(scope="module")
def cases(libs):
    return ep.p_cases(libs)


def all_splits_equal(frames, w, h, gop, R, q, cuts_list, where, rule=None):
    seg0 = None
    for cuts in cuts_list:
        seg = ec.run_split(frames, w, h, gop, R, cuts, q, rule)
        if seg0 is None:
            seg0 = seg
            one = ec.one_call(seg, w, h, gop, R, q, rule)
        ec.assert_segment(seg, one, (where, cuts))
    return one


@pytest.mark.parametrize("gop,R", CONFIGS)
@pytest.mark.parametrize("q", SCALES)
def test_every_split_of_the_pan(q, gop, R):
    assert len(ec.splits(7)) == 64 and sorted(map(tuple, ec.splits(3))) == [(1, 1, 1), (1, 2), (2, 1), (3,)]
    one = all_splits_equal(PAN[:7], 64, 48, gop, R, q, ec.splits(7), "pan")
    assert ep.picture_types(one.stream(0)) == ep.expected_types(7, gop)


@pytest.mark.parametrize("gop,R", CONFIGS)
@pytest.mark.parametrize("q", SCALES)
def test_every_split_of_the_other_inputs(cases, q, gop, R):
    for name in ("noise", "one_macroblock"):
        frames, w, h = cases[name]
        all_splits_equal(frames, w, h, gop, R, q, ec.splits(len(frames)), name)
    for name in ("content_177x145", "flat_wide"):
        frames, w, h = cases[name]
        n = len(frames)
        all_splits_equal(frames, w, h, gop, R, q, [[1] * n, [1, n - 1]], name)


def test_the_oracle_decodes_every_concatenation_to_the_reconstructions(libs, cases):
    def held(frames, w, h, cuts_list, where):
        for cuts in cuts_list:
            seg = ec.run_split(frames, w, h, 3, 7, cuts, 8)
            got = ep.oracle_frames(libs, np.frombuffer(b"".join(seg.pieces), dtype=np.uint8))
            assert len(got) == len(frames), (where, cuts)
            for k in range(len(frames)):
                assert np.array_equal(got[k], seg.recon[k]), (where, cuts, k)
    held(PAN[:7], 64, 48, ec.splits(7), "pan")
    for name in ("noise", "content_177x145", "flat_wide", "one_macroblock"):
        frames, w, h = cases[name]
        held(frames, w, h, [[1] * len(frames), [1, len(frames) - 1]], name)


@pytest.mark.parametrize("n,gop,T", [(6, 3, 150), (8, 4, 100)])
def test_rate_every_split_of_whole_gops(libs, cases, n, gop, T):
    """er.rate_cases' pan_gop3_T150 and pan_gop4_T100, cut to whole GOPs: m = gop is then the one call's m too"""
    c = er.rate_cases(libs, cases)["pan_gop%d_T%d" % (gop, T)]
    assert (c.gop, c.T, c.search) == (gop, T, 7) and all(np.array_equal(a, b) for a, b in zip(c.frames, PAN[:7]))
    one = all_splits_equal(PAN[:n], 64, 48, gop, 7, 8, ec.splits(n), "rate", rule=c.rule())
    assert len({q for q, _, _ in one.rate}) > 1          # the rule chose, and not one scale throughout


@pytest.mark.parametrize("W", [1, 16])
def test_rate_streams(W):
    """three streams with a gap in their numbers, whole GOPs each, calls that cut the GOPs differently per stream"""
    pan9 = ep.pan_frames(64, 48, 9, (2, 1))
    own = {0: PAN[:3], 2: PAN[1:7], 5: pan9[:6]}
    rule = dict(T=120, q_min=1, q_max=31, W=W)
    # stream 5's second call: levels 1, 2, 0, 1 -- its first picture reads the spent bytes, its last, of the same level, writes them
    calls = [{0: 1, 2: 2, 5: 1}, {0: 2, 2: 1, 5: 4}, {2: 3}, {5: 1}]
    led, at = ec.Ledger(), {s: 0 for s in own}
    with ec.Chain(64, 48, 7) as c:
        c.set_gop(3, 7)
        c.set_rate(**rule)
        for call in calls:
            frames, streams = [], []
            for s in sorted(call):
                frames += own[s][at[s]:at[s] + call[s]]
                streams += [s] * call[s]
                at[s] += call[s]
            led.add(frames, streams, c.encode(frames, streams), False)
        assert [c.chain_info(s) for s in (0, 1, 2, 5)] == [(True, 3), (False, 0), (True, 6), (True, 6)]
    for s in own:
        (seg,) = led.segments[s]
        assert len(seg.frames) == len(own[s])
        ec.assert_segment(seg, ec.one_call(seg, 64, 48, 3, 7, rule=rule), (W, s))


def test_rate_incomplete_gop_budgets():
    """five pictures at gop 3 as [2, 1, 2]: the last GOP stays incomplete and is still budgeted for three -- every budget from the
    REPORTED bytes, in Python integers, as enc_rate.h states it with m = gop"""
    gop, T, W, q_max = 3, 150, 4, 31
    led = ec.Ledger()
    with ec.Chain(64, 48) as c:
        c.set_gop(gop, 7)
        c.set_rate(T, 1, q_max, W)
        for a, b in ((0, 2), (2, 3), (3, 5)):
            led.add(PAN[a:b], None, c.encode(PAN[a:b]), False)
    (seg,) = led.segments[0]
    for k, (q, budget, size) in enumerate(seg.rate):
        level = k % gop
        spent = sum(seg.sizes[k - level:k])
        left = max(gop * T - spent, 0)
        w, S = (W, W + gop - 1) if level == 0 else (1, gop - level)
        assert budget == left * w // S, k
        assert size == seg.sizes[k] and (size <= budget or q == q_max), k
    one = er.sim_encode_rate(PAN[:5], 64, 48, gop, 7, T, W=W, end=False)
    assert seg.rate[:3] == one.rate[:3] and seg.rate[3][1] != one.rate[3][1]      # the one call cuts its last GOP short: m = 2


def test_streams_come_and_go():
    """stream numbers 0, 2, 5 over six calls: 2 is absent from two of them, 5 is reset in the middle of a GOP, 0 is closed with
    END + CHAIN and goes on; every segment equals its one-call encode"""
    pan9 = ep.pan_frames(64, 48, 9, (2, 1))
    own = {0: PAN[:7], 2: pan9[:4], 5: pan9[2:8]}
    calls = [((0, 2, 5), False), ((0, 2, 5), False), ((0, 5), False), ((0,), True), ((0, 2, 5), False), ((0, 2, 5), False)]
    led, at = ec.Ledger(), {s: 0 for s in own}
    with ec.Chain(64, 48, 6) as c:
        c.set_gop(3, 7)
        for i, (present, end) in enumerate(calls):
            if i == 2:
                assert c.chain_info(5) == (True, 2)
                c.chain_reset(5)
                led.cut(5)
                assert c.chain_info(5) == (False, 0) and c.chain_info(0) == (True, 2)
            frames = [own[s][at[s]] for s in present]
            for s in present:
                at[s] += 1
            r = c.encode(frames, list(present), end=end)
            led.add(frames, list(present), r, end)
            if i == 3:
                assert c.chain_info(0) == (False, 0) and c.chain_info(2) == (True, 2)
        assert [c.chain_info(s) for s in (0, 2, 5)] == [(True, 2), (True, 4), (True, 3)]
        with pytest.raises(RuntimeError):
            c.chain_reset(6)
    assert [len(seg.frames) for seg in led.segments[0]] == [4, 2]
    assert [len(seg.frames) for seg in led.segments[2]] == [4]
    assert [len(seg.frames) for seg in led.segments[5]] == [2, 3]
    for s, segs in led.segments.items():
        for i, seg in enumerate(segs):
            one = ec.one_call(seg, 64, 48, 3, 7, closed=(s == 0 and i == 0))
            ec.assert_segment(seg, one, (s, i))
            assert ep.picture_types(one.stream(0))[0] == 1


def same_result(a, b):
    return a.triple() == b.triple() and a.stats == b.stats and all(np.array_equal(x, y) for x, y in zip(a.recon, b.recon))


def test_unchained_calls_between_chained_ones(cases):
    """a call without the flag reads no record and writes none: it is what it was, and the chain around it goes on"""
    noise = cases["noise"][0]
    led = ec.Ledger()
    with ec.Chain(64, 48, 2) as c:
        c.set_gop(3, 7)
        for a, b in ((0, 2), (2, 3), (3, 7)):
            led.add(PAN[a:b], None, c.encode(PAN[a:b], None, 8, end=b == 7), b == 7)
            before = c.record(0)
            for frames, streams in ((noise, None), (PAN[4:7] + noise[:2], [0, 0, 0, 1, 1])):
                got = c.encode(frames, streams, 5, end=True, chain=False)
                assert same_result(got, ep.sim_encode_p(frames, 64, 48, 3, 7, streams=streams, qscale=5, max_streams=2))
            assert c.record(0) == before
    (seg,) = led.segments[0]
    ec.assert_segment(seg, ec.one_call(seg, 64, 48, 3, 7), "chained")
    with ec.Chain(64, 48, 7) as c:                           # and with rate control: er's case of streams with a short GOP
        pan9 = ep.pan_frames(64, 48, 9, (2, 1))
        c.set_gop(3, 7)
        c.set_rate(120, 1, 31, 4)
        c.encode(pan9[:2], [2, 2])
        got = c.encode(pan9, er.PAN_STREAMS, end=True, chain=False)
        want = er.sim_encode_rate(pan9, 64, 48, 3, 7, 120, streams=er.PAN_STREAMS, max_streams=7)
        assert same_result(got, want) and got.rate == want.rate
        assert c.chain_info(2) == (True, 2) and c.chain_info(0) == (False, 0)


def test_the_records():
    """ordinals, parity, the ends of a chain, and the wrap before 2 ** 32"""
    with ec.Chain(64, 48, 3) as c:
        c.set_gop(3, 0)
        assert c.encode(PAN[:2], [1, 1]).ordinals == [0, 1]
        assert c.record(1) == dict(have=1, n=2, parity=1, rated=0) and c.record(0)["have"] == 0
        assert c.encode(PAN[2:3], [1]).ordinals == [2] and c.record(1)["parity"] == 0
        assert c.encode(PAN[3:5], [1, 2]).ordinals == [3, 0]
        assert c.encode(PAN[:1], [1], cap=64) is None        # overflow: the call's streams are reset, the others stay
        assert c.chain_info(1) == (False, 0) and c.chain_info(2) == (True, 1)
        c.set_gop(3, 0)
        assert c.chain_info(2) == (False, 0)
        c.encode(PAN[:1], [0])
        c.encode(PAN[:1], [2])
        c.chain_reset()
        assert [c.chain_info(s) for s in range(3)] == [(False, 0)] * 3
        for gop in (3, 4, 1024):
            c.set_gop(gop, 0)
            first = next(v for v in range(0xffffffff - 1024 + 1, 1 << 32) if v % gop == 0)    # the GOP that begins at 0 instead
            assert ec.next_ordinal(first - 1, gop) == 0 and ec.next_ordinal(first - 2, gop) == first - 1 and ec.next_ordinal(7, gop) == 8
            c.set_record(0, 1, first - 2, parity=0)
            r = c.encode(PAN[:4], [0, 0, 0, 0])
            assert r.ordinals == [first - 2, first - 1, 0, 1]
            assert ep.picture_types(r.stream(0)) == [2, 2, 1, 2]
            assert c.chain_info(0) == (True, 2)


def test_python_module_and_exports(hip_lib):
    from jsmpeg_amd import encode
    lib = ctypes.CDLL(hip_lib)
    assert encode.CHAIN == 2
    for name in ("jsmpeg_hip_encoder_chain_reset", "jsmpeg_hip_encoder_chain_info"):
        assert name in encode.SYMBOLS and hasattr(lib, name), name
    header = open(os.path.join(ei.ROOT, "include", "jsmpeg_hip.h")).read()
    assert "#define JSMPEG_HIP_ENC_CHAIN 2u" in header and "P CHAINS DO NOT CROSS CALLS" not in header


def test_kernels_use_no_scratch():
    from jsmpeg_amd import build
    usage = build.check_kernel_resources()
    for k in ("k_enc_motion", "k_enc_measure_p", "k_enc_rate_measure", "k_enc_rate_scan", "k_enc_rate_pick", "k_enc_write_p"):
        name = [n for n in usage if k in n]
        assert name, k
        assert usage[name[0]]["ScratchSize"] == 0, k


def test_sanitizers_on_the_rule_and_the_driver(tmp_path):
    """enc_chain.h's host functions and the simulator's driver around them as a stand-alone program (its own main, g++
    -fsanitize=address,undefined) over the 64 cuts of the pan at both configurations and scales.  Without shift-base, as in
    tools/sanitize_sim.py: the dequantiser the encoder shares with the decoder (recon_block.h) shifts negative levels left"""
    out_dir = os.path.join(ec.SIM_DIR, "_asan")
    os.makedirs(out_dir, exist_ok=True)
    exe = os.path.join(out_dir, "sim_chain_main")
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in ec.sim_deps() + [__file__]):
        subprocess.check_call(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize=shift-base", "-fno-sanitize-recover=all", "-DSIM_CHAIN_MAIN"] + ec.CXXFLAGS +
                              ["-o", exe, ec.SIM_SRC])
    data = tmp_path / "pan.bin"
    np.stack(PAN[:7]).tofile(str(data))
    r = subprocess.run([exe, str(data), "64", "48", "7"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-3000:]
    assert "256 cuts equal the one call" in r.stdout
