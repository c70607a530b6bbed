"""The MP2 encoder's rule at every setting it accepts and at the edges of its arithmetic, without a GPU: the numpy restatement
(tests/mp2_enc_ref.py) against the simulator (tests/sim/sim_mp2_enc.cpp: the kernel's own functions) on the inputs of
tests/mp2_enc_inputs.py (ALL_SETTINGS, edge_inputs, the padding period), and the CONDITIONS ON THOSE INPUTS: what they must
reach -- every pair winning a round, ties the order decides, both ends of the allocation loop, every code, the analysis at
its bounds, the conversion's ties, every store alignment -- each computed from the restatement or the closed-form plan, never
from the code under test, so that an input that stops reaching its edge fails here.  tests/test_gpu_mp2_encode_edges.py
holds the kernel to the simulator on the same inputs."""
import collections
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
import mp2_enc_inputs as inputs
import mp2_enc_ref as ref
from mp2_enc_util import SimState, oracle_decode, sim_analysis, sim_encode, sim_lib, sim_main, write_cases
from test_mp2_enc_sim import _branch

sys.path.insert(0, os.path.join(ROOT, "tools"))
import mp2_enc_bounds      # noqa: E402

SETTINGS = inputs.ALL_SETTINGS
IDS = [inputs.setting_id(c) for c in SETTINGS]
KINDS = inputs.EDGE_KINDS
TABLES = {(27, 1): "3-B.2a", (30, 1): "3-B.2b", (8, 0): "3-B.2c", (12, 0): "3-B.2d"}


@functools.lru_cache(maxsize=None)
def edge_pcm(rate):
    return inputs.edge_inputs(rate)


@functools.lru_cache(maxsize=None)
def restated(cfg):
    """{input: (bytes, infos per frame)} of the restatement -- computed once, shared, never changed"""
    out = {}
    for kind, x in edge_pcm(inputs.RATES[cfg[0]]).items():
        infos = []
        data, _ = ref.encode(cfg, x, infos=infos)
        out[kind] = (data, infos)
    return out


@functools.lru_cache(maxsize=None)
def simulated(cfg):
    """(bytes per input, stats per frame) of ONE simulated call with a stream per input: the call the GPU test makes"""
    xs = edge_pcm(inputs.RATES[cfg[0]])
    return sim_encode(cfg, [xs[k] for k in KINDS])


def every_info():
    """(setting, input, frame, info) over everything restated"""
    for cfg in SETTINGS:
        for kind in KINDS:
            for f, info in enumerate(restated(cfg)[kind][1]):
                yield cfg, kind, f, info


def table_of(cfg):
    return TABLES[ref.table_select(*cfg)]


# ------------------------------------------------------------------------------------------------ the three statements

def test_every_setting_the_rule_accepts():
    assert len(SETTINGS) == 60 == len(set(SETTINGS))
    assert sorted(SETTINGS) == sorted((sr, ch, br) for sr in range(3) for ch in (1, 2) for br in range(1, 15) if not ref.refused(sr, ch, br))
    L = sim_lib()
    assert all(L.sim_mp2_enc_rule(*cfg, None) == 0 for cfg in SETTINGS)
    assert {table_of(c) for c in SETTINGS} == set(TABLES.values())
    assert tuple(KINDS) == tuple(edge_pcm(44100))


@pytest.mark.parametrize("cfg", SETTINGS, ids=IDS)
def test_restatement_and_simulator_write_the_same_bytes(cfg):
    pieces, _ = simulated(cfg)
    for kind, got in zip(KINDS, pieces):
        assert got == restated(cfg)[kind][0], kind


@pytest.mark.parametrize("cfg", SETTINGS, ids=IDS)
def test_stats_block_equals_the_restatement(cfg):
    _, stats = simulated(cfg)
    k = 0
    for kind in KINDS:
        for f, info in enumerate(restated(cfg)[kind][1]):
            size = ref.frame_bytes(cfg[0], cfg[2], f)
            want = [len(info["codes"]), info["used"], 8 * size - info["used"], max(info["code"].values())]
            assert [int(v) for v in stats[k]] == want and info["left"] == want[2], (kind, f)
            k += 1
    assert k == len(stats)


@pytest.mark.parametrize("cfg", SETTINGS, ids=IDS)
def test_oracle_decodes_every_frame_at_its_closed_form_size(cfg, libs):
    pieces, _ = simulated(cfg)
    xs = edge_pcm(inputs.RATES[cfg[0]])
    for kind, data in zip(KINDS, pieces):
        pcm, sizes = oracle_decode(libs, data)
        n = len(xs[kind])
        assert len(pcm) == n and sizes == [ref.frame_bytes(cfg[0], cfg[2], f) for f in range(n)] and sum(sizes) == len(data), kind


# ------------------------------------------------------------------------------------------------ what the inputs reach

def test_every_pair_wins_a_round_and_every_lane_does():
    """the device takes a round's winner from a wave-wide maximum; a lane that maximum failed to see would change bytes only in
    a round that lane wins.  Per setting, every pair q = 2 sb + ch that exists wins at least one round."""
    won = collections.defaultdict(set)
    for cfg, _, _, info in every_info():
        won[cfg].update(2 * sb + ch for sb, ch in info["winners"])
    lanes = set()
    for cfg in SETTINGS:
        sblimit, _ = ref.table_select(*cfg)
        want = {2 * sb + ch for sb in range(sblimit) for ch in range(cfg[1])}
        assert won[cfg] == want, (cfg, sorted(want - won[cfg]))
        lanes |= won[cfg]
    assert lanes == set(range(60))


def test_rounds_are_decided_by_the_order_of_ties():
    """rounds in which several open pairs share the largest noise value, so that (lower subband, then channel 0) decides: among
    the two channels of one subband, among pairs of one 16-lane row, among pairs of different rows"""
    seen = collections.Counter()
    for _, _, _, info in every_info():
        for tied in info["ties"]:
            qs = sorted(2 * sb + ch for sb, ch in tied)
            seen["channels"] += any(a >> 1 == b >> 1 for a in qs for b in qs if a < b)
            seen["row"] += any(a >> 1 != b >> 1 and a >> 4 == b >> 4 for a in qs for b in qs if a < b)
            seen["rows"] += any(a >> 4 != b >> 4 for a in qs for b in qs if a < b)
    print("tied rounds:", dict(seen))
    assert seen["channels"] and seen["row"] and seen["rows"]


def test_the_loop_ends_both_ways_in_every_table():
    """per allocation table: a frame that ends with every loud pair at its top code and more bits left than the table's dearest
    raise, and a frame that ends because no raise fits.  (Per table: at 32 kbit/s the first does not occur.)"""
    ends, most = collections.defaultdict(set), {}
    for cfg, kind, f, info in every_info():
        assert info["rounds"] <= 540
        if info["end"]:
            ends[table_of(cfg)].add(info["end"])
        if info["rounds"] > most.get(table_of(cfg), (0,))[0]:
            most[table_of(cfg)] = (info["rounds"], inputs.setting_id(cfg), kind, f)
    print("most rounds per table:", most)
    assert dict(ends) == {t: {"top", "fit"} for t in TABLES.values()}
    dcs = [info for cfg, kind, f, info in every_info() if cfg == (1, 2, 14) and kind == "dc" and f == 2]
    assert len(dcs) == 1
    for info in dcs:                      # stereo 48 kHz 384 kbit/s, third frame: only subbands 0 and 1 are loud, their four pairs climb to 15
        assert info["end"] == "top" and info["left"] > 1000 and {p: c for p, c in info["code"].items() if c} == {(0, 0): 15, (0, 1): 15, (1, 0): 15, (1, 1): 15}


def test_every_code_is_reached():
    scfsi, first, tops, branches = set(), set(), collections.defaultdict(set), set()
    for cfg, _, _, info in every_info():
        scfsi.update(info["sel"][p] for p in info["codes"])
        first |= info["first_nsf"]
        for (sb, ch), code in info["code"].items():
            if code:
                branches.add(_branch(info["high"], sb, code))
                if code == (1 << ref.nbal(info["high"], sb)) - 1:
                    tops[table_of(cfg)].add(code)
    assert scfsi == {0, 1, 2, 3} and first == {1, 2, 3}
    assert dict(tops) == {"3-B.2a": {15, 7, 3}, "3-B.2b": {15, 7, 3}, "3-B.2c": {15, 7}, "3-B.2d": {15, 7}}
    want = {("low", 1), ("low", 2), ("low", 3), ("low", 15), ("low", "2^n"), ("high<3", 1), ("high<3", "2^n"), ("high<11", 15),
            ("high<11", "odd"), ("high<11", "2^n"), ("high<23", 7), ("high<23", "odd"), ("high<23", "2^n"), ("high>=23", 3), ("high>=23", "odd")}
    assert branches == want, want - branches


def test_the_quantiser_is_clamped_at_both_ends():
    """samples at or above the top level (c1 == 0) and below the lowest one (c1 == steps) of their quantiser occur, on the
    frames of bounds() as well"""
    total, on_bounds = np.zeros(2, np.int64), np.zeros(2, np.int64)
    for _, kind, _, info in every_info():
        total += info["clamped"]
        if kind == "bounds":
            on_bounds += info["clamped"]
    assert total.all() and on_bounds.all(), (total, on_bounds)


# ------------------------------------------------------------------------------------------------ the analysis at its bounds

def _bounds_tracks():
    """int64 [2][480 + 4 * 1152]: bounds() as the encoder's integers behind a silent history"""
    s16 = ref.pcm_s16(inputs.bounds())
    return np.concatenate([np.zeros((2, 480), np.int64), s16.transpose(1, 0, 2).reshape(2, -1)], axis=1)


def _attainable():
    """from the integer tables alone: the largest |Y[i]|, |Z[t]| and |acc[k]| any PCM can produce"""
    tap = np.abs(ref.W).reshape(8, 64).sum(axis=0)
    y = 32767 * tap
    z = np.array([y[16]] + [y[16 + t] + y[16 - t] for t in range(1, 17)] + [y[16 + t] + y[80 - t] for t in range(17, 32)])
    acc = [32767 * sum(abs(int(ref.W[n]) * int(ref.MATRIX[k][n % 64])) for n in range(512)) for k in range(32)]
    return y, z, acc


def test_bounds_input_drives_the_analysis_to_its_bounds():
    """Y, the folded Z and its halves, and S[k] for k = 0, 7, 15, 16, 31 at the largest values any PCM can give, in both signs;
    the simulator's Y, Z, halves and S (the kernel's functions) equal the restatement's there.

    The tool's y_max (3 037 042 162) is attained exactly.  Its z_max = 2 y_max (6 074 084 324) is a triangle bound no PCM
    reaches: Z[t] folds two DIFFERENT Y, and only Y[0] has the largest tap sum.  The largest |Z| any PCM gives is 5 863 523 582
    (t = 16: Y[32] + Y[0]); that figure, and the |high half| 89 471 that goes with it (the tool bounds it by 92 684), are what is
    asserted exactly.  Likewise s_max (22 298 327) is a triangle bound; the attainable |S| is 14 211 140 (k = 0)."""
    b = mp2_enc_bounds.bounds()
    tracks = _bounds_tracks()
    y_att, z_att, acc_att = _attainable()
    windows = {name: g for name, g, _ in inputs.bounds_windows()}
    Y = np.stack([np.concatenate([ref.window_sums(tracks[ch, 1152 * f:1152 * f + 1632]) for f in range(inputs.BOUNDS_FRAMES)]) for ch in range(2)])
    Z = np.stack([ref.fold(Y[ch]) for ch in range(2)])                              # [ch][sub-block][t]
    S = np.stack([np.concatenate([ref.analysis(tracks[ch, 1152 * f:1152 * f + 1632]) for f in range(inputs.BOUNDS_FRAMES)]) for ch in range(2)])
    assert np.array_equal(Y[1], -Y[0]) and np.array_equal(Z[1], -Z[0])
    # Y: every i at its maximum at once, and the tool's figure exactly
    assert np.array_equal(Y[0, windows["y"]], y_att) and np.array_equal(Y[1, windows["y"]], -y_att)
    assert int(np.abs(Y).max()) == b["y_max"] == int(y_att.max()) and b["y_bits"] == 33
    # Z: t <= 16 on 'y', t >= 17 on 'z'; the largest of all, and its high half
    assert np.array_equal(Z[0, windows["y"], :17], z_att[:17]) and np.array_equal(Z[0, windows["z"], 17:], z_att[17:])
    assert np.array_equal(np.abs(Z).max(axis=(0, 1)), z_att)
    z_top = int(z_att.max())
    assert int(np.abs(Z).max()) == z_top == 5863523582 and z_top < b["z_max"] == 2 * b["y_max"]
    hi = Z >> 16
    assert int(np.abs(hi).max()) == -((-z_top) >> 16) == 89471 <= b["z_hi_max"]
    assert 32 * 32768 * int(np.abs(hi).max()) < b["half_sum_max"] == 97186217984
    # S: the five k, both signs, in Python integers
    for k in inputs.BOUNDS_K:
        g = windows["s%d" % k]
        acc = sum(int(ref.W[n]) * int(ref.MATRIX[k][n % 64]) * int(tracks[0, 480 + 32 * g + 31 - n]) for n in range(512))
        assert acc == acc_att[k] and abs(acc) < 1 << 53
        assert int(S[0, g, k]) == (acc + (1 << 27)) >> 28 and int(S[1, g, k]) == (-acc + (1 << 27)) >> 28
        assert int(np.abs(S[:, :, k]).max()) == (acc_att[k] + (1 << 27)) >> 28
    assert (acc_att[7] + (1 << 27)) >> 28 == 14191380
    s_top = max((a + (1 << 27)) >> 28 for a in acc_att)
    assert s_top == 14211140 < b["s_max"] == 22298327
    # mp2e_scale_index's fall-back ("0 if there is none") cannot be reached from PCM: 2 max|S| stays below scalefactor(0)
    assert 2 * s_top < ref.scalefactor(0) == 1 << 25
    # the kernel's functions on the same samples
    for ch in range(2):
        for f in range(inputs.BOUNDS_FRAMES):
            sY, sZ, halves, sS = sim_analysis(tracks[ch, 1152 * f:1152 * f + 1632])
            rows = slice(36 * f, 36 * f + 36)
            assert np.array_equal(sY, Y[ch, rows]) and np.array_equal(sZ, Z[ch, rows]) and np.array_equal(sS, S[ch, rows])
            assert np.array_equal(halves[:, :, 0], Z[ch, rows] & 0xffff) and np.array_equal(halves[:, :, 1], Z[ch, rows] >> 16)


def test_bounds_input_reaches_the_frames():
    """the S of the encoded frames (the restatement's info) are the ones above: the stream of bounds() carries them"""
    for cfg in ((1, 2, 14), (2, 1, 1)):
        infos = restated(cfg)["bounds"][1]
        S = np.concatenate([i["S"] for i in infos], axis=1)                          # [ch][sub-block][k]
        assert int(np.abs(S).max()) == 14211140


# ------------------------------------------------------------------------------------------------ the input conversion

def test_conversion_edges():
    L = sim_lib()
    vals = inputs.conversion_values()
    f32 = np.float32
    with np.errstate(over="ignore"):
        prod = {k: f32(v * f32(32767.0)) for k, v in vals.items() if np.isfinite(v)}
    # what the set contains: exact ties to an even and to an odd value in both signs, the products either side of +-32767
    for name, k in (("tie_even_pos", 1000), ("tie_odd_pos", 1001), ("tie_small_even", 2), ("tie_small_odd", 1), ("tie_top_pos", 32766)):
        assert float(prod[name]) == k + 0.5
    for name, k in (("tie_even_neg", 1000), ("tie_odd_neg", 1001), ("tie_top_neg", 32766)):
        assert float(prod[name]) == -(k + 0.5)
    assert prod["below_one"] < f32(32767.0) == prod["one"] < prod["above_one"]
    assert prod["below_minus_one"] < f32(-32767.0) == prod["minus_one"] < prod["above_minus_one"]
    tiny = np.finfo(np.float32).tiny
    assert 0 < vals["subnormal_min"] < vals["subnormal_max"] < tiny == vals["normal_min"] and vals["subnormal_neg"] < 0
    assert np.signbit(vals["minus_zero"]) and not np.signbit(vals["zero"]) and vals["minus_zero"] == 0
    assert vals["flt_max"] == np.finfo(np.float32).max == -vals["minus_flt_max"] and np.isposinf(vals["inf"]) and np.isneginf(vals["minus_inf"])
    assert np.isnan(vals["nan"]) and vals["half_below"] < vals["half"] < vals["half_above"] and float(prod["half"]) == 0.5
    want = dict(tie_even_pos=1000, tie_odd_pos=1002, tie_even_neg=-1000, tie_odd_neg=-1002, tie_small_even=2, tie_small_odd=2, tie_top_pos=32766,
                tie_top_neg=-32766, below_one=32767, one=32767, above_one=32767, below_minus_one=-32767, minus_one=-32767, above_minus_one=-32767,
                subnormal_min=0, subnormal_max=0, subnormal_neg=0, normal_min=0, normal_min_neg=0, zero=0, minus_zero=0, flt_max=32767,
                minus_flt_max=-32767, inf=32767, minus_inf=-32767, nan=0, half_below=0, half=0, half_above=1, half_neg_below=-1, half_neg=0,
                half_neg_above=0)
    assert set(want) == set(vals)
    for name, v in vals.items():
        assert L.sim_mp2_enc_pcm_s16(float(v)) == want[name] == int(ref.pcm_s16(v)), name
    # every sample of the stream, and every named value is in it, in both channels
    x = inputs.conversion(48000)
    got = np.array([L.sim_mp2_enc_pcm_s16(float(v)) for v in x.reshape(-1)], np.int64).reshape(x.shape)
    assert np.array_equal(got, ref.pcm_s16(x))
    bits = x.view(np.uint32)
    for name, v in vals.items():
        for ch in range(2):
            assert (bits[:, ch, :] == np.float32(v).view(np.uint32)).sum() >= 6, name


# ------------------------------------------------------------------------------------------------ the padding period and the store

def _plan(cfg, calls):
    """the closed-form plan of chained calls ([call][stream] frame counts): [(call, stream, ordinal, begin, end, tail)] per frame"""
    done, out = [0] * len(calls[0]), []
    for c, call in enumerate(calls):
        at = 0
        for s, n in enumerate(call):
            base = at - ref.frame_offset(cfg[0], cfg[2], done[s])
            for f in range(n):
                o = done[s] + f
                out.append([c, s, o, base + ref.frame_offset(cfg[0], cfg[2], o), base + ref.frame_offset(cfg[0], cfg[2], o + 1), 0])
            if n:
                at = out[-1][4]
                out[-1][5] = -at % 16
                at += out[-1][5]
            done[s] += n
    return out


def test_period_calls_reach_every_store_alignment():
    """from the closed-form plan alone: begin mod 4 takes 0..3, (begin mod 4, end mod 4) takes every combination the 49-frame
    period offers, the tails behind the streams take every length 0..15 -- for a setting with an odd b and one with an even b"""
    assert [144000 * ref.KBPS[br - 1] // 44100 % 2 for _, _, br in inputs.PERIOD_SETTINGS] == [1, 0]
    for cfg in inputs.PERIOD_SETTINGS:
        counts = inputs.period_counts(cfg)
        assert counts[0] == 50 and len(counts) == 16 and max(counts[1:]) <= 32, counts    # (streams of 1..16 frames do not give every tail at b = 417)
        off = [ref.frame_offset(cfg[0], cfg[2], n) for n in range(99)]
        assert [off[n + 50] - off[n + 49] for n in range(49)] == [off[n + 1] - off[n] for n in range(49)]      # the period is 49
        assert len({off[n + 1] - off[n] for n in range(49)}) == 2
        offered = {(off[n] % 4, off[n + 1] % 4) for n in range(49)}
        unchained = _plan(cfg, [counts])
        assert {(b % 4, e % 4) for _, s, _, b, e, _ in unchained if s == 0} == offered
        assert {b % 4 for _, _, _, b, _, _ in unchained} == {0, 1, 2, 3}
        tails = {t for c, s, o, b, e, t in unchained if o + 1 == counts[s]}
        assert tails == set(range(16)), sorted(tails)
        chained = _plan(cfg, inputs.chain_calls(counts))
        assert {b % 4 for _, _, _, b, _, _ in chained} == {0, 1, 2, 3}

@pytest.mark.parametrize("cfg", inputs.PERIOD_SETTINGS, ids=[inputs.setting_id(c) for c in inputs.PERIOD_SETTINGS])
def test_period_stream_and_its_chained_pieces(cfg, libs):
    """50 frames, one past the padding period: restatement = simulator; streams with every tail in one call (sim_encode asserts
    the zeros between streams and the untouched bytes behind the total); chained calls of 1, 7, 41 and 1 frames give the same
    streams; the simulator's ranges are the closed-form plan's"""
    counts = inputs.period_counts(cfg)
    xs = inputs.period_streams(cfg)
    whole, stats = sim_encode(cfg, xs)
    assert whole[0] == ref.encode(cfg, xs[0])[0]
    plan = _plan(cfg, [counts])
    assert [len(w) for w in whole] == [ref.frame_offset(cfg[0], cfg[2], n) for n in counts] and len(stats) == len(plan) == sum(counts)
    sizes = oracle_decode(libs, whole[0])[1]
    assert sizes == [ref.frame_bytes(cfg[0], cfg[2], n) for n in range(50)] and len(set(sizes)) == 2
    for x, w in zip(xs[1:], whole[1:]):
        assert w == sim_encode(cfg, [x])[0][0]
    state, done, pieces = SimState(len(xs)), [0] * len(xs), [b""] * len(xs)
    for call in inputs.chain_calls(counts):
        got, _ = sim_encode(cfg, [x[d:d + n] for x, d, n in zip(xs, done, call)], chain=True, state=state)
        pieces = [p + g for p, g in zip(pieces, got)]
        done = [d + n for d, n in zip(done, call)]
    assert pieces == whole


# ------------------------------------------------------------------------------------------------ the sanitizers

def test_simulator_under_the_sanitizers_at_the_edges(tmp_path):
    """the stand-alone program (its own main, g++ -fsanitize=address,undefined; nothing is loaded into Python under a sanitizer):
    bounds(), dc(), conversion() and the other edge inputs at one setting per table, and the 50-frame stream whole and chained.
    UBSan on the 64-bit analysis at its bounds is the point."""
    cases, total = [], 0
    for cfg in ((1, 2, 14), (2, 2, 13), (1, 1, 2), (2, 1, 1)):
        xs = edge_pcm(inputs.RATES[cfg[0]])
        cases.append((cfg, [[len(xs[k]) for k in KINDS]], [xs[k] for k in KINDS]))
        total += sum(len(p) for p in simulated(cfg)[0])
    for cfg in inputs.PERIOD_SETTINGS:
        counts, xs = inputs.period_counts(cfg), inputs.period_streams(cfg)
        cases.append((cfg, [counts], xs))
        cases.append((cfg, inputs.chain_calls(counts), xs))
        total += 2 * sum(ref.frame_offset(cfg[0], cfg[2], n) for n in counts)
    path = str(tmp_path / "cases.bin")
    write_cases(path, cases)
    r = subprocess.run([sim_main(), path], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    words = r.stdout.split()
    assert words[:2] == ["cases", str(len(cases))] and int(words[3]) == total
