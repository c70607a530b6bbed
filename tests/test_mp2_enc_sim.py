"""The MP2 encoder's rule (jsmpeg_amd/csrc/mp2_enc.h) without a GPU: the kernel's own per-lane functions, compiled by g++ into
a TEST-ONLY simulator (tests/sim/sim_mp2_enc.cpp), against the numpy restatement (tests/mp2_enc_ref.py), the oracle decoder,
a float64 filterbank, an exhaustive quantiser and the float64 yardstick of tools/mp2_enc_quality.py.  Launch shapes, LDS and
the host runtime are covered by tests/test_gpu_mp2_encode.py."""
import ctypes
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
import mp2_enc_inputs as inputs
import mp2_enc_ref as ref
from mp2_enc_util import SimState, oracle_decode, sim_encode, sim_lib, sim_main, write_cases

sys.path.insert(0, os.path.join(ROOT, "tools"))
import mp2_enc_bounds      # noqa: E402
import mp2_enc_quality     # noqa: E402

CASES = inputs.cases()
CASE_IDS = ["%s-%s" % c for c in CASES]


@functools.lru_cache(maxsize=None)
def encoded(name, kind):
    """one (configuration, input) through the simulator: (x, bytes, stats, S, dbg) -- computed once, shared, never changed"""
    cfg = inputs.CONFIGS[name]
    x = inputs.pcm(kind, inputs.RATES[cfg[0]], 3)
    (data,), stats, S, dbg = sim_encode(cfg, [x], want_debug=True)
    return x, data, stats, S, dbg


@functools.lru_cache(maxsize=None)
def restated(name, kind):
    infos = []
    data, _ = ref.encode(inputs.CONFIGS[name], inputs.pcm(kind, inputs.RATES[inputs.CONFIGS[name][0]], 3), infos=infos)
    return data, infos


@pytest.mark.parametrize("name,kind", CASES, ids=CASE_IDS)
def test_restatement_and_simulator_write_the_same_bytes(name, kind):
    assert encoded(name, kind)[1] == restated(name, kind)[0]


@pytest.mark.parametrize("name,kind", CASES, ids=CASE_IDS)
def test_oracle_decodes_every_frame_at_its_closed_form_size(name, kind, libs):
    cfg = inputs.CONFIGS[name]
    _, data, _, _, _ = encoded(name, kind)
    pcm, sizes = oracle_decode(libs, data)
    assert len(pcm) == 3 and sizes == [ref.frame_bytes(cfg[0], cfg[2], n) for n in range(3)] and sum(sizes) == len(data)
    if kind == "silence":                            # header, allocation of zeros, nothing else: decodes to zeros
        at = 0
        for n in sizes:
            assert data[at:at + 2] == b"\xff\xfd" and not any(data[at + 4:at + n])
            at += n
        assert not pcm.any()


def test_settings_iso_forbids_are_refused():
    L = sim_lib()
    for sr in range(3):
        for br in range(1, 15):
            for ch in (1, 2):
                assert (L.sim_mp2_enc_rule(sr, ch, br, None) < 0) == ref.refused(sr, ch, br)
    assert [ref.KBPS[br - 1] for br in range(1, 15) if ref.refused(0, 2, br)] == [32, 48, 56, 80]
    assert [ref.KBPS[br - 1] for br in range(1, 15) if ref.refused(0, 1, br)] == [224, 256, 320, 384]
    for bad in ((3, 2, 10), (0, 3, 10), (0, 0, 10), (0, 2, 0), (0, 2, 15)):
        assert L.sim_mp2_enc_rule(*bad, None) < 0


def _branch(high, sb, code):
    """which branch of mp2_steps an allocation code takes"""
    if not high:
        return ("low", code if code in (1, 2, 3, 15) else "2^n")
    if sb < 3:
        return ("high<3", 1 if code == 1 else "2^n")
    if sb < 11:
        return ("high<11", 15 if code == 15 else ("odd" if code < 5 else "2^n"))
    if sb < 23:
        return ("high<23", 7 if code == 7 else ("odd" if code < 5 else "2^n"))
    return ("high>=23", 3 if code == 3 else "odd")


def test_the_configurations_reach_every_steps_branch_and_table():
    want = {("low", 1), ("low", 2), ("low", 3), ("low", 15), ("low", "2^n"), ("high<3", 1), ("high<3", "2^n"), ("high<11", 15),
            ("high<11", "odd"), ("high<11", "2^n"), ("high<23", 7), ("high<23", "odd"), ("high<23", "2^n"), ("high>=23", 3), ("high>=23", "odd")}
    seen, tables = set(), set()
    for name, kind in CASES:
        cfg = inputs.CONFIGS[name]
        sblimit, high = ref.table_select(*cfg)
        tables.add((sblimit, high))
        dbg = encoded(name, kind)[4]
        for f in range(3):
            for q in range(64):
                if dbg[f, q, 0]:
                    seen.add(_branch(high, q >> 1, int(dbg[f, q, 0])))
    assert tables == {(8, 0), (12, 0), (27, 1), (30, 1)}
    assert seen == want, want - seen


def test_tables_window_sums_and_cosines():
    L = sim_lib()
    win, cos = np.zeros(512, np.int32), np.zeros(128, np.int32)
    L.sim_mp2_enc_tables(ctypes.c_void_p(win.ctypes.data), ctypes.c_void_p(cos.ctypes.data))
    assert np.array_equal(win, ref.W) and np.array_equal(cos, np.rint(32768.0 * np.cos(np.arange(128) * np.pi / 64.0)).astype(np.int64))
    assert subprocess.call([sys.executable, os.path.join(ROOT, "tools", "gen_mp2_enc_cos.py"), "--check"]) == 0
    b = mp2_enc_bounds.bounds()
    assert b["window_tap_sum"] <= 92686 and b["window_sum"] == 5574752 == int(np.abs(ref.W).sum())
    assert b["y_bits"] == 33 and b["acc_below_2_53"] and b["s_below_2_25"]
    for i in range(63):
        assert L.sim_mp2_enc_scale_index(0) == 62
        sf = ref.scalefactor(i)
        assert L.sim_mp2_enc_scale_index(sf // 2) == i and L.sim_mp2_enc_scale_index(sf // 2 + 1) == max(0, i - 1)
    assert [L.sim_mp2_enc_gain(s) for s in (0, 3, 5, 7, 9, 15, 65535)] == [0, 48, 62, 72, 80, 96, 384] == [ref.gain(s) for s in (0, 3, 5, 7, 9, 15, 65535)]
    for x, want in ((0.0, 0), (1.0, 32767), (-1.0, -32767), (7.0, 32767), (float("inf"), 32767), (float("-inf"), -32767), (float("nan"), 0),
                    (0.5 / 32767, 0), (1.5 / 32767, 2), (2.5 / 32767, 2), (-1.5 / 32767, -2)):
        assert L.sim_mp2_enc_pcm_s16(x) == want == int(ref.pcm_s16(np.float32(x))), x


@pytest.mark.parametrize("name", list(inputs.CONFIGS))
def test_filterbank_against_float64(name):
    """S / 2^23 against ISO's analysis in float64 with the same window values, within the bound tools/mp2_enc_bounds.py derives
    from the cosines' rounding and the final shift (derived, not measured)"""
    cfg = inputs.CONFIGS[name]
    bound = mp2_enc_bounds.bounds()["s_error_units"] + 1e-3          # + the float64 sum's own error, far below a unit
    cosm = np.array([[np.cos((2 * k + 1) * (i - 16) * np.pi / 64.0) for i in range(64)] for k in range(32)])
    C = ref.W.astype(np.float64) / 2.0 ** 21
    worst = 0.0
    for kind in ("sine", "noise", "square", "wild"):
        x, _, _, S, _ = encoded(name, kind)
        s16 = ref.pcm_s16(x).astype(np.float64) / 2.0 ** 15
        for ch in range(cfg[1]):
            track = np.concatenate([np.zeros(480), s16[:, ch, :].reshape(-1)])
            for f in range(3):
                idx = 1152 * f + 480 + 32 * np.arange(36)[:, None] + 31 - np.arange(512)[None, :]
                want = ((C[None, :] * track[idx]).reshape(36, 8, 64).sum(axis=1) @ cosm.T) * 2.0 ** 23
                worst = max(worst, float(np.abs(S[f, ch] - want).max()))
    print("filterbank %s: worst |S - float64| = %.2f units, bound %.2f" % (name, worst, bound))
    assert worst <= bound


ALL_STEPS = (3, 5, 7, 9) + tuple((1 << n) - 1 for n in range(4, 16)) + (65535,)


def test_quantiser_is_the_exhaustive_argmin():
    L = sim_lib()
    rng = np.random.RandomState(7)
    checked = 0
    for steps in ALL_STEPS:
        for index in (0, 1, 2, 30, 62):
            sf = ref.scalefactor(index)
            codes = np.arange(steps)
            lv = 256 * ref.requantise(codes, steps, sf)
            for c in (0, 1, steps // 2, steps - 1):
                assert L.sim_mp2_enc_requantise(int(c), steps, sf) * 256 == lv[c]
            picks = rng.randint(0, steps, 6)
            samples = [0, 1, -1, sf // 2, -(sf // 2), sf, -sf, 1 << 24, -(1 << 24)] + [int(v) for v in rng.randint(-sf // 2 - 300, sf // 2 + 300, 12)]
            samples += [int(lv[c]) + d for c in picks for d in (-129, -128, -127, 0, 127, 128, 129)]
            samples += [int(lv[c] + lv[c + 1]) // 2 + d for c in picks if c + 1 < steps for d in (-1, 0, 1)]
            for S in samples:
                want = int(np.argmin(np.abs(lv - S)))                # the first of equal minima: the lower code
                assert L.sim_mp2_enc_quantise(S, steps, sf) == want == int(ref.quantise(np.array([S]), steps, index)[0]), (steps, index, S)
                checked += 1
    assert checked > 5000


@pytest.mark.parametrize("name,kind", CASES, ids=CASE_IDS)
def test_coded_samples_lie_within_half_a_step(name, kind):
    """every coded sample: |256 requantise(code) - S| <= half a quantiser step plus one unit of the decoder's domain (its
    requantiser truncates), unless the code was clamped at either end"""
    _, infos = restated(name, kind)
    n = 0
    for info in infos:
        for (sb, ch), codes in info["codes"].items():
            steps = ref.steps_of(info["high"], sb, info["code"][sb, ch])
            for part in range(3):
                sf = ref.scalefactor(info["idx"][sb, ch][part])
                c = codes[12 * part:12 * part + 12]
                S = info["S"][ch, 12 * part:12 * part + 12, sb]
                err = np.abs(256 * ref.requantise(c, steps, sf) - S)
                step = 256.0 * ({3: 16384, 5: 10922, 9: 6553}.get(steps, 65536 >> ref.code_bits(steps))) * sf / 2.0 ** 24
                free = (c > 0) & (c < steps - 1)
                assert (err[free] <= step / 2 + 256).all(), (sb, ch, part)
                n += int(free.sum())
    assert n or kind == "silence"


@pytest.mark.parametrize("name,kind", CASES, ids=CASE_IDS)
def test_allocation_properties(name, kind):
    cfg = inputs.CONFIGS[name]
    sblimit, high = ref.table_select(*cfg)
    _, data, stats, _, dbg = encoded(name, kind)
    for f in range(3):
        size = ref.frame_bytes(cfg[0], cfg[2], f)
        pairs, used, left, top = (int(v) for v in stats[f])
        assert used <= 8 * size and left == 8 * size - used
        assert pairs == int((dbg[f, :, 0] != 0).sum()) and top == int(dbg[f, :, 0].max())
        for q in range(64):
            code, loud, nsf = int(dbg[f, q, 0]), int(dbg[f, q, 4]), int(dbg[f, q, 5])
            sb, ch = q >> 1, q & 1
            if sb >= sblimit or ch >= cfg[1] or not loud:
                assert code == 0                                   # a silent pair (and a pair that is not there) has no bits
                continue
            if code < (1 << ref.nbal(high, sb)) - 1:               # the loop ended: its raise does not fit
                so, sn = ref.steps_of(high, sb, code), ref.steps_of(high, sb, code + 1)
                assert 12 * (ref.granule_bits(sn) - ref.granule_bits(so)) + (2 + 6 * nsf if code == 0 else 0) > left, (f, q)
        assert int(dbg[f, 0, 7]) <= 255 and restated(name, kind)[1][f]["rounds"] <= 540


def test_chain_pieces_are_the_stream_of_one_call(libs):
    """pieces of 1, 2, 1, 0, 3 frames per chained call, concatenated, are the 7-frame stream of one call at 44.1 kHz (both
    padding states); chain_reset restarts ordinal and history"""
    cfg = inputs.CONFIGS["stereo_44k_192"]
    x = inputs.pcm("noise", 44100, 7, seed=3)
    (whole,), _ = sim_encode(cfg, [x])
    assert {ref.frame_bytes(cfg[0], cfg[2], n) for n in range(7)} == {626, 627}
    state = SimState(4)
    pieces, at = [], 0
    for n in (1, 2, 1, 0, 3):
        (p,), _ = sim_encode(cfg, [x[at:at + n]], numbers=[2], chain=True, state=state)
        pieces.append(p)
        at += n
        assert state.info(2) == (True, at) and state.info(0) == (False, 0)
    assert b"".join(pieces) == whole and pieces[3] == b""
    assert oracle_decode(libs, whole)[1] == [ref.frame_bytes(cfg[0], cfg[2], n) for n in range(7)]
    (unchained,), _ = sim_encode(cfg, [x[3:5]], numbers=[2], state=state)                    # an unchained call touches no state
    assert unchained == sim_encode(cfg, [x[3:5]])[0][0] and state.info(2) == (True, 7)
    state.reset(2)
    (again,), _ = sim_encode(cfg, [x[:2]], numbers=[2], chain=True, state=state)
    assert again == whole[:len(again)] and state.info(2) == (True, 2)
    mono = inputs.CONFIGS["mono_44k_192"]
    (whole,), _ = sim_encode(mono, [x])
    state = SimState(1)
    assert b"".join(sim_encode(mono, [x[a:b]], chain=True, state=state)[0][0] for a, b in ((0, 3), (3, 4), (4, 7))) == whole


def test_several_streams_in_one_call():
    cfg = inputs.CONFIGS["stereo_44k_128"]
    xs = [inputs.pcm(k, 44100, n, seed=i) for i, (k, n) in enumerate((("sine", 3), ("noise", 0), ("square", 1), ("wild", 2), ("sweep", 3)))]
    pieces, stats = sim_encode(cfg, xs, numbers=[0, 2, 3, 5, 6])
    assert [len(p) for p in pieces] == [sum(ref.frame_bytes(cfg[0], cfg[2], n) for n in range(len(x))) for x in xs]
    for x, p in zip(xs, pieces):
        assert p == (sim_encode(cfg, [x])[0][0] if len(x) else b"")
    assert len(stats) == 9


@functools.lru_cache(maxsize=None)
def _yardstick():
    return json.load(open(os.path.join(ROOT, "profiles", "mp2_enc_bounds.json")))


def test_round_trip_lag_is_481_everywhere(libs):
    """decode(encode(x)) against x: the largest cross-correlation lies at ONE lag for every configuration, with positive sign"""
    lags = set()
    for name, cfg in inputs.CONFIGS.items():
        x, data, _, _, _ = encoded(name, "noise")
        pcm, _ = oracle_decode(libs, data)
        a = mp2_enc_quality.clean(x[:, 0, :]).reshape(-1)
        d = pcm[:, 0, :].reshape(-1).astype(np.float64)
        corr = [float(np.dot(a[:len(a) - lag], d[lag:])) for lag in range(0, 1200)]
        lag = int(np.argmax(np.abs(corr)))
        assert corr[lag] > 0
        lags.add(lag)
    assert lags == {481} and _yardstick()["lag_samples"] == 481


@pytest.mark.parametrize("name,kind", CASES, ids=CASE_IDS)
def test_round_trip_snr_against_the_float64_yardstick(name, kind, libs):
    """the integer encoder's SNR through the oracle decoder is at least the float64 restatement's (tools/mp2_enc_quality.py,
    profiles/mp2_enc_bounds.json) minus 1 dB"""
    cfg = inputs.CONFIGS[name]
    x, data, _, _, _ = encoded(name, kind)
    pcm, _ = oracle_decode(libs, data)
    got = mp2_enc_quality.snr_db(x, pcm, cfg[1])
    want = _yardstick()["float64_snr_db"]["%s/%s" % (name, kind)]
    print("round trip %s/%s: %s dB, float64 yardstick %s dB" % (name, kind, None if got is None else round(got, 2), want))
    if kind == "silence":
        assert got is None and want is None and not pcm.any()
    else:
        assert got >= want - 1.0


def test_python_module(hip_lib):
    from jsmpeg_amd import build, mp2_encode
    L = mp2_encode.lib()
    for s in mp2_encode.SYMBOLS:
        assert getattr(L, s)
    S = sim_lib()
    for name, (sr, ch, br) in inputs.CONFIGS.items():
        for n in (0, 1, 2, 48, 49, 440, 441, 44099, 44100, 10 ** 6, 2 ** 32 - 2):
            assert mp2_encode.frame_offset(n, sr, br) == ref.frame_offset(sr, br, n) == S.sim_mp2_enc_frame_offset(sr, ch, br, n)
            assert mp2_encode.frame_bytes(n, sr, br) == ref.frame_bytes(sr, br, n) == S.sim_mp2_enc_frame_bytes(sr, ch, br, n)
            assert mp2_encode.default_pts(n, inputs.RATES[sr]) == ref.default_pts(n, inputs.RATES[sr]) == S.sim_mp2_enc_default_pts(sr, ch, br, n)
    assert mp2_encode.es_bytes([3, 0, 1], 0, 10) == 1888 + 0 + 640
    usage = build.check_kernel_resources()
    mine = [k for k in usage if "k_mp2e_frame" in k]
    assert mine and all(usage[k].get("ScratchSize", 0) == 0 for k in mine)


def test_simulator_under_the_sanitizers(tmp_path):
    """the stand-alone program (its own main, g++ -fsanitize=address,undefined): every (configuration, input) and the chain's
    pieces, each stream's samples in a buffer of exactly the frames' size; nothing is loaded into Python under a sanitizer"""
    cases = []
    for name, kind in CASES:
        cfg = inputs.CONFIGS[name]
        cases.append((cfg, [[3]], [inputs.pcm(kind, inputs.RATES[cfg[0]], 3)]))
    x = inputs.pcm("noise", 44100, 7, seed=3)
    y = inputs.pcm("sine", 44100, 4, seed=4)
    cases.append((inputs.CONFIGS["stereo_44k_192"], [[1, 2], [2, 0], [1, 1], [0, 0], [3, 1]], [x, y]))
    cases.append((inputs.CONFIGS["mono_44k_192"], [[3], [1], [3]], [x]))
    path = str(tmp_path / "cases.bin")
    write_cases(path, cases)
    r = subprocess.run([sim_main(), path], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    words = r.stdout.split()
    assert words[:2] == ["cases", str(len(cases))] and len(cases) == 58
    total = sum(len(encoded(n, k)[1]) for n, k in CASES)               # a chain's pieces add up to the stream of one call
    total += sum(len(p) for p in sim_encode(inputs.CONFIGS["stereo_44k_192"], [x, y])[0]) + len(sim_encode(inputs.CONFIGS["mono_44k_192"], [x])[0][0])
    assert int(words[3]) == total
