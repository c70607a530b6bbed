"""The log-mel rule at the edges the kernel's dispatch has (tests/logmel_inputs.py: twelve shapes, one per path of lm_wg_dft /
lm_tiles), without a GPU: the proof that the lattice covers those paths, the simulator against torch.stft in float64 under the
periodic Hann window and under a rising one, the live bands, the tables, chains in pieces down to single samples and with a
carry at its cap, non-finite, tiny and huge samples -- and the chain cases under the sanitizers.  The device file
(test_gpu_logmel_edges.py) compares k_logmel with this simulator bit for bit; what anchors the simulator is here."""
import os
import subprocess

import numpy as np
import pytest

import logmel_ref as ref
from logmel_inputs import CHAIN_SHAPES, DTYPE_NAMES, IDS, LATTICE, LAYOUT_NAMES, LIVE_BANDS, NUMBERS, REQUIRED, VALUE_IDS, VALUE_SHAPES, WINDOWS, all_configs, carry_split, \
    chain_row, coverage, dispatch, edge_splits, lattice_output, rising, shape, stream_lengths, window_of
from logmel_util import CONFIGS, F, SimState, frames_axis, sim_basis, sim_features, sim_filters, sim_main, sim_rule, sim_scale, write_cases
from test_logmel_sim import bits, lm, neighbours, noise, run_pieces, same_bits  # noqa: F401  (lm: the fixture)


# ------------------------------------------------------------------ the coverage proof
def test_the_lattice_and_the_configs_cover_every_path_of_the_dispatch():
    """every item is the reason for a row of the lattice: whoever edits it reads here what was lost"""
    missing = [item for item in REQUIRED if item not in coverage(all_configs())]
    assert not missing, missing
    # ... and the existing configs alone do not: these are the paths no device test had run
    old = coverage(CONFIGS.values())
    assert {("tail", 1), ("tail", 2), ("tail", 3), ("group", (0, 2)), ("group", (1, 2)), ("group", (1, 3)), ("full", True)}.isdisjoint(old)
    assert not any(("hop_class", c) in old for c in (2, 4, 6, 9))


def test_each_row_reaches_what_it_is_there_for():
    d = {k: dispatch(sim_rule(**LATTICE[k])) for k in NUMBERS}
    assert [d[k]["tail"] for k in (1, 2, 3, 4, 6)] == [1, 2, 3, 3, 3]
    assert [d[k]["hop_class"] for k in NUMBERS] == ["odd", "odd", "2mod4", 2, 6, 2, 4, "odd", "2mod4", 2, 9, "2mod4"]
    assert d[5]["groups"] == {(0, 2), (0, 1)} and d[6]["groups"] == {(0, 2)} and d[7]["groups"] == {(0, 3), (0, 2)}
    assert d[8]["groups"] == {(0, 4), (1, 1)} and d[9]["groups"] == {(0, 4), (1, 2)} and d[10]["groups"] == {(0, 4), (1, 3)}
    assert d[11]["groups"] == {(0, 4), (1, 4), (2, 1)} and d[12]["groups"] == {(0, 4), (1, 4)}
    assert [k for k in NUMBERS if d[k]["full"]] == [4, 6, 8, 9, 10, 12]      # n_fft + 2 a multiple of 32
    assert 4 * sim_rule(**LATTICE[11])["lds_floats"] == 133380 and 4 * sim_rule(**LATTICE[12])["lds_floats"] == 132992
    assert LATTICE[2]["n_mels"] * F < 256                           # fewer items than threads in lm_wg_mel
    combos = [lattice_output(k, end, w)[:2] for k in NUMBERS for end in (True, False) for w in WINDOWS]
    assert all(combos.count((t, lay)) >= 2 for t in DTYPE_NAMES for lay in LAYOUT_NAMES)
    assert all(lattice_output(k, e, w)[1] == "time_major" for k in (1, 2) for e in (True, False) for w in WINDOWS)
    assert all("float32" in [lattice_output(k, e, w)[0] for e in (True, False) for w in WINDOWS] for k in NUMBERS)


# ------------------------------------------------------------------ tables
@pytest.mark.parametrize("number", VALUE_SHAPES, ids=VALUE_IDS)
def test_basis_and_filters_within_one_neighbour_of_float64_and_equal_to_the_simulators(lm, number):
    """n_fft = 34, 38, 62 .. have almost no exact quarter turns, where the existing shapes have many"""
    cfg = shape(number)
    n_fft = cfg["n_fft"]
    for name in WINDOWS:
        w = window_of(name, n_fft)
        got = lm.basis(window=w, **cfg)
        want = ref.basis(n_fft, None if w is None else w.astype(np.float64))
        assert got.shape == (n_fft, sim_rule(**cfg)["cols"]) and 0 <= got.shape[1] - want.shape[1] < 32
        assert neighbours(got[:, :want.shape[1]], want).all() and not got[:, want.shape[1]:].any()
        assert same_bits(got, sim_basis(window=w, **cfg))
    fb, rg = lm.filters(**cfg)
    want = ref.filters(cfg["sample_rate"], n_fft, cfg["n_mels"], 0.0, 0.0, cfg["mel_scale"], cfg["mel_norm"])
    assert fb.shape == want.shape and neighbours(fb, want).all()
    sfb, srg = sim_filters(**cfg)
    assert same_bits(fb, sfb) and np.array_equal(rg, srg)
    assert int((rg[:, 1] > rg[:, 0]).sum()) == LIVE_BANDS.get(number, cfg["n_mels"])


# ------------------------------------------------------------------ values
@pytest.mark.parametrize("name", WINDOWS)
@pytest.mark.parametrize("number", VALUE_SHAPES, ids=VALUE_IDS)
def test_values_against_torch_stft_in_float64(number, name, capsys):
    """test_logmel_sim's method and its derived bound (logmel_ref.mel_bound, unscaled) at the twelve shapes; live bands only, the
    empty ones hold the pad value bit for bit"""
    cfg = shape(number)
    n_fft, hop, n_mels = cfg["n_fft"], cfg["hop"], cfg["n_mels"]
    w = window_of(name, n_fft)
    w64 = None if w is None else w.astype(np.float64)
    fb64 = ref.filters(cfg["sample_rate"], n_fft, n_mels, 0.0, 0.0, cfg["mel_scale"], cfg["mel_norm"])
    _, rg = sim_filters(**cfg)
    live = rg[:, 1] > rg[:, 0]
    assert int(live.sum()) == LIVE_BANDS.get(number, n_mels)
    x = noise(5 * hop + n_fft, 4)
    mel, re, im = ref.mel_float64(x, n_fft, hop, fb64, w64)
    bound = ref.mel_bound(x, n_fft, hop, fb64, rg, re, im, w64)
    if not live.all():
        empty = frames_axis(sim_features([x], end=True, scale="db", window=w, **cfg)[0], "mel_major")[0, :len(mel), ~live]
        assert not mel[:, ~live].any() and same_bits(empty, np.full_like(empty, sim_scale("db", 1e-10, np.zeros(1, np.float32))[0]))
    mel, bound = mel[:, live], bound[:, live]
    assert mel.min() > 1e-10 and (bound < mel).all()                 # the reference alone stays clear of the clamp
    got, counts = sim_features([x], end=True, scale="power", window=w, **cfg)
    assert counts == [len(mel)]
    d = np.abs(frames_axis(got, "mel_major")[0, :counts[0], live].T.astype(np.float64) - mel)
    with capsys.disabled():
        print("\nlogmel shape %s, %s: worst difference / bound %.3g" % (number, name, (d / bound).max()))
    assert (d <= bound).all()


# ------------------------------------------------------------------ chains
@pytest.mark.parametrize("end", [False, True], ids=["open", "end"])
@pytest.mark.parametrize("number", CHAIN_SHAPES, ids=[IDS[k - 1] for k in CHAIN_SHAPES])
def test_pieces_equal_the_whole_bit_for_bit(number, end):
    """every split of chain_splits, the split whose carry is exactly n_fft - 1 samples and the split into single samples"""
    cfg = LATTICE[number]
    n_fft, hop = cfg["n_fft"], cfg["hop"]
    n, splits = edge_splits(n_fft, hop)
    N = carry_split(n_fft, hop)[0]
    assert N >= n_fft and N - max(0, min(ref.frames(N, False, n_fft, hop) * hop - n_fft // 2, N - 1 - n_fft // 2)) == n_fft - 1
    cfg = dict(cfg, scale="log10", row=chain_row(n_fft, hop), window=rising(n_fft))
    x = noise(n, 21)
    whole, counts = sim_features([x], end=end, **cfg)
    assert counts == [ref.frames(n, end, n_fft, hop)]
    wrong = []
    for split in splits:
        got, state = run_pieces([x], [[p] for p in split], end, cfg)
        if not same_bits(got[0], frames_axis(whole, "mel_major")[0, :counts[0]]):
            wrong.append(split if len(split) < 10 else "singles")
        assert (int(state.rec[0, 0]) & 0xffffffff) == (0 if end else 1) and (end or int(state.rec[0, 1]) == n)
    assert not wrong, wrong


# ------------------------------------------------------------------ non-finite, tiny and huge samples
def test_a_non_finite_sample_stays_in_the_frames_whose_window_covers_it():
    """one NaN, then one +inf, at sample 100 of a noise stream at shape 3 (n_fft 38, hop 6): frames 14 to 19 cover it.  NaN:
    exactly those frames are NaN in POWER and the pad value in DB (max(mel, floor) as `mel > floor ? mel : floor` answers floor
    for NaN).  +inf: inf times a basis entry is +-inf, so re and im of those frames are +-inf or NaN, the power +inf or NaN and
    no output of them is finite; DB is the pad value where the mel sum is NaN and the logarithm's value of +inf (128, times 10
    log10 2) where it is +inf.  Every other frame equals the clean stream's bit for bit."""
    cfg = LATTICE[3]
    clean = noise(40 * 6 + 38, 50)
    hit = np.arange(14, 20)
    pad = sim_scale("db", 1e-10, np.zeros(1, np.float32))[0]
    want_p, counts = sim_features([clean], scale="power", **cfg)
    want_db, _ = sim_features([clean], scale="db", **cfg)
    rest = np.setdiff1d(np.arange(counts[0]), hit)
    assert counts == [47]
    for bad in (np.nan, np.inf):
        x = clean.copy()
        x[100] = bad
        p, c = sim_features([x], scale="power", **cfg)
        db, _ = sim_features([x], scale="db", **cfg)
        assert c == counts
        assert same_bits(p[0][:, rest], want_p[0][:, rest]) and same_bits(db[0][:, rest], want_db[0][:, rest])
        assert same_bits(p[0][:, c[0]:], want_p[0][:, c[0]:])
        if bad is np.nan:
            assert np.isnan(p[0][:, hit]).all() and (bits(db[0][:, hit]) == bits(np.array([pad]))[0]).all()
        else:
            assert not np.isfinite(p[0][:, hit]).any() and np.isposinf(p[0][:, hit]).any()
            at_inf = sim_scale("db", 1e-10, np.array([np.inf], np.float32))[0]
            assert same_bits(db[0][:, hit], np.where(np.isnan(p[0][:, hit]), pad, at_inf).astype(np.float32)) and np.isfinite(db).all()


def test_tiny_samples_give_subnormal_powers_and_huge_ones_a_finite_db():
    cfg = LATTICE[3]
    x = noise(40 * 6 + 38, 51, 1.0)
    p, c = sim_features([x * np.float32(1e-21)], scale="power", **cfg)
    live = p[0][:, :c[0]]
    assert c == [47] and (live > 0).all() and (live < np.finfo(np.float32).tiny).all()
    p, _ = sim_features([x * np.float32(3e18)], scale="power", **cfg)
    assert np.isposinf(p).any() and not np.isnan(p).any()             # some powers overflow; the mel sum makes no NaN of them
    db, _ = sim_features([x * np.float32(3e18)], scale="db", **cfg)
    assert np.isfinite(db).all() and db[0][:, :c[0]].min() > 300.0


# ------------------------------------------------------------------ sanitizers
def test_stand_alone_program_is_clean_under_the_sanitizers_at_the_edge_chains(tmp_path):
    """ASan + UBSan over the simulator's stand-alone program: the chain cases of shapes 1 to 4, the n_fft - 1 carry and the
    single-sample split included; inputs in buffers of exactly the samples' size, outputs of exactly the call's size; nothing is
    preloaded"""
    cases = []
    for number in (1, 2, 3, 4):
        cfg = LATTICE[number]
        n, splits = edge_splits(cfg["n_fft"], cfg["hop"])
        x = noise(n, 60 + number)
        for end in (0, 1):
            for i, split in enumerate(splits):
                out = dict(cfg, row=chain_row(cfg["n_fft"], cfg["hop"]), layout=LAYOUT_NAMES[i & 1], dtype=DTYPE_NAMES[i % 3], scale=("log10", "db", "power")[i % 3])
                cases.append((out, end, [[p] for p in split], [x]))
    path = os.path.join(str(tmp_path), "cases.bin")
    write_cases(path, cases)
    r = subprocess.run([sim_main(), path], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-3000:]
    assert r.stdout.startswith("cases %d bytes " % len(cases))


def test_stream_lengths_sit_on_the_tiles_edges():
    for number in NUMBERS:
        n_fft, hop = LATTICE[number]["n_fft"], LATTICE[number]["hop"]
        frames = [ref.frames(n, True, n_fft, hop) for n in stream_lengths(n_fft, hop)]
        assert frames[:2] == [0, 0] and frames[2] == (n_fft // 2 + 1) // hop + 1
        assert frames[-4:] == [F - 1, F, F + 1, 2 * F + 1] if n_fft <= 256 else frames[3:] == [F, F + 1]
