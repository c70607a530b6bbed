"""The log-mel rule (jsmpeg_amd/csrc/logmel.h, C ABI part 12) without a GPU: the library's tables against a float64 restatement
and against the simulator's, frame placement pinned by unit impulses, the closed-form counts, the simulator (tests/sim/
sim_logmel.cpp: the kernel's own per-lane bodies and the host's own plan, the DFT's chains in fmaf) against torch.stft in
float64 with a derived tolerance, the header's logarithm over every mantissa, chains in pieces, the narrow types, the scales,
the pad value, the refusals -- and under the sanitizers.  Every test here fails without the feature: the header, the module
and the library's jsmpeg_hip_logmel_* symbols do not exist."""
import os
import subprocess

import numpy as np
import pytest

import logmel_ref as ref
from logmel_util import CONFIGS, WHISPER, F, SimState, chain_splits, frames_axis, sim_basis, sim_features, sim_filters, sim_frames, sim_log2, sim_main, \
    sim_rule, sim_scale, write_cases

KEYS = list(CONFIGS)
IDS = ["%d_%d_%d" % k for k in KEYS]

# the header's lm_log2 against float64 np.log2: the maximum over all 2^23 mantissas of [1, 2), measured by
# test_the_logarithm_over_every_mantissa (5.58e-08) -- the polynomial's fit and its float32 evaluation.  At another exponent e
# the final fmaf rounds e + log2(m) once more: half a unit in the last place of the result on top.
LOG2_ERR = 5.6e-8


def log2_bound(l2):
    return LOG2_ERR + 2.0 ** -24 * np.abs(l2)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({2: np.uint16, 4: np.uint32}[a.dtype.itemsize])


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def neighbours(got, want64):
    """got is the float32 nearest to want64 or one of its two neighbours"""
    near = want64.astype(np.float32)
    lo, hi = np.nextafter(near, np.float32(-np.inf)), np.nextafter(near, np.float32(np.inf))
    return (got >= lo) & (got <= hi)


@pytest.fixture(scope="module")
def lm(hip_lib):
    from jsmpeg_amd import logmel
    return logmel


def noise(n, seed, amp=0.5):
    return (np.random.default_rng(seed).uniform(-1.0, 1.0, n) * amp).astype(np.float32)


# ------------------------------------------------------------------ tables
@pytest.mark.parametrize("key", KEYS, ids=IDS)
def test_basis_within_one_neighbour_of_float64_and_equal_to_the_simulators(lm, key):
    cfg = CONFIGS[key]
    n_fft = key[0]
    got = lm.basis(**cfg)
    want = ref.basis(n_fft)
    assert got.shape[0] == n_fft and got.shape[1] % 32 == 0 and 0 <= got.shape[1] - want.shape[1] < 32
    assert lm.plan(**cfg)["cols"] == got.shape[1] and lm.plan(**cfg)["bins"] == n_fft // 2 + 1
    assert neighbours(got[:, :want.shape[1]], want).all()
    assert not got[:, want.shape[1]:].any()
    assert same_bits(got, sim_basis(**cfg))


def test_a_user_window_is_folded_in_and_need_not_be_symmetric(lm):
    cfg = CONFIGS[(32, 8, 8)]
    w = np.linspace(0.1, 1.0, 32).astype(np.float32)
    got = lm.basis(window=w, **cfg)
    assert neighbours(got[:, :34], ref.basis(32, w.astype(np.float64))).all()
    assert same_bits(got, sim_basis(window=w, **cfg))
    assert not same_bits(got, lm.basis(window=w[::-1].copy(), **cfg))


@pytest.mark.parametrize("key", KEYS, ids=IDS)
@pytest.mark.parametrize("mel_scale,mel_norm", [("htk", "none"), ("slaney", "slaney"), ("htk", "slaney"), ("slaney", "none")])
def test_filters_within_one_neighbour_of_float64_and_equal_to_the_simulators(lm, key, mel_scale, mel_norm):
    cfg = dict(CONFIGS[key], mel_scale=mel_scale, mel_norm=mel_norm)
    fb, rg = lm.filters(**cfg)
    want = ref.filters(cfg["sample_rate"], key[0], key[2], cfg["f_min"], cfg["f_max"], mel_scale, mel_norm)
    assert fb.shape == want.shape and neighbours(fb, want).all()
    sfb, srg = sim_filters(**cfg)
    assert same_bits(fb, sfb) and np.array_equal(rg, srg)
    for m in range(key[2]):
        nz = np.nonzero(fb[m])[0]
        assert (rg[m, 0], rg[m, 1]) == ((nz[0], nz[-1] + 1) if len(nz) else (0, 0))


def test_whisper_filters_have_no_empty_band(lm):
    fb, rg = lm.filters(**WHISPER)
    assert fb.shape == (80, 201) and (rg[:, 1] > rg[:, 0]).all() and (fb.sum(axis=1) > 0).all()


# ------------------------------------------------------------------ indices
@pytest.mark.parametrize("key", [(400, 160, 80), (32, 8, 8)], ids=["400_160_80", "32_8_8"])
def test_unit_impulses_give_the_basis_entries_bit_for_bit(key):
    """a unit impulse at sample j makes re / im of every frame the entries B[k][c] of the rows k at which the frame (with both
    reflections, written here with np.pad) holds the impulse -- two rows where a reflection doubles it, summed in ascending k by
    the chain, which float32 addition restates exactly"""
    cfg = CONFIGS[key]
    n_fft, hop = key[0], key[1]
    h, n = n_fft // 2, 3 * hop + n_fft
    B = sim_basis(**cfg)[:, :2 * (h + 1)]
    for j in (0, 1, h, n - 1, n - 2):
        x = np.zeros(n, np.float32)
        x[j] = 1.0
        _, counts, dft = sim_features([x], end=True, want_dft=True, scale="power", **cfg)
        assert counts == [n // hop + 1]
        padded = np.pad(x, (h, h), mode="reflect")
        for t in range(counts[0]):
            want = np.zeros(2 * (h + 1), np.float32)
            for k in np.nonzero(padded[t * hop:t * hop + n_fft])[0]:
                want = want + B[k]                                 # float32: one rounding per step, as fmaf(1, b, acc)
            assert same_bits(dft[0, t].reshape(-1), want), (j, t)


# ------------------------------------------------------------------ counts
@pytest.mark.parametrize("key", [(400, 160, 80), (32, 8, 8), (512, 128, 128)], ids=["400_160_80", "32_8_8", "512_128_128"])
def test_counts_are_closed_form(lm, key):
    n_fft, hop = key[0], key[1]
    cfg = CONFIGS[key]
    for n in range(3 * n_fft + 1):
        for end in (False, True):
            want = ref.frames(n, end, n_fft, hop)
            assert sim_frames(n, end, **cfg) == want
            if n % 7 == 0 or n <= n_fft:
                assert lm.frames(n, end, n_fft=n_fft, hop=hop) == want
    # the simulator hands out exactly these, and torch agrees with the END form
    import torch
    for n in (n_fft // 2 + 1, n_fft, 2 * n_fft + 3):
        x = noise(n, n)
        assert sim_features([x], end=True, scale="power", **cfg)[1] == [ref.frames(n, True, n_fft, hop)] == \
            [torch.stft(torch.from_numpy(x), n_fft, hop_length=hop, window=torch.ones(n_fft), return_complex=True).shape[-1]]
        assert sim_features([x], end=False, scale="power", **cfg)[1] == [ref.frames(n, False, n_fft, hop)]
    assert sim_features([noise(n_fft // 2, 1)], end=True, scale="power", **cfg)[1] == [0]


# ------------------------------------------------------------------ values
def value_inputs(n_fft, n):
    """noise at amplitude 0.5; a sine on a bin, one between bins and DC, each over noise at 0.05 so that every band carries
    energy well above the bound (an on-bin sine under the periodic Hann window is exactly zero three bins away)"""
    t = np.arange(n)
    low = noise(n, 5, 0.05)
    return {"noise": noise(n, 4), "sine_on_bin": (0.5 * np.sin(2 * np.pi * 10 * t / n_fft)).astype(np.float32) + low,
            "sine_between": (0.5 * np.sin(2 * np.pi * 10.5 * t / n_fft)).astype(np.float32) + low, "dc": np.full(n, 0.4, np.float32) + low}


@pytest.mark.parametrize("key", KEYS, ids=IDS)
def test_values_against_torch_stft_in_float64(key, capsys):
    """the simulator against torch.stft in float64, the float64 filterbank and numpy's logs; the tolerance is derived per output
    from the test's own input (logmel_ref.mel_bound), through p, the mel sum and the logarithm, never tuned"""
    cfg = CONFIGS[key]
    n_fft, hop, n_mels = key
    fb64 = ref.filters(cfg["sample_rate"], n_fft, n_mels, cfg["f_min"], cfg["f_max"], cfg["mel_scale"], cfg["mel_norm"])
    _, rg = sim_filters(**cfg)
    live = rg[:, 1] > rg[:, 0]              # (512 bins of 31 Hz under 128 HTK bands: the lowest filter is narrower than a bin and empty)
    assert live.sum() >= n_mels - 1
    worst = {}
    for name, x in value_inputs(n_fft, 5 * hop + n_fft).items():
        mel, re, im = ref.mel_float64(x, n_fft, hop, fb64)
        bound = ref.mel_bound(x, n_fft, hop, fb64, rg, re, im)
        empty = frames_axis(sim_features([x], end=True, scale="db", **cfg)[0], "mel_major")[0, :len(mel), ~live]
        assert not mel[:, ~live].any() and same_bits(empty, np.full_like(empty, sim_scale("db", 1e-10, np.zeros(1, np.float32))[0]))
        mel, bound = mel[:, live], bound[:, live]
        assert mel.min() > 1e-10 and (bound < mel).all(), name          # the reference alone stays clear of the clamp
        got, counts = sim_features([x], end=True, scale="power", **cfg)
        assert counts == [len(mel)]
        d = np.abs(frames_axis(got, "mel_major")[0, :counts[0], live].T.astype(np.float64) - mel)
        worst[name, "power"] = (d / bound).max()
        assert (d <= bound).all(), (name, "power")
        for scale in ("log", "log10", "db"):
            got, _ = sim_features([x], end=True, scale=scale, **cfg)
            c = ref.LOG_SCALE[scale]
            want = c * np.log2(mel)
            tol = -c * np.log2(1.0 - bound / mel) + c * log2_bound(np.log2(mel) + 1.0) + 2.0 ** -23 * (np.abs(want) + 1.0)
            d = np.abs(frames_axis(got, "mel_major")[0, :counts[0], live].T.astype(np.float64) - want)
            worst[name, scale] = (d / tol).max()
            assert (d <= tol).all(), (name, scale)
    with capsys.disabled():
        print("\nlogmel %r: worst difference / bound: %s" % (key, ", ".join("%s %s %.3g" % (k[0], k[1], v) for k, v in worst.items())))


# ------------------------------------------------------------------ the logarithm
def test_the_logarithm_over_every_mantissa(capsys):
    m = (np.arange(1 << 23, dtype=np.uint32) | np.uint32(0x3f800000)).view(np.float32)
    err = np.abs(sim_log2(m).astype(np.float64) - np.log2(m.astype(np.float64))).max()
    with capsys.disabled():
        print("\nlm_log2 over [1, 2): max |error| %.4g" % err)
    assert 5.0e-8 < err <= LOG2_ERR                                        # the figure, not a margin
    step = np.arange(4096, dtype=np.uint32) * np.uint32(2048) + np.uint32(1023)
    for e in range(1, 255):
        v = (step | np.uint32(e << 23)).view(np.float32)
        want = np.log2(v.astype(np.float64))
        assert (np.abs(sim_log2(v).astype(np.float64) - want) <= log2_bound(want)).all(), e


def test_inputs_at_or_below_floor_give_exactly_the_scale_of_floor():
    for floor in (1e-10, 1e-5, 3.0):
        f32 = np.float32(floor)
        x = np.array([0.0, -1.0, f32, np.nextafter(f32, np.float32(0)), f32 * np.float32(0.5), 1e-38], np.float32)
        for scale in ("log", "log10", "db"):
            out = sim_scale(scale, floor, x)
            assert len(set(bits(out).tolist())) == 1
            assert abs(float(out[0]) - ref.LOG_SCALE[scale] * np.log2(float(f32))) <= 2e-6 * max(1.0, abs(float(out[0])))
            assert sim_scale(scale, floor, np.array([np.nextafter(f32, np.float32(np.inf)) * np.float32(1.01)], np.float32))[0] > out[0]
    assert same_bits(sim_scale("power", 1e-10, np.array([0.0, 0.25], np.float32)), np.array([0.0, 0.25], np.float32))


# ------------------------------------------------------------------ chains
def run_pieces(xs, calls, end, cfg, state=None, numbers=None):
    """xs: the streams; calls: per call the piece length of every stream.  The frames of every stream, call after call."""
    n_streams = len(xs)
    state = state or SimState(max(numbers or [n_streams - 1]) + 1, **cfg)
    done = [0] * n_streams
    out = [[] for _ in xs]
    for k, call in enumerate(calls):
        pieces = [xs[s][done[s]:done[s] + call[s]] for s in range(n_streams)]
        feats, counts = sim_features(pieces, numbers=numbers, chain=True, end=end and k + 1 == len(calls), state=state, **cfg)
        feats = frames_axis(feats, cfg.get("layout", "mel_major"))
        for s in range(n_streams):
            out[s].append(feats[s, :counts[s]])
            done[s] += call[s]
    assert done == [len(x) for x in xs]
    return [np.concatenate(o) for o in out], state


@pytest.mark.parametrize("end", [False, True], ids=["open", "end"])
@pytest.mark.parametrize("layout,dtype", [("mel_major", "float32"), ("time_major", "float16")])
@pytest.mark.parametrize("key", [(400, 160, 80), (32, 8, 8)], ids=["400_160_80", "32_8_8"])
def test_pieces_equal_the_whole_bit_for_bit(key, layout, dtype, end):
    n_fft, hop = key[0], key[1]
    n, splits = chain_splits(n_fft, hop)
    cfg = dict(CONFIGS[key], layout=layout, dtype=dtype, scale="log10", row=12)
    x, y = noise(n, 21), noise(n, 22)
    whole, counts = sim_features([x, y], end=end, **cfg)
    whole = frames_axis(whole, layout)
    assert counts == [ref.frames(n, end, n_fft, hop)] * 2
    for split in splits:
        got, state = run_pieces([x], [[p] for p in split], end, cfg)
        assert same_bits(got[0], whole[0, :counts[0]]), split
        assert (int(state.rec[0, 0]) & 0xffffffff) == (0 if end else 1) and (end or int(state.rec[0, 1]) == n)
    # two streams with different splits in the same calls
    a, b = splits[4], splits[-3]                                   # [2 hop, rest] and the single-sample pieces
    calls = [[a[0], b[0]], [0, b[1]], [a[1], b[2]], [0, b[3]], [0, b[4]], [0, b[5]]]
    got, _ = run_pieces([x, y], calls, end, cfg)
    assert same_bits(got[0], whole[0, :counts[0]]) and same_bits(got[1], whole[1, :counts[1]])
    # stream numbers, not places, carry the state
    got, _ = run_pieces([y], [[p] for p in splits[7]], end, cfg, numbers=[3])
    assert same_bits(got[0], whole[1, :counts[1]])


def test_an_unchained_call_touches_no_state_and_reset_starts_from_nothing():
    cfg = dict(WHISPER, scale="log10", row=12)
    n = 7 * 160 + 400
    x = noise(n, 23)
    state = SimState(1, **cfg)
    first, c1 = sim_features([x[:700]], chain=True, end=False, state=state, **cfg)
    rec, carry = state.rec.copy(), state.carry.copy()
    sim_features([noise(900, 24)], chain=False, end=True, state=state, **cfg)
    assert np.array_equal(rec, state.rec) and same_bits(carry, state.carry)
    second, c2 = sim_features([x[700:]], chain=True, end=True, state=state, **cfg)
    whole, c = sim_features([x], end=True, **cfg)
    assert same_bits(np.concatenate([first[0, :, :c1[0]], second[0, :, :c2[0]]], axis=1), whole[0, :, :c[0]])
    sim_features([x[:700]], chain=True, end=False, state=state, **cfg)
    state.reset(0)
    again, c3 = sim_features([x], chain=True, end=True, state=state, **cfg)
    assert c3 == c and same_bits(again, whole)


def test_the_carry_holds_fewer_than_n_fft_samples():
    """the rule of logmel.h: after N samples the carry keeps x[max(0, min(F hop - h, N - 1 - h)) .. N), at most n_fft - 1"""
    for key in KEYS:
        n_fft, hop = key[0], key[1]
        h = n_fft // 2
        assert sim_rule(**CONFIGS[key])["carry"] == n_fft
        for n in range(1, 3 * n_fft):
            keep0 = max(0, min(ref.frames(n, False, n_fft, hop) * hop - h, n - 1 - h))
            assert n - keep0 <= n_fft - 1


# ------------------------------------------------------------------ narrow types, scales, padding, refusals
def test_narrow_types_equal_torchs_cpu_cast():
    import torch
    x = noise(5 * 160 + 400, 30)
    for scale in ("power", "log10", "whisper"):
        f32, _ = sim_features([x], scale=scale, **WHISPER)
        for dtype, tt in (("float16", torch.float16), ("bfloat16", torch.bfloat16)):
            got, _ = sim_features([x], scale=scale, dtype=dtype, **WHISPER)
            want = torch.from_numpy(f32).to(tt).view(torch.int16).numpy().view(np.uint16)
            assert np.array_equal(bits(got), want), (scale, dtype)


@pytest.mark.parametrize("layout", ["mel_major", "time_major"])
def test_whisper_is_the_formula_over_the_log10_output_and_pads_hold_the_pad_value(layout):
    xs = [noise(5 * 160 + 400, 31), noise(300, 32, 0.01), noise(100, 33), np.zeros(0, np.float32)]
    cfg = dict(WHISPER, layout=layout, row=11)
    l10, counts = sim_features(xs, scale="log10", **cfg)
    wh, counts2 = sim_features(xs, scale="whisper", **cfg)
    assert counts == counts2 == [8, 2, 0, 0]
    l10, wh = frames_axis(l10, layout), frames_axis(wh, layout)
    floor10 = sim_scale("log10", 1e-10, np.zeros(1, np.float32))[0]
    for s, c in enumerate(counts):
        M = l10[s, :c].max() if c else floor10
        low = np.float32(M - np.float32(8.0))
        assert same_bits(wh[s, :c], (np.maximum(l10[s, :c], low) + np.float32(4.0)) * np.float32(0.25))
        assert (bits(wh[s, c:]) == bits(np.array([(low + np.float32(4.0)) * np.float32(0.25)], np.float32))[0]).all()
        assert (bits(l10[s, c:]) == bits(np.array([floor10]))[0]).all()
    for scale, pad in (("power", np.float32(0)), ("db", sim_scale("db", 1e-10, np.zeros(1, np.float32))[0]), ("log", sim_scale("log", 1e-10, np.zeros(1, np.float32))[0])):
        got, _ = sim_features(xs, scale=scale, **cfg)
        got = frames_axis(got, layout)
        for s, c in enumerate(counts):
            assert (bits(got[s, c:]) == bits(np.array([pad], np.float32))[0]).all()
    assert abs(float(floor10) + 10.0) < 1e-5
    # a frame of zeros gets the pad value
    z, cz = sim_features([np.zeros(400, np.float32)], scale="db", **cfg)
    assert cz == [3] and len(set(bits(z).reshape(-1).tolist())) == 1


def test_refusals(lm):
    x = noise(5 * 160 + 400, 34)
    assert sim_features([x], row=8, **WHISPER)[1] == [8]
    with pytest.raises(RuntimeError, match="-1$"):
        sim_features([x], row=7, **WHISPER)
    with pytest.raises(RuntimeError, match="-2000002"):
        sim_features([x], scale="whisper", chain=True, state=SimState(1, **WHISPER), **WHISPER)
    for bad in (dict(n_fft=401), dict(hop=201), dict(n_fft=30, hop=8), dict(n_fft=1026), dict(n_mels=0), dict(n_mels=257), dict(sample_rate=7999), dict(hop=0)):
        assert sim_rule(**dict(WHISPER, **bad)) is None, bad
        with pytest.raises(ValueError, match="n_fft even in 32 .. 1024"):
            lm.plan(**dict(WHISPER, **bad))
    with pytest.raises(ValueError, match="f_min < f_max"):
        lm.filters(**dict(WHISPER, f_max=9000.0))
    with pytest.raises(ValueError, match="scale"):
        lm.plan(**dict(WHISPER, scale="magnitude"))
    with pytest.raises(ValueError, match="window"):
        lm.basis(window=np.ones(399, np.float32), **WHISPER)

    class Wrong:
        form, dtype, channels, row, _numbers = "frames", "float32", 1, 0, []

        def device_out(self):
            raise AssertionError("not reached")
        stream_out = device_out
    half = Wrong()
    half.form, half.dtype = "waveform", "float16"
    for r in (Wrong(), half):
        with pytest.raises(ValueError, match="form='waveform' and dtype='float32'"):
            lm.LogMel.features(object.__new__(lm.LogMel), r)
    for name in lm.SYMBOLS:
        assert hasattr(lm.lib(), name), name


# ------------------------------------------------------------------ sanitizers, resources
def test_stand_alone_program_is_clean_under_the_sanitizers(tmp_path):
    """ASan + UBSan over the simulator's stand-alone program, the chain cases: inputs in buffers of exactly the samples' size,
    outputs of exactly the call's size; nothing is preloaded"""
    cases = []
    for key in ((400, 160, 80), (32, 8, 8)):
        n, splits = chain_splits(key[0], key[1])
        x, y = noise(n, 41), noise(n, 42)
        for end in (0, 1):
            for i, split in enumerate(splits):
                cfg = dict(CONFIGS[key], row=12, layout=("mel_major", "time_major")[i & 1], dtype=("float32", "float16", "bfloat16")[i % 3], scale=("log10", "db", "power")[i % 3])
                cases.append((cfg, end, [[p] for p in split], [x]))
            a, b = splits[4], splits[-3]
            cases.append((dict(CONFIGS[key], row=12), end, [[a[0], b[0]], [0, b[1]], [a[1], b[2]], [0, b[3]], [0, b[4]], [0, b[5]]], [x, y]))
        cases.append((dict(CONFIGS[key], row=12, scale="whisper"), 1, [[n, key[0] // 2, 0]], [x, y[:key[0] // 2], y[:0]]))
    path = os.path.join(str(tmp_path), "cases.bin")
    write_cases(path, cases)
    r = subprocess.run([sim_main(), path], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-3000:]
    assert r.stdout.startswith("cases %d bytes " % len(cases))


def test_k_logmel_uses_no_scratch_and_the_tiles_lds():
    """LDS is dynamic, sized by the tile of the design: the span of F = 32 frames, (F - 1) hop + n_fft words, skewed by one word
    in 2^ctz(hop) when ctz(hop) >= 2, and p[F][bins | 1]"""
    from jsmpeg_amd import build, logmel
    usage = build.check_kernel_resources()
    mine = {k: v for k, v in usage.items() if "k_logmel" in k}
    assert len(mine) == 2 and all(v["ScratchSize"] == 0 and v["LDS Size"] == 0 for v in mine.values())
    assert F == 32
    for key, (sh, extra) in {(400, 160, 80): (5, (31 * 160 + 400) >> 5), (512, 128, 128): (7, (31 * 128 + 512) >> 7), (32, 8, 8): (3, (31 * 8 + 32) >> 3),
                             (1024, 256, 64): (8, (31 * 256 + 1024) >> 8)}.items():
        n_fft, hop = key[0], key[1]
        want = (F - 1) * hop + n_fft + extra + F * ((n_fft // 2 + 1) | 1)
        r = sim_rule(**CONFIGS[key])
        assert r["lds_floats"] == want and r["sh"] == sh and r["fstride"] % 2 == 1 and r["F"] == F
        assert logmel.plan(**CONFIGS[key])["lds_bytes"] == 4 * want <= 160 * 1024 and logmel.plan(**CONFIGS[key])["frames_per_workgroup"] == F
    assert sim_rule(**dict(WHISPER, hop=162))["sh"] == 31 and sim_rule(**dict(WHISPER, hop=161))["sh"] == 31
    # the largest tile any accepted config asks for still fits
    assert max(4 * sim_rule(**dict(WHISPER, n_fft=1024, hop=hop))["lds_floats"] for hop in range(400, 513)) <= 160 * 1024
