"""k_logmel on the GPU at every path of its dispatch (tests/logmel_inputs.py: the lattice and the proof of what it covers),
against the simulator bit for bit: every tail length of lm_tiles' pipeline, every tile count per wave in the first and second
round, every hop class, full and padded last tiles, under the periodic Hann window and under a rising one that gives the tail's
k terms full weight; chains down to single samples and with a carry at its cap, hundreds of sparse stream numbers, rows of 1, 32
and 33 columns, the whisper maximum at a block's edge, non-finite, subnormal and huge values.  No tolerance anywhere but in the
one test that compares the device with torch.stft in float64 directly, and that one is logmel_ref.mel_bound, derived.  What
anchors the simulator itself: test_logmel_edges.py."""
import numpy as np
import pytest

import logmel_ref as ref
from logmel_inputs import CHAIN_SHAPES, IDS, LATTICE, LIVE_BANDS, NUMBERS, SINGLE_SAMPLE_ON_DEVICE, WINDOWS, chain_row, edge_splits, lattice_output, lattice_row, \
    rising, stream_lengths, window_of
from logmel_util import CONFIGS, WHISPER, F, frames_axis, sim_features, sim_filters, sim_scale
from test_gpu_logmel import bits, noise, on_device, same_bits, torch  # noqa: F401  (torch: the fixture)

pytestmark = pytest.mark.gpu


def same_bits_or_nan(got, want):
    """NaN where the simulator has NaN (the matrix unit's NaN need not carry x86's sign and payload), bit for bit elsewhere"""
    nan = np.isnan(want)
    return got.shape == want.shape and np.array_equal(np.isnan(got), nan) and np.array_equal(bits(got)[~nan], bits(want)[~nan])


@pytest.fixture(scope="module")
def lattice_streams():
    return {k: [noise(n, 700 + 10 * k + i) for i, n in enumerate(stream_lengths(c["n_fft"], c["hop"]))] for k, c in LATTICE.items()}


# ------------------------------------------------------------------ every shape of the lattice
@pytest.mark.parametrize("window", WINDOWS)
@pytest.mark.parametrize("end", [True, False], ids=["end", "open"])
@pytest.mark.parametrize("number", NUMBERS, ids=IDS)
def test_every_path_of_the_dispatch_equals_the_simulator_bit_for_bit(number, end, window, torch, hip_lib, lattice_streams):
    from jsmpeg_amd import logmel
    cfg = LATTICE[number]
    n_fft, hop = cfg["n_fft"], cfg["hop"]
    xs = lattice_streams[number]
    keep, ptrs, counts = on_device(torch, xs)
    dtype, layout, scale = lattice_output(number, end, window)
    run = dict(cfg, scale=scale, layout=layout, dtype=dtype, row=lattice_row(n_fft), window=window_of(window, n_fft))
    want, frames = sim_features(xs, end=end, **run)
    if end:
        assert frames[:3] == [0, 0, (n_fft // 2 + 1) // hop + 1] and frames[-2:] == ([F + 1, 2 * F + 1] if n_fft <= 256 else [F, F + 1])
    with logmel.LogMel(max_streams=len(xs), max_samples=max(counts), **run) as lm:
        lm.features(ptrs, counts, end=end)
        assert lm.counts() == frames
        assert [lm.stream_out(i) for i in range(len(xs))] == [(i * cfg["n_mels"] * run["row"], frames[i]) for i in range(len(xs))]
        got = lm.read()
        assert same_bits(got, want), (dtype, layout, scale)
        assert dtype != "float32" or np.isfinite(got).all()


@pytest.mark.parametrize("number", [3, 6, 10], ids=[IDS[2], IDS[5], IDS[9]])
def test_device_against_torch_stft_in_float64(number, torch, hip_lib):
    """the device's POWER output against float64 directly, within the derived bound: this file does not rest on the header it
    shares with the simulator alone.  The rising window; live bands only."""
    from jsmpeg_amd import logmel
    cfg = LATTICE[number]
    n_fft, hop, n_mels = cfg["n_fft"], cfg["hop"], cfg["n_mels"]
    w = rising(n_fft)
    fb64 = ref.filters(cfg["sample_rate"], n_fft, n_mels, 0.0, 0.0, cfg["mel_scale"], cfg["mel_norm"])
    _, rg = sim_filters(**cfg)
    live = rg[:, 1] > rg[:, 0]
    assert int(live.sum()) == LIVE_BANDS.get(number, n_mels)
    x = noise(5 * hop + n_fft, 4)
    mel, re, im = ref.mel_float64(x, n_fft, hop, fb64, w.astype(np.float64))
    bound = ref.mel_bound(x, n_fft, hop, fb64, rg, re, im, w.astype(np.float64))
    keep, ptrs, counts = on_device(torch, [x])
    with logmel.LogMel(max_streams=1, max_samples=len(x), scale="power", window=w, **cfg) as lm:
        lm.features(ptrs, counts)
        assert lm.counts() == [len(mel)]
        got = lm.read()[0, :, :len(mel)].T
    assert not got[:, ~live].any() and not mel[:, ~live].any()
    mel, bound = mel[:, live], bound[:, live]
    assert mel.min() > 1e-10 and (bound < mel).all()
    assert (np.abs(got[:, live].astype(np.float64) - mel) <= bound).all()


# ------------------------------------------------------------------ chains
def run_calls(lm, ptrs, numbers, calls, end):
    """calls: per call {place in numbers: piece length}; a place that is missing is absent from that call.  END rides on the last
    call.  -> the frames of every place, call after call"""
    done = [0] * len(numbers)
    out = [[] for _ in numbers]
    for k, call in enumerate(calls):
        places = sorted(call)
        lm.features([ptrs[s] + 4 * done[s] for s in places], [call[s] for s in places], streams=[numbers[s] for s in places], chain=True,
                    end=end and k + 1 == len(calls))
        got = frames_axis(lm.read(), lm.layout)
        for i, c in enumerate(lm.counts()):
            out[places[i]].append(got[i, :c])
            done[places[i]] += call[places[i]]
    return [np.concatenate(o) for o in out]


@pytest.mark.parametrize("end", [False, True], ids=["open", "end"])
@pytest.mark.parametrize("number", CHAIN_SHAPES, ids=[IDS[k - 1] for k in CHAIN_SHAPES])
def test_chains_on_the_device(number, end, torch, hip_lib):
    """chain_splits' list, the split whose carry holds exactly n_fft - 1 samples and (shapes 1 and 3) the split into single
    samples, three streams (numbers 0, 1 and max_streams - 1) in the same calls; then one of them absent from a middle call and
    END on a call without samples.  The pieces concatenated equal the simulator's single call."""
    from jsmpeg_amd import logmel
    shape = LATTICE[number]
    n_fft, hop = shape["n_fft"], shape["hop"]
    n, splits = edge_splits(n_fft, hop, singles=number in SINGLE_SAMPLE_ON_DEVICE)
    top = 4
    numbers = [0, 1, top]
    xs = [noise(n, 800 + 10 * number + i) for i in range(3)]
    keep, ptrs, _ = on_device(torch, xs)
    cfg = dict(shape, scale="log10", row=chain_row(n_fft, hop), window=rising(n_fft), layout="time_major" if number <= 2 else "mel_major")
    whole, counts = sim_features(xs, end=end, **cfg)
    whole = frames_axis(whole, cfg["layout"])
    with logmel.LogMel(max_streams=top + 1, max_samples=n, **cfg) as lm:
        for split in splits:
            got = run_calls(lm, ptrs, numbers, [{0: p, 1: p, 2: p} for p in split], end)
            for s in range(3):
                assert same_bits(got[s], whole[s, :counts[s]]), (split if len(split) < 10 else "singles", s)
            assert lm.chain_info(top) == ((False, 0, 0) if end else (True, n, counts[2]))
            lm.chain_reset()
            assert lm.chain_info(0) == (False, 0, 0)
        # stream 1 is not in the second call at all; the last call brings no samples, only END
        a, b = 3 * hop, hop + 1
        calls = [{0: a, 1: a, 2: a}, {0: b, 2: b}, {0: n - a - b, 1: n - a, 2: n - a - b}, {0: 0, 1: 0, 2: 0}]
        got = run_calls(lm, ptrs, numbers, calls, end)
        for s in range(3):
            assert same_bits(got[s], whole[s, :counts[s]]), s


# ------------------------------------------------------------------ many streams
def test_three_hundred_sparse_stream_numbers_and_the_bytes_behind_the_call(torch, hip_lib):
    """max_streams 1000, 300 streams with ascending sparse numbers ending at 999: one unchained call, then a chained pair over the
    same numbers, whose carries lie up to the top of the carry buffer.  The output buffer has room for 1000 streams; the bytes
    behind the call's 300 stay as they were."""
    from jsmpeg_amd import logmel
    key = (32, 8, 8)
    n_fft, hop, n_mels = key
    rng = np.random.default_rng(900)
    numbers = sorted(int(v) for v in rng.choice(999, 299, replace=False)) + [999]
    lengths = [0, n_fft // 2, n_fft // 2 + 1] + [int(v) for v in rng.integers(0, 40 * hop + 1, 296)] + [40 * hop]
    xs = [noise(n, 1000 + i) for i, n in enumerate(lengths)]
    keep, ptrs, counts = on_device(torch, xs)
    cfg = dict(CONFIGS[key], scale="db", row=(40 * hop + n_fft // 2) // hop + 2)
    elems = n_mels * cfg["row"]
    want, frames = sim_features(xs, numbers=numbers, end=True, **cfg)
    with logmel.LogMel(max_streams=1000, max_samples=40 * hop, **cfg) as lm:
        def capacity():
            lm.sync()
            out = np.zeros(1000 * elems, np.float32)
            assert lm.L.jsmpeg_hip_device_read(out.ctypes.data, lm.device_out()[0], out.nbytes) >= 0
            return out
        lm.features(ptrs[-1:], counts[-1:])                         # (a first pass: the buffer can be asked for)
        before = capacity()
        lm.features(ptrs, counts, streams=numbers)
        assert lm.counts() == frames and lm.device_out()[1] == 300 * elems * 4
        assert [lm.stream_out(s) for s in numbers] == [(i * elems, frames[i]) for i in range(300)]
        assert lm.stream_out(next(s for s in range(1000) if s not in numbers)) == (0, 0)
        assert same_bits(lm.read(), want)
        after = capacity()
        assert same_bits(after[:300 * elems].reshape(want.shape), want) and same_bits(after[300 * elems:], before[300 * elems:])
        # the chained pair: every stream cut somewhere, the last one (number 999) with samples in both calls
        cuts = [int(v) for v in rng.integers(0, np.array(lengths) + 1)]
        cuts[-1] = 171
        want = frames_axis(want, "mel_major")
        lm.features(ptrs, cuts, streams=numbers, chain=True, end=False)
        first, c1 = frames_axis(lm.read(), "mel_major"), lm.counts()
        assert lm.chain_info(999) == (True, 171, ref.frames(171, False, n_fft, hop))
        lm.features([p + 4 * c if p else 0 for p, c in zip(ptrs, cuts)], [n - c for n, c in zip(lengths, cuts)], streams=numbers, chain=True, end=True)
        second, c2 = frames_axis(lm.read(), "mel_major"), lm.counts()
        assert [a + b for a, b in zip(c1, c2)] == frames
        for i in range(300):
            assert same_bits(np.concatenate([first[i, :c1[i]], second[i, :c2[i]]]), want[i, :frames[i]]), (i, numbers[i], lengths[i], cuts[i])
        assert lm.chain_info(999) == (False, 0, 0)


# ------------------------------------------------------------------ rows
def test_rows_of_1_32_and_33_columns_and_a_row_far_behind_the_frames(torch, hip_lib):
    from jsmpeg_amd import logmel
    shape = LATTICE[4]
    n_fft, hop, h = shape["n_fft"], shape["hop"], shape["n_fft"] // 2
    x = noise(h + 40 * hop, 1100)
    keep, ptrs, _ = on_device(torch, [x])
    for row in (1, F, F + 1):
        cfg = dict(shape, scale="log", row=row)
        fits = h + (row - 1) * hop + 1                              # open: exactly `row` frames
        want, frames = sim_features([x[:fits]], end=False, **cfg)
        assert frames == [row]
        with logmel.LogMel(max_streams=1, max_samples=len(x), **cfg) as lm:
            lm.features(ptrs, [fits], end=False)
            assert lm.counts() == [row] and same_bits(lm.read(), want)
            with pytest.raises(RuntimeError, match="yields %d frames, row is %d: nothing was enqueued" % (row + 1, row)):
                lm.features(ptrs, [fits + hop], end=False)
            assert lm.query() and lm.counts() == [row] and same_bits(lm.read(), want)
    cfg = dict(shape, scale="db", row=5 * F)
    want, frames = sim_features([x[:h + 1]], end=True, **cfg)
    pad = sim_scale("db", 1e-10, np.zeros(1, np.float32))[0]
    with logmel.LogMel(max_streams=1, max_samples=len(x), **cfg) as lm:
        lm.features(ptrs, [h + 1])
        got = lm.read()
        assert lm.counts() == frames == [3] and same_bits(got, want)
        assert (bits(got[0, :, 3:]) == bits(np.array([pad]))[0]).all() and (got[0, :, :3] > pad).all()


# ------------------------------------------------------------------ the whisper scale
@pytest.mark.parametrize("number", [5, 7], ids=[IDS[4], IDS[6]])
def test_the_whisper_maximum_belongs_to_one_stream_of_one_call(number, torch, hip_lib):
    """the stream's maximum lies in its last, partial block; a loud stream next to an all-zero one; then a quiet call on the same
    handle, in which the first call's maximum must not live on"""
    from jsmpeg_amd import logmel
    shape = LATTICE[number]
    n_fft, hop = shape["n_fft"], shape["hop"]
    n = (F + 4) * hop
    loud = noise(n, 1200 + number, 0.001)
    loud[n - 2 * hop:] = noise(2 * hop, 1300 + number, 0.9)         # frames F + 2 .. F + 4, of F + 5: behind the first block
    quiet = noise(n, 1400 + number, 0.0005)
    zero = np.zeros(n, np.float32)
    cfg = dict(shape, scale="whisper", row=F + 9, dtype="float32", layout="time_major" if number == 7 else "mel_major")
    keep, ptrs, counts = on_device(torch, [loud, zero, quiet])
    with logmel.LogMel(max_streams=2, max_samples=n, **cfg) as lm:
        want, frames = sim_features([loud, zero], **cfg)
        l10, _ = sim_features([loud], **dict(cfg, scale="log10"))
        l10 = frames_axis(l10, cfg["layout"])[0]
        assert frames == [F + 5] * 2 and l10[F:F + 5].max() > l10[:F].max() + 2.0          # the maximum is in the second block
        lm.features(ptrs[:2], counts[:2])
        got = lm.read()
        assert lm.counts() == frames and same_bits(got, want)
        # the zero stream kept its own maximum, log10 of floor: (-10 + 4) / 4 in its frames and (-18 + 4) / 4 behind them
        assert sorted(set(got[1].reshape(-1).tolist())) == [-3.5, -1.5] and got[0].min() > -1.5
        want, frames = sim_features([quiet, zero], **cfg)
        lm.features([ptrs[2], ptrs[1]], counts[:2])
        assert lm.counts() == frames and same_bits(lm.read(), want)


# ------------------------------------------------------------------ non-finite, tiny and huge samples
@pytest.mark.parametrize("name", ["shape_3", "whisper_config"])
def test_non_finite_tiny_and_huge_samples_equal_the_simulator(name, torch, hip_lib):
    """one NaN and one +inf sample stay in the frames whose window covers them; at amplitude 1e-21 every power is a float32
    subnormal and is kept, in lm_power and in the mel sum, as the x86 simulator keeps it; at 3e18 some powers overflow and DB stays
    finite.  NaN is compared as a mask."""
    from jsmpeg_amd import logmel
    shape = LATTICE[3] if name == "shape_3" else WHISPER
    n_fft, hop = shape["n_fft"], shape["hop"]
    clean = noise(40 * hop + n_fft, 1500, 1.0)
    with_nan, with_inf = clean * np.float32(0.5), clean * np.float32(0.5)
    with_nan[100], with_inf[100] = np.nan, np.inf
    xs = [with_nan, with_inf, clean * np.float32(1e-21), clean * np.float32(3e18)]
    keep, ptrs, counts = on_device(torch, xs)
    for scale in ("power", "db") + (("whisper",) if name == "whisper_config" else ()):
        cfg = dict(shape, scale=scale)
        want, frames = sim_features(xs, **cfg)
        with logmel.LogMel(max_streams=4, max_samples=len(clean), **cfg) as lm:
            lm.features(ptrs, counts)
            got = lm.read()
            assert lm.counts() == frames
        assert same_bits_or_nan(got, want), scale
        hit = [t for t in range(frames[0]) if t * hop - n_fft // 2 <= 100 < t * hop + n_fft // 2]
        if scale == "power":
            assert np.isnan(got[0][:, hit]).all() and not np.isfinite(got[1][:, hit]).any()
            assert np.isfinite(np.delete(got[:2], hit, axis=2)).all()
            tiny = got[2][:, :frames[2]]
            assert (tiny > 0).all() and (tiny < np.finfo(np.float32).tiny).all()
        else:
            assert np.isfinite(got).all()
