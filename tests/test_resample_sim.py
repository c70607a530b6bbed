"""The PCM resampler's rule (jsmpeg_amd/csrc/pcm_resample.h, C ABI part 11) without a GPU: the plan and the taps of the
library, the filter's response measured from that table, and the simulator (tests/sim/sim_resample.cpp: the kernel's own
per-lane bodies and the host's own plan, compiled with g++) against a float64 statement of the same sum -- sample values,
counts, chains in pieces, END, mono, gain, the narrow types -- and under the sanitizers.  Every test here fails without the
feature: the header, the module and the library's jsmpeg_hip_resample_* symbols do not exist."""
import os
import subprocess

import numpy as np
import pytest

import resample_ref as ref
from resample_util import FRAME, SimState, sim_lib, sim_main, sim_plan, sim_resample, sim_taps, write_cases

GPU_PAIRS = [(48000, 16000), (44100, 16000), (32000, 44100), (44100, 48000), (48000, 32000)]
PAIR_IDS = ["%d_%d" % p for p in ref.PAIRS]


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({2: np.uint16, 4: np.uint32}[a.dtype.itemsize])


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


@pytest.fixture(scope="module")
def rs(hip_lib):
    from jsmpeg_amd import resample
    return resample


@pytest.fixture(scope="module")
def lib_taps(rs):
    return {p: rs.taps(*p) for p in ref.PAIRS}


# ------------------------------------------------------------------ plan

def test_plan_of_all_18_pairs(rs):
    assert len(ref.PAIRS) == 18
    for pair in ref.PAIRS:
        L, M, H = ref.plan(*pair)
        assert rs.plan(*pair) == (L, M, H) == sim_plan(*pair), pair
        assert rs.taps(*pair).shape == (L, 2 * H)
    table = {(44100, 16000): (160, 441, 45, 14400), (32000, 22050): (441, 640, 24, 21168), (48000, 8000): (1, 6, 96, 192),
             (32000, 44100): (441, 320, 16, 14112)}
    for pair, (L, M, H, floats) in table.items():
        assert rs.plan(*pair) == (L, M, H) and rs.taps(*pair).size == floats
    assert max(rs.taps(*p).size for p in ref.PAIRS) == 441 * 48


@pytest.mark.parametrize("pair", [(48000, 48000), (32000, 32000), (22050, 44100), (48000, 11025), (0, 16000), (48000, 0), (96000, 48000)])
def test_plan_refuses_other_pairs(rs, pair):
    with pytest.raises(ValueError, match="not a supported pair"):
        rs.plan(*pair)
    assert sim_plan(*pair) is None


# ------------------------------------------------------------------ taps

@pytest.mark.parametrize("pair", ref.PAIRS, ids=PAIR_IDS)
def test_taps_within_one_ulp_of_float64(pair, lib_taps):
    """each tap of jsmpeg_hip_resample_taps against the float64 numpy statement of w (np.sinc, np.i0): two correct double
    evaluations can straddle a rounding tie of the one rounding to float32 and nothing more, so the library's tap is the
    float32 nearest to the float64 value or one of its two neighbours"""
    got = lib_taps[pair]
    want = ref.taps64(*pair)
    near = want.astype(np.float32)
    lo, hi = np.nextafter(near, np.float32(-np.inf)), np.nextafter(near, np.float32(np.inf))
    ok = (got >= lo) & (got <= hi)
    assert ok.all(), (pair, np.argwhere(~ok)[:4], got[~ok][:4], want[~ok][:4])
    assert same_bits(got, sim_taps(*pair))                         # the table the kernel reads is the table the simulator reads


# ------------------------------------------------------------------ response

@pytest.mark.parametrize("pair", ref.PAIRS, ids=PAIR_IDS)
def test_response_measured_from_the_table(pair, lib_taps):
    """the library's table as the prototype at rate in L, 2^20-point FFT: DC gain within 1e-4 of 1; nowhere below 0.8 of the
    lower Nyquist more than 0.4 dB under the maximum; everything that folds onto that band (within 0.8 of the lower Nyquist
    of a multiple of the output rate) at most -90 dB.  In float64 from the formula the worst pairs give 0.375 dB and -91.1 dB."""
    in_rate, out_rate = pair
    L, M, H = ref.plan(*pair)
    h = lib_taps[pair].astype(np.float64)
    g = h[:, ::-1].T.reshape(-1)                                   # g[k + H L] = w(k / L): k = (H - 1 - j) L + p
    n = 1 << 20
    G = np.abs(np.fft.rfft(g, n)) / L
    f = np.arange(len(G)) * (in_rate * L / n)
    assert abs(G[0] - 1.0) <= 1e-4
    top = G.max()
    edge = 0.8 * 0.5 * min(in_rate, out_rate)
    band = f <= edge
    ripple = -20 * np.log10(G[band].min() / top)
    k = np.rint(f / out_rate)
    folds = (k >= 1) & (np.abs(f - k * out_rate) <= edge)
    leak = 20 * np.log10(max(G[folds].max(), 1e-300) / top)
    print("%d -> %d: DC %.7f, ripple %.4f dB, folding %.2f dB" % (in_rate, out_rate, G[0], ripple, leak))
    assert ripple <= 0.4
    assert leak <= -90.0


# ------------------------------------------------------------------ sample values

KINDS = ("noise", "dc", "sine", "impulse_first", "impulse_last")


@pytest.mark.parametrize("pair", ref.PAIRS, ids=PAIR_IDS)
def test_sample_values_against_a_float64_dot_product(pair):
    """the simulator against a float64 dot product of the same float32 taps and inputs: per sample at most 2 H 2^-24 sum |h x|
    apart (the running-error bound of 2 H fused steps, u = 2^-24; the float64 sum's own error is 2^-29 of that and below).
    The impulses' outputs ARE the taps, bit for bit, which pins n, p and j."""
    in_rate, out_rate = pair
    L, M, H = ref.plan(*pair)
    taps = sim_taps(*pair)
    frames = 2
    N = frames * FRAME
    xs = [ref.signal(k, in_rate, out_rate, frames, seed=7) for k in KINDS]
    wave, counts = sim_resample(in_rate, out_rate, xs, end=True)
    assert counts == [ref.outputs(in_rate, out_rate, N + H)] * len(KINDS)
    worst = 0.0
    for i, kind in enumerate(KINDS):
        for ch in range(2):
            want, mag = ref.dot64(taps, ref.channel(xs[i], ch), L, M, H, counts[i])
            diff = np.abs(wave[i, ch, :counts[i]].astype(np.float64) - want)
            bound = 2 * H * 2.0 ** -24 * mag
            assert (diff <= bound).all(), (pair, kind, ch, int(np.argmax(diff - bound)))
            worst = max(worst, float((diff[mag > 0] / mag[mag > 0]).max()) * 2 ** 24) if (mag > 0).any() else worst
    print("%d -> %d: worst %.2f 2^-24 sum|h x| at %d taps" % (in_rate, out_rate, worst, 2 * H))
    m = np.arange(counts[0], dtype=np.int64)
    n, p = (m * M) // L, (m * M) % L
    first = wave[KINDS.index("impulse_first"), 0, :counts[0]]
    j = 2 * H - 1 - n                                              # x[n - 2 H + 1 + j] = x[0]
    want = np.where((j >= 0) & (j < 2 * H), taps[p, np.clip(j, 0, 2 * H - 1)], np.float32(0))
    assert same_bits(first, want.astype(np.float32))
    assert (j >= 0).sum() == ref.outputs(in_rate, out_rate, 2 * H)       # the outputs that reach sample 0: n < 2 H
    last = wave[KINDS.index("impulse_last"), 0, :counts[0]]
    j = (N - 1) - n + 2 * H - 1
    want = np.where((j >= 0) & (j < 2 * H), taps[p, np.clip(j, 0, 2 * H - 1)], np.float32(0))
    assert same_bits(last, want.astype(np.float32)) and last.any()


def test_dc_comes_out_as_dc():
    """behind the filter's rise a constant 1.0 is each phase's tap sum: within the response's 1e-4 of 1 on average"""
    for pair in GPU_PAIRS:
        L, M, H = ref.plan(*pair)
        wave, counts = sim_resample(*pair, [ref.signal("dc", *pair, 3)])
        settled = wave[0, 0, ref.outputs(*pair, 2 * H):counts[0]]
        assert abs(float(settled.astype(np.float64).mean()) - 1.0) < 1e-4 and np.abs(settled - 1.0).max() < 2e-3


# ------------------------------------------------------------------ counts

@pytest.mark.parametrize("pair", ref.PAIRS, ids=PAIR_IDS)
def test_counts_are_closed_form(pair):
    L, M, H = ref.plan(*pair)
    xs = [ref.noise(f, seed=f) for f in range(7)]
    wave, counts = sim_resample(*pair, xs)
    assert counts == [-((-FRAME * f * L) // M) for f in range(7)] == [int(sim_lib().sim_resample_outputs(*pair, FRAME * f)) for f in range(7)]
    wave, counts = sim_resample(*pair, xs, end=True)
    assert counts == [0] + [-((-(FRAME * f + H) * L) // M) for f in range(1, 7)]      # a stream without any input has no tail
    frames, counts = sim_resample(*pair, xs, form="frames")
    assert counts == [FRAME * f * L // M // FRAME for f in range(7)]


# ------------------------------------------------------------------ pieces equal the whole

SPLITS = [(1, 1, 3), (2, 3), (1, 0, 4), (1, 1, 1, 1, 1)]


def run_pieces(pair, form, end, streams, splits, channels=2, gain=1.0, dtype="float32"):
    """every stream fed by its own split (all of equal length) in the same chained calls -> per stream the pieces concatenated"""
    state = SimState(len(streams))
    done = [0] * len(streams)
    got = [[] for _ in streams]
    calls = len(splits[0])
    for c in range(calls):
        parts = [x[d:d + s[c]] for x, d, s in zip(streams, done, splits)]
        out, counts = sim_resample(*pair, parts, channels=channels, form=form, dtype=dtype, gain=gain, chain=True, end=end and c == calls - 1, state=state)
        for i in range(len(streams)):
            got[i].append(out[i] if form == "frames" else out[i][:, :counts[i]])
            done[i] += splits[i][c]
    assert [state.info(i)[0] for i in range(len(streams))] == [not end] * len(streams)
    return [np.concatenate(g, axis=0 if form == "frames" else 1) for g in got]


def run_whole(pair, form, end, streams, channels=2, gain=1.0, dtype="float32"):
    out, counts = sim_resample(*pair, streams, channels=channels, form=form, dtype=dtype, gain=gain, end=end)
    return [out[i] if form == "frames" else out[i][:, :counts[i]] for i in range(len(streams))]


@pytest.mark.parametrize("end", [False, True], ids=["open", "end"])
@pytest.mark.parametrize("form", ["waveform", "frames"])
@pytest.mark.parametrize("pair", GPU_PAIRS, ids=["%d_%d" % p for p in GPU_PAIRS])
def test_pieces_equal_the_whole_bit_for_bit(pair, form, end):
    """five frames as 1+1+3, 2+3, 1+0+4 (absent from the middle call) and five single calls (both carries more than once)
    against one call; then two streams with different splits in the same calls"""
    x, y = ref.noise(5, seed=11), ref.noise(5, seed=12)
    whole = run_whole(pair, form, end, [x, y])
    for split in SPLITS:
        got = run_pieces(pair, form, end, [x], [split])
        assert same_bits(got[0], whole[0]), (pair, form, end, split)
    for sa, sb in (((1, 1, 3), (1, 0, 4)), ((2, 3), (4, 1)), ((1, 1, 1, 1, 1), (0, 2, 0, 3, 0))):
        got = run_pieces(pair, form, end, [x, y], [sa, sb])
        assert same_bits(got[0], whole[0]) and same_bits(got[1], whole[1]), (pair, form, end, sa, sb)
    if form == "frames":
        count = ref.outputs(*pair, 5 * FRAME + (ref.plan(*pair)[2] if end else 0))
        assert len(whole[0]) == (-(-count // FRAME) if end else count // FRAME)


def test_pieces_equal_the_whole_mono_gain_and_narrow_types():
    x = ref.noise(5, seed=13)
    for pair, kw in (((44100, 16000), dict(channels=1, dtype="float16")), ((48000, 32000), dict(channels=1, gain=2.0)),
                     ((32000, 44100), dict(dtype="bfloat16", gain=0.5))):
        for form in ("waveform", "frames"):
            if form == "frames":
                kw = dict(kw, dtype="float32")
            whole = run_whole(pair, form, True, [x], **kw)
            for split in SPLITS:
                assert same_bits(run_pieces(pair, form, True, [x], [split], **kw)[0], whole[0]), (pair, form, split)


def test_an_unchained_call_touches_no_state_and_reset_starts_from_zeros():
    pair = (48000, 32000)
    x = ref.noise(3, seed=14)
    state = SimState(2)
    sim_resample(*pair, [x[:1]], numbers=[1], chain=True, state=state)
    before = (state.rec.copy(), state.carry.copy(), state.part.copy())
    alone, _ = sim_resample(*pair, [x[1:2]], numbers=[1], state=state)                 # no CHAIN: from nothing, stores nothing
    assert same_bits(alone, sim_resample(*pair, [x[1:2]])[0])
    assert all(np.array_equal(a, b) for a, b in zip(before, (state.rec, state.carry, state.part)))
    assert state.info(1) == (True, FRAME, ref.outputs(*pair, FRAME)) and state.info(0) == (False, 0, 0)
    state.reset(1)
    again, counts = sim_resample(*pair, [x[1:]], numbers=[1], chain=True, state=state)
    assert same_bits(again, sim_resample(*pair, [x[1:]])[0]) and state.info(1) == (True, 2 * FRAME, counts[0])


# ------------------------------------------------------------------ END

@pytest.mark.parametrize("pair", GPU_PAIRS, ids=["%d_%d" % p for p in GPU_PAIRS])
def test_end_is_the_stream_followed_by_h_zeros(pair):
    L, M, H = ref.plan(*pair)
    x = ref.noise(2, seed=15)
    longer = np.concatenate([x, np.zeros((1, 2, FRAME), np.float32)])
    count = ref.outputs(*pair, 2 * FRAME + H)
    wave, counts = sim_resample(*pair, [x], end=True)
    ref_wave, ref_counts = sim_resample(*pair, [longer])
    assert counts == [count] and ref_counts[0] > count
    assert same_bits(wave[0][:, :count], ref_wave[0][:, :count])
    assert counts[0] > sim_resample(*pair, [x])[1][0]                                  # the tail is more than nothing
    # FRAMES: END pads the last frame with zeros; neither CHAIN nor END drops the partial frame
    frames, n = sim_resample(*pair, [x], form="frames", end=True)
    assert n == [-(-count // FRAME)]
    flat = np.concatenate([frames[0][:, c, :].reshape(-1)[None] for c in range(2)])
    assert same_bits(flat[:, :count], wave[0][:, :count]) and not flat[:, count:].any()
    dropped, n = sim_resample(*pair, [x], form="frames")
    assert n == [ref.outputs(*pair, 2 * FRAME) // FRAME] and same_bits(dropped[0], frames[0][:n[0]])


# ------------------------------------------------------------------ mono, gain, narrow types

def test_mono_is_the_filter_over_the_mix():
    for pair in GPU_PAIRS:
        x = ref.noise(2, seed=16)
        mix = np.float32(0.5) * (x[:, 0, :] + x[:, 1, :])                              # float32: one rounding
        assert mix.dtype == np.float32
        both = np.ascontiguousarray(np.stack([mix, mix], axis=1))
        mono, counts = sim_resample(*pair, [x], channels=1, end=True)
        stereo, counts2 = sim_resample(*pair, [both], channels=2, end=True)
        assert counts == counts2 and mono.shape[1] == 1
        assert same_bits(mono[0, 0], stereo[0, 0]) and same_bits(mono[0, 0], stereo[0, 1])
        frames, _ = sim_resample(*pair, [x], channels=1, form="frames", end=True)      # a mono handle writes the mix to both channels
        assert same_bits(frames[0][:, 0, :], frames[0][:, 1, :])
        assert same_bits(frames[0][:, 0, :].reshape(-1)[:counts[0]], mono[0, 0, :counts[0]])


def test_gain_two_doubles_every_sample_exactly():
    for pair in GPU_PAIRS:
        x = ref.noise(2, seed=17)
        one, _ = sim_resample(*pair, [x], end=True)
        two, _ = sim_resample(*pair, [x], gain=2.0, end=True)
        zero, _ = sim_resample(*pair, [x], gain=0.0, end=True)                         # 0 means 1.0
        assert same_bits(two, one * np.float32(2.0)) and same_bits(zero, one)


def test_narrow_types_equal_torchs_cpu_cast():
    import torch
    for pair in GPU_PAIRS[:3]:
        x = ref.noise(2, seed=18)
        x[0, 0, :8] = [0.0, -0.0, 1e-9, -3e-8, 6.1e-5, 5.96e-8, 2.98e-8, 1.0]         # zeros, float16 subnormals and below
        f32, counts = sim_resample(*pair, [x], gain=2.0, end=True)
        for dtype, tdt in (("float16", torch.float16), ("bfloat16", torch.bfloat16)):
            got, c = sim_resample(*pair, [x], dtype=dtype, gain=2.0, end=True)
            want = torch.from_numpy(f32).to(tdt).view(torch.int16).numpy().view(np.uint16)
            assert c == counts and np.array_equal(bits(got), want), (pair, dtype)


def test_narrow_roundings_on_crafted_bits():
    """rs_f16_bits / rs_bf16_bits over ties, subnormals, the overflow edge and random patterns against torch's CPU cast"""
    import torch
    L = sim_lib()
    r = np.random.default_rng(19)
    edge = [0x00000000, 0x80000000, 0x33000000, 0x33000001, 0x32ffffff, 0x33800000, 0x33c00000, 0x387fe000, 0x387ff000, 0x38800000, 0x38801000,
            0x38803000, 0x3f800000, 0x3f801000, 0x3f803000, 0x3f802fff, 0x477fe000, 0x477fefff, 0x477ff000, 0x47800000, 0x7f7fffff, 0x7f800000,
            0xff800000, 0x3f808000, 0x3f818000, 0x3f807fff, 0x7f7f8000, 0x00000001, 0x007fffff, 0x00800000]
    u = np.concatenate([np.array(edge, np.uint32), r.integers(0, 1 << 32, 4000, dtype=np.uint64).astype(np.uint32),
                        (r.integers(0x33000000, 0x48000000, 4000, dtype=np.uint64)).astype(np.uint32)])
    f = u.view(np.float32)
    f = f[~np.isnan(f)]
    t = torch.from_numpy(f.copy())
    want16 = t.to(torch.float16).view(torch.int16).numpy().view(np.uint16)
    wantbf = t.to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    got16 = np.array([L.sim_resample_f16(float(v)) for v in f], np.uint16)
    gotbf = np.array([L.sim_resample_bf16(float(v)) for v in f], np.uint16)
    assert np.array_equal(got16, want16) and np.array_equal(gotbf, wantbf)


def test_row_and_frame_limits_are_refused():
    x = ref.noise(2, seed=20)
    count = ref.outputs(48000, 16000, 2 * FRAME)
    wave, counts = sim_resample(48000, 16000, [x], row=count)
    assert counts == [count] and wave.shape[2] == count
    with pytest.raises(RuntimeError, match="-1$"):
        sim_resample(48000, 16000, [x], row=count - 1)
    with pytest.raises(RuntimeError, match="-2$"):
        sim_resample(48000, 16000, [x[:1], x], row=count - 1)


# ------------------------------------------------------------------ sanitizers, resources

def test_stand_alone_program_is_clean_under_the_sanitizers(tmp_path):
    """ASan + UBSan over the simulator's stand-alone program: inputs in buffers of exactly the frames' size, outputs of
    exactly the call's size; nothing is preloaded"""
    cases = []
    x, y = ref.noise(5, seed=21), ref.noise(4, seed=22)
    for pair in GPU_PAIRS + [(48000, 8000), (32000, 22050)]:
        cases.append(((*pair, 2, 0, 0, 8000), 1.0, True, [(1, 0), (1, 2), (3, 2)], [x, y]))
        cases.append(((*pair, 1, 1, 0, 0), 2.0, True, [(1, 1), (1, 1), (1, 1), (1, 1), (1, 0)], [x, y]))
        cases.append(((*pair, 2, 1, 0, 0), 1.0, False, [(2, 4), (3, 0)], [x, y]))
        cases.append(((*pair, 1, 0, 1, ref.outputs(*pair, 5 * FRAME)), 1.0, False, [(5, 4)], [x, y]))
        cases.append(((*pair, 2, 0, 2, ref.outputs(*pair, 5 * FRAME + ref.plan(*pair)[2])), 1.0, True, [(5, 0)], [x, y[:0]]))
    path = os.path.join(tmp_path, "cases.bin")
    write_cases(path, cases)
    r = subprocess.run([sim_main(), path], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-3000:]
    assert r.stdout.startswith("cases %d bytes " % len(cases))


def test_k_resample_uses_no_scratch():
    from jsmpeg_amd import build
    usage = build.check_kernel_resources()
    mine = [v for k, v in usage.items() if "k_resample" in k]
    assert len(mine) == 1 and mine[0]["ScratchSize"] == 0 and mine[0]["LDS Size"] <= 7168
