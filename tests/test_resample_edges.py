"""The PCM resampler's edges without a GPU, on the simulator (tests/sim/sim_resample.cpp: the kernel's per-lane bodies and the
host's plan from jsmpeg_amd/csrc/pcm_resample.h): chains of all 18 pairs in both forms -- 48000 -> 8000, whose calls hand out
no frame five times in a row, among them --, END on a call without input, the largest call the 32-bit arithmetic takes and the
first one it refuses, and inputs so small that the sums and the narrow outputs are subnormal.  tests/test_gpu_resample_edges.py
runs the same inputs (tests/resample_inputs.py) on the device."""
import ctypes

import numpy as np
import pytest

import resample_inputs as inp
import resample_ref as ref
from resample_inputs import FRAME, same_bits
from resample_util import DTYPES, END, FORMS, SimState, sim_lib, sim_resample, sim_taps


@pytest.fixture(scope="module")
def noise8():
    return [ref.noise(inp.CHAIN_FRAMES, seed=31 + i) for i in range(2)]


def run_chain(pair, form, end, streams, splits, leave_out=False, **kw):
    """every stream fed by its own split in the same chained calls, END on the last -> (per stream the pieces concatenated,
    per stream the count of every call, the state behind the last call).  leave_out: a stream without frames is listed with
    a count of 0 in even calls and in the last one, and not listed at all in the other odd calls"""
    state = SimState(len(streams))
    done = [0] * len(streams)
    got, per_call = [[] for _ in streams], [[] for _ in streams]
    calls = len(splits[0])
    for c in range(calls):
        listed = [i for i, s in enumerate(splits) if s[c] or not leave_out or c % 2 == 0 or c == calls - 1]
        parts = [streams[i][done[i]:done[i] + splits[i][c]] for i in listed]
        out, counts = sim_resample(*pair, parts, form=form, numbers=listed, chain=True, end=end and c == calls - 1, state=state, **kw)
        for i in range(len(streams)):
            if i in listed:
                k = listed.index(i)
                got[i].append(out[k] if form == "frames" else out[k][:, :counts[k]])
            per_call[i].append(counts[listed.index(i)] if i in listed else 0)
            done[i] += splits[i][c]
    return [np.concatenate(g, axis=0 if form == "frames" else 1) for g in got], per_call, state


def run_whole(pair, form, end, streams, **kw):
    out, counts = sim_resample(*pair, streams, form=form, end=end, **kw)
    return [out[i] if form == "frames" else out[i][:, :counts[i]] for i in range(len(streams))]


# ------------------------------------------------------------------ pieces equal the whole

@pytest.mark.parametrize("end", [False, True], ids=["open", "end"])
@pytest.mark.parametrize("form", ["waveform", "frames"])
@pytest.mark.parametrize("pair", ref.PAIRS, ids=inp.PAIR_IDS)
def test_pieces_equal_the_whole_for_every_pair(pair, form, end, noise8):
    """eight frames in eight single calls (each carry and each partial frame written four times), as 2+0+6 and as 1+7 against
    one call; then two streams with different splits in the same calls, one of them absent -- listed without frames, or
    left out of the call -- while the device holds samples of its partial frame.  The whole frames a FRAMES call hands out are the closed form."""
    x, y = noise8
    whole = run_whole(pair, form, end, [x, y])
    for split in inp.SPLITS:
        got, per_call, state = run_chain(pair, form, end, [x], [split])
        assert same_bits(got[0], whole[0]), (pair, form, end, split)
        assert state.info(0)[0] == (not end)
        if form == "frames":
            assert per_call[0] == inp.whole_frames_per_call(pair, split, end), (pair, split)
    held = 0
    for sa, sb in inp.PAIRED:
        got, per_call, _ = run_chain(pair, form, end, [x, y], [sa, sb], leave_out=sb is inp.ABSENT)
        assert same_bits(got[0], whole[0]) and same_bits(got[1], whole[1]), (pair, form, end, sa, sb)
        if form == "frames":
            assert per_call == [inp.whole_frames_per_call(pair, s, end) for s in (sa, sb)]
        held += sum(1 for c in range(1, len(sb)) if sb[c] == 0 and sb[c - 1] == 0 and inp.lead_before_call(pair, sb, c))
    assert held >= 2                                              # absent more than once with a partial frame on the device
    if form == "frames" and not end:                             # an open chain drops nothing: the rest is on the device
        count = ref.outputs(*pair, inp.CHAIN_FRAMES * FRAME)
        assert len(whole[0]) == count // FRAME


@pytest.mark.parametrize("pair", [(48000, 8000), (44100, 8000)], ids=["48000_8000", "44100_8000"])
def test_five_calls_in_a_row_hand_out_nothing(pair):
    """FRAMES, single-frame calls at a sixth of the rate: 192 (208.98) outputs per frame, so five calls only move a growing
    lead from part[parity] to part[parity ^ 1]; the sixth completes the frame -- for 48000 -> 8000 exactly, lead + count ==
    1152, so nothing goes to part although the call may write it"""
    x = ref.noise(inp.CHAIN_FRAMES, seed=33)
    assert inp.whole_frames_per_call(pair, inp.SINGLES, False) == [0, 0, 0, 0, 0, 1, 0, 0]
    assert inp.whole_frames_per_call(pair, inp.SINGLES, True) == [0, 0, 0, 0, 0, 1, 0, 1]
    for end in (False, True):
        got, per_call, _ = run_chain(pair, "frames", end, [x], [inp.SINGLES])
        assert per_call[0] == inp.whole_frames_per_call(pair, inp.SINGLES, end)
        assert same_bits(got[0], run_whole(pair, "frames", end, [x])[0])
    assert [inp.lead_before_call(pair, inp.SINGLES, c) for c in range(1, 6)] == [ref.outputs(*pair, c * FRAME) for c in range(1, 6)]
    if pair == (48000, 8000):
        assert inp.lead_before_call(pair, inp.SINGLES, 5) + 192 == FRAME and inp.lead_before_call(pair, inp.SINGLES, 6) == 0
    # the frame the sixth call hands out is the waveform's first 1152 samples: the leads were carried, not recomputed
    wave = run_whole(pair, "waveform", False, [x])[0]
    state = SimState(1)
    for c in range(6):
        out, counts = sim_resample(*pair, [x[c:c + 1]], form="frames", chain=True, state=state)
        assert counts == [int(c == 5)]
    assert same_bits(out[0][0], wave[:, :FRAME])


# ------------------------------------------------------------------ END on a call without input

@pytest.mark.parametrize("form", ["waveform", "frames"])
@pytest.mark.parametrize("pair", inp.LIMIT_PAIRS, ids=["%d_%d" % p for p in inp.LIMIT_PAIRS])
def test_end_on_a_call_without_input_yields_the_tail(pair, form):
    """a chained stream with state gets frames = 0 with END: exactly the outputs that H zero samples add, read from the carry
    alone; in FRAMES form the last frame filled with zeros.  A stream without state gets nothing."""
    L, M, H = ref.plan(*pair)
    x = ref.noise(3, seed=34)
    whole = run_whole(pair, form, True, [x])[0]
    state = SimState(2)
    a, ca = sim_resample(*pair, [x[:2]], form=form, numbers=[1], chain=True, state=state)
    b, cb = sim_resample(*pair, [x[2:]], form=form, numbers=[1], chain=True, state=state)
    assert state.info(1) == (True, 3 * FRAME, ref.outputs(*pair, 3 * FRAME))
    t, ct = sim_resample(*pair, [x[:0], x[:0]], form=form, numbers=[0, 1], chain=True, end=True, state=state)
    assert state.info(1) == (False, 0, 0) and ct[0] == 0
    before, after = ref.outputs(*pair, 3 * FRAME), ref.outputs(*pair, 3 * FRAME + H)
    if form == "waveform":
        assert ct[1] == after - before > 0
        got = np.concatenate([a[0][:, :ca[0]], b[0][:, :cb[0]], t[1][:, :ct[1]]], axis=1)
    else:
        assert ct[1] == -(-after // FRAME) - before // FRAME == 1
        got = np.concatenate([a[0], b[0], t[1]], axis=0)
        flat = t[1][0].reshape(2, FRAME)
        assert not flat[:, after % FRAME:].any() and flat[:, before % FRAME:after % FRAME].any()
    assert same_bits(got, whole)


# ------------------------------------------------------------------ the 32-bit arithmetic of a call

def plan_only(pair, frames, end, row):
    """sim_resample_call's return code for streams of `frames` frames behind ONE real frame of memory: a refused plan reads
    no sample"""
    L = sim_lib()
    n = len(frames)
    cfg = np.array([*pair, 2, FORMS["waveform"], DTYPES["float32"], row], np.int32)
    mem = np.zeros((1, 2, FRAME), np.float32)
    ptrs = (ctypes.c_void_p * n)(*[mem.ctypes.data if f else None for f in frames])
    fr = np.array(frames, np.uint32)
    out = np.zeros(64, np.uint8)
    offset, count = np.zeros(n, np.uint64), np.zeros(n, np.uint64)
    return L.sim_resample_call(cfg.ctypes.data, 1.0, ptrs, fr.ctypes.data, None, n, END if end else 0, None, None, None, out.ctypes.data, 0,
                               offset.ctypes.data, count.ctypes.data)



@pytest.mark.parametrize("pair", [p for p in ref.PAIRS if ref.plan(*p)[0] > 3], ids=["%d_%d" % p for p in ref.PAIRS if ref.plan(*p)[0] > 3])
def test_the_first_refused_frame_count(pair):
    """the host refuses a call whose (inputs + tail) L + M is above 2^32 - 1.  With row = 1 the largest accepted count is
    refused for its row (-1 - i: the 32-bit check comes first and passed), one frame more for the arithmetic (-1000001 - i)"""
    L, M, H = ref.plan(*pair)
    pinned = {441: 8454, 320: 11650, 160: 23301, 147: 25362, 80: 46603}
    for end in (True, False):
        most = inp.most_frames(pair, end)
        tail = H if end else 0
        assert (most * FRAME + tail) * L + M <= 0xffffffff < ((most + 1) * FRAME + tail) * L + M
        assert plan_only(pair, [0, most], end, 1) == -1 - 1
        assert plan_only(pair, [0, most + 1], end, 1) == -1000001 - 1
        assert plan_only(pair, [most + 1, 1], end, 1) == -1000001 - 0
        assert plan_only(pair, [1, 0, most + 1], end, 1 << 20) == -1000001 - 2
    assert inp.most_frames(pair) == pinned[L]
    assert inp.most_frames(inp.EDGE_PAIR) == inp.EDGE_FRAMES == 8454


def test_the_largest_call_equals_the_closed_form():
    """32000 -> 44100, 8454 frames, stereo, END: the last output's k M is 4 294 909 440, 57 856 below 2^32.  Every output
    of both channels is the impulses' closed form: one bit too few anywhere in o + k M moves the late impulses' outputs"""
    pair, frames = inp.EDGE_PAIR, inp.EDGE_FRAMES
    L, M, H = ref.plan(*pair)
    count = ref.outputs(*pair, frames * FRAME + H)
    assert count == 13421593 and (count - 1) * M == 4294909440 == (1 << 32) - 57856
    x, positions = inp.impulse_streams(pair, frames)
    wave, counts = sim_resample(*pair, [x], end=True, row=count)
    assert counts == [count]
    taps = sim_taps(*pair)
    for ch in range(2):
        want = inp.impulse_want(pair, taps, positions[ch], count)
        assert np.flatnonzero(want)[-1] > count - 2 * H * 2 and np.count_nonzero(want) > 100
        assert same_bits(wave[0, ch], want), ch


# ------------------------------------------------------------------ impulses at the layout's and the workgroups' edges

@pytest.mark.parametrize("pair", ref.PAIRS, ids=inp.PAIR_IDS)
def test_impulses_at_the_edges_are_the_taps(pair):
    """three frames of the impulse layout, stereo and mono with gain 2.0: the closed form pins n, p and j at sample 0, at the
    frame edge, at the stream's end and on both sides of a workgroup's edge"""
    L, M, H = ref.plan(*pair)
    x, positions = inp.impulse_streams(pair, 3)
    assert positions[0] and positions[1] and len(positions[0]) + len(positions[1]) >= 7
    assert FRAME - 1 in positions[0] and FRAME in positions[1]
    edges = inp.edge_positions(pair, 3)
    assert edges and any(q in positions[0] + positions[1] for q in edges)
    count = ref.outputs(*pair, 3 * FRAME + H)
    taps = sim_taps(*pair)
    wave, counts = sim_resample(*pair, [x], end=True)
    mono, mono_counts = sim_resample(*pair, [inp.one_channel(x, 0), inp.one_channel(x, 1)], channels=1, gain=2.0, end=True)
    assert counts == [count] and mono_counts == [count, count]
    for ch in range(2):
        want = inp.impulse_want(pair, taps, positions[ch], count)
        assert same_bits(wave[0, ch, :count], want), (pair, ch)
        assert same_bits(mono[ch, 0, :count], inp.impulse_want(pair, taps, positions[ch], count, height=0.5, gain=2.0)), (pair, ch)
        assert same_bits(mono[ch, 0, :count], want)               # 2.0 * (0.5 * tap) is the tap


# ------------------------------------------------------------------ tiny inputs

@pytest.mark.parametrize("e,dtype", inp.TINY, ids=inp.TINY_IDS)
def test_tiny_inputs_give_subnormal_outputs(e, dtype):
    """noise scaled by 2^e: float32 sums and narrow outputs below the smallest normal number exist and are kept -- nothing is
    flushed to zero -- and the narrow bits are torch's CPU cast of the float32 result"""
    import torch
    pair = inp.TINY_PAIR
    x = inp.tiny(1, e, seed=35)
    f32, counts = sim_resample(*pair, [x], end=True)
    got, c = sim_resample(*pair, [x], dtype=dtype, end=True)
    assert c == counts == [ref.outputs(*pair, FRAME + ref.plan(*pair)[2])]
    small, nonzero = inp.subnormals(got, dtype)
    print("2^%d %s: %d of %d nonzero samples are subnormal" % (e, dtype, small, nonzero))
    assert small > 0
    if e == -140:
        assert small == nonzero                                   # every input is subnormal, every tap below 1
    if dtype == "float32":
        # against float64 over the same taps and inputs: a fused step's rounding is 2^-24 of its result or, where that is
        # subnormal, half a unit of 2^-149 -- so a flushed sum (off by all of itself, about 2^e) is far outside
        L, M, H = ref.plan(*pair)
        for ch in range(2):
            want, mag = ref.dot64(sim_taps(*pair), ref.channel(x, ch), L, M, H, c[0])
            diff = np.abs(f32[0, ch, :c[0]].astype(np.float64) - want)
            assert (diff <= 2 * H * (2.0 ** -24 * mag + 2.0 ** -150)).all()
        assert same_bits(got, f32)
    else:
        tdt = {"float16": torch.float16, "bfloat16": torch.bfloat16}[dtype]
        want = torch.from_numpy(f32).to(tdt).view(torch.int16).numpy().view(np.uint16)
        assert np.array_equal(inp.bits(got), want)
