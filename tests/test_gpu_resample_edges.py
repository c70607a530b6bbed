"""The PCM resampler's edges on the device (C ABI part 11, jsmpeg_amd/resample.py), with the inputs of
tests/resample_inputs.py: all 18 rate pairs against the simulator AND against references that share no code with it (the
impulses' closed form, a float64 dot product), chains in eight calls in both forms, the largest call the 32-bit arithmetic
takes, subnormal sums and outputs, 70 streams in one FRAMES call.  Bits are asserted, never times.  Every call here is a valid
call or a refusal that launches nothing.  Needs an MI355X."""
import time

import numpy as np
import pytest

import resample_inputs as inp
import resample_ref as ref
from resample_inputs import FRAME, same_bits
from resample_util import SimState, sim_resample

pytestmark = pytest.mark.gpu

#          channels, form, dtype, gain, end
VARIANTS = [(2, "waveform", "float32", 1.0, True), (1, "waveform", "float16", 1.0, False), (2, "waveform", "bfloat16", 2.0, True),
            (2, "frames", "float32", 1.0, True), (1, "frames", "float32", 2.0, True)]


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


@pytest.fixture(scope="module")
def rsm(hip_lib):
    from jsmpeg_amd import resample
    return resample


@pytest.fixture(scope="module")
def inputs():
    """noise: three streams of eight frames"""
    return [ref.noise(inp.CHAIN_FRAMES, seed=200 + i) for i in range(3)]


def on_device(torch, streams):
    """float32 [frames][2][1152] per stream -> (tensors to keep alive, device pointers, frame counts)"""
    keep = [torch.from_numpy(np.ascontiguousarray(s, dtype=np.float32)).cuda() for s in streams]
    torch.cuda.synchronize()
    return keep, [t.data_ptr() if len(s) else 0 for t, s in zip(keep, streams)], [len(s) for s in streams]


def gpu_streams(rs):
    """the last call's result per stream of the call, cut to its count: waveform [channels][count], frames [count][2][1152];
    FRAMES offsets are the running sum of the counts"""
    out, counts = rs.read(), rs.counts()
    if rs.form == "frames":
        at, res = 0, []
        for i, s in enumerate(rs._numbers):
            assert rs.stream_out(s) == (at, counts[i])
            res.append(out[at:at + counts[i]])
            at += counts[i]
        assert at == len(out)
        return res
    for i in range(len(counts)):
        assert not out[i, :, counts[i]:].any()                    # a padded batch: zeros behind the count
    return [out[i][:, :counts[i]] for i in range(len(counts))]


def sim_streams(pair, streams, form, **kw):
    out, counts = sim_resample(*pair, streams, form=form, **kw)
    return [out[i] if form == "frames" else out[i][:, :counts[i]] for i in range(len(streams))], counts


# ------------------------------------------------------------------ every pair against the simulator

@pytest.mark.parametrize("pair", ref.PAIRS, ids=inp.PAIR_IDS)
def test_every_pair_equals_the_simulator_bit_for_bit(pair, torch, rsm, inputs):
    """three streams of 0, 1 and 3 frames in one call: stereo float32 with END, mono float16 without, stereo bfloat16 with a
    gain of 2.0, FRAMES stereo with END, FRAMES mono with a gain of 2.0 and END (without it the
    slowest pairs complete no frame from three)"""
    xs = [inputs[0][:0], inputs[1][:1], inputs[2][:3]]
    keep, ptrs, frames = on_device(torch, xs)
    for channels, form, dtype, gain, end in VARIANTS:
        want, counts = sim_streams(pair, xs, form, channels=channels, dtype=dtype, gain=gain, end=end)
        with rsm.Resampler(*pair, channels=channels, form=form, dtype=dtype, gain=gain, max_streams=3, max_frames=4) as rs:
            rs.resample(ptrs, frames, end=end)
            assert rs.counts() == counts and counts[0] == 0 and counts[2] > 0
            got = gpu_streams(rs)
            for i in range(3):
                assert same_bits(got[i], want[i]), (pair, channels, form, dtype, gain, end, i)


# ------------------------------------------------------------------ every pair against what is not the simulator

@pytest.mark.parametrize("pair", ref.PAIRS, ids=inp.PAIR_IDS)
def test_impulses_on_the_device_are_the_taps(pair, torch, rsm):
    """the impulse layout -- sample 0, the frame edge, the stream's end, both sides of a workgroup's edge -- stereo and mono
    with a gain of 2.0: the device's waveform is the closed form over the library's own table, which pins n, p and j without
    the simulator"""
    L, M, H = ref.plan(*pair)
    x, positions = inp.impulse_streams(pair, 3)
    count = ref.outputs(*pair, 3 * FRAME + H)
    taps = rsm.taps(*pair)
    want = [inp.impulse_want(pair, taps, positions[ch], count) for ch in range(2)]
    assert want[0].any() and want[1].any()
    keep, ptrs, frames = on_device(torch, [x, inp.one_channel(x, 0), inp.one_channel(x, 1)])
    with rsm.Resampler(*pair, max_streams=1, max_frames=3) as rs:
        rs.resample(ptrs[:1], frames[:1], end=True)
        assert rs.counts() == [count] == [rs.row]
        got = rs.read()
        for ch in range(2):
            assert same_bits(got[0, ch], want[ch]), (pair, ch)
    with rsm.Resampler(*pair, channels=1, gain=2.0, max_streams=2, max_frames=6) as rs:
        rs.resample(ptrs[1:], frames[1:], end=True)
        assert rs.counts() == [count, count]
        got = rs.read()
        for ch in range(2):
            assert same_bits(got[ch, 0, :count], inp.impulse_want(pair, taps, positions[ch], count, height=0.5, gain=2.0)), (pair, ch)
            assert same_bits(got[ch, 0, :count], want[ch]) and not got[ch, 0, count:].any()


@pytest.mark.parametrize("pair", ref.PAIRS, ids=inp.PAIR_IDS)
def test_noise_on_the_device_against_a_float64_dot_product(pair, torch, rsm, inputs):
    """two frames of noise: every device sample within 2 H 2^-24 sum |h x| of the float64 dot product of the same float32 taps
    and inputs -- the running-error bound of 2 H fused steps that tests/test_resample_sim.py derives"""
    L, M, H = ref.plan(*pair)
    x = inputs[0][:2]
    taps = rsm.taps(*pair)
    keep, ptrs, frames = on_device(torch, [x])
    with rsm.Resampler(*pair, max_streams=1, max_frames=2) as rs:
        rs.resample(ptrs, frames, end=True)
        count = rs.counts()[0]
        assert count == ref.outputs(*pair, 2 * FRAME + H)
        got = rs.read()
    worst = 0.0
    for ch in range(2):
        want, mag = ref.dot64(taps, ref.channel(x, ch), L, M, H, count)
        diff = np.abs(got[0, ch, :count].astype(np.float64) - want)
        bound = 2 * H * 2.0 ** -24 * mag
        worst = max(worst, float((diff[mag > 0] / bound[mag > 0]).max()))
        print("%d -> %d channel %d: worst share of the bound %.4f" % (*pair, ch, float((diff[mag > 0] / bound[mag > 0]).max())))
        assert (diff <= bound).all(), (pair, ch, int(np.argmax(diff - bound)))
    print("RATIO %d %d %.4f" % (*pair, worst))


# ------------------------------------------------------------------ chains

def sim_chain(pair, form, streams, numbers, splits, top):
    """the simulator through the same chained calls, every stream listed in every call -> per stream the count of each call"""
    state = SimState(top + 1)
    done = [0] * len(streams)
    per_call = [[] for _ in streams]
    for c in range(len(splits[0])):
        parts = [x[d:d + s[c]] for x, d, s in zip(streams, done, splits)]
        _, counts = sim_resample(*pair, parts, form=form, numbers=numbers, chain=True, end=c == len(splits[0]) - 1, state=state)
        for i in range(len(streams)):
            per_call[i].append(counts[i])
            done[i] += splits[i][c]
    return per_call


@pytest.mark.parametrize("form", ["waveform", "frames"])
@pytest.mark.parametrize("pair", ref.PAIRS, ids=inp.PAIR_IDS)
def test_eight_calls_on_the_device_equal_one(pair, form, torch, rsm, inputs):
    """streams 0 and max_streams - 1 in eight single-frame calls, stream 2 as 2+0+0+0+0+0+6+0 -- listed without frames in
    calls 1 to 3, left out of calls 4 and 5, while its partial frame waits on the device --, END on the last call: the pieces
    concatenated are the simulator's one call bit for bit; the whole frames of every FRAMES call are the simulator's and the
    closed form"""
    top = 5
    numbers, splits = [0, 2, top], [inp.SINGLES, inp.ABSENT, inp.SINGLES]
    xs = [inputs[0], inputs[1], inputs[2]]
    whole, _ = sim_streams(pair, xs, form, end=True)
    sim_counts = sim_chain(pair, form, xs, numbers, splits, top)
    axis = 0 if form == "frames" else 1
    got, per_call, done = [[], [], []], [[], [], []], [0, 0, 0]
    with rsm.Resampler(*pair, form=form, max_streams=top + 1, max_frames=8) as rs:
        for c in range(8):
            listed = [i for i in range(3) if not (i == 1 and c in (4, 5))]
            parts = [xs[i][done[i]:done[i] + splits[i][c]] for i in listed]
            keep, ptrs, frames = on_device(torch, parts)
            rs.resample(ptrs, frames, [numbers[i] for i in listed], chain=True, end=c == 7)
            counts, res = rs.counts(), gpu_streams(rs)
            for k, i in enumerate(listed):
                got[i].append(res[k])
                per_call[i].append(counts[k])
                done[i] += splits[i][c]
            if 1 not in listed:
                per_call[1].append(0)
            if c == 5:
                assert rs.chain_info(2) == (True, 2 * FRAME, ref.outputs(*pair, 2 * FRAME))
        assert [rs.chain_info(s) for s in numbers] == [(False, 0, 0)] * 3
    for i in range(3):
        assert same_bits(np.concatenate(got[i], axis=axis), whole[i]), (pair, form, i)
    assert per_call == sim_counts
    if form == "frames":
        assert per_call == [inp.whole_frames_per_call(pair, s, True) for s in splits]
        if pair in ((48000, 8000), (44100, 8000)):
            assert per_call[0] == [0, 0, 0, 0, 0, 1, 0, 1]


@pytest.mark.parametrize("form", ["waveform", "frames"])
@pytest.mark.parametrize("pair", inp.LIMIT_PAIRS, ids=["%d_%d" % p for p in inp.LIMIT_PAIRS])
def test_end_without_input_on_the_device(pair, form, torch, rsm, inputs):
    """a chained stream with state gets frames = 0 with END: the tail comes out of the carry alone, and in FRAMES form the
    last frame is filled with zeros; a listed stream without state gets nothing"""
    L, M, H = ref.plan(*pair)
    x = inputs[1][:3]
    whole, _ = sim_streams(pair, [x], form, end=True)
    axis = 0 if form == "frames" else 1
    with rsm.Resampler(*pair, form=form, max_streams=2, max_frames=2) as rs:
        pieces = []
        for part in (x[:2], x[2:]):
            keep, ptrs, frames = on_device(torch, [part])
            rs.resample(ptrs, frames, [1], chain=True)
            pieces.append(gpu_streams(rs)[0])
        assert rs.chain_info(1) == (True, 3 * FRAME, ref.outputs(*pair, 3 * FRAME))
        rs.resample([0, 0], [0, 0], [0, 1], chain=True, end=True)
        before, after = ref.outputs(*pair, 3 * FRAME), ref.outputs(*pair, 3 * FRAME + H)
        assert rs.counts() == ([0, after - before] if form == "waveform" else [0, 1])
        tail = gpu_streams(rs)
        assert tail[0].size == 0 and rs.chain_info(1) == (False, 0, 0)
        if form == "frames":
            assert not tail[1][0][:, after % FRAME:].any()
        assert same_bits(np.concatenate(pieces + [tail[1]], axis=axis), whole[0])


# ------------------------------------------------------------------ the largest call

def test_the_largest_call_the_32_bit_arithmetic_takes(torch, rsm):
    """32000 -> 44100, 8454 frames of the impulse layout in one stream, stereo float32, END: 13 421 593 outputs per channel,
    the last one's k M 57 856 below 2^32; the whole read-back is the closed form.  8455 frames are above the handle's
    max_frames; a handle that allows them refuses the call for its arithmetic, moves no state and works right after."""
    pair, frames = inp.EDGE_PAIR, inp.EDGE_FRAMES
    L, M, H = ref.plan(*pair)
    count = 13421593
    assert inp.most_frames(pair) == frames and ref.outputs(*pair, frames * FRAME + H) == count
    x, positions = inp.impulse_streams(pair, frames)
    taps = rsm.taps(*pair)
    keep, ptrs, _ = on_device(torch, [x])
    with rsm.Resampler(*pair, max_streams=1, max_frames=frames) as rs:
        t0 = time.perf_counter()
        rs.resample(ptrs, [frames], end=True)
        assert rs.counts() == [count] == [rs.row]
        got = rs.read()
        print("LARGEST call and read-back %.3f s, kernel %.3f ms" % (time.perf_counter() - t0, rs.timings()["kernel_ms"]))
        for ch in range(2):
            want = inp.impulse_want(pair, taps, positions[ch], count)
            assert np.flatnonzero(want)[-1] > count - 4 * H
            assert same_bits(got[0, ch], want), ch
        with pytest.raises(RuntimeError, match="max_frames"):
            rs.resample(ptrs, [frames + 1], end=True)
    small = x[:1]
    small_want, small_counts = sim_streams(pair, [small], "waveform", end=True)
    with rsm.Resampler(*pair, max_streams=1, max_frames=frames + 1, row=small_counts[0]) as rs:
        for chain in (True, False):
            with pytest.raises(RuntimeError, match="32-bit arithmetic"):
                rs.resample(ptrs, [frames + 1], chain=chain, end=True)
        assert rs.chain_info(0) == (False, 0, 0)
        with pytest.raises(RuntimeError, match="nothing was resampled"):
            rs.device_out()
        rs.resample(ptrs, [1], chain=True, end=True)
        assert rs.counts() == small_counts and same_bits(gpu_streams(rs)[0], small_want[0])


# ------------------------------------------------------------------ tiny inputs

@pytest.mark.parametrize("e,dtype", inp.TINY, ids=inp.TINY_IDS)
def test_tiny_inputs_on_the_device(e, dtype, torch, rsm):
    """noise scaled by 2^e: subnormal float32 sums and subnormal narrow outputs come out of the device as out of the
    simulator, bit for bit -- the build keeps them"""
    pair = inp.TINY_PAIR
    x = inp.tiny(1, e, seed=35)
    want, counts = sim_streams(pair, [x], "waveform", dtype=dtype, end=True)
    small, nonzero = inp.subnormals(want[0], dtype)
    assert small > 0
    keep, ptrs, frames = on_device(torch, [x])
    assert same_bits(keep[0].cpu().numpy(), x)                    # the inputs reach the device unflushed
    with rsm.Resampler(*pair, dtype=dtype, max_streams=1, max_frames=1) as rs:
        rs.resample(ptrs, frames, end=True)
        assert rs.counts() == counts
        got = gpu_streams(rs)[0]
    assert inp.subnormals(got, dtype) == (small, nonzero)
    assert same_bits(got, want[0])


# ------------------------------------------------------------------ many streams

def test_seventy_streams_in_frames_form(torch, rsm):
    """44100 -> 8000, FRAMES, chained: 70 streams with sparse ascending numbers up to max_streams - 1 = 95, three calls with
    0, 1 or 2 frames per stream in turn, END on the third, where every stream holds 209 to 627 samples of a partial frame.
    max_frames is exactly the largest call's total, and no call is refused for the buffer's capacity."""
    pair, top = (44100, 8000), 95
    numbers = sorted(int(v) for v in np.random.default_rng(5).choice(top, 69, replace=False)) + [top]
    assert len(numbers) == 70 == len(set(numbers))
    per_call = [[(i + c) % 3 for i in range(70)] for c in range(3)]
    xs = [ref.noise(3, seed=300 + i) for i in range(70)]
    state = SimState(top + 1)
    done = [0] * 70
    with rsm.Resampler(*pair, form="frames", max_streams=top + 1, max_frames=max(sum(f) for f in per_call)) as rs:
        for c, fr in enumerate(per_call):
            parts = [x[d:d + f] for x, d, f in zip(xs, done, fr)]
            if c == 2:
                leads = [ref.outputs(*pair, d * FRAME) % FRAME for d in done]
                assert sum(1 for v in leads if v) > 35 and set(leads) <= {0, 209, 418, 627}
            keep, ptrs, frames = on_device(torch, parts)
            rs.resample(ptrs, frames, numbers, chain=True, end=c == 2)
            want, counts = sim_streams(pair, parts, "frames", numbers=numbers, chain=True, end=c == 2, state=state)
            assert rs.counts() == counts and sum(counts) == (70 if c == 2 else 0)
            got = gpu_streams(rs)
            for i in range(70):
                assert same_bits(got[i], want[i]), (c, i, numbers[i])
            done = [d + f for d, f in zip(done, fr)]
        assert done == [3] * 70
        assert [rs.chain_info(s)[0] for s in range(top + 1)] == [False] * (top + 1)
