"""The PCM resampler on the device (C ABI part 11, jsmpeg_amd/resample.py) against the simulator of the same rule
(tests/sim/sim_resample.cpp): bits are asserted, never times.  A few frames per case.  The kernel's workgroup is 256 slots
(RS_WG in pcm_resample.h): with END's tail no count used here is a multiple of it, so every stream ends in a partial block
behind whole ones (streams of 1 and 3 frames take 2 to 19 blocks); without END 48000 -> 32000 ends on a block's edge.  Every test here fails without the feature: the module and the library's
jsmpeg_hip_resampler_* symbols do not exist.  Needs an MI355X."""
import numpy as np
import pytest

import resample_ref as ref
from resample_util import FRAME, SimState, sim_resample

pytestmark = pytest.mark.gpu

BLOCK = 256
PAIRS = [(48000, 16000), (44100, 16000), (32000, 44100), (44100, 48000), (48000, 32000)]
PAIR_IDS = ["%d_%d" % p for p in PAIRS]
#          channels, form, dtype, gain, end
VARIANTS = [(2, "waveform", "float32", 1.0, True), (1, "waveform", "float32", 1.0, False), (1, "waveform", "float16", 1.0, True),
            (2, "waveform", "bfloat16", 2.0, True), (2, "waveform", "float16", 1.0, False), (1, "waveform", "bfloat16", 1.0, True),
            (2, "frames", "float32", 1.0, True), (1, "frames", "float32", 2.0, True), (2, "frames", "float32", 1.0, False)]


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


@pytest.fixture(scope="module")
def inputs():
    """the streams every test shares: noise, so that no two samples agree by accident"""
    return [ref.noise(5, seed=100 + i) for i in range(4)]


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({2: np.uint16, 4: np.uint32}[a.dtype.itemsize])


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def on_device(torch, streams):
    """float32 [frames][2][1152] per stream -> (tensors to keep alive, device pointers, frame counts)"""
    keep = [torch.from_numpy(np.ascontiguousarray(s, dtype=np.float32)).cuda() for s in streams]
    torch.cuda.synchronize()
    return keep, [t.data_ptr() if len(s) else 0 for t, s in zip(keep, streams)], [len(s) for s in streams]


def gpu_streams(rs):
    """the last call's result per stream of the call, cut to its count: waveform [channels][count], frames [count][2][1152]"""
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


@pytest.mark.parametrize("pair", PAIRS, ids=PAIR_IDS)
def test_kernel_equals_the_simulator_bit_for_bit(pair, torch, hip_lib, inputs):
    """three streams of 0, 1 and 3 frames in one call; stereo and mono, both forms, the three types, a gain of 2.0"""
    from jsmpeg_amd import resample
    xs = [inputs[0][:0], inputs[1][:1], inputs[2][:3]]
    keep, ptrs, frames = on_device(torch, xs)
    for channels, form, dtype, gain, end in VARIANTS:
        want, counts = sim_streams(pair, xs, form, channels=channels, dtype=dtype, gain=gain, end=end)
        with resample.Resampler(*pair, channels=channels, form=form, dtype=dtype, gain=gain, max_streams=3, max_frames=4) as rs:
            rs.resample(ptrs, frames, end=end)
            assert rs.counts() == counts and counts[0] == 0
            if form == "waveform":
                assert counts[2] > BLOCK and (not end or (counts[1] % BLOCK and counts[2] % BLOCK))      # with the tail: a partial last block
                assert rs.row == resample.outputs(*pair, 4 * FRAME + rs.plan[2]) and rs.row % BLOCK
            got = gpu_streams(rs)
            for i in range(3):
                assert same_bits(got[i], want[i]), (pair, channels, form, dtype, gain, end, i)
            t = rs.timings()
            assert t["total_ms"] >= t["kernel_ms"] > 0
            if form == "waveform":
                w = rs.waveform()
                assert tuple(w.shape) == (3, channels, rs.row) and str(w.dtype) == "torch." + dtype and w.data_ptr() == rs.device_out()[0]
                host = w.cpu()
                assert np.array_equal(bits(host.view(torch.int16).numpy() if dtype != "float32" else host.numpy()), bits(rs.read()))


def test_tensor_on_another_torch_stream(torch, hip_lib, inputs):
    """resample_tensor right behind the kernel that produced the tensor, on a non-default torch stream"""
    from jsmpeg_amd import resample
    pair = (48000, 16000)
    xs = np.stack([inputs[0][:2], inputs[1][:2]])
    half = torch.from_numpy(xs * np.float32(0.5)).cuda()
    torch.cuda.synchronize()
    want, counts = sim_streams(pair, [xs[0], xs[1]], "waveform", channels=1, dtype="float16", end=True)
    with resample.Resampler(*pair, channels=1, dtype="float16", max_streams=2, max_frames=4) as rs:
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            x = half * 2.0                                        # exact: the simulator's input is xs
            rs.resample_tensor(x, end=True)
        got = gpu_streams(rs)
        assert same_bits(got[0], want[0]) and same_bits(got[1], want[1])
        assert rs.delay_seconds == 48 / 48000
        with pytest.raises(ValueError):
            rs.resample_tensor(x.double())


@pytest.mark.parametrize("form", ["waveform", "frames"])
@pytest.mark.parametrize("pair", [(44100, 16000), (32000, 44100), (48000, 32000)], ids=["44100_16000", "32000_44100", "48000_32000"])
def test_chains_on_the_device(pair, form, torch, hip_lib, inputs):
    """streams 0 and max_streams - 1: 1 + 2 frames over two calls equal 3 in one; five single calls (the carries swap each
    time) equal one call; a stream absent from the middle call keeps its state; chain_reset starts from zeros"""
    from jsmpeg_amd import resample
    top = 5
    x, y = inputs[0], inputs[1]
    whole, _ = sim_streams(pair, [x, y], form, end=True)
    whole3, _ = sim_streams(pair, [x[:3], y[:3]], form)
    cat = (lambda parts: np.concatenate(parts, axis=0)) if form == "frames" else (lambda parts: np.concatenate(parts, axis=1))
    with resample.Resampler(*pair, form=form, max_streams=top + 1, max_frames=6) as rs:
        def call(parts, numbers, end=False):
            keep, ptrs, frames = on_device(torch, parts)
            rs.resample(ptrs, frames, numbers, chain=True, end=end)
            return gpu_streams(rs)
        # 1 + 2 = 3
        a = call([x[:1], y[:1]], [0, top])
        b = call([x[1:3], y[1:3]], [0, top])
        assert same_bits(cat([a[0], b[0]]), whole3[0]) and same_bits(cat([a[1], b[1]]), whole3[1])
        assert rs.chain_info(0) == (True, 3 * FRAME, resample.outputs(*pair, 3 * FRAME)) == rs.chain_info(top)
        assert rs.chain_info(1) == (False, 0, 0)
        # chain_reset: from zeros again.  Stream 0 in five single calls, stream `top` as 1 + 0 + 4 in the same calls
        rs.chain_reset()
        assert rs.chain_info(0) == (False, 0, 0) == rs.chain_info(top)
        got0, got1 = [], []
        for k, n1 in enumerate((1, 0, 4, 0, 0)):
            done1 = sum((1, 0, 4, 0, 0)[:k])
            r = call([x[k:k + 1], y[done1:done1 + n1]], [0, top], end=k == 4)
            got0.append(r[0])
            got1.append(r[1])
            if k == 1:
                assert rs.chain_info(top) == (True, FRAME, resample.outputs(*pair, FRAME))      # absent from the call: untouched
        assert same_bits(cat(got0), whole[0]) and same_bits(cat(got1), whole[1])
        assert rs.chain_info(0) == (False, 0, 0) == rs.chain_info(top)                           # END with CHAIN ends the chains
        # the same state in the simulator: stream 0 goes on, stream 1 begins, stream `top` was reset alone
        state = SimState(top + 1)
        call([x[:2], y[:2]], [0, top])
        sim_resample(*pair, [x[:2], y[:2]], form=form, numbers=[0, top], chain=True, state=state)
        rs.chain_reset(top)
        state.reset(top)
        parts = [x[2:4], inputs[2][:1], y[2:3]]
        got = call(parts, [0, 1, top])
        want, _ = sim_streams(pair, parts, form, numbers=[0, 1, top], chain=True, state=state)
        assert all(same_bits(g, w) for g, w in zip(got, want))
        assert same_bits(got[2], sim_streams(pair, [y[2:3]], form)[0][0])                          # the reset stream: as from nothing
        assert [rs.chain_info(s) for s in (0, 1, top)] == [state.info(s) for s in (0, 1, top)]


def test_from_the_decoders(torch, hip_lib):
    """resample_batch over an Mp2Batch decode of a generated stream equals the simulator over read_pcm; resample_live over
    the same stream written in two ticks equals the batch result, bit for bit"""
    from jsmpeg_amd import mp2, resample, synth
    pair = (48000, 16000)
    audio, offs = synth.generate_mp2_config("mp2_joint_48k_128", 4)
    bounds = [int(o) for o in offs] + [len(audio)]
    with mp2.Mp2Batch(1, len(audio) + 64) as b, resample.Resampler(*pair, channels=1, dtype="float16", max_streams=2, max_frames=4) as rs:
        b.upload([audio])
        assert b.decode() == 4
        pcm = b.read_pcm(0)
        want, counts = sim_streams(pair, [pcm], "waveform", channels=1, dtype="float16", end=True)
        rs.resample_batch(b, end=True)
        assert rs.counts() == counts == [resample.outputs(*pair, 4 * FRAME + 48)]
        batch_result = gpu_streams(rs)[0]
        assert same_bits(batch_result, want[0]) and batch_result.any()
    with mp2.Mp2Batch(1, len(audio) + 64) as b, resample.Resampler(44100, 16000, max_streams=1, max_frames=4) as rs:
        b.upload([audio])
        b.decode()
        with pytest.raises(ValueError, match="48000"):
            rs.resample_batch(b)
    with mp2.Mp2Live(2, max_frames_per_tick=2) as live, resample.Resampler(*pair, channels=1, dtype="float16", max_streams=2, max_frames=4) as rs:
        live.open()
        a = live.open()                                           # live id 1 is the stream number
        pieces = []
        for tick in range(2):
            live.write(a, tick * 0.05, audio[bounds[2 * tick]:bounds[2 * tick + 2]])
            assert live.tick() == 2
            frames = rs.resample_live(live, end=tick == 1)
            assert [f["stream"] for f in frames] == [a, a] and rs._numbers == [a]
            pieces.append(gpu_streams(rs)[0])
        assert same_bits(np.concatenate(pieces, axis=1), batch_result)
        assert rs.chain_info(a) == (False, 0, 0)


def test_into_the_encoder(torch, hip_lib, inputs):
    """FRAMES 48000 -> 32000 with gain 2.0: frames() goes to Mp2Encoder(sample_rate_index=2) with chain=True, over two calls,
    resampler and encoder on ONE HIP stream with no host wait between them; the encoder's bytes equal those of encode_tensor
    over the simulator's frames, and the frame sizes are the closed form"""
    from jsmpeg_amd import mp2_encode, resample
    pair, cfg = (48000, 32000), (2, 2, 4)                          # 32 kHz, stereo, 64 kbit/s
    x = inputs[3] * np.float32(0.25)
    state, sim_frames = SimState(1), []
    side = torch.cuda.Stream()
    es = b""
    sizes = []
    with resample.Resampler(*pair, form="frames", gain=2.0, max_streams=1, max_frames=3) as rs, \
            mp2_encode.Mp2Encoder(*cfg, 1, 4, 1 << 14) as enc, mp2_encode.Mp2Encoder(*cfg, 1, 4, 1 << 14) as enc2:
        for lo, hi in ((0, 2), (2, 5)):
            keep, ptrs, frames = on_device(torch, [x[lo:hi]])
            rs.resample(ptrs, frames, chain=True, stream=side.cuda_stream)
            p, counts, numbers = rs.frames()                       # closed form: nothing waited for
            enc.encode(p, counts, numbers, chain=True, stream=side.cuda_stream)
            es += enc.es(0)                                        # settles the encoder, and with it the resampler's pass in front of it
            sizes += [b for _, b in enc.frame_ranges()]
            rs.sync()
            f, n = sim_resample(*pair, [x[lo:hi]], form="frames", gain=2.0, chain=True, state=state)
            assert counts == n and same_bits(rs.read(), f[0])
            sim_frames.append(f[0])
        sim_frames = np.concatenate(sim_frames)
        assert len(sim_frames) == 5 * FRAME * 2 // 3 // FRAME == 3
        enc2.encode_tensor(torch.from_numpy(sim_frames[None]).cuda())
        assert es == enc2.es(0) and len(es) > 0
        assert sizes == [mp2_encode.frame_bytes(n, cfg[0], cfg[2]) for n in range(3)] and sum(sizes) == len(es)
        assert enc.chain_info(0) == (True, 3)


def test_refusals(torch, hip_lib, inputs):
    """each returns an error, launches nothing -- no state moves -- and a correct call right after works"""
    from jsmpeg_amd import resample
    pair = (48000, 16000)
    xs = [inputs[0][:2], inputs[1][:1]]
    keep, ptrs, frames = on_device(torch, xs)
    want, counts = sim_streams(pair, xs, "waveform")
    for bad in ((48000, 48000), (32000, 32000), (22050, 16000), (48000, 12000), (0, 0)):
        with pytest.raises(RuntimeError, match="not a supported pair"):
            resample.Resampler(*bad, max_streams=1, max_frames=1)
    with pytest.raises(RuntimeError, match="channels_out"):
        resample.Resampler(*pair, channels=3)
    with pytest.raises(RuntimeError, match="FRAMES: F32"):
        resample.Resampler(*pair, form="frames", dtype="float16")

    def good(rs, numbers=None):
        rs.resample(ptrs, frames, numbers)
        got = gpu_streams(rs)
        assert same_bits(got[0], want[0]) and same_bits(got[1], want[1])

    with resample.Resampler(*pair, max_streams=4, max_frames=3) as rs:
        with pytest.raises(RuntimeError, match="nothing was resampled"):
            rs.device_out()
        with pytest.raises(RuntimeError, match="max_frames"):
            rs.resample([ptrs[0], ptrs[0]], [2, 2], chain=True)
        good(rs)
        with pytest.raises(RuntimeError, match="ascend"):
            rs.resample(ptrs, frames, [2, 1], chain=True)
        good(rs)
        with pytest.raises(RuntimeError, match="ascend"):
            rs.resample(ptrs, frames, [1, 1], chain=True)
        with pytest.raises(RuntimeError, match="max_streams"):
            rs.resample(ptrs, frames, [1, 4], chain=True)
        with pytest.raises(RuntimeError, match="NULL"):
            rs.resample([0, ptrs[1]], frames, chain=True)
        with pytest.raises(RuntimeError, match="unknown flags"):
            rs._ok(rs.L.jsmpeg_hip_resampler_resample(rs.h, None, None, None, 0, 4, None))
        assert [rs.chain_info(s)[0] for s in range(4)] == [False] * 4
        good(rs, [1, 3])
        rs.resample(ptrs, frames, chain=True)
        assert rs.query() in (False, True)
        assert rs.counts() == counts                              # closed form: answered while the pass may still run
        with pytest.raises(RuntimeError, match="in flight"):
            rs.resample(ptrs, frames, chain=True)
        with pytest.raises(RuntimeError, match="in flight"):
            rs.chain_reset()
        rs.sync()
        assert rs.query() is True
        assert rs.chain_info(0) == (True, 2 * FRAME, counts[0])   # the refused second call moved nothing
        rs.chain_reset()
        good(rs)
        rs.resample([], [])                                       # a call without streams is a call
        assert rs.device_out()[1] == 0 and rs.counts() == []
    with resample.Resampler(*pair, max_streams=2, max_frames=3, row=counts[0] - 1) as rs:
        with pytest.raises(RuntimeError, match="row is %d" % (counts[0] - 1)):
            rs.resample(ptrs, frames, chain=True)
        assert rs.chain_info(0) == (False, 0, 0)
        rs.resample(ptrs[1:], frames[1:])                         # the shorter stream fits
        assert same_bits(gpu_streams(rs)[0], want[1])
    with resample.Resampler(*pair, max_streams=2, max_frames=3, row=counts[0]) as rs:
        good(rs)                                                  # a count equal to row fits
