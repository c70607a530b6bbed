"""k_logmel on the GPU against the simulator, bit for bit (C ABI part 12) -- which is also the check that v_mfma_f32_32x32x2_f32
IS the k-ascending fmaf chain the rule writes: the simulator runs that chain with fmaf.  Stream lengths sit on the tile's edges
(F = 32 frames per workgroup) and the four configs end in different last columns of the padded basis.  Every test here fails
without the feature: the module and the library's jsmpeg_hip_logmel_* symbols do not exist."""
import numpy as np
import pytest

from logmel_util import CONFIGS, WHISPER, F, chain_splits, frames_axis, sim_features

pytestmark = pytest.mark.gpu

KEYS = list(CONFIGS)
IDS = ["%d_%d_%d" % k for k in KEYS]


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({2: np.uint16, 4: np.uint32}[a.dtype.itemsize])


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def noise(n, seed, amp=0.5):
    return (np.random.default_rng(seed).uniform(-1.0, 1.0, n) * amp).astype(np.float32)


def on_device(torch, streams):
    """float32 samples per stream -> (tensors to keep alive, device pointers, counts)"""
    keep = [torch.from_numpy(np.ascontiguousarray(s, dtype=np.float32)).cuda() for s in streams]
    torch.cuda.synchronize()
    return keep, [t.data_ptr() if len(s) else 0 for t, s in zip(keep, streams)], [len(s) for s in streams]


def edge_lengths(n_fft, hop):
    """0, h, h + 1, 3 hop + h -+ 1 samples, and END frame counts of F - 1, F, F + 1 and 2 F + 1"""
    h = n_fft // 2
    return [0, h, h + 1, 3 * hop + h - 1, 3 * hop + h + 1] + [(t - 1) * hop + hop // 2 for t in (F - 1, F, F + 1, 2 * F + 1)]


@pytest.fixture(scope="module")
def edge_streams():
    return {key: [noise(n, 200 + i) for i, n in enumerate(edge_lengths(key[0], key[1]))] for key in KEYS}


@pytest.mark.parametrize("key", KEYS, ids=IDS)
def test_kernel_equals_the_simulator_bit_for_bit(key, torch, hip_lib, edge_streams):
    from jsmpeg_amd import logmel
    n_fft, hop = key[0], key[1]
    xs = edge_streams[key]
    keep, ptrs, counts = on_device(torch, xs)
    row = 2 * F + 3
    for end in (True, False):
        cfg = dict(CONFIGS[key], scale="log10", row=row)
        want, frames = sim_features(xs, end=end, **cfg)
        if end:
            assert frames[:3] == [0, 0, (n_fft // 2 + 1) // hop + 1] and frames[-4:] == [F - 1, F, F + 1, 2 * F + 1]
        with logmel.LogMel(max_streams=len(xs), max_samples=max(counts), **cfg) as lm:
            lm.features(ptrs, counts, end=end)
            assert lm.counts() == frames
            got = lm.read()
            assert same_bits(got, want) and np.isfinite(got).all()
            assert [lm.stream_out(i) for i in range(len(xs))] == [(i * key[2] * row, frames[i]) for i in range(len(xs))]
            t = lm.tensor()
            assert tuple(t.shape) == want.shape and same_bits(t.cpu().numpy(), want)


def test_each_scale_both_layouts_three_dtypes(torch, hip_lib):
    from jsmpeg_amd import logmel
    xs = [noise(0, 1), noise(5 * 160 + 400, 2), noise(300, 3, 0.01), noise((F + 1) * 160, 4)]
    keep, ptrs, counts = on_device(torch, xs)
    for scale in ("power", "log", "log10", "db", "whisper"):
        for layout in ("mel_major", "time_major"):
            for dtype in ("float32", "float16", "bfloat16"):
                cfg = dict(WHISPER, scale=scale, layout=layout, dtype=dtype, row=F + 4)
                want, frames = sim_features(xs, end=True, **cfg)
                with logmel.LogMel(max_streams=4, max_samples=max(counts), **cfg) as lm:
                    lm.features(ptrs, counts)
                    assert lm.counts() == frames == [0, 8, 2, F + 2]
                    assert same_bits(lm.read(), want), (scale, layout, dtype)
                    if dtype == "bfloat16" and scale == "whisper":
                        assert np.array_equal(lm.tensor().view(torch.int16).cpu().numpy().view(np.uint16), want)


def test_a_user_window_and_an_odd_hop(torch, hip_lib):
    """hop = 2 mod 4 and an odd hop take the unskewed LDS map; a window that is not symmetric"""
    from jsmpeg_amd import logmel
    w = np.linspace(0.05, 1.0, 64).astype(np.float32)
    xs = [noise(40 * 21 + 7, 5), noise(33, 6)]
    keep, ptrs, counts = on_device(torch, xs)
    for hop in (21, 22):
        cfg = dict(sample_rate=8000, n_fft=64, hop=hop, n_mels=20, mel_scale="htk", mel_norm="none", scale="db", window=w, row=45)
        want, frames = sim_features(xs, end=True, **cfg)
        with logmel.LogMel(max_streams=2, max_samples=max(counts), **cfg) as lm:
            lm.features(ptrs, counts)
            assert lm.counts() == frames and same_bits(lm.read(), want)


@pytest.mark.parametrize("end", [False, True], ids=["open", "end"])
def test_chains_on_the_device(end, torch, hip_lib):
    """the CPU tests' split list with three streams (numbers 0, 1 and max_streams - 1) in the same calls, then two streams with
    different splits; every piece is read from the device and the pieces concatenated equal the simulator's single call.  The
    carries swap on every call with samples, so both are used many times."""
    from jsmpeg_amd import logmel
    n, splits = chain_splits(400, 160)
    top = 4
    xs = [noise(n, 300 + i) for i in range(3)]
    keep, ptrs, _ = on_device(torch, xs)
    cfg = dict(WHISPER, scale="log10", row=12)
    whole, counts = sim_features(xs, end=end, **cfg)
    whole = frames_axis(whole, "mel_major")

    def run(lm, calls, numbers):
        done = [0] * len(numbers)
        out = [[] for _ in numbers]
        for k, call in enumerate(calls):
            lm.features([ptrs[s] + 4 * done[s] for s in range(len(numbers))], call, streams=numbers, chain=True, end=end and k + 1 == len(calls))
            got = frames_axis(lm.read(), "mel_major")
            for s, c in enumerate(lm.counts()):
                out[s].append(got[s, :c])
                done[s] += call[s]
        return [np.concatenate(o) for o in out]

    with logmel.LogMel(max_streams=top + 1, max_samples=n, **cfg) as lm:
        for split in splits:
            got = run(lm, [[p] * 3 for p in split], [0, 1, top])
            for s in range(3):
                assert same_bits(got[s], whole[s, :counts[s]]), (split, s)
            assert lm.chain_info(top) == ((False, 0, 0) if end else (True, n, counts[2]))
            lm.chain_reset()
            assert lm.chain_info(0) == (False, 0, 0)
        a, b = splits[4], splits[-3]
        got = run(lm, [[a[0], b[0]], [0, b[1]], [a[1], b[2]], [0, b[3]], [0, b[4]], [0, b[5]]], [1, 3])
        assert same_bits(got[0], whole[0, :counts[0]]) and same_bits(got[1], whole[1, :counts[1]])
        lm.chain_reset()
        # an unchained call in between touches no state
        lm.features([ptrs[2]], [700], streams=[2], chain=True, end=False)
        first = frames_axis(lm.read(), "mel_major")[0, :lm.counts()[0]]
        lm.features([ptrs[0]], [n], streams=[2])
        lm.sync()
        lm.features([ptrs[2] + 4 * 700], [n - 700], streams=[2], chain=True, end=end)
        second = frames_axis(lm.read(), "mel_major")[0, :lm.counts()[0]]
        assert same_bits(np.concatenate([first, second]), whole[2, :counts[2]])


def test_decode_resample_features_on_one_stream_without_a_wait(torch, hip_lib):
    """Mp2Batch.decode -> Resampler.resample_batch -> LogMel.features(resampler) enqueued on ONE HIP stream; no sync() of the
    resampler or of the features handle in between.  The result equals the simulator fed the resampler's read-out."""
    from jsmpeg_amd import logmel, mp2, resample, synth
    audio, _ = synth.generate_mp2_config("mp2_joint_48k_128", 4)
    side = torch.cuda.Stream()
    with mp2.Mp2Batch(1, len(audio) + 64) as b, resample.Resampler(48000, 16000, channels=2, max_streams=1, max_frames=4) as rs:
        b.upload([audio])
        assert b.decode(side.cuda_stream, sync=False) == 4
        rs.resample_batch(b, end=True, stream=side.cuda_stream)
        valid = rs.counts()[0]
        for channel, counts in ((0, None), (1, "row")):
            cfg = dict(WHISPER, scale="whisper", dtype="float16", row=(rs.row + 200) // 160 + 2)
            with logmel.LogMel(max_streams=1, max_samples=rs.row, **cfg) as lm:
                lm.features(rs, counts=counts, channel=channel, stream=side.cuda_stream)
                frames = lm.stream_out(0)[1]
                got = lm.read()
                wave = rs.read()
                x = wave[0, channel] if counts == "row" else wave[0, channel, :valid]
                want, c = sim_features([x], end=True, **cfg)
                assert c == [frames] == [len(x) // 160 + 1] and same_bits(got, want) and wave[0, channel].any()
        with resample.Resampler(48000, 16000, channels=1, dtype="float16", max_streams=1, max_frames=4) as half, \
                logmel.LogMel(max_streams=1, max_samples=half.row, **WHISPER) as lm:
            half.resample_batch(b, end=True)
            with pytest.raises(ValueError, match="form='waveform' and dtype='float32'"):
                lm.features(half)


def test_tensor_on_another_torch_stream_and_a_second_call(torch, hip_lib):
    """features(tensor) right behind the kernel that produced the tensor, on a non-default torch stream; then a second call on
    the same handle, whose stream_out before sync agrees with the counts after it"""
    from jsmpeg_amd import logmel
    n = 9 * 160 + 123
    x = np.stack([noise(n, 400), noise(n, 401)])
    cfg = dict(WHISPER, scale="db", layout="time_major", row=12)
    side = torch.cuda.Stream()
    with logmel.LogMel(max_streams=2, max_samples=n, **cfg) as lm:
        host = torch.from_numpy(x).pin_memory()
        with torch.cuda.stream(side):
            t = host.to("cuda", non_blocking=True) * 2.0
            lm.features(t, counts=[n, 500])
        want, frames = sim_features([x[0] * np.float32(2.0), x[1, :500] * np.float32(2.0)], end=True, **cfg)
        before = [lm.stream_out(s) for s in range(2)]
        assert [c for _, c in before] == frames
        assert same_bits(lm.read(), want)
        with torch.cuda.stream(side):
            lm.features(t, counts=[300, n], end=False)
        before = [lm.stream_out(s) for s in range(2)]
        lm.sync()
        assert lm.query() and [lm.stream_out(s) for s in range(2)] == before and lm.counts() == [c for _, c in before]
        want, frames = sim_features([x[0, :300] * np.float32(2.0), x[1] * np.float32(2.0)], end=False, **cfg)
        assert lm.counts() == frames and same_bits(lm.read(), want)
        assert lm.timings()["kernel_ms"] > 0


def test_refusals_on_the_device(torch, hip_lib):
    from jsmpeg_amd import logmel
    xs = [noise(5 * 160 + 400, 500)]
    keep, ptrs, counts = on_device(torch, xs)
    want, frames = sim_features(xs, end=True, scale="whisper", row=8, **WHISPER)
    with logmel.LogMel(max_streams=1, max_samples=counts[0], scale="whisper", row=7, **WHISPER) as lm:
        with pytest.raises(RuntimeError, match="row is 7"):
            lm.features(ptrs, counts)
        with pytest.raises(RuntimeError, match="refused with CHAIN"):
            lm.features(ptrs, counts, chain=True)
        with pytest.raises(RuntimeError, match="max_samples"):
            lm.features(ptrs, [counts[0] + 1])
        with pytest.raises(RuntimeError, match="max_streams"):
            lm.features(ptrs * 2, counts * 2)
        with pytest.raises(RuntimeError, match="no features"):
            lm.device_out()
        lm.features(ptrs, [counts[0] - 160])                      # one frame fewer fits
        assert lm.counts() == [7] and lm.read().shape == (1, 80, 7)
    with logmel.LogMel(max_streams=1, max_samples=counts[0], scale="whisper", row=8, **WHISPER) as lm:
        lm.features(ptrs, counts)
        with pytest.raises(RuntimeError, match="in flight"):
            lm.features(ptrs, counts)
        assert same_bits(lm.read(), want)
    for bad in (dict(n_fft=401), dict(hop=201), dict(max_streams=0)):
        with pytest.raises((RuntimeError, ValueError)):
            logmel.LogMel(**dict(dict(WHISPER, max_streams=1, max_samples=16), **bad))
