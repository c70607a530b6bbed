"""The MP2 encoder on the device (C ABI part 9, jsmpeg_amd/mp2_encode.py) against the simulator of the same rule
(tests/sim/sim_mp2_enc.cpp): bytes are asserted, never times.  Every test here fails without the feature: the module and the
library's jsmpeg_hip_mp2_encoder_* symbols do not exist.  Needs an MI355X."""
import ctypes

import numpy as np
import pytest

import mp2_enc_inputs as inputs
from mp2_enc_util import SimState, oracle_decode, sim_encode
from mp2_util import FIXTURES, FIXTURE_IDS, load_case, same_bits

pytestmark = pytest.mark.gpu

KINDS = ("sine", "noise", "square", "wild")
S44 = inputs.CONFIGS["stereo_44k_192"]


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


def on_device(torch, streams):
    """float32 [frames][2][1152] per stream -> (tensors to keep alive, device pointers, frame counts)"""
    keep = [torch.from_numpy(np.ascontiguousarray(s, dtype=np.float32)).cuda() for s in streams]
    torch.cuda.synchronize()
    return keep, [t.data_ptr() if len(s) else 0 for t, s in zip(keep, streams)], [len(s) for s in streams]


def whole_es(enc):
    from jsmpeg_amd import batch
    p, total = enc.device_es()
    out = np.zeros(max(1, total), dtype=np.uint8)
    L = batch.lib()
    L.jsmpeg_hip_device_read.restype = ctypes.c_int
    L.jsmpeg_hip_device_read.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64]
    if total:
        assert L.jsmpeg_hip_device_read(out.ctypes.data, p, total) == 0
    return out[:total]


def check_layout(enc, numbers, pieces):
    """stream ranges: 16-byte aligned begins, zeros up to the next multiple of 16, the frames tile the streams"""
    es, at = whole_es(enc), 0
    ranges, k = enc.frame_ranges(), 0
    for s, want in zip(numbers, pieces):
        b, e = enc.stream_range(s)
        assert b == at and b % 16 == 0 and e - b == len(want) and es[b:e].tobytes() == want, s
        at = (e + 15) & ~15
        assert not es[e:at].any()
        pos = b
        while pos < e:
            assert ranges[k][0] == pos
            pos += ranges[k][1]
            k += 1
        assert pos == e
    assert at == len(es) and k == len(ranges)


@pytest.mark.parametrize("name", list(inputs.CONFIGS))
def test_gpu_bytes_equal_the_simulator(name, torch, hip_lib):
    from jsmpeg_amd import mp2_encode
    cfg = inputs.CONFIGS[name]
    xs = [inputs.pcm(k, inputs.RATES[cfg[0]], 3) for k in KINDS]
    want, stats = sim_encode(cfg, xs)
    keep, ptrs, frames = on_device(torch, xs)
    with mp2_encode.Mp2Encoder(cfg[0], cfg[1], cfg[2], 4, 12, mp2_encode.es_bytes(frames, cfg[0], cfg[2])) as enc:
        enc.encode(ptrs, frames)
        for s in range(4):
            assert enc.es(s) == want[s], (name, KINDS[s])
        check_layout(enc, range(4), want)
        for k in range(12):
            st = enc.frame_stats(k)
            assert [st["coded_pairs"], st["bits_used"], st["bits_left"], st["top_code"]] == [int(v) for v in stats[k]]
        t = enc.timings()
        assert t["total_ms"] >= t["kernel_ms"] > 0


def test_streams_of_unequal_length_and_numbers_with_gaps(torch, hip_lib):
    from jsmpeg_amd import mp2_encode
    xs = [inputs.pcm(k, 44100, n, seed=i) for i, (k, n) in enumerate((("sine", 3), ("noise", 0), ("square", 1), ("wild", 2), ("sweep", 3)))]
    numbers = [0, 2, 3, 5, 6]
    want, _ = sim_encode(S44, xs, numbers=numbers)
    keep, ptrs, frames = on_device(torch, xs)
    with mp2_encode.Mp2Encoder(*S44, 8, 9, 1 << 16) as enc:
        enc.encode(ptrs, frames, numbers)
        assert [enc.es(s) for s in numbers] == want and want[1] == b""
        check_layout(enc, numbers, want)
        assert enc.stream_range(1) == (0, 0) and enc.stream_range(7) == (0, 0)
        assert enc.ts_units()[2] == [0, 0, 0, 3, 5, 5, 6, 6, 6]


def test_chain_across_calls(torch, hip_lib):
    """three streams, calls of (1, 2, 1), (2, 0, 1), (1, 1, 1) frames: each stream's pieces concatenated equal one unchained
    call; chain_reset of one stream, chain_info, a chained call on a stream without state"""
    from jsmpeg_amd import mp2_encode
    xs = [inputs.pcm(k, 44100, 4, seed=10 + i) for i, k in enumerate(("noise", "sine", "sweep"))]
    xs[1] = xs[1][:3]
    xs[2] = xs[2][:3]
    whole, _ = sim_encode(S44, xs)
    with mp2_encode.Mp2Encoder(*S44, 4, 8, 1 << 16) as enc:
        done, pieces = [0, 0, 0], [b"", b"", b""]
        for call in ((1, 2, 1), (2, 0, 1), (1, 1, 1)):
            parts = [x[d:d + n] for x, d, n in zip(xs, done, call)]
            keep, ptrs, frames = on_device(torch, parts)
            enc.encode(ptrs, frames, [0, 1, 3], chain=True)
            for i, s in enumerate((0, 1, 3)):
                pieces[i] += enc.es(s)
                done[i] += call[i]
                assert enc.chain_info(s) == (True, done[i])
            assert enc.chain_info(2) == (False, 0)
        assert pieces == whole
        # an unchained call in between touches nothing; then stream 1 alone is reset
        keep, ptrs, frames = on_device(torch, [xs[0][:1]])
        enc.encode(ptrs, frames, [1])
        assert enc.es(1) == whole[0][:len(enc.es(1))] and enc.chain_info(1) == (True, 3)
        enc.chain_reset(1)
        assert enc.chain_info(1) == (False, 0) and enc.chain_info(0) == (True, 4)
        state = SimState(4)                                       # the same history in the simulator: stream 0 goes on, 1 and 2 begin
        sim_encode(S44, [xs[0]], numbers=[0], chain=True, state=state)
        more = [inputs.pcm("noise", 44100, 2, seed=20 + i) for i in range(3)]
        want, _ = sim_encode(S44, more, numbers=[0, 1, 2], chain=True, state=state)
        keep, ptrs, frames = on_device(torch, more)
        enc.encode(ptrs, frames, [0, 1, 2], chain=True)
        assert [enc.es(s) for s in (0, 1, 2)] == want
        assert want[1] == sim_encode(S44, [more[1]])[0][0] and want[0] != sim_encode(S44, [more[0]])[0][0]
        assert [enc.chain_info(s) for s in range(4)] == [(True, 6), (True, 2), (True, 2), (True, 3)]
        enc.encode(ptrs, frames, [0, 1, 2], chain=True, end=True)   # END with CHAIN: the call's chains end behind it
        assert [enc.chain_info(s) for s in range(4)] == [(False, 0), (False, 0), (False, 0), (True, 3)]


def test_hand_off_on_the_device(torch, hip_lib, libs):
    """Mp2Batch.upload_device straight from device_es() with the stream ranges: PCM bit-equal to the oracle's decode of es()"""
    from jsmpeg_amd import mp2, mp2_encode
    xs = [inputs.pcm("sweep", 44100, 3), inputs.pcm("noise", 44100, 2, seed=5)]
    keep, ptrs, frames = on_device(torch, xs)
    with mp2_encode.Mp2Encoder(*S44, 2, 5, 1 << 15) as enc, mp2.Mp2Batch(2, 1 << 15) as back:
        enc.encode(ptrs, frames)
        p, total = enc.device_es()
        ranges = [enc.stream_range(s) for s in range(2)]
        back.upload_device(p, total, [r[0] for r in ranges], [r[1] for r in ranges])
        assert back.decode() == 5
        for s in range(2):
            want, sizes = oracle_decode(libs, enc.es(s))
            assert len(want) == frames[s] and same_bits(back.read_pcm(s), want)


def test_transcode_from_an_mp2_batch(torch, hip_lib):
    """encode_batch from the Mp2Batch that decoded the fixture mp2_stereo_44k_192: the simulator's bytes for that PCM"""
    from jsmpeg_amd import mp2, mp2_encode
    fx, data, offs = load_case(FIXTURES[FIXTURE_IDS.index("stereo_44k_192")])
    with mp2.Mp2Batch(1, len(data) + 64) as b, mp2_encode.Mp2Encoder(*S44, 1, fx["n_frames"], 1 << 16) as enc:
        b.upload([data])
        n = b.decode()
        pcm = b.read_pcm(0)
        want, _ = sim_encode(S44, [pcm])
        enc.encode_batch(b)
        assert enc.count == n == fx["n_frames"] and enc.es(0) == want[0]
    with mp2.Mp2Batch(1, len(data) + 64) as b, mp2_encode.Mp2Encoder(1, 2, 10, 1, fx["n_frames"], 1 << 16) as enc:
        b.upload([data])
        b.decode()
        with pytest.raises(ValueError, match="44100"):
            enc.encode_batch(b)


def test_tensor_on_another_torch_stream(torch, hip_lib):
    """encode_tensor right behind the kernel that produced the tensor, on a non-default torch stream"""
    from jsmpeg_amd import mp2_encode
    xs = np.stack([inputs.pcm("noise", 44100, 3, seed=30 + i) for i in range(2)])
    half = torch.from_numpy(xs * np.float32(0.5)).cuda()
    torch.cuda.synchronize()
    with mp2_encode.Mp2Encoder(*S44, 2, 6, 1 << 15) as enc:
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            x = half * 2.0                                        # exact: the simulator's input is xs
            enc.encode_tensor(x)
        want, _ = sim_encode(S44, [xs[0], xs[1]])
        assert [enc.es(0), enc.es(1)] == want
        with pytest.raises(ValueError):
            enc.encode_tensor(x.double())


def test_ts_units_through_the_device_mux(torch, hip_lib, libs):
    """ts_units() -> encode.ts_mux_device(stream_id 0xC0, pid 0x101), counters carried over two chained calls; the packets
    through Mp2Batch.upload_ts: read_bytes is the ES, one write per frame with the default PTS, PCM bit-equal to the direct decode"""
    from jsmpeg_amd import encode, mp2, mp2_encode
    xs = [inputs.pcm("sine", 44100, 5, seed=40), inputs.pcm("noise", 44100, 4, seed=41)]
    ts, es, pts, cc = [b"", b""], [b"", b""], [[], []], None
    with mp2_encode.Mp2Encoder(*S44, 2, 6, 1 << 15) as enc:
        for call in ((3, 2), (2, 2)):
            done = [len(p) for p in pts]
            keep, ptrs, frames = on_device(torch, [x[d:d + n] for x, d, n in zip(xs, done, call)])
            enc.encode(ptrs, frames, chain=True)
            ranges, seconds, numbers = enc.ts_units()
            dev_es, total = enc.device_es()
            cap = encode.ts_bound(total, len(ranges), 2)
            out = torch.zeros(cap, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            n, where, cc_out = encode.ts_mux_device(dev_es, ranges, seconds, out.data_ptr(), cap, numbers, 2, stream_id=0xC0, pid=0x101, continuity=cc)
            host = out.cpu().numpy()
            for s in range(2):
                b, e = where[s]
                assert (e - b) % 188 == 0 and e > b
                if cc is not None:
                    assert host[b + 3] & 15 == cc[s]              # the stream's first packet goes on where the last call stopped
                ts[s] += host[b:e].tobytes()
                es[s] += enc.es(s)
                pts[s] += [t for t, k in zip(seconds, numbers) if k == s]
            cc = cc_out
        assert cc != [0, 0]
    want, _ = sim_encode(S44, xs)
    assert es == want
    with mp2.Mp2Batch(2, 1 << 16) as back:
        back.upload_ts([np.frombuffer(t, np.uint8) for t in ts], 0xC0)
        assert back.decode() == 9
        for s in range(2):
            assert back.read_bytes(s).tobytes() == es[s]
            writes = back.ts_writes(s)
            sizes = [mp2_encode.frame_bytes(n, 0, 10) for n in range(len(xs[s]))]
            assert [w[2] for w in writes] == sizes and [w[1] for w in writes] == [sum(sizes[:n]) for n in range(len(sizes))]
            assert [w[0] for w in writes] == pytest.approx([mp2_encode.default_pts(n, 44100) / 90000.0 for n in range(len(xs[s]))], abs=1e-9)
            assert pts[s] == [mp2_encode.default_pts(n, 44100) / 90000.0 for n in range(len(xs[s]))]
            assert same_bits(back.read_pcm(s), oracle_decode(libs, es[s])[0])


def test_refusals(torch, hip_lib):
    """what the host knows is refused at enqueue and the handle stays usable; a second call while one is in flight is REFUSED,
    as the video encoder does it; query never waits"""
    from jsmpeg_amd import mp2_encode
    for bad in ((0, 2, 1), (0, 2, 2), (1, 2, 3), (2, 2, 5), (0, 1, 11), (1, 1, 14), (3, 2, 10), (0, 3, 10), (0, 2, 15)):
        with pytest.raises(RuntimeError, match="Layer II"):
            mp2_encode.Mp2Encoder(*bad, 1, 1, 4096)
    xs = [inputs.pcm("noise", 44100, 3, seed=50), inputs.pcm("sine", 44100, 2, seed=51)]
    want, _ = sim_encode(S44, xs)
    keep, ptrs, frames = on_device(torch, xs)
    need = mp2_encode.es_bytes(frames, 0, 10)
    with mp2_encode.Mp2Encoder(*S44, 2, 5, need - 1) as enc:
        with pytest.raises(RuntimeError, match="max_es_bytes"):
            enc.encode(ptrs, frames, chain=True)
        assert enc.chain_info(0) == (False, 0)                    # nothing was enqueued, nothing moved
        enc.encode(ptrs[:1], frames[:1])
        assert enc.es(0) == want[0]
    with mp2_encode.Mp2Encoder(*S44, 4, 5, need) as enc:
        with pytest.raises(RuntimeError, match="ascend"):
            enc.encode(ptrs, frames, [2, 1])
        with pytest.raises(RuntimeError, match="ascend"):
            enc.encode(ptrs, frames, [1, 1])
        with pytest.raises(RuntimeError, match="max_streams"):
            enc.encode(ptrs, frames, [1, 4])
        with pytest.raises(RuntimeError, match="max_frames"):
            enc.encode([ptrs[0], ptrs[0]], [3, 3])
        with pytest.raises(RuntimeError, match="NULL"):
            enc.encode([0, ptrs[1]], frames)
        with pytest.raises(RuntimeError, match="nothing was encoded"):
            enc.device_es()
        enc.encode(ptrs, frames)
        assert enc.query() in (False, True)
        assert len(enc.frame_ranges()) == 5                       # closed form: answered while the pass may still run
        with pytest.raises(RuntimeError, match="in flight"):
            enc.encode(ptrs, frames)
        with pytest.raises(RuntimeError, match="in flight"):
            enc.chain_reset()
        enc.sync()
        assert enc.query() is True
        assert [enc.es(0), enc.es(1)] == want
        enc.encode([], [])                                        # a call without streams is a call
        assert enc.device_es()[1] == 0 and enc.count == 0


def test_live_tick_to_the_encoder(torch, hip_lib):
    """encode_live: the frames of an Mp2Live tick from their device_pcm pointers, the live stream id as the stream number of a
    chained call -- a stream that joins late begins at ordinal 0, the other goes on"""
    from jsmpeg_amd import mp2, mp2_encode, synth
    audio, offs = synth.generate_mp2_config("mp2_varying_44k", 6)
    bounds = [int(o) for o in offs] + [len(audio)]
    state = SimState(3)
    with mp2.Mp2Live(3, max_frames_per_tick=2) as live, mp2_encode.Mp2Encoder(*S44, 3, 6, 1 << 15) as enc:
        a, b = live.open(), live.open()
        for tick in range(3):
            live.write(a, tick * 0.05, audio[bounds[2 * tick]:bounds[2 * tick + 2]])
            if tick:
                live.write(b, tick * 0.05, audio[bounds[tick - 1]:bounds[tick]])
            assert live.tick() == (3 if tick else 2)
            pcm, frames = live.read_pcm(), live.frames()
            coded = enc.encode_live(live)
            ids = sorted({f["stream"] for f in frames})
            assert [f["stream"] for f in coded] == sorted(f["stream"] for f in frames) and ids == ([a, b] if tick else [a])
            want, _ = sim_encode(S44, [pcm[[i for i, f in enumerate(frames) if f["stream"] == s]] for s in ids], numbers=ids, chain=True, state=state)
            assert [enc.es(s) for s in ids] == want
        assert enc.chain_info(a) == (True, 6) and enc.chain_info(b) == (True, 2)
