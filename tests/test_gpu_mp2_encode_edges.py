"""The MP2 encoder on the device at EVERY setting the rule accepts and at the edges of its arithmetic, against the simulator of
the same rule (tests/sim/sim_mp2_enc.cpp): bytes and statistics are asserted, exactly.  The inputs are those of
tests/mp2_enc_inputs.py (edge_inputs, the padding period); what they reach -- every pair winning an allocation round, ties,
both ends of the loop, the analysis at its bounds, the conversion's ties, every store alignment -- is asserted without a GPU in
tests/test_mp2_enc_edges.py.  The decoder kernels (Mp2Batch) get the encoder's streams at all 60 settings.  Needs an MI355X."""
import ctypes

import numpy as np
import pytest

import mp2_enc_inputs as inputs
from mp2_enc_util import oracle_decode, sim_encode
from mp2_util import same_bits
from test_gpu_mp2_encode import check_layout, on_device

pytestmark = pytest.mark.gpu

SETTINGS = inputs.ALL_SETTINGS
KINDS = inputs.EDGE_KINDS
CANARY = 0xA5
BEHIND = 256          # bytes of the ES buffer behind the call's total that must stay as they were


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


def _device_lib():
    from jsmpeg_amd import batch
    L = batch.lib()
    L.jsmpeg_hip_device_read.restype = ctypes.c_int
    L.jsmpeg_hip_device_read.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64]
    L.jsmpeg_hip_device_fill.restype = ctypes.c_int
    L.jsmpeg_hip_device_fill.argtypes = [ctypes.c_void_p, ctypes.c_int32, ctypes.c_uint64]
    return L


def fill_es(enc, cap):
    """the whole ES buffer (cap = the handle's max_es_bytes) to the canary; the handle has settled a call, possibly an empty one"""
    p, _ = enc.device_es()
    assert _device_lib().jsmpeg_hip_device_fill(p, CANARY, cap) == 0


def check_canary(enc, cap, numbers, pieces):
    """the ES buffer after a call into a canary-filled buffer: the streams' bytes, zeros up to the next multiple of 16 behind
    each, and the canary everywhere behind the call's total"""
    p, total = enc.device_es()
    out = np.zeros(cap, np.uint8)
    assert _device_lib().jsmpeg_hip_device_read(out.ctypes.data, p, cap) == 0
    at = 0
    for s, want in zip(numbers, pieces):
        b, e = enc.stream_range(s)
        assert (b, e) == (at, at + len(want)) and out[b:e].tobytes() == want, s
        at = (e + 15) & ~15
        assert not out[e:at].any(), s
    assert at == total and total + BEHIND <= cap and (out[total:] == CANARY).all()


@pytest.mark.parametrize("cfg", SETTINGS, ids=[inputs.setting_id(c) for c in SETTINGS])
def test_gpu_equals_the_simulator_at_every_setting(cfg, torch, hip_lib, libs):
    """one handle, one call with a stream per edge input: bytes, layout and statistics are the simulator's; the same buffer
    handed to Mp2Batch on the device decodes bit-equal to the oracle"""
    from jsmpeg_amd import mp2, mp2_encode
    named = inputs.edge_inputs(inputs.RATES[cfg[0]])
    xs = [named[k] for k in KINDS]
    want, stats = sim_encode(cfg, xs)
    keep, ptrs, frames = on_device(torch, xs)
    need = mp2_encode.es_bytes(frames, cfg[0], cfg[2])
    with mp2_encode.Mp2Encoder(cfg[0], cfg[1], cfg[2], len(xs), sum(frames), need) as enc, mp2.Mp2Batch(len(xs), need + 64) as back:
        enc.encode(ptrs, frames)
        for s, kind in enumerate(KINDS):
            assert enc.es(s) == want[s], kind
        check_layout(enc, range(len(xs)), want)
        for k in range(sum(frames)):
            st = enc.frame_stats(k)
            assert [st["coded_pairs"], st["bits_used"], st["bits_left"], st["top_code"]] == [int(v) for v in stats[k]], k
        p, total = enc.device_es()
        ranges = [enc.stream_range(s) for s in range(len(xs))]
        back.upload_device(p, total, [r[0] for r in ranges], [r[1] for r in ranges])
        assert back.decode() == sum(frames)
        for s, kind in enumerate(KINDS):
            pcm, sizes = oracle_decode(libs, want[s])
            assert len(pcm) == frames[s] and same_bits(back.read_pcm(s), pcm), kind


@pytest.mark.parametrize("cfg", inputs.PERIOD_SETTINGS, ids=[inputs.setting_id(c) for c in inputs.PERIOD_SETTINGS])
def test_padding_period_and_every_store_alignment(cfg, torch, hip_lib):
    """a stream of 50 frames at 44.1 kHz (one past the padding period) and streams whose ends leave every tail 0..15, in one call
    and cut into chained calls of 1, 7, 41 and 1 frames, each into a buffer filled with a canary: the simulator's bytes, zeros
    between the streams, the canary behind the total"""
    from jsmpeg_amd import mp2_encode
    counts, xs = inputs.period_counts(cfg), inputs.period_streams(cfg)
    numbers = list(range(len(xs)))
    whole, stats = sim_encode(cfg, xs)
    cap = mp2_encode.es_bytes(counts, cfg[0], cfg[2]) + BEHIND
    with mp2_encode.Mp2Encoder(cfg[0], cfg[1], cfg[2], len(xs), sum(counts), cap) as enc:
        enc.encode([], [])                                        # a call without streams: the buffer's address
        assert enc.device_es()[1] == 0
        fill_es(enc, cap)
        keep, ptrs, frames = on_device(torch, xs)
        enc.encode(ptrs, frames)
        check_canary(enc, cap, numbers, whole)
        check_layout(enc, numbers, whole)
        for k in (0, 48, 49, sum(counts) - 1):
            st = enc.frame_stats(k)
            assert [st["coded_pairs"], st["bits_used"], st["bits_left"], st["top_code"]] == [int(v) for v in stats[k]], k
        done, pieces = [0] * len(xs), [b""] * len(xs)
        for call in inputs.chain_calls(counts):
            fill_es(enc, cap)
            keep, ptrs, frames = on_device(torch, [x[d:d + n] for x, d, n in zip(xs, done, call)])
            enc.encode(ptrs, frames, chain=True)
            got = [enc.es(s) for s in numbers]
            check_canary(enc, cap, numbers, got)
            pieces = [p + g for p, g in zip(pieces, got)]
            done = [d + n for d, n in zip(done, call)]
            assert [enc.chain_info(s) for s in numbers] == [(True, d) for d in done]
        assert pieces == whole
        fill_es(enc, cap)                                         # unchained again behind the chain: the same bytes, nothing else touched
        keep, ptrs, frames = on_device(torch, xs)
        enc.encode(ptrs, frames)
        check_canary(enc, cap, numbers, whole)


def test_mono_reads_channel_zero_only(torch, hip_lib):
    """a mono handle: bounds() and conversion() in the RIGHT channel with the left silent give the bytes of silence; in the left
    channel, with NaN, infinities and full scale in the right, the bytes of the same left channel over a right channel of zeros"""
    from jsmpeg_amd import mp2_encode
    cfg = (1, 1, 10)                                              # mono 48 kHz 192 kbit/s
    xs, zeroed = [], []
    for x in (inputs.bounds(), inputs.conversion(48000)):
        right_only = np.zeros_like(x)
        right_only[:, 1, :] = x[:, 0, :]
        left = x.copy()
        left[:, 1, :] = x[::-1, 1, ::-1]
        left[:, 1, ::7] = np.float32(np.nan)
        left[:, 1, 3::7] = np.float32(np.inf)
        left[:, 1, 5::7] = np.float32(-1.0)
        clean = x.copy()
        clean[:, 1, :] = 0
        xs += [right_only, left]
        zeroed += [np.zeros_like(x), clean]
    want, stats = sim_encode(cfg, zeroed)
    assert want == sim_encode(cfg, xs)[0] and want[1] != want[0]
    keep, ptrs, frames = on_device(torch, xs)
    with mp2_encode.Mp2Encoder(*cfg, len(xs), sum(frames), mp2_encode.es_bytes(frames, cfg[0], cfg[2])) as enc:
        enc.encode(ptrs, frames)
        assert [enc.es(s) for s in range(len(xs))] == want
        check_layout(enc, range(len(xs)), want)
        assert [enc.frame_stats(k)["coded_pairs"] for k in range(frames[0])] == [0] * frames[0]
