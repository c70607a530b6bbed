"""The encoder's chains across calls on the device (JSMPEG_HIP_ENC_CHAIN; Encoder.encode(chain=True)): every call's buffer,
ranges, kinds and reconstructions equal the chain simulator's call (sim_chain_* of tests/sim/sim_encode_pass.cpp, which tests/test_enc_chain_sim.py
ties to the one-call simulators and the oracle), and every stream's pieces, concatenated, equal ONE unchained call over the same
pictures on the same handle.  Bytes are asserted, never times."""
import ctypes
import os

import numpy as np
import pytest

import enc_chain_inputs as ec
import enc_inputs as ei
import enc_p_inputs as ep
import enc_ref
from conftest import ROOT
from jsmpeg_amd import hashing

pytestmark = pytest.mark.gpu

PAN = ep.pan_frames(64, 48, 7, (3, -2))


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


@pytest.fixture(scope="module")
def cases(libs):
    return ep.p_cases(libs)


def on_device(torch, frames):
    t = torch.from_numpy(np.ascontiguousarray(np.stack(frames))).cuda()
    return t, [t.data_ptr() + k * t.shape[1] for k in range(t.shape[0])]


def whole_buffer(enc):
    """the call's device buffer on the host, its 256-byte tail checked"""
    from jsmpeg_amd import batch
    p, total = enc.device_es()
    out = np.zeros(total + 256, dtype=np.uint8)
    L = batch.lib()
    L.jsmpeg_hip_device_read.restype = ctypes.c_int
    L.jsmpeg_hip_device_read.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64]
    assert L.jsmpeg_hip_device_read(out.ctypes.data, p, total + 256) == 0
    assert np.all(out[total:] == 0xff)
    return out[:total].tobytes()


def recon_bytes(enc, k):
    return np.concatenate([p.ravel() for p in enc.recon(k)])


def result_of(enc, streams, n, rate=False):
    """the encoder's last call as the simulators report theirs"""
    present = sorted(set(streams)) if streams is not None else [0]
    r = ep.Result(whole_buffer(enc), enc.picture_ranges(), {s: enc.stream_range(s) for s in present}, [recon_bytes(enc, k) for k in range(n)], None,
                  [tuple(enc.picture_stats(k)[name] for name in ep.KINDS) for k in range(n)])
    r.rate = [tuple(enc.picture_rate(k)[name] for name in ("q", "budget", "bytes")) for k in range(n)] if rate else None
    return r


def assert_equals(got, want, where):
    assert got.buf == want.buf, where
    assert got.ranges == want.ranges, where
    assert got.streams == want.streams, where
    assert got.stats == want.stats, where
    for k in range(len(want.ranges)):
        assert np.array_equal(got.recon[k], want.recon[k]), (where, k)
    if getattr(want, "rate", None) is not None:
        assert got.rate == [(q, min(b, 0xffffffff), s) for q, b, s in want.rate], where


class Device:
    """an Encoder with ec.Chain's encode: the frames go up, the call runs, its result comes back"""

    def __init__(self, torch, enc, rate=False):
        self.torch, self.enc, self.rate = torch, enc, rate

    def encode(self, frames, streams=None, qscale=8, end=False, chain=True):
        self.keep, ptrs = on_device(self.torch, frames)
        self.enc.encode(ptrs, streams, qscale, end=end, chain=chain)
        return result_of(self.enc, streams, len(frames), self.rate)


def both(dev, sim, frames, streams, led, where, end=False, qscale=8):
    """the same chained call on the device and in the simulator: equal, and into the ledger"""
    got, want = dev.encode(frames, streams, qscale, end=end), sim.encode(frames, streams, qscale, end=end)
    assert_equals(got, want, where)
    led.add(frames, streams, got, end)
    return got


def capacity(frames):
    return 64 + len(frames) * (len(frames[0]) * 4 + 4096)


def test_every_split_of_the_pan(torch, hip_lib):
    from jsmpeg_amd import encode
    with encode.Encoder(64, 48, 7, 1, capacity(PAN)) as enc, ec.Chain(64, 48) as sim:
        dev = Device(torch, enc)
        enc.set_gop(3, 7)
        sim.set_gop(3, 7)
        one = dev.encode(PAN, None, 8, end=True, chain=False)
        assert_equals(one, ep.sim_encode_p(PAN, 64, 48, 3, 7, qscale=8), "one call")
        for cuts in ec.splits(7):
            led, at = ec.Ledger(), 0
            for i, n in enumerate(cuts):
                both(dev, sim, PAN[at:at + n], None, led, (cuts, i), end=i + 1 == len(cuts))
                at += n
            (seg,) = led.segments[0]
            ec.assert_segment(seg, one, cuts)
            assert enc.chain_info(0) == (False, 0)


def test_one_picture_per_call(torch, hip_lib):
    """five calls of one picture -- each reads one carry frame and writes the other, the parity returns twice -- then a call of two"""
    from jsmpeg_amd import encode
    with encode.Encoder(64, 48, 7, 1, capacity(PAN)) as enc, ec.Chain(64, 48) as sim:
        dev = Device(torch, enc)
        enc.set_gop(3, 7)
        sim.set_gop(3, 7)
        led, seen = ec.Ledger(), set()
        for k in range(5):
            both(dev, sim, PAN[k:k + 1], None, led, k)
            assert enc.chain_info(0) == (True, k + 1)
            seen.add(enc.recon_ptr(0))
        assert len(seen) == 2                                  # the stream's two carry frames, in turns
        both(dev, sim, PAN[5:7], None, led, "two", end=True)
        one = dev.encode(PAN, None, 8, end=True, chain=False)
        ec.assert_segment(led.segments[0][0], one, "one per call")
        assert ep.picture_types(one.stream(0)) == ep.expected_types(7, 3)


@pytest.mark.parametrize("name", ["flat_wide", "content_177x145"])
def test_two_calls(torch, hip_lib, cases, name):
    from jsmpeg_amd import encode
    frames, w, h = cases[name]
    with encode.Encoder(w, h, len(frames), 1, capacity(frames)) as enc, ec.Chain(w, h) as sim:
        dev = Device(torch, enc)
        enc.set_gop(3, 7)
        sim.set_gop(3, 7)
        led = ec.Ledger()
        both(dev, sim, frames[:1], None, led, 0)
        both(dev, sim, frames[1:], None, led, 1, end=True)
        ec.assert_segment(led.segments[0][0], dev.encode(frames, None, 8, end=True, chain=False), name)


def test_two_streams_one_reset(torch, hip_lib):
    """stream numbers 1 and 4, a picture each per call; 4 is reset before the third call"""
    from jsmpeg_amd import encode
    pan9 = ep.pan_frames(64, 48, 9, (2, 1))
    own = {1: PAN[:4], 4: pan9[:4]}
    with encode.Encoder(64, 48, 4, 5, capacity(PAN)) as enc, ec.Chain(64, 48, 5) as sim:
        dev = Device(torch, enc)
        enc.set_gop(3, 7)
        sim.set_gop(3, 7)
        led = ec.Ledger()
        for i in range(4):
            if i == 2:
                for h in (enc, sim):
                    h.chain_reset(4)
                led.cut(4)
                assert enc.chain_info(4) == (False, 0) and enc.chain_info(1) == (True, 2)
            both(dev, sim, [own[1][i], own[4][i]], [1, 4], led, i)
        assert enc.chain_info(1) == (True, 4) and enc.chain_info(4) == (True, 2) and enc.chain_info(0) == (False, 0)
        assert [len(s.frames) for s in led.segments[1]] == [4] and [len(s.frames) for s in led.segments[4]] == [2, 2]
        for s, segs in led.segments.items():
            for i, seg in enumerate(segs):
                one = dev.encode(seg.frames, None, 8, end=False, chain=False)
                ec.assert_segment(seg, one, (s, i))


@pytest.mark.parametrize("cuts", [[1, 2, 3], [4, 2]], ids=lambda c: "-".join(map(str, c)))
def test_rate_control(torch, hip_lib, cuts):
    """six pictures of the pan at gop 3, T 150: whole GOPs, so the chained calls choose what the one call chooses"""
    from jsmpeg_amd import encode
    frames = PAN[:6]
    with encode.Encoder(64, 48, 6, 1, capacity(frames)) as enc, ec.Chain(64, 48) as sim:
        dev = Device(torch, enc, rate=True)
        for h in (enc, sim):
            h.set_gop(3, 7)
            h.set_rate(150, 1, 31, 4)
        led, at = ec.Ledger(), 0
        for i, n in enumerate(cuts):
            both(dev, sim, frames[at:at + n], None, led, (cuts, i), end=i + 1 == len(cuts))
            at += n
        one = dev.encode(frames, None, 8, end=True, chain=False)
        (seg,) = led.segments[0]
        ec.assert_segment(seg, one, cuts)
        assert seg.rate == one.rate and [r[2] for r in seg.rate] == [b for _, b in one.ranges]
        assert len({q for q, _, _ in one.rate}) > 1


def test_tensor_input(torch, hip_lib):
    from jsmpeg_amd import encode
    w, h = 64, 48
    rgb = np.random.default_rng(3).integers(0, 256, (4, h, w, 3), dtype=np.uint8)
    rgb[1:] = np.roll(rgb[0], 2, axis=1)
    frames = [enc_ref.rgb_to_frame(rgb[k]) for k in range(4)]
    with encode.Encoder(w, h, 4, 1, capacity(frames)) as enc:
        enc.set_gop(3, 7)
        t, ptrs = on_device(torch, frames)
        enc.encode(ptrs, None, 6)
        want, recon = enc.es(0), [recon_bytes(enc, k) for k in range(4)]
        x = torch.from_numpy(np.ascontiguousarray(rgb)).cuda()
        pieces = []
        for a, b in ((0, 1), (1, 4)):
            enc.encode_tensor(x[a:b].contiguous(), qscale=6, end=b == 4, chain=True)
            pieces.append(enc.es(0))
            for k in range(a, b):
                assert np.array_equal(recon_bytes(enc, k - a), recon[k]), k
        assert b"".join(pieces) == want


def test_overflow_resets_the_streams_of_the_call(torch, hip_lib):
    from jsmpeg_amd import encode
    flat, noise = ei.flat_frame(64, 48, 9), ei.noise_frame(64, 48, 1)
    with ec.Chain(64, 48, 2) as sim:
        sim.set_gop(3, 7)
        sim.encode([flat, flat], [0, 1], 1)
        need = len(sim.encode([noise], [0], 1).buf)            # what the call that is to overflow needs: its one-call size
    with encode.Encoder(64, 48, 2, 2, need - 1) as enc:
        dev = Device(torch, enc)
        enc.set_gop(3, 7)
        dev.encode([flat, flat], [0, 1], 1)
        assert enc.chain_info(0) == (True, 1) and enc.chain_info(1) == (True, 1)
        t, ptrs = on_device(torch, [noise])
        enc.encode(ptrs, [0], 1, end=False, chain=True)
        with pytest.raises(RuntimeError, match="max_es_bytes"):
            enc.sync()
        with pytest.raises(RuntimeError, match="overflowed"):
            enc.es(0)
        assert enc.chain_info(0) == (False, 0) and enc.chain_info(1) == (True, 1)
        got = dev.encode([flat], [0], 1)
        assert ep.picture_types(got.stream(0)) == [1]
        fresh = dev.encode([flat], [0], 1, end=False, chain=False)
        assert got.buf == fresh.buf and got.ranges == fresh.ranges and np.array_equal(got.recon[0], fresh.recon[0])
        assert enc.chain_info(0) == (True, 1)


def test_relay_round_trip(torch, hip_lib):
    """two live streams in, a picture per stream and tick through encode_live(chain=True), every stream's piece into a second
    Live: what that one decodes is the encoder's reconstruction, bit for bit"""
    from jsmpeg_amd import encode
    from jsmpeg_amd import live as jl
    es = np.fromfile(os.path.join(ROOT, "tests", "golden", "enc_pan_176x144.m1v"), dtype=np.uint8)
    offs = [int(v) for v in np.load(os.path.join(ROOT, "tests", "golden", "enc_pan_176x144.offsets.npy"))]
    ticks = 5
    with jl.Live(176, 144, 2, pictures_per_tick=2, store_bytes=1 << 18) as src, jl.Live(176, 144, 2, pictures_per_tick=2, store_bytes=1 << 18) as dst, \
            encode.Encoder(176, 144, 2, 2, 1 << 20) as enc:
        enc.set_gop(4, 7)
        ids, out, types, coded = [src.open()], [dst.open()], {0: [], 1: []}, 0
        for t in range(ticks):
            if t == 1:                                         # a second stream joins: the first keeps its number and its chain
                ids.append(src.open())
                out.append(dst.open())
            for j, i in enumerate(ids):
                src.write(i, es[offs[t - j]:offs[t - j + 1]], pts=t / 30.0)
            assert src.tick(flush=True) == len(ids)
            used = enc.encode_live(src, qscale=6, end=False, chain=True)
            order = [p.stream for p in used]
            assert order == sorted(ids)
            for p in used:
                dst.write(out[ids.index(p.stream)], np.frombuffer(enc.es(p.stream), dtype=np.uint8), pts=t / 30.0)
            assert dst.tick(flush=True) == len(ids)
            hs = dst.frame_hashes()
            for q, pic in enumerate(dst.pictures()):
                j = out.index(pic.stream)
                assert int(hs[q]) == hashing.frame_hash(*enc.recon(order.index(ids[j]))), (t, j)
                types[j].append(pic.type)
                coded += 1
        assert types == {0: [1, 2, 2, 2, 1], 1: [1, 2, 2, 2]} and coded == 9
        assert enc.chain_info(ids[0]) == (True, ticks) and enc.chain_info(ids[1]) == (True, ticks - 1)


def test_refusals(torch, hip_lib):
    from jsmpeg_amd import encode
    from jsmpeg_amd import live as jl
    with encode.Encoder(64, 48, 2, 2, 1 << 16) as enc:
        enc.set_gop(3, 7)
        t, ptrs = on_device(torch, PAN[:2])
        enc.encode(ptrs[:1], None, 8, end=False, chain=True)
        with pytest.raises(RuntimeError, match="in flight"):
            enc.chain_reset(0)
        enc.sync()
        enc.chain_reset(0)
        for call in (lambda: enc.chain_reset(2), lambda: enc.chain_info(2)):
            with pytest.raises(RuntimeError, match="max_streams"):
                call()
        s = np.zeros(1, np.uint32)
        arr = (ctypes.c_void_p * 1)(ptrs[0])
        assert enc.L.jsmpeg_hip_encoder_encode(enc.h, arr, s.ctypes.data, None, 1, 8, 4, None) < 0
        from jsmpeg_amd import batch
        assert "unknown flags 0x4" in batch.last_error()
        assert enc.L.jsmpeg_hip_encoder_encode(enc.h, arr, s.ctypes.data, None, 1, 8, 3, None) == 0     # END | CHAIN
        enc.sync()
        assert enc.chain_info(0) == (False, 0)
    es = np.fromfile(os.path.join(ROOT, "tests", "golden", "enc_pan_176x144.m1v"), dtype=np.uint8)
    offs = np.load(os.path.join(ROOT, "tests", "golden", "enc_pan_176x144.offsets.npy"))
    with jl.Live(176, 144, 2, pictures_per_tick=1, store_bytes=1 << 18) as lv, encode.Encoder(176, 144, 2, 1, 1 << 20) as enc:
        enc.set_gop(3, 7)
        ids = [lv.open(), lv.open()]
        for i in ids:
            lv.write(i, es[int(offs[0]):int(offs[1])], pts=0.0)
        assert lv.tick(flush=True) == 2
        with pytest.raises(ValueError, match="max_streams"):
            enc.encode_live(lv, chain=True)                    # live stream id 1 on a handle of one stream
        enc.encode_live(lv, pictures=[k for k, p in enumerate(lv.pictures()) if p.stream == 0], end=False, chain=True)
        assert enc.chain_info(0) == (True, 1)
        enc.encode_live(lv, pictures=[k for k, p in enumerate(lv.pictures()) if p.stream == 0], chain=True)     # end=True, the default, closes the stream
        assert enc.chain_info(0) == (False, 0)
