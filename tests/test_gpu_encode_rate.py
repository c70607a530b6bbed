"""The encoder's rate control on the device (jsmpeg_hip_encoder_set_rate; jsmpeg_amd/encode.py Encoder.set_rate): the GPU's
bytes, ranges, kinds, reconstructions and chosen scales equal the CPU simulator's (sim_encode_rate of tests/sim/sim_encode_pass.cpp) and, on the
small inputs, the brute-force restatement's (tests/enc_rate_ref.py); one handle across calls with the rule changed in between;
the round trip through Batch on the device; tensor input; the pass as a pure enqueue; overflow and refusals.  Bytes and work
done are asserted, never times."""
import ctypes
import os

import numpy as np
import pytest

import enc_inputs as ei
import enc_p_inputs as ep
import enc_rate_inputs as er
import enc_rate_ref
from conftest import ROOT
from jsmpeg_amd import hashing

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


@pytest.fixture(scope="module")
def cases(libs):
    return er.rate_cases(libs)


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


def rates(enc, n):
    return [tuple(min(v, 0xffffffff) for v in (r["q"], r["budget"], r["bytes"])) for r in (enc.picture_rate(k) for k in range(n))]


def assert_equals(enc, streams, want, rate, where):
    """buffer, ranges, stream ranges, kinds, reconstructions and the choice of the encoder's last call against a result of the
    simulator or the restatement; rate: [(q, budget, bytes)]"""
    n = len(want.ranges)
    assert rates(enc, n) == [(q, min(b, 0xffffffff), s) for q, b, s in rate], where
    assert whole_buffer(enc) == want.buf, where
    assert enc.picture_ranges() == want.ranges, where
    assert {s: enc.stream_range(s) for s in sorted(set(streams))} == want.streams, where
    for k in range(n):
        assert enc.picture_rate(k)["bytes"] == enc.picture_ranges()[k][1], (where, k)
        assert tuple(enc.picture_stats(k)[name] for name in ep.KINDS) == want.stats[k], (where, k)
        assert np.array_equal(np.concatenate([p.ravel() for p in enc.recon(k)]), want.recon[k]), (where, k)


def run_case(torch, enc, c):
    t, ptrs = on_device(torch, c.frames)
    enc.set_gop(c.gop, c.search)
    enc.set_rate(c.T, c.q_min, c.q_max, c.W)
    enc.encode(ptrs, c.streams, 3)
    return t, ptrs


NAMES = ("pan_gop3_T150", "pan_gop4_T100", "pan_T20", "pan_T1500", "pan_gop1", "noise_T1500", "noise_T4000", "flat_grey", "flat_wide",
         "content_177x145", "content_177x145_R0", "one_macroblock", "range_4_16", "range_8_8", "streams_W1", "streams_W16")


@pytest.mark.parametrize("name", NAMES)
def test_cases_equal_the_simulator_and_the_restatement(torch, hip_lib, cases, name):
    from jsmpeg_amd import encode
    c = cases[name]
    n = len(c.frames)
    streams = c.streams or [0] * n
    with encode.Encoder(c.width, c.height, n, c.max_streams or 1, 64 + n * (len(c.frames[0]) * 4 + 4096)) as enc:
        keep = run_case(torch, enc, c)
        want = c.sim()
        assert_equals(enc, streams, want, want.rate, (name, "simulator"))
        if c.small:
            ref = enc_rate_ref.encode(c.frames, c.width, c.height, c.gop, c.search, streams=c.streams, **c.rule())
            assert_equals(enc, streams, ref, list(zip(ref.rate.q, ref.rate.budget, ref.rate.bytes)), (name, "restatement"))
        del keep


def test_a_range_of_one_scale_is_the_fixed_scale_call(torch, hip_lib, cases):
    from jsmpeg_amd import encode
    c = cases["range_8_8"]
    with encode.Encoder(c.width, c.height, len(c.frames), 1, 1 << 20) as enc:
        keep = run_case(torch, enc, c)
        assert whole_buffer(enc) == ep.sim_encode_p(c.frames, c.width, c.height, c.gop, c.search, qscale=8).buf
        del keep


def test_a_call_of_1100_pictures(torch, hip_lib):
    """the long call of the GOP tests over the range 6 .. 10: 158 GOPs, the picks of seven levels each reading the bytes the
    levels before left, five streams with gaps, the 256-picture steps of the placement; the simulator is the judge"""
    from jsmpeg_amd import encode
    long_call = ep.long_call()
    frames, w, h, streams, _ = long_call
    n = len(frames)
    want = er.sim_long(long_call)
    with encode.Encoder(w, h, n, ep.LONG_MAX_STREAMS, 64 + n * (len(frames[0]) * 4 + 4096)) as enc:
        t, ptrs = on_device(torch, frames)
        enc.set_gop(er.LONG_GOP, er.LONG_SEARCH)
        rule = er.LONG_RULE
        enc.set_rate(rule["T"], rule["q_min"], rule["q_max"], rule["W"])
        enc.encode(ptrs, streams, 31)
        assert_equals(enc, streams, want, want.rate, "long")


def test_one_handle_across_calls(torch, hip_lib, cases):
    """on, another range and GOP, off, on again at gop 1: nothing of the call before may stay"""
    from jsmpeg_amd import encode
    c = cases["pan_gop3_T150"]
    frames, w, h = c.frames, c.width, c.height
    with encode.Encoder(w, h, len(frames), 1, 1 << 18) as enc:
        t, ptrs = on_device(torch, frames)
        enc.set_gop(3, 7)
        enc.set_rate(150)
        enc.encode(ptrs, None, 8)
        want = c.sim()
        assert_equals(enc, [0], want, want.rate, "on")
        enc.set_gop(4, 3)
        enc.set_rate(100, 4, 16, 9)
        enc.encode(ptrs, None, 8)
        want = er.sim_encode_rate(frames, w, h, 4, 3, 100, 4, 16, 9)
        assert_equals(enc, [0], want, want.rate, "another range")
        enc.set_rate(0)
        enc.encode(ptrs, None, 8)
        assert whole_buffer(enc) == ep.sim_encode_p(frames, w, h, 4, 3, qscale=8).buf
        with pytest.raises(RuntimeError, match="rate control off"):
            enc.picture_rate(0)
        enc.set_gop(1, 0)
        enc.encode(ptrs, None, 8)
        assert (whole_buffer(enc), enc.picture_ranges(), {0: enc.stream_range(0)}) == ei.sim_encode(frames, w, h, qscale=8)
        with pytest.raises(RuntimeError, match="gop 1"):
            enc.recon_ptr(0)
        enc.set_rate(250)
        enc.encode(ptrs, None, 8)
        want = cases["pan_gop1"].sim()
        assert_equals(enc, [0], want, want.rate, "on again")


def test_round_trip_on_the_device(torch, hip_lib):
    """decode a golden fixture with Batch, encode its 13 pictures as two streams under rate control from the pool, attach the
    encoder's buffer to a second Batch as it is: its decode is the encoder's own reconstruction of every picture"""
    from jsmpeg_amd import batch as jb
    from jsmpeg_amd import encode
    es = np.fromfile(os.path.join(ROOT, "tests", "golden", "enc_pan_176x144.m1v"), dtype=np.uint8)
    streams = [0] * 7 + [1] * 6
    with jb.Batch(176, 144, 1, 16, 1 << 20) as src, jb.Batch(176, 144, 2, 16, 1 << 20) as dst, \
            encode.Encoder(176, 144, 16, 2, 1 << 20) as enc:
        src.upload([es])
        assert src.decode() == 13
        enc.set_gop(4, 7)
        enc.set_rate(encode.bytes_per_picture(360_000, enc.frame_rate_code))
        enc.encode_batch(src, list(range(13)), streams=streams, qscale=6)
        enc.sync()
        chosen = [enc.picture_rate(k)["q"] for k in range(13)]
        assert len(set(chosen)) > 1
        own = [int(hashing.frame_hash(*enc.recon(k))) for k in range(13)]
        ptr, total = enc.device_es()
        begin, end = zip(*(enc.stream_range(s) for s in (0, 1)))
        dst.attach_device(ptr, total, begin, end)
        assert dst.decode() == 13
        infos = dst.pictures()
        assert [i.stream for i in infos] == streams and all(i.decoded for i in infos)
        assert [int(v) for v in dst.frame_hashes()[:13]] == own


def test_tensor_input(torch, hip_lib):
    """encode_tensor under rate control: the bytes of the frames made from the same pictures"""
    from jsmpeg_amd import encode
    w, h = 177, 145
    base = (np.indices((h + 8, w + 8)).sum(0)[None] * np.array([1, 2, 3])[:, None, None]) % 256
    rgb = np.stack([base[:, k:k + h, 2 * k:2 * k + w] for k in range(4)]).astype(np.uint8)
    frames = list(ei.sim_rgb(rgb, 0, 0))
    want = er.sim_encode_rate(frames, w, h, 3, 7, 2500)
    assert len(set(r[0] for r in want.rate)) > 1
    with encode.Encoder(w, h, 4, 1, 1 << 21) as enc:
        enc.set_gop(3, 7)
        enc.set_rate(2500)
        enc.encode_tensor(torch.from_numpy(rgb).cuda(), qscale=5)
        assert_equals(enc, [0], want, want.rate, "tensor")
        t, ptrs = on_device(torch, frames)
        enc.encode(ptrs, None, 5)
        assert_equals(enc, [0], want, want.rate, "frames")


def test_pure_enqueue(torch, hip_lib):
    """with a rate-controlled pass in flight query is callable, a second encode, set_gop and set_rate are refused; sync
    returns 0 afterwards"""
    from jsmpeg_amd import encode
    hd = ei.content_frames(1920, 1080, 1) * 4
    with encode.Encoder(1920, 1080, 4, 1, 16 << 20) as enc:
        t, ptrs = on_device(torch, hd)
        enc.set_gop(4, 7)
        enc.set_rate(60000)
        torch.cuda.synchronize()
        enc.encode(ptrs, None, 4)
        assert enc.query() in (False, True)
        with pytest.raises(RuntimeError, match="in flight"):
            enc.encode(ptrs, None, 4)
        with pytest.raises(RuntimeError, match="in flight"):
            enc.set_gop(2, 0)
        with pytest.raises(RuntimeError, match="in flight"):
            enc.set_rate(0)
        enc.sync()
        assert enc.query() is True
        assert enc.L.jsmpeg_hip_encoder_sync(enc.h) == 0
        mbs = 120 * 68
        assert enc.picture_stats(0)["intra"] == mbs
        assert all(enc.picture_stats(k)["intra"] == 0 and sum(enc.picture_stats(k).values()) == mbs for k in range(1, 4))
        for k in range(4):
            r = enc.picture_rate(k)
            assert r["bytes"] == enc.picture_ranges()[k][1] and (r["bytes"] <= r["budget"] or r["q"] == 31)


def test_overflow(torch, hip_lib, cases):
    """a max_es_bytes too small for the call: sync fails with the message, the readers refuse, the next call works"""
    from jsmpeg_amd import encode
    c = cases["noise_T4000"]
    want = c.sim()
    need = len(want.buf)
    with encode.Encoder(c.width, c.height, 4, 1, need - 16) as enc:
        keep = run_case(torch, enc, c)
        with pytest.raises(RuntimeError, match="max_es_bytes"):
            enc.sync()
        for reader in (lambda: enc.es(0), enc.device_es, lambda: enc.recon_ptr(0), lambda: enc.picture_stats(0), lambda: enc.picture_rate(0)):
            with pytest.raises(RuntimeError, match="overflowed"):
                reader()
        enc.set_rate(1500)
        enc.encode(keep[1], None, 1)
        small = cases["noise_T1500"].sim()
        assert_equals(enc, [0], small, small.rate, "after")
        del keep
    with encode.Encoder(c.width, c.height, 4, 1, need) as enc:
        keep = run_case(torch, enc, c)
        assert_equals(enc, [0], want, want.rate, "fits")
        del keep


def test_refusals(torch, hip_lib):
    from jsmpeg_amd import encode
    with encode.Encoder(64, 48, 2, 1, 1 << 16) as enc:
        for args, why in (((100, 0, 31, 4), "q_min 0"), ((100, 1, 32, 4), "q_max 32"), ((100, 9, 8, 4), "q_min 9, q_max 8"),
                          ((100, 1, 31, 0), "i_weight 0"), ((100, 1, 31, 256), "i_weight 256"), ((0, 0, 31, 4), "q_min 0")):
            with pytest.raises(RuntimeError, match=why):
                enc.set_rate(*args)
        with pytest.raises(RuntimeError, match="nothing was encoded"):
            enc.picture_rate(0)
        t, ptrs = on_device(torch, [ei.flat_frame(64, 48, 1)] * 2)
        enc.encode(ptrs, None, 3)
        with pytest.raises(RuntimeError, match="rate control off"):
            enc.picture_rate(0)
        before = (whole_buffer(enc), enc.picture_ranges())
        with pytest.raises(RuntimeError):
            enc.set_rate(100, 5, 4, 4)
        enc.encode(ptrs, None, 3)
        assert (whole_buffer(enc), enc.picture_ranges()) == before              # a refused set_rate changed nothing: still off
        enc.set_rate(100)
        for bad in (0, 32):                                                     # the scales are checked as before, and unused
            with pytest.raises(RuntimeError, match="quantiser_scale"):
                enc.encode(ptrs, None, bad)
        enc.encode(ptrs, None, 3)
        a = (whole_buffer(enc), rates(enc, 2))
        enc.encode(ptrs, None, 29)
        assert (whole_buffer(enc), rates(enc, 2)) == a
        with pytest.raises(RuntimeError, match="picture 2 of 2"):
            enc.picture_rate(2)
        assert enc.L.jsmpeg_hip_encoder_set_rate(None, 100, 1, 31, 4) < 0
        assert enc.L.jsmpeg_hip_encoder_picture_rate(None, 0, None) < 0


def test_exports(hip_lib):
    from jsmpeg_amd import encode
    L = encode.lib()
    for name in ("jsmpeg_hip_encoder_set_rate", "jsmpeg_hip_encoder_picture_rate"):
        assert name in encode.SYMBOLS and getattr(L, name)
