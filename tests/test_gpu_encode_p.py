"""The encoder's GOP pass on the device (jsmpeg_hip_encoder_set_gop; jsmpeg_amd/encode.py Encoder.set_gop): the GPU's bytes,
ranges, kinds and reconstructions equal the CPU simulator's (sim_encode_p of tests/sim/sim_encode_pass.cpp) and the independent restatement's
(tests/enc_p_ref.py); the round trip through Batch on the device; tensor input; the pass as a pure enqueue; overflow and
refusals.  Bytes and work done are asserted, never times."""
import ctypes
import os

import numpy as np
import pytest

import enc_inputs as ei
import enc_p_inputs as ep
import enc_p_ref
import enc_ref
from conftest import ROOT
from jsmpeg_amd import cabi, hashing

pytestmark = pytest.mark.gpu


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


def assert_equals(enc, streams, want, where):
    """buffer, ranges, stream ranges, kinds and reconstructions of the encoder's last call against a simulator / restatement result"""
    assert whole_buffer(enc) == want.buf, where
    assert enc.picture_ranges() == want.ranges, where
    assert {s: enc.stream_range(s) for s in sorted(set(streams))} == want.streams, where
    for k in range(len(want.ranges)):
        assert tuple(enc.picture_stats(k)[n] for n in ep.KINDS) == want.stats[k], (where, k)
        assert np.array_equal(recon_bytes(enc, k), want.recon[k]), (where, k)


@pytest.mark.parametrize("gop,R", ep.GOPS)
@pytest.mark.parametrize("q", ep.SCALES)
def test_small_inputs_equal_the_simulator_and_the_restatement(torch, hip_lib, cases, q, gop, R):
    from jsmpeg_amd import encode
    for name, (frames, w, h) in cases.items():
        n = len(frames)
        with encode.Encoder(w, h, n, 1, 64 + n * (len(frames[0]) * 4 + 4096)) as enc:
            t, ptrs = on_device(torch, frames)
            enc.set_gop(gop, R)
            enc.encode(ptrs, None, q)
            assert_equals(enc, [0], ep.sim_encode_p(frames, w, h, gop, R, qscale=q), (name, "simulator"))
            assert_equals(enc, [0], enc_p_ref.encode(frames, w, h, gop, R, qscale=q), (name, "restatement"))


@pytest.fixture(scope="module")
def ranged(libs, cases):
    return ep.range_cases(libs, cases)


@pytest.fixture(scope="module")
def range_encoders(torch, hip_lib, ranged):
    """one Encoder per picture size, kept from radius to radius, and every case's frames on the device"""
    from jsmpeg_amd import encode
    encs, dev = {}, {}
    for name, (frames, w, h) in ranged.items():
        if (w, h) not in encs:
            encs[(w, h)] = encode.Encoder(w, h, 4, 1, 64 + 4 * (len(frames[0]) * 4 + 4096))
        dev[name] = on_device(torch, frames)
    yield encs, dev
    for enc in encs.values():
        enc.close()


@pytest.mark.parametrize("R", ep.RADII)
def test_every_search_range_equals_the_simulator(ranged, range_encoders, R):
    """k_enc_motion at every radius -- its staged rows, its passes over the items and the partial last one, the group
    alignment, the half-pel step at the window's edge -- against the simulator, which tests/test_enc_p_sim.py ties to the
    restatement and the oracle on these inputs.  The handles live across the radii (set_gop between calls: nothing of the
    radius before may stay).  `intra_threshold` (the decision at equality) and `checker_ties` (the order among equal SADs)
    are among the cases, so the device's decision and reduction are held to those edges here too"""
    encs, dev = range_encoders
    for q in (1, 8):
        for name, (frames, w, h) in ranged.items():
            enc = encs[(w, h)]
            enc.set_gop(4, R)
            enc.encode(dev[name][1], None, q)
            assert_equals(enc, [0], ep.sim_encode_p(frames, w, h, 4, R, qscale=q), (name, q, R))


@pytest.fixture(scope="module")
def long_call():
    return ep.long_call()


@pytest.fixture(scope="module")
def long_encoder(torch, hip_lib, long_call):
    from jsmpeg_amd import encode
    frames, w, h, streams, qs = long_call
    n = len(frames)
    with encode.Encoder(w, h, n, ep.LONG_MAX_STREAMS, 64 + n * (len(frames[0]) * 4 + 4096)) as enc:
        yield enc, on_device(torch, frames)


_long = {}


def long_want(long_call, gop, R):
    if (gop, R) not in _long:
        frames, w, h, streams, qs = long_call
        _long[(gop, R)] = ep.sim_encode_p(frames, w, h, gop, R, streams=streams, qscale=qs, max_streams=ep.LONG_MAX_STREAMS)
    return _long[(gop, R)]


@pytest.mark.parametrize("gop,R", ep.LONG_GOPS)
def test_a_call_of_1100_pictures(long_call, long_encoder, gop, R):
    """k_enc_place's second to fifth step of 256 pictures with the state it carries across them, 18 blocks of the picture scan,
    up to 1024 levels, stream numbers with gaps -- and the same call once more behind a short one on the same handle"""
    frames, w, h, streams, qs = long_call
    enc, (t, ptrs) = long_encoder
    want = long_want(long_call, gop, R)
    absent = [s for s in range(ep.LONG_MAX_STREAMS) if s not in streams]
    enc.set_gop(gop, R)
    enc.encode(ptrs, streams, qs)
    assert_equals(enc, streams, want, "first")
    assert [enc.stream_range(s) for s in absent] == [(0, 0)] * len(absent)
    a, b = 556, 561                                         # two pictures of stream 4, three of stream 7
    enc.encode(ptrs[a:b], streams[a:b], qs[a:b], end=False)
    assert_equals(enc, streams[a:b], ep.sim_encode_p(frames[a:b], w, h, gop, R, streams=streams[a:b], qscale=qs[a:b], end=False,
                                                      max_streams=ep.LONG_MAX_STREAMS), "short")
    enc.encode(ptrs, streams, qs)
    assert_equals(enc, streams, want, "again")
    assert [enc.stream_range(s) for s in absent] == [(0, 0)] * len(absent)


def test_round_trip_of_the_long_call(long_call, long_encoder):
    """the 1100 pictures at gop 300, R 15, through Batch from the encoder's buffer -- the present streams' ranges, in order --
    by decode() and by enqueue(): the encoder's own reconstructions, picture types and levels by ordinal"""
    from jsmpeg_amd import batch as jb
    frames, w, h, streams, qs = long_call
    enc, (t, ptrs) = long_encoder
    gop, n = 300, len(frames)
    enc.set_gop(gop, 15)
    enc.encode(ptrs, streams, qs)
    enc.sync()
    own = [int(hashing.frame_hash(*enc.recon(k))) for k in range(n)]
    present = sorted(set(streams))
    begin, end = zip(*(enc.stream_range(s) for s in present))
    ptr, total = enc.device_es()
    ordinal = ep.ordinals(streams)
    with jb.Batch(w, h, len(present), n + 4, total + 4096) as dst:
        for how in ("decode", "enqueue"):
            dst.attach_device(ptr, total, begin, end)
            if how == "decode":
                assert dst.decode() == n
            else:
                assert dst.enqueue() == 0
                dst.sync()
            infos = dst.pictures()
            assert len(infos) == n and all(i.decoded for i in infos), how
            assert [i.stream for i in infos] == [present.index(s) for s in streams], how
            assert [int(v) for v in dst.frame_hashes()[:n]] == own, how
            assert [i.type for i in infos] == [1 if o % gop == 0 else 2 for o in ordinal], how
            assert [i.level for i in infos] == [o % gop for o in ordinal], how


def test_ragged_levels(torch, hip_lib, cases):
    """streams of 3, 1 and 2 pictures with gop 2: levels of 3 and 2 pictures, a scale per picture, the end flag on and off"""
    from jsmpeg_amd import encode
    frames = cases["enc_pan_176x144"][0][:6]
    streams, qs = [0, 0, 0, 1, 2, 2], [3, 9, 31, 8, 1, 5]
    with encode.Encoder(176, 144, 6, 4, 1 << 20, 3) as enc:
        t, ptrs = on_device(torch, frames)
        enc.set_gop(2, 7)
        for end in (True, False):
            enc.encode(ptrs, streams, qs, end)
            assert_equals(enc, streams, ep.sim_encode_p(frames, 176, 144, 2, 7, streams=streams, qscale=qs, frame_rate_code=3, end=end, max_streams=4), end)


def test_1080p_pair_twice(torch, hip_lib):
    from jsmpeg_amd import encode
    hd = ei.content_frames(1920, 1080, 2)
    want = ep.sim_encode_p(hd, 1920, 1080, 2, 7, qscale=8)
    assert want.stats[1][1] and want.stats[1][2]
    with encode.Encoder(1920, 1080, 2, 1, 8 << 20) as enc:
        t, ptrs = on_device(torch, hd)
        enc.set_gop(2, 7)
        for run in range(2):
            enc.encode(ptrs, None, 8)
            assert_equals(enc, [0], want, run)


def test_gop_1_is_the_intra_pass(torch, hip_lib, cases):
    from jsmpeg_amd import encode
    frames, w, h = cases["content_177x145"]
    with encode.Encoder(w, h, 3, 1, 1 << 20) as enc:
        t, ptrs = on_device(torch, frames)
        enc.set_gop(3, 7)
        enc.encode(ptrs, None, 8)
        enc.sync()
        enc.set_gop(1, 9)
        enc.encode(ptrs, None, 8)
        assert (whole_buffer(enc), enc.picture_ranges(), {0: enc.stream_range(0)}) == ei.sim_encode(frames, w, h, qscale=8)
        assert enc.picture_stats(1) == dict(intra=120, coded=0, not_coded=0, skipped=0)
        with pytest.raises(RuntimeError, match="gop 1"):
            enc.recon_ptr(0)


def test_round_trip_on_the_device(torch, hip_lib, libs):
    """decode a golden fixture with Batch, encode its 13 pictures as two streams with gop 4 from the pool, attach the encoder's
    buffer to a second Batch, decode it -- and once more through enqueue: the hashes of the encoder's own reconstructions, and the
    oracle's decode of the same streams"""
    from jsmpeg_amd import batch as jb
    from jsmpeg_amd import encode
    es = np.fromfile(os.path.join(ROOT, "tests", "golden", "enc_pan_176x144.m1v"), dtype=np.uint8)
    streams = [0] * 7 + [1] * 6
    with jb.Batch(176, 144, 1, 16, 1 << 20) as src, jb.Batch(176, 144, 2, 16, 1 << 20) as dst, \
            encode.Encoder(176, 144, 16, 2, 1 << 20) as enc:
        src.upload([es])
        assert src.decode() == 13
        enc.set_gop(4, 7)
        enc.encode_batch(src, list(range(13)), streams=streams, qscale=6)
        enc.sync()
        own = [int(hashing.frame_hash(*enc.recon(k))) for k in range(13)]
        oracle = []
        for s in (0, 1):
            frames, _, _ = cabi.decode_stream(libs["oracle"], np.frombuffer(enc.es(s), dtype=np.uint8), keep="planes")
            oracle += [int(hashing.frame_hash(*f)) for f in frames]
        assert own == oracle
        ptr, total = enc.device_es()
        begin, end = zip(*(enc.stream_range(s) for s in (0, 1)))
        for how in ("decode", "enqueue"):
            dst.attach_device(ptr, total, begin, end)
            if how == "decode":
                assert dst.decode() == 13
            else:
                assert dst.enqueue() == 0
                dst.sync()
            infos = dst.pictures()
            assert [i.stream for i in infos] == streams and all(i.decoded for i in infos)
            assert [int(h) for h in dst.frame_hashes()[:13]] == own, how
            ordinals = list(range(7)) + list(range(6))
            assert [i.type for i in infos] == [1 if o % 4 == 0 else 2 for o in ordinals]
            assert [i.level for i in infos] == [o % 4 for o in ordinals]


def test_tensor_input(torch, hip_lib):
    from jsmpeg_amd import encode
    w, h = 177, 145
    rgb = np.random.default_rng(w).integers(0, 256, (4, 3, h, w), dtype=np.uint8)
    base = (np.indices((h + 8, w + 8)).sum(0)[None] * np.array([1, 2, 3])[:, None, None]) % 256
    for k in range(1, 4):
        rgb[k] = base[:, k:k + h, 2 * k:2 * k + w]                   # the same picture moving: predicted macroblocks
    frames = list(ei.sim_rgb(rgb, 0, 0))
    want = ep.sim_encode_p(frames, w, h, 3, 7, qscale=5)
    assert sum(s[1] + s[2] + s[3] for s in want.stats) > 0
    with encode.Encoder(w, h, 4, 1, 1 << 21) as enc:
        enc.set_gop(3, 7)
        enc.encode_tensor(torch.from_numpy(rgb).cuda(), qscale=5)
        assert_equals(enc, [0], want, "tensor")


def test_pure_enqueue(torch, hip_lib):
    """with a gop pass in flight query is callable, a second encode and set_gop are refused; sync returns 0 afterwards"""
    from jsmpeg_amd import encode
    hd = ei.content_frames(1920, 1080, 1) * 8
    with encode.Encoder(1920, 1080, 8, 1, 32 << 20) as enc:
        t, ptrs = on_device(torch, hd)
        enc.set_gop(8, 15)
        torch.cuda.synchronize()
        enc.encode(ptrs, None, 4)
        assert enc.query() in (False, True)
        with pytest.raises(RuntimeError, match="in flight"):
            enc.encode(ptrs, None, 4)
        with pytest.raises(RuntimeError, match="in flight"):
            enc.set_gop(2, 0)
        enc.sync()
        assert enc.query() is True
        assert enc.L.jsmpeg_hip_encoder_sync(enc.h) == 0
        mbs = 120 * 68
        assert enc.picture_stats(0)["intra"] == mbs
        # the same picture eight times: nothing of pictures 1 .. 7 is intra
        assert all(enc.picture_stats(k)["intra"] == 0 and sum(enc.picture_stats(k).values()) == mbs for k in range(1, 8))


def test_overflow(torch, hip_lib, cases):
    """a max_es_bytes too small for the call: sync fails with the message, nothing is valid, the next call works"""
    from jsmpeg_amd import encode
    frames, w, h = cases["noise"]
    want = ep.sim_encode_p(frames, w, h, 5, 7, qscale=1)
    need = len(want.buf)
    with encode.Encoder(w, h, 4, 1, need - 16) as enc:
        t, ptrs = on_device(torch, frames)
        enc.set_gop(5, 7)
        enc.encode(ptrs, None, 1)
        with pytest.raises(RuntimeError, match="max_es_bytes"):
            enc.sync()
        for reader in (lambda: enc.es(0), enc.device_es, lambda: enc.recon_ptr(0), lambda: enc.picture_stats(0)):
            with pytest.raises(RuntimeError, match="overflowed"):
                reader()
        enc.encode(ptrs, None, 31)
        assert_equals(enc, [0], ep.sim_encode_p(frames, w, h, 5, 7, qscale=31), "after")
    with encode.Encoder(w, h, 4, 1, need) as enc:
        t, ptrs = on_device(torch, frames)
        enc.set_gop(5, 7)
        enc.encode(ptrs, None, 1)
        assert_equals(enc, [0], want, "fits")


def test_refusals(torch, hip_lib):
    from jsmpeg_amd import encode
    with encode.Encoder(64, 48, 2, 1, 1 << 16) as enc:
        for args, why in (((0, 7), "gop 0"), ((1025, 7), "gop 1025"), ((4, 16), "search_range 16")):
            with pytest.raises(RuntimeError, match=why):
                enc.set_gop(*args)
        with pytest.raises(RuntimeError, match="nothing was encoded"):
            enc.recon_ptr(0)
        t, ptrs = on_device(torch, [ei.flat_frame(64, 48, 1)] * 2)
        enc.encode(ptrs, None, 3)
        with pytest.raises(RuntimeError, match="gop 1"):
            enc.recon_ptr(0)
        # a refused call launches nothing and changes nothing: the handle is idle, the last call's results and the GOP stand
        before = (whole_buffer(enc), enc.picture_ranges())
        for args in ((0, 7), (4, 16)):
            with pytest.raises(RuntimeError):
                enc.set_gop(*args)
            assert enc.query() is True and (whole_buffer(enc), enc.picture_ranges()) == before
        enc.encode(ptrs, None, 3)
        assert (whole_buffer(enc), enc.picture_ranges()) == before and enc.picture_stats(1)["intra"] == 12      # still gop 1
        enc.set_gop(2, 0)
        enc.encode(ptrs, None, 3)
        assert enc.picture_stats(1) == dict(intra=0, coded=0, not_coded=6, skipped=6)
        with pytest.raises(RuntimeError):
            enc.set_gop(2, 16)
        enc.encode(ptrs, None, 3)
        assert enc.picture_stats(1) == dict(intra=0, coded=0, not_coded=6, skipped=6)                           # still gop 2, R 0
        with pytest.raises(RuntimeError, match="picture 2 of 2"):
            enc.picture_stats(2)
        with pytest.raises(RuntimeError, match="picture 2 of 2"):
            enc.recon_ptr(2)
        assert enc.L.jsmpeg_hip_encoder_set_gop(None, 2, 0) < 0


def test_exports(hip_lib):
    from jsmpeg_amd import encode
    L = encode.lib()
    for name in ("jsmpeg_hip_encoder_set_gop", "jsmpeg_hip_encoder_recon", "jsmpeg_hip_encoder_picture_stats"):
        assert name in encode.SYMBOLS and getattr(L, name)
