"""The intra encoder on the device (C ABI part 8, jsmpeg_amd/encode.py): the GPU's bytes equal the CPU simulator's
(tests/sim/sim_encode_pass.cpp) and the independent restatement's (tests/enc_ref.py); round trips through Batch and Live on the
device; tensor input; the pass as a pure enqueue; overflow and refusals.  Bytes and work done are asserted, never times."""
import ctypes
import os

import numpy as np
import pytest

import enc_inputs as ei
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
    return ei.small_cases(libs)


def on_device(torch, frames):
    """[N, frame_bytes] uint8 on the device and the rows' addresses"""
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


def result_of(enc, streams):
    return whole_buffer(enc), enc.picture_ranges(), {s: enc.stream_range(s) for s in sorted(set(streams))}


def gpu_encode(torch, frames, w, h, streams=None, qscale=8, end=True, frame_rate_code=0, max_streams=None, cap=None):
    from jsmpeg_amd import encode
    n = len(frames)
    cap = cap or 64 + n * (len(frames[0]) * 4 + 4096)
    with encode.Encoder(w, h, max(1, n), max_streams or (max(streams) + 1 if streams else 1), cap, frame_rate_code) as enc:
        t, ptrs = on_device(torch, frames)
        enc.encode(ptrs, streams, qscale, end)
        enc.sync()
        return result_of(enc, streams or [0])


@pytest.mark.parametrize("q", [1, 8, 31])
def test_small_inputs_equal_the_simulator_and_the_restatement(torch, hip_lib, cases, q):
    for name, (frames, w, h) in cases.items():
        got = gpu_encode(torch, frames, w, h, qscale=q)
        assert got == ei.sim_encode(frames, w, h, qscale=q), name
        assert got == enc_ref.encode(frames, w, h, qscale=q), name


def test_streams_scales_flags_equal_all_three(torch, hip_lib, cases):
    frames = cases["enc_pan_176x144"][0] + cases["content_176x144"][0]
    streams, qs = [0, 0, 2, 3, 3], [1, 31, 8, 2, 5]
    for end in (True, False):
        got = gpu_encode(torch, frames, 176, 144, streams, qs, end, frame_rate_code=3, max_streams=5)
        assert got == ei.sim_encode(frames, 176, 144, streams=streams, qscale=qs, frame_rate_code=3, end=end, max_streams=5)
        assert got == enc_ref.encode(frames, 176, 144, streams=streams, qscale=qs, frame_rate_code=3, end=end)


def test_noise_at_q1_equals_the_simulator(torch, hip_lib):
    frames = [ei.noise_frame(64, 48, 1), ei.noise_frame(64, 48, 2)]
    assert gpu_encode(torch, frames, 64, 48, qscale=1) == ei.sim_encode(frames, 64, 48, qscale=1)


def test_1080p_pair_and_what_the_bytes_do_not_depend_on(torch, hip_lib, libs):
    """against the simulator; the same picture bytes whatever the count, the grouping into streams, and on a second run"""
    from jsmpeg_amd import encode
    hd = ei.content_frames(1920, 1080, 2)
    want = ei.sim_encode(hd, 1920, 1080, qscale=8)
    with encode.Encoder(1920, 1080, 4, 4, 8 << 20) as enc:
        t, ptrs = on_device(torch, hd)
        for run in range(2):
            enc.encode(ptrs, None, 8)
            assert result_of(enc, [0]) == want
        pics = [want[0][o:o + b] for o, b in want[1]]
        enc.encode(ptrs[:1], None, 8)
        buf, ranges, _ = result_of(enc, [0])
        assert [buf[o:o + b] for o, b in ranges] == pics[:1]
        enc.encode(ptrs, [1, 3], 8)
        buf, ranges, sr = result_of(enc, [1, 3])
        got = [buf[o:o + b] for o, b in ranges]
        assert got[0] == pics[0] and got[1][:20] == pics[0][:20] and got[1][20:] == pics[1][20:]   # a stream's first picture: time code 0
        assert sr[1][0] == 16 and sr[3][0] % 16 == 0 and enc.stream_range(0) == (0, 0)
        enc.encode([ptrs[1], ptrs[0], ptrs[1], ptrs[0]], [0, 0, 1, 2], 8)
        buf, ranges, _ = result_of(enc, [0, 1, 2])
        got = [buf[o:o + b] for o, b in ranges]
        assert got[0][20:] == pics[1][20:] and got[1][20:] == pics[0][20:] and got[2][20:] == pics[1][20:] and got[3] == pics[0]
        ms = enc.timings()
        assert ms["total_ms"] > 0 and ms["convert_ms"] >= 0


def oracle_hashes(libs, es):
    frames, _, _ = cabi.decode_stream(libs["oracle"], np.frombuffer(es, dtype=np.uint8), keep="planes")
    return [hashing.frame_hash(*f) for f in frames]


def test_round_trip_on_the_device(torch, hip_lib, libs):
    """decode a golden fixture with Batch, encode its pictures (two streams) from the pool, attach the encoder's buffer to a
    second Batch, decode it -- and once more through enqueue: the oracle's decode of the same streams"""
    from jsmpeg_amd import batch as jb
    from jsmpeg_amd import encode
    es = np.fromfile(os.path.join(ROOT, "tests", "golden", "enc_pan_176x144.m1v"), dtype=np.uint8)
    with jb.Batch(176, 144, 2, 32, 1 << 20) as src, jb.Batch(176, 144, 2, 32, 4 << 20) as dst, \
            encode.Encoder(176, 144, 32, 2, 4 << 20) as enc:
        src.upload([es, es])
        assert src.decode() == 26
        pics = list(range(26))
        enc.encode_batch(src, pics, qscale=[2 + p % 7 for p in pics])
        enc.sync()
        want = [oracle_hashes(libs, enc.es(s)) for s in (0, 1)]
        assert len(want[0]) == len(want[1]) == 13
        ptr, total = enc.device_es()
        begin, end = zip(*(enc.stream_range(s) for s in (0, 1)))
        for how in ("decode", "enqueue"):
            dst.attach_device(ptr, total, begin, end)
            if how == "decode":
                assert dst.decode() == 26
            else:
                assert dst.enqueue() == 0
                dst.sync()
            hs = dst.frame_hashes()
            infos = dst.pictures()
            assert len(infos) == 26 and all(i.type == 1 and i.level == 0 and i.decoded for i in infos)
            for s in (0, 1):
                assert [int(hs[p]) for p, i in enumerate(infos) if i.stream == s] == want[s], how
            assert np.array_equal(dst.read_es(0), np.frombuffer(enc.es(0), dtype=np.uint8))
        # a picture that was not decoded is refused
        src.upload([es])
        src.select([(0, 0)])
        src.decode()
        skipped = [p for p, i in enumerate(src.pictures()) if not i.decoded]
        assert skipped
        with pytest.raises(ValueError, match="not decoded"):
            enc.encode_batch(src, [0, skipped[0]])


def test_live_round_trip(torch, hip_lib, libs):
    """encode_live after a tick of two streams == encode over the pictures' device_frame pointers"""
    from jsmpeg_amd import encode
    from jsmpeg_amd import live as jl
    es = np.fromfile(os.path.join(ROOT, "tests", "golden", "enc_pan_176x144.m1v"), dtype=np.uint8)
    offs = np.load(os.path.join(ROOT, "tests", "golden", "enc_pan_176x144.offsets.npy"))
    with jl.Live(176, 144, 2, pictures_per_tick=2, store_bytes=1 << 18) as lv, encode.Encoder(176, 144, 8, 2, 1 << 20) as enc:
        ids = [lv.open(), lv.open()]
        for i in ids:
            lv.write(i, es[int(offs[0]):int(offs[2])], pts=0.0)
        assert lv.tick(flush=True) == 4
        used = enc.encode_live(lv, qscale=6)
        assert [p.stream for p in used] == [ids[0], ids[0], ids[1], ids[1]]
        a = result_of(enc, [0, 1])
        enc.encode([p.device_frame for p in used], [0, 0, 1, 1], 6)
        assert result_of(enc, [0, 1]) == a
        want, _, _ = cabi.decode_stream(libs["oracle"], es, keep="planes", max_frames=2)
        frames = [ei.frame_of(*f) for f in want]
        assert a == ei.sim_encode(frames + frames, 176, 144, streams=[0, 0, 1, 1], qscale=6)


@pytest.mark.parametrize("size", [(176, 144), (177, 145)], ids=lambda s: "%dx%d" % s)
def test_tensor_input(torch, hip_lib, size):
    """NCHW and NHWC, RGB and BGR: the bytes of encode over planes computed by the restatement's conversion"""
    from jsmpeg_amd import encode
    w, h = size
    rgb = np.random.default_rng(w).integers(0, 256, (3, h, w, 3), dtype=np.uint8)
    rgb[2] = (np.indices((h, w)).sum(0)[..., None] * np.array([1, 2, 3])) % 256
    frames = [enc_ref.rgb_to_frame(rgb[k]) for k in range(3)]
    want = ei.sim_encode(frames, w, h, streams=[0, 1, 1], qscale=5)
    with encode.Encoder(w, h, 3, 2, 1 << 21) as enc:
        for layout in ("nchw", "nhwc"):
            for order in ("rgb", "bgr"):
                src = rgb[..., ::-1] if order == "bgr" else rgb
                x = torch.from_numpy(np.ascontiguousarray(src.transpose(0, 3, 1, 2) if layout == "nchw" else src)).cuda()
                enc.encode_tensor(x, streams=[0, 1, 1], qscale=5, order=order)
                assert result_of(enc, [0, 1]) == want, (layout, order)
        with pytest.raises(ValueError):
            enc.encode_tensor(torch.zeros((1, 3, h + 1, w), dtype=torch.uint8, device="cuda"))
        with pytest.raises(ValueError):
            enc.encode_tensor(torch.zeros((1, 3, h, w), dtype=torch.float32, device="cuda"))


def test_tensor_round_trip_quality(torch, hip_lib, libs):
    """Batch.tensor(uint8) -> encode_tensor -> decode: the luma PSNR against the first decode is finite and above the q = 31
    figure of the same content (printed; tools/encode_bench.py records it in profiles/enc_notes.md)"""
    from jsmpeg_amd import batch as jb
    from jsmpeg_amd import encode
    es = np.fromfile(os.path.join(ROOT, "tests", "golden", "enc_pan_176x144.m1v"), dtype=np.uint8)
    first, _, _ = cabi.decode_stream(libs["oracle"], es, keep="planes", max_frames=4)
    frames = [ei.frame_of(*f) for f in first]
    with jb.Batch(176, 144, 1, 16, 1 << 20) as b, encode.Encoder(176, 144, 4, 1, 1 << 20) as enc:
        b.upload([es])
        b.decode()
        x = b.tensor(pictures=[0, 1, 2, 3], dtype=torch.uint8)
        got = {}
        for q in (8, 31):
            enc.encode_tensor(x, qscale=q)
            dec, _, _ = cabi.decode_stream(libs["oracle"], np.frombuffer(enc.es(0), dtype=np.uint8), keep="planes")
            assert len(dec) == 4
            got[q] = ei.psnr(*ei.luma_sse(dec, frames, 176, 144))
        print("tensor round trip, enc_pan_176x144, luma PSNR against the first decode: q 8 %.2f dB, q 31 %.2f dB" % (got[8], got[31]))
        assert np.isfinite(got[8]) and got[8] > got[31]


def test_pure_enqueue(torch, hip_lib):
    """with a pass in flight query is callable and a second encode is refused; sync returns 0 afterwards"""
    from jsmpeg_amd import encode
    hd = ei.content_frames(1920, 1080, 1) * 8
    with encode.Encoder(1920, 1080, 8, 1, 32 << 20) as enc:
        t, ptrs = on_device(torch, hd)
        torch.cuda.synchronize()
        enc.encode(ptrs, None, 4)
        assert enc.query() in (False, True)
        with pytest.raises(RuntimeError, match="in flight"):
            enc.encode(ptrs, None, 4)
        enc.sync()
        assert enc.query() is True
        assert enc.L.jsmpeg_hip_encoder_sync(enc.h) == 0
        assert len(enc.picture_ranges()) == 8 and len({whole_buffer(enc)[o + 20:o + b] for o, b in enc.picture_ranges()}) == 1


def test_overflow(torch, hip_lib):
    """a max_es_bytes too small for a noise picture: sync fails with the message, es() is refused, the next call works"""
    from jsmpeg_amd import encode
    noise, flat = [ei.noise_frame(64, 48, 1)], [ei.flat_frame(64, 48, 9)]
    need = len(ei.sim_encode(noise, 64, 48, qscale=1)[0])
    with encode.Encoder(64, 48, 1, 1, need - 16) as enc:
        t, ptrs = on_device(torch, noise + flat)
        enc.encode(ptrs[:1], None, 1)
        with pytest.raises(RuntimeError, match="max_es_bytes"):
            enc.sync()
        with pytest.raises(RuntimeError, match="overflowed"):
            enc.es(0)
        with pytest.raises(RuntimeError, match="overflowed"):
            enc.device_es()
        enc.encode(ptrs[1:], None, 1)
        enc.sync()
        assert result_of(enc, [0]) == ei.sim_encode(flat, 64, 48, qscale=1)
    with encode.Encoder(64, 48, 1, 1, need) as enc:
        t, ptrs = on_device(torch, noise)
        enc.encode(ptrs, None, 1)
        enc.sync()
        assert result_of(enc, [0]) == ei.sim_encode(noise, 64, 48, qscale=1)


def test_refusals(torch, hip_lib):
    from jsmpeg_amd import encode
    for bad in (dict(width=0), dict(height=0), dict(width=4096), dict(height=176 * 16), dict(max_pictures=0), dict(max_streams=0),
                dict(frame_rate_code=9)):
        kw = dict(width=64, height=48, max_pictures=2, max_streams=2, max_es_bytes=1 << 16, frame_rate_code=0)
        kw.update(bad)
        with pytest.raises(RuntimeError):
            encode.Encoder(**kw)
    with encode.Encoder(64, 48, 2, 2, 1 << 16) as enc:
        t, ptrs = on_device(torch, [ei.flat_frame(64, 48, 1)] * 3)
        for args, why in (((ptrs[:2], None, 0), "quantiser_scale"), ((ptrs[:2], None, 32), "quantiser_scale"),
                          ((ptrs[:2], None, [3, 0]), "qscale"), ((ptrs[:2], [1, 0], 3), "ascend"), ((ptrs[:2], [0, 2], 3), "max_streams"),
                          ((ptrs, None, 3), "max_pictures"), (([ptrs[0], 0], None, 3), "NULL"), (([ptrs[0] + 4], None, 3), "aligned")):
            with pytest.raises(RuntimeError, match=why):
                enc.encode(*args)
        with pytest.raises(RuntimeError, match="nothing was encoded"):
            enc.es(0)
        enc.encode(ptrs[:2], [0, 1], 3)
        assert len(enc.es(0)) == len(enc.es(1)) > 28
        with pytest.raises(RuntimeError):
            enc.stream_range(2)
