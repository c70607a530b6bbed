"""The encoder's scaled input on the device (jsmpeg_hip_encoder_encode_scaled, Encoder.encode_scaled; the rule:
jsmpeg_amd/csrc/enc_scale.h): the planes k_enc_scale leaves in the handle's frame store equal the CPU simulator's
(tests/sim/sim_encode_scale.cpp) and the numpy restatement's (tests/enc_scale_ref.py) bit for bit, and everything behind them
-- the intra pass, the level loop with rate control and chains, a relay from a Live -- equals the existing simulators over
those planes.  Bytes are asserted, never times."""
import ctypes
import os

import numpy as np
import pytest

import enc_chain_inputs as ec
import enc_inputs as ei
import enc_p_inputs as ep
import enc_ref
import enc_scale_inputs as si
import enc_scale_ref as es
from conftest import ROOT

pytestmark = pytest.mark.gpu

PAN = ep.pan_frames(64, 48, 7, (3, -2))
PAN9 = ep.pan_frames(64, 48, 9, (2, 1))


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


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


def source_bytes(enc, k):
    return np.concatenate([p.ravel() for p in enc.source(k)])


def recon_bytes(enc, k):
    return np.concatenate([p.ravel() for p in enc.recon(k)])


def capacity(frames):
    return 64 + len(frames) * (len(frames[0]) * 4 + 4096)


@pytest.mark.parametrize("name", sorted(si.CASES))
def test_planes_and_bytes(torch, hip_lib, name):
    """(fails without the feature: jsmpeg_hip_encoder_encode_scaled is missing)"""
    from jsmpeg_amd import encode
    w, h, crop, ow, oh, aa = si.CASES[name]
    frames, want = si.case_frames(name), si.case_want(name)
    with encode.Encoder(ow, oh, 2, 2, capacity(want)) as enc:
        t, ptrs = on_device(torch, frames)
        enc.encode_scaled(ptrs, (w, h), crop, bool(aa), streams=[0, 1], qscale=5)
        for k in range(2):
            got = source_bytes(enc, k)
            assert np.array_equal(got, want[k]), (name, k, int(np.count_nonzero(got != want[k])))
            assert np.array_equal(got, si.sim_frame(frames[k], w, h, ow, oh, crop, aa)), (name, k)
            assert enc.source_ptr(k) not in ptrs
        assert result_of(enc, [0, 1]) == ei.sim_encode(want, ow, oh, streams=[0, 1], qscale=5)
        assert enc.timings()["convert_ms"] > 0
        # the same geometry again (the table is kept), then another one on the same handle, then the first again
        enc.encode_scaled(ptrs[::-1], (w, h), crop, bool(aa), streams=[0, 1], qscale=5)
        assert np.array_equal(source_bytes(enc, 0), want[1]) and np.array_equal(source_bytes(enc, 1), want[0])
        enc.encode_scaled(ptrs[:1], (w, h), None, not aa, qscale=5)
        assert np.array_equal(source_bytes(enc, 0), es.scale_frame(frames[0], w, h, ow, oh, None, not aa)), name
        enc.encode_scaled(ptrs, (w, h), crop, bool(aa), streams=[0, 1], qscale=5)
        assert np.array_equal(source_bytes(enc, 1), want[1])


def test_equal_size_is_a_copy(torch, hip_lib):
    from jsmpeg_amd import encode
    frames = ei.content_frames(177, 145, 2)
    with encode.Encoder(177, 145, 2, 1, capacity(frames)) as enc:
        t, ptrs = on_device(torch, frames)
        enc.encode_scaled(ptrs, (177, 145), qscale=7)
        got = result_of(enc, [0])
        for k in range(2):
            a, b = enc.source(k), es.source_planes(frames[k], 177, 145)
            assert np.array_equal(a[0][:145, :177], b[0][:145, :177]) and np.array_equal(a[1][:73, :89], b[1][:73, :89])
            assert np.array_equal(source_bytes(enc, k), es.scale_frame(frames[k], 177, 145, 177, 145))
        assert got == ei.sim_encode([es.scale_frame(f, 177, 145, 177, 145) for f in frames], 177, 145, qscale=7)


def test_source_after_the_other_entry_points(torch, hip_lib):
    from jsmpeg_amd import encode
    w, h = 65, 33
    frames = [ei.noise_frame(w, h, 1), ei.noise_frame(w, h, 2)]
    rgb = np.random.default_rng(8).integers(0, 256, (2, h, w, 3), dtype=np.uint8)
    with encode.Encoder(w, h, 2, 1, capacity(frames)) as enc:
        with pytest.raises(RuntimeError, match="nothing was encoded"):
            enc.source(0)
        t, ptrs = on_device(torch, frames)
        enc.encode(ptrs, None, 6)
        for k in range(2):
            assert enc.source_ptr(k) == ptrs[k] and np.array_equal(source_bytes(enc, k), frames[k])
        enc.encode_tensor(torch.from_numpy(rgb).cuda(), qscale=6)
        for k in range(2):
            assert enc.source_ptr(k) not in ptrs and np.array_equal(source_bytes(enc, k), enc_ref.rgb_to_frame(rgb[k]))
        with pytest.raises(RuntimeError, match="picture 2 of 2"):
            enc.source(2)


class Scaled:
    """ec.Chain's encode on the device through encode_scaled: the source frames go up, the call's result comes back"""

    def __init__(self, torch, enc, size, rate):
        self.torch, self.enc, self.size, self.rate = torch, enc, size, rate

    def encode(self, frames, streams, qscale=8, end=False, chain=True):
        self.keep, ptrs = on_device(self.torch, frames)
        enc, n = self.enc, len(frames)
        enc.encode_scaled(ptrs, self.size, streams=streams, qscale=qscale, end=end, chain=chain)
        present = sorted(set(streams)) if streams is not None else [0]
        r = ep.Result(whole_buffer(enc), enc.picture_ranges(), {s: enc.stream_range(s) for s in present}, [recon_bytes(enc, k) for k in range(n)], None,
                      [tuple(enc.picture_stats(k)[name] for name in ep.KINDS) for k in range(n)])
        r.rate = [tuple(enc.picture_rate(k)[name] for name in ("q", "budget", "bytes")) for k in range(n)] if self.rate else None
        r.source = [source_bytes(enc, k) for k in range(n)]
        return r


def test_the_scaled_store_feeds_the_level_loop(torch, hip_lib):
    """the 64x48 pans upscaled to 80x64, gop 3 with rate control, two streams, three chained calls of two pictures per stream:
    every call equals the chain simulator's over the restatement-scaled frames, and every stream's pieces the one-call simulator's"""
    from jsmpeg_amd import encode
    rule = dict(T=260, q_min=1, q_max=31, W=4)
    own = {0: PAN[:6], 1: PAN9[:6]}
    scaled = {s: [es.scale_frame(f, 64, 48, 80, 64) for f in own[s]] for s in own}
    with encode.Encoder(80, 64, 4, 2, capacity(scaled[0][:4])) as enc, ec.Chain(80, 64, 2) as sim:
        dev = Scaled(torch, enc, (64, 48), True)
        for h in (enc, sim):
            h.set_gop(3, 7)
            h.set_rate(rule["T"], rule["q_min"], rule["q_max"], rule["W"])
        led = ec.Ledger()
        for i in range(3):
            pick = lambda d: d[0][2 * i:2 * i + 2] + d[1][2 * i:2 * i + 2]
            got = dev.encode(pick(own), [0, 0, 1, 1], end=i == 2)
            want = sim.encode(pick(scaled), [0, 0, 1, 1], end=i == 2)
            for k in range(4):
                assert np.array_equal(got.source[k], pick(scaled)[k]), (i, k)
                assert np.array_equal(got.recon[k], want.recon[k]), (i, k)
            assert got.buf == want.buf and got.ranges == want.ranges and got.streams == want.streams and got.stats == want.stats, i
            assert got.rate == [(q, min(b, 0xffffffff), n) for q, b, n in want.rate], i
            led.add(pick(scaled), [0, 0, 1, 1], got, i == 2)
        for s in (0, 1):
            (seg,) = led.segments[s]
            one = ec.one_call(seg, 80, 64, 3, 7, rule=rule)
            ec.assert_segment(seg, one, s)
            assert ep.picture_types(one.stream(0)) == ep.expected_types(6, 3)
        assert enc.chain_info(0) == (False, 0)


GOLDEN = os.path.join(ROOT, "tests", "golden", "enc_pan_176x144")


def test_relay_round_trip(torch, hip_lib, libs):
    """a Live at 176x144 fed the golden pan, a picture per tick through encode_live into an 80x64 encoder, chained, gop 4: the
    pieces are the one-call simulator's stream over the restatement-scaled oracle pictures, and the oracle decodes it"""
    from jsmpeg_amd import encode
    from jsmpeg_amd import live as jl
    ticks = 6
    es_in = np.fromfile(GOLDEN + ".m1v", dtype=np.uint8)
    offs = [int(v) for v in np.load(GOLDEN + ".offsets.npy")]
    first, w, h = ei.golden_frames(libs, "enc_pan_176x144", ticks)
    assert (w, h) == (176, 144) and len(first) == ticks
    scaled = [es.scale_frame(f, 176, 144, 80, 64) for f in first]
    with jl.Live(176, 144, 1, pictures_per_tick=1, store_bytes=1 << 18) as lv, encode.Encoder(80, 64, 1, 1, 1 << 18) as enc:
        enc.set_gop(4, 7)
        i, pieces = lv.open(), []
        for t in range(ticks):
            lv.write(i, es_in[offs[t]:offs[t + 1]], pts=t / 30.0)
            assert lv.tick(flush=True) == 1
            used = enc.encode_live(lv, qscale=6, end=t + 1 == ticks, chain=True)
            assert len(used) == 1 and enc.source_ptr(0) != used[0].device_frame
            assert np.array_equal(source_bytes(enc, 0), scaled[t]), t
            pieces.append(enc.es(0))
    out = b"".join(pieces)
    want = ep.sim_encode_p(scaled, 80, 64, 4, 7, qscale=6, end=True)
    assert out == want.stream(0).tobytes()
    dec = ep.oracle_frames(libs, np.frombuffer(out, dtype=np.uint8))
    assert len(dec) == ticks and ep.picture_types(np.frombuffer(out, dtype=np.uint8)) == ep.expected_types(ticks, 4)
    cw, ch = enc_ref.coded(80, 64)
    psnr = ei.psnr(*ei.luma_sse([(d[:cw * ch],) for d in dec], scaled, 80, 64))
    print("relay 176x144 -> 80x64, gop 4, q 6: luma PSNR against the scaled pictures %.2f dB" % psnr)
    assert np.isfinite(psnr) and psnr > 20.0


def test_two_renditions_from_one_tick(torch, hip_lib, libs):
    """two encoders fed from the same tick of two live streams, each on a HIP stream of its own, both in flight at once: each
    equals what it writes alone, and the simulator over the restatement-scaled pictures"""
    from jsmpeg_amd import encode
    from jsmpeg_amd import live as jl
    es_in = np.fromfile(GOLDEN + ".m1v", dtype=np.uint8)
    offs = [int(v) for v in np.load(GOLDEN + ".offsets.npy")]
    first, _, _ = ei.golden_frames(libs, "enc_pan_176x144", 2)
    sizes = [(80, 64), (48, 32)]
    with jl.Live(176, 144, 2, pictures_per_tick=1, store_bytes=1 << 18) as lv, encode.Encoder(80, 64, 2, 2, 1 << 18) as a, \
            encode.Encoder(48, 32, 2, 2, 1 << 18) as b:
        ids = [lv.open(), lv.open()]
        lv.write(ids[0], es_in[offs[0]:offs[1]], pts=0.0)
        lv.write(ids[1], es_in[offs[0]:offs[1]], pts=0.0)
        assert lv.tick(flush=True) == 2
        alone = []
        for enc in (a, b):
            enc.encode_live(lv, qscale=4)
            alone.append((result_of(enc, [0, 1]), [source_bytes(enc, k) for k in range(2)]))
        s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        a.encode_live(lv, qscale=4, stream=s1.cuda_stream)
        b.encode_live(lv, qscale=4, stream=s2.cuda_stream)
        for enc, (res, planes), (ow, oh) in zip((a, b), alone, sizes):
            assert result_of(enc, [0, 1]) == res
            want = [es.scale_frame(first[0], 176, 144, ow, oh)] * 2
            for k in range(2):
                assert np.array_equal(source_bytes(enc, k), planes[k]) and np.array_equal(planes[k], want[k]), (ow, k)
            assert res == ei.sim_encode(want, ow, oh, streams=[0, 1], qscale=4)


def test_batch_of_another_size_and_a_crop(torch, hip_lib, libs):
    """encode_batch: another size goes through encode_scaled, the same size stays on encode unless a crop is given"""
    from jsmpeg_amd import batch as jb
    from jsmpeg_amd import encode
    es_in = np.fromfile(GOLDEN + ".m1v", dtype=np.uint8)
    first, _, _ = ei.golden_frames(libs, "enc_pan_176x144", 2)
    with jb.Batch(176, 144, 1, 16, 1 << 20) as src, encode.Encoder(88, 72, 2, 1, 1 << 18) as half, encode.Encoder(176, 144, 2, 1, 1 << 20) as same:
        src.upload([es_in])
        src.decode()
        half.encode_batch(src, [0, 1], streams=[0, 0], qscale=5)
        assert np.array_equal(source_bytes(half, 1), es.scale_frame(first[1], 176, 144, 88, 72))
        half.encode_batch(src, [0, 1], streams=[0, 0], qscale=5, crop=(32, 16, 88, 72), antialias=False)
        assert np.array_equal(source_bytes(half, 0), es.scale_frame(first[0], 176, 144, 88, 72, (32, 16, 88, 72), False))
        same.encode_batch(src, [0, 1], streams=[0, 0], qscale=5)
        assert same.source_ptr(0) == src.frame_pool_ptr
        same.encode_batch(src, [0, 1], streams=[0, 0], qscale=5, crop=(0, 0, 100, 100))
        assert same.source_ptr(0) != src.frame_pool_ptr
        assert np.array_equal(source_bytes(same, 0), es.scale_frame(first[0], 176, 144, 176, 144, (0, 0, 100, 100)))


def test_pure_enqueue(torch, hip_lib):
    """with a scaled pass in flight query is callable and a second call is refused"""
    from jsmpeg_amd import encode
    hd = si.case_frames("7_1080p_to_640x360")
    with encode.Encoder(640, 360, 8, 1, 8 << 20) as enc:
        t, ptrs = on_device(torch, hd)
        torch.cuda.synchronize()
        enc.encode_scaled([ptrs[0], ptrs[1]] * 4, (1920, 1080), qscale=4)
        assert enc.query() in (False, True)
        with pytest.raises(RuntimeError, match="in flight"):
            enc.encode_scaled(ptrs, (1920, 1080), qscale=4)
        enc.sync()
        assert enc.query() is True and enc.L.jsmpeg_hip_encoder_sync(enc.h) == 0
        want = si.case_want("7_1080p_to_640x360")
        for k in range(8):
            assert np.array_equal(source_bytes(enc, k), want[k & 1]), k


def test_overflow(torch, hip_lib):
    """a scaled call that overflows max_es_bytes fails in sync(); the next call works"""
    from jsmpeg_amd import encode
    noise, smooth = ei.noise_frame(64, 48, 1), si.smooth_frame(64, 48)
    want = [es.scale_frame(f, 64, 48, 160, 112, None, False) for f in (noise, smooth)]
    need = len(ei.sim_encode(want[:1], 160, 112, qscale=1)[0])
    with encode.Encoder(160, 112, 1, 1, need - 16) as enc:
        t, ptrs = on_device(torch, [noise, smooth])
        enc.encode_scaled(ptrs[:1], (64, 48), antialias=False, qscale=1)
        with pytest.raises(RuntimeError, match="max_es_bytes"):
            enc.sync()
        for reader in (lambda: enc.es(0), lambda: enc.source(0)):
            with pytest.raises(RuntimeError, match="overflowed"):
                reader()
        enc.encode_scaled(ptrs[1:], (64, 48), antialias=False, qscale=1)
        enc.sync()
        assert result_of(enc, [0]) == ei.sim_encode(want[1:], 160, 112, qscale=1)


def test_refusals(torch, hip_lib):
    """every descriptor refusal launches nothing and leaves the handle working and the call before readable"""
    from jsmpeg_amd import batch, encode
    frames = [ei.noise_frame(176, 144, 1), ei.noise_frame(176, 144, 2)]
    want = [es.scale_frame(f, 176, 144, 64, 48) for f in frames]
    with encode.Encoder(64, 48, 2, 2, capacity(want)) as enc:
        t, ptrs = on_device(torch, frames)
        enc.encode_scaled(ptrs, (176, 144), streams=[0, 1], qscale=3)
        before = result_of(enc, [0, 1])
        assert before == ei.sim_encode(want, 64, 48, streams=[0, 1], qscale=3)
        for size, crop, aa, why in (((0, 144), None, 1, "1 .. 4095"), ((176, 0), None, 1, "1 .. 4095"), ((4096, 144), None, 1, "1 .. 4095"),
                                    ((176, 4096), None, 1, "1 .. 4095"), ((176, 144), (100, 0, 100, 100), 1, "crop"),
                                    ((176, 144), (0, 100, 100, 100), 1, "crop"), ((176, 144), (0, 0, 0, 10), 1, "crop"),
                                    ((176, 144), (2, 2, 0, 0), 1, "crop"), ((176, 144), (1, 0, 64, 48), 1, "even"),
                                    ((176, 144), (0, 1, 64, 48), 1, "even"), ((176, 144), None, 2, "antialias")):
            src = encode.EncSource(size[0], size[1], *(crop or (0, 0, 0, 0)), aa)
            arr = (ctypes.c_void_p * 2)(*ptrs)
            assert enc.L.jsmpeg_hip_encoder_encode_scaled(enc.h, arr, ctypes.byref(src), None, None, 2, 3, 1, None) < 0, (size, crop, aa)
            assert why in batch.last_error(), batch.last_error()
            assert enc.query() is True and result_of(enc, [0, 1]) == before and np.array_equal(source_bytes(enc, 1), want[1])
        arr = (ctypes.c_void_p * 2)(*ptrs)
        assert enc.L.jsmpeg_hip_encoder_encode_scaled(enc.h, arr, None, None, None, 2, 3, 1, None) < 0 and "null source" in batch.last_error()
        # the existing argument checks apply as they do to encode()
        for args, kw, why in (((ptrs,), dict(qscale=0), "quantiser_scale"), ((ptrs,), dict(streams=[1, 0]), "ascend"),
                              ((ptrs + ptrs[:1],), dict(), "max_pictures"), (([ptrs[0], 0],), dict(), "NULL"), (([ptrs[0] + 4],), dict(), "aligned")):
            with pytest.raises(RuntimeError, match=why):
                enc.encode_scaled(*args, (176, 144), **kw)
        assert result_of(enc, [0, 1]) == before
        enc.encode_scaled(ptrs[::-1], (176, 144), crop=(174, 142, 2, 2), streams=[0, 1], qscale=3)     # flush with the right and bottom edges
        assert np.array_equal(source_bytes(enc, 0), es.scale_frame(frames[1], 176, 144, 64, 48, (174, 142, 2, 2)))
