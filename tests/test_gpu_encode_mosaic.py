"""The encoder's mosaic input on the device (jsmpeg_hip_encoder_set_mosaic / _encode_mosaic, Encoder.encode_mosaic; the rule:
jsmpeg_amd/csrc/enc_mosaic.h): the planes k_enc_mosaic leaves in the handle's frame store equal the CPU simulator's
(tests/sim/sim_encode_mosaic.cpp) and the numpy restatement's (tests/enc_mosaic_ref.py) bit for bit, and everything behind them
-- the intra pass, the level loop with rate control and chains, a relay from two Lives -- equals the existing simulators over
those planes.  Bytes are asserted, never times.  (Every test here fails without the feature: set_mosaic is missing.)"""
import ctypes
import os

import numpy as np
import pytest

import enc_chain_inputs as ec
import enc_inputs as ei
import enc_mosaic_inputs as mi
import enc_mosaic_ref as em
import enc_p_inputs as ep
import enc_ref
import enc_scale_inputs as si
import enc_scale_ref as es
from conftest import ROOT

pytestmark = pytest.mark.gpu

PAN = ep.pan_frames(64, 48, 7, (3, -2))
PAN9 = ep.pan_frames(64, 48, 9, (2, 1))
GOLDEN = os.path.join(ROOT, "tests", "golden", "enc_pan_176x144")


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


class Device:
    """source frames on the device, kept alive: ptr(frame) -> its address, None -> None"""

    def __init__(self, torch):
        self.torch, self.keep = torch, []

    def ptr(self, frame):
        if frame is None:
            return None
        t = self.torch.from_numpy(np.ascontiguousarray(frame, dtype=np.uint8)).cuda()
        self.keep.append(t)
        assert t.data_ptr() % 16 == 0
        return t.data_ptr()

    def pictures(self, pictures):
        return [[self.ptr(f) for f in pic] for pic in pictures]


def cells_of(cells):
    from jsmpeg_amd import encode
    return [encode.cell((sw, sh), x, y, w, h, crop, bool(aa)) for sw, sh, crop, aa, x, y, w, h in cells]


def device_read(ptr, n):
    from jsmpeg_amd import batch
    out = np.zeros(n, dtype=np.uint8)
    L = batch.lib()
    L.jsmpeg_hip_device_read.restype = ctypes.c_int
    L.jsmpeg_hip_device_read.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64]
    assert L.jsmpeg_hip_device_read(out.ctypes.data, ptr, n) == 0
    return out


def whole_buffer(enc):
    """the call's device buffer on the host, its 256-byte tail checked"""
    p, total = enc.device_es()
    out = device_read(p, total + 256)
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


@pytest.mark.parametrize("name", sorted(mi.LAYOUTS))
def test_planes_and_bytes(torch, hip_lib, name):
    """two pictures on two streams, cells absent from the second: source(k) equals the restatement and the simulator, the
    streams the pass simulator's over those planes; the same layout again, another layout on the handle, the first again"""
    from jsmpeg_amd import encode
    w, h, fill, cells, present = mi.LAYOUTS[name]
    frames, want = mi.layout_frames(name), mi.layout_want(name)
    dev = Device(torch)
    with encode.Encoder(w, h, 2, 2, capacity(want)) as enc:
        enc.set_mosaic(cells_of(cells), fill)
        ptrs = dev.pictures(frames)
        enc.encode_mosaic(ptrs, streams=[0, 1], qscale=5)
        for k in range(2):
            got = source_bytes(enc, k)
            assert np.array_equal(got, want[k]), (name, k, int(np.count_nonzero(got != want[k])))
            assert np.array_equal(got, mi.sim_frame(cells, frames[k], w, h, fill)), (name, k)
            assert enc.source_ptr(k) not in [p for pic in ptrs for p in pic]
        first = result_of(enc, [0, 1])
        assert first == ei.sim_encode(want, w, h, streams=[0, 1], qscale=5)
        assert enc.timings()["convert_ms"] > 0
        enc.encode_mosaic(ptrs, streams=[0, 1], qscale=5)
        assert result_of(enc, [0, 1]) == first and np.array_equal(source_bytes(enc, 1), want[1])
        # another layout: the cells in reverse order (what overlaps is pasted the other way round), another fill, all present
        other = (fill[2], fill[0], fill[1])
        enc.set_mosaic(cells_of(cells[::-1]), other)
        enc.encode_mosaic([ptrs[0][::-1]], qscale=5)
        assert np.array_equal(source_bytes(enc, 0), em.compose(cells[::-1], frames[0][::-1], w, h, other)), name
        enc.set_mosaic(cells_of(cells), fill)
        enc.encode_mosaic(ptrs, streams=[0, 1], qscale=5)
        assert result_of(enc, [0, 1]) == first and np.array_equal(source_bytes(enc, 0), want[0])


@pytest.mark.parametrize("name", ["1_odd_177x145_to_65x33", "6_odd_crop_plain"])
def test_one_cell_is_encode_scaled(torch, hip_lib, name):
    """one cell over the whole picture equals encode_scaled ON THE DEVICE, in planes and in bytes"""
    from jsmpeg_amd import encode
    w, h, crop, ow, oh, aa = si.CASES[name]
    frames, want = si.case_frames(name), si.case_want(name)
    dev = Device(torch)
    ptrs = [dev.ptr(f) for f in frames]
    with encode.Encoder(ow, oh, 2, 2, capacity(want)) as a, encode.Encoder(ow, oh, 2, 2, capacity(want)) as b:
        a.encode_scaled(ptrs, (w, h), crop, bool(aa), streams=[0, 1], qscale=5)
        b.set_mosaic([encode.cell((w, h), 0, 0, ow, oh, crop, bool(aa))], (1, 2, 3))
        b.encode_mosaic([[p] for p in ptrs], streams=[0, 1], qscale=5)
        for k in range(2):
            assert np.array_equal(source_bytes(a, k), source_bytes(b, k)) and np.array_equal(source_bytes(b, k), want[k]), (name, k)
        assert result_of(a, [0, 1]) == result_of(b, [0, 1])


class Mosaic:
    """ec.Chain's encode on the device through encode_mosaic: a picture is a list of source frames, one per cell"""

    def __init__(self, torch, enc):
        self.torch, self.enc = torch, enc

    def encode(self, pictures, streams, qscale=8, end=False, chain=True):
        dev = Device(self.torch)
        enc, n = self.enc, len(pictures)
        enc.encode_mosaic(dev.pictures(pictures), streams=streams, qscale=qscale, end=end, chain=chain)
        present = sorted(set(streams)) if streams is not None else [0]
        r = ep.Result(whole_buffer(enc), enc.picture_ranges(), {s: enc.stream_range(s) for s in present}, [recon_bytes(enc, k) for k in range(n)], None,
                      [tuple(enc.picture_stats(k)[name] for name in ep.KINDS) for k in range(n)])
        r.rate = [tuple(enc.picture_rate(k)[name] for name in ("q", "budget", "bytes")) for k in range(n)]
        r.source = [source_bytes(enc, k) for k in range(n)]
        return r


def test_the_composed_store_feeds_the_level_loop(torch, hip_lib):
    """two 64x48 pans side by side in an 80x64 encoder (40x64 each, the second stream with the pans swapped), gop 3 with rate
    control, two streams, three chained calls of two pictures per stream: every call equals the chain simulator's over the
    restatement's planes, and every stream's pieces the one-call simulator's"""
    from jsmpeg_amd import encode
    rule = dict(T=260, q_min=1, q_max=31, W=4)
    cells = [(64, 48, None, 1, 0, 0, 40, 64), (64, 48, None, 1, 40, 0, 40, 64)]
    own = {0: [[a, b] for a, b in zip(PAN[:6], PAN9[:6])], 1: [[b, a] for a, b in zip(PAN[:6], PAN9[:6])]}
    composed = {s: [em.compose(cells, pic, 80, 64) for pic in own[s]] for s in own}
    with encode.Encoder(80, 64, 4, 2, capacity(composed[0][:4])) as enc, ec.Chain(80, 64, 2) as sim:
        enc.set_mosaic(cells_of(cells))
        dev = Mosaic(torch, enc)
        for h in (enc, sim):
            h.set_gop(3, 7)
            h.set_rate(rule["T"], rule["q_min"], rule["q_max"], rule["W"])
        led = ec.Ledger()
        for i in range(3):
            pick = lambda d: d[0][2 * i:2 * i + 2] + d[1][2 * i:2 * i + 2]
            got = dev.encode(pick(own), [0, 0, 1, 1], end=i == 2)
            want = sim.encode(pick(composed), [0, 0, 1, 1], end=i == 2)
            for k in range(4):
                assert np.array_equal(got.source[k], pick(composed)[k]), (i, k)
                assert np.array_equal(got.recon[k], want.recon[k]), (i, k)
            assert got.buf == want.buf and got.ranges == want.ranges and got.streams == want.streams and got.stats == want.stats, i
            assert got.rate == [(q, min(b, 0xffffffff), n) for q, b, n in want.rate], i
            led.add(pick(composed), [0, 0, 1, 1], got, i == 2)
        for s in (0, 1):
            (seg,) = led.segments[s]
            one = ec.one_call(seg, 80, 64, 3, 7, rule=rule)
            ec.assert_segment(seg, one, s)
            assert ep.picture_types(one.stream(0)) == ep.expected_types(6, 3)
        assert enc.chain_info(0) == (False, 0)


def test_relay_of_two_lives(torch, hip_lib, libs):
    """a Live at 176x144 with two streams -- one fed the golden pan, one that never decodes anything -- and a Live at 64x48 fed
    an encoded pan, a picture per tick; encode_mosaic_latest composes a 240x144 picture per tick, chained, gop 2.  The planes are
    the restatement's over the oracle's pictures, the oracle decodes the relayed stream, and a frame pointer handed out
    before a tick holds its picture for the two further pictures a ring of pictures_per_tick + 2 = 3 frames promises"""
    from jsmpeg_amd import encode
    from jsmpeg_amd import live as jl
    ticks = 3
    es_a = np.fromfile(GOLDEN + ".m1v", dtype=np.uint8)
    offs = [int(v) for v in np.load(GOLDEN + ".offsets.npy")]
    pics_a, w, h = ei.golden_frames(libs, "enc_pan_176x144", ticks)
    assert (w, h) == (176, 144)
    buf, ranges, streams = ei.sim_encode(PAN[:ticks], 64, 48, qscale=3)
    b0, b1 = streams[0]
    es_b = np.frombuffer(buf, dtype=np.uint8)
    cuts = [o for o, _ in ranges] + [b1]
    pics_b = ep.oracle_frames(libs, es_b[b0:b1])
    assert len(pics_b) == ticks
    cells = [(176, 144, None, 1, 0, 0, 176, 144), (176, 144, None, 1, 176, 96, 64, 48), (64, 48, None, 0, 176, 0, 64, 96)]
    fill = (30, 140, 110)
    composed = [em.compose(cells, [pics_a[t], None, pics_b[t]], 240, 144, fill) for t in range(ticks)]
    with jl.Live(176, 144, 2, pictures_per_tick=1, store_bytes=1 << 18) as la, jl.Live(64, 48, 1, pictures_per_tick=1, store_bytes=1 << 16) as lb, \
            encode.Encoder(240, 144, 1, 1, 1 << 19) as enc:
        enc.set_gop(2, 7)
        enc.set_mosaic(cells_of(cells), fill)
        a0, a1, b = la.open(), la.open(), lb.open()
        sources = [(la, a0), (la, a1), (lb, b)]
        assert la.latest_frames([a0, a1]) == [None, None]
        pieces, held = [], None
        for t in range(ticks):
            la.write(a0, es_a[offs[t]:offs[t + 1]], pts=t / 30.0)
            lb.write(b, es_b[cuts[t]:cuts[t + 1]], pts=t / 30.0)
            assert la.tick(flush=True) == 1 and lb.tick(flush=True) == 1
            if held is not None:                                     # handed out before this tick and the one before
                assert np.array_equal(device_read(held, len(pics_a[0])), pics_a[0]), t
            present = enc.encode_mosaic_latest(sources, qscale=4, end=t + 1 == ticks, chain=True)
            assert present == [True, False, True]
            assert np.array_equal(source_bytes(enc, 0), composed[t]), t
            pieces.append(enc.es(0))
            if t == 0:
                (held,) = la.latest_frames([a0])
                assert held == la.pictures()[0].device_frame
        with pytest.raises(RuntimeError, match="not open"):
            la.latest_frames([7])
        with pytest.raises(ValueError, match="cell 2"):
            enc.encode_mosaic_latest([(la, a0), (la, a1), (la, a0)])
    out = np.frombuffer(b"".join(pieces), dtype=np.uint8)
    assert out.tobytes() == ep.sim_encode_p(composed, 240, 144, 2, 7, qscale=4, end=True).stream(0).tobytes()
    dec = ep.oracle_frames(libs, out)
    assert len(dec) == ticks and ep.picture_types(out) == ep.expected_types(ticks, 2)
    cw, ch = enc_ref.coded(240, 144)
    psnr = ei.psnr(*ei.luma_sse([(d[:cw * ch],) for d in dec], composed, 240, 144))
    print("relay 176x144 + 64x48 -> 240x144, gop 2, q 4: luma PSNR against the composed pictures %.2f dB" % psnr)
    assert np.isfinite(psnr) and psnr > 20.0


def test_pure_enqueue(torch, hip_lib):
    """with a mosaic pass in flight query is callable, a second encode_mosaic is refused and so is set_mosaic"""
    from jsmpeg_amd import encode
    hd = si.case_frames("7_1080p_to_640x360")
    cells = [(1920, 1080, None, 1, 0, 0, 320, 360), (1920, 1080, (480, 0, 960, 1080), 1, 320, 0, 320, 360)]
    dev = Device(torch)
    p0, p1 = dev.ptr(hd[0]), dev.ptr(hd[1])
    with encode.Encoder(640, 360, 8, 1, 8 << 20) as enc:
        enc.set_mosaic(cells_of(cells))
        torch.cuda.synchronize()
        enc.encode_mosaic([[p0, p1], [p1, None]] * 4, qscale=4)
        assert enc.query() in (False, True)
        with pytest.raises(RuntimeError, match="in flight"):
            enc.encode_mosaic([[p0, p1]], qscale=4)
        with pytest.raises(RuntimeError, match="in flight"):
            enc.set_mosaic(cells_of(cells[:1]))
        enc.sync()
        assert enc.query() is True and len(enc.cells) == 2
        want = [em.compose(cells, [hd[0], hd[1]], 640, 360), em.compose(cells, [hd[1], None], 640, 360)]
        for k in range(8):
            assert np.array_equal(source_bytes(enc, k), want[k & 1]), k


def test_overflow(torch, hip_lib):
    """a mosaic call that overflows max_es_bytes fails in sync(); the next call works"""
    from jsmpeg_amd import encode
    noise, smooth = ei.noise_frame(64, 48, 1), si.smooth_frame(64, 48)
    cells = [(64, 48, None, 0, 0, 0, 160, 112), (64, 48, None, 0, 80, 56, 80, 56)]
    want = [em.compose(cells, [f, f], 160, 112) for f in (noise, smooth)]
    need = len(ei.sim_encode(want[:1], 160, 112, qscale=1)[0])
    dev = Device(torch)
    pn, ps = dev.ptr(noise), dev.ptr(smooth)
    with encode.Encoder(160, 112, 1, 1, need - 16) as enc:
        enc.set_mosaic(cells_of(cells))
        enc.encode_mosaic([[pn, pn]], qscale=1)
        with pytest.raises(RuntimeError, match="max_es_bytes"):
            enc.sync()
        for reader in (lambda: enc.es(0), lambda: enc.source(0)):
            with pytest.raises(RuntimeError, match="overflowed"):
                reader()
        enc.encode_mosaic([[ps, ps]], qscale=1)
        enc.sync()
        assert result_of(enc, [0]) == ei.sim_encode(want[1:], 160, 112, qscale=1)


def test_refusals(torch, hip_lib):
    """every refusal launches nothing and leaves the handle working, the layout as it was and the call before readable"""
    from jsmpeg_amd import batch, encode
    cells = [(176, 144, None, 1, 0, 0, 64, 48), (64, 48, None, 1, 32, 24, 32, 24)]
    frames = [[ei.noise_frame(176, 144, 1), ei.noise_frame(64, 48, 2)], [ei.noise_frame(176, 144, 3), None]]
    want = [em.compose(cells, f, 64, 48) for f in frames]
    dev = Device(torch)
    ptrs = dev.pictures(frames)
    with encode.Encoder(64, 48, 2, 2, capacity(want)) as enc:
        with pytest.raises(RuntimeError, match="no mosaic layout"):
            enc.encode_mosaic([[]])
        enc.set_mosaic(cells_of(cells))
        enc.encode_mosaic(ptrs, streams=[0, 1], qscale=3)
        before = result_of(enc, [0, 1])
        assert before == ei.sim_encode(want, 64, 48, streams=[0, 1], qscale=3)

        def unchanged():
            assert enc.query() is True and result_of(enc, [0, 1]) == before and np.array_equal(source_bytes(enc, 1), want[1])
        good = cells[0]
        for bad, why in (([good] * 65, "1 .. 64 cells"), ([good, (64, 48, None, 1, 1, 0, 8, 8)], "mosaic cell 1: cell x and y must be even"),
                         ([(64, 48, None, 1, 0, 2, 8, 47)], "mosaic cell 0: cell rectangle outside"), ([good, (64, 48, None, 1, 0, 0, 0, 8)], "cell 1: cell width and height"),
                         ([good, good, (64, 48, (1, 0, 8, 8), 1, 0, 0, 8, 8)], "cell 2: crop_x and crop_y must be even"),
                         ([(4096, 48, None, 1, 0, 0, 8, 8)], "cell 0: source width and height")):
            with pytest.raises(RuntimeError, match=why):
                enc.set_mosaic(cells_of(bad))
            unchanged()
        assert enc.L.jsmpeg_hip_encoder_set_mosaic(enc.h, None, 2, 0) < 0 and "null cells" in batch.last_error()
        assert enc.L.jsmpeg_hip_encoder_set_mosaic(enc.h, cells_of(cells)[0], 1, 1 << 24) < 0 and "fill" in batch.last_error()
        assert len(enc.cells) == 2
        # the call's own checks, and those of the other entry points
        for pics, kw, why in (([[ptrs[0][0] + 4, ptrs[0][1]]], dict(), "cell 0 of picture 0 is not 16-byte aligned"),
                              ([ptrs[0], [ptrs[1][0], ptrs[0][1] + 8]], dict(), "cell 1 of picture 1 is not 16-byte aligned"),
                              (ptrs, dict(qscale=0), "quantiser_scale"), (ptrs, dict(streams=[1, 0]), "ascend"), (ptrs, dict(streams=[0, 2]), "max_streams"),
                              (ptrs + ptrs[:1], dict(), "max_pictures")):
            with pytest.raises(RuntimeError, match=why):
                enc.encode_mosaic(pics, **kw)
            unchanged()
        for pics in ([ptrs[0][:1]], [ptrs[0] + ptrs[0][:1]], [ptrs[0], []]):
            with pytest.raises(ValueError, match="frame pointers"):
                enc.encode_mosaic(pics)
        unchanged()
        # the layout before is still the one in force; an empty list removes it
        enc.encode_mosaic(ptrs[::-1], streams=[0, 1], qscale=3)
        assert np.array_equal(source_bytes(enc, 0), want[1]) and np.array_equal(source_bytes(enc, 1), want[0])
        enc.set_mosaic([])
        with pytest.raises(ValueError, match="frame pointers"):
            enc.encode_mosaic(ptrs)
        with pytest.raises(RuntimeError, match="no mosaic layout"):
            enc.encode_mosaic([[]])
        assert np.array_equal(source_bytes(enc, 0), want[1])
