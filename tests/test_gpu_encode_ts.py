"""MPEG-TS on the device behind the encoder's pass (jsmpeg_hip_encoder_set_ts, Encoder.set_ts; the rule:
jsmpeg_amd/csrc/enc_ts.h): every stream's packets equal the host mux (jsmpeg_hip_ts_mux_host) over the same call's picture
ranges, the continuity counters go on from call to call per stream number, the ES buffer is what it is without TS, and the
packets go back through this library's demuxers to the pictures the encoder reconstructed.  Bytes are asserted, never times."""
import ctypes

import numpy as np
import pytest

import enc_inputs as ei
import enc_p_inputs as ep
import enc_ts_inputs as et

pytestmark = pytest.mark.gpu

PAN = ep.pan_frames(64, 48, 9, (3, -2))
PAN_B = ep.pan_frames(64, 48, 9, (2, 1))
PAN_C = ep.pan_frames(64, 48, 9, (-1, 2))


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


def on_device(torch, frames):
    t = torch.from_numpy(np.ascontiguousarray(np.stack(frames))).cuda()
    return t, [t.data_ptr() + k * t.shape[1] for k in range(t.shape[0])]


def whole_es(enc):
    """the call's ES buffer on the host"""
    from jsmpeg_amd import batch
    p, total = enc.device_es()
    out = np.zeros(total + 256, dtype=np.uint8)
    L = batch.lib()
    L.jsmpeg_hip_device_read.restype = ctypes.c_int
    L.jsmpeg_hip_device_read.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64]
    assert L.jsmpeg_hip_device_read(out.ctypes.data, p, total + 256) == 0
    assert np.all(out[total:] == 0xff)
    return out[:total]


def recon_bytes(enc, k):
    return np.concatenate([p.ravel() for p in enc.recon(k)])


def capacity(frames):
    return 64 + len(frames) * (len(frames[0]) * 4 + 4096)


def units_of(enc, streams, end):
    """{stream: [(offset, bytes)]} of the last call: the picture ranges, a stream's last one run on over the end code"""
    out = {}
    for k, (r, s) in enumerate(zip(enc.picture_ranges(), streams)):
        out.setdefault(s, []).append(r)
    for s, rs in out.items():
        if end:
            rs[-1] = (rs[-1][0], rs[-1][1] + 4)
        assert rs[0][0] == enc.stream_range(s)[0] and rs[-1][0] + rs[-1][1] == enc.stream_range(s)[1]      # every byte of the stream
    return out


def check_call(enc, streams, pts, cc_in, end, where):
    """every stream's TS of the last call equals the host mux of its piece from counter cc_in[s]; the picture ranges tile the
    stream ranges; ts_all is the same bytes in one copy.  Returns {stream: (ts bytes, counter out)}"""
    es = whole_es(enc)
    units, pr, out, at = units_of(enc, streams, end), enc.ts_picture_ranges(), {}, 0
    whole, ranges = enc.ts_all()
    assert sorted(ranges) == sorted(units) and len(whole) == enc.device_ts()[1]
    for s in sorted(units):
        idx = [k for k, v in enumerate(streams) if v == s]
        want, cc = et.host_mux(es, units[s], [pts[k] for k in idx], cc_in.get(s, 0))
        b, e, nxt = enc.ts_range(s)
        assert b % 16 == 0 and 0 <= b - at < 16 and ranges[s] == (b, e), (where, s)
        got = enc.ts(s)
        assert got == want and nxt == cc and bytes(whole[b:e]) == want, (where, s)
        pos = b
        for k in idx:
            assert pr[k][0] == pos and pr[k][1] % 188 == 0 and pr[k][1] > 0, (where, k)
            pos += pr[k][1]
        assert pos == e, (where, s)
        out[s], at = (got, cc), e
    assert at == len(whole)
    return out


def test_gop_1_three_streams_with_end(torch, hip_lib):
    """(fails without the feature: jsmpeg_hip_encoder_set_ts is missing)"""
    from jsmpeg_amd import encode
    frames, streams = PAN[:8], [0, 0, 0, 2, 5, 5, 5, 5]
    t, ptrs = on_device(torch, frames)
    with encode.Encoder(64, 48, 8, 6, capacity(frames)) as enc, encode.Encoder(64, 48, 8, 6, capacity(frames)) as plain:
        enc.set_ts(encode.ts_bound(capacity(frames), 8, 3))
        enc.encode(ptrs, streams, 6, end=True)
        plain.encode(ptrs, streams, 6, end=True)
        assert np.array_equal(whole_es(enc), whole_es(plain))            # the ES buffer, byte for byte the call's with TS off
        assert enc.picture_ranges() == plain.picture_ranges() and [enc.stream_range(s) for s in (0, 2, 5)] == [plain.stream_range(s) for s in (0, 2, 5)]
        pts = [3000 * o for o in (0, 1, 2, 0, 0, 1, 2, 3)]                # the default rule at 30 / s: the ordinal in the stream
        out = check_call(enc, streams, pts, {}, True, "gop 1")
        assert [out[s][0][3] & 15 for s in (0, 2, 5)] == [0, 0, 0]
        assert enc.ts_range(1) == (0, 0, 0) and enc.timings()["write_ms"] > 0
        with pytest.raises(RuntimeError, match="TS is off"):
            plain.ts(0)


def test_chained_relay_with_rate_control(torch, hip_lib):
    """gop 4, search 7, rate control, one picture per stream per call, 9 calls with explicit pts; stream 1 joins at call 2,
    stream 3 leaves at call 5"""
    from jsmpeg_amd import batch as jb
    from jsmpeg_amd import encode
    from jsmpeg_amd import live as jl
    own = {0: PAN, 1: PAN_B, 3: PAN_C}
    present = lambda i: [s for s in (0, 1, 3) if (s != 1 or i >= 2) and (s != 3 or i < 5)]
    pieces, recons, stamps, cc = {0: [], 1: [], 3: []}, {0: [], 1: [], 3: []}, {0: [], 1: [], 3: []}, {}
    with encode.Encoder(64, 48, 3, 4, capacity(PAN[:3])) as enc, jl.Live(64, 48, 4, pictures_per_tick=1, store_bytes=1 << 18) as lv:
        enc.set_gop(4, 7)
        enc.set_rate(400, 1, 31, 4)
        enc.set_ts(encode.ts_bound(capacity(PAN[:3]), 3, 3))
        ids = {s: lv.open() for s in (0, 1, 3)}
        for i in range(9):
            streams = present(i)
            frames = [own[s][len(pieces[s])] for s in streams]
            secs = [i / 25.0 + 0.001 * s for s in streams]
            t, ptrs = on_device(torch, frames)
            enc.encode(ptrs, streams, 8, end=i == 8, chain=True, pts=secs)
            out = check_call(enc, streams, [int(round(v * 90000.0)) for v in secs], cc, i == 8, i)
            for k, s in enumerate(streams):
                pieces[s].append(out[s][0])
                cc[s] = out[s][1]
                recons[s].append(recon_bytes(enc, k))
                stamps[s].append(int(round(secs[k] * 90000.0)) / 90000.0)
                lv.write_ts(ids[s], np.frombuffer(out[s][0], np.uint8))
            assert lv.tick(flush=True) == len(streams), i
            shown = {p.stream: np.concatenate(lv.read_frame(j)) for j, p in enumerate(lv.pictures())}
            for k, s in enumerate(streams):
                assert np.array_equal(shown[ids[s]], recons[s][-1]), (i, s)
        assert [len(pieces[s]) for s in (0, 1, 3)] == [9, 7, 5]
        assert any(c for c in cc.values())                                # the counters moved
    with jb.Batch(64, 48, 3, 32, 1 << 20) as dst:
        dst.upload_ts([np.frombuffer(b"".join(pieces[s]), np.uint8) for s in (0, 1, 3)])
        assert dst.decode() == 21
        infos, at = dst.pictures(), {0: 0, 1: 0, 2: 0}
        for p, info in enumerate(infos):
            s = (0, 1, 3)[info.stream]
            assert info.decoded and np.array_equal(np.concatenate(dst.read_frame(p)), recons[s][at[info.stream]]), (p, s)
            at[info.stream] += 1
        for n, s in enumerate((0, 1, 3)):
            assert [w[0] for w in dst.ts_writes(n)] == stamps[s], s


def test_a_picture_above_65527_bytes(torch, hip_lib):
    from jsmpeg_amd import batch as jb
    from jsmpeg_amd import encode
    frames = [ei.noise_frame(320, 240)]
    t, ptrs = on_device(torch, frames)
    with encode.Encoder(320, 240, 1, 1, capacity(frames)) as enc, jb.Batch(320, 240, 1, 4, 1 << 20) as dst:
        enc.set_ts(encode.ts_bound(capacity(frames), 1, 1))
        enc.encode(ptrs, None, 1, end=True, pts=[1.5])
        (off, n), = enc.picture_ranges()
        assert n > 65527
        out = check_call(enc, [0], [135000], {}, True, "big")
        ts = np.frombuffer(out[0][0], np.uint8)
        assert bytes(ts[4:8]) == b"\x00\x00\x01\xe0" and ts[8] == 0 and ts[9] == 0       # PES_packet_length 0
        dst.upload_ts([ts])
        assert dst.ts_writes(0) == [(1.5, 0, n + 4)]
        assert np.array_equal(dst.read_es(0)[:n + 4], whole_es(enc)[off:off + n + 4])


def test_overflow_leaves_the_counters(torch, hip_lib):
    from jsmpeg_amd import encode
    t, ptrs = on_device(torch, PAN[:4])
    with encode.Encoder(64, 48, 3, 2, capacity(PAN[:3])) as enc:
        enc.set_gop(4, 0)
        enc.encode(ptrs[:1], [1], 2, end=False, chain=True)
        need = enc.picture_ranges()[0][1]
        room = encode.ts_bound(need, 1, 1)
        enc.chain_reset()
        enc.set_ts(room)
        enc.encode(ptrs[:1], [1], 2, end=False, chain=True)
        first = check_call(enc, [1], [0], {}, False, "fits")
        assert first[1][1] == (len(first[1][0]) // 188) % 16 and enc.chain_info(1) == (True, 1)
        enc.chain_reset()
        enc.encode(ptrs[:3], [0, 1, 1], 2, end=False, chain=True)         # three I-sized streams' worth: the ES fits, the TS does not
        with pytest.raises(RuntimeError, match="max_ts_bytes"):
            enc.sync()
        for reader in (lambda: enc.ts(1), lambda: enc.ts_all(), lambda: enc.ts_range(1), lambda: enc.es(1), lambda: enc.device_ts()):
            with pytest.raises(RuntimeError, match="overflowed"):
                reader()
        assert enc.chain_info(0) == (False, 0) and enc.chain_info(1) == (False, 0)
        enc.encode(ptrs[:1], [1], 2, end=False, chain=True)               # set_ts is NOT called again
        check_call(enc, [1], [0], {1: first[1][1]}, False, "after the overflow")
        assert enc.ts_range(0) == (0, 0, 0)                               # stream 0's counter is where the failed call found it too


def test_refusals_and_the_off_state(torch, hip_lib):
    from jsmpeg_amd import batch, encode
    t, ptrs = on_device(torch, PAN[:2])
    with encode.Encoder(64, 48, 2, 2, capacity(PAN[:2])) as enc:
        enc.encode(ptrs, [0, 1], 5)
        before = whole_es(enc).tobytes()
        for reader in (lambda: enc.ts(0), lambda: enc.ts_all(), lambda: enc.ts_range(0), lambda: enc.ts_picture_ranges(), lambda: enc.device_ts()):
            with pytest.raises(RuntimeError, match="TS is off"):
                reader()
        p90 = np.zeros(2, np.uint64)
        assert enc.L.jsmpeg_hip_encoder_ts_pts(enc.h, p90.ctypes.data, 2) < 0 and "TS is off" in batch.last_error()
        enc.encode(ptrs, [0, 1], 5)
        with pytest.raises(RuntimeError, match="in flight"):
            enc.set_ts(1 << 16)
        enc.sync()
        for sid, pid, why in ((0xE0, 0x2000, "pid"), (0x100, 0x100, "stream id")):
            with pytest.raises(RuntimeError, match=why):
                enc.set_ts(1 << 16, sid, pid)
        enc.set_ts(1 << 16, 0xE1, 0x1fff)
        with pytest.raises(RuntimeError, match="switched on after"):
            enc.ts(0)
        with pytest.raises(RuntimeError, match="3 pts values"):
            enc.encode(ptrs, [0, 1], 5, pts=[0.0, 0.1, 0.2])
        assert enc.query() is True and whole_es(enc).tobytes() == before  # nothing was launched
        enc.encode(ptrs, [0, 1], 5)                                       # the next call is not bound by the refused count
        es = whole_es(enc)
        for s in (0, 1):
            want, cc = et.host_mux(es, [enc.picture_ranges()[s][:1] + (enc.picture_ranges()[s][1] + 4,)], [0], 0, 0xE1, 0x1fff)
            assert enc.ts(s) == want and enc.ts_range(s)[2] == cc
        enc.encode([], None, 5)
        assert enc.device_ts()[1] == 0 and enc.ts(0) == b"" and enc.ts_picture_ranges() == [] and len(enc.ts_all()[0]) == 0
        enc.set_ts(0)
        with pytest.raises(RuntimeError, match="TS is off"):
            enc.ts(0)


def test_pure_enqueue(torch, hip_lib):
    """with a pass that ends in the mux in flight query is callable and a second call is refused"""
    from jsmpeg_amd import encode
    frames = [ei.noise_frame(640, 360, 1), ei.noise_frame(640, 360, 2)] * 4
    t, ptrs = on_device(torch, frames[:2])
    torch.cuda.synchronize()
    with encode.Encoder(640, 360, 8, 4, 8 << 20) as enc:
        enc.set_ts(encode.ts_bound(8 << 20, 8, 4))
        streams = [0, 0, 1, 1, 1, 3, 3, 3]
        enc.encode([ptrs[0], ptrs[1]] * 4, streams, 4)
        assert enc.query() in (False, True)
        with pytest.raises(RuntimeError, match="in flight"):
            enc.encode(ptrs, None, 4)
        with pytest.raises(RuntimeError, match="in flight"):
            enc._ok(enc.L.jsmpeg_hip_encoder_ts_pts(enc.h, None, 0))
        enc.sync()
        assert enc.query() is True and enc.L.jsmpeg_hip_encoder_sync(enc.h) == 0
        check_call(enc, streams, [3000 * o for o in (0, 1, 0, 1, 2, 0, 1, 2)], {}, True, "in flight")
