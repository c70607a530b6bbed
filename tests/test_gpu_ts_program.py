"""The TS program mux on the device (C ABI part 10, jsmpeg_amd/ts_program.py; the rule: jsmpeg_amd/csrc/ts_prog.h): k_tsp_plan
and k_tsp_write over synthetic device bytes equal the host program mux (jsmpeg_hip_ts_program_mux_host) and the CPU simulator,
ranges, unit ranges and state included; the overflow and the refusals; and the relay loop end to end -- Encoder and Mp2Encoder
chained over two calls, mux_encoders behind each pair on one HIP stream without a sync -- whose programs go back through this
library's two batch decoders.  Bytes are asserted, never times.  Every test here fails without the feature: the module and the
library's jsmpeg_hip_ts_program_* symbols do not exist."""
import ctypes

import numpy as np
import pytest

import enc_p_inputs as ep
import mp2_enc_inputs as minputs
import ts_prog_inputs as tp

pytestmark = pytest.mark.gpu

CANARY = 64


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


def on_device(torch, src):
    """a table's bytes on the device, padded to whole dwords (the kernel reads the aligned dwords around a unit's ends)"""
    host = np.zeros((src.size + 3) // 4 * 4 + 16, np.uint8)
    host[:src.size] = src
    return torch.from_numpy(host).cuda()


class Held:
    pass


def device_mux(torch, case, cap=None):
    """TsProgram.mux over the case into a caller's buffer of `cap` bytes with a canary behind it, the handle set to the state
    the case enters with.  .failed: sync's message or None; .state: all words behind the call; .buf: the buffer on the host"""
    from jsmpeg_amd import ts_program
    cap = case.bound() if cap is None else cap
    v, a = on_device(torch, case.video.src), on_device(torch, case.audio.src)
    out = torch.full((cap + CANARY,), 0xA5, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    r = Held()
    with ts_program.TsProgram(case.cfg(cap)) as prog:
        for s, w in case.state.items():
            prog.set_state(s, w)
        prog.set_output(out.data_ptr(), cap)
        prog.mux(v.data_ptr(), case.video.ranges, case.video.pts, case.video.streams, a.data_ptr(), case.audio.ranges, case.audio.pts, case.audio.streams)
        try:
            prog.sync()
            r.failed = None
        except RuntimeError as e:
            r.failed = str(e)
        r.state = [prog.state(s) for s in range(case.n_streams)]
        host = out.cpu().numpy()
        assert np.all(host[cap:] == 0xA5)
        r.buf = host[:cap]
        if r.failed is None:
            r.total = prog.device_ts()[1]
            r.ranges = {s: prog.stream_range(s) for s in case.present()}
            assert all(prog.stream_range(s) == (0, 0) for s in range(case.n_streams) if s not in case.present())
            r.units = (prog.unit_ranges(tp.VIDEO), prog.unit_ranges(tp.AUDIO))
            whole = prog.ts_all()
            assert sorted(whole) == case.present() and all(whole[s] == bytes(r.buf[b:e]) for s, (b, e) in r.ranges.items())
    return r


def held(torch, case, where):
    """the device's call equals the host program mux and the simulator: bytes, ranges, unit ranges, all five words"""
    got = device_mux(torch, case)
    assert got.failed is None, (where, got.failed)
    tp.assert_equal(case, got, tp.host_mux(case), where)
    sim = tp.sim_mux(case)
    assert (got.total, got.ranges, got.state) == (sim.total, sim.ranges, sim.state), where
    assert got.units == tuple([u[:3] for u in k] for k in sim.units), where
    return got


def test_every_size_1_to_400_as_pcr_units(torch, hip_lib):
    got = held(torch, tp.pcr_sweep_case(), "sweep")
    assert np.all(got.buf[:got.total:188] == 0x47)


def test_edges(torch, hip_lib):
    for b in tp.EDGE_ONE_PACKET:
        held(torch, tp.one_unit_case(b), ("one packet", b))
        held(torch, tp.one_unit_case(b, psi=True, state={0: [15, 15, 15, 15, 0]}), ("one packet, PSI", b))
        held(torch, tp.one_unit_case(b, kind=tp.AUDIO), ("one packet, audio carries the PCR", b))
    for b in tp.EDGE_UNSIZED:
        for pcr in (True, False):
            held(torch, tp.one_unit_case(b, pcr=pcr), ("unsized", b, pcr))
    got = held(torch, tp.counters_at_15_case(), "15")
    assert got.buf[3] & 15 == 15 and got.buf[188 + 3] & 15 == 15 and got.buf[376 + 3] & 15 == 15


def test_random_cases_and_the_empty_call(torch, hip_lib):
    for i, c in enumerate(tp.random_cases(24, seed=31)):
        held(torch, c, ("random", i))
    empty = tp.Case(None, None, 3, {1: [1, 2, 3, 4, 1]})
    got = device_mux(torch, empty, cap=188)
    assert got.failed is None and got.total == 0 and got.units == ([], []) and got.state == [[0] * 5, [1, 2, 3, 4, 1], [0] * 5]
    assert np.all(got.buf == 0xA5)


@pytest.mark.parametrize("n", [255, 256, 257])
def test_chunk_edges_of_the_plan(torch, hip_lib, n):
    held(torch, tp.count_case(n, n, 3), n)


def test_65_streams_and_a_long_stream(torch, hip_lib):
    held(torch, tp.count_case(130, 195, 65), 65)
    held(torch, tp.count_case(600, 580, 2, per_stream=300), "long")


def test_overflow_leaves_the_buffer_and_the_state(torch, hip_lib):
    c = tp.three_stream_program()
    need = tp.sim_mux(c).total
    short = device_mux(torch, c, cap=need - 1)
    assert short.failed and "nothing was written" in short.failed and str(need) in short.failed
    assert np.all(short.buf == 0xA5) and short.state == c.words()
    exact = device_mux(torch, c, cap=need)
    assert exact.failed is None and exact.total == need and bytes(exact.buf) == bytes(tp.host_mux(c).buf)


def test_refusals(torch, hip_lib):
    from jsmpeg_amd import ts_program
    src, ranges = tp.back_to_back([300, 20, 50], 81)
    d = on_device(torch, src)
    out = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    for kw, why in ((dict(video_pid=0x2000), "0x1fff"), (dict(video_pid=0x101), "differ"), (dict(audio_pid=0), "PID 0"),
                    (dict(video_pid=0x1fff, audio_pid=0x1fff), "both kinds"), (dict(max_video_units=0, max_audio_units=0), "max_video_units")):
        with pytest.raises(RuntimeError, match=why):
            ts_program.TsProgram(ts_program.config(2, **{**dict(max_video_units=4, max_audio_units=4, max_ts_bytes=4096), **kw}))
    with ts_program.TsProgram(ts_program.config(2, 4, 4, 4096, audio_pid=0x1fff)) as prog:
        for args, why in (((ranges, [0, 10, 5], [0, 0, 0]), "pts"), ((ranges, [0, 10, 20], [1, 0, 0]), "ascend"), ((ranges, [0, 10, 20], [0, 0, 2]), "max_streams"),
                          ((ranges + ranges, [0] * 6, None), "max_video_units")):
            with pytest.raises(RuntimeError, match=why):
                prog.mux(d.data_ptr(), *args)
        with pytest.raises(RuntimeError, match="absent"):
            prog.mux(None, (), (), None, d.data_ptr(), ranges[:1], [0], None)
        with pytest.raises(RuntimeError, match="aligned"):
            prog.set_output(out.data_ptr() + 2, 1000)
        with pytest.raises(RuntimeError, match="nothing was muxed"):
            prog.device_ts()
        assert prog.query() is True
        prog.mux(d.data_ptr(), ranges, [0, 10, 20], [0, 0, 1])
        for again in (lambda: prog.mux(d.data_ptr(), ranges, [0, 10, 20], [0, 0, 1]), lambda: prog.reset(), lambda: prog.set_output(out.data_ptr(), 4096),
                      lambda: prog.set_state(0, [0] * 5)):
            with pytest.raises(RuntimeError, match="in flight"):
                again()
        prog.sync()
        want = ts_program.program_mux_host(prog.cfg, src, ranges, [0, 10, 20], [0, 0, 1])[0]
        assert prog.device_ts()[1] == len(want) and prog.ts(1) == bytes(want[-(len(prog.ts(1))):]) and prog.timings()["total_ms"] > 0
        prog.reset(0)
        assert prog.state(0) == [0] * 5 and prog.state(1)[4] == 1


# ---------------------------------------------------------------------------------------------------- end to end

def device_bytes(ptr, n):
    from jsmpeg_amd import batch
    out = np.zeros(max(1, n), dtype=np.uint8)
    L = batch.lib()
    L.jsmpeg_hip_device_read.restype = ctypes.c_int
    L.jsmpeg_hip_device_read.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64]
    if n:
        assert L.jsmpeg_hip_device_read(out.ctypes.data, ptr, n) == 0
    return out[:n]


def packets_of(ts):
    """[(pid, payload_unit_start, counter, offset)]"""
    assert len(ts) % 188 == 0
    ts = bytes(ts)                                             # (plain integers: no uint8 arithmetic)
    return [((ts[p + 1] & 0x1f) << 8 | ts[p + 2], bool(ts[p + 1] & 0x40), ts[p + 3] & 15, p) for p in range(0, len(ts), 188)]


def test_relay_loop_end_to_end(torch, hip_lib):
    """two streams of 176x144, 6 pictures with gop 3 in two chained calls of 3, four stereo 44.1 kHz 192 kbit/s frames per
    stream in two chained calls of 2; mux_encoders behind each pair on the null stream with no sync in between"""
    from jsmpeg_amd import batch as jb
    from jsmpeg_amd import encode, mp2, mp2_encode, ts_program
    S44 = minputs.CONFIGS["stereo_44k_192"]
    pictures = [ep.pan_frames(176, 144, 6, (3, -2)), ep.pan_frames(176, 144, 6, (2, 1))]
    pcm = [minputs.pcm("sine", 44100, 4, seed=60), minputs.pcm("noise", 44100, 4, seed=61)]
    es_cap = 64 + 6 * (len(pictures[0][0]) * 4 + 4096)
    cfg = ts_program.config(2, 6, 4, ts_program.program_bound(es_cap, 6, 1 << 14, 4, 2), pcr_lead_90k=9000)
    pieces, es_v, es_a = [b"", b""], [b"", b""], [b"", b""]
    state = [[0] * 5, [0] * 5]
    with encode.Encoder(176, 144, 6, 2, es_cap) as enc, mp2_encode.Mp2Encoder(*S44, 2, 4, 1 << 14) as aenc, ts_program.TsProgram(cfg) as prog:
        enc.set_gop(3, 7)
        for call in range(2):
            frames = [f for s in range(2) for f in pictures[s][3 * call:3 * call + 3]]
            t = torch.from_numpy(np.ascontiguousarray(np.stack(frames))).cuda()
            x = [torch.from_numpy(np.ascontiguousarray(p[2 * call:2 * call + 2], dtype=np.float32)).cuda() for p in pcm]
            torch.cuda.synchronize()
            streams = [0, 0, 0, 1, 1, 1]
            enc.encode([t.data_ptr() + k * t.shape[1] for k in range(6)], streams, 6, end=call == 1, chain=True)
            aenc.encode([v.data_ptr() for v in x], [2, 2], chain=True)
            prog.mux_encoders(enc, aenc)
            prog.sync()
            # the same call on the host over the read-back ES and ranges
            v_dev, v_total = enc.device_es()
            a_dev, a_total = aenc.device_es()
            v_ranges = enc.picture_ranges()
            if call == 1:
                v_ranges = [(o, n + (4 if k in (2, 5) else 0)) for k, (o, n) in enumerate(v_ranges)]       # a stream's last picture runs on over the end code
            v_pts = [3000 * (3 * call + k % 3) for k in range(6)]                                         # 30 / s: 3000 ticks per chain ordinal
            a_ranges, _, a_streams = aenc.ts_units()
            a_pts = [mp2_encode.default_pts(2 * call + k % 2, 44100) for k in range(4)]
            assert a_streams == [0, 0, 1, 1]
            want, ranges, after = ts_program.program_mux_host(cfg, device_bytes(v_dev, v_total + 4), v_ranges, v_pts, streams,
                                                              device_bytes(a_dev, a_total), a_ranges, a_pts, a_streams, state)
            got = prog.ts_all()
            for s in range(2):
                b, e = ranges[s]
                assert prog.stream_range(s) == (b, e) and got[s] == bytes(want[b:e]), (call, s)
                assert prog.state(s) == after[s], (call, s)
                pieces[s] += got[s]
                es_v[s] += enc.es(s)
                es_a[s] += aenc.es(s)
            vu = prog.unit_ranges(ts_program.VIDEO)
            assert [u[2] for u in vu] == [376, 0, 0, 376, 0, 0] and all(u[2] == 0 for u in prog.unit_ranges(ts_program.AUDIO)), call
            state = after
        assert state[0][4] == 1 and any(state[0][:4])
    # the pieces are one valid stream: every PID's counter unbroken, PSI only in front of the I pictures
    for s in range(2):
        ts = np.frombuffer(pieces[s], np.uint8)
        last, pk = {}, packets_of(ts)
        for pid, start, cc, at in pk:
            assert pid in (0, 0x1000, 0x100, 0x101) and (pid not in last or cc == (last[pid] + 1) & 15), (s, at)
            last[pid] = cc
        pats = [i for i, p in enumerate(pk) if p[0] == 0]
        assert len(pats) == 2
        for i in pats:
            assert pk[i + 1][0] == 0x1000 and pk[i + 2][:2] == (0x100, True), (s, i)
            at = pk[i + 2][3]
            skip = 1 + int(ts[at + 4])
            assert bytes(ts[at + 4 + skip + 14:at + 4 + skip + 18]) == tp.KEY, (s, i)               # the PES behind the PCR field begins a sequence header
    # the SAME bytes through both batch decoders: the pictures and the PCM of the plain ES
    with jb.Batch(176, 144, 2, 16, 1 << 20) as a, jb.Batch(176, 144, 2, 16, 1 << 20) as b:
        a.upload_ts([np.frombuffer(p, np.uint8) for p in pieces], 0xE0)
        b.upload([np.frombuffer(e, np.uint8) for e in es_v])
        assert a.decode() == 12 and b.decode() == 12
        assert [a.read_es(s).tobytes()[:len(es_v[s])] for s in range(2)] == es_v
        assert list(a.frame_hashes()) == list(b.frame_hashes())
    with mp2.Mp2Batch(2, 1 << 16) as a, mp2.Mp2Batch(2, 1 << 16) as b:
        a.upload_ts([np.frombuffer(p, np.uint8) for p in pieces], 0xC0)
        b.upload([np.frombuffer(e, np.uint8) for e in es_a])
        assert a.decode() == 8 and b.decode() == 8
        for s in range(2):
            assert a.read_bytes(s).tobytes() == es_a[s]
            assert np.asarray(a.read_pcm(s)).tobytes() == np.asarray(b.read_pcm(s)).tobytes(), s


def test_es_overflow_of_the_video_encoder_is_a_refusal(torch, hip_lib):
    """a max_es_bytes too small for the picture: the encoder's call overflows, the program behind it has nothing to mux --
    sync fails with a message, nothing is written, the state stays"""
    from jsmpeg_amd import encode, ts_program
    frames = ep.pan_frames(64, 48, 1, (1, 1))
    t = torch.from_numpy(np.ascontiguousarray(np.stack(frames))).cuda()
    out = torch.full((4096 + CANARY,), 0xA5, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    with encode.Encoder(64, 48, 1, 1, 64) as enc, ts_program.TsProgram(ts_program.config(1, 1, 1, 4096, audio_pid=0x1fff)) as prog:
        prog.set_state(0, [3, 4, 5, 6, 1])
        prog.set_output(out.data_ptr(), 4096)
        enc.encode([t.data_ptr()], None, 2)
        prog.mux_encoders(enc, None)
        with pytest.raises(RuntimeError, match="max_es_bytes"):
            prog.sync()
        for reader in (lambda: prog.device_ts(), lambda: prog.ts(0), lambda: prog.stream_range(0), lambda: prog.unit_ranges(0)):
            with pytest.raises(RuntimeError, match="max_es_bytes"):
                reader()
        with pytest.raises(RuntimeError, match="max_es_bytes"):
            enc.sync()
        assert prog.state(0) == [3, 4, 5, 6, 1]
        assert bool((out == 0xA5).all())
