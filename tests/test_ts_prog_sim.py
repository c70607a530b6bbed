"""The TS program mux's rule (jsmpeg_amd/csrc/ts_prog.h, C ABI part 10) without a GPU: the simulator of the device plan
(tests/sim/sim_ts_prog.cpp: every unit's rank by binary search, the per-lane steps around prefix sums, then every output dword
on its own, in reverse order) against jsmpeg_hip_ts_program_mux_host, a serial walk that shares nothing with it, byte for byte
and with all five state words per stream; both against jsmpeg_hip_ts_mux_host where the program reduces to it; the order, the
PSI tables through a parser of the test's own, two calls against one, the reference's demuxer over a three-stream program, the
plan's wave and chunk edges, and the simulator's driver under the sanitizers."""
import ctypes
import hashlib
import json
import os
import subprocess
import tempfile

import numpy as np
import pytest

import enc_inputs as ei
import enc_ts_inputs as et
import ts_prog_inputs as tp
from conftest import ROOT, have_reference

MASK = tp.PTS_MASK


# ---------------------------------------------------------------------------------------------------- reduction

def reduces(c, kind, where, aligned=False):
    """PSI off, PCR off, one table empty: per stream jsmpeg_hip_ts_mux_host's bytes and counter, from both"""
    case, pts = tp.from_enc_ts(c, kind)
    sid, pid, word = (0xE0, 0x100, 2) if kind == tp.VIDEO else (0xC0, 0x101, 3)
    got, host = tp.sim_mux(case, aligned=aligned), tp.host_mux(case)
    for s in c.present():
        idx = c.of(s)
        want, cc = et.host_mux(c.es, [c.ranges[i] for i in idx], [pts[i] for i in idx], c.cc[s], sid, pid)
        for r, who in ((got, "sim"), (host, "host")):
            b, e = r.ranges[s]
            assert bytes(r.buf[b:e]) == want, (where, who, s)
            assert r.state[s][word] == cc and r.state[s][:2] == [0, 0] and r.state[s][5 - word] == 0, (where, who, s)
    tp.assert_equal(case, got, host, where)


@pytest.mark.parametrize("kind", [tp.VIDEO, tp.AUDIO], ids=["video", "audio_0xC0"])
def test_one_table_without_psi_and_pcr_is_the_part_8_mux(hip_lib, kind):
    for seed, cc in ((1, 11), (4, 15)):
        c = et.sizes_case(seed)
        c.cc[0] = cc
        reduces(c, kind, ("sizes", seed))
        reduces(c, kind, ("sizes", seed), aligned=True)
    reduces(et.sweep_case(), kind, "sweep")
    reduces(et.sweep_case(), kind, "sweep", aligned=True)
    reduces(et.three_stream_case(), kind, "three streams")
    for i, c in enumerate(et.random_cases()):
        reduces(c, kind, ("random", i), aligned=bool(i & 1))


def test_geometry_reduces_to_enc_ts_at_lead0_0():
    for b in list(range(1, 401)) + [65527, 65528, 184 * 400 - 14, 184 * 400 - 13, 100000]:
        assert tp.sim().sim_tsp_packets(b, 0) == et.sim().sim_ts_packets(b), b


# ---------------------------------------------------------------------------------------------------- simulator == host program mux

@pytest.mark.parametrize("aligned", [False, True], ids=["bytes", "aligned_dwords"])
def test_sim_equals_host_on_every_size_1_to_400_as_pcr_units(hip_lib, aligned):
    c = tp.pcr_sweep_case()
    assert [b for _, b in c.video.ranges] == list(range(1, 401)) and c.pcr and c.psi
    got = tp.sim_equals_host(c, "sweep", aligned)
    for (at, nbytes, psi, cc), (_, b) in zip(got.units[0], c.video.ranges):
        assert nbytes - psi == 188 * ((14 + b + 8 + 183) // 184), b            # sized units: lead = 8


def test_sim_equals_host_on_pcr_units_one_by_one(hip_lib):
    for b in range(1, 401):
        c = tp.one_unit_case(b)
        got = tp.sim_equals_host(c, ("one", b), aligned=bool(b & 1))
        assert got.total == 188 * ((14 + b + 8 + 183) // 184), b
        first = got.buf[:188]
        base = (100 - 9000) % (1 << 33)                                          # pts < pcr_lead wraps modulo 2^33
        assert first[3] & 0x20 and first[4] >= 7 and first[5] == 0x10, b
        assert list(first[6:12]) == [(base >> 25) & 255, (base >> 17) & 255, (base >> 9) & 255, (base >> 1) & 255, ((base & 1) << 7) | 0x7e, 0], b


def test_the_one_packet_edge(hip_lib):
    """14 + bytes + 8 around 184: 161 leaves a stuffing byte behind the PCR, 162 fits exactly, 163 needs a second packet"""
    want = {161: (1, 8), 162: (1, 7), 163: (2, 7)}
    for b in tp.EDGE_ONE_PACKET:
        for psi in (False, True):
            got = tp.sim_equals_host(tp.one_unit_case(b, psi=psi), ("edge", b, psi))
            at = 376 if psi else 0
            assert got.total == at + 188 * want[b][0] and got.buf[at + 4] == want[b][1], b
            if b == 161:
                assert got.buf[at + 12] == 0xff
        tp.sim_equals_host(tp.one_unit_case(b, kind=tp.AUDIO), ("edge, audio carries the PCR", b))


def test_unsized_units(hip_lib):
    """bytes > 65527 (PES_packet_length 0): a full last packet gets a stuffing byte in the first one -- behind the PCR when
    (14 + bytes + 8) % 184 == 0, and not at all when only (14 + bytes) % 184 == 0 (the PCR's 8 bytes moved the end)"""
    pcr_full, plain_full = tp.EDGE_UNSIZED
    assert (14 + pcr_full + 8) % 184 == 0 and (14 + plain_full) % 184 == 0 and min(tp.EDGE_UNSIZED) > 65527
    for b in tp.EDGE_UNSIZED:
        for pcr in (True, False):
            got = tp.sim_equals_host(tp.one_unit_case(b, pcr=pcr), ("unsized", b, pcr), aligned=True)
            lead = (8 if pcr else 0) + (1 if (14 + b + (8 if pcr else 0)) % 184 == 0 else 0)
            assert got.total == 188 * ((14 + b + lead + 183) // 184), (b, pcr)
            assert (got.buf[4] + 1 if got.buf[3] & 0x20 else 0) == lead, (b, pcr)
            last = got.buf[got.total - 188:got.total]
            assert last[3] & 0x20, (b, pcr)                                   # the last packet always carries a field: ts.js ends the PES there


def test_counters_entering_at_15(hip_lib):
    c = tp.counters_at_15_case()
    got = tp.sim_equals_host(c, "15")
    assert got.buf[3] & 15 == 15 and got.buf[188 + 3] & 15 == 15 and got.buf[376 + 3] & 15 == 15     # PAT, PMT, the first video packet
    a_at = got.units[1][0][0]
    assert got.buf[a_at + 3] & 15 == 15 and got.buf[a_at + 188 + 3] & 15 == 0
    assert got.state[0][4] == 1


def test_sim_equals_host_on_random_cases(hip_lib):
    cases = tp.random_cases()
    assert len(cases) == 300 and any(len(c.present()) == 5 for c in cases)
    assert any(c.video_pid == 0x1fff for c in cases) and any(c.audio_pid == 0x1fff for c in cases)
    assert any(c.psi and c.pcr for c in cases) and any(not c.psi and not c.pcr for c in cases)
    only = [set(c.video.streams) ^ set(c.audio.streams) for c in cases if len(c.video) and len(c.audio)]
    assert any(only), "no stream with one kind only beside streams with both"
    assert any(b > 65527 for c in cases for _, b in c.video.ranges + c.audio.ranges)
    ties = 0
    for i, c in enumerate(cases):
        tp.sim_equals_host(c, ("random", i), aligned=bool(i & 1))
        ties += sum(1 for s in c.present() if len({p for k, j in c.merged(s) for p in [c.tables()[k].pts[j]]}) < len(c.merged(s)))
    assert ties > 100


# ---------------------------------------------------------------------------------------------------- order

def test_order_tiling_and_counters(hip_lib):
    cases = [tp.pcr_sweep_case(), tp.counters_at_15_case(), tp.three_stream_program()] + tp.random_cases(60, seed=99)
    for i, c in enumerate(cases):
        got = tp.sim_mux(c)
        v, a = c.video, c.audio
        vs, vp = np.ascontiguousarray(v.streams, np.uint32), np.ascontiguousarray(v.pts, np.uint64)
        as_, ap = np.ascontiguousarray(a.streams, np.uint32), np.ascontiguousarray(a.pts, np.uint64)
        ranks = [tp.sim().sim_tsp_rank(vs.ctypes.data, vp.ctypes.data, len(v), as_.ctypes.data, ap.ctypes.data, len(a), k, j)
                 for k, t in enumerate(c.tables()) for j in range(len(t))]
        order = [u for s in c.present() for u in c.merged(s)]                   # a stable sort by (pts, kind), stream after stream
        flat = [(0, j) for j in range(len(v))] + [(1, j) for j in range(len(a))]
        assert sorted(ranks) == list(range(len(flat))) and [flat[ranks.index(m)] for m in range(len(flat))] == order, i
        for s in c.present():
            pos, cc = got.ranges[s][0], list(c.words()[s])
            for k, j in c.merged(s):
                at, nbytes, psi, word = got.units[k][j]
                assert at == pos, (i, s, k, j)
                if psi:
                    assert psi == 376 and (word >> 4) & 15 == cc[0] and (word >> 8) & 15 == cc[1], (i, s, k, j)
                    cc[0], cc[1] = (cc[0] + 1) & 15, (cc[1] + 1) & 15
                packets = tp.sim().sim_tsp_packets(c.tables()[k].ranges[j][1], c.lead0(k))
                assert nbytes == psi + 188 * packets and word & 15 == cc[2 + k], (i, s, k, j)
                cc[2 + k] = (cc[2 + k] + packets) & 15
                pos += nbytes
            assert pos == got.ranges[s][1] and cc[:4] == got.state[s][:4] and got.state[s][4] == 1, (i, s)
        for s in range(c.n_streams):
            if s not in c.present():
                assert got.state[s] == c.words()[s], (i, s)


def test_pcr_wraps_below_the_lead(hip_lib):
    for pts, lead in ((100, 9000), (0, 1), ((1 << 33) + 5, 10), (MASK, 0)):
        c = tp.one_unit_case(300, pts=pts)
        c.pcr_lead = lead
        got = tp.sim_equals_host(c, ("wrap", pts))
        p = got.buf[:188]
        base = (int(p[6]) << 25) | (int(p[7]) << 17) | (int(p[8]) << 9) | (int(p[9]) << 1) | (int(p[10]) >> 7)
        assert base == (pts - lead) % (1 << 33) and p[10] & 0x7f == 0x7e and p[11] == 0, pts


# ---------------------------------------------------------------------------------------------------- PSI

def crc_residue(section):
    c = 0xffffffff
    for b in section:
        c ^= b << 24
        for _ in range(8):
            c = ((c << 1) ^ 0x04C11DB7) & 0xffffffff if c & 0x80000000 else (c << 1) & 0xffffffff
    return c


def parse_psi(packet, pid):
    """the test's own parser of a PAT / PMT packet -> the section's fields"""
    assert len(packet) == 188 and packet[0] == 0x47 and packet[1] & 0x40 and ((packet[1] & 0x1f) << 8 | packet[2]) == pid
    assert packet[3] & 0xf0 == 0x10 and packet[4] == 0                              # payload only; pointer_field 0
    sec = packet[5:]
    assert sec[1] & 0xb0 == 0xb0 and sec[1] & 0x40 == 0                             # section syntax, '0', reserved
    n = (sec[1] & 0x0f) << 8 | sec[2]
    assert crc_residue(sec[:3 + n]) == 0 and all(b == 0xff for b in sec[3 + n:])
    assert sec[5] == 0xc1 and sec[6] == 0 and sec[7] == 0                           # version 0, current; section 0 of 0
    return dict(table=sec[0], ident=sec[3] << 8 | sec[4], body=bytes(sec[8:3 + n - 4]))


def test_psi_tables(hip_lib):
    from jsmpeg_amd import ts_program
    for video_pid, audio_pid in ((0x100, 0x101), (0x1fff, 0x44), (0x31, 0x1fff), (0x1ffe, 0x10)):
        cfg = ts_program.config(video_pid=video_pid, audio_pid=audio_pid, pmt_pid=0x1abc, program_number=0x1234, transport_stream_id=0xbeef)
        pat, pmt = ts_program.psi_packets(cfg)
        a = parse_psi(pat, 0)
        assert a["table"] == 0 and a["ident"] == 0xbeef and a["body"] == bytes([0x12, 0x34, 0xe0 | 0x1a, 0xbc])
        m = parse_psi(pmt, 0x1abc)
        body = m["body"]
        assert m["table"] == 2 and m["ident"] == 0x1234
        carrier = video_pid if video_pid != 0x1fff else audio_pid
        assert (body[0] & 0x1f) << 8 | body[1] == carrier and body[0] & 0xe0 == 0xe0 and body[2:4] == bytes([0xf0, 0])
        es = [(body[i], (body[i + 1] & 0x1f) << 8 | body[i + 2], (body[i + 3] & 0x0f) << 8 | body[i + 4]) for i in range(4, len(body), 5)]
        assert es == [(t, p, 0) for t, p in ((0x01, video_pid), (0x03, audio_pid)) if p != 0x1fff]
    c = tp.counters_at_15_case()
    c.program_number, c.transport_stream_id, c.pmt_pid = 77, 1001, 0x200
    got = tp.sim_equals_host(c, "psi in place")
    pat, pmt = ts_program.psi_packets(c.cfg())
    assert bytes(got.buf[:3]) + bytes(got.buf[4:188]) == pat[:3] + pat[4:] and bytes(got.buf[188:191]) + bytes(got.buf[192:376]) == pmt[:3] + pmt[4:]


def test_psi_goes_in_front_of_unstarted_streams_and_key_pictures_once(hip_lib):
    seen = dict(both=0, first=0, key=0, none=0)
    for i, c in enumerate([tp.counters_at_15_case(), tp.pcr_sweep_case(), tp.three_stream_program()] + tp.random_cases(120, seed=123)):
        got = tp.sim_mux(c)
        for s in c.present():
            for o, (k, j) in enumerate(c.merged(s)):
                first = o == 0 and not c.words()[s][4]
                key = k == tp.VIDEO and c.is_key(j)
                want = 376 if c.psi and (first or key) else 0
                assert got.units[k][j][2] == want, (i, s, k, j)
                at = got.units[k][j][0]
                pids = [(int(got.buf[at + 188 * p + 1]) & 0x1f) << 8 | int(got.buf[at + 188 * p + 2]) for p in range(3)] if want else []
                assert pids == ([0, c.pmt_pid, (c.video_pid, c.audio_pid)[k]] if want else []), (i, s, k, j)
                if c.psi:
                    seen["both" if first and key else "first" if first else "key" if key else "none"] += 1
        # no PAT anywhere else
        n_pat = sum(1 for s in c.present() for p in range(got.ranges[s][0], got.ranges[s][1], 188) if got.buf[p + 1] & 0x1f == 0 and got.buf[p + 2] == 0)
        assert n_pat == sum(1 for k in (0, 1) for u in got.units[k] if u[2]), i
    assert min(seen.values()) > 0, seen


def test_started_carries_to_the_next_call(hip_lib):
    src, ranges = tp.back_to_back([300, 300], 61)
    a_src, a_ranges = tp.back_to_back([200], 62)
    c = tp.Case(tp.Table(src, ranges, [0, 3000]), tp.Table(a_src, a_ranges, [1000]), 2, psi=True)
    one = tp.sim_equals_host(c, "first call")
    assert [u[2] for u in one.units[0]] == [376, 0] and one.units[1][0][2] == 0 and one.state[0][4] == 1 and one.state[1][4] == 0
    again = c.with_tables(c.video, c.audio, {0: one.state[0]})
    two = tp.sim_equals_host(again, "second call")
    assert [u[2] for u in two.units[0]] == [0, 0] and two.total == one.total - 376
    assert two.state[0][:2] == one.state[0][:2]                                     # no PSI: its counters rest


# ---------------------------------------------------------------------------------------------------- two calls, overflow

def test_two_calls_equal_one(hip_lib):
    cases = [(tp.pcr_sweep_case(), 600000), (tp.counters_at_15_case(), 6000), (tp.three_stream_program(), 90000 + 4000)]
    cases += [(c, 3000) for c in tp.random_cases(40, seed=7)]
    for i, (c, T) in enumerate(cases):
        one = tp.sim_mux(c)
        first, rest = c.split(T)
        a = tp.sim_mux(first)
        b = tp.sim_mux(rest.with_tables(rest.video, rest.audio, {s: a.state[s] for s in range(c.n_streams)}))
        tp.assert_equal(first, a, tp.host_mux(first), (i, "first"))
        assert b.state == one.state, i
        for s in c.present():
            (ab, ae), (bb, be), (ob, oe) = a.ranges.get(s, (0, 0)), b.ranges.get(s, (0, 0)), one.ranges[s]
            assert bytes(a.buf[ab:ae]) + bytes(b.buf[bb:be]) == bytes(one.buf[ob:oe]), (i, s)


def test_overflow_writes_nothing_and_keeps_the_state(hip_lib):
    for i, c in enumerate([tp.pcr_sweep_case(), tp.counters_at_15_case(), tp.three_stream_program()] + tp.random_cases(40, seed=8)):
        got = tp.sim_mux(c)
        need = got.total
        short = tp.sim_mux(c, cap=need - 1)
        assert short.total == -1 and short.state == c.words() and np.all(short.buf == 0xA5), i
        with pytest.raises(RuntimeError, match="do not fit"):
            tp.host_mux(c, cap=need - 1)
        exact = tp.sim_mux(c, cap=need)
        assert exact.total == need and bytes(exact.buf) == bytes(got.buf[:need]) and exact.state == got.state, i
        assert tp.host_mux(c, cap=need).total == need


def test_host_mux_refuses_what_the_rule_excludes(hip_lib):
    src, ranges = tp.back_to_back([100, 100, 100], 71)
    good = tp.Case(tp.Table(src, ranges, [0, 10, 20], [0, 0, 1]), None, 2)
    assert tp.host_mux(good).total == ((2 * 188 + 15) & ~15) + 188                  # stream 1 begins at a multiple of 16
    for bad, why in ((tp.Case(tp.Table(src, ranges, [0, 10, 5], [0, 0, 0]), None, 2), "pts"),
                     (tp.Case(tp.Table(src, ranges, [0, 10, 20], [1, 0, 0]), None, 2), "ascend"),
                     (tp.Case(tp.Table(src, ranges, [0, 10, 20], [0, 0, 2]), None, 2), "max_streams"),
                     (tp.Case(tp.Table(src, ranges, [0, 10, 20]), None, 1, video_pid=0x1fff), "absent"),
                     (tp.Case(tp.Table(src, ranges, [0, 10, 20]), None, 1, video_pid=0x101), "differ"),
                     (tp.Case(tp.Table(src, ranges, [0, 10, 20]), None, 1, pmt_pid=0), "PID 0"),
                     (tp.Case(tp.Table(src, ranges, [0, 10, 20]), None, 1, audio_pid=0x2000), "0x1fff"),
                     (tp.Case(None, None, 1, video_pid=0x1fff, audio_pid=0x1fff), "both kinds")):
        with pytest.raises(RuntimeError, match=why):
            tp.host_mux(bad)


def test_bound_module_function(hip_lib):
    from jsmpeg_amd import ts_program
    for args in ((0, 0, 0, 0, 1), (1, 1, 1, 1, 1), (65528, 1, 0, 0, 1), (1 << 33, 4000, 1 << 30, 13000, 64)):
        want = 188 * (args[0] // 184 + args[2] // 184 + 4 * args[1] + 2 * args[3] + 2 * args[4]) + 15 * args[4]
        assert ts_program.program_bound(*args) == tp.sim().sim_tsp_bound(*args) == want


# ---------------------------------------------------------------------------------------------------- the reference's demuxer

@pytest.mark.reference
@pytest.mark.skipif(not have_reference(), reason="needs the reference tree")
def test_reference_ts_js_gives_back_every_unit_of_both_kinds(hip_lib):
    from jsmpeg_amd import batch as jb
    L = jb.lib()
    fn = L.jsmpeg_hip_ts_demux_host
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint64), ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint64,
                   ctypes.POINTER(ctypes.c_uint64), ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32]
    c = tp.three_stream_program()
    got = tp.sim_equals_host(c, "three streams")
    for s in c.present():
        b, e = got.ranges[s]
        ts = np.ascontiguousarray(got.buf[b:e])
        with tempfile.NamedTemporaryFile(suffix=".ts", delete=False) as f:
            f.write(ts.tobytes())
        try:
            for kind, sid in ((tp.VIDEO, 224), (tp.AUDIO, 192)):
                t = c.tables()[kind]
                idx = [i for i in range(len(t)) if t.streams[i] == s]
                ref = json.loads(subprocess.check_output(["node", os.path.join(ROOT, "oracle", "ref_node_ts.js"), f.name, str(sid)]))
                assert len(ref["writes"]) == len(idx), (s, kind)
                es = np.zeros(t.payload + 16, np.uint8)
                total = ctypes.c_uint64()
                pts, off, ln = np.zeros(64, np.float64), np.zeros(64, np.uint64), np.zeros(64, np.uint32)
                n = fn(ts.ctypes.data, ts.size, None, 0, sid, es.ctypes.data, es.size, ctypes.byref(total), pts.ctypes.data, off.ctypes.data, ln.ctypes.data, 64)
                assert n == len(idx), (s, kind)
                for k, (w, i) in enumerate(zip(ref["writes"], idx)):
                    o, nb = t.ranges[i]
                    md5 = hashlib.md5(t.src[o:o + nb].tobytes()).hexdigest()
                    assert w["length"] == nb and w["md5"] == md5 and w["pts"] == (t.pts[i] & MASK) / 90000.0, (s, kind, i)
                    assert int(ln[k]) == nb and pts[k] == w["pts"] and hashlib.md5(es[int(off[k]):int(off[k]) + nb].tobytes()).hexdigest() == md5, (s, kind, i)
        finally:
            os.unlink(f.name)


# ---------------------------------------------------------------------------------------------------- wave and chunk edges

@pytest.mark.parametrize("n", [255, 256, 257])
def test_chunk_edges_of_the_plan(hip_lib, n):
    tp.sim_equals_host(tp.count_case(n, 3), ("video", n))
    tp.sim_equals_host(tp.count_case(3, n), ("audio", n))
    tp.sim_equals_host(tp.count_case(n, n, 3), ("both", n), aligned=True)


def test_a_stream_with_more_than_256_units_of_each_kind(hip_lib):
    c = tp.count_case(600, 580, 2, per_stream=300)
    assert min(c.video.streams.count(0), c.audio.streams.count(0)) > 256
    tp.sim_equals_host(c, "long stream")


@pytest.mark.parametrize("n_streams", [64, 65])
def test_64_and_65_streams(hip_lib, n_streams):
    c = tp.count_case(2 * n_streams, 3 * n_streams, n_streams)
    assert len(c.present()) == n_streams
    tp.sim_equals_host(c, n_streams)


# ---------------------------------------------------------------------------------------------------- build

def test_python_module_and_exports(hip_lib):
    from jsmpeg_amd import ts_program
    lib = ctypes.CDLL(hip_lib)
    for name in ("jsmpeg_hip_ts_program_create", "jsmpeg_hip_ts_program_destroy", "jsmpeg_hip_ts_program_mux", "jsmpeg_hip_ts_program_mux_encoders",
                 "jsmpeg_hip_ts_program_sync", "jsmpeg_hip_ts_program_query", "jsmpeg_hip_ts_program_ts", "jsmpeg_hip_ts_program_stream_range",
                 "jsmpeg_hip_ts_program_unit_range", "jsmpeg_hip_ts_program_read", "jsmpeg_hip_ts_program_state", "jsmpeg_hip_ts_program_reset",
                 "jsmpeg_hip_ts_program_timings", "jsmpeg_hip_ts_program_mux_host", "jsmpeg_hip_ts_program_bound"):
        assert name in ts_program.SYMBOLS and hasattr(lib, name), name
    for name in ts_program.SYMBOLS:
        assert hasattr(lib, name), name
    for name in ("mux", "mux_encoders", "sync", "ts_all", "ts", "unit_ranges", "state", "reset", "timings"):
        assert hasattr(ts_program.TsProgram, name), name
    assert callable(ts_program.program_mux_host) and callable(ts_program.program_bound) and callable(ts_program.psi_packets)
    assert os.path.exists(os.path.join(ROOT, "jsmpeg_amd", "csrc", "ts_prog.h"))


def test_kernels_use_no_scratch():
    from jsmpeg_amd import build
    usage = build.check_kernel_resources()
    for k in ("k_tsp_plan", "k_tsp_write"):
        name = [n for n in usage if k in n]
        assert name, k
        assert usage[name[0]]["ScratchSize"] == 0, k


def test_sanitizers_on_the_rule_and_the_driver():
    """ts_prog.h's functions and the simulator's driver as a stand-alone program (its own main, g++
    -fsanitize=address,undefined): the reduction to enc_ts.h, 1 .. 400 as PCR units in one call and one by one, the edges,
    random two-table cases, each taken apart again by the driver's own demuxer -- the source buffers exactly the units' size,
    so a fetch outside a unit at either end of a buffer is an error"""
    out_dir = os.path.join(ei.SIM_DIR, "_asan")
    os.makedirs(out_dir, exist_ok=True)
    exe = os.path.join(out_dir, "sim_tsp_main")
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in ei.sim_deps(tp.SIM_SRC) + [__file__]):
        subprocess.check_call(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DSIM_TSP_MAIN"] + ei.CXXFLAGS +
                              ["-o", exe, tp.SIM_SRC])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-3000:]
    assert "993 cases hold" in r.stdout
