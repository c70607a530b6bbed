"""The directed and the random inputs of the device TS demux (k_ts_parse / k_ts_walk / k_ts_gather), judged WITHOUT a GPU:
 - every directed case of tests/ts_craft.py puts its packets on the lanes and chunk edges it claims (a later edit of the
   builder must not move an edge off its lane quietly);
 - the input the device refuses (tests/golden/excluded_ts_*.json) still holds the restatement to ts.js;
 - the random sweep of tests/test_gpu_ts_walk.py is not vacuous -- judged on the restatement alone, over the same seeds;
 - the host demuxer of the live streams (jsmpeg_hip_ts_demux_host) gives the restatement's result on all of it."""
import ctypes
import glob
import hashlib
import json
import os

import numpy as np
import pytest

import ts_craft
from conftest import ROOT
from oracle import checkers
from test_ts_demux import as_fixture_writes, host_demux, load_case

EXCLUDED = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "excluded_ts_*.json")))
EXCLUDED_IDS = [os.path.basename(p)[12:-5] for p in EXCLUDED]
E0 = 0xE0


def headers(ts):
    """What every packet of an ALIGNED TS says by itself, as arrays over the packets."""
    p = ts[:len(ts) // 188 * 188].reshape(-1, 188).astype(np.int64)
    rows = np.arange(len(p))
    pusi, pid, af = (p[:, 1] >> 6) & 1, ((p[:, 1] & 0x1f) << 8) | p[:, 2], (p[:, 3] >> 4) & 3
    idx = np.where(af & 2, 5 + p[:, 4], 4)

    def at(k):
        return np.where(idx + k < 188, p[rows, np.minimum(idx + k, 187)], -1)
    is_pes = (pusi == 1) & ((af & 1) == 1) & (at(0) == 0) & (at(1) == 0) & (at(2) == 1)
    hlen = np.where(is_pes, at(8), 0)
    v = [at(9 + k) for k in range(5)]
    pts = (((v[0] >> 1) & 7) << 30) | (((v[1] << 7) | (v[2] >> 1)) << 15) | ((v[3] << 7) | (v[4] >> 1))
    return dict(n=len(p), pusi=pusi, pid=pid, af=af, idx=idx, is_pes=is_pes, sid=np.where(is_pes, at(3), -1),
                plen=np.where(is_pes, at(4) * 256 + at(5), 0), hlen=hlen, has_pts=is_pes & ((at(7) & 0x80) != 0), pts=pts,
                begin=idx + np.where(is_pes, 9 + hlen, 0))


def last_packet_of_writes(h, writes, stream_id=E0):
    """The packet whose payload is the end of each write: from the restatement's write boundaries and the payload sizes
    (PES headers inside their packets only, which holds for the cases this is used on)."""
    sid_of, end, total = {}, [], 0
    for i in range(h["n"]):
        if h["is_pes"][i]:
            sid_of[h["pid"][i]] = h["sid"][i]
        if (h["af"][i] & 1) and sid_of.get(h["pid"][i]) == stream_id:
            total += 188 - h["begin"][i]
            end.append((total, i))
    out = []
    for _, off, n in writes:
        hit = [i for e, i in end if e == off + n]
        assert hit, (off, n)
        out.append(hit[0])
    return out


def judged(libs, name):
    ts = ts_craft.CASES[name]()
    es, writes = checkers.oracle_ts_demux(libs["oracle"], ts, E0)
    reasons = checkers.oracle_ts_write_reasons(libs["oracle"])
    assert len(reasons) == len(writes)
    return ts, headers(ts), writes, reasons


@pytest.mark.parametrize("at", [255, 256, 257])
def test_chunk_carry_length_places_header_and_completion(at, libs):
    ts, h, writes, reasons = judged(libs, "chunk_carry_length_%d" % at)
    assert list(np.flatnonzero(h["plen"] != 0)) == [250] and h["sid"][250] == E0
    by_length = [k for k, r in enumerate(reasons) if r & 2]
    assert len(by_length) == 1 and reasons[by_length[0]] == 2
    assert last_packet_of_writes(h, writes)[by_length[0]] == at
    assert not h["pusi"][251:at + 10].any() and ((h["af"][251:at + 10] == 1) & (h["pid"][251:at + 10] == ts_craft.V)).all()


def test_chunk_carry_length_far_spans_a_whole_chunk(libs):
    ts, h, writes, reasons = judged(libs, "chunk_carry_length_far")
    assert list(np.flatnonzero((h["plen"] != 0) & (h["sid"] == E0))) == [100]
    by_length = [k for k, r in enumerate(reasons) if r & 2]
    assert len(by_length) == 1 and last_packet_of_writes(h, writes)[by_length[0]] == 620
    assert not (h["is_pes"][101:621] & (h["sid"] == E0)[101:621]).any()          # nothing renews the header in chunks 1 and 2


def test_chunk_carry_pid_map_places_the_headers(libs):
    ts, h, writes, _ = judged(libs, "chunk_carry_pid_map")
    v, v2 = h["pid"] == ts_craft.V, h["pid"] == ts_craft.V2
    assert h["is_pes"][255] and v[255] and h["sid"][255] == 0xE1
    assert h["is_pes"][512] and v[512] and h["sid"][512] == E0
    assert set(h["sid"][256:512][(v & h["is_pes"])[256:512]]) == {0xE1} and set(h["sid"][:255][(v & h["is_pes"])[:255]]) == {E0}
    assert set(h["sid"][v2 & h["is_pes"]]) == {E0}
    # the packets right behind the chunk edge stand on the carried map alone: data of both PIDs, no header of PID 0x100
    assert not (v & h["is_pes"])[256:264].any() and (v & (h["af"] == 1))[256:264].any() and (v2 & (h["af"] == 1))[256:264].any()
    assert not (v & h["is_pes"])[513:520].any() and (v & (h["af"] & 1 == 1))[513:520].any()
    # what the destination gets in chunk 1 is PID 0x101 alone
    last = last_packet_of_writes(h, writes)
    assert all(h["pid"][i] == ts_craft.V2 for i in last if 256 <= i < 512) and any(256 <= i < 512 for i in last)


def test_wave_edges_places_the_starts(libs):
    ts, h, writes, reasons = judged(libs, "wave_edges")
    starts = np.flatnonzero(h["is_pes"] & (h["sid"] == E0))
    assert list(starts) == list(ts_craft.WAVE_EDGES) + [256, 256 + 63, 256 + 127, 256 + 191, 511]
    with_len = [int(i) for i in starts if h["plen"][i]]
    assert with_len == [0, 64, 128, 192, 256 + 63, 256 + 127, 256 + 191, 511]
    last = last_packet_of_writes(h, writes)
    assert [last[k] for k, r in enumerate(reasons) if r & 2] == [i + 2 for i in with_len]     # 321, 385, 449: the next wave; 513: the next chunk


def test_two_headers_one_pid_one_chunk_places_the_headers(libs):
    ts, h, _, _ = judged(libs, "two_headers_one_pid_one_chunk")
    at = np.flatnonzero(h["is_pes"])
    assert list(at) == [0, 50, 60, 70, 250, 254, 258] and list(h["sid"][at]) == [E0, E0, 0xE1, E0, E0, 0xE1, E0]
    assert (h["pid"] == ts_craft.V).all()


@pytest.mark.parametrize("name,n,lead", [("dense_writes", 600, 0)] + [("dense_writes_%d" % n, n, 3) for n in ts_craft.DENSE_COUNTS])
def test_dense_writes_has_the_candidates_it_claims(name, n, lead, libs):
    ts, h, writes, reasons = judged(libs, name)
    assert h["n"] == n + lead and (h["pid"][:lead] == 0x1fff).all()
    d = slice(lead, None)
    assert (h["is_pes"][d] & (h["sid"][d] == E0) & (h["af"][d] == 1)).all()      # every packet a start without stuffing: n candidates
    assert ((h["plen"][d] != 0) == (np.arange(n) % 2 == 1)).all()
    assert len(writes) == 2 * (n // 2) and reasons == [1, 2] * (n // 2)           # two writes out of every second packet
    assert all(w[2] == 170 for w in writes)


def test_pts_33_bits_places_the_timestamps(libs):
    ts, h, writes, _ = judged(libs, "pts_33_bits")
    at = np.flatnonzero(h["is_pes"])
    assert [int(h["pts"][i]) if h["has_pts"][i] else None for i in at] == list(ts_craft.PTS_33)
    assert [w[0] for w in writes] == [(p or 0) / 90000.0 for p in ts_craft.PTS_33]
    assert max(p or 0 for p in ts_craft.PTS_33) >> 32 == 1


def test_negative_total_places_the_headers(libs):
    ts, h, writes, reasons = judged(libs, "negative_total")
    neg = np.flatnonzero(h["is_pes"] & (h["plen"] != 0) & (h["plen"] < h["hlen"] + 3))
    assert list(neg) == [4, 7, 10] and h["begin"][7] == 188 and not h["has_pts"][10]
    assert [w for w in writes if w[2] == 0] == [(15000 / 90000.0, writes[3][1], 0)]
    assert last_packet_of_writes(h, writes)[1] == 4 and reasons[1] == 2


def test_reserved_and_af_only_places_the_packets(libs):
    ts, h, writes, reasons = judged(libs, "reserved_and_af_only")
    assert list(h["af"][[3, 5, 7, 9]]) == [0, 0, 2, 2] and list(h["pusi"][[3, 5, 7, 9]]) == [0, 1, 0, 1]
    assert h["pusi"][11] and h["af"][11] == 1 and not h["is_pes"][11]
    assert (h["pid"][:17] == ts_craft.V).all() and reasons[:4] == [1, 1, 1, 1]
    assert [w[0] for w in writes[:5]] == [30000 / 90000.0] * 5                     # none of them starts a PES
    assert last_packet_of_writes(h, writes)[:3] == [4, 8, 10]


@pytest.mark.parametrize("name,n", [("sixteen_pids", 16), ("seventeen_pids", 17)])
def test_n_pids_carry_pes_headers(name, n, libs):
    ts, h, _, _ = judged(libs, name)
    assert len(set(h["pid"][h["is_pes"]])) == n


def test_end_of_data_places_the_packet():
    k = ts_craft.END_AT
    for name in ("end_of_data_inner_write", "end_of_data_inner_partial", "end_of_data_before_partial", "end_of_data_last"):
        ts = ts_craft.CASES[name]()
        h = headers(ts)
        assert h["pusi"][k] and h["af"][k] == 3 and h["idx"][k] == 188 and h["pid"][k] == ts_craft.V
    assert ts_craft.WRITES["end_of_data_inner_write"][0] == 188 * (k + 1)
    assert ts_craft.WRITES["end_of_data_inner_partial"][0] == 188 * (k + 1) + 50
    assert len(ts_craft.CASES["end_of_data_before_partial"]()) == 188 * (k + 1) + 60
    assert len(ts_craft.CASES["end_of_data_last"]()) == 188 * (k + 1)
    assert len(ts_craft.CASES["end_of_data_inner_write"]()) > 188 * (k + 7)


def test_spill_places_the_headers():
    ts = ts_craft.CASES["spill_adjacent"]()
    h = headers(ts)
    p = ts.reshape(-1, 188)
    assert [int(h["idx"][i]) for i in ts_craft.SPILL_AT] == [185, 183, 180]         # the stream id, the length, header_length are the next packet's
    for i in ts_craft.SPILL_AT:
        assert h["pusi"][i] and bytes(p[i, h["idx"][i]:h["idx"][i] + 3]) == b"\x00\x00\x01"
    junk = ts_craft.CASES["spill_junk"]()
    at = 188 * (ts_craft.SPILL_AT[0] + 1)
    assert len(junk) == len(ts) + 30 and np.array_equal(junk[:at], ts[:at]) and np.array_equal(junk[at + 30:], ts[at:])
    assert junk[at] == E0 and 0x47 not in junk[at:at + 30]


def test_header_past_packet_places_the_header():
    h = headers(ts_craft.CASES["header_past_packet"]())
    assert h["is_pes"][2] and h["sid"][2] == E0 and h["begin"][2] > 188
    assert (h["begin"][np.arange(h["n"]) != 2] <= 188).all()


@pytest.mark.parametrize("path", EXCLUDED, ids=EXCLUDED_IDS)
def test_oracle_matches_reference_on_what_the_device_refuses(path, libs):
    fx, ts = load_case(path)
    assert fx["refused"] == ts_craft.REFUSED[(fx["case"], "write_sizes" in fx)]
    es, writes = checkers.oracle_ts_demux(libs["oracle"], ts, fx["stream_id"], fx.get("write_sizes"))
    assert as_fixture_writes(es, writes) == fx["writes"]


@pytest.mark.parametrize("path", EXCLUDED, ids=EXCLUDED_IDS)
def test_host_demuxer_matches_reference_on_what_the_device_refuses(path, hip_lib):
    """the host demuxer reads on in the written bytes like ts.js does: it has nothing to refuse"""
    from jsmpeg_amd import batch as jb
    fx, ts = load_case(path)
    es, writes = host_demux(jb.lib(), ts, fx["stream_id"], fx.get("write_sizes"))
    assert as_fixture_writes(es, writes) == fx["writes"]
    assert hashlib.md5(es.tobytes()).hexdigest() == fx["total_md5"]


def test_every_refused_case_has_its_fixture():
    have = {(json.load(open(p))["case"], "write_sizes" in json.load(open(p))) for p in EXCLUDED}
    assert have == set(ts_craft.REFUSED)


# ---------------------------------------------------------------------------------------------------------------------
# the random sweep

def framed_packets(libs, ts, sizes):
    """the packets ts.js parses (the restatement's framing, which the host pre-pass of upload_ts is held to)"""
    ora = ctypes.CDLL(libs["oracle"])
    ora.ts_oracle_packets.restype = ctypes.c_long
    u64 = ctypes.c_uint64
    ts = np.ascontiguousarray(ts)
    cap = len(ts) // 188 + 8
    at = (u64 * cap)()
    ws = (u64 * max(1, len(sizes or [])))(*(sizes or []))
    n = ora.ts_oracle_packets(ctypes.c_void_p(ts.ctypes.data), ctypes.c_size_t(len(ts)), ws, ctypes.c_int(len(sizes or [])), at,
                              ctypes.c_size_t(cap), None)
    return np.array(at[:n], dtype=np.int64)


def test_random_sweep_is_not_vacuous(libs):
    """Over the seeds of the GPU sweep, by the restatement alone: no input is one the device refuses (no framed packet --
    not even one that resync made out of junk -- has a header reaching to or past its end, at most 16 PIDs carry PES
    headers); at least 90 % of the non-empty streams give three or more writes; each way a write ends -- by length, by
    stuffing, by the next payload start, still pending at the end of the input -- occurs at least 20 times; every batch
    has streams on both sides of 256 and of 512 packets and one of 0, 1, 255, 256 or 257."""
    ends = dict(length=0, stuffing=0, next_start=0, pending=0)
    streams = enough = 0
    for b in range(ts_craft.SWEEP_BATCHES):
        sid = ts_craft.sweep_stream_id(b)
        for way, tss, sizes in ts_craft.sweep_runs(b):
            assert len(tss) == 8
            if way == "one_write":
                n = sorted(len(ts) // 188 for ts in tss)
                assert ts_craft.SWEEP_FIXED[b % 5] in n and any(1 < x < 255 for x in n) and any(257 < x < 512 for x in n) and n[-1] > 512
            for s, ts in enumerate(tss):
                ws = None if sizes is None else sizes[s]
                at = framed_packets(libs, ts, ws)
                if len(at):
                    h = headers(np.concatenate([ts[a:a + 188] for a in at]))
                    assert not ((h["pusi"] == 1) & (h["af"] & 1 == 1) & (h["idx"] + 14 > 188)).any(), (b, way, s)
                    assert (h["begin"][h["af"] & 1 == 1] <= 188).all(), (b, way, s)
                    assert len(set(h["pid"][h["is_pes"]])) <= 16, (b, way, s)
                es, writes = checkers.oracle_ts_demux(libs["oracle"], ts, sid, ws)
                reasons = checkers.oracle_ts_write_reasons(libs["oracle"])
                ends["length"] += sum(1 for r in reasons if r & 2)
                ends["stuffing"] += sum(1 for r in reasons if r == 4)
                ends["next_start"] += sum(1 for r in reasons if r == 1)
                ends["pending"] += len(es) > sum(w[2] for w in writes)
                if len(at):
                    streams += 1
                    enough += len(writes) >= 3
    assert min(ends.values()) >= 20, ends
    assert enough >= 0.9 * streams, (enough, streams)


def test_live_streams_host_demuxer_on_the_random_sweep(libs, hip_lib):
    """the generated inputs of the sweep through jsmpeg_hip_ts_demux_host: same bytes, same write() boundaries, same pts as
    the restatement (the equality of the host demuxer's own sweep in test_ts_demux.py)"""
    from jsmpeg_amd import batch as jb
    for b in range(ts_craft.SWEEP_BATCHES):
        sid = ts_craft.sweep_stream_id(b)
        for way, tss, sizes in ts_craft.sweep_runs(b):
            for s, ts in enumerate(tss):
                ws = None if sizes is None else sizes[s]
                if ws is not None and not ws:
                    continue                            # no write() at all
                want_es, want_w = checkers.oracle_ts_demux(libs["oracle"], ts, sid, ws)
                got_es, got_w = host_demux(jb.lib(), ts, sid, ws)
                assert got_w == want_w, (b, way, s)
                assert np.array_equal(got_es, want_es[:len(got_es)]) and len(got_es) == sum(w[2] for w in want_w), (b, way, s)
