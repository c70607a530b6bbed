"""The device TS demux (k_ts_parse / k_ts_walk / k_ts_gather behind upload_ts) on what its GPU-specific code can get wrong:
the directed cases of tests/ts_craft.py reach it through the fixtures of test_ts_demux.py; here are the input it must
REFUSE (tests/golden/excluded_ts_*.json) and a random sweep of ragged batches against the CPU restatement of ts.js.
tests/test_ts_walk_cases.py shows on the CPU that the sweep is not vacuous."""
import numpy as np
import pytest

import ts_craft
from oracle import checkers
from test_ts_demux import as_fixture_writes, load_case
from test_ts_walk_cases import EXCLUDED, EXCLUDED_IDS

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("path", EXCLUDED, ids=EXCLUDED_IDS)
def test_device_demux_refuses_what_it_cannot_match(path, hip_lib, libs):
    """upload_ts raises with the stated message -- nothing is silently different from ts.js --, the write list of the
    upload before it is gone (its rows lie at another upload's offsets), and the handle goes on working: the next
    upload_ts gives the restatement's result."""
    from jsmpeg_amd import batch as jb
    fx, ts = load_case(path)
    ws = fx.get("write_sizes")
    good = ts_craft.CASES["negative_total"]()
    want_es, want_w = checkers.oracle_ts_demux(libs["oracle"], good, 0xE0)
    with jb.Batch(176, 144, 2, 64, 1 << 20) as b:
        b.upload_ts([good, good], 0xE0)
        assert b.ts_writes(0) == want_w
        with pytest.raises(RuntimeError, match=fx["refused"]):
            b.upload_ts([good, ts], fx["stream_id"], None if ws is None else [[len(good)], ws])
        with pytest.raises(RuntimeError, match="no TS upload"):
            b.ts_writes(0)
        b.upload_ts([ts[:188 * 2], good], 0xE0)
        assert b.ts_writes(1) == want_w
        assert np.array_equal(b.read_es(1), want_es[:sum(w[2] for w in want_w)])


def check_batch(libs, handle, read, tss, sizes, sid, tag):
    for s, ts in enumerate(tss):
        want_es, want_w = checkers.oracle_ts_demux(libs["oracle"], ts, sid, None if sizes is None else sizes[s])
        assert handle.ts_writes(s) == want_w, (tag, s)                   # pts with ==: both sides divide the same integer by 90000.0
        got = read(s)
        assert len(got) == sum(w[2] for w in want_w) and np.array_equal(got, want_es[:len(got)]), (tag, s)


def test_audio_handle_refuses_the_same(hip_lib, libs):
    """the three refusals through mp2.Mp2Batch.upload_ts, each after a good upload whose write list it must take along"""
    from jsmpeg_amd import mp2
    good = [ts_craft.CASES["sixteen_pids"](), ts_craft.CASES["video_audio_null"]()]
    with mp2.Mp2Batch(2, 1 << 20) as b:
        for case, sid in (("spill_junk", 0xE0), ("seventeen_pids", 0xC0), ("header_past_packet", 0xE0)):
            b.upload_ts(good, 0xC0)
            assert len(b.ts_writes(0)) > 0
            with pytest.raises(RuntimeError, match=ts_craft.REFUSED[(case, False)]):
                b.upload_ts([good[0], ts_craft.CASES[case]()], sid)
            with pytest.raises(RuntimeError, match="no TS upload"):
                b.ts_writes(0)
        b.upload_ts(good, 0xC0)
        check_batch(libs, b, b.read_bytes, good, None, 0xC0, "after the refusals")


def test_random_sweep_matches_the_restatement(hip_lib, libs):
    """30 batches of 8 generated streams (ts_craft.sweep_runs: packet counts on both sides of 256 and 512 and one of 0, 1,
    255, 256, 257; up to 6 PIDs; PES with and without length and PTS; stuffing, adaptation-field-only, reserved and null
    packets, payload starts that are no PES), each in one write(), in write() calls of random sizes, and damaged (junk
    between packets, truncated end): the same destination.write triples and the same bytes as the restatement, with 0xE0
    or 0xC0 connected."""
    from jsmpeg_amd import batch as jb
    with jb.Batch(176, 144, 8, 64, 1 << 21) as b:
        for k in range(ts_craft.SWEEP_BATCHES):
            sid = ts_craft.sweep_stream_id(k)
            for way, tss, sizes in ts_craft.sweep_runs(k):
                b.upload_ts(tss, sid, sizes)
                check_batch(libs, b, b.read_es, tss, sizes, sid, (k, way))


def test_random_sweep_through_the_audio_handle(hip_lib, libs):
    """the same kernels behind mp2.Mp2Batch.upload_ts (one write() per stream), a few batches"""
    from jsmpeg_amd import mp2
    with mp2.Mp2Batch(8, 1 << 21) as b:
        for k in (1, 2, 4, 7):
            sid = ts_craft.sweep_stream_id(k)
            for way, tss, _ in ts_craft.sweep_runs(k):
                if way == "pieces":
                    continue
                b.upload_ts(tss, sid)
                check_batch(libs, b, b.read_bytes, tss, None, sid, (k, way))
