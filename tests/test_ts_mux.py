"""The host-side TS mux of C ABI part 8 (jsmpeg_hip_ts_mux_host): the demuxer pinned to the reference's ts.js
(jsmpeg_hip_ts_demux_host, tests/test_ts_demux.py) over its output gives back the bytes, one write per unit with that unit's
range and pts -- in one write, in ragged writes, and for two mux calls with the continuity counter carried; and the same
through ts.js itself under Node where the reference is present."""
import hashlib
import json
import os
import subprocess
import tempfile

import numpy as np
import pytest

from conftest import ROOT, have_reference
from test_ts_demux import host_demux


def units_case(seed, sizes):
    """`sizes` units back to back behind 5 bytes that belong to no unit; bytes that hold no TS sync pattern by design of
    the demuxer (a PES payload is never searched for sync)"""
    rng = np.random.default_rng(seed)
    es = rng.integers(0, 256, 5 + sum(sizes), dtype=np.uint8)
    ranges, at = [], 5
    for n in sizes:
        ranges.append((at, n))
        at += n
    pts = [(1 << 33) / 90000.0 - 1.0 if i == 0 else 0.5 + i / 30.0 for i in range(len(sizes))]     # the first: a PTS that needs bit 32
    return es, ranges, pts


# 170: the PES fits one packet with stuffing; 174: exactly one full packet; 14 + n a multiple of 184 below and above the
# 16-bit PES length (65527 payload bytes is the last one that has a length); a picture-sized unit
SIZES = [170, 174, 1, 184 * 3 - 14, 1000, 65527, 65528, 184 * 400 - 14, 184 * 400 - 13, 100000]


def check(writes, got_es, es, ranges, pts):
    assert len(writes) == len(ranges)
    at = 0
    for (p, off, n), (o, b), t in zip(writes, ranges, pts):
        assert (off, n) == (at, b)
        assert np.array_equal(got_es[off:off + n], es[o:o + b])
        assert p == int(round(t * 90000.0)) / 90000.0
        at += b
    assert len(got_es) == at


@pytest.fixture(scope="module")
def L(hip_lib):
    from jsmpeg_amd import encode
    return encode.lib()


def test_demux_gives_back_every_unit(L):
    from jsmpeg_amd import encode
    es, ranges, pts = units_case(1, SIZES)
    ts, cc = encode.ts_mux(es, ranges, pts)
    assert len(ts) % 188 == 0 and np.all(ts[::188] == 0x47)
    assert cc == (len(ts) // 188) % 16
    assert np.array_equal(ts[3::188] & 15, np.arange(len(ts) // 188) % 16)
    got_es, writes = host_demux(L, ts, 0xE0)
    check(writes, got_es, es, ranges, pts)


def test_ragged_writes(L):
    from jsmpeg_amd import encode
    es, ranges, pts = units_case(2, SIZES)
    ts, _ = encode.ts_mux(es, ranges, pts)
    rng = np.random.default_rng(3)
    sizes, left = [], len(ts)
    while left:
        n = int(min(left, rng.integers(1, 5000)))
        sizes.append(n)
        left -= n
    got_es, writes = host_demux(L, ts, 0xE0, sizes)
    check(writes, got_es, es, ranges, pts)


def test_two_calls_carry_the_continuity_counter(L):
    from jsmpeg_amd import encode
    es, ranges, pts = units_case(4, SIZES)
    a, cc = encode.ts_mux(es, ranges[:4], pts[:4])
    b, cc2 = encode.ts_mux(es, ranges[4:], pts[4:], continuity=cc)
    whole, cc3 = encode.ts_mux(es, ranges, pts)
    assert np.array_equal(np.concatenate([a, b]), whole) and cc2 == cc3
    got_es, writes = host_demux(L, np.concatenate([a, b]), 0xE0)
    check(writes, got_es, es, ranges, pts)


def test_needed_bytes_and_refusals(L):
    import ctypes
    from jsmpeg_amd import batch
    es, ranges, pts = units_case(5, [300, 20])
    off = np.array([r[0] for r in ranges], np.uint64)
    ln = np.array([r[1] for r in ranges], np.uint32)
    p90 = np.array([90000, 93000], np.uint64)
    need = L.jsmpeg_hip_ts_mux_host(es.ctypes.data, off.ctypes.data, ln.ctypes.data, p90.ctypes.data, 2, 0xE0, 0x100, None, None, 0)
    assert need == 188 * 3
    out = np.zeros(need, np.uint8)
    assert L.jsmpeg_hip_ts_mux_host(es.ctypes.data, off.ctypes.data, ln.ctypes.data, p90.ctypes.data, 2, 0xE0, 0x100, None, out.ctypes.data, need - 1) < 0
    assert "ts_cap" in batch.last_error()
    assert L.jsmpeg_hip_ts_mux_host(es.ctypes.data, off.ctypes.data, ln.ctypes.data, p90.ctypes.data, 2, 0xE0, 0x2000, None, out.ctypes.data, need) < 0
    cc = ctypes.c_uint8(15)
    assert L.jsmpeg_hip_ts_mux_host(es.ctypes.data, off.ctypes.data, ln.ctypes.data, p90.ctypes.data, 2, 0xE0, 0x100, ctypes.byref(cc), out.ctypes.data, need) == need
    assert cc.value == 2 and list(out[3::188] & 15) == [15, 0, 1]


@pytest.mark.reference
@pytest.mark.skipif(not have_reference(), reason="needs the reference tree")
@pytest.mark.parametrize("write_sizes", [None, [1000, 77, 188 * 40 + 3]], ids=["one_write", "ragged"])
def test_reference_ts_js_gives_back_every_unit(L, write_sizes):
    from jsmpeg_amd import encode
    es, ranges, pts = units_case(6, SIZES)
    ts, _ = encode.ts_mux(es, ranges, pts)
    with tempfile.NamedTemporaryFile(suffix=".ts", delete=False) as f:
        f.write(ts.tobytes())
    try:
        cmd = ["node", os.path.join(ROOT, "oracle", "ref_node_ts.js"), f.name, "224"]
        if write_sizes:
            cmd.append(",".join(str(x) for x in write_sizes + [len(ts) - sum(write_sizes)]))
        ref = json.loads(subprocess.check_output(cmd))
    finally:
        os.unlink(f.name)
    assert len(ref["writes"]) == len(ranges)
    for w, (o, b), t in zip(ref["writes"], ranges, pts):
        assert w["length"] == b and w["md5"] == hashlib.md5(es[o:o + b].tobytes()).hexdigest()
        assert w["pts"] == int(round(t * 90000.0)) / 90000.0
