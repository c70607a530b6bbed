"""The slice parse's DEVICE-ONLY parts (slice_parse.h: the inline-asm 64-bit window over the LDS ring and its copy of row 0, the
refill in one piece and in two halves with its hold-back, the token ring's drains and its dword-by-dword tail, the start
phase) under the crafted streams of tests/parse_inputs.py -- symbols at chosen bit positions, every payload_off & 15, the turns
that consume the most bits, every end of a slice, short and long slices in one wavefront.  tests/test_parse_edges.py checks on
the CPU what the sets hold and reach and that oracle, simulator and the reference's C agree on them; here every way into the
parse kernels is held against the oracle's decode of the same bytes, bit for bit: the batch as created with each kernel
forced (k_parse, k_parse_split), enqueue + sync (the *_planned kernels), the one-picture interface without decode-ahead, a
narrow ticket configuration in a child process, and the company streams as one batch and as sixteen copies.

A failure names the stream, the picture, the first differing macroblock, its slice (row and start byte), and the first
macroblock record or token of the device that differs from the simulator's (jsmpeg_hip_batch_debug_read 4 and 5; only the slots
the simulator's records count: the device buffer is not cleared, an odd run's alignment slot holds whatever the ring held).
The records are diagnostics; the picture is the contract.

The 24 streams are written once per module (under a second) and decoded once by the oracle.  Needs an MI355X."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import parse_inputs as P
from conftest import ROOT
from jsmpeg_amd import batch as jb
from jsmpeg_amd import cabi, hashing

pytestmark = pytest.mark.gpu

SETS = [fn.__name__ for fn in P.SETS]
BY_NAME = {fn.__name__: fn for fn in P.SETS}
_want = {}


def streams_of(name):
    return [P.written(s) for s in BY_NAME[name]()["streams"]]


def expected(libs, w):
    """the oracle's pictures of a stream, once: (planes per picture, device-style hash per picture)"""
    if w["name"] not in _want:
        frames, _, _ = cabi.decode_stream(libs["oracle"], w["es"], keep="planes")
        assert len(frames) == len(w["desc"]["pictures"])
        _want[w["name"]] = (frames, [hashing.frame_hash(*f) for f in frames])
    return _want[w["name"]]


def geometry(w):
    d = w["desc"]
    return d["width"], d["height"], (d["width"] + 15) >> 4, (d["height"] + 15) >> 4


def slice_of(w, p, mb):
    """the slice that holds macroblock mb of picture p -> (row its start code names, byte offset of the start code in the stream)"""
    d = w["desc"]
    _, _, mbw, mbh = geometry(w)
    es = w["es"]
    pos = np.flatnonzero((es[:-3] == 0) & (es[1:-2] == 0) & (es[2:-1] == 1))
    codes = es[pos + 3]
    pics = [i for i in range(len(pos)) if codes[i] == 0x00]
    first = pics[p]
    last = pics[p + 1] if p + 1 < len(pics) else len(pos)
    sl = [i for i in range(first, last) if 1 <= codes[i] <= 0xAF]
    pic = d["pictures"][p]
    starts = [s["start"] if isinstance(s, dict) else s for s in pic.get("slices", range(0, mbw * mbh, mbw))]
    k = max(i for i, s in enumerate(starts) if s <= mb)
    return int(codes[sl[k]]) - 1, int(pos[sl[k]])


def device_vs_simulator(b, w, p):
    """the first macroblock record and the first token of picture p (of a one-stream batch) where the device differs from the
    simulator -> text"""
    width, height, mbw, mbh = geometry(w)
    mbn = mbw * mbh
    es = w["es"]
    n = len(w["desc"]["pictures"])
    so = os.path.join(ROOT, "tests", "sim", "libjsmpeg_sim.so")
    src = [os.path.join(ROOT, "tests", "sim", "sim_decode.cpp"), os.path.join(ROOT, "jsmpeg_amd", "csrc", "slice_parse.h")]
    if not os.path.exists(so) or any(os.path.getmtime(f) > os.path.getmtime(so) for f in src):
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-Wno-unknown-pragmas", "-I", os.path.join(ROOT, "jsmpeg_amd", "csrc"),
                               "-o", so, os.path.join(ROOT, "tests", "sim", "sim_decode.cpp")])
    sim = ctypes.CDLL(so)
    sim.sim_dump_counts.restype = ctypes.POINTER(ctypes.c_uint32)
    sim.sim_set_dumps.argtypes = [ctypes.c_void_p] * 5
    sim.sim_decode_stream.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_int]
    s_mb = np.zeros((n + 2) * mbn * 4, np.uint32)
    s_tok = np.zeros((len(es) + 1024) * 4, np.uint16)
    out = np.zeros(n * mbn * 384, np.uint8)
    sim.sim_set_dumps(None, None, None, s_mb.ctypes.data, s_tok.ctypes.data)
    try:
        sim.sim_decode_stream(es.ctypes.data, len(es), width, height, out.ctypes.data, n)
    finally:
        sim.sim_set_dumps(None, None, None, None, None)
    ntok = int(sim.sim_dump_counts()[3])
    L = jb.lib()
    L.jsmpeg_hip_batch_debug_read.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint64]

    def rd(what, dtype, count):
        a = np.zeros(count, dtype)
        if L.jsmpeg_hip_batch_debug_read(b.h, what, a.ctypes.data, 0, a.nbytes) != 0:
            return None
        return a
    text = []
    g_mb = rd(4, np.uint32, n * mbn * 4)
    if g_mb is not None:
        g, s = g_mb.reshape(n, mbn, 4)[p], s_mb[:n * mbn * 4].reshape(n, mbn, 4)[p]
        g, s = g.copy(), s.copy()
        g[:, 3] &= 0x00ffffff                                      # (the epoch byte counts the device's passes)
        s[:, 3] &= 0x00ffffff
        bad = np.flatnonzero((g != s).any(axis=1))
        if len(bad):
            a = int(bad[0])
            text.append("first differing record: macroblock %d (row %d, column %d): device %s, simulator %s; %d records differ"
                        % (a, a // mbw, a % mbw, [hex(int(x)) for x in g[a]], [hex(int(x)) for x in s[a]], len(bad)))
        else:
            text.append("all %d records of the picture equal the simulator's" % mbn)
    g_tok = rd(5, np.uint16, ntok)
    if g_tok is not None:
        # only the slots the simulator's records of this picture count: the device buffer is not cleared, and the alignment slot
        # behind an odd run holds whatever the lane's ring held (never read; it differs with the order the slices are taken in)
        sim.sim_dump_tok_off.restype = ctypes.POINTER(ctypes.c_uint64)
        base = int(sim.sim_dump_tok_off()[p])
        recs = s_mb[:n * mbn * 4].reshape(n, mbn, 4)[p]
        first = None
        differ = 0
        for a in range(mbn):
            v = [int(x) for x in recs[a]]
            at = base + v[0]
            cnts = v[2] | ((v[3] & 0xffff) << 32)
            for blk in range(6):
                c = (cnts >> (8 * blk)) & 255
                for i in range(at, at + c):
                    if i < ntok and g_tok[i] != s_tok[i]:
                        differ += 1
                        if first is None:
                            first = (a, blk, i - at, i)
                at += (c + 1) & ~1
        if first is None:
            text.append("every token the records count is the simulator's")
        else:
            a, blk, k, i = first
            text.append("first differing token: macroblock %d block %d token %d (slot %d): device 0x%04x, simulator 0x%04x; %d differ"
                        % (a, blk, k, i, int(g_tok[i]), int(s_tok[i]), differ))
    return "; ".join(text)


def explain(w, p, got, want, b=None):
    """picture p differs: where, in which slice, and what the device recorded there"""
    _, _, mbw, _ = geometry(w)
    for plane, (g, e) in enumerate(zip(got, want)):                 # Y, Cr, Cb
        bad = np.flatnonzero(np.asarray(g).ravel() != np.asarray(e).ravel())
        if len(bad) == 0:
            continue
        stride = mbw * 16 if plane == 0 else mbw * 8
        y, x = divmod(int(bad[0]), stride)
        mb = (y >> 4) * mbw + (x >> 4) if plane == 0 else (y >> 3) * mbw + (x >> 3)
        row, at = slice_of(w, p, mb)
        text = ("%s picture %d (%s), plane %d, pixel (%d, %d): macroblock %d (row %d, column %d) of the slice whose start code names row %d at byte %d "
                "(payload_off & 15 = %d); %d bytes of the plane differ, got %d want %d"
                % (w["name"], p, w["desc"]["pictures"][p]["type"], plane, x, y, mb, mb // mbw, mb % mbw, row, at, (at + 4) & 15, len(bad),
                   int(np.asarray(g).ravel()[bad[0]]), int(np.asarray(e).ravel()[bad[0]])))
        if b is not None:
            text += "; " + device_vs_simulator(b, w, p)
        return text
    return "%s picture %d: hashes differ, planes do not" % (w["name"], p)


def check_batch(b, ws, libs, copies=1):
    """a batch that holds the streams ws, `copies` times over, in order"""
    want, frames, owner = [], [], []
    for _ in range(copies):
        for w in ws:
            f, h = expected(libs, w)
            want += h
            frames += f
            owner += [(w, i) for i in range(len(h))]
    assert b.picture_count == len(want)
    dev = [int(x) for x in b.frame_hashes()]
    for p in range(len(want)):
        if dev[p] != want[p]:
            w, i = owner[p]
            raise AssertionError(explain(w, i, b.read_frame(p), frames[p], b if len(ws) == 1 and copies == 1 else None) + " (batch picture %d)" % p)


def new_batch(ws, copies=1):
    width, height, _, _ = geometry(ws[0])
    assert all(geometry(w)[:2] == (width, height) for w in ws)
    pics = sum(len(w["desc"]["pictures"]) for w in ws)
    size = sum(len(w["es"]) + 64 for w in ws)
    return jb.Batch(width, height, copies * len(ws), copies * pics + 4, copies * size + 8192)


@pytest.mark.parametrize("split", ["0", "1"], ids=["k_parse", "k_parse_split"])
@pytest.mark.parametrize("name", SETS)
def test_batch_as_created(name, split, hip_lib, libs, monkeypatch):
    monkeypatch.setenv("JSMPEG_HIP_PARSE_SPLIT", split)
    for w in streams_of(name):
        with new_batch([w]) as b:
            b.upload([w["es"]])
            assert b.decode() == len(w["desc"]["pictures"])
            check_batch(b, [w], libs)


@pytest.mark.parametrize("name", SETS)
def test_enqueue_and_sync(name, hip_lib, libs):
    """the pass planned on the device: k_parse_planned / k_parse_split_planned"""
    for w in streams_of(name):
        with new_batch([w]) as b:
            b.upload([w["es"]])
            assert b.enqueue() == 0
            b.sync()
            check_batch(b, [w], libs)


@pytest.mark.parametrize("name", SETS)
def test_one_picture_interface(name, hip_lib, libs, monkeypatch):
    monkeypatch.setenv("JSMPEG_HIP_DECODE_AHEAD", "0")
    for w in streams_of(name):
        frames, _ = expected(libs, w)
        got, _, _ = cabi.decode_stream(hip_lib, w["es"], keep="planes")
        assert len(got) == len(frames)
        for p in range(len(frames)):
            if any(not np.array_equal(g, e) for g, e in zip(got[p], frames[p])):
                raise AssertionError(explain(w, p, got[p], frames[p]))


TICKETS = dict(JSMPEG_HIP_PARSE_RESIDENT="1", JSMPEG_HIP_PARSE_LANES="64", JSMPEG_HIP_PARSE_HEAD="5,1,23,2")


@pytest.mark.parametrize("name", SETS)
def test_narrow_tickets(name, hip_lib, libs, tmp_path):
    """one parse workgroup whose wavefronts draw every further batch of slices by ticket, the first 5 slices one per wavefront,
    the next 18 two per wavefront, the rest 64: a segmentation no stream's slice count is a multiple of (the library reads
    these once per process: a fresh child, each stream twice in its batch)"""
    want = {w["name"]: [int(h) for h in expected(libs, w)[1]] for w in streams_of(name)}
    path = tmp_path / "want.json"
    path.write_text(json.dumps(want))
    code = r'''
import json, os, sys
sys.path.insert(0, %r); sys.path.insert(0, os.path.join(%r, "tests"))
import parse_inputs as P
from jsmpeg_amd import batch as jb
want = json.load(open(%r))
bad = []
for s in dict((fn.__name__, fn) for fn in P.SETS)[%r]()["streams"]:
    w = P.written(s)
    d, es, n = w["desc"], w["es"], len(w["desc"]["pictures"])
    with jb.Batch(d["width"], d["height"], 2, 2 * n + 4, 2 * len(es) + 8192) as b:
        b.upload([es, es])
        assert b.decode() == 2 * n
        dev = [int(x) for x in b.frame_hashes()]
        bad += [(w["name"], p) for p in range(2 * n) if dev[p] != want[w["name"]][p %% n]]
print("BAD", bad)
assert not bad
''' % (ROOT, ROOT, str(path), name)
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, **TICKETS), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]


@pytest.mark.parametrize("split", ["0", "1"], ids=["k_parse", "k_parse_split"])
def test_company_in_one_batch(split, hip_lib, libs, monkeypatch):
    """short header-heavy slices and long coefficient-heavy ones in the same wavefronts: as a batch of the two streams, and either
    of them sixteen times -- every copy equal to the stream alone (which test_batch_as_created holds to the oracle)"""
    monkeypatch.setenv("JSMPEG_HIP_PARSE_SPLIT", split)
    a, c = streams_of("company")
    for ws, copies in (([a, c], 1), ([c, a], 1), ([a, c], 8), ([a], 16), ([c], 16)):
        with new_batch(ws, copies) as b:
            b.upload([w["es"] for w in ws] * copies)
            assert b.decode() == copies * sum(len(w["desc"]["pictures"]) for w in ws)
            check_batch(b, ws, libs, copies)
