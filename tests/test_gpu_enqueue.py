"""jsmpeg_hip_batch_enqueue: the pass as a pure enqueue, planned on the device (csrc/enqueue_plan.h, kernels.hip k_plan /
k_parse_planned) -- the golden fixtures and the oracle through enqueue + sync, the ordered launch by streams and the plan
left to the host at sync (status 8), no host wait behind a busy stream, two batches in flight from one thread, the overflow,
the fallbacks, a flagged launch, and what a batch with a pass in flight refuses.  Needs an MI355X."""
import glob
import hashlib
import json
import os
import subprocess
import sys
import threading
import time

import numpy as np
import pytest

from conftest import ROOT
from jsmpeg_amd import batch as jb
from jsmpeg_amd import cabi, hashing, synth

pytestmark = pytest.mark.gpu

FIXTURES = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "frames_*.json")))


def md5_planes(planes):
    h = hashlib.md5()
    for p in planes:
        h.update(p.tobytes())
    return h.hexdigest()


def oracle_hashes(libs, es):
    frames, _, _ = cabi.decode_stream(libs["oracle"], es, keep="planes")
    return [hashing.frame_hash(*f) for f in frames]


def info_tuple(b):
    return [(i.stream, i.es_offset, i.type, i.decoded, i.level, i.forward, i.n_slices) for i in b.pictures()]


@pytest.mark.parametrize("path", FIXTURES, ids=[os.path.basename(p)[7:-5] for p in FIXTURES])
def test_golden_fixture_through_enqueue(path, hip_lib):
    """every fixture, one stream: enqueue returns 0, sync settles, the decoded pictures' planes are the golden ones (the pictures
    the reference consumes without decoding -- B / D / f_code 0 -- are listed and have no frame) and the picture table is decode's"""
    fx = json.load(open(path))
    es, _ = synth.generate_config(fx["config"], n_frames=fx["n_frames"], **fx["overrides"])
    n = len(fx.get("abi_frame_md5", fx["frame_md5"]))
    with jb.Batch(fx["info"]["width"], fx["info"]["height"], 1, n + 4, len(es) + 8192) as b:
        b.upload([es])
        assert b.decode() == n
        want_info = info_tuple(b)
        for rep in range(2):
            assert b.enqueue() == 0
            b.sync()
            assert b.picture_count == n
            assert info_tuple(b) == want_info
            decoded = [p for p, i in enumerate(b.pictures()) if i.decoded]
            assert len(decoded) == fx["n_frames"]
            assert [md5_planes(b.read_frame(p)) for p in decoded] == fx["frame_md5"], (os.path.basename(path), rep)
            assert b.timings()["host_ms"] == 0.0


ENC = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "enc1080", "frames_enc1080_*.json")))
END = np.frombuffer(bytes([0, 0, 1, 0xB7]), np.uint8)


def test_coded_video_gops_and_their_rotation_into_sixteen_streams(hip_lib):
    """the four encoder-made 1080p GOPs (coded video: long intra slices, the parse's critical-picture rule) through enqueue: as
    four streams, and rotated into 16 streams of all four GOPs -- which the device orders BY STREAMS at the engine's own setting
    (group from the geometry, the distance rule), status 0 -- every picture against the golden vectors"""
    assert len(ENC) == 4
    cases = []
    for path in ENC:
        fx = json.load(open(path))
        es = np.fromfile(os.path.join(os.path.dirname(path), fx["case"] + ".m1v"), dtype=np.uint8)
        assert hashlib.md5(es.tobytes()).hexdigest() == fx["es_md5"]
        cases.append((fx, es))
    rot = [np.concatenate([cases[(k + r) % 4][1][:-4] for k in range(4)] + [END]) for r in range(4)]
    for streams, want, ordered in (([es for _, es in cases], [fx["frame_md5"] for fx, _ in cases], False),
                                   ([rot[s % 4] for s in range(16)],
                                    [sum((cases[(k + s % 4) % 4][0]["frame_md5"] for k in range(4)), []) for s in range(16)], True)):
        total = sum(len(w) for w in want)
        with jb.Batch(1920, 1080, len(streams), total + 8, sum(len(s) for s in streams) + 64 * len(streams) + 4096) as b:
            b.upload(streams)
            assert b.enqueue() == 0
            b.sync()
            assert b.picture_count == total
            info = b.recon_info()
            if ordered:
                assert info["launches"] == 1 and info["status"] == 0 and info["group"] == 2, info
            got = {}
            for p, i in enumerate(b.pictures()):
                got.setdefault(i.stream, []).append(p)
            for s, w in enumerate(want):
                ps = got[s] if not ordered or s % 5 == 0 else got[s][::7]
                ws = w if not ordered or s % 5 == 0 else w[::7]
                assert [md5_planes(b.read_frame(p)) for p in ps] == ws, s


def test_sixteen_streams_take_the_ordered_launch_and_a_narrow_batch_status_8(hip_lib, libs):
    streams, want = [], []
    for s in range(16):
        es, offs = synth.generate_config("cfg1_720p", n_frames=24, stream=s % 4, width=640, height=368, gop=(6 if s % 2 else 12))
        streams.append(es)
        want += oracle_hashes(libs, es)
    os.environ["JSMPEG_HIP_RECON_ORDER"] = "2"          # (read when a batch is created: two streams of a class in lockstep)
    try:
        b = jb.Batch(640, 368, 16, len(want) + 8, sum(len(s) for s in streams) + 8192)
    finally:
        os.environ.pop("JSMPEG_HIP_RECON_ORDER", None)
    with b:
        b.upload(streams)
        for rep in range(2):
            assert b.enqueue() == 0
            b.sync()
            info = b.recon_info()
            assert info["launches"] == 1 and info["status"] == 0 and info["group"] == 2, info
            assert [int(h) for h in b.frame_hashes()] == want
            c = b.counters()
            assert c["pictures"] == len(want) and c["decoded"] == len(want)
    # ragged and narrow: 3 streams of different lengths, each one GOP -- nothing the device can deal: planned at sync
    streams, want = [], []
    for s, n in enumerate((40, 9, 17)):
        es, _ = synth.generate_config("cfg1_720p", n_frames=n, stream=s, width=176, height=144, gop=64)
        streams.append(es)
        want += oracle_hashes(libs, es)
    with jb.Batch(176, 144, 3, len(want) + 8, sum(len(s) for s in streams) + 8192) as b:
        b.upload(streams)
        assert b.enqueue() == 0
        b.sync()
        assert b.recon_info()["status"] == 8
        assert [int(h) for h in b.frame_hashes()] == want


def _sleep_cycles_for(torch, seconds):
    """torch.cuda._sleep's cycles for `seconds` on this GPU (calibrated; fails, never skips, if it cannot get there)"""
    cycles = 1 << 20
    for _ in range(12):
        a, z = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        torch.cuda._sleep(cycles)
        z.record()
        z.synchronize()
        ms = a.elapsed_time(z)
        if ms >= 50:
            return int(cycles * seconds * 1000.0 / ms)
        cycles *= 4
    raise AssertionError("torch.cuda._sleep cannot be calibrated to %.1f s" % seconds)


def test_enqueue_does_not_wait_for_the_device(hip_lib, libs):
    torch = pytest.importorskip("torch")
    es, _ = synth.generate_config("cfg1_720p", n_frames=24, stream=1, width=352, height=288)
    want = oracle_hashes(libs, es)
    cycles = _sleep_cycles_for(torch, 0.5)
    st = torch.cuda.Stream()
    with jb.Batch(352, 288, 8, 8 * 24 + 8, 8 * (len(es) + 64) + 8192) as b:
        b.upload([es] * 8)
        b.decode(stream=st.cuda_stream)
        for call, bound in (("enqueue", None), ("decode", None)):
            with torch.cuda.stream(st):
                torch.cuda._sleep(cycles)
            took = {}

            def run():
                t0 = time.perf_counter()
                took["rc"] = getattr(b, call)(stream=st.cuda_stream) if call == "enqueue" else b.decode(stream=st.cuda_stream, sync=False)
                took["s"] = time.perf_counter() - t0
            th = threading.Thread(target=run)
            th.start()
            th.join(30)
            ev = torch.cuda.Event()
            ev.record(st)
            if call == "enqueue":
                assert took["rc"] == 0 and took["s"] < 0.125, took
                assert not ev.query(), "the stream drained while enqueue ran: it waited"
                assert b.query() is False                 # the pass is behind the sleep: query says so and does not wait
            else:
                assert took["s"] > 0.3, took          # decode waits for the index behind the sleep
            b.sync()
            assert b.query() is True
            assert [int(h) for h in b.frame_hashes()] == want * 8


def test_two_batches_in_flight_from_one_thread(hip_lib, libs):
    torch = pytest.importorskip("torch")
    es_a, _ = synth.generate_config("cfg1_720p", n_frames=30, stream=1, width=352, height=288, gop=10)
    es_b, _ = synth.generate_config("cfg1_720p", n_frames=18, stream=2, width=640, height=368, gop=6)
    want_a, want_b = oracle_hashes(libs, es_a) * 8, oracle_hashes(libs, es_b) * 12
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    with jb.Batch(352, 288, 8, len(want_a) + 8, 8 * (len(es_a) + 64) + 8192) as a, \
         jb.Batch(640, 368, 12, len(want_b) + 8, 12 * (len(es_b) + 64) + 8192) as b:
        a.upload([es_a] * 8)
        b.upload([es_b] * 12)
        assert a.enqueue(stream=sa.cuda_stream) == 0
        for k in range(4):
            assert b.enqueue(stream=sb.cuda_stream) == 0
            a.sync()
            assert [int(h) for h in a.frame_hashes()] == want_a, k
            if k < 3:
                assert a.enqueue(stream=sa.cuda_stream) == 0
            b.sync()
            assert [int(h) for h in b.frame_hashes()] == want_b, k


def test_an_overflow_fails_at_sync_with_decodes_message(hip_lib, libs):
    es, _ = synth.generate_config("cfg1_720p", n_frames=20, stream=3, width=176, height=144)
    want = oracle_hashes(libs, es)
    with jb.Batch(176, 144, 2, 24, 2 * (len(es) + 64) + 8192) as b:
        b.upload([es, es])                      # 40 pictures in a table of 24
        with pytest.raises(RuntimeError) as e_dec:
            b.decode()
        assert b.enqueue() == 0
        with pytest.raises(RuntimeError) as e_enq:
            b.sync()
        assert "overflow" in str(e_enq.value) and str(e_enq.value) == str(e_dec.value)
        b.upload([es])
        assert b.enqueue() == 0
        b.sync()
        assert [int(h) for h in b.frame_hashes()] == want


def test_fallbacks_return_1_and_decode(hip_lib, libs):
    es, _ = synth.generate_config("cfg1_720p", n_frames=12, stream=4, width=176, height=144, gop=6)
    want = oracle_hashes(libs, es)
    with jb.Batch(176, 144, 8, 8 * 12 + 8, 8 * (len(es) + 64) + 8192) as b:
        b.upload([es] * 8)
        b.set_reconstruct("levels")
        assert b.enqueue() == 1
        b.sync()
        assert [int(h) for h in b.frame_hashes()] == want * 8
        b.set_reconstruct("auto")
        b.link_streams([-1] * 8)
        assert b.enqueue() == 1
        b.sync()
        assert [int(h) for h in b.frame_hashes()] == want * 8


def test_a_pass_in_flight_refuses_uploads_and_a_second_enqueue(hip_lib, libs):
    es, _ = synth.generate_config("cfg1_720p", n_frames=12, stream=5, width=176, height=144)
    want = oracle_hashes(libs, es)
    with jb.Batch(176, 144, 8, 8 * 12 + 8, 8 * (len(es) + 64) + 8192) as b:
        b.upload([es] * 8)
        assert b.enqueue() == 0
        for call in (lambda: b.enqueue(), lambda: b.upload([es]), lambda: b.decode(), lambda: b.link_streams([-1] * 8),
                     lambda: b.seed_stream(0, None, None)):
            with pytest.raises(RuntimeError, match="in flight"):
                call()
        assert b.picture_count == 8 * 12          # a reader settles the pass first
        b.sync()
        assert [int(h) for h in b.frame_hashes()] == want * 8
        while not b.query():
            time.sleep(0.001)
        b.upload([es])
        assert b.enqueue() == 0 and b.picture_count == 12


def test_a_flagged_enqueued_launch_is_done_over(hip_lib):
    code = r'''
import hashlib, json, os, sys
sys.path.insert(0, %r)
from jsmpeg_amd import batch as jb, synth
fx = json.load(open(os.path.join(%r, "tests", "golden", "frames_long_gop_p_chain.json")))
es, _ = synth.generate_config(fx["config"], n_frames=fx["n_frames"], **fx["overrides"])
with jb.Batch(fx["info"]["width"], fx["info"]["height"], 8, 8 * fx["n_frames"] + 4, 8 * (len(es) + 64) + 8192) as b:
    b.upload([es] * 8)
    assert b.enqueue() == 0
    b.sync()
    info = b.recon_info()
    print("INFO", info)
    assert info["status"] in (1, 2, 3) and info["launches"] > 1
    for p in range(8 * fx["n_frames"]):
        h = hashlib.md5()
        for plane in b.read_frame(p):
            h.update(plane.tobytes())
        assert h.hexdigest() == fx["frame_md5"][p %% fx["n_frames"]], p
    assert b.enqueue() == 1                   # demoted: level by level from now on
    b.sync()
print("DONE")
''' % (ROOT, ROOT)
    env = dict(os.environ, JSMPEG_HIP_RECON_BREAK="8", JSMPEG_HIP_RECON_PATIENCE="2000", JSMPEG_HIP_RECON_ORDER="2")
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "DONE" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    assert "flagged itself" in r.stderr
