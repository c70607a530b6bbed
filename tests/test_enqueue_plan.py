"""The device plan of an enqueued pass (jsmpeg_amd/csrc/enqueue_plan.h: what k_plan runs on one workgroup) on the CPU: the
planner's stages run one "thread" after the other (tests/sim/plan_main.cpp, built here with g++) over random picture tables --
1-300 streams, ragged GOPs, skipped pictures, streams that begin with a predicted picture, overflowed tables -- and what it
writes is checked against the host path's own functions: `stale` against jm_plan_stale, the sequence against jm_plan_ordered
(by streams, or by GOP chains after jm_plan_chains), the waits (earlier in their class), the parse's sizing against the walk and
the parse rules field by field (and against the library's jsmpeg_hip_debug_parse_plan, the decode path's jm_plan_parse)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from jsmpeg_amd import build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "jsmpeg_amd", "csrc")
KIND = {0: "host", 1: "streams", 2: "chains"}


@pytest.fixture(scope="module")
def sim(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("plan") / "libplan_sim.so")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-Wno-unknown-pragmas", "-I", CSRC,
                           "-o", out, os.path.join(ROOT, "tests", "sim", "plan_main.cpp")])
    lib = ctypes.CDLL(out)
    lib.sim_plan_check.restype = ctypes.c_int
    lib.sim_plan_check.argtypes = [ctypes.c_uint32] + [ctypes.c_void_p] * 5 + [ctypes.c_uint32] + [ctypes.c_void_p] * 3
    lib.sim_plan_message.restype = ctypes.c_char_p
    return lib


def table(rng, n_streams, pics_per_stream, p_intra=0.15, p_skip=0.1, p_first_p=0.3, gop=None):
    """a picture table as the index makes one: streams one behind the other, pictures in ES order; fwd = the stream's last
    decoded picture for a predicted one, -1 for an intra picture and for a stream's first decoded picture"""
    stream, decoded, fwd, n_slices, pos, es_end = [], [], [], [], [], []
    at = 64
    for s in range(n_streams):
        n = int(pics_per_stream if np.isscalar(pics_per_stream) else rng.integers(*pics_per_stream))
        last = -1
        for i in range(n):
            p = len(stream)
            dec = rng.random() >= p_skip
            intra = (i % gop == 0) if gop else (last < 0 and rng.random() >= p_first_p) or rng.random() < p_intra
            stream.append(s)
            decoded.append(1 if dec else 0)
            fwd.append(-1 if (not dec or intra or last < 0) else last)
            n_slices.append(int(rng.integers(1, 69)) if dec else 0)
            pos.append(at)
            at += int(rng.integers(200, 40000)) * (4 if intra else 1)
            if dec:
                last = p
        es_end.append(at)
        at += 64
    return dict(stream=stream, decoded=decoded, fwd=fwd, n_slices=n_slices, pos=pos, es_end=es_end, es_bytes=at)


def check(sim, t, group=3, tiles=200, try_streams=1, try_chains=1, streams_forced=0, chains_forced=0, brk=-1, overflow=0,
          split=-1, head=None, rows_cap=None):
    n = len(t["stream"])
    arr = lambda v, dt: np.ascontiguousarray(v, dtype=dt)
    st, de, fw, ns, po = (arr(t["stream"], np.uint32), arr(t["decoded"], np.uint8), arr(t["fwd"], np.int32),
                          arr(t["n_slices"], np.uint32), arr(t["pos"], np.uint32))
    ee = arr(t["es_end"], np.uint32)
    slices = int(ns.sum())
    head = head or (0, 0, 1, 0, 1)
    if rows_cap is None:
        rows_cap = (n + 8) * 108 // 800
    knobs = arr([group, tiles, try_streams, try_chains, streams_forced, chains_forced, brk, rows_cap, overflow,
                 slices + n + 10, slices, 1 << 22, t["es_bytes"], 8160, split, *head], np.int32)
    out = np.zeros(16, dtype=np.uint32)
    rc = sim.sim_plan_check(n, st.ctypes.data, de.ctypes.data, fw.ctypes.data, ns.ctypes.data, po.ctypes.data,
                            len(ee), ee.ctypes.data, knobs.ctypes.data, out.ctypes.data)
    assert rc == 0, sim.sim_plan_message().decode()
    return dict(kind=KIND[int(out[0])], host_kind=KIND[int(out[15])], rows=int(out[1]), lockstep=int(out[2]), lanes=int(out[3]),
                long_slices=int(out[4]), bpm=int(out[5]), split=int(out[6]), lanes_per_wave=int(out[7]), batches=int(out[8]),
                t_cold=int(out[9]), head_lanes=int(out[10]), head_batches=int(out[11]), head_end=int(out[12]))


def test_random_tables_plan_as_the_host_functions_do(sim):
    rng = np.random.default_rng(1234)
    kinds = {}
    for trial in range(160):
        n_streams = int(rng.choice([1, 2, 5, 8, 9, 16, 33, 64, 150, 300]))
        per = (1, 40) if trial % 3 else int(rng.integers(1, 30))
        t = table(rng, n_streams, per, p_intra=float(rng.choice([0.0, 0.1, 0.4])), p_skip=float(rng.choice([0.0, 0.1, 0.3])))
        r = check(sim, t, group=int(rng.integers(1, 6)), tiles=int(rng.choice([12, 80, 200, 510])),
                  streams_forced=int(rng.integers(0, 2)), brk=int(rng.integers(-1, 40)))
        kinds[r["kind"]] = kinds.get(r["kind"], 0) + 1
    assert kinds.get("streams", 0) > 10 and kinds.get("chains", 0) > 5 and kinds.get("host", 0) > 5, kinds


def test_gop_chains_of_one_long_stream_and_chains_forced(sim):
    rng = np.random.default_rng(7)
    r = check(sim, table(rng, 1, 288, gop=12, p_skip=0.0))           # one stream of 24 GOPs: dealt by GOP chains, 3 a class
    assert r["kind"] == "chains" and r["rows"] >= 30
    r = check(sim, table(rng, 64, 20, gop=10, p_skip=0.05), try_streams=0, chains_forced=1)
    assert r["kind"] == "chains"


def test_too_many_rows_defers_to_the_host(sim):
    rng = np.random.default_rng(9)
    r = check(sim, table(rng, 1, 120, p_intra=0.0, p_skip=0.0, p_first_p=0.0))   # one long chain: nothing to deal
    assert r["kind"] == "host" and r["host_kind"] == "host"
    t = table(rng, 9, 30, p_skip=0.0, p_intra=0.0, p_first_p=0.0)
    for i in range(30, 60):                                          # one stream twice as long as the others: ragged
        t["decoded"].append(1); t["stream"].append(8); t["fwd"].append(len(t["fwd"]) - 1); t["n_slices"].append(3)
        t["pos"].append(t["es_end"][-1] + 100 * i)
    t["es_end"][-1] += 100 * 61
    r = check(sim, t)
    assert r["kind"] == "host"
    r = check(sim, table(rng, 16, 10, p_skip=0.0), rows_cap=5)        # fine plan, but a grid of 5 rows: deferred
    assert r["kind"] == "host" and r["host_kind"] == "host"


def test_an_overflowed_table_plans_nothing(sim):
    rng = np.random.default_rng(3)
    r = check(sim, table(rng, 16, 12), overflow=1)
    assert r["kind"] == "host" and r["batches"] == 0 and r["lanes"] == 0


def test_parse_sizing_equals_the_decode_paths(sim):
    """the planner's figures fed to the library's jsmpeg_hip_debug_parse_plan (the decode path's jm_plan_parse) give the
    planner's launch, field by field -- with the overrides a test may force (JSMPEG_HIP_PARSE_SPLIT / _HEAD)"""
    lib = build.load_hip_library()
    f = lib.jsmpeg_hip_debug_parse_plan
    f.restype = ctypes.c_int
    f.argtypes = [ctypes.c_uint32] * 3 + [ctypes.c_int, ctypes.POINTER(ctypes.c_uint32)]
    rng = np.random.default_rng(11)
    env = dict(os.environ)
    try:
        for trial in range(40):
            split = int(rng.choice([-1, -1, 0, 1]))
            head = (1, 10, 4, 200, 16) if trial % 5 == 4 else None
            os.environ.pop("JSMPEG_HIP_PARSE_SPLIT", None)
            os.environ.pop("JSMPEG_HIP_PARSE_HEAD", None)
            if split >= 0:
                os.environ["JSMPEG_HIP_PARSE_SPLIT"] = str(split)
            if head:
                os.environ["JSMPEG_HIP_PARSE_HEAD"] = "%d,%d,%d,%d" % head[1:]
            t = table(rng, int(rng.choice([1, 4, 16, 64])), (2, 60), p_intra=0.2)
            r = check(sim, t, split=split, head=head)
            out = (ctypes.c_uint32 * 12)()
            assert f(r["lanes"], r["long_slices"], r["bpm"], 1, out) == 0
            assert (r["split"], r["lanes_per_wave"], r["batches"], r["t_cold"], r["head_lanes"], r["head_batches"], r["head_end"]) == \
                (out[0], out[1], out[2], out[5], out[6], out[7], out[8]), (trial, r, list(out))
    finally:
        os.environ.clear()
        os.environ.update(env)
