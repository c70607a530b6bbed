"""Selected frames only (jsmpeg_hip_batch_select) without a GPU: select_plan.h -- the rules k_select (kernels.hip) runs behind
the index -- compiled by g++ into a TEST-ONLY simulator (tests/sim/sim_select.cpp).  The scan form, run chunk by chunk as the
kernel runs it, against its sequential definition and against a brute-force closure in Python that follows `forward` from
every selected picture; the widening rule on made-up cover counts; the library's exports and Batch.select's argument check."""
import ctypes
import glob
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "jsmpeg_amd", "csrc")
NONE = 0xffffffff
DROPPED, SELECTED = 1, 2
I, P, B = 1, 2, 3


@pytest.fixture(scope="module")
def sim():
    so = os.path.join(ROOT, "tests", "sim", "libjsmpeg_sim_select.so")
    src = os.path.join(ROOT, "tests", "sim", "sim_select.cpp")
    deps = [src] + glob.glob(os.path.join(CSRC, "*.h")) + [os.path.join(ROOT, "include", "jsmpeg_hip.h")]
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wno-unknown-pragmas", "-I", CSRC,
                               "-I", os.path.join(ROOT, "include"), "-o", so, src])
    lib = ctypes.CDLL(so)
    vp, u32 = ctypes.c_void_p, ctypes.c_uint32
    lib.sim_select.restype = ctypes.c_int
    lib.sim_select.argtypes = [u32, u32] + [vp] * 8 + [u32] + [vp] * 9
    lib.sim_select_widen.restype = ctypes.c_int
    lib.sim_select_widen.argtypes = [u32, u32] + [vp] * 6 + [u32, vp, vp]
    return lib


def make_table(rng):
    """a whole decode's picture table: streams of 1 .. 700 pictures, GOPs of 1 .. 40, skipped pictures sprinkled in, now and
    then a stream without a sequence header (nothing decoded) or one that begins with P pictures"""
    n_streams = int(rng.integers(1, 5))
    lo, hi, decoded, types, nslices = [], [], [], [], []
    for s in range(n_streams):
        n = int(rng.integers(1, 701)) if rng.random() < 0.5 else int(rng.integers(1, 60))
        gop = int(rng.integers(1, 41))
        headerless = rng.random() < 0.08
        skip_rate = float(rng.choice([0.0, 0.05, 0.3]))
        phase = int(rng.integers(0, gop)) if rng.random() < 0.2 else 0       # the stream's first pictures are P pictures
        lo.append(len(decoded))
        for k in range(n):
            t = I if (k + phase) % gop == 0 else P
            dec = not headerless
            if rng.random() < skip_rate:
                if rng.random() < 0.5:
                    t = B                                                    # B / D: consumed, not decoded
                dec = False                                                  # (a P picture with f_code 0 otherwise)
            types.append(t)
            decoded.append(1 if dec else 0)
            nslices.append(int(rng.integers(1, 5)))
        hi.append(len(decoded))
    return dict(n_streams=n_streams, lo=lo, hi=hi, decoded=decoded, types=types, nslices=nslices)


def make_requests(rng, t):
    """empty, full, duplicate and out-of-range requests among the ordinary ones"""
    reqs = []
    for s in range(t["n_streams"]):
        n_dec = sum(t["decoded"][t["lo"][s]:t["hi"][s]])
        kind = rng.random()
        if kind < 0.15:
            continue                                                         # a stream nobody asks for
        if kind < 0.25:
            reqs += [(s, f) for f in range(n_dec)]                           # all of it
            continue
        k = int(rng.integers(1, 7))
        fr = [int(rng.integers(0, max(1, n_dec))) for _ in range(k)]
        if rng.random() < 0.3:
            fr += fr[:1]                                                     # a repeat
        if rng.random() < 0.3:
            fr.append(n_dec + int(rng.integers(0, 50)))                      # no such frame
        reqs += [(s, f) for f in fr]
    order = rng.permutation(len(reqs))
    return [reqs[i] for i in order]


def layout(t, reqs, cap=1 << 20):
    nbits = [0] * t["n_streams"]
    for s, f in reqs:
        if f < cap:
            nbits[s] = max(nbits[s], f + 1)
    off = [0]
    for s in range(t["n_streams"]):
        off.append(off[-1] + ((nbits[s] + 31) & ~31))
    bits = np.zeros(max(1, off[-1] // 32), dtype=np.uint32)
    for s, f in reqs:
        if f < cap:
            i = off[s] + f
            bits[i >> 5] |= np.uint32(1 << (i & 31))
    return bits, np.array(off, dtype=np.uint32), np.array(nbits + [0], dtype=np.uint32)


def brute_force(t, reqs):
    n = len(t["decoded"])
    fwd, level, before_last = [-1] * n, [0] * n, [-1] * n
    frames = []                                                              # per stream: its decoded pictures
    for s in range(t["n_streams"]):
        dec = [p for p in range(t["lo"][s], t["hi"][s]) if t["decoded"][p]]
        frames.append(dec)
        for i, p in enumerate(dec):
            if t["types"][p] == P and i > 0:
                fwd[p], level[p] = dec[i - 1], level[dec[i - 1]] + 1
            if i >= 2:
                before_last[p] = dec[i - 2]
    req_pic = [frames[s][f] if f < len(frames[s]) else None for s, f in reqs]
    needed = set()
    for p in req_pic:
        while p is not None and p >= 0 and p not in needed:
            needed.add(p)
            p = fwd[p]
    return dict(fwd=fwd, level=level, before_last=before_last, req_pic=req_pic, needed=needed, frames=frames,
                selected={p for p in req_pic if p is not None})


def run_sim(sim, t, reqs, width):
    n = len(t["decoded"])
    bits, off, nbits = layout(t, reqs)
    a = lambda x, d: np.ascontiguousarray(x, dtype=d)
    lo, hi = a(t["lo"], np.uint32), a(t["hi"], np.uint32)
    dec, typ, nsl = a(t["decoded"], np.uint8), a(t["types"], np.uint8), a(t["nslices"], np.uint32)
    out = dict(decoded=np.zeros(n, np.uint8), pad=np.zeros(n, np.uint32), fwd=np.zeros(n, np.int32), level=np.zeros(n, np.int32),
               nslices=np.zeros(n, np.uint32), frame_pic=np.full(max(1, int(off[-1])), 0x55555555, np.uint32),
               before_last=np.full(n, -7, np.int32), sc_owner=np.zeros(max(1, int(nsl.sum())), np.uint32), totals=np.zeros(3, np.uint32))
    assert sim.sim_select(n, t["n_streams"], lo.ctypes.data, hi.ctypes.data, dec.ctypes.data, typ.ctypes.data, nsl.ctypes.data,
                          bits.ctypes.data, off.ctypes.data, nbits.ctypes.data, width,
                          *[out[k].ctypes.data for k in ("decoded", "pad", "fwd", "level", "nslices", "frame_pic", "before_last",
                                                         "sc_owner", "totals")]) == 0
    out["off"], out["nbits"] = off, nbits
    return out


def check_against_brute_force(t, reqs, out, bf):
    n = len(t["decoded"])
    assert out["fwd"].tolist() == bf["fwd"] and out["level"].tolist() == bf["level"]
    assert {p for p in range(n) if out["decoded"][p]} == bf["needed"]
    for p in range(n):
        whole = t["decoded"][p]
        assert bool(out["pad"][p] & DROPPED) == bool(whole and p not in bf["needed"])
        assert bool(out["pad"][p] & SELECTED) == (p in bf["selected"])
        assert out["nslices"][p] == (t["nslices"][p] if p in bf["needed"] else 0)
    assert out["before_last"].tolist() == bf["before_last"]
    for (s, f), want in zip(reqs, bf["req_pic"]):
        got = int(out["frame_pic"][out["off"][s] + f]) if f < out["nbits"][s] else NONE
        assert got == (NONE if want is None else want)
    # the slice codes: a needed picture keeps its own, a dropped one's go back to nobody
    k = 0
    for p in range(n):
        if not t["decoded"][p]:
            continue
        for _ in range(t["nslices"][p]):
            assert out["sc_owner"][k] == (p if p in bf["needed"] else NONE)
            k += 1
    assert out["totals"].tolist() == [len(bf["needed"]), sum(t["nslices"][p] for p in bf["needed"]),
                                      max([bf["level"][p] + 1 for p in bf["needed"]], default=0)]


N_TABLES = 2200


def test_scan_form_is_the_sequential_definition_is_the_brute_force_closure(sim):
    rng = np.random.default_rng(20261016)
    crossed = 0
    for _ in range(N_TABLES):
        t = make_table(rng)
        reqs = make_requests(rng, t)
        bf = brute_force(t, reqs)
        seq = run_sim(sim, t, reqs, 0)
        check_against_brute_force(t, reqs, seq, bf)
        for width in (256, 5):                       # 256: the kernel's workgroup; 5: many chunks, every carry in play
            scan = run_sim(sim, t, reqs, width)
            for k in ("decoded", "pad", "nslices", "frame_pic", "before_last", "sc_owner", "totals"):
                assert np.array_equal(scan[k], seq[k]), (k, width)
        # a chain of needed pictures that crosses the 256-picture chunk boundary of its stream
        for s in range(t["n_streams"]):
            for p in range(t["lo"][s] + 256, t["hi"][s], 256):
                crossed += p in bf["needed"] and bf["fwd"][p] >= 0
    assert crossed >= 50


def test_edge_selections(sim):
    rng = np.random.default_rng(7)
    t = make_table(rng)
    for reqs in ([], [(0, 0)], [(0, 0), (0, 0)], [(0, 10 ** 6)], [(0, 0xffffffff)], [(t["n_streams"] - 1, 3)] * 4):
        bf = brute_force(t, reqs)
        for width in (0, 256, 3):
            check_against_brute_force(t, reqs, run_sim(sim, t, reqs, width), bf)


def test_widening_rule(sim):
    """A stream is widened exactly when a needed picture with unwritten macroblocks showed, in the thinned pass, another frame
    than the whole decode shows there -- always so when its before-last picture lies outside the closure; the widened selection
    is a prefix: every frame up to the stream's last needed one."""
    rng = np.random.default_rng(314)
    mb = 40
    n_widened = n_outside = n_exact_uncovered = 0
    for _ in range(600):
        t = make_table(rng)
        reqs = make_requests(rng, t)
        bf = brute_force(t, reqs)
        out = run_sim(sim, t, reqs, 256)
        n = len(t["decoded"])
        covered = np.full(n, mb, np.uint32)
        for p in bf["needed"]:
            if rng.random() < 0.06:
                covered[p] = int(rng.integers(0, mb))
        stream = np.zeros(n, np.uint32)
        for s in range(t["n_streams"]):
            stream[t["lo"][s]:t["hi"][s]] = s
        stale, widen = np.zeros(n, np.int32), np.zeros(t["n_streams"], np.uint32)
        got = sim.sim_select_widen(n, t["n_streams"], stream.ctypes.data, out["decoded"].ctypes.data, out["pad"].ctypes.data,
                                   out["fwd"].ctypes.data, out["before_last"].ctypes.data, covered.ctypes.data, mb,
                                   stale.ctypes.data, widen.ctypes.data)
        want = {}
        for s in range(t["n_streams"]):
            thin = [p for p in bf["frames"][s] if p in bf["needed"]]
            for i, p in enumerate(thin):
                used = thin[i - 2] if i >= 2 else -1
                assert stale[p] == used
                if covered[p] >= mb:
                    continue
                outside = bf["before_last"][p] >= 0 and bf["before_last"][p] not in bf["needed"]
                n_outside += outside
                if outside:
                    assert used != bf["before_last"][p]
                if used != bf["before_last"][p]:
                    want[s] = 1 + bf["frames"][s].index(thin[-1])
                else:
                    n_exact_uncovered += 1
        assert got == len(want)
        assert widen.tolist() == [want.get(s, 0) for s in range(t["n_streams"])]
        n_widened += len(want)
    assert n_widened >= 20 and n_outside >= 20 and n_exact_uncovered >= 20


def test_library_exports_the_selection_abi():
    from jsmpeg_amd import batch, build
    names = ("jsmpeg_hip_batch_select", "jsmpeg_hip_batch_selected", "jsmpeg_hip_batch_select_info")
    for name in names:
        assert name in batch.BATCH_SYMBOLS
    if not os.path.exists(build.LIB_HIP):
        build.build_hip()
    out = subprocess.run(["nm", "-D", "--defined-only", build.LIB_HIP], stdout=subprocess.PIPE, text=True, check=True).stdout
    for name in names:
        assert (" T " + name + "\n") in out, name
    header = open(os.path.join(ROOT, "include", "jsmpeg_hip.h")).read()
    for name in names:
        assert ("int " + name + "(") in header


def test_select_refuses_malformed_requests_without_a_device():
    from jsmpeg_amd.batch import Batch
    b = Batch.__new__(Batch)                         # no library, no handle: the check comes first
    for bad in (5, [(0,)], [(0, 1, 2)], [(0, -1)], [(-1, 0)], [(0, 1.5)], [("0", 0)], [(0, 1 << 32)], [None], [(True, 0)]):
        with pytest.raises(ValueError):
            b.select(bad)


def test_k_select_uses_no_scratch():
    from jsmpeg_amd import build
    import shutil
    if not shutil.which("hipcc"):
        pytest.skip("no hipcc")
    usage = build.check_kernel_resources()
    name = [k for k in usage if "k_select" in k]
    assert name and usage[name[0]].get("ScratchSize", 0) == 0
