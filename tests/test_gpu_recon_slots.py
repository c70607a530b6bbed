"""The reconstruct's SLOT PACKING (kernels.hip jm_recon_tile: which blocks of a tile need the transform, their rank by ballot
across four wavefronts, the low-frequency class in front of the rest, the blocks that find no slot and take the later passes,
the wavefront that withholds its row stores meanwhile) exists on the device only.  Here every tile form holds chosen counts of
both classes at chosen lanes (tests/craft_es.py sweep_stream; tests/test_craft_es.py checks on the CPU that the pairs visit
every branch a tile can reach, and that oracle, simulator and the reference's C agree on the streams), and every way into the
three kernels is held against the oracle's decode of the same bytes: the batch as created, per-level launches with the dense
form off (k_recon_intra with later passes, k_recon) and on (k_recon_intra_dense), sixteen copies in one ordered launch, the
one-picture interface (k_recon for intra pictures too), enqueue + sync.  A failure names the picture, the tile's (A, B,
placement) and the first differing block.  A failure here over a green simulator points at the packing.

One more test forces the reconstruct's forms over the golden fixtures, as test_gpu_parity does for the parse's.

The ten streams are written once per module (8 s) and decoded once by the oracle (6 s).  Needs an MI355X."""
import glob
import hashlib
import json
import os

import numpy as np
import pytest

import craft_es as C
from conftest import ROOT
from jsmpeg_amd import batch as jb
from jsmpeg_amd import cabi, hashing, synth
from test_gpu_ordered import order_env

pytestmark = pytest.mark.gpu

CASES = [(w, h, p) for (w, h) in C.SWEEP_SHAPES for p in (0, 1)]
IDS = ["%dx%d-%s" % (w, h, "predicted" if p else "intra") for w, h, p in CASES]
_want = {}


def expected(libs, case):
    """the oracle's pictures of a sweep stream, once: (stream, planes per picture, device-style hash per picture)"""
    if case not in _want:
        S = C.sweep_stream(*case)
        frames, _, _ = cabi.decode_stream(libs["oracle"], S["es"], keep="planes")
        assert len(frames) == len(S["plan"])
        _want[case] = (S, frames, [hashing.frame_hash(*f) for f in frames])
    return _want[case]


def explain(case, p, got, want):
    """picture p differs: which tile, which (A, B, placement), which block first"""
    S = C.sweep_stream(*case)
    w, h = case[0], case[1]
    mbw = (w + 15) >> 4
    tiles = C.tiles_of(w, h)
    for plane, (g, e) in enumerate(zip(got, want)):              # Y, Cr, Cb
        bad = np.flatnonzero(np.asarray(g).ravel() != np.asarray(e).ravel())
        if len(bad) == 0:
            continue
        stride = mbw * 16 if plane == 0 else mbw * 8
        y, x = divmod(int(bad[0]), stride)
        bx, by = x >> 3, y >> 3
        if plane == 0:
            mb, blk = (by >> 1) * mbw + (bx >> 1), ((by & 1) << 1) | (bx & 1)
        else:
            mb, blk = by * mbw + bx, 5 if plane == 1 else 4        # block 4 is the Cb plane, the third
        where = [(t, lane) for t, tl in enumerate(tiles) for lane, m, b in tl["lanes"] if (m, b) == (mb, blk)]
        t, lane = where[0]
        plan = S["plan"][p]
        counts = C.tile_counts(S["desc"], p, tiles)[t]
        return ("picture %d (%s), plane %d, pixel (%d, %d): macroblock %d block %d = tile %d (%s) lane %d, class %d; the tile's (A, B) = (%d, %d), planned %s; "
                "%d bytes of the plane differ, got %d want %d" % (p, S["desc"]["pictures"][p]["type"], plane, x, y, mb, blk, t, tiles[t]["kind"], lane,
                                                                  dict(counts[2])[lane], counts[0], counts[1], plan[t] if plan else "(reference picture)",
                                                                  len(bad), int(np.asarray(g).ravel()[bad[0]]), int(np.asarray(e).ravel()[bad[0]])))
    return "picture %d: hashes differ, planes do not" % p


def check_batch(b, case, libs, copies=1):
    S, frames, want = expected(libs, case)
    n = len(want)
    assert b.picture_count == copies * n
    dev = [int(x) for x in b.frame_hashes()]
    for p in range(copies * n):
        if dev[p] != want[p % n]:
            raise AssertionError(explain(case, p % n, b.read_frame(p), frames[p % n]) + " (copy %d)" % (p // n))


def new_batch(case, es, copies=1):
    n = len(C.sweep_stream(*case)["plan"])
    return jb.Batch(case[0], case[1], copies, copies * n + 4, copies * (len(es) + 64) + 8192)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_sweep_batch_as_created(case, hip_lib, libs):
    S, _, _ = expected(libs, case)
    with new_batch(case, S["es"]) as b:
        b.upload([S["es"]])
        assert b.decode() == len(S["plan"])
        check_batch(b, case, libs)


@pytest.mark.parametrize("dense", [0, 1], ids=["slots_220", "dense"])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_sweep_level_by_level(case, dense, hip_lib, libs):
    """per-level launches: the intra pictures through k_recon_intra (220 slots, later passes) or k_recon_intra_dense (a slot per
    lane), the predicted ones through k_recon"""
    S, _, _ = expected(libs, case)
    with order_env(JSMPEG_HIP_RECON_DENSE=dense):
        b = new_batch(case, S["es"])
    with b:
        b.set_reconstruct("levels")
        b.upload([S["es"]])
        assert b.decode() == len(S["plan"])
        info = b.recon_info()
        assert info["launches"] == (2 if case[2] else 1) and info["group"] == 0 and info["status"] == 0, info
        check_batch(b, case, libs)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_sweep_sixteen_streams_in_one_ordered_launch(case, hip_lib, libs):
    S, _, _ = expected(libs, case)
    with order_env(JSMPEG_HIP_RECON_ORDER=2, JSMPEG_HIP_RECON_DENSE=0):
        b = new_batch(case, S["es"], 16)
    with b:
        b.upload([S["es"]] * 16)
        assert b.decode() == 16 * len(S["plan"])
        info = b.recon_info()
        assert info["launches"] == 1 and info["status"] == 0 and info["group"] == (2 if case[2] else 0), info
        check_batch(b, case, libs, 16)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_sweep_one_picture_interface(case, hip_lib, libs, monkeypatch):
    """a picture per decode(), no decode-ahead: k_recon for every picture, the intra ones too"""
    S, frames, _ = expected(libs, case)
    monkeypatch.setenv("JSMPEG_HIP_DECODE_AHEAD", "0")
    got, _, _ = cabi.decode_stream(hip_lib, S["es"], keep="planes")
    assert len(got) == len(frames)
    for p in range(len(frames)):
        if any(not np.array_equal(g, e) for g, e in zip(got[p], frames[p])):
            raise AssertionError(explain(case, p, got[p], frames[p]))


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_sweep_enqueue_and_sync(case, hip_lib, libs):
    S, _, _ = expected(libs, case)
    with new_batch(case, S["es"]) as b:
        b.upload([S["es"]])
        assert b.enqueue() == 0
        b.sync()
        check_batch(b, case, libs)


@pytest.mark.parametrize("dense", [0, 1], ids=["slots_220", "dense"])
def test_reconstruct_forms_match_golden(dense, hip_lib):
    """every fixture of moderate size level by level with the dense form forced off and on (left to themselves the launches pick
    it by the intra pictures' bytes per macroblock)"""
    seen = 0
    for path in sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "frames_*.json"))):
        fx = json.load(open(path))
        if fx["n_frames"] * fx["info"]["coded_size"] > 40e6 or "abi_frame_md5" in fx:
            continue
        es, _ = synth.generate_config(fx["config"], n_frames=fx["n_frames"], **fx["overrides"])
        with order_env(JSMPEG_HIP_RECON_DENSE=dense):
            b = jb.Batch(fx["info"]["width"], fx["info"]["height"], 1, fx["n_frames"] + 2, len(es) + 1024)
        with b:
            b.set_reconstruct("levels")
            b.upload([es])
            assert b.decode() == fx["n_frames"]
            assert b.recon_info()["group"] == 0
            for p in range(fx["n_frames"]):
                h = hashlib.md5()
                for plane in b.read_frame(p):
                    h.update(plane.tobytes())
                assert h.hexdigest() == fx["frame_md5"][p], (os.path.basename(path), p)
        seen += 1
    assert seen >= 15
