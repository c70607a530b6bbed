"""The crafted streams of tests/craft_es.py, on the CPU: that they are what they claim to be (conditions on the INPUTS: which
branches of the reconstruct's slot packing a sweep visits, how far the bounds set drives the transform, how much of it can be
seen through the clamp), and that the oracle, the simulator of the device functions and -- where it is present -- the
reference's own C agree on them.  The GPU side is tests/test_gpu_recon_slots.py and, for the committed bounds fixture, every
test that globs tests/golden/frames_*.json.

The packing itself (kernels.hip jm_recon_tile: ranks by ballot across four wavefronts, the low-frequency class in front, later
passes) runs on the device only; the accounting below restates its arithmetic to REPORT which branches a stream's (A, B) pairs
reach.  It is never an expected value: expected pictures come from the oracle.

Writing the ten sweep streams takes about 8 s here, decoding them on the oracle and the simulator about as long again."""
import hashlib
import json
import os

import numpy as np
import pytest

import craft_es as C
from conftest import ROOT, have_reference
from jsmpeg_amd import cabi
from test_sim_device_functions import sim  # noqa: F401  (the simulator library, a fixture)

WG, WAVES = 256, 4
SLOTS = {"k_recon / k_recon_intra": 220, "k_recon_intra_dense": 256}


def packing(a, b, slots):
    """the packing's arithmetic for a tile with `a` low-frequency and `b` other transform blocks -> what it decides"""
    later_pass = min(slots, WG // 2)
    up = (a + 31) & ~31
    fewer_rounds = (b + 31) // 32 < (a + b + 31) // 32 - a // 32
    fits = up + b <= slots
    first_b = up if fewer_rounds and fits else a
    total = first_b + b
    held = min(total, slots)
    rounds = [(r0 + 32 * w, r0 + 32 * w + 32 <= first_b) for r0 in range(0, held, WG // 2) for w in range(WAVES) if r0 + 32 * w < held]
    idle = [1 for r0 in range(0, max(held, 1), WG // 2) for w in range(WAVES) if r0 + 32 * w >= held]
    passes = [min(total - base, later_pass) for base in range(slots, total, later_pass)]
    return dict(first_b=first_b, total=total, rounds=rounds, passes=passes, fewer_rounds=fewer_rounds, fits=fits, held=held, idle=len(idle))


def branches(a, b, slots):
    p = packing(a, b, slots)
    out = {("a block ranks at or past the slots", p["total"] > slots), ("rounding up saves a full-transform round", p["fewer_rounds"]),
           ("second first-pass round", p["held"] > WG // 2), ("later passes", len(p["passes"])),
           ("a wavefront round past the last packed block", p["idle"] > 0)}
    if p["fewer_rounds"]:
        out.add(("rounded up start fits the slots", p["fits"]))
    out |= {("wavefront round wholly in front of the second class", low) for _, low in p["rounds"]}
    out |= {("later pass full", n == min(slots, WG // 2)) for n in p["passes"]}
    return out


def waiting_waves(classes, a, b, slots):
    """which wavefronts hold a block whose transform waits for a later pass (they withhold all their row stores)"""
    first_b = packing(a, b, slots)["first_b"]
    na = nb = 0
    waves = set()
    for lane, c in classes:
        if c == C.LOWF:
            rank, na = na, na + 1
        elif c == C.FULL:
            rank, nb = first_b + nb, nb + 1
        else:
            continue
        if rank >= slots:
            waves.add(lane // 64)
    return frozenset(waves)


def test_the_accounting_on_hand_cases():
    assert packing(20, 20, 220)["first_b"] == 32 and packing(20, 12, 220)["first_b"] == 20
    assert packing(5, 188, 220)["total"] == 220 and packing(5, 189, 220)["total"] == 194
    p = packing(0, 256, 220)
    assert p["passes"] == [36] and len(p["rounds"]) == 7 and p["idle"] == 1
    assert packing(64, 1, 220)["rounds"] == [(0, True), (32, True), (64, False)]
    assert packing(5, 225, 256)["first_b"] == 5 and packing(5, 224, 256)["first_b"] == 32 and packing(31, 193, 256)["first_b"] == 31 and packing(31, 194, 256)["first_b"] == 32


@pytest.mark.parametrize("predicted", [0, 1], ids=["intra", "predicted"])
@pytest.mark.parametrize("shape", C.SWEEP_SHAPES, ids=["%dx%d" % s for s in C.SWEEP_SHAPES])
def test_a_sweep_visits_every_branch_its_tiles_can_reach(shape, predicted):
    """per tile kind: the planned (A, B) is what the description holds, every pair of the grid is there in three placements, and
    the pairs visit every outcome of every branch of the packing that ANY (A, B) the tile can hold reaches -- for 220 slots and
    for the dense form's 256"""
    S = C.sweep_stream(shape[0], shape[1], predicted)
    tiles = C.tiles_of(*shape)
    seen, placed, waits = {}, {}, {}
    for p, plan in enumerate(S["plan"]):
        assert (S["desc"]["pictures"][p]["type"] == "P") == (bool(predicted) and plan is not None)
        if plan is None:
            continue
        counts = C.tile_counts(S["desc"], p, tiles)
        for t, (a, b, place) in zip(range(len(tiles)), plan):
            assert counts[t][:2] == (a, b), (p, t, counts[t][:2], (a, b))
            kind = tiles[t]["kind"]
            placed.setdefault(kind, set()).add((a, b, place))
            for name, slots in SLOTS.items():
                seen.setdefault((kind, name), set()).update(branches(a, b, slots))
                waits.setdefault((kind, name), set()).add(waiting_waves(counts[t][2], a, b, slots))
    for t in tiles:
        kind, cap = t["kind"], len(t["lanes"])
        assert placed[kind] == {(a, b, pl) for a, b in C.ab_grid(cap) for pl in C.PLACEMENTS}, kind
        for name, slots in SLOTS.items():
            reach = set()
            for a in range(cap + 1):
                for b in range(cap + 1 - a):
                    reach |= branches(a, b, slots)
            assert seen[(kind, name)] == reach, (kind, name, sorted(reach - seen[(kind, name)], key=str))
            if cap > slots:
                # both sides of everything the tile can reach, spelled out
                for what in ("a block ranks at or past the slots", "rounding up saves a full-transform round", "rounded up start fits the slots",
                             "wavefront round wholly in front of the second class", "second first-pass round"):
                    assert {(what, True), (what, False)} <= seen[(kind, name)], (kind, name, what)
                assert {("later passes", 0), ("later passes", 1), ("later pass full", False)} <= seen[(kind, name)]
                # the wavefront that withholds its row stores: alone, with others, all four, and none
                w = waits[(kind, name)]
                assert frozenset() in w and frozenset(range(WAVES)) in w and any(len(x) == 1 for x in w) and any(0 in x and len(x) < WAVES for x in w), (kind, name)
    # the predicted sweep holds P tiles with more transform blocks than slots, all four half-pel cases, every macroblock type,
    # both vector units and a second f_code
    if predicted:
        ps = [p for p in S["desc"]["pictures"] if p["type"] == "P"]
        assert {(mv[0] & 1, mv[1] & 1) for p in ps if not p["full_pel"] for _, kind, mv, _ in p["mbs"] if mv} == {(0, 0), (0, 1), (1, 0), (1, 1)}
        assert {kind for p in ps for _, kind, _, _ in p["mbs"]} == {"intra", "coded", "coded_mv", "mv"}
        assert {(p["full_pel"], p["f_code"]) for p in ps} >= {(0, 1), (1, 1), (0, 2)}
        assert any(a + b > 220 for plan in S["plan"] if plan for a, b, _ in plan) or max(len(t["lanes"]) for t in tiles) <= 220


def branch_report():
    """per tile kind, the branches the sweeps visit (what SUMMARY / DESIGN.md quote): python tests/test_craft_es.py"""
    for shape in C.SWEEP_SHAPES:
        S = C.sweep_stream(shape[0], shape[1], 1)
        tiles = C.tiles_of(*shape)
        for kind in sorted({t["kind"] for t in tiles}):
            got = set()
            for plan in S["plan"]:
                if plan:
                    for t, (a, b, _) in zip(tiles, plan):
                        if t["kind"] == kind:
                            got |= branches(a, b, 220)
            print("%dx%d  %-40s %s" % (shape[0], shape[1], kind, "; ".join("%s: %s" % (k, "/".join(str(v) for _, v in sorted(x for x in got if x[0] == k)))
                                                                            for k in sorted({k for k, _ in got}))))


def _md5s(frames):
    out = []
    for f in frames:
        h = hashlib.md5()
        for p in f:
            h.update(p.tobytes())
        out.append(h.hexdigest())
    return out


_oracle_cache = {}


def oracle_md5(libs, key, es):
    if key not in _oracle_cache:
        _oracle_cache[key] = cabi.decode_stream(libs["oracle"], es)[0]
    return _oracle_cache[key]


@pytest.mark.parametrize("predicted", [0, 1], ids=["intra", "predicted"])
@pytest.mark.parametrize("shape", C.SWEEP_SHAPES, ids=["%dx%d" % s for s in C.SWEEP_SHAPES])
def test_sweep_simulator_equals_oracle(shape, predicted, sim, libs):  # noqa: F811
    """the shared jm_recon_* functions, block by block, against the oracle: a GPU failure over a green simulator points at the packing"""
    S = C.sweep_stream(shape[0], shape[1], predicted)
    es, n = S["es"], len(S["plan"])
    want = oracle_md5(libs, (shape, predicted), es)
    assert len(want) == n
    mbw, mbh = (shape[0] + 15) >> 4, (shape[1] + 15) >> 4
    fb = mbw * mbh * 384
    out = np.zeros(n * fb, dtype=np.uint8)
    sim.sim_split_service(0)
    assert sim.sim_decode_stream(es.ctypes.data, len(es), shape[0], shape[1], out.ctypes.data, n) == n
    got = [hashlib.md5(out[i * fb:(i + 1) * fb].tobytes()).hexdigest() for i in range(n)]
    bad = [i for i in range(n) if got[i] != want[i]]
    assert not bad, (bad[:8], S["plan"][bad[0]])


@pytest.mark.reference
@pytest.mark.skipif(not have_reference(), reason="needs /root/reference")
@pytest.mark.parametrize("predicted", [0, 1], ids=["intra", "predicted"])
@pytest.mark.parametrize("shape", C.SWEEP_SHAPES, ids=["%dx%d" % s for s in C.SWEEP_SHAPES])
def test_sweep_reference_equals_oracle(shape, predicted, libs):
    """the reference's own C on the whole sweep: pins the oracle where the GPU tests lean on it"""
    S = C.sweep_stream(shape[0], shape[1], predicted)
    want = oracle_md5(libs, (shape, predicted), S["es"])
    got = cabi.decode_stream(libs["ref"], S["es"])[0]
    assert got == want


# ---- the transform at its bounds: tests/golden/craft_bounds_192x192.m1v ----

def bounds_fixture():
    return json.load(open(os.path.join(ROOT, "tests", "golden", "frames_%s.json" % C.BOUNDS_NAME)))


def test_bounds_stream_is_the_committed_one():
    es, offs = C.bounds_stream()
    assert len(es) < 512 * 1024
    assert es.tobytes() == open(os.path.join(ROOT, "tests", "golden", C.BOUNDS_NAME + ".m1v"), "rb").read()
    assert list(offs) == list(np.load(os.path.join(ROOT, "tests", "golden", C.BOUNDS_NAME + ".offsets.npy")))
    assert hashlib.md5(es.tobytes()).hexdigest() == bounds_fixture()["es_md5"]


def test_bounds_set_reaches_what_the_fixture_records():
    """the tool's own network, fed the set: the four figures of the fixture, all inside the tool's bounds -- and far beyond
    anything a random stream reaches (2000 random-sign full-amplitude blocks: |output| 9865, operand 1 431 202)"""
    S = C.bounds_blocks()
    assert (len(S["pixel"]), len(S["site"]), len(S["ladder"]), len(S["random"])) == (128, 192, 32, 512)
    assert all(v in (2047, -2048) for blk in S["pixel"] + S["site"] + S["random"] for v in blk)
    assert [dc for dc, _ in S["ladder"]] == [128 + 255 * i for i in range(1, 16)] + [3953] + [128 - 255 * i for i in range(1, 17)]
    fig = C.bounds_figures()
    assert fig == bounds_fixture()["bounds"], fig
    out_bound, op_bound = C.idct_bounds.main()
    assert max(fig["max_output_non_intra"], -fig["min_output_non_intra"], fig["max_abs_output_dc_ladder"]) < out_bound == 18473
    assert fig["max_operand"] < op_bound == 4364608 < 1 << 23
    # what the set is for: the column pass' results do not fit int16, the final ones need more than 15 bits
    assert fig["max_output_non_intra"] >= 14310 and fig["min_output_non_intra"] <= -14311 and fig["max_operand"] >= 1775219
    assert fig["max_abs_output_dc_ladder"] > 16384


def test_bounds_pictures_can_be_seen_through(libs):
    """extremes that clamp to 0 or 255 show a wrap, not a wrong rounding: at least 2000 pixels of the oracle's two pictures
    (every block of them is a full-amplitude one) lie strictly inside 1..254"""
    es, _ = C.bounds_stream()
    frames, _, _ = cabi.decode_stream(libs["oracle"], es, keep="planes")
    assert len(frames) == 2
    inside = sum(int(np.count_nonzero((p > 0) & (p < 255))) for f in frames for p in f)
    print("pixels inside 1..254:", inside)
    assert inside >= 2000
    assert _md5s(frames) == bounds_fixture()["frame_md5"]
    # ... and both rails are there in both pictures
    for f in frames:
        assert int(np.count_nonzero(f[0] == 0)) > 1000 and int(np.count_nonzero(f[0] == 255)) > 1000


if __name__ == "__main__":
    branch_report()
