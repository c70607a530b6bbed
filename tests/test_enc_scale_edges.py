"""The edges of the encoder's scaled input without a GPU: the weight rule of enc_scale.h over the whole contract (no weight
below 0 or above 16384, every sum exact, nothing moved where the first form was already right), the named inputs of
tests/enc_scale_inputs.py -- EDGES, CROPS, TINY, RATIOS, which tests/test_gpu_encode_scale_edges.py runs on the device -- through
the simulator and the numpy restatement, and a proof from the simulator's tile walker (sim_es_walk: k_enc_scale's own
expressions over the header's tile constants) that every named input reaches the edge of the kernel it is named for."""
import numpy as np
import pytest

import enc_scale_inputs as si
import enc_scale_ref as es

ONE = es.ONE
GRID_OUT = range(1, 9)          # with every n_in in 1 .. 4095


def sampled_pairs(n=2000, seed=31):
    """seeded (n_in, n_out, aa) outside the grid: n_in at least 512, n_out from 9 up, either direction"""
    rng = np.random.default_rng(seed)
    return [(int(rng.integers(512, 4096)), int(rng.integers(9, 4096)), int(rng.integers(0, 2))) for _ in range(n)]


def test_weights_are_0_to_16384_and_sum_exactly_over_the_whole_contract():
    """(fails on the rule before this test: 632 values of n_in from 1280 have a weight below 0 for n_out = 1, the worst -105 at
    3120, and 120 from 2870 for n_out = 2, the worst -13 at 3418)"""
    bad, second = [], {}
    pairs = [(n_in, n_out, aa) for n_out in GRID_OUT for n_in in range(1, 4096) for aa in (1, 0)] + sampled_pairs()
    for n_in, n_out, aa in pairs:
        lo, hi, exact, cum = si.axis_scan(n_in, n_out, aa)
        if lo < 0 or hi > ONE or not exact:
            bad.append((n_in, n_out, aa, lo, hi, exact))
        if cum:
            second.setdefault((n_out, aa), []).append(n_in)
    assert not bad, (len(bad), bad[:8])
    # where the second form runs: what the rule's text says, and nowhere else
    assert sorted(second) == [(1, 1), (2, 1)], sorted(second)
    assert (len(second[1, 1]), second[1, 1][0], second[1, 1][-1]) == (632, 1280, 3268)
    assert (len(second[2, 1]), second[2, 1][0], second[2, 1][-1]) == (120, 2870, 4095)


def old_axis(n_in, n_out, aa):
    """The rule as it was before the second form, kept here to show that nothing else moved: (xmin[n_out], xsize[n_out], the
    weights one index after the other, the smallest weight per index) -- the first tap of the largest W takes 16384 - sum W,
    whatever that makes of it."""
    i = np.arange(n_out, dtype=np.int64)
    c = (2 * i + 1) * n_in
    if n_in == n_out:
        return i, np.ones(n_out, np.int64), np.full(n_out, ONE, np.int64), np.full(n_out, ONE, np.int64)
    if aa and n_in > n_out:
        j = np.maximum(0, (c - 2 * n_in) // (2 * n_out) - 1)[:, None] + np.arange(2 * n_in // n_out + 5, dtype=np.int64)[None, :]
        n = 2 * n_in - np.abs((2 * j + 1) * n_out - c[:, None])
        valid = (n > 0) & (j < n_in)
        n = np.where(valid, n, 0)
    else:
        i0, r = np.divmod(np.maximum(0, c - n_out), 2 * n_out)
        one = (i0 >= n_in - 1) | (r == 0)
        j = np.minimum(i0, n_in - 1)[:, None] + np.arange(2, dtype=np.int64)[None, :]
        n = np.stack([np.where(one, 1, 2 * n_out - r), np.where(one, 0, r)], axis=1)
        valid = n > 0
    N = n.sum(axis=1, keepdims=True)
    w = (2 * ONE * n + N) // (2 * N)
    rows = np.arange(n_out)
    w[rows, np.argmax(w, axis=1)] += ONE - w.sum(axis=1)
    return j[rows, np.argmax(valid, axis=1)], valid.sum(axis=1), w[valid], np.where(valid, w, ONE).min(axis=1)


def test_nothing_else_moved():
    """the table the kernel reads still holds the functions' weights over the whole grid (plan check 6 fired at 3037 -> 3 x 1
    and 3111 -> 16 x 1 before), and every output index the old rule left non-negative keeps its old weights"""
    for n_out in GRID_OUT:
        for aa in (1, 0):
            wrong = [(n_in, rc) for n_in in range(1, 4096) for rc in [si.plan_check(n_in, 1, n_out, 1, None, aa)[0]] if rc]
            assert not wrong, (n_out, aa, len(wrong), wrong[:8])
    assert si.plan_check(3037, 3, 1, 1)[0] == 0 and si.plan_check(3111, 16, 1, 1)[0] == 0
    kept = moved = 0
    for n_in, n_out, aa in [(n_in, n_out, aa) for n_out in GRID_OUT for n_in in range(1, 4096) for aa in (1, 0)] + sampled_pairs():
        xmin, xsize, w, lo = old_axis(n_in, n_out, aa)
        got_min, got_size, got_w = si.sim_axis(n_in, n_out, aa)
        assert np.array_equal(got_min, xmin) and np.array_equal(got_size, xsize), (n_in, n_out, aa)
        if lo.min() >= 0:
            assert np.array_equal(got_w, w), (n_in, n_out, aa)
            kept += 1
        else:
            same = np.repeat(lo >= 0, xsize)
            assert np.array_equal(got_w[same], w[same]) and not np.array_equal(got_w[~same], w[~same]), (n_in, n_out, aa)
            moved += 1
    assert moved == 632 + 120 and kept == 2 * 8 * 4095 + 2000 - moved, (kept, moved)


def test_second_form_is_the_restatement_s():
    """the header's closed form of the running sums against the restatement's plain cumulative sum, at the ends and the
    worst of each failing range"""
    for n_in, n_out in ((1280, 1), (3120, 1), (3268, 1), (2870, 2), (3418, 2), (4095, 2)):
        want = es.axis_taps(n_in, n_out, 1)
        xmin, xsize, w = si.sim_axis(n_in, n_out, 1)
        assert si.axis_scan(n_in, n_out, 1)[3] == n_out
        assert [(int(a), len(ws)) for a, ws in want] == list(zip(xmin.tolist(), xsize.tolist())), (n_in, n_out)
        assert [v for _, ws in want for v in ws] == w.tolist(), (n_in, n_out)
        assert w.min() >= 0 and all(sum(ws) == ONE for _, ws in want)


NAMED = si.named_geometries()


@pytest.mark.parametrize("name,geo", NAMED, ids=[n for n, _ in NAMED])
def test_named_inputs_simulator_equals_restatement(name, geo):
    w, h, crop, ow, oh, aa = geo
    frames = si.geometry_frames(w, h)
    assert all(f.nbytes < 300 * 1000 for f in frames) and not np.array_equal(frames[0], frames[1])
    for k, (f, want) in enumerate(zip(frames, si.geometry_want(geo))):
        got = si.sim_frame(f, w, h, ow, oh, crop, aa)
        assert got is not None and np.array_equal(got, want), (name, k)
    rc, plan = si.plan_check(w, h, ow, oh, crop, aa)
    assert rc == 0 and plan["words"] <= plan["bound"] and plan["rows"] >= 4, (name, rc, plan)


def test_ratios_are_on_the_second_form_where_they_say():
    """RATIOS come from the scan: each failing axis is one the first form left negative, the others are not"""
    second = lambda n_in, n_out: si.axis_scan(n_in, n_out, 1)[3] > 0
    for name, (w, h, crop, ow, oh, aa) in si.RATIOS.items():
        assert aa == 1 and crop is None and min(w, h) == 2, name
        luma, chroma = (second(w, ow), second(h, oh)), (second((w + 1) >> 1, (ow + 1) >> 1), second((h + 1) >> 1, (oh + 1) >> 1))
        if name.startswith("chroma_only"):
            assert luma == (False, False) and chroma == (True, False), name
        elif name.startswith("vertical"):
            assert luma == (False, True), name
        else:
            assert luma == (True, False), name


def walks(names_and_geos):
    return [(name, r) for name, (w, h, crop, ow, oh, aa) in names_and_geos for r in si.walk(w, h, ow, oh, crop, aa)]


def test_walker_agrees_with_the_plan():
    """the walker's records are the plan's tiles, in the kernel's order: luma, Cr, Cb, row by row"""
    for name, (w, h, crop, ow, oh, aa) in NAMED:
        recs = si.walk(w, h, ow, oh, crop, aa)
        cw, ch = es.coded(ow, oh)
        assert len(recs) == si.plan_check(w, h, ow, oh, crop, aa)[1]["tiles"], name
        assert [r["kind"] for r in recs] == sorted(r["kind"] for r in recs)
        for kind, (pw, ph) in enumerate(((cw, ch), (cw // 2, ch // 2), (cw // 2, ch // 2))):
            mine = [r for r in recs if r["kind"] == kind]
            assert sum(r["nw"] * r["nh"] for r in mine) == pw * ph, (name, kind)
            assert [(r["ty"], r["tx"]) for r in mine] == sorted((r["ty"], r["tx"]) for r in mine)
        for r in recs:
            assert r["stride"] % (8 if r["kind"] else 16) == 0 and r["stride"] * r["cr_max"] <= 16384 and 1 <= r["last_rows"] <= r["cr_max"] <= 32
            assert r["chunks"] >= 1 and r["straddle"] <= r["nh"] and (r["chunks"] > 1 or r["straddle"] == 0)
        assert [dict(r, kind=2) for r in recs if r["kind"] == 1] == [r for r in recs if r["kind"] == 2], "Cr and Cb walk alike"


# what each of EDGES is named for: name -> a predicate over its records (luma: kind 0, chroma: kind 1)
def _any(recs, kind, **want):
    return any(r["kind"] == kind and all(r[k] == v for k, v in want.items()) for r in recs)


EDGE_CLASSES = {
    "stride_4096_cr_4": lambda r: _any(r, 0, stride=4096, cr_max=4, chunks=10, straddle=18) and _any(r, 1, stride=2048, cr_max=8),
    "identity_rows_cr_4": lambda r: _any(r, 0, cr_max=4, ty=0, straddle=0, chunks=8) and _any(r, 0, ty=1, chunks=1, last_rows=1) and _any(r, 1, last_rows=1),
    "cr_7_last_chunk_6": lambda r: _any(r, 0, cr_max=7, last_rows=6, straddle=13) and _any(r, 1, cr_max=15) and _any(r, 0, ty=1, nh=16),
    "cr_30_full_tile": lambda r: _any(r, 0, cr_max=30, nw=128, ty=0) and _any(r, 0, cr_max=30, ty=1),
    "three_columns_aa": lambda r: _any(r, 0, tx=2, nw=16, replicated=1) and _any(r, 1, tx=1, nw=8) and _any(r, 1, last_rows=1) and _any(r, 0, tx=2, ty=1, replicated=3),
    "three_columns_plain": lambda r: _any(r, 0, tx=2, nw=16, replicated=1) and _any(r, 1, tx=1, nw=8) and _any(r, 0, tx=2, ty=1, replicated=3),
    "upscale_300x40": lambda r: [x["nw"] for x in r if x["kind"] == 0 and x["ty"] == 0] == [128, 128, 48] and [x["nw"] for x in r if x["kind"] == 1] == [128, 24]
    and all(x["chunks"] == 1 for x in r),
    "tall_125_to_1": lambda r: _any(r, 0, chunks=15, cr_max=32, straddle=27) and _any(r, 0, chunks=15, straddle=28) and _any(r, 0, ty=2),
}


@pytest.mark.parametrize("name", sorted(si.EDGES))
def test_each_edge_reaches_what_it_is_named_for(name):
    w, h, crop, ow, oh, aa = si.EDGES[name]
    recs = si.walk(w, h, ow, oh, crop, aa)
    assert EDGE_CLASSES[name](recs), (name, recs)
    if name == "identity_rows_cr_4":
        assert h == oh, "one vertical tap per row"


def test_edges_and_crops_cover_the_tile_walk():
    """a condition on the inputs: if a tile constant changes and one of these falls away, the inputs are what changes"""
    crops = [("crop", si.CROP_SOURCE + (c,) + si.CROP_OUT + (aa,)) for c in si.CROPS for aa in (1, 0)]
    recs = [r for _, r in walks(sorted(si.EDGES.items()) + crops)]
    luma, chroma = [r for r in recs if r["kind"] == 0], [r for r in recs if r["kind"] == 1]
    cr = {r["cr_max"] for r in recs}
    assert 4 in cr and cr & {7, 8} and cr & {15, 16} and cr & {30, 31} and 32 in cr, sorted(cr)
    assert any(r["chunks"] == 1 for r in recs) and any(r["chunks"] >= 10 for r in recs)
    assert any(r["last_rows"] == 1 for r in recs)
    assert any(r["straddle"] > 0 and r["cr_max"] <= 8 for r in recs)
    assert max(r["tx"] for r in luma) >= 2 and max(r["tx"] for r in chroma) >= 1
    assert any(r["nw"] < 128 for r in luma) and any(r["nw"] < 128 for r in chroma)
    assert any(r["nh"] < 32 for r in recs)
    assert any(r["replicated"] & 1 for r in recs) and any(r["replicated"] & 2 for r in recs)
    assert {0, 2, 14} <= {r["phase"] for r in luma} and {0, 1, 7} <= {r["phase"] for r in chroma}
    # the crops' ends: 1, 15 and 0 mod 16, and flush with the source's right and bottom edges
    ends = {(x + w) % 16 for x, _, w, _ in si.CROPS}
    assert {1, 15, 0} <= ends and any(x + w == si.CROP_SOURCE[0] and y + h == si.CROP_SOURCE[1] for x, y, w, h in si.CROPS)
    assert {x % 16 for x, _, _, _ in si.CROPS} == {0, 2, 14} and any(w == 1 for _, _, w, _ in si.CROPS) and any(w == 2 for _, _, w, _ in si.CROPS)
