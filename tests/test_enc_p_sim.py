"""The encoder's GOP pass (I + P pictures, jsmpeg_amd/csrc/enc_motion.h) without a GPU: the CPU simulator of its kernels
(sim_encode_p of tests/sim/sim_encode_pass.cpp) against the independent restatement (tests/enc_p_ref.py), and the oracle as judge of every stream:
it decodes each one to the encoder's own reconstruction, bit for bit -- the closed loop."""
import json
import os

import numpy as np
import pytest

import enc_inputs as ei
import enc_p_inputs as ep
import enc_p_ref
import enc_ref
from conftest import ROOT


@pytest.fixture(scope="module")
def cases(libs):
    return ep.p_cases(libs)


_results = {}


def sim_result(cases, name, q, gop, R):
    key = (name, q, gop, R)
    if key not in _results:
        frames, w, h = cases[name]
        _results[key] = ep.sim_encode_p(frames, w, h, gop, R, qscale=q)
    return _results[key]


def every(cases):
    for name in cases:
        for gop, R in ep.GOPS:
            yield name, gop, R


@pytest.mark.parametrize("q", ep.SCALES)
def test_simulator_equals_the_restatement(cases, q):
    for name, gop, R in every(cases):
        frames, w, h = cases[name]
        got, want = sim_result(cases, name, q, gop, R), enc_p_ref.encode(frames, w, h, gop, R, qscale=q)
        where = (name, q, gop, R)
        assert got.vectors == want.vectors, where
        assert got.stats == want.stats, where
        assert all(np.array_equal(a, b) for a, b in zip(got.recon, want.recon)), where
        assert got.ranges == want.ranges and got.streams == want.streams, where
        assert got.buf == want.buf, where


@pytest.mark.parametrize("q", ep.SCALES)
def test_the_oracle_decodes_every_stream_to_the_encoders_reconstruction(libs, cases, q):
    for name, gop, R in every(cases):
        r = sim_result(cases, name, q, gop, R)
        n = len(cases[name][0])
        es = r.stream(0)
        assert ep.picture_types(es) == ep.expected_types(n, gop), (name, q, gop, R)
        dec = ep.oracle_frames(libs, es)
        assert len(dec) == n, (name, q, gop, R)
        for k in range(n):
            assert np.array_equal(dec[k], r.recon[k]), (name, q, gop, R, k)
        # a P picture's range begins at its picture start code, an I picture's at its sequence header
        for k, (off, _) in enumerate(r.ranges):
            assert r.buf[off:off + 4] == (b"\x00\x00\x01\x00" if k % gop else b"\x00\x00\x01\xb3"), (name, k)


def test_streams_scales_and_the_end_flag(libs, cases):
    """ragged levels: streams of 3, 1 and 2 pictures, gop 2, a scale per picture -- and each stream decodes to its reconstruction"""
    frames = cases["enc_pan_176x144"][0][:6]
    streams, qs = [0, 0, 0, 1, 2, 2], [3, 9, 31, 8, 1, 5]
    for end in (True, False):
        got = ep.sim_encode_p(frames, 176, 144, 2, 7, streams=streams, qscale=qs, frame_rate_code=3, end=end, max_streams=4)
        want = enc_p_ref.encode(frames, 176, 144, 2, 7, streams=streams, qscale=qs, frame_rate_code=3, end=end)
        assert got.triple() == (want.buf, want.ranges, want.streams)
        assert got.stats == want.stats
        for s, ks in ((0, [0, 1, 2]), (1, [3]), (2, [4, 5])):
            es = got.stream(s)
            assert ep.picture_types(es) == [1, 2, 1][:len(ks)]
            dec = ep.oracle_frames(libs, es)
            assert len(dec) == len(ks) and all(np.array_equal(dec[i], got.recon[k]) for i, k in enumerate(ks))


def test_every_kind_shows_on_the_input_meant_for_it(cases):
    def total(name, q, gop, R):
        return np.sum(sim_result(cases, name, q, gop, R).stats[1:], axis=0)
    intra, coded, not_coded, skipped = total("content_176x144", 8, 3, 7)
    assert coded and not_coded
    assert total("scene_cut", 8, 3, 0)[0] and total("noise", 1, 3, 7)[0]          # intra macroblocks inside a P picture
    assert total("content_176x144", 31, 3, 0)[3] and total("flat_grey", 8, 3, 7)[3]
    r = sim_result(cases, "scene_cut", 8, 3, 0)
    kinds = [v is None for v in r.vectors[1]]
    assert any(a != b for a, b in zip(kinds, kinds[1:]))                          # intra next to non-intra: DC predictor resets


def test_a_whole_pel_pan_is_found_exactly(cases):
    r = sim_result(cases, "whole_pel_pan", 1, 3, 7)
    mbw, mbh = 4, 3
    for k in (1, 2):
        # the pan shows new content at the right and at the top: macroblocks away from those edges
        for row in range(1, mbh):
            for col in range(0, mbw - 1):
                assert r.vectors[k][row * mbw + col] == (6, -4), (k, row, col)


def test_a_half_pel_pan_takes_the_half_pel_step(cases):
    r = sim_result(cases, "half_pel_pan", 1, 3, 7)
    mbw = 4
    # picture 1 is the source interpolated at (1.5, 0.5): exactly the decoder's prediction for (3, 1) from picture 0
    for row in range(0, 2):
        for col in range(0, mbw - 1):
            assert r.vectors[1][row * mbw + col] == (3, 1), (row, col)
    assert any(v is not None and (v[0] & 1 or v[1] & 1) for v in r.vectors[2])


def test_flat_grey(cases):
    frames, w, h = cases["flat_grey"]
    for q in ep.SCALES:
        for gop, R in ep.GOPS:
            r = sim_result(cases, "flat_grey", q, gop, R)
            assert all(np.array_equal(a, b) for a, b in zip(r.recon, frames))     # lossless
            for k in range(1, 3):
                # per row the first and the last macroblock, "MC, not coded" with a zero vector; the other one is skipped
                assert r.stats[k] == (0, 0, 4, 2)
                assert r.vectors[k] == [(0, 0)] * 6
                # picture header 9 bytes; a slice: 38 bits of header, "1 001 1 1", "011 001 1 1"
                assert r.ranges[k][1] == 9 + 2 * ((38 + 6 + 8 + 7) // 8)
            assert r.buf == enc_p_ref.encode(frames, w, h, gop, R, qscale=q).buf


def test_a_skipped_run_of_46_takes_an_escape(cases):
    frames, w, h = cases["flat_wide"]
    r = sim_result(cases, "flat_wide", 8, 3, 7)
    assert r.stats[1] == (0, 0, 2, 46)
    o, b = r.ranges[1]
    # 9 bytes of picture header, 38 bits of slice header, "1 001 1 1", escape (11 bits) + increment 14 (8 bits) + "001 1 1"
    assert b == 9 + (38 + 6 + 11 + 8 + 5 + 7) // 8
    bits = "".join("{:08b}".format(v) for v in r.buf[o + 9:o + b])
    assert bits[38 + 6:38 + 6 + 19] == "00000001000" + "00000111"


def test_one_macroblock_is_first_and_last(cases):
    for q in ep.SCALES:
        r = sim_result(cases, "one_macroblock", q, 3, 7)
        assert r.stats[1][3] == 0 and sum(r.stats[1]) == 1          # identical to the picture before, and still written
        assert sum(r.stats[2]) == 1


def test_noise_clips_and_escapes(cases):
    frames, w, h = cases["noise"]
    ref = enc_p_ref.code_picture(frames[2], None, 64, 48, 1, 7, False).recon
    pic = enc_p_ref.code_picture(frames[3], ref, 64, 48, 1, 7, True)
    lv = np.abs(pic.levels[pic.kind == "C"])
    assert lv.size and lv.max() == 255                              # clipped: 8 * 65 / 1 is 260
    lv = np.abs(enc_p_ref.code_picture(frames[1], enc_p_ref.code_picture(frames[0], None, 64, 48, 1, 7, False).recon, 64, 48, 1, 7, True).levels)
    assert np.count_nonzero(lv > 40) and np.count_nonzero(lv > 127)  # both escape forms
    # (5, 15) makes pictures 0 .. 3 one GOP: the clipped picture is predicted there, and equals the restatement and the oracle above
    assert sim_result(cases, "noise", 1, 5, 15).stats[3][1] > 0


def test_a_last_macroblock_inside_one_byte_gets_stuffing(libs, cases):
    """the reference ends a slice when the next whole bytes are a start code: a last macroblock of 6 bits that begins inside a
    byte would never be read.  Some slice of the inputs must have met the case (the restatement decides it on its own)"""
    frames, w, h = cases["content_177x145"]
    r = sim_result(cases, "content_177x145", 31, 3, 0)
    want = enc_p_ref.encode(frames, w, h, 3, 0, qscale=31)
    assert sum(want.stuffed) > 0 and r.buf == want.buf
    # where: the stuffing code and the 6 bits of "1 001 1 1" are the last 17 bits of a slice that was stuffed
    k = next(i for i, n in enumerate(want.stuffed) if n)
    o, b = r.ranges[k]
    pic = r.buf[o:o + b]
    ends = [i for i in range(len(pic) - 3) if pic[i:i + 3] == b"\x00\x00\x01"][2:] + [len(pic)]      # behind every slice of the P picture
    tails = ["".join("{:08b}".format(v) for v in pic[e - 4:e]).rstrip("0") for e in ends]
    assert sum(t.endswith("00000001111" + "100111") for t in tails) == want.stuffed[k]


@pytest.mark.parametrize("q", ep.SCALES)
def test_gop_1_is_the_intra_encoder(cases, q):
    for name in ("content_177x145", "one_macroblock", "noise"):
        frames, w, h = cases[name]
        assert ep.sim_encode_p(frames, w, h, 1, 9, qscale=q).triple() == ei.sim_encode(frames, w, h, qscale=q), name


def test_a_gop_makes_the_stream_smaller(cases):
    still = [ep.pan_frames(176, 144, 1, (0, 0))[0]] * 13
    for frames in (cases["enc_pan_176x144"][0], still):
        for q in ep.SCALES:
            assert len(ep.sim_encode_p(frames, 176, 144, 12, 7, qscale=q).buf) < len(ei.sim_encode(frames, 176, 144, qscale=q)[0]), q


def test_quality_holds_the_recorded_gap(libs):
    """luma PSNR of gop 12, R 7 against the intra encoder at the same scale (the yardstick), held to the recorded gap plus a
    tenth of it; and, per case, PSNR does not fall from the first P picture of the GOP to the last by more than the recorded
    figure of that case (the loop is closed: a steady loss is a bug; the run is deterministic, so no slack)"""
    import importlib.util
    spec = importlib.util.spec_from_file_location("enc_p_quality", os.path.join(ROOT, "tools", "enc_p_quality.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    with open(os.path.join(ROOT, "profiles", "enc_p_bounds.json")) as f:
        recorded = json.load(f)
    fresh = tool.measure(libs)
    for q in (str(v) for v in tool.SCALES):
        a, b = fresh[q], recorded["scales"][q]
        print(q, a, b)
        assert a["gap_db"] <= b["gap_db"] + abs(b["gap_db"]) / 10.0, q
        assert sorted(a["gop_fall_db"]) == sorted(b["gop_fall_db"]) == recorded["inputs"]
        for case, fall in a["gop_fall_db"].items():
            assert fall <= b["gop_fall_db"][case], (q, case)


# ---------------------------------------------------------------------------------------------------- every search range

RANGE_SCALES = (1, 8)


@pytest.fixture(scope="module")
def ranged(libs, cases):
    return ep.range_cases(libs, cases)


_ranged = {}


def range_results(ranged, name, q, R):
    """(simulator, restatement) of a range case at gop 4, computed once"""
    key = (name, q, R)
    if key not in _ranged:
        frames, w, h = ranged[name]
        _ranged[key] = (ep.sim_encode_p(frames, w, h, 4, R, qscale=q), enc_p_ref.encode(frames, w, h, 4, R, qscale=q))
    return _ranged[key]


@pytest.mark.parametrize("R", ep.RADII)
def test_every_search_range(libs, ranged, R):
    """each radius has its own number of items, its own group alignment and staged rows in the search: simulator == restatement,
    the oracle decodes the stream to the encoder's reconstruction, and every P picture's header carries the f_code of the range"""
    for q in RANGE_SCALES:
        for name, (frames, w, h) in ranged.items():
            got, want = range_results(ranged, name, q, R)
            where = (name, q, R)
            assert got.vectors == want.vectors, where
            assert got.stats == want.stats, where
            assert all(np.array_equal(a, b) for a, b in zip(got.recon, want.recon)), where
            assert got.ranges == want.ranges and got.streams == want.streams, where
            assert got.buf == want.buf, where
            es, n = got.stream(0), len(frames)
            assert ep.picture_types(es) == ep.expected_types(n, 4), where
            dec = ep.oracle_frames(libs, es)
            assert len(dec) == n, where
            for k in range(n):
                assert np.array_equal(dec[k], got.recon[k]), (where, k)
                if k % 4:
                    assert ep.p_header(got.buf, got.ranges[k][0]) == (k % 4, 2, 0, 1 if R <= 7 else 2), (where, k)


def test_the_range_cases_reach_the_edge_of_every_range_and_the_wrap(ranged):
    """coverage, from the restatement's vectors: at every R > 0 some vector component is 2 R + 1 half-pels and some is
    -(2 R + 1) -- the outermost full-pel candidate and the half-pel step beyond it, on both sides of the staged window --
    and the differential against the predictor leaves [-16 f, 16 f - 1] (jm_encp_wrap) at a range with f_code 1 and at one with 2"""
    wrapped = set()
    for R in ep.RADII[1:]:
        seen = set()
        for q in RANGE_SCALES:
            for name, (frames, w, h) in ranged.items():
                want = range_results(ranged, name, q, R)[1]
                seen |= {c for pic in want.vectors for v in pic if v is not None for c in v}
                if ep.wrapped_differentials(want.vectors, (w + 15) // 16, 16 if R <= 7 else 32):
                    wrapped.add(R)
        assert 2 * R + 1 in seen and -(2 * R + 1) in seen, R
    assert any(R <= 7 for R in wrapped) and any(R >= 8 for R in wrapped), wrapped


@pytest.mark.parametrize("R", (0, 7))
def test_the_intra_decision_at_equality(ranged, R):
    """activity + 512 < SAD: 639 < 639 and 640 < 640 are predicted (the second is the equality), 639 < 641 and 638 < 642 intra"""
    frames, w, h = ranged["intra_threshold"]
    for q in RANGE_SCALES:
        for r in range_results(ranged, "intra_threshold", q, R):
            assert np.array_equal(r.recon[0], frames[0]), (q, R)                    # the flat picture is the reference as it was
            assert r.vectors[1] == [(0, 0), (0, 0), None, None], (q, R)
            assert r.stats[1][0] == 2, (q, R)


def brute_force_vector(cur, ref, cw, ch, col, row, R):
    """enc_motion.h's rule 1 by brute force for one macroblock: the full-pel candidates a decoder can read (the test encoder's
    mv_ok) ordered by (SAD, dx^2 + dy^2, dy, dx), then a half-pel neighbour only with a strictly smaller SAD, ordered by
    (SAD, vertical step, horizontal step).  Returns the vector in half-pels and how many full-pel candidates share the least SAD"""
    from mpeg1_enc import mv_ok
    blk = cur[row * 16:row * 16 + 16, col * 16:col * 16 + 16].astype(np.int64)
    p = np.zeros((ch + 1, cw + 1), dtype=np.int64)
    p[:ch, :cw] = ref

    def sad(mh, mv):
        x, y, oh, ov = col * 16 + (mh >> 1), row * 16 + (mv >> 1), mh & 1, mv & 1
        a, b, c, d = (p[y + j:y + j + 16, x + i:x + i + 16] for j in (0, 1) for i in (0, 1))
        pred = (a + b + c + d + 2) >> 2 if oh and ov else (a + b + 1) >> 1 if oh else (a + c + 1) >> 1 if ov else a
        return int(np.abs(blk - pred).sum())

    full = [(sad(2 * dx, 2 * dy), dx * dx + dy * dy, dy, dx) for dy in range(-R, R + 1) for dx in range(-R, R + 1)
            if mv_ok(cw, ch, col, row, 2 * dx, 2 * dy)]
    best = min(full)
    ties = sum(1 for c in full if c[0] == best[0])
    mh, mv = 2 * best[3], 2 * best[2]
    rng = 16 if R <= 7 else 32
    half = [(sad(mh + hh, mv + hv), hv, hh) for hv in (-1, 0, 1) for hh in (-1, 0, 1)
            if (hh or hv) and -rng <= mh + hh < rng and -rng <= mv + hv < rng and mv_ok(cw, ch, col, row, mh + hh, mv + hv)]
    if R and half and min(half)[0] < best[0]:
        return (mh + min(half)[2], mv + min(half)[1]), ties
    return (mh, mv), ties


@pytest.mark.parametrize("R", (3, 7, 12))
def test_ties_go_by_the_stated_order(ranged, R):
    """the checkerboard, its shift by 2 pels, the checkerboard: picture 0 reconstructs with a period of 8 (every block alike) and
    picture 1 has a period of 4, so a candidate's SAD over 16 columns is that of the candidate 4 pels further -- (-2, 0) and
    (2, 0) tie exactly, whatever the quantiser did.  The simulator's vectors are the restatement's, and the brute-force minimum
    where no candidate leaves the picture"""
    frames, w, h = ranged["checker_ties"]
    for q in RANGE_SCALES:
        got, want = range_results(ranged, "checker_ties", q, R)
        assert got.vectors == want.vectors, (q, R)
        for k in (1, 2):
            cur, ref = enc_ref.planes(frames[k], w, h)[0], enc_ref.planes(got.recon[k - 1], w, h)[0]
            for col in (1, 2):                                                       # 4 x 3 macroblocks: row 1, columns 1 and 2
                vector, ties = brute_force_vector(cur, ref, w, h, col, 1, R)
                assert got.vectors[k][4 + col] == vector, (q, R, k, col)
                assert k != 1 or ties >= 2, (q, R, col)


# ---------------------------------------------------------------------------------------------------- a call past 256 pictures

@pytest.fixture(scope="module")
def long_call():
    return ep.long_call()


_long = {}


def long_result(long_call, gop, R, end):
    key = (gop, R, end)
    if key not in _long:
        frames, w, h, streams, qs = long_call
        _long[key] = ep.sim_encode_p(frames, w, h, gop, R, streams=streams, qscale=qs, end=end, max_streams=ep.LONG_MAX_STREAMS)
    return _long[key]


@pytest.mark.parametrize("end", (True, False))
@pytest.mark.parametrize("gop,R", ep.LONG_GOPS)
def test_a_call_of_1100_pictures(libs, long_call, gop, R, end):
    """five streams with gaps in their numbers, boundaries on both sides of pictures 256 and 512, levels up to 1023: every
    stream decodes to its reconstructions, and the buffer is what jsmpeg_hip_batch_attach_device asks for"""
    frames, w, h, streams, qs = long_call
    r = long_result(long_call, gop, R, end)                 # (sim_encode_p has looked at the 256 bytes behind the total)
    ordinal = ep.ordinals(streams)
    present = sorted(set(streams))
    assert sorted(r.streams) == present
    for s in present:
        ks = [k for k in range(len(streams)) if streams[k] == s]
        es = r.stream(s)
        assert ep.picture_types(es) == ep.expected_types(len(ks), gop), s
        dec = ep.oracle_frames(libs, es)
        assert len(dec) == len(ks), s
        for i, k in enumerate(ks):
            assert np.array_equal(dec[i], r.recon[k]), (s, i)
        assert r.streams[s] == (r.ranges[ks[0]][0], sum(r.ranges[ks[-1]]) + (4 if end else 0)), s
    for k, (off, _) in enumerate(r.ranges):
        if ordinal[k] % gop:
            assert ep.p_header(r.buf, off) == (ordinal[k] % gop, 2, 0, 1 if R <= 7 else 2), k
        else:
            assert r.buf[off:off + 4] == b"\x00\x00\x01\xb3", k
    assert sum(1 for k, s in enumerate(r.stats) if ordinal[k] % gop and 0 < s[0] < 6) > 0       # intra macroblocks inside P pictures
    assert sum(s[3] for s in r.stats) > 0                                                     # and skipped ones
    spans = [r.streams[s] for s in present]
    assert spans[0][0] >= 16 and all(b % 16 == 0 for b, _ in spans)
    assert all(b2 - e1 >= 8 for (_, e1), (b2, _) in zip(spans, spans[1:])), spans
    outside = np.ones(len(r.buf), dtype=bool)
    for b, e in spans:
        outside[b:e] = False
    assert np.all(np.frombuffer(r.buf, dtype=np.uint8)[outside] == 0xff)
    assert [r.table[s] for s in range(ep.LONG_MAX_STREAMS) if s not in present] == [(0, 0)] * (ep.LONG_MAX_STREAMS - len(present))


@pytest.mark.parametrize("gop,R", ep.LONG_GOPS)
def test_a_call_past_256_pictures_equals_the_restatement(long_call, gop, R):
    """the restatement is too slow for 1100 pictures: the call's first 263, which cross picture 256 and the stream boundaries
    at 255, 257 and 258 (the sequence end code off as well where the restatement takes a second, not ten)"""
    frames, w, h, streams, qs = long_call
    n = 263
    for end in (True, False) if R < 15 else (True,):
        got = ep.sim_encode_p(frames[:n], w, h, gop, R, streams=streams[:n], qscale=qs[:n], end=end, max_streams=ep.LONG_MAX_STREAMS)
        want = enc_p_ref.encode(frames[:n], w, h, gop, R, streams=streams[:n], qscale=qs[:n], end=end)
        assert got.vectors == want.vectors and got.stats == want.stats, end
        assert all(np.array_equal(a, b) for a, b in zip(got.recon, want.recon)), end
        assert got.triple() == (want.buf, want.ranges, want.streams), end
        # placement has no memory of the pictures behind: the sub-call's pictures lie where the whole call's do
        assert got.ranges == long_result(long_call, gop, R, end).ranges[:n]


# ---------------------------------------------------------------------------------------------------- the quantiser's division

def test_the_reciprocal_is_the_integer_division():
    """jm_encp_quant_inter divides by q as mulhi(2 n, floor(2^31 / q) + 1): exhaustively for n < 2^16 (the encoder's n, |c8| >> 4,
    stays below 2^11) and every quantiser scale"""
    n = np.arange(1 << 16, dtype=np.uint32)
    for q in range(1, 32):
        assert np.array_equal(ep.sim_recip_div(n, q), n // q), q
