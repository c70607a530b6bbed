"""The slice parse at its edges, on the CPU: that the crafted streams of tests/parse_inputs.py hold what they claim (counted
again here over the descriptions, by a walk that restates the slice layer's syntax and the decoder's predictor rules, and a
second time over the macroblock records the simulator wrote), what they REACH in the walk of jsmpeg_amd/csrc/slice_parse.h
(the simulator's reach counters, tests/sim/sim_decode.cpp: bits per turn, head-room in the compressed-data ring, occupancy of
the token ring, bit phases and ring positions of the looks, refills held back, finish tails), and that oracle, simulator (both
forms of the ring service) and -- where it is present -- the reference's own C agree on every stream.  The GPU side is
tests/test_gpu_parse_edges.py.

What the figures say (profiles/parse_edges_notes.md has the tables):
  * The most bits a lane consumes in one turn is 102, not JM_STEP_BITS = 136: a turn is service, COLD, DC, COEF, SLOW, COEF, and
    a lane runs SLOW in the turn of its header only if the COEF step in front of it consumed nothing (it hands an escape on
    without taking a bit), so COLD 64 (increment 11, type 5, quantiser 5, two vectors of 11 + 6, pattern 9: an intra header
    has neither vector nor pattern) + SLOW 28 + COEF 10.  The header's sum adds a DC to a header with vectors and counts both
    COEF steps beside the SLOW step.  136 is a safe bound, 34 bits wider than needed.
  * jm_lane_finish never sees an odd tail on a valid stream: every block ends on an even slot (the alignment slot of an odd
    run), slices begin on multiples of 16 slots.  Tails 0, 2 .. 14 are met; 1, 3 .. 15 are asserted to be zero.

Writing all 24 streams takes under a second, the decodes a few seconds."""
import ctypes
import hashlib

import numpy as np
import pytest

import craft_es as C
import parse_inputs as P
from conftest import have_reference
from craft_es import E
from jsmpeg_amd import cabi
from test_sim_device_functions import sim  # noqa: F401  (the simulator library, a fixture)

KINDS = ("COLD", "DC", "COEF", "SLOW", "slice header")
MB_INTRA, MB_PRED = 0x20, 0x40


# ----------------------------------------------------------------------------------------------------------------
# the independent count: a walk over a description

def census(desc):
    """what a description holds, symbol by symbol -> dict of sets and counts, `slices` (per slice: picture, start, bits, tokens,
    slots) and `records` (per picture, per macroblock: (flag, quantiser, mvh, mvv, six token counts) as the parse must record it)"""
    mbw, mbh = (desc["width"] + 15) >> 4, (desc["height"] + 15) >> 4
    F = dict(vlc=set(), first=set(), esc=set(), eob_after=set(), last63=0, incs=set(), first_incs=set(), stuffing=0, esc_in_a_row=set(),
             types={"I": set(), "P": set()}, cbp=set(), motion={}, wraps={}, dc={True: set(), False: set()}, dc_after={}, q_to=set(),
             slices=[], records=[], block_counts=set(), user_data=[], extra=set())
    for t, pic in enumerate(desc["pictures"]):
        is_p = pic["type"] == "P"
        f_code, full_pel = pic.get("f_code", 1), pic.get("full_pel", 0)
        r_size = f_code - 1
        span = 16 << r_size
        mbs = pic["mbs"]
        F["user_data"].append(pic.get("user_data"))
        recs = [None] * (mbw * mbh)
        slices = [s if isinstance(s, dict) else dict(start=s) for s in pic.get("slices", range(0, mbw * mbh, mbw))]
        for si, sl in enumerate(slices):
            start = sl["start"]
            stop = slices[si + 1]["start"] if si + 1 < len(slices) else mbw * mbh
            q = mbs[start][0]
            F["extra"].add(sl.get("extra", 0))
            bits = 5 + 9 * sl.get("extra", 0) + 1
            tokens = slots = 0
            pmh = pmv = 0
            first = True
            inc = start - sl.get("row", start // mbw) * mbw + 1
            before = "slice start"
            last_bits = 0
            for addr in range(start, stop):
                entry = mbs[addr]
                new_q, kind, mv, blocks = entry[:4]
                opts = entry[4] if len(entry) > 4 else {}
                if kind == "skip":
                    inc += 1
                    pmh = pmv = 0
                    before = "skipped"
                    recs[addr] = (MB_PRED, q, 0, 0, (0,) * 6)
                    continue
                mb_bits = 11 * opts.get("stuffing", 0) + 11 * ((inc - 1) // 33) + len(E.INV["MBA"][(inc - 1) % 33 + 1])
                F["stuffing"] += opts.get("stuffing", 0)
                (F["first_incs"] if first else F["incs"]).add(inc)
                F["esc_in_a_row"].add((inc - 1) // 33)
                first, inc = False, 1
                use_q = new_q != q
                if use_q:
                    F["q_to"].add(new_q)
                q = new_q
                esc = opts.get("esc", {})
                counts = [0] * 6
                if kind == "intra":
                    ty = 0x11 if use_q else 0x01
                    mb_bits += len(E.INV["MBTYPE_P" if is_p else "MBTYPE_I"][ty]) + 5 * use_q
                    pmh = pmv = 0
                    F["dc_after"].setdefault(before, set()).update(b for b in range(6) if blocks[b][0] != 0)
                    for b, (diff, levels) in enumerate(blocks):
                        F["dc"][b < 4].add(diff)
                        size = abs(diff).bit_length()
                        mb_bits += len(E.INV["DCSIZE_LUMA" if b < 4 else "DCSIZE_CHROMA"][size]) + size
                        syms = C.coef_symbols(levels, False, esc.get(b, ()))
                        _count_block(F, syms, 1)
                        counts[b] = 1 + len(syms)
                        mb_bits += sum(len(s[3]) for s in syms) + 2
                    recs[addr] = (MB_INTRA, q, 0, 0, tuple(counts))
                    before = "intra"
                else:
                    ty = {"coded": 0x02, "coded_mv": 0x0A, "mv": 0x08}[kind] | (0x10 if use_q else 0)
                    mb_bits += len(E.INV["MBTYPE_P"][ty]) + 5 * use_q
                    if kind == "coded":
                        pmh = pmv = 0
                    else:
                        given = opts.get("mv_d", (None, None))
                        for cur, prev, g in ((mv[0], pmh, given[0]), (mv[1], pmv, given[1])):
                            d = cur - prev
                            d = d + 2 * span if d < -span else (d - 2 * span if d >= span else d)
                            if g is not None:
                                d = g
                            F["motion"].setdefault((f_code, full_pel), set()).add(d)
                            if prev + d >= span:
                                F["wraps"].setdefault((f_code, full_pel), set()).add("top")
                            if prev + d < -span:
                                F["wraps"].setdefault((f_code, full_pel), set()).add("bottom")
                            ad = abs(d) - 1
                            code = 0 if d == 0 else ((ad >> r_size) + 1) * (1 if d > 0 else -1)
                            mb_bits += len(E.INV["MOTION"][code]) + (r_size if d else 0)
                        pmh, pmv = mv
                    cbp = sum(0x20 >> b for b in range(6) if blocks[b] is not None)
                    if cbp:
                        F["cbp"].add(cbp)
                        mb_bits += len(E.INV["CBP"][cbp])
                        for b in range(6):
                            if blocks[b] is not None:
                                syms = C.coef_symbols(blocks[b], True, esc.get(b, ()))
                                _count_block(F, syms, 0)
                                counts[b] = len(syms)
                                mb_bits += sum(len(s[3]) for s in syms) + 2
                    recs[addr] = (MB_PRED, q, pmh << full_pel, pmv << full_pel, tuple(counts))
                    before = "non-intra"
                F["types"][pic["type"]].add(ty)
                tokens += sum(counts)
                slots += sum((c + 1) & ~1 for c in counts)
                bits += mb_bits
                last_bits = mb_bits
            F["slices"].append(dict(picture=t, start=start, row=sl.get("row", start // mbw), bits=bits, tokens=tokens, slots=slots,
                                    mbs=stop - start, last_bits=last_bits))
        F["records"].append(recs)
    return F


def _count_block(F, syms, base):
    pos = base - 1
    for run, lv, form, _ in syms:
        pos += run + 1
        if form == "vlc":
            F["vlc"].add((run, lv))
        elif form == "first":
            F["first"].add(lv)
        else:
            F["esc"].add((run, lv, form))
    assert pos <= 63
    F["last63"] += pos == 63
    F["eob_after"].add((base, base + len(syms)))       # (intra?, tokens in front of the end_of_block)
    F["block_counts"].add(base + len(syms))


_census = {}


def census_of(w):
    if w["name"] not in _census:
        _census[w["name"]] = census(w["desc"])
    return _census[w["name"]]


def merged(cs, key):
    out = set()
    for c in cs:
        out |= c[key]
    return out


def slice_payloads(es):
    """[(position of the start code, payload bytes)] of every slice of a written stream"""
    es = np.asarray(es)
    pos = np.flatnonzero((es[:-3] == 0) & (es[1:-2] == 0) & (es[2:-1] == 1))
    out = []
    for i, p in enumerate(pos):
        if 1 <= es[p + 3] <= 0xAF:
            out.append((int(p), int(pos[i + 1]) - int(p) - 4))
    return out


# ----------------------------------------------------------------------------------------------------------------
# the claims

def test_symbols_holds_every_symbol():
    S = P.symbols()
    cl = S["claims"]
    cs = [census_of(P.written(s)) for s in S["streams"]]
    vlc, first, esc = merged(cs, "vlc"), merged(cs, "first"), merged(cs, "esc")
    # every DCT run/level code in both signs (the table's 110 and "11s"), and the first-coefficient form
    want = {(r, s * m) for (r, m) in E.COEFF for s in (1, -1)} | {(0, 1), (0, -1)}
    assert vlc == want and len(want) == cl["dct_codes"] == 222
    assert first == {1, -1}
    # end_of_block after 1 .. 64 tokens, in intra blocks (the DC is the first) and in non-intra ones
    eob = merged(cs, "eob_after")
    assert {n for base, n in eob if base == 1} == set(cl["eob_after"]) == {n for base, n in eob if base == 0} == set(range(1, 65))
    # escapes: the named runs x the named levels, each in the form its level calls for
    for run in cl["esc_runs"]:
        for lv in cl["esc_levels"]:
            assert (run, lv, "esc20" if abs(lv) <= 127 else "esc28") in esc, (run, lv)
    assert set(cl["esc_runs"]) == {0, 1, 31, 32, 62, 63} and set(cl["esc_levels"]) == {s * m for m in (1, 127, 128, 129, 255) for s in (1, -1)}
    assert sum(c["last63"] for c in cs) >= 3
    # increments: every code behind skipped macroblocks, one and two escapes in a row, stuffing; large FIRST increments too
    incs = merged(cs, "incs")
    assert set(range(1, 34)) <= incs and incs >= set(cl["increments"]) and {0, 1, 2} <= merged(cs, "esc_in_a_row")
    assert any(33 < i <= 66 for i in incs) and any(66 < i <= 99 for i in incs)
    assert merged(cs, "first_incs") >= set(cl["first_increments"]) and sum(c["stuffing"] for c in cs) >= 5
    types_i, types_p = set(), set()
    for c in cs:
        types_i |= c["types"]["I"]
        types_p |= c["types"]["P"]
    assert types_i == set(cl["types_i"]) == {0x01, 0x11} and types_p == set(cl["types_p"]) == {0x01, 0x02, 0x08, 0x0A, 0x11, 0x12, 0x1A}
    assert merged(cs, "cbp") == set(range(1, 64)) == set(cl["patterns"])
    # motion: per f_code and vector unit every code with residual bits all zero and all one, and a wrap at each end
    motion, wraps = {}, {}
    for c in cs:
        for k, v in c["motion"].items():
            motion.setdefault(k, set()).update(v)
        for k, v in c["wraps"].items():
            wraps.setdefault(k, set()).update(v)
    for f_code in range(1, 8):
        f = 1 << (f_code - 1)
        need = {0} | {s * (((code - 1) << (f_code - 1)) + r + 1) for code in range(1, 17) for r in (0, f - 1) for s in (1, -1)}
        for full_pel in (0, 1):
            assert need <= motion[(f_code, full_pel)], (f_code, full_pel, sorted(need - motion[(f_code, full_pel)]))
            assert set(cl["motion"][(f_code, full_pel)]) <= motion[(f_code, full_pel)]
            assert wraps[(f_code, full_pel)] == {"top", "bottom"}, (f_code, full_pel)
    # dct_dc_size 0 .. 8 in both tables with each size's extreme differentials
    for luma in (True, False):
        dc = set()
        for c in cs:
            dc |= c["dc"][luma]
        assert {0} | {s * m for k in range(1, 9) for m in ((1 << k) - 1, 1 << (k - 1)) for s in (1, -1)} <= dc
        assert {abs(d).bit_length() for d in dc} == set(cl["dc_sizes"]) == set(range(9))
    # the DC predictor of every block after an intra, a non-intra and a skipped neighbour (non-zero differentials show it)
    after = {}
    for c in cs:
        for k, v in c["dc_after"].items():
            after.setdefault(k, set()).update(v)
    for k in ("intra", "non-intra", "skipped"):
        assert after[k] == set(range(6)), k
    assert {1, 31} <= merged(cs, "q_to")


def test_phases_is_one_sequence_at_every_start_phase():
    S = P.phases()
    ws = [P.written(s) for s in S["streams"]]
    assert len(ws) == 16
    base = ws[0]["es"].tobytes()
    k = base.find(b"\x00\x00\x01\xb2") + 4
    starts = set()
    for n, w in enumerate(ws):
        assert census_of(w)["user_data"][0] == n
        es = w["es"].tobytes()
        assert es == base[:k] + bytes([C.USER_DATA_BYTE]) * n + base[k:]                 # nothing but the shift
        sl = slice_payloads(w["es"])
        assert len(sl) == 18
        starts.add(tuple((p + 4) & 15 for p, _ in sl))
    per_slice = list(zip(*starts))
    assert all(set(col) == set(range(16)) for col in per_slice)                          # every slice at every payload_off & 15
    c = census_of(ws[0])
    assert c["extra"] == set(range(8)) and c["types"]["P"] == {0x01, 0x02, 0x08, 0x0A, 0x11, 0x12, 0x1A} and c["types"]["I"] == {0x01, 0x11}
    assert {f for _, _, f in c["esc"]} == {"esc20", "esc28"} and c["stuffing"] > 0 and max(c["incs"]) > 2


def test_worst_turns_holds_the_longest_codes():
    S = P.worst_turns()
    cl = S["claims"]
    tall, dense = [P.written(s) for s in S["streams"]]
    pic = tall["desc"]["pictures"][1]
    assert pic["f_code"] == 7 and pic["slices"] == [0]
    n_p = n_i = 0
    prev_q = pic["mbs"][0][0]
    run = 0
    for addr, mb in enumerate(pic["mbs"]):
        if mb[1] == "skip":
            run += 1
            continue
        if addr and run >= 21:
            inc = run + 1
            assert len(E.INV["MBA"][inc]) == 11 and mb[0] != prev_q                      # the longest increment, a type with quantiser
            if mb[1] == "intra":
                assert len(E.INV["MBTYPE_P"][0x11]) == 6 and all(abs(d) == 255 for d, _ in mb[3])
                n_i += 1
            else:
                assert mb[1] == "coded_mv" and len(E.INV["MBTYPE_P"][0x1A]) == 5
                for d in mb[2]:                                                          # skipped macroblocks in front: the predictor is 0
                    code = ((abs(d) - 1) >> 6) + 1
                    assert len(E.INV["MOTION"][code]) == 11 and code >= 11
                cbp = sum(0x20 >> b for b in range(6) if mb[3][b] is not None)
                assert cbp == cl["cbp"] and len(E.INV["CBP"][cbp]) == 9 == max(len(v) for v in E.INV["CBP"].values())
                n_p += 1
            for blk in mb[3]:
                levels = blk[1] if mb[1] == "intra" else blk
                if levels is not None:
                    syms = C.coef_symbols(levels, mb[1] != "intra")
                    assert syms[0][2] == "esc28" and sum(len(s[3]) for s in syms[1:]) + 2 == 10   # a 28-bit escape, then a full pair look
        prev_q = mb[0]
        run = 0
    assert n_p >= 100 and n_i >= 30 and n_p + n_i == 141
    assert max(len(v) for v in E.INV["MBA"].values()) == 11 and max(len(v) for v in E.INV["MOTION"].values()) == 11
    assert cl["turn_bits_p"] == 102 and cl["turn_bits_i"] == 75
    c = census_of(dense)
    assert c["block_counts"] == {64} and len(c["slices"]) == 18 and all(s["tokens"] == 11 * 6 * 64 for s in c["slices"])
    # 64 tokens in 2 + 63 * 3 + 2 bits: no block of 64 tokens is shorter
    assert min(s["bits"] for s in c["slices"] if s["picture"] == 1) == 6 + 11 * (1 + len(E.INV["MBTYPE_P"][0x02]) + len(E.INV["CBP"][63]) + 6 * 193)


def test_tails_holds_every_end():
    S = P.tails()
    cl = S["claims"]
    w = P.written(S["streams"][0])
    c = census_of(w)
    tok = [s["tokens"] for s in c["slices"]]
    assert set(cl["slice_tokens"]) <= set(tok) and {0, 16, 32} <= set(tok)
    assert {t % 16 for t in tok} == set(range(16)) == set(cl["token_residues"])
    assert {s["slots"] % 16 for s in c["slices"]} == set(range(0, 16, 2)) == set(cl["slot_residues"])        # slots are even: see the module's text
    zero = [s for s in c["slices"] if s["tokens"] == 0]
    assert any(s["mbs"] == 11 for s in zero) and any(s["mbs"] == 1 and s["bits"] == 15 for s in zero)      # vector-only + skipped; the shortest
    assert c["block_counts"] >= set(range(1, 65)) == set(cl["block_counts"])
    # the written stream, measured: the census' bit count is the payload's, so the slack is what it says
    pay = slice_payloads(w["es"])
    assert len(pay) == len(c["slices"])
    for (p, n), s in zip(pay, c["slices"]):
        assert n == (s["bits"] + 7) // 8 and s["last_bits"] > 8, (p, n, s)
    assert {n % 16 for _, n in pay} == set(range(16)) == set(cl["payload_residues"])
    assert {-s["bits"] % 8 for s in c["slices"]} == set(range(8)) == set(cl["slack_bits"])
    assert any((p + 4 + n) % 16 == 0 for p, n in pay) and cl["ends_on_chunk"]                               # (streams lie at 16-byte aligned places)
    assert min(n for _, n in pay) == cl["shortest_bytes"] == 2 and max(n for _, n in pay) >= 3 * cl["longest_bytes_at_least"]


def test_company_is_two_kinds_of_slices():
    S = P.company()
    a, b = [P.written(s) for s in S["streams"]]
    assert (a["desc"]["width"], a["desc"]["height"]) == (b["desc"]["width"], b["desc"]["height"]) == S["claims"]["size"]
    assert [len(a["desc"]["pictures"]), len(b["desc"]["pictures"])] == S["claims"]["pictures"]
    pa, pb = [n for _, n in slice_payloads(a["es"])][9:], [n for _, n in slice_payloads(b["es"])]
    ca, cb = census_of(a), census_of(b)
    assert len(pa) > 120 and max(pa) < 40 and min(pb) > 1000 and len(pb) == 36
    assert sum(s["tokens"] for s in ca["slices"][9:]) < 2 * len(pa) and min(s["tokens"] for s in cb["slices"]) > 1000


# ----------------------------------------------------------------------------------------------------------------
# the simulator: records, reach, pictures

def bind(sim):  # noqa: F811
    sim.sim_reach.restype = ctypes.POINTER(ctypes.c_uint64)
    sim.sim_reach_layout.restype = ctypes.c_char_p
    sim.sim_parse_constants.restype = ctypes.POINTER(ctypes.c_int)
    sim.sim_dump_counts.restype = ctypes.POINTER(ctypes.c_uint32)
    sim.sim_set_dumps.argtypes = [ctypes.c_void_p] * 5
    return sim


def constants(sim):  # noqa: F811
    c = bind(sim).sim_parse_constants()
    return dict(zip(("STEP_BITS", "TK_RING", "COEF_SLOTS", "COEF_REPEAT", "REFILL_MIN", "ES_RING_DW", "TK_GROUP", "R_COUNT"), [c[i] for i in range(8)]))


def read_reach(sim):  # noqa: F811
    r = bind(sim).sim_reach()
    out, i = {}, 0
    for field in sim.sim_reach_layout().decode().split(","):
        name, n = field.split(":")
        out[name] = [int(r[i + j]) for j in range(int(n))]
        i += int(n)
    assert i == constants(sim)["R_COUNT"]
    for k in ("max_turn_bits", "min_room", "min_room_turn", "max_occ_turn", "max_occ_step", "max_occ_after", "held_back", "landed_later"):
        out[k] = out[k][0]
    out["min_margin"] = out["min_margin"][0] - (1 << 32)
    out["phase"] = [out["phase"][32 * k:32 * k + 32] for k in range(5)]
    return out


def sim_decode(sim, w, split, records=False):  # noqa: F811
    """-> (md5 per picture, stale windows[, records per picture: uint32[mbs][4]])"""
    d, es = w["desc"], w["es"]
    n = len(d["pictures"])
    mbs = ((d["width"] + 15) >> 4) * ((d["height"] + 15) >> 4)
    fb = mbs * 384
    out = np.zeros(n * fb, dtype=np.uint8)
    bind(sim).sim_split_service(split)
    rec = np.zeros((n + 1) * mbs * 4, dtype=np.uint32)
    sim.sim_set_dumps(None, None, None, rec.ctypes.data if records else None, None)
    try:
        got = sim.sim_decode_stream(es.ctypes.data, len(es), d["width"], d["height"], out.ctypes.data, n)
    finally:
        sim.sim_set_dumps(None, None, None, None, None)
    assert got == n, (w["name"], got)
    md5 = [hashlib.md5(out[i * fb:(i + 1) * fb].tobytes()).hexdigest() for i in range(n)]
    return (md5, rec[:n * mbs * 4].reshape(n, mbs, 4)) if records else md5


_reach = {}


def reach_of(sim, fn, split):  # noqa: F811
    """the reach figures over one whole input set with one form of the service (and its stale windows, pictures and records)"""
    key = (fn.__name__, split)
    if key not in _reach:
        bind(sim).sim_reach_reset_all()
        pics = {}
        for s in fn()["streams"]:
            w = P.written(s)
            pics[w["name"]] = sim_decode(sim, w, split, records=True)
        r = read_reach(sim)
        r["stale"] = int(sim.sim_stale_windows())
        r["pictures"] = pics
        _reach[key] = r
    return _reach[key]


SETS = [fn.__name__ for fn in P.SETS]
BY_NAME = {fn.__name__: fn for fn in P.SETS}
SPLITS = pytest.mark.parametrize("split", [1, 0], ids=["service_in_two_halves", "service_in_one_piece"])

_oracle = {}


def oracle_md5(libs, w):
    if w["name"] not in _oracle:
        _oracle[w["name"]] = cabi.decode_stream(libs["oracle"], w["es"])[0]
    return _oracle[w["name"]]


@SPLITS
@pytest.mark.parametrize("name", SETS)
def test_simulator_equals_oracle_and_no_window_is_stale(name, split, sim, libs):  # noqa: F811
    r = reach_of(sim, BY_NAME[name], split)
    for s in BY_NAME[name]()["streams"]:
        w = P.written(s)
        want = oracle_md5(libs, w)
        assert len(want) == len(w["desc"]["pictures"])
        got = r["pictures"][w["name"]][0]
        bad = [i for i in range(len(want)) if got[i] != want[i]]
        assert not bad, (w["name"], bad[:8])
    assert r["stale"] == 0


@pytest.mark.parametrize("name", SETS)
def test_the_simulators_records_are_the_descriptions(name, sim):  # noqa: F811
    """the second count: every macroblock record the parse wrote -- kind, quantiser, vector, six token counts -- is what the
    description says, so the claims counted over the descriptions are claims about what the parse saw"""
    r = reach_of(sim, BY_NAME[name], 1)
    for s in BY_NAME[name]()["streams"]:
        w = P.written(s)
        rec = r["pictures"][w["name"]][1]
        for t, want in enumerate(census_of(w)["records"]):
            for addr, x in enumerate(want):
                assert x is not None, (w["name"], t, addr)
                flag, q, mvh, mvv, counts = x
                v = [int(a) for a in rec[t, addr]]
                got_counts = tuple(((v[2] | ((v[3] & 0xffff) << 32)) >> (8 * b)) & 255 for b in range(6))
                got = ((v[3] >> 16) & 0x60, (v[3] >> 16) & 31, ((v[1] & 0xffff) ^ 0x8000) - 0x8000, ((v[1] >> 16) ^ 0x8000) - 0x8000, got_counts)
                # a block of 64 tokens: its count's byte holds 64
                assert got == (flag, q, mvh, mvv, counts), (w["name"], t, addr, got, x)


# what each set reaches, with the service in two halves / in one piece where they differ: exact figures (python
# tests/test_parse_edges.py prints them).  max_turn_bits: see the module's text; min_room_turn 168 = JM_STEP_BITS + 32 is the least
# the blocked rule lets a lane begin a turn with; max_occ_turn 24 = JM_TK_RING - 2 - JM_COEF_SLOTS * JM_COEF_REPEAT likewise.
REACH = {
    ('symbols', 1): {'max_turn_bits': 39, 'max_step_bits': [32, 16, 10, 28], 'min_room': 140, 'min_room_turn': 168, 'min_margin': 106, 'max_occ_turn': 24, 'max_occ_after': 30},
    ('symbols', 0): {'max_turn_bits': 39, 'max_step_bits': [32, 16, 10, 28], 'min_room': 140, 'min_room_turn': 168, 'min_margin': 106, 'max_occ_turn': 24, 'max_occ_after': 29},
    ('phases', 1): {'max_turn_bits': 72, 'max_step_bits': [43, 16, 10, 28], 'min_room': 129, 'min_room_turn': 168, 'min_margin': 91, 'max_occ_turn': 24, 'max_occ_after': 28},
    ('phases', 0): {'max_turn_bits': 72, 'max_step_bits': [43, 16, 10, 28], 'min_room': 131, 'min_room_turn': 168, 'min_margin': 99, 'max_occ_turn': 24, 'max_occ_after': 28},
    ('worst_turns', 1): {'max_turn_bits': 102, 'max_step_bits': [64, 16, 10, 28], 'min_room': 77, 'min_room_turn': 169, 'min_margin': 35, 'max_occ_turn': 24, 'max_occ_after': 28},
    ('worst_turns', 0): {'max_turn_bits': 102, 'max_step_bits': [64, 16, 10, 28], 'min_room': 77, 'min_room_turn': 169, 'min_margin': 35, 'max_occ_turn': 24, 'max_occ_after': 28},
    ('tails', 1): {'max_turn_bits': 37, 'max_step_bits': [22, 10, 9, 28], 'min_room': 136, 'min_room_turn': 168, 'min_margin': 104, 'max_occ_turn': 24, 'max_occ_after': 30},
    ('tails', 0): {'max_turn_bits': 37, 'max_step_bits': [22, 10, 9, 28], 'min_room': 136, 'min_room_turn': 168, 'min_margin': 104, 'max_occ_turn': 24, 'max_occ_after': 30},
    ('company', 1): {'max_turn_bits': 46, 'max_step_bits': [35, 10, 10, 28], 'min_room': 136, 'min_room_turn': 168, 'min_margin': 95, 'max_occ_turn': 24, 'max_occ_after': 28},
    ('company', 0): {'max_turn_bits': 46, 'max_step_bits': [35, 10, 10, 28], 'min_room': 140, 'min_room_turn': 168, 'min_margin': 100, 'max_occ_turn': 24, 'max_occ_after': 28},
}


@SPLITS
@pytest.mark.parametrize("name", SETS)
def test_what_the_set_reaches(name, split, sim):  # noqa: F811
    K = constants(sim)
    r = reach_of(sim, BY_NAME[name], split)
    got = {k: r[k] for k in ("max_turn_bits", "max_step_bits", "min_room", "min_room_turn", "min_margin", "max_occ_turn", "max_occ_after")}
    print(name, split, got)
    assert got == REACH[(name, split)]
    # the bounds the header states, for every set
    assert r["max_turn_bits"] <= 102 <= K["STEP_BITS"] == 136
    assert r["min_room_turn"] >= K["STEP_BITS"] + 32
    assert r["min_margin"] >= 0                                   # at every step: head-room >= 32 + the bits that step consumed
    blocked_at = K["TK_RING"] - 2 - K["COEF_SLOTS"] * K["COEF_REPEAT"]
    assert r["max_occ_turn"] <= blocked_at == 24 and r["max_occ_after"] <= K["TK_RING"] == 32
    assert all(r["tails"][n] == 0 for n in range(1, 16, 2))       # no odd tail on a valid stream


@SPLITS
def test_the_turn_bound(split, sim):  # noqa: F811
    """worst_turns() reaches the attainable maximum, 102 bits in one turn (COLD 64 + SLOW 28 + COEF 10; the intra form 75), every
    step kind its own maximum, and does so with the least head-room a turn may begin with -- see the module's text for why
    it is not JM_STEP_BITS"""
    r = reach_of(sim, P.worst_turns, split)
    assert r["max_turn_bits"] == 102 == P.worst_turns()["claims"]["turn_bits_p"]
    assert r["max_step_bits"] == [64, 16, 10, 28]                 # COLD, DC (a chroma block's 8 + 8), COEF (a full pair look), SLOW
    assert r["min_margin"] >= 0


@SPLITS
def test_phases_alone_meets_every_bit_phase_and_every_wrap(split, sim):  # noqa: F811
    r = reach_of(sim, P.phases, split)
    for k in range(4):
        assert all(r["phase"][k][p] > 0 for p in range(32)), (KINDS[k], [p for p in range(32) if not r["phase"][k][p]])
    for k in range(4):
        assert 0 < r["span_wrap"][k] < r["span_chunk"][k] < r["span_row"][k], KINDS[k]
    # the slice header's looks (jm_lane_init) lie in the slice's first chunks: every phase, row and chunk boundaries, never the wrap
    assert all(r["phase"][4]) and r["span_chunk"][4] > 0 and r["span_wrap"][4] == 0


@SPLITS
def test_the_token_ring_and_the_refill_are_driven_to_their_limits(split, sim):  # noqa: F811
    K = constants(sim)
    tails = [0] * 16
    drains = [0, 0]
    occ_turn = occ_after = held = later = 0
    served = [0] * 5
    for fn in P.SETS:
        r = reach_of(sim, fn, split)
        tails = [a + b for a, b in zip(tails, r["tails"])]
        drains = [a + b for a, b in zip(drains, r["drains"])]
        served = [a + b for a, b in zip(served, r["served"])]
        occ_turn, occ_after = max(occ_turn, r["max_occ_turn"]), max(occ_after, r["max_occ_after"])
        held += r["held_back"]
        later += r["landed_later"]
    assert all(tails[n] > 0 for n in range(0, 16, 2)) and all(tails[n] == 0 for n in range(1, 16, 2)), tails
    assert drains[0] > 0 and drains[1] > 0
    assert occ_turn == K["TK_RING"] - 2 - K["COEF_SLOTS"] * K["COEF_REPEAT"] and occ_after <= K["TK_RING"]
    dense = reach_of(sim, P.worst_turns, split)
    assert dense["max_occ_turn"] == 24 and dense["max_occ_after"] == REACH[("worst_turns", split)]["max_occ_after"]
    # a lane is given two chunks, three after its longest turns, four at its slice's start -- and never ONE: JM_REFILL_MIN = 2 holds
    # a single chunk back unless the lane is blocked, and a blocked lane (less than 168 bits left) has room for two
    assert held > 0 and served[1] == 0 and all(served[n] > 0 for n in (2, 3, 4)) and K["REFILL_MIN"] == 2, (held, served)
    assert (later > 0) == bool(split)


@pytest.mark.reference
@pytest.mark.skipif(not have_reference(), reason="needs /root/reference")
@pytest.mark.parametrize("name", SETS)
def test_reference_equals_oracle(name, libs):
    """the reference's own C on every stream: these are valid streams, so the oracle the GPU tests lean on must agree"""
    for s in BY_NAME[name]()["streams"]:
        w = P.written(s)
        assert cabi.decode_stream(libs["ref"], w["es"])[0] == oracle_md5(libs, w), w["name"]


def reach_report():
    import glob
    import os
    import subprocess
    from conftest import ROOT
    so = os.path.join(ROOT, "tests", "sim", "libjsmpeg_sim.so")
    csrc = os.path.join(ROOT, "jsmpeg_amd", "csrc")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-Wno-unknown-pragmas", "-I", csrc, "-o", so,
                           os.path.join(ROOT, "tests", "sim", "sim_decode.cpp")])
    lib = ctypes.CDLL(so)
    lib.sim_decode_stream.restype = ctypes.c_int
    lib.sim_stale_windows.restype = ctypes.c_ulonglong
    lib.sim_decode_stream.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_int]
    for fn in P.SETS:
        for split in (1, 0):
            r = reach_of(lib, fn, split)
            print("    (%r, %d): %r," % (fn.__name__, split, {k: r[k] for k in ("max_turn_bits", "max_step_bits", "min_room", "min_room_turn", "min_margin",
                                                                                   "max_occ_turn", "max_occ_after")}))
            print("#", {k: r[k] for k in ("span_row", "span_chunk", "span_wrap", "drains", "tails", "held_back", "served", "landed_later", "turn_steps", "stale")})
            print("#  phases with no look:", {KINDS[k]: [p for p in range(32) if not r["phase"][k][p]] for k in range(5)})


if __name__ == "__main__":
    reach_report()
