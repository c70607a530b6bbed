"""Writes tests/golden/enc_pass_pin.json: an md5 per call of the encoder's CPU simulator over everything the call leaves -- the
whole output buffer, the picture and stream ranges, every reconstruction, of the macroblocks' info words what the helpers give
out (Result.vectors: intra or not, and the vector; the other bits enter only through the counts and the stream's bytes), the
counts by kind, the (q, budget, bytes) triples and the ordinals, where a call has them.  Only the helpers' public functions
are used (ei.sim_encode, ep.sim_encode_p, er.sim_encode_rate, Case.sim, er.sim_long, ec.Chain), so the same writer runs on both
sides of a change to the simulator or to the headers it compiles: tests/test_enc_pass_pin.py recomputes every entry and holds it
to the file.  The file was written BEFORE the simulators were merged into tests/sim/sim_encode_pass.cpp and is only rewritten
when the encoder's output is meant to change:  python tests/golden/make_enc_pass_pin.py"""
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import enc_chain_inputs as ec  # noqa: E402
import enc_inputs as ei  # noqa: E402
import enc_p_inputs as ep  # noqa: E402
import enc_rate_inputs as er  # noqa: E402

PIN = os.path.join(HERE, "enc_pass_pin.json")
GROUPS = ("intra", "p", "rate", "chain")
INTRA_SCALES = (1, 8, 31)
CONFIGS = ((3, 7), (4, 0))             # (gop, search range)
P_SCALES = (1, 8)
RANGE_RADII = (0, 15)
RANGE_GOP = 3
CHAIN_RULES = (None, dict(T=150))
SMALL_NAMES = ("enc_pan_176x144", "enc_wide_search_208x160", "content_176x144", "content_177x145", "flat", "stripes", "one_macroblock")
P_NAMES = ("content_176x144", "content_177x145", "enc_pan_176x144", "whole_pel_pan", "half_pel_pan", "flat_grey", "flat_wide", "one_macroblock",
           "scene_cut", "noise")
RANGE_NAMES = ("noise", "whole_pel_pan", "half_pel_pan", "content_177x145", "one_macroblock", "fast_pan", "checker_ties", "intra_threshold")
RATE_NAMES = ("pan_gop3_T150", "pan_gop4_T100", "pan_T20", "pan_T1500", "pan_gop1", "noise_T1500", "noise_T4000", "flat_grey", "flat_wide",
              "content_177x145", "content_177x145_R0", "one_macroblock", "range_4_16", "range_8_8", "streams_W1", "streams_W16")


def digest(*results):
    """md5 over one or more calls' results: ei.sim_encode's triple, or an ep.Result (with .rate / .ordinals where it has them)"""
    h = hashlib.md5()
    for r in results:
        assert r is not None, "a pinned call overflowed"
        if isinstance(r, tuple):
            buf, ranges, streams = r
            rest = ()
        else:
            buf, ranges, streams = r.triple()
            h.update(repr(r.table).encode())
            for f in r.recon:
                h.update(f.tobytes())
            rest = (r.vectors, r.stats, getattr(r, "rate", None), getattr(r, "ordinals", None))
        h.update(buf)
        h.update(repr((ranges, sorted(streams.items()), rest)).encode())
    return h.hexdigest()


def rule_name(rule):
    return "T%d" % rule["T"] if rule else "no_rule"


def names():
    """every entry the pin must hold, from the lists above alone"""
    out = ["intra/%s/q%d" % (n, q) for n in SMALL_NAMES for q in INTRA_SCALES]
    out += ["intra/streams_176x144/end%d/rate_code%d" % (e, c) for e in (1, 0) for c in (5, 3)]
    out += ["p/%s/gop%d_R%d/q%d" % (n, g, R, q) for n in P_NAMES for g, R in CONFIGS for q in P_SCALES]
    out += ["p/range/%s/R%d" % (n, R) for n in RANGE_NAMES for R in RANGE_RADII]
    out += ["p/long_call/gop7_R1/end%d" % e for e in (1, 0)]
    out += ["rate/%s" % n for n in RATE_NAMES] + ["rate/long_call"]
    out += ["chain/pan7/gop%d_R%d/%s/cuts_%s" % (g, R, rule_name(rule), "-".join(map(str, cuts)))
            for g, R in CONFIGS for rule in CHAIN_RULES for cuts in ec.splits(7)]
    out += ["chain/streams_come_and_go", "chain/unchained_between_chained"]
    return out


def intra_entries(libs):
    small = ei.small_cases(libs)
    assert tuple(small) == SMALL_NAMES
    for name, (frames, w, h) in small.items():
        for q in INTRA_SCALES:
            yield "intra/%s/q%d" % (name, q), digest(ei.sim_encode(frames, w, h, qscale=q))
    frames, w, h = small["enc_pan_176x144"]
    frames = frames + small["content_176x144"][0]
    for end in (1, 0):
        for code in (5, 3):
            yield ("intra/streams_176x144/end%d/rate_code%d" % (end, code),
                   digest(ei.sim_encode(frames, w, h, streams=[0, 0, 2, 3, 3], qscale=[1, 31, 8, 2, 5], frame_rate_code=code, end=bool(end), max_streams=5)))


def p_entries(libs):
    base = ep.p_cases(libs)
    assert tuple(base) == P_NAMES
    for name, (frames, w, h) in base.items():
        for gop, R in CONFIGS:
            for q in P_SCALES:
                yield "p/%s/gop%d_R%d/q%d" % (name, gop, R, q), digest(ep.sim_encode_p(frames, w, h, gop, R, qscale=q))
    ranged = ep.range_cases(libs, base)
    assert tuple(ranged) == RANGE_NAMES
    for name, (frames, w, h) in ranged.items():
        for R in RANGE_RADII:
            yield "p/range/%s/R%d" % (name, R), digest(ep.sim_encode_p(frames, w, h, RANGE_GOP, R))
    frames, w, h, streams, scales = ep.long_call()
    for end in (1, 0):
        yield ("p/long_call/gop7_R1/end%d" % end,
               digest(ep.sim_encode_p(frames, w, h, 7, 1, streams=streams, qscale=scales, end=bool(end), max_streams=ep.LONG_MAX_STREAMS)))


def rate_entries(libs):
    cases = er.rate_cases(libs)
    assert tuple(cases) == RATE_NAMES
    for name, c in cases.items():
        yield "rate/%s" % name, digest(c.sim())
    yield "rate/long_call", digest(er.sim_long(ep.long_call()))


def pan_split(frames, gop, R, rule, cuts):
    """ec.run_split's calls, every call's whole result kept"""
    out, at = [], 0
    with ec.Chain(64, 48) as c:
        c.set_gop(gop, R)
        if rule:
            c.set_rate(rule["T"], rule.get("q_min", 1), rule.get("q_max", 31), rule.get("W", 4))
        for i, n in enumerate(cuts):
            out.append(c.encode(frames[at:at + n], None, 8, end=i + 1 == len(cuts), chain=True))
            at += n
    return out


def come_and_go(PAN):
    """the calls of tests/test_enc_chain_sim.py::test_streams_come_and_go"""
    pan9 = ep.pan_frames(64, 48, 9, (2, 1))
    own = {0: PAN[:7], 2: pan9[:4], 5: pan9[2:8]}
    calls = [((0, 2, 5), False), ((0, 2, 5), False), ((0, 5), False), ((0,), True), ((0, 2, 5), False), ((0, 2, 5), False)]
    out, at = [], {s: 0 for s in own}
    with ec.Chain(64, 48, 6) as c:
        c.set_gop(3, 7)
        for i, (present, end) in enumerate(calls):
            if i == 2:
                c.chain_reset(5)
            frames = [own[s][at[s]] for s in present]
            for s in present:
                at[s] += 1
            out.append(c.encode(frames, list(present), end=end))
    return out


def unchained_between(PAN, noise):
    """the calls of tests/test_enc_chain_sim.py::test_unchained_calls_between_chained_ones"""
    out = []
    with ec.Chain(64, 48, 2) as c:
        c.set_gop(3, 7)
        for a, b in ((0, 2), (2, 3), (3, 7)):
            out.append(c.encode(PAN[a:b], None, 8, end=b == 7))
            for frames, streams in ((noise, None), (PAN[4:7] + noise[:2], [0, 0, 0, 1, 1])):
                out.append(c.encode(frames, streams, 5, end=True, chain=False))
    with ec.Chain(64, 48, 7) as c:
        pan9 = ep.pan_frames(64, 48, 9, (2, 1))
        c.set_gop(3, 7)
        c.set_rate(120, 1, 31, 4)
        out.append(c.encode(pan9[:2], [2, 2]))
        out.append(c.encode(pan9, er.PAN_STREAMS, end=True, chain=False))
    return out


def chain_entries(libs):
    PAN = ep.pan_frames(64, 48, 8, (3, -2))
    for gop, R in CONFIGS:
        for rule in CHAIN_RULES:
            for cuts in ec.splits(7):
                yield ("chain/pan7/gop%d_R%d/%s/cuts_%s" % (gop, R, rule_name(rule), "-".join(map(str, cuts))),
                       digest(*pan_split(PAN[:7], gop, R, rule, cuts)))
    yield "chain/streams_come_and_go", digest(*come_and_go(PAN))
    yield "chain/unchained_between_chained", digest(*unchained_between(PAN, ep.p_cases(libs)["noise"][0]))


def entries(libs, group):
    return dict({"intra": intra_entries, "p": p_entries, "rate": rate_entries, "chain": chain_entries}[group](libs))


def main():
    from jsmpeg_amd import build
    libs = {"synth": build.build_synth(), "oracle": build.build_oracle(), "ref": build.build_ref()}
    pin = {}
    for group in GROUPS:
        pin.update(entries(libs, group))
    assert sorted(pin) == sorted(names())
    with open(PIN, "w") as f:
        json.dump(pin, f, indent=0, sort_keys=True)
        f.write("\n")
    print("%d entries -> %s" % (len(pin), PIN))


if __name__ == "__main__":
    main()
