"""Writes tests/golden/enc_ts_mux_pin.json: the sha256 of jsmpeg_hip_ts_mux_host's output and the continuity counter it hands
back, over tests/test_ts_mux.py's units_case(1, SIZES) and units_case(4, SIZES) with a start counter of 11.  The file was
written BEFORE the function was rewritten on jsmpeg_amd/csrc/enc_ts.h and is only rewritten when the mux's bytes are meant to
change; tests/test_enc_ts_sim.py recomputes both entries and holds them to the file.  (Not ts_*.json: that pattern is
tests/test_ts_demux.py's, every file of it a demuxer fixture.)  python tests/golden/make_enc_ts_mux_pin.py"""
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

PIN = os.path.join(HERE, "enc_ts_mux_pin.json")
SEEDS = (1, 4)
START = 11


def entries():
    from jsmpeg_amd import encode
    from test_ts_mux import SIZES, units_case
    out = {}
    for seed in SEEDS:
        es, ranges, pts = units_case(seed, SIZES)
        ts, cc = encode.ts_mux(es, ranges, pts, continuity=START)
        out["units_case_%d" % seed] = dict(sha256=hashlib.sha256(ts.tobytes()).hexdigest(), bytes=int(ts.size), continuity_out=cc)
    return out


if __name__ == "__main__":
    with open(PIN, "w") as f:
        json.dump(dict(start=START, cases=entries()), f, indent=1, sort_keys=True)
        f.write("\n")
    print(open(PIN).read())
