"""What rate control (jsmpeg_amd/csrc/enc_rate.h) does on the test cases, CPU build: per case of tests/enc_rate_inputs.py the
chosen scales and the total bytes against n * T, from the simulator of the kernels (tests/sim/sim_encode_pass.cpp).  Writes the
`cases` section of profiles/enc_rate_notes.md.  No device.
    python tools/enc_rate_table.py"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for d in ("", "tools", "tests", os.path.join("tests", "enc")):
    sys.path.insert(0, os.path.join(ROOT, d))


def main():
    import enc_p_inputs as ep
    import enc_rate_inputs as er
    from enc_quality import replace_section
    from jsmpeg_amd import build
    libs = {"oracle": build.build_oracle(), "ref": build.build_ref()}
    lines = ["## What the rule does on the test cases (CPU build, written by tools/enc_rate_table.py)", "",
             "Bytes are the pictures' (`picture_range`), without end codes and gaps.  Over budget: pictures that fit at no scale of the",
             "range and were written at q_max.", "",
             "| case | size, pictures | gop, search | T | range, W | chosen q | bytes | of n * T | over budget |", "|---|---|---|---|---|---|---|---|---|"]
    rows = [(name, c, c.sim()) for name, c in er.rate_cases(libs).items()]
    long_call = ep.long_call()
    rows.append(("long call", er.Case(long_call[0], long_call[1], long_call[2], er.LONG_GOP, er.LONG_SEARCH, streams=long_call[3], **er.LONG_RULE), er.sim_long(long_call)))
    for name, c, r in rows:
        n = len(c.frames)
        qs = [v[0] for v in r.rate]
        chosen = " ".join(str(q) for q in qs) if n <= 16 else ", ".join("%d x q %d" % (qs.count(q), q) for q in sorted(set(qs)))
        lines.append("| %s | %d x %d, %d | %d, %d | %d | %d .. %d, %d | %s | %d | %d | %d |" % (
            name, c.width, c.height, n, c.gop, c.search, c.T, c.q_min, c.q_max, c.W, chosen, sum(v[2] for v in r.rate), n * c.T,
            sum(1 for v in r.rate if v[2] > v[1])))
    replace_section(os.path.join(ROOT, "profiles", "enc_rate_notes.md"), "cases", "\n".join(lines))
    return 0


if __name__ == "__main__":
    sys.exit(main())
