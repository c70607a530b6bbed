"""Measures the intra encoder's integer transform against a float64 one on the CPU build (the simulator of
tests/sim/sim_encode_pass.cpp against tests/enc_ref.py with scipy's dctn), over the inputs of tests/enc_inputs.py, and writes
the figures: profiles/enc_bounds.json (tests/test_enc_sim.py reads its bounds from it) and the quality section of
profiles/enc_notes.md.  No GPU.

    python tools/enc_quality.py
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import enc_inputs  # noqa: E402
from jsmpeg_amd import build  # noqa: E402

NOTES = os.path.join(ROOT, "profiles", "enc_notes.md")
BOUNDS = os.path.join(ROOT, "profiles", "enc_bounds.json")


def replace_section(path, name, text):
    """the text between <!-- name --> and <!-- /name --> of a notes file (appended when the markers are not there)"""
    begin, end = "<!-- %s -->" % name, "<!-- /%s -->" % name
    body = open(path).read() if os.path.exists(path) else "# Intra encoder: notes\n"
    block = "%s\n%s\n%s" % (begin, text.strip("\n"), end)
    if begin in body and end in body:
        body = body[:body.index(begin)] + block + body[body.index(end) + len(end):]
    else:
        body = body.rstrip("\n") + "\n\n" + block + "\n"
    with open(path, "w") as f:
        f.write(body)


def main():
    libs = {"oracle": build.build_oracle(), "ref": build.build_ref()}
    cases = enc_inputs.quality_cases(libs)
    m = enc_inputs.measure_quality(libs, cases)
    with open(BOUNDS, "w") as f:
        json.dump({"inputs": sorted(cases), "scales": {str(q): dict(gap_db=v["gap_db"], share=v["share"]) for q, v in m.items()}}, f, indent=1)
        f.write("\n")
    lines = ["## Quality of the integer transform (CPU build, measured by tools/enc_quality.py)", "",
             "The encoder's levels and streams (the simulator runs the kernels' own device functions) against the same encoder with a",
             "float64 `scipy.fft.dctn` and `np.rint` in place of the 14-bit integer transform, over: " + ", ".join(sorted(cases)) + ".",
             "Luma PSNR is of decode(stream) against the source, over the display area, all pictures pooled.", "",
             "| q | levels | differing share | largest difference | PSNR integer (dB) | PSNR float64 (dB) | gap (dB) |",
             "|---|---|---|---|---|---|---|"]
    for q, v in m.items():
        lines.append("| %d | %d | %.3e | %d | %.4f | %.4f | %+.5f |" % (q, v["levels"], v["share"], v["worst"], v["psnr_int"], v["psnr_float"], v["gap_db"]))
    lines += ["", "tests/test_enc_sim.py holds a run to: no level off by more than 1; the share at most twice the one above; the PSNR gap",
              "at most the one above plus a tenth of it; and, as a condition, a gap of at most 0.1 dB at every q >= 2."]
    replace_section(NOTES, "quality", "\n".join(lines))
    for q, v in m.items():
        print(q, v)


if __name__ == "__main__":
    main()
