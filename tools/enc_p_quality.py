"""Measures the encoder's I + P streams on the CPU build (the simulator of tests/sim/sim_encode_pass.cpp, gop 12, search range 7)
against the project's intra encoder at the same quantiser scale -- the yardstick: what the library could do before -- and writes
profiles/enc_p_bounds.json (tests/test_enc_p_sim.py holds a fresh run to it) and the quality section of profiles/enc_p_notes.md.
Luma PSNR of the oracle's decode against the source, over the display area.  No GPU.

    python tools/enc_p_quality.py
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import enc_inputs as ei  # noqa: E402
import enc_p_inputs as ep  # noqa: E402
from jsmpeg_amd import build, cabi  # noqa: E402

NOTES = os.path.join(ROOT, "profiles", "enc_p_notes.md")
BOUNDS = os.path.join(ROOT, "profiles", "enc_p_bounds.json")
SCALES = (1, 2, 8, 31)
GOP, SEARCH, PICTURES = 12, 7, 13


def quality_cases(libs):
    """13 pictures each: one whole GOP and the I picture of the next"""
    return {"content_176x144": (ei.content_frames(176, 144, PICTURES), 176, 144),
            "content_177x145": (ei.content_frames(177, 145, PICTURES), 177, 145),
            "enc_pan_176x144": ei.golden_frames(libs, "enc_pan_176x144", PICTURES)}


def per_picture_sse(libs, es, frames, w, h):
    dec, _, _ = cabi.decode_stream(libs["oracle"], np.ascontiguousarray(es, dtype=np.uint8), keep="planes")
    assert len(dec) == len(frames)
    return [ei.luma_sse([d], [f], w, h)[0] for d, f in zip(dec, frames)]


def measure(libs, cases=None):
    """{str(q): psnr_intra, psnr_ip, gap_db (intra minus I + P), gop_fall_db {case: the fall of the case's PSNR from the first P
    picture of the GOP to its last}, bytes_intra, bytes_ip}"""
    cases = cases or quality_cases(libs)
    out = {}
    for q in SCALES:
        sse_i = sse_p = n_px = bytes_i = bytes_p = 0
        fall = {}
        for name, (frames, w, h) in sorted(cases.items()):
            intra = ei.sim_encode(frames, w, h, qscale=q)
            ip = ep.sim_encode_p(frames, w, h, GOP, SEARCH, qscale=q)
            si = per_picture_sse(libs, ei.stream_of(intra), frames, w, h)
            sp = per_picture_sse(libs, ip.stream(0), frames, w, h)
            sse_i, sse_p, n_px = sse_i + sum(si), sse_p + sum(sp), n_px + len(frames) * w * h
            bytes_i, bytes_p = bytes_i + len(intra[0]), bytes_p + len(ip.buf)
            fall[name] = ei.psnr(sp[1], w * h) - ei.psnr(sp[GOP - 1], w * h)
        out[str(q)] = dict(psnr_intra=ei.psnr(sse_i, n_px), psnr_ip=ei.psnr(sse_p, n_px), gap_db=ei.psnr(sse_i, n_px) - ei.psnr(sse_p, n_px),
                           gop_fall_db=fall, bytes_intra=bytes_i, bytes_ip=bytes_p)
    return out


def main():
    from enc_quality import replace_section
    libs = {"oracle": build.build_oracle(), "ref": build.build_ref()}
    cases = quality_cases(libs)
    m = measure(libs, cases)
    with open(BOUNDS, "w") as f:
        json.dump({"inputs": sorted(cases), "gop": GOP, "search": SEARCH, "scales": m}, f, indent=1)
        f.write("\n")
    lines = ["## Quality of I + P streams (CPU build, measured by tools/enc_p_quality.py)", "",
             "gop %d, search range %d, %d pictures each of: %s.  Luma PSNR of decode(stream) against the source, all pictures pooled;" % (GOP, SEARCH, PICTURES, ", ".join(sorted(cases))),
             "the yardstick is the intra encoder at the same scale.  Fall: the drop of a case's PSNR from the first P picture of the GOP",
             "to its last, per case in the order above (tests/test_enc_p_sim.py holds each case to its own figure).", "",
             "| q | PSNR intra (dB) | PSNR I + P (dB) | gap (dB) | fall along a GOP (dB), per case | bytes intra | bytes I + P |",
             "|---|---|---|---|---|---|---|"]
    for q, v in m.items():
        lines.append("| %s | %.3f | %.3f | %+.3f | %s | %d | %d |" % (q, v["psnr_intra"], v["psnr_ip"], v["gap_db"], " / ".join("%+.3f" % v["gop_fall_db"][c] for c in sorted(cases)),
                                                                       v["bytes_intra"], v["bytes_ip"]))
    replace_section(NOTES, "quality", "\n".join(lines))
    for q, v in m.items():
        print(q, v)


if __name__ == "__main__":
    main()
