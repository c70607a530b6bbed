"""What a rendition loses on the way through RGB, from the CPU restatements only (no device): the two 1080p content frames
scaled to 640x360 and 1280x720 (a) directly, plane by plane, by the encoder's rule (tests/enc_scale_ref.py restating
jsmpeg_amd/csrc/enc_scale.h) and (b) through Batch.tensor(uint8) + encode_tensor as restated by tests/tensor_ref.py (integer
BT.601 to RGB, torch's antialiased resize, rounding to uint8) and tests/enc_ref.py (RGB back to Y | Cr | Cb, chroma averaged
2x2).  Mean and maximum absolute difference per plane kind, and how far the direct rule is from torch's unrounded float on the
tests' named cases.  Writes the `loss` section of profiles/enc_scale_notes.md.
    python tools/enc_scale_loss.py"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

W, H = 1920, 1080
SIZES = ((640, 360), (1280, 720))


def rgb_route(frame, ow, oh):
    import enc_ref
    import tensor_ref
    cw, ch = enc_ref.coded(W, H)
    src = tensor_ref.rgb(*tensor_ref.planes(frame, cw, ch), W, H)
    u8 = tensor_ref.reference(src, (oh, ow), None, True, u8=True).numpy().astype(np.uint8)
    return enc_ref.rgb_to_frame(np.ascontiguousarray(u8.transpose(1, 2, 0)))


def excess_over_half():
    """the worst |direct rule - torch's unrounded float| - 0.5 over the tests' named cases"""
    import torch
    import torch.nn.functional as F
    import enc_scale_inputs as si
    import enc_scale_ref as es
    worst = {}
    for name, (w, h, crop, ow, oh, aa) in sorted(si.CASES.items()):
        m = None
        for f in si.case_frames(name):
            for p, got in zip(es.crops(f, w, h, crop), es.scaled_planes(f, w, h, ow, oh, crop, bool(aa))):
                if got.shape == p.shape or (got.shape[1] == 1 and got.shape[0] != p.shape[0]):
                    continue
                x = torch.from_numpy(np.ascontiguousarray(p)).float()[None, None]
                want = F.interpolate(x, size=got.shape, mode="bilinear", align_corners=False, antialias=bool(aa))[0, 0].numpy()
                m = max(m or 0.0, float(np.abs(got - want.astype(np.float64)).max()))
        worst[name] = None if m is None else m - 0.5
    return worst


def main():
    import enc_ref
    import enc_scale_inputs as si
    import enc_scale_ref as es
    from enc_quality import replace_section
    frames = si.case_frames("7_1080p_to_640x360")
    lines = ["## What the route through RGB loses (CPU restatements only, measured by tools/enc_scale_loss.py)", "",
             "The two 1080p content frames, scaled directly by the rule and through `Batch.tensor(uint8)` + `encode_tensor` (integer BT.601 to RGB,",
             "torch's antialiased resize, uint8, RGB back to Y | Cr | Cb with the chroma averaged 2x2).  Absolute difference over the display area:", "",
             "| to | plane | mean | max |", "|---|---|---|---|"]
    for ow, oh in SIZES:
        d = {"Y": [], "Cr": [], "Cb": []}
        for f in frames:
            a = es.source_planes(es.scale_frame(f, W, H, ow, oh), ow, oh)
            b = es.source_planes(rgb_route(f, ow, oh), ow, oh)
            for name, pa, pb, (pw, ph) in zip(("Y", "Cr", "Cb"), a, b, ((ow, oh), ((ow + 1) >> 1, (oh + 1) >> 1), ((ow + 1) >> 1, (oh + 1) >> 1))):
                d[name].append(np.abs(pa[:ph, :pw].astype(np.int32) - pb[:ph, :pw].astype(np.int32)))
        for name in ("Y", "Cr", "Cb"):
            v = np.concatenate([x.ravel() for x in d[name]])
            lines.append("| %dx%d | %s | %.3f | %d |" % (ow, oh, name, float(v.mean()), int(v.max())))
    worst = excess_over_half()
    lines += ["", "## The rule against torch (CPU, tests' named cases)", "",
              "Worst |integer value - F.interpolate's unrounded float| - 0.5 per case (ties in the rounding plus the 14-bit weights):", "",
              "| case | excess over 0.5 |", "|---|---|"]
    lines += ["| %s | %s |" % (k, "(a copy)" if v is None else "%.5f" % v) for k, v in worst.items()]
    top = max(v for v in worst.values() if v is not None)
    lines += ["", "The worst is %.5f; tests/test_enc_scale_sim.py holds every case to 0.5 + E with E = 0.0125, a little more than twice that (the ceiling is 0.05)." % top, ""]
    replace_section(os.path.join(ROOT, "profiles", "enc_scale_notes.md"), "loss", "\n".join(lines))
    print("\n".join(lines))
    return 0


if __name__ == "__main__":
    sys.exit(main())
