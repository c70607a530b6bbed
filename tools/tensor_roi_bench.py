"""Tensor rows from regions of interest on one MI355X: 64 decoded 1080p pictures, 16 boxes each (sides 32 .. 400, fixed
seed) -> 224 x 224 f16 NCHW with ImageNet normalisation.  One Batch.tensor_rois call (k_tensor_roi) against the two routes
a host has without it, on the same tree and in the same run: one Batch.tensor(crop=) call per box, and Batch.tensor of the
whole pictures followed by torch crop + F.interpolate per box.  Device-event timing after warm-up, `--reps` repeats; one
JSON record (--out).  Nothing here is tuned towards a result: the three routes get the same boxes and the same output."""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402  (the benchmark's content generator)
from jsmpeg_amd import batch as jb  # noqa: E402

W, H = 1920, 1080
SIZE = (224, 224)
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def timed(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def make_boxes(pictures, per_picture, seed):
    rng = np.random.default_rng(seed)
    rois = []
    for p in range(pictures):
        for _ in range(per_picture):
            bw, bh = (int(v) for v in rng.integers(32, 401, 2))
            rois.append((p, int(rng.integers(0, W - bw + 1)), int(rng.integers(0, H - bh + 1)), bw, bh))
    return rois


def source_bytes(rois):
    """what a row must read at the least: its box's luma and the chroma under it"""
    return sum(bw * bh + 2 * ((x + bw + 1) // 2 - x // 2) * ((y + bh + 1) // 2 - y // 2) for _, x, y, bw, bh in rois)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pictures", type=int, default=64)
    ap.add_argument("--boxes", type=int, default=16, help="per picture")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    streams = [g[0] for g in bench.generate_streams(0, a.pictures, 1, "cfg2_1080p")]
    rois = make_boxes(a.pictures, a.boxes, a.seed)
    n = len(rois)
    kw = dict(size=SIZE, dtype=torch.float16, mean=MEAN, std=STD)
    read, written = source_bytes(rois), n * 3 * SIZE[0] * SIZE[1] * 2
    rec = {"content": "cfg2_1080p generator content, %d pictures of 1920x1080, %d boxes each (sides 32 .. 400, seed %d)" % (
        a.pictures, a.boxes, a.seed), "output": "224x224 f16 NCHW, ImageNet mean / std", "reps": a.reps, "rows": n,
        "source_bytes": read, "output_bytes": written}
    with jb.Batch(W, H, a.pictures, a.pictures * 3, sum(len(s) for s in streams) + 4096 * a.pictures, device=0) as b:
        b.upload(streams)
        assert b.decode() == a.pictures and all(i.decoded for i in b.pictures())
        d_rois = torch.tensor(rois, dtype=torch.int32, device="cuda:0")
        out = torch.empty((n, 3) + SIZE, dtype=torch.float16, device="cuda:0")

        def single():
            b.tensor_rois(d_rois, None, out=out, **kw)

        def per_box():
            for r, (p, x, y, bw, bh) in enumerate(rois):
                b.tensor([p], crop=(x, y, bw, bh), out=out[r:r + 1], **kw)

        ms = timed(single, a.warmup, a.reps)
        rec["tensor_rois_one_call"] = {"ms": ms, "read_gbs": read / ms / 1e6, "write_gbs": written / ms / 1e6,
                                       "gbs": (read + written) / ms / 1e6}
        _, status = b.tensor_rois(d_rois, None, out=out, **kw)
        assert bool((status == 1).all())
        want = out.clone()
        ms = timed(per_box, 1, max(1, a.reps // 2))
        assert torch.equal(out, want), "the per-box route gives other rows"
        rec["tensor_crop_call_per_box"] = {"ms": ms, "calls": n}

        # whole pictures at full size (f32, normalised), then crop and antialiased resize per box in torch
        mean = torch.tensor(MEAN, device="cuda:0")[None, :, None, None]
        std = torch.tensor(STD, device="cuda:0")[None, :, None, None]
        full = torch.empty((a.pictures, 3, H, W), dtype=torch.float32, device="cuda:0")

        def whole_then_torch():
            b.tensor(None, out=full)
            for r, (p, x, y, bw, bh) in enumerate(rois):
                v = F.interpolate(full[p:p + 1, :, y:y + bh, x:x + bw], size=SIZE, mode="bilinear", align_corners=False, antialias=True)
                out[r:r + 1] = ((v - mean) / std).half()

        ms = timed(whole_then_torch, 1, max(1, a.reps // 2))
        rec["whole_pictures_then_torch_per_box"] = {"ms": ms, "intermediate_bytes": full.numel() * 4,
                                                    "max_abs_diff_to_one_call": float((out.float() - want.float()).abs().max())}
    one = rec["tensor_rois_one_call"]["ms"]
    rec["speedup_vs_call_per_box"] = rec["tensor_crop_call_per_box"]["ms"] / one
    rec["speedup_vs_whole_then_torch"] = rec["whole_pictures_then_torch_per_box"]["ms"] / one
    print(json.dumps(rec, indent=1))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rec, f, indent=1)


if __name__ == "__main__":
    main()
