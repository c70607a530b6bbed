"""C ABI part 7 on one MI355X: decoded 1080p pictures -> resized RGB tensors (k_tensor), against the device-copy rate of
the same run and against the composite path a host builds today (render_rgba_device + .float() + F.interpolate(antialias)
+ normalise + .half()).  Content: bench.py's cfg2 generator content (64 streams x 120 pictures).  Device-event timing after
warm-up, `--reps` repeats; one JSON record (--out).  Kernel times: run it under `rocprofv3 --kernel-trace --stats`."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402  (the benchmark's content generator)
from jsmpeg_amd import batch as jb, live as jl  # noqa: E402

W, H = 1920, 1080
PLANES = W * H * 3 // 2                      # 3,110,400 B read per picture


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


def copy_rate(warmup, reps):
    """tools/hbm_copy_probe.py's method: a device-to-device copy of a large tensor, bytes read + written per second"""
    n = 1 << 31
    x = torch.ones(n, dtype=torch.uint8, device="cuda")
    y = torch.empty_like(x)
    ms = timed(lambda: y.copy_(x), warmup, reps)
    del x, y
    torch.cuda.empty_cache()
    return 2 * n / ms / 1e6          # GB/s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=64)
    ap.add_argument("--frames", type=int, default=120)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--identity", type=int, default=1024, help="pictures of the identity and composite rows")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    gen = bench.generate_streams(0, a.streams, a.frames, "cfg2_1080p")
    streams = [g[0] for g in gen]
    rec = {"content": "cfg2_1080p generator content, %d streams x %d pictures, 1920x1080" % (a.streams, a.frames), "reps": a.reps}
    rec["copy_gbs"] = copy_rate(a.warmup, a.reps)
    with jb.Batch(W, H, a.streams, a.streams * (a.frames + 1), sum(len(s) for s in streams) + 4096 * a.streams, device=0) as b:
        b.upload(streams)
        n = b.decode()
        assert all(i.decoded for i in b.pictures()), "every picture of the content is decoded (I / P)"
        rows = {}

        def row(name, count, size, antialias, bytes_per_pic):
            out = torch.empty((count, 3) + size, dtype=torch.float16, device="cuda:0")
            pics = list(range(count))
            ms = timed(lambda: b.tensor(pics, size=size, dtype=torch.float16, antialias=antialias, out=out), a.warmup, a.reps)
            total = bytes_per_pic * count
            bound = total / (rec["copy_gbs"] * 1e6)
            rows[name] = {"pictures": count, "ms": ms, "algorithmic_bytes": total, "gbs": total / ms / 1e6,
                          "copy_bound_ms": bound, "ratio_to_copy_bound": ms / bound}
            del out
            torch.cuda.empty_cache()

        row("aa_1080p_to_224_f16_nchw", n, (224, 224), True, PLANES + 224 * 224 * 3 * 2)
        row("plain_1080p_to_224_f16_nchw", n, (224, 224), False, PLANES + 224 * 224 * 3 * 2)
        m = min(a.identity, n)
        row("identity_1080p_f16_nchw", m, (H, W), True, PLANES + H * W * 3 * 2)
        row("aa_1080p_to_224_f16_nchw_%d" % m, m, (224, 224), True, PLANES + 224 * 224 * 3 * 2)

        # the composite path of today, in chunks (memory): RGBA at full size, float, antialiased resize, normalise, half
        chunk = 128
        rgba = torch.empty((chunk, H, W, 4), dtype=torch.uint8, device="cuda:0")
        res = torch.empty((m, 3, 224, 224), dtype=torch.float16, device="cuda:0")
        stream = torch.cuda.current_stream().cuda_stream

        def composite():
            for f in range(0, m, chunk):
                c = min(chunk, m - f)
                b.render_rgba_device(f, c, rgba.data_ptr(), stream)
                x = rgba[:c, :, :, :3].permute(0, 3, 1, 2).float()
                y = F.interpolate(x, size=(224, 224), mode="bilinear", align_corners=False, antialias=True)
                res[f:f + c] = (y / 255.0).half()
        ms = timed(composite, 1, max(1, a.reps // 2))
        fused = rows["aa_1080p_to_224_f16_nchw_%d" % m]["ms"]
        rows["composite_render_rgba_float_interpolate_%d" % m] = {"pictures": m, "ms": ms, "fused_ms": fused, "speedup_fused": ms / fused}
        del rgba, res
        torch.cuda.empty_cache()
        rec["rows"] = rows

    # latest_tensor: 64 live 1080p streams, the newest frame of each -> one 224x224 f16 batch; host clock around call + sync
    offs = [g[1] for g in gen]
    with jl.Live(W, H, a.streams, pictures_per_tick=1, store_bytes=1 << 20, device=0) as lv:
        ids = [lv.open() for _ in range(a.streams)]
        for i, (es, of) in zip(ids, zip(streams, offs)):
            lv.write(i, es[int(of[0]):int(of[1])])
        assert lv.tick(flush=True) == a.streams
        out = torch.empty((a.streams, 3, 224, 224), dtype=torch.float16, device="cuda:0")
        for _ in range(a.warmup + 3):
            lv.latest_tensor(ids, size=(224, 224), dtype=torch.float16, out=out)
        torch.cuda.synchronize()
        times = []
        for _ in range(50):
            t0 = time.perf_counter()
            lv.latest_tensor(ids, size=(224, 224), dtype=torch.float16, out=out)
            torch.cuda.synchronize()
            times.append((time.perf_counter() - t0) * 1e3)
        rec["rows"]["latest_tensor_64_live_1080p_to_224_f16"] = {"streams": a.streams, "median_ms": float(np.median(times)),
                                                                "min_ms": float(np.min(times)), "read_bytes": PLANES * a.streams}
    print(json.dumps(rec, indent=1))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rec, f, indent=1)


if __name__ == "__main__":
    main()
