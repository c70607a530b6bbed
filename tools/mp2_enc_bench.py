#!/usr/bin/env python3
"""Times the MP2 encoder (C ABI part 9) on the audio of the benchmark batch: 64 streams x 154 frames, stereo 44.1 kHz at
192 kbit/s, PCM already in HBM.  Reports ms per call and frames per second from the handle's device events, the ratio to a
device-to-device copy of the same bytes (PCM in + ES out) timed in the same run, alternating with the encodes, and the live
tick: one frame per stream x 64 streams, chained.  To see what bounds the kernel the batch is also run on silence (no
allocation rounds, nothing to quantise) and on a sine (a few pairs): the differences are the allocation loop and the
quantiser.  Needs an MI355X; prints one JSON line and writes it to --out.

    python tools/mp2_enc_bench.py [--streams 64] [--frames 154] [--steps 20] [--warmup 3] [--out bench_out/mp2_enc_bench.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=64)
    ap.add_argument("--frames", type=int, default=154)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    from jsmpeg_amd import mp2_encode
    if not torch.cuda.is_available():
        raise SystemExit("mp2_enc_bench: no GPU (a time taken elsewhere says nothing)")
    S, F = a.streams, a.frames
    g = torch.Generator(device="cuda").manual_seed(1)
    t = torch.arange(F * 1152, device="cuda", dtype=torch.float32) / 44100.0
    sine = (0.5 * torch.sin(2 * torch.pi * 1000.0 * t)).reshape(F, 1, 1152).expand(S, F, 2, 1152).contiguous()
    inputs = {"noise": 0.1 * torch.randn(S, F, 2, 1152, device="cuda", generator=g), "sine": sine, "silence": torch.zeros(S, F, 2, 1152, device="cuda")}
    es_bytes = mp2_encode.es_bytes([F] * S, 0, 10)
    pcm_bytes = S * F * 2 * 1152 * 4
    src = torch.empty(pcm_bytes + es_bytes, dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(src)
    out = {"streams": S, "frames_per_stream": F, "pcm_bytes": pcm_bytes, "es_bytes": es_bytes, "steps": a.steps}
    with mp2_encode.Mp2Encoder(0, 2, 10, S, S * F, es_bytes) as enc:
        for kind, x in inputs.items():
            kernel, wall, copy = [], [], []
            for i in range(a.warmup + a.steps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                enc.encode_tensor(x)
                enc.sync()
                t1 = time.perf_counter()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                dst.copy_(src)
                e1.record()
                torch.cuda.synchronize()
                if i >= a.warmup:
                    kernel.append(enc.timings()["kernel_ms"])
                    wall.append((t1 - t0) * 1e3)
                    copy.append(e0.elapsed_time(e1))
            k, c = statistics.median(kernel), statistics.median(copy)
            out[kind] = {"kernel_ms": round(k, 4), "kernel_ms_min": round(min(kernel), 4), "kernel_ms_max": round(max(kernel), 4),
                         "call_wall_ms": round(statistics.median(wall), 4), "frames_per_s": round(S * F / (k * 1e-3)),
                         "copy_ms": round(c, 4), "ratio_to_copy": round(k / c, 2), "frame_stats": [enc.frame_stats(k) for k in (0, 1, S * F - 1)]}
    # the live tick: one frame per stream, chained, a call per tick
    with mp2_encode.Mp2Encoder(0, 2, 10, S, S, mp2_encode.es_bytes([1] * S, 0, 10) + 16 * S) as enc:
        x = inputs["noise"]
        kernel, wall = [], []
        for i in range(a.warmup + a.steps):
            tick = x[:, i % F:i % F + 1].contiguous()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            enc.encode_tensor(tick, chain=True)
            enc.sync()
            t1 = time.perf_counter()
            if i >= a.warmup:
                kernel.append(enc.timings()["kernel_ms"])
                wall.append((t1 - t0) * 1e3)
        out["live_tick"] = {"kernel_ms": round(statistics.median(kernel), 4), "call_wall_ms": round(statistics.median(wall), 4),
                            "frames_per_s": round(S / (statistics.median(kernel) * 1e-3))}
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
