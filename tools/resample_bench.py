#!/usr/bin/env python3
"""Times the PCM resampler (C ABI part 11) against what a host does today without it, on the same GPU in the same run:
the same PCM tensor resampled with torch.nn.functional.conv1d, one strided convolution per phase.

  64 streams x 154 frames (3.7 s of 48 kHz audio each)
  A: 48000 -> 16000, mono, float16 waveform     (audio for a speech model)
  B: 48000 -> 32000, stereo, frames             (an audio rendition for the MP2 encoder)

Prints one JSON line per case: device milliseconds per call (the median over --steps calls, torch events around the enqueue)
for the resampler and for the baseline, their ratio, and the largest difference between the two results (the baseline sums
in another order, so it is close, not equal).  profiles/resample_notes.md keeps what was measured."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

FRAME = 1152


def baseline(torch, x, taps, L, M, H, mono, dtype):
    """x: [S, F, 2, 1152] float32 -> [S, channels, count]: per residue r of the output ordinal modulo L one conv1d of stride M
    (m = r + L k has n = floor(r M / L) + M k and phase (r M) mod L), the results interleaved"""
    F = torch.nn.functional
    S, frames = x.shape[0], x.shape[1]
    w = x.permute(0, 2, 1, 3).reshape(S, 2, frames * FRAME)
    if mono:
        w = 0.5 * (w[:, :1] + w[:, 1:])
    C = w.shape[1]
    count = -((-frames * FRAME * L) // M)
    per = -(-count // L)
    w = F.pad(w, (2 * H - 1, per * M + 2 * H)).reshape(S * C, 1, -1)
    outs = []
    for r in range(L):
        n0, p = (r * M) // L, (r * M) % L
        outs.append(F.conv1d(w[:, :, n0:], taps[p].reshape(1, 1, -1), stride=M)[:, 0, :per])
    y = torch.stack(outs, dim=-1).reshape(S, C, per * L)[:, :, :count]
    return y.to(dtype)


def timed(torch, fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=64)
    ap.add_argument("--frames", type=int, default=154)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    import torch
    from jsmpeg_amd import resample
    r = np.random.default_rng(1)
    x = torch.from_numpy(r.uniform(-1, 1, (a.streams, a.frames, 2, FRAME)).astype(np.float32)).cuda()
    cases = [("48000->16000 mono f16 waveform", 48000, 16000, 1, "waveform", "float16"),
             ("48000->32000 stereo frames", 48000, 32000, 2, "frames", "float32")]
    for name, fin, fout, ch, form, dtype in cases:
        L, M, H = resample.plan(fin, fout)
        taps = torch.from_numpy(resample.taps(fin, fout)).cuda()
        tdt = {"float16": torch.float16, "float32": torch.float32}[dtype]
        with resample.Resampler(fin, fout, channels=ch, form=form, dtype=dtype, max_streams=a.streams, max_frames=a.streams * a.frames,
                                row=resample.outputs(fin, fout, a.frames * FRAME) if form == "waveform" else None) as rs:
            def ours():
                rs.resample_tensor(x)
                rs.sync()
            ours_ms = timed(torch, ours, a.steps, a.warmup)
            kernel_ms = rs.timings()["kernel_ms"]
            base_ms = timed(torch, lambda: baseline(torch, x, taps, L, M, H, ch == 1, tdt), a.steps, a.warmup)
            want = baseline(torch, x, taps, L, M, H, ch == 1, tdt).float().cpu().numpy()
            got = rs.read()
            if form == "frames":                                  # whole frames only: compare what both have
                n = got.shape[0] // a.streams
                got = got.reshape(a.streams, n, 2, FRAME).transpose(0, 2, 1, 3).reshape(a.streams, 2, n * FRAME)
                want = want[:, :, :n * FRAME]
            diff = float(np.abs(got.astype(np.float32) - want).max())
        print(json.dumps(dict(case=name, streams=a.streams, frames=a.frames, resampler_ms=round(ours_ms, 4), resampler_kernel_ms=round(kernel_ms, 4),
                              conv1d_ms=round(base_ms, 4), ratio=round(base_ms / ours_ms, 2), max_abs_diff=diff)), flush=True)


if __name__ == "__main__":
    main()
