#!/usr/bin/env python3
"""Times the log-mel features (C ABI part 12) against what a host does today without them, on the same GPU in the same run:
torch.stft + a matmul with the same filterbank + log10 and the clamp, in float32.

  A: 64 streams x 30 s at 16 kHz, the Whisper config (n_fft 400, hop 160, 80 Slaney bands), scale "whisper", one call with END
  B: 64 chained streams x 384 samples per tick, scale "log10" (the baseline keeps its own 240-sample history per stream and
     runs torch.stft(center=False) over history + tick)

Prints one JSON line per case: device milliseconds per call (the median over --steps calls, torch events around the enqueue)
for the features and for the baseline, their ratio, the kernel's own time and its FLOP rate (the DFT's 2 n_fft cols flops per
frame, useful columns and issued ones), the largest difference between the two results, and for A the same call with the
naive LDS map (JSMPEG_HIP_LOGMEL_NO_SKEW, same results).  profiles/logmel_notes.md keeps what was measured."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

WHISPER = dict(sample_rate=16000, n_fft=400, hop=160, n_mels=80, f_min=0.0, f_max=8000.0, mel_scale="slaney", mel_norm="slaney")


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


def mel_torch(torch, x, fb, window, center):
    z = torch.stft(x, 400, hop_length=160, window=window, center=center, pad_mode="reflect", return_complex=True)
    return torch.matmul(fb, z.real * z.real + z.imag * z.imag)


def whisper_torch(torch, x, fb, window):
    l = torch.clamp(mel_torch(torch, x, fb, window, True), min=1e-10).log10()
    l = torch.maximum(l, l.amax(dim=(1, 2), keepdim=True) - 8.0)
    return (l + 4.0) / 4.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=64)
    ap.add_argument("--seconds", type=int, default=30)
    ap.add_argument("--tick", type=int, default=384)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    import torch
    from jsmpeg_amd import logmel
    r = np.random.default_rng(1)
    n = 16000 * a.seconds
    x = torch.from_numpy(r.uniform(-0.5, 0.5, (a.streams, n)).astype(np.float32)).cuda()
    fb = torch.from_numpy(logmel.filters(**WHISPER)[0]).cuda()
    window = torch.hann_window(400, periodic=True, device="cuda")
    frames = n // 160 + 1
    cols = logmel.plan(**WHISPER)["cols"]

    base_ms = timed(torch, lambda: whisper_torch(torch, x, fb, window), a.steps, a.warmup)
    want = whisper_torch(torch, x, fb, window).cpu().numpy()
    for label, env in (("skewed", None), ("naive", "1")):
        if env:
            os.environ["JSMPEG_HIP_LOGMEL_NO_SKEW"] = env
        else:
            os.environ.pop("JSMPEG_HIP_LOGMEL_NO_SKEW", None)
        with logmel.LogMel(scale="whisper", max_streams=a.streams, max_samples=n, row=frames, **WHISPER) as lm:
            def ours():
                lm.features(x)
                lm.sync()
            ours_ms = timed(torch, ours, a.steps, a.warmup)
            kernel_ms = lm.timings()["kernel_ms"]
            diff = float(np.abs(lm.read() - want).max())
        flop = 2.0 * 400 * a.streams * frames
        print(json.dumps(dict(case="A: %d x %d s, whisper, one call" % (a.streams, a.seconds), lds_map=label, frames=frames, logmel_ms=round(ours_ms, 4),
                              kernels_ms=round(kernel_ms, 4), torch_ms=round(base_ms, 4), ratio=round(base_ms / ours_ms, 2),
                              tflops_useful=round(flop * 402 / kernel_ms / 1e9, 2), tflops_issued=round(flop * cols / kernel_ms / 1e9, 2), max_abs_diff=diff)), flush=True)
    os.environ.pop("JSMPEG_HIP_LOGMEL_NO_SKEW", None)

    ticks = torch.from_numpy(r.uniform(-0.5, 0.5, (8, a.streams, a.tick)).astype(np.float32)).cuda()
    state = dict(history=torch.zeros((a.streams, 240), device="cuda"), i=0)

    def base_tick():
        buf = torch.cat([state["history"], ticks[state["i"] % 8]], dim=1)
        state["i"] += 1
        state["history"] = buf[:, -240:]
        return torch.clamp(mel_torch(torch, buf, fb, window, False), min=1e-10).log10()
    base_ms = timed(torch, base_tick, a.steps, a.warmup)
    with logmel.LogMel(scale="log10", max_streams=a.streams, max_samples=a.tick, **WHISPER) as lm:
        count = dict(i=0)

        def ours_tick():
            lm.features(ticks[count["i"] % 8], chain=True)
            count["i"] += 1
            lm.sync()
        ours_ms = timed(torch, ours_tick, a.steps, a.warmup)
        kernel_ms = lm.timings()["kernel_ms"]
        made = lm.counts()[0]
    print(json.dumps(dict(case="B: %d chained streams x %d samples per tick, log10" % (a.streams, a.tick), frames_per_tick=made, logmel_ms=round(ours_ms, 4),
                          kernels_ms=round(kernel_ms, 4), torch_ms=round(base_ms, 4), ratio=round(base_ms / ours_ms, 2))), flush=True)


if __name__ == "__main__":
    main()
