"""The resampler's rule (jsmpeg_amd/csrc/pcm_resample.h) restated in numpy float64, and the inputs of its tests.  Nothing here
knows the library or the simulator."""
import math

import numpy as np

IN_RATES = (32000, 44100, 48000)
OUT_RATES = (8000, 16000, 22050, 24000, 32000, 44100, 48000)
PAIRS = [(i, o) for i in IN_RATES for o in OUT_RATES if i != o]
FRAME = 1152


def plan(in_rate, out_rate):
    """(L, M, H): the closed forms of the issue"""
    g = math.gcd(in_rate, out_rate)
    L, M = out_rate // g, in_rate // g
    H = 16 if L >= M else -((-16 * M) // L)
    return L, M, H


def prototype(t, H, c):
    """w(t) in float64: c sinc(c t) I0(9 sqrt(1 - (t / H)^2)) / I0(9) inside |t| < H, 0 outside"""
    t = np.asarray(t, np.float64)
    inside = np.abs(t) < H
    u = np.where(inside, t / H, 0.0)
    w = c * np.sinc(c * t) * np.i0(9.0 * np.sqrt(1.0 - u * u)) / np.i0(9.0)
    return np.where(inside, w, 0.0)


def taps64(in_rate, out_rate):
    """h[p][j] = w(H - 1 - j + p / L) in float64"""
    L, M, H = plan(in_rate, out_rate)
    c = 0.90 * min(1.0, L / M)
    p = np.arange(L, dtype=np.float64)[:, None]
    j = np.arange(2 * H, dtype=np.float64)[None, :]
    return prototype((H - 1 - j) + p / L, H, c)


def outputs(in_rate, out_rate, n):
    L, M, _ = plan(in_rate, out_rate)
    return -((-n * L) // M)


def dot64(taps32, x32, L, M, H, count):
    """(y, bound) in float64 from the SAME float32 taps and inputs: y[m] = sum_j h[p][j] x[n - 2 H + 1 + j] and
    bound[m] = sum_j |h x|; x: one channel, zeros in front of it and behind it"""
    h = np.asarray(taps32, np.float64)
    x = np.concatenate([np.zeros(2 * H - 1), np.asarray(x32, np.float64), np.zeros(2 * H)])
    m = np.arange(count, dtype=np.int64)
    n, p = (m * M) // L, (m * M) % L
    idx = n[:, None] + np.arange(2 * H)[None, :]          # x[n - 2 H + 1 + j] of the stream = x[n + j] of the padded array
    idx = np.minimum(idx, len(x) - 1)
    prod = h[p] * x[idx]
    return prod.sum(axis=1), np.abs(prod).sum(axis=1)


def frames_of(left, right=None):
    """one or two channel arrays (a multiple of 1152 long) -> float32 [frames][2][1152]"""
    left = np.asarray(left, np.float32)
    right = left if right is None else np.asarray(right, np.float32)
    assert len(left) % FRAME == 0 and len(left) == len(right)
    return np.ascontiguousarray(np.stack([left.reshape(-1, FRAME), right.reshape(-1, FRAME)], axis=1))


def channel(x, ch):
    """[frames][2][1152] -> the samples of one channel"""
    return np.asarray(x)[:, ch, :].reshape(-1)


def noise(frames, seed=0, scale=1.0):
    """full-scale noise, float32 [frames][2][1152], the channels independent"""
    r = np.random.default_rng(seed)
    return (r.uniform(-1.0, 1.0, (frames, 2, FRAME)) * scale).astype(np.float32)


def signal(kind, in_rate, out_rate, frames, seed=0):
    n = frames * FRAME
    if kind == "noise":
        return noise(frames, seed)
    if kind == "dc":
        return frames_of(np.ones(n))
    if kind == "sine":                                    # 0.7 of the lower Nyquist; the right channel a quarter period behind
        f = 0.7 * 0.5 * min(in_rate, out_rate)
        t = np.arange(n) / in_rate
        return frames_of(np.sin(2 * np.pi * f * t), np.cos(2 * np.pi * f * t))
    if kind == "impulse_first":
        x = np.zeros(n)
        x[0] = 1.0
        return frames_of(x)
    if kind == "impulse_last":
        x = np.zeros(n)
        x[-1] = 1.0
        return frames_of(x)
    raise ValueError(kind)
