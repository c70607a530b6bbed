"""Seeded PCM and the configurations of the MP2 encoder tests (tests/test_mp2_enc_sim.py, tests/test_gpu_mp2_encode.py,
tools/mp2_enc_quality.py).  Every input is float32 [frames][2][1152], the decoder's own layout; the two channels differ."""
import numpy as np

# name -> (sample_rate_index, channels, bitrate_index): all four allocation tables, all three rates, both paddings at 44.1 kHz
CONFIGS = {
    "mono_48k_48": (1, 1, 2),          # Table 3-B.2c
    "mono_32k_32": (2, 1, 1),          # 3-B.2d
    "stereo_44k_64": (0, 2, 4),        # 3-B.2c, two channels
    "stereo_44k_128": (0, 2, 8),       # 3-B.2a
    "stereo_44k_192": (0, 2, 10),      # 3-B.2b
    "stereo_48k_384": (1, 2, 14),      # 3-B.2a
    "stereo_32k_320": (2, 2, 13),      # 3-B.2b
    "mono_44k_192": (0, 1, 10),        # 3-B.2b, one channel
}
RATES = (44100, 48000, 32000)
KINDS = ("sine", "sweep", "noise", "silence", "square", "gap", "wild")


def _time(frames, rate):
    return np.arange(frames * 1152, dtype=np.float64) / rate


def _layout(left, right):
    """two tracks of frames * 1152 samples -> [frames][2][1152] float32"""
    frames = len(left) // 1152
    out = np.empty((frames, 2, 1152), np.float32)
    out[:, 0, :] = np.asarray(left, np.float32).reshape(frames, 1152)
    out[:, 1, :] = np.asarray(right, np.float32).reshape(frames, 1152)
    return np.ascontiguousarray(out)


def pcm(kind, rate, frames=3, seed=0):
    t = _time(frames, rate)
    rng = np.random.RandomState(1000 + seed + 17 * KINDS.index(kind))
    if kind == "sine":                                  # 1 kHz at -6 dB; the right channel at 1.5 kHz
        return _layout(0.5 * np.sin(2 * np.pi * 1000.0 * t), 0.5 * np.sin(2 * np.pi * 1500.0 * t + 0.3))
    if kind == "sweep":                                 # log sweep 50 Hz .. 0.45 fs
        f0, f1, T = 50.0, 0.45 * rate, t[-1] + 1.0 / rate
        ph = 2 * np.pi * f0 * T / np.log(f1 / f0) * (np.exp(t / T * np.log(f1 / f0)) - 1.0)
        return _layout(0.7 * np.sin(ph), 0.7 * np.cos(ph))
    if kind == "noise":                                 # white noise at -20 dB
        return _layout(0.1 * rng.randn(len(t)), 0.1 * rng.randn(len(t)))
    if kind == "silence":
        return _layout(np.zeros(len(t)), np.zeros(len(t)))
    if kind == "square":                                # full scale: S passes the largest scalefactor
        sq = np.where(np.sin(2 * np.pi * 440.0 * t) >= 0, 1.0, -1.0)
        return _layout(sq, -sq)
    if kind == "gap":                                   # one frame of silence between two loud ones
        x = pcm("noise", rate, frames, seed) * 5.0
        x[1:frames - 1] = 0.0
        return x
    if kind == "wild":                                  # NaN, +-inf and |x| > 1 among ordinary samples
        a, b = 0.4 * rng.randn(len(t)), 0.4 * rng.randn(len(t))
        for v in (a, b):
            idx = rng.choice(len(t), 40, replace=False)
            v[idx[:10]] = np.nan
            v[idx[10:20]] = np.inf
            v[idx[20:30]] = -np.inf
            v[idx[30:]] = rng.choice([-7.5, 3.0, 1.0001, -1.0001], 10)
        return _layout(a, b)
    raise ValueError(kind)


def cases():
    """every (config name, kind)"""
    return [(c, k) for c in CONFIGS for k in KINDS]
