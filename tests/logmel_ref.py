"""The log-mel rule (jsmpeg_amd/csrc/logmel.h) restated in numpy float64 from its formulas, the independent reference of the
value test (torch.stft in float64) and its derived tolerance.  torchaudio and librosa are not needed: the HTK and Slaney mel
scales are written out from their definitions.  Nothing here reads the library or the simulator."""
import numpy as np

LOG_SCALE = {"log": np.log(2.0), "log10": np.log10(2.0), "db": 10.0 * np.log10(2.0)}       # times log2


def window(n_fft):
    """the periodic Hann window"""
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(n_fft) / n_fft)


def basis(n_fft, w=None):
    """float64 [n_fft][2 bins]: column 2 b = w cos(2 pi k b / n_fft), 2 b + 1 = -w sin(..); the angle from (k b) mod n_fft, a
    multiple of a quarter turn exact"""
    w = window(n_fft) if w is None else np.asarray(w, np.float64)
    k, b = np.arange(n_fft)[:, None], np.arange(n_fft // 2 + 1)[None, :]
    j = (k * b) % n_fft
    a = 2.0 * np.pi * j / n_fft
    c, s = np.cos(a), np.sin(a)
    quarter = (4 * j) % n_fft == 0
    q = (4 * j) // n_fft
    c = np.where(quarter, np.array([1.0, 0.0, -1.0, 0.0])[q % 4], c)
    s = np.where(quarter, np.array([0.0, 1.0, 0.0, -1.0])[q % 4], s)
    out = np.zeros((n_fft, 2 * (n_fft // 2 + 1)))
    out[:, 0::2] = w[:, None] * c
    out[:, 1::2] = -(w[:, None] * s)
    return out


def hz_to_mel(f, mel_scale):
    f = np.asarray(f, np.float64)
    if mel_scale == "htk":
        return 2595.0 * np.log10(1.0 + f / 700.0)
    return np.where(f < 1000.0, 3.0 * f / 200.0, 15.0 + 27.0 * np.log(np.maximum(f, 1e-300) / 1000.0) / np.log(6.4))


def mel_to_hz(m, mel_scale):
    m = np.asarray(m, np.float64)
    if mel_scale == "htk":
        return 700.0 * (10.0 ** (m / 2595.0) - 1.0)
    return np.where(m < 15.0, 200.0 * m / 3.0, 1000.0 * np.exp(np.log(6.4) * (m - 15.0) / 27.0))


def filters(sample_rate, n_fft, n_mels, f_min=0.0, f_max=0.0, mel_scale="htk", mel_norm="none"):
    """float64 [n_mels][bins]: triangles on n_mels + 2 points evenly spaced on the mel scale"""
    bins = n_fft // 2 + 1
    f_max = f_max or sample_rate / 2.0
    freqs = (sample_rate / 2.0) * np.arange(bins) / (bins - 1)
    pts = mel_to_hz(np.linspace(hz_to_mel(f_min, mel_scale), hz_to_mel(f_max, mel_scale), n_mels + 2), mel_scale)
    up = (freqs[None, :] - pts[:-2, None]) / (pts[1:-1] - pts[:-2])[:, None]
    down = (pts[2:, None] - freqs[None, :]) / (pts[2:] - pts[1:-1])[:, None]
    fb = np.maximum(0.0, np.minimum(up, down))
    if mel_norm == "slaney":
        fb = fb * (2.0 / (pts[2:] - pts[:-2]))[:, None]
    return fb


def frames(n, end, n_fft, hop):
    h = n_fft // 2
    if n <= h:
        return 0
    return (n if end else n - h) // hop + 1


def mel_float64(x, n_fft, hop, fb64, w=None):
    """torch.stft in float64 on the CPU (center, reflect) -> (mel power [frames][n_mels], re, im [frames][bins])"""
    import torch
    w = window(n_fft) if w is None else np.asarray(w, np.float64)
    z = torch.stft(torch.from_numpy(np.asarray(x, np.float64)), n_fft, hop_length=hop, window=torch.from_numpy(w), center=True, pad_mode="reflect",
                   return_complex=True).numpy().T
    p = z.real ** 2 + z.imag ** 2
    return p @ fb64.T, z.real, z.imag


def framed_abs_sum(x, n_fft, hop, w=None):
    """sum_k |w_k x_k| of every END frame, float64"""
    w = window(n_fft) if w is None else np.asarray(w, np.float64)
    x = np.asarray(x, np.float64)
    h = n_fft // 2
    padded = np.concatenate([x[1:h + 1][::-1], x, x[-h - 1:-1][::-1]])
    t = frames(len(x), True, n_fft, hop)
    return np.array([np.sum(np.abs(w * padded[i * hop:i * hop + n_fft])) for i in range(t)])


def mel_bound(x, n_fft, hop, fb64, ranges, re, im, w=None):
    """the derived bound of |mel(float32 rule) - mel(float64)| per [frame][m]:
    |d re|, |d im| <= E = 1.01 (n_fft + 8) 2^-24 sum_k |w_k x_k| (the running error of an n_fft-term fused chain plus the
    table's rounding); p = re^2 + im^2 moves by at most 2 (|re| + |im|) E + 2 E^2 plus its own two roundings, 2^-23 p; the mel
    sum adds (hi - lo + 4) 2^-24 relative on sum fb p"""
    u = 2.0 ** -24
    e = 1.01 * (n_fft + 8) * u * framed_abs_sum(x, n_fft, hop, w)[:, None]
    p = re ** 2 + im ** 2
    dp = 2.0 * (np.abs(re) + np.abs(im)) * e + 2.0 * e * e + 2.0 * u * p
    width = (ranges[:, 1] - ranges[:, 0] + 4)[None, :]
    return dp @ fb64.T + width * u * ((p + dp) @ fb64.T)
