"""Seeded PCM and the configurations of the MP2 encoder tests (tests/test_mp2_enc_sim.py, tests/test_gpu_mp2_encode.py,
tools/mp2_enc_quality.py).  Every input is float32 [frames][2][1152], the decoder's own layout; the two channels differ."""
import numpy as np

import mp2_enc_ref as ref

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
    if kind == "square":                                # full scale (no PCM makes 2 |S| pass the largest scalefactor: test_mp2_enc_edges.py)
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


# ------------------------------------------------------------------------------------------------------------------------
# The inputs of tests/test_mp2_enc_edges.py and tests/test_gpu_mp2_encode_edges.py: every setting the rule accepts, and PCM
# crafted to reach what the seven kinds above do not.  What each one reaches is asserted in test_mp2_enc_edges.py.

ALL_SETTINGS = [(sr, ch, br) for sr in range(3) for ch in (1, 2) for br in range(1, 15) if not ref.refused(sr, ch, br)]
assert len(ALL_SETTINGS) == 60


def setting_id(cfg):
    return "%s_%dk_%d" % ("mono" if cfg[1] == 1 else "stereo", RATES[cfg[0]] // 1000, ref.KBPS[cfg[2] - 1])


def comb(rate, frames, levels_left, levels_right, envelope=None):
    """a sine at every subband's centre (sb + 0.5) fs / 64 with the amplitude levels_*[sb]; envelope: a gain per part (384
    samples), [3 * frames] or [2][3 * frames]"""
    t = np.arange(frames * 1152, dtype=np.float64)
    tracks = []
    for ch, levels in enumerate((levels_left, levels_right)):
        x = np.zeros(len(t))
        for sb, a in enumerate(levels):
            if a:
                x += a * np.sin(2 * np.pi * (sb + 0.5) / 64.0 * t + 0.7 * sb + 0.4 * ch)
        if envelope is not None:
            e = np.asarray(envelope, np.float64)
            x *= np.repeat(e[ch] if e.ndim == 2 else e, 384)
        tracks.append(x)
    return _layout(*tracks)


FLAT = np.full(32, 1.0 / 40)
TILT = 2.0 ** (-np.arange(32) / 2.0) / 4


def dc(rate, frames, level=0.01):
    """a constant, of opposite signs in the two channels: behind the first frame only the lowest subbands are loud, their pairs
    climb to the top code and the loop ends with bits left"""
    x = np.full(frames * 1152, level)
    return _layout(x, -x)


BOUNDS_K = (0, 7, 15, 16, 31)
BOUNDS_FRAMES = 4


def bounds_windows():
    """[(name, global sub-block g, signs [512])]: the newest 512 samples X[n] (n = 0 newest) of sub-block g -- the sample at
    32 g + 31 - n -- get the sign pattern, at full scale.  The sub-blocks lie 16 apart, so the windows are disjoint:
    'y'    sign(W[n]): every Y[i] at its largest at once, and the folded Z[t] for t <= 16;
    'z'    the same with the taps of i = 49..63 flipped: Z[t] = Y[16 + t] - Y[80 - t] at its largest for t >= 17;
    's<k>' sign(W[n] COS[(2 k + 1)(n mod 64 - 16)]): S[k] at the largest value any PCM can give."""
    sw = np.where(ref.W < 0, -1.0, 1.0)
    i = np.arange(512) % 64
    out = [("y", sw), ("z", np.where(i >= 49, -sw, sw))]
    for k in BOUNDS_K:
        out.append(("s%d" % k, np.where(ref.W * ref.MATRIX[k][i] < 0, -1.0, 1.0)))
    return [(name, 15 + 16 * j, s) for j, (name, s) in enumerate(out)]


def bounds():
    """full-scale samples whose signs drive the analysis to the bounds tools/mp2_enc_bounds.py derives (bounds_windows), silence
    between them; the right channel is the left negated"""
    x = np.zeros(BOUNDS_FRAMES * 1152)
    for _, g, signs in bounds_windows():
        x[32 * g + 31 - np.arange(512)] = signs
    return _layout(x, -x)


def _f32(v):
    return np.float32(v)


def exact_product(target):
    """a binary32 x with x * 32767.0f == target exactly in binary32 (searched among the neighbours of target / 32767)"""
    x = _f32(target / 32767.0)
    for _ in range(64):
        x = np.nextafter(x, _f32(-np.inf))
    for _ in range(129):
        if _f32(x * _f32(32767.0)) == _f32(target):
            return x
        x = np.nextafter(x, _f32(np.inf))
    raise ValueError(target)


def conversion_values():
    """{name: binary32 value} of the input conversion's edges"""
    tiny, fmax, up, down = np.finfo(np.float32).tiny, np.finfo(np.float32).max, _f32(np.inf), _f32(-np.inf)
    half = exact_product(0.5)
    v = {"tie_even_pos": exact_product(1000.5), "tie_odd_pos": exact_product(1001.5), "tie_even_neg": exact_product(-1000.5),
         "tie_odd_neg": exact_product(-1001.5), "tie_small_even": exact_product(2.5), "tie_small_odd": exact_product(1.5),
         "tie_top_pos": exact_product(32766.5), "tie_top_neg": exact_product(-32766.5),
         "below_one": np.nextafter(_f32(1.0), down), "one": _f32(1.0), "above_one": np.nextafter(_f32(1.0), up),
         "below_minus_one": np.nextafter(_f32(-1.0), down), "minus_one": _f32(-1.0), "above_minus_one": np.nextafter(_f32(-1.0), up),
         "subnormal_min": _f32(1e-45), "subnormal_max": np.nextafter(tiny, _f32(0)), "subnormal_neg": _f32(-1e-45), "normal_min": tiny,
         "normal_min_neg": -tiny, "zero": _f32(0.0), "minus_zero": _f32(-0.0), "flt_max": fmax, "minus_flt_max": -fmax,
         "inf": up, "minus_inf": down, "nan": _f32(np.nan),
         "half_below": np.nextafter(half, down), "half": half, "half_above": np.nextafter(half, up),
         "half_neg_below": np.nextafter(-half, down), "half_neg": -half, "half_neg_above": np.nextafter(-half, up)}
    return v


def conversion(rate, frames=2):
    """the conversion's edge values, each at several places of both channels, among ordinary samples (a sine and low noise)"""
    rng = np.random.RandomState(4242)
    t = _time(frames, rate)
    x = _layout(0.3 * np.sin(2 * np.pi * 700.0 * t) + 0.01 * rng.randn(len(t)), 0.2 * np.sin(2 * np.pi * 2100.0 * t) + 0.01 * rng.randn(len(t)))
    vals = list(conversion_values().values())
    flat = x.reshape(frames, 2, 1152)
    for ch in range(2):
        where = rng.choice(frames * 1152, 6 * len(vals), replace=False)
        for j, at in enumerate(where):
            flat[at // 1152, ch, at % 1152] = vals[j % len(vals)]
    return flat


def edge_inputs(rate):
    """name -> PCM: the streams of one call per setting (2 .. 4 frames each)"""
    steps = [1.0, 1.0, 0.25, 0.25, 0.25, 1.0]                                  # scalefactor triples a = b != c, then a != b = c
    solo = np.zeros(32)
    solo[17], solo[6] = 0.5, 0.4
    quiet = np.zeros(32)
    quiet[:2] = 1e-3
    return {
        "flat": comb(rate, 2, FLAT, 0.9 * FLAT),
        "tilt": comb(rate, 2, TILT, TILT[::-1].copy()),
        "tilt_swapped": comb(rate, 2, TILT[::-1].copy(), TILT),
        "steps": comb(rate, 2, FLAT, 0.9 * FLAT, steps),
        "solo": comb(rate, 2, solo + quiet, np.roll(solo, 3) + quiet),
        "dc": dc(rate, 3),
        "bounds": bounds(),
        "conversion": conversion(rate),
    }


# The padding period and the store: at 44.1 kHz the padding pattern repeats after 49 frames.  One setting with an odd b (417
# bytes at 128 kbit/s) and one with an even b (626 at 192 kbit/s); a stream of 50 frames and short streams whose ends leave
# every tail 0..15 up to the next multiple of 16; the same streams cut into chained calls of 1, 7, 41 and 1 frames.
PERIOD_SETTINGS = ((0, 2, 8), (0, 2, 10))
PERIOD_FRAMES = 50
CHAIN_PIECES = (1, 7, 41, 1)


def tail_of(cfg, frames):
    return -ref.frame_offset(cfg[0], cfg[2], frames) % 16


def period_counts(cfg):
    """frame counts per stream: 50, then the shortest streams that add a tail length not seen yet, until all 16 are there"""
    counts, seen = [PERIOD_FRAMES], {tail_of(cfg, PERIOD_FRAMES)}
    for n in range(1, 49):
        if len(seen) == 16:
            break
        if tail_of(cfg, n) not in seen:
            counts.append(n)
            seen.add(tail_of(cfg, n))
    return counts


def period_streams(cfg):
    return [pcm("noise" if i % 2 == 0 else "sweep", RATES[cfg[0]], n, seed=100 + i) for i, n in enumerate(period_counts(cfg))]


def chain_calls(counts):
    """[call][stream] frame counts: every stream cut at 1, 8, 49 and 50 frames"""
    calls, done = [], [0] * len(counts)
    for piece in CHAIN_PIECES:
        call = [min(piece, n - d) for n, d in zip(counts, done)]
        done = [d + c for d, c in zip(done, call)]
        calls.append(call)
    assert done == list(counts)
    return calls


EDGE_KINDS = ("flat", "tilt", "tilt_swapped", "steps", "solo", "dc", "bounds", "conversion")
