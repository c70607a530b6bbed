"""Inputs and closed forms shared by tests/test_resample_edges.py (the simulator) and tests/test_gpu_resample_edges.py (the
device): unit impulses whose outputs ARE the taps, the splits of the chain tests, the largest call the 32-bit arithmetic takes,
the tiny inputs.  Test infrastructure only: nothing here knows the library or the simulator; the rule is restated from
jsmpeg_amd/csrc/pcm_resample.h in integers."""
import numpy as np

import resample_ref as ref

FRAME = ref.FRAME
BLOCK = 256                                    # RS_WG: output slots per workgroup
PAIR_IDS = ["%d_%d" % p for p in ref.PAIRS]
LIMIT_PAIRS = [(48000, 8000), (44100, 8000), (32000, 22050)]     # the LDS span and the carry; never phase 0; the largest table
EDGE_PAIR = (32000, 44100)                     # L = 441: the largest L, and it makes more outputs than inputs
EDGE_FRAMES = 8454


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({2: np.uint16, 4: np.uint32}[a.dtype.itemsize])


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


# ------------------------------------------------------------------ impulses

def edge_positions(pair, frames, end=True):
    """input indices q = floor(256 b M / L) - H: output 256 b (the first of workgroup b of an unchained stream) reads
    n = q + H, output 256 b - 1 at least n - ceil(M / L) >= q, so outputs on BOTH sides of the workgroup's edge read the
    impulse at q (their n lies in [q, q + 2 H)).  b: the first edge, the middle one and the last one of the stream."""
    L, M, H = ref.plan(*pair)
    N = frames * FRAME
    count = ref.outputs(*pair, N + (H if end else 0))
    last = (count - 1) // BLOCK
    out = []
    for b in sorted({1, (last + 1) // 2, last}):
        q = (BLOCK * b * M) // L - H
        if b >= 1 and 0 <= q < N:
            lo, hi = ((BLOCK * b - 1) * M) // L, (BLOCK * b * M) // L
            assert q <= lo and hi < q + 2 * H                     # both neighbours of the edge read q
            out.append(q)
    return out


def impulse_streams(pair, frames):
    """-> (x, positions): x float32 [frames][2][1152] of zeros with unit impulses, positions = (left's, right's) ascending
    sample indices.  Within a channel any two impulses are more than 2 H apart (no output reads two of them), so adjacent
    positions lie in different channels.  Always there: sample 0; 1151 (left) and 1152 (right), the frame edge of the layout;
    2 * 1152 - 1; the last sample and the one 2 H before it.  Where they fit: edge_positions()."""
    L, M, H = ref.plan(*pair)
    N = frames * FRAME
    placed = ([], [])

    def fits(ch, q):
        return all(abs(q - o) > 2 * H for o in placed[ch])

    def place(q, forced=None, must=True):
        if not 0 <= q < N or q in placed[0] or q in placed[1]:
            return
        for ch in ([forced] if forced is not None else sorted((0, 1), key=lambda c: len(placed[c]))):
            if fits(ch, q):
                placed[ch].append(q)
                return
        assert not must, (pair, frames, q)

    place(FRAME - 1, 0)
    place(FRAME, 1)
    for q in (0, 2 * FRAME - 1, N - 1, N - 1 - 2 * H):
        place(q)
    for q in edge_positions(pair, frames):
        place(q, must=False)
    x = np.zeros((frames, 2, FRAME), np.float32)
    for ch in range(2):
        placed[ch].sort()
        for q in placed[ch]:
            x[q // FRAME, ch, q % FRAME] = 1.0
    assert N - 1 in placed[0] + placed[1] and (N - 1 - 2 * H in placed[0]) != (N - 1 in placed[0])
    return x, (list(placed[0]), list(placed[1]))


def impulse_want(pair, taps, positions, count, height=1.0, gain=1.0):
    """the first `count` outputs of one filter channel whose input is `height` at `positions` and 0 elsewhere.  Output m has
    n = m M div L and p = m M mod L (int64); an impulse at q is its x[n - 2 H + 1 + j] at j = q - n + 2 H - 1, so the output
    is gain * (taps[p][j] * height) where 0 <= j < 2 H and +0.0 everywhere else.  Exact for positions more than 2 H apart:
    fmaf(h, height, +0) is the float32 product, every other step adds h * 0, and +0 + -0 = +0."""
    L, M, H = ref.plan(*pair)
    taps = np.asarray(taps, np.float32)
    assert taps.shape == (L, 2 * H)
    want = np.zeros(count, np.float32)
    for q in positions:
        lo = max(0, (q * L) // M - 2)
        m = np.arange(lo, min(count, ((q + 2 * H) * L) // M + 3), dtype=np.int64)
        n, p = (m * M) // L, (m * M) % L
        j = q - n + 2 * H - 1
        ok = (j >= 0) & (j < 2 * H)
        assert not want[m[ok]].any()                              # no output reads two impulses
        want[m[ok]] = np.float32(gain) * (taps[p[ok], j[ok]] * np.float32(height))
    return want


def one_channel(x, ch):
    """x with only channel ch kept: what a mono handle mixes to 0.5 at that channel's impulses"""
    y = np.zeros_like(x)
    y[:, ch, :] = x[:, ch, :]
    return y


# ------------------------------------------------------------------ chains

CHAIN_FRAMES = 8
SINGLES = (1,) * 8
SPLITS = [SINGLES, (2, 0, 6), (1, 7)]
ABSENT = (2, 0, 0, 0, 0, 0, 6, 0)              # absent for five calls with two frames' worth of outputs behind it
PAIRED = [(SINGLES, ABSENT), ((1, 0, 3, 0, 0, 4, 0, 0), (3, 0, 0, 0, 5, 0, 0, 0))]


def whole_frames_per_call(pair, split, end):
    """FRAMES form, one chained stream fed `split` frames per call, END on the last call: the whole frames each call hands
    out, floor(m1 / 1152) - floor(m0 / 1152), the last frame padded under END.  A call without input and without END's tail
    hands out nothing."""
    L, M, H = ref.plan(*pair)
    out, N, m0 = [], 0, 0
    for c, f in enumerate(split):
        last = end and c == len(split) - 1
        tail = H if last and (f or N) else 0
        N += f * FRAME
        m1 = -((-(N + tail) * L) // M)
        out.append((-(-m1 // FRAME) if last else m1 // FRAME) - m0 // FRAME)
        m0 = m1
    return out


def lead_before_call(pair, split, call):
    """samples of the partial frame a chained FRAMES stream holds on the device when call `call` begins"""
    return ref.outputs(*pair, sum(split[:call]) * FRAME) % FRAME


# ------------------------------------------------------------------ the 32-bit arithmetic of a call

def most_frames(pair, end=True):
    """the largest frame count of one stream whose (inputs + tail) L + M fits 32 bits"""
    L, M, H = ref.plan(*pair)
    return ((0xffffffff - M) // L - (H if end else 0)) // FRAME


# ------------------------------------------------------------------ tiny inputs

#        scale = 2^e, dtype: float32 sums that are subnormal in part (-120) and throughout (-140); subnormal halves; bfloat16
#        shares float32's exponents, so its subnormals need float32's
TINY_PAIR = (48000, 16000)
TINY = [(-120, "float32"), (-140, "float32"), (-17, "float16"), (-120, "bfloat16"), (-130, "bfloat16")]
TINY_IDS = ["2^%d_%s" % t for t in TINY]
SMALLEST_NORMAL = {"float32": 2.0 ** -126, "float16": 2.0 ** -14, "bfloat16": 2.0 ** -126}


def tiny(frames, e, seed=0):
    """noise scaled by 2^e (exactly: a power of two), float32 [frames][2][1152]"""
    return ref.noise(frames, seed=seed, scale=2.0 ** e)


def as_float64(a, dtype):
    """values of an output array: bfloat16 arrives as its bits"""
    if dtype == "bfloat16":
        return (np.asarray(a, np.uint16).astype(np.uint32) << 16).view(np.float32).astype(np.float64)
    return np.asarray(a).astype(np.float64)


def subnormals(a, dtype):
    """how many samples of `a` are nonzero and below the type's smallest normal number; how many are nonzero"""
    v = np.abs(as_float64(a, dtype))
    return int(((v > 0) & (v < SMALLEST_NORMAL[dtype])).sum()), int((v > 0).sum())
