"""jsmpeg_amd/csrc/mp2_enc.h restated in numpy integers (TEST ONLY): the second statement of the MP2 encoder's rule, written
from the header's comment, that the simulator's bytes (tests/sim/sim_mp2_enc.cpp: the kernel's own functions) must equal.
Table rules (ISO 11172-3 Tables 3-B.2a-d as mp2_tables.h states them) are restated here as well; the window's integers are
read from mp2_window.h (data), the cosines come from numpy."""
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KBPS = (32, 48, 56, 64, 80, 96, 112, 128, 160, 192, 224, 256, 320, 384)
RATES = (44100, 48000, 32000)


def window():
    """W[512]: ISO's analysis window C[i] * 2^21 (the synthesis window's committed integers and their symmetry)"""
    text = open(os.path.join(ROOT, "jsmpeg_amd", "csrc", "mp2_window.h")).read()
    body = text[text.index("MP2_WINDOW_HALF_X2[257]"):]
    half = [int(v) for v in re.findall(r"-?\d+", body[body.index("{") + 1:body.index("}")])]
    assert len(half) == 257
    w = np.zeros(512, np.int64)
    for i in range(512):
        m = i if i <= 256 else 512 - i
        w[i] = half[m] if (i <= 256 or m % 64 == 0) else -half[m]
    return w


def cosines():
    return np.rint(32768.0 * np.cos(np.arange(128) * np.pi / 64.0)).astype(np.int64)


W = window()
COS = cosines()
MATRIX = np.array([[COS[((2 * k + 1) * (i - 16)) % 128] for i in range(64)] for k in range(32)], np.int64)     # [k][i]


def refused(sr, ch, br):
    if not (0 <= sr <= 2 and 1 <= ch <= 2 and 1 <= br <= 14):
        return True
    k = KBPS[br - 1]
    return (ch == 2 and k in (32, 48, 56, 80)) or (ch == 1 and k >= 224)


def table_select(sr, ch, br):
    per = KBPS[br - 1] // ch
    if per <= 48:
        return (12 if sr == 2 else 8), 0
    if per <= 80:
        return 27, 1
    return (27 if sr == 1 else 30), 1


def nbal(high, sb):
    if high:
        return 4 if sb < 11 else (3 if sb < 23 else 2)
    return 4 if sb < 2 else 3


def steps_of(high, sb, code):
    if code == 0:
        return 0
    if not high:
        return {1: 3, 2: 5, 3: 9, 15: 65535}.get(code, (1 << code) - 1)
    if sb < 3:
        return 3 if code == 1 else (1 << (code + 1)) - 1
    if sb < 11:
        return 65535 if code == 15 else (2 * code + 1 if code < 5 else (1 << (code - 1)) - 1)
    if sb < 23:
        return 65535 if code == 7 else (2 * code + 1 if code < 5 else (1 << (code - 1)) - 1)
    return 65535 if code == 3 else 2 * code + 1


def code_bits(steps):
    return {3: 5, 5: 7, 9: 10}.get(steps, int(steps).bit_length())


def grouped(steps):
    return steps in (3, 5, 9)


def granule_bits(steps):
    return 0 if steps == 0 else (code_bits(steps) if grouped(steps) else 3 * code_bits(steps))


def gain(steps):
    return 0 if steps == 0 else int(round(24.0 * np.log2(steps + 1.0)))


def scalefactor(i):
    if i == 63:
        return 0
    shift, k = divmod(i, 3)
    base = (0x02000000, 0x01965FEA, 0x01428A30)[k]
    return (base + ((1 << shift) >> 1)) >> shift


SCALEFACTORS = np.array([scalefactor(i) for i in range(63)], np.int64)


def requantise(code, steps, sf):
    """the decoder's fixed-point requantiser, vectorised over `code`"""
    scale = {3: 16384, 5: 10922, 9: 6553}.get(steps, 65536 >> code_bits(steps))
    mid = ((steps + 1) >> 1) - 1
    val = (mid - np.asarray(code, np.int64)) * scale
    return (val * (sf >> 12) + ((val * (sf & 4095) + 2048) >> 12)) >> 12


_levels = {}


def levels(steps, index):
    key = (steps, index)
    if key not in _levels:
        _levels[key] = 256 * requantise(np.arange(steps), steps, scalefactor(index))
    return _levels[key]


def quantise(S, steps, index):
    """argmin over the codes of |256 requantise - S|, ties to the lower code; S an int64 array.  The levels fall with the code:
    the candidates are the first code at or below S and the lowest code of the level just above."""
    lv = levels(steps, index)
    neg = -lv
    S = np.asarray(S, np.int64)
    c1 = np.searchsorted(neg, -S, "left")
    above = lv[np.maximum(c1 - 1, 0)]
    c0 = np.searchsorted(neg, -above, "left")
    below = lv[np.minimum(c1, steps - 1)]
    take1 = (c1 < steps) & ((S - below) < (above - S))
    out = np.where(take1, c1, c0)
    return np.where(c1 == 0, 0, out)


def frame_offset(sr, br, n):
    N, fs = 144000 * KBPS[br - 1], RATES[sr]
    return n * (N // fs) + n * (N % fs) // fs


def frame_bytes(sr, br, n):
    return frame_offset(sr, br, n + 1) - frame_offset(sr, br, n)


def default_pts(n, rate):
    return n * 1152 * 90000 // rate


def pcm_s16(x):
    x = np.asarray(x, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        v = x * np.float32(32767.0)
        s = np.where(np.isnan(v), np.float32(0), np.clip(np.rint(v), -32767.0, 32767.0))
    return s.astype(np.int64)


def window_sums(samples):
    """samples: int64 [480 + 1152] of one channel -> Y [36][64]"""
    idx = 480 + 32 * np.arange(36)[:, None] + 31 - np.arange(512)[None, :]
    return (W[None, :] * samples[idx]).reshape(36, 8, 64).sum(axis=1)


def fold(Y):
    """Y [36][64] -> the kernel's folded Z [36][32]: Z[0] = Y[16], Z[t] = Y[16 + t] + Y[16 - t] (t <= 16), Y[16 + t] - Y[80 - t] above"""
    t = np.arange(32)
    other = np.where(t <= 16, Y[:, 16 - np.minimum(t, 16)], -Y[:, np.minimum(80 - t, 63)])
    other[:, 0] = 0
    return Y[:, 16 + t] + other


def analysis(samples):
    """samples: int64 [480 + 1152] of one channel -> S [36][32]"""
    acc = window_sums(samples) @ MATRIX.T                      # [36][32]
    return (acc + (1 << 27)) >> 28


def scale_index(M):
    """largest i in 0..62 with scalefactor(i) >= 2 M, 0 if none"""
    ok = np.nonzero(SCALEFACTORS >= 2 * int(M))[0]
    return int(ok[-1]) if len(ok) else 0


def dearest_raise(sblimit, high):
    """the most bits one raise can cost in the table: over its subbands and codes, the first raise with three scalefactors"""
    return max(12 * (granule_bits(steps_of(high, sb, code + 1)) - granule_bits(steps_of(high, sb, code))) + (20 if code == 0 else 0)
               for sb in range(sblimit) for code in range((1 << nbal(high, sb)) - 1))


class Bits:
    def __init__(self):
        self.v, self.n = 0, 0

    def put(self, value, n):
        assert 0 <= value < (1 << n)
        self.v = (self.v << n) | int(value)
        self.n += n

    def bytes(self, total):
        assert self.n <= 8 * total
        return (self.v << (8 * total - self.n)).to_bytes(total, "big")


def encode_frame(cfg, samples, n, info=None):
    """cfg = (sample_rate_index, channels, bitrate_index); samples int64 [2][480 + 1152] (history first); n the ordinal.
    -> the frame's bytes.  info (a dict) receives S, codes, indices, silent, nsf, scfsi, left, used, and what the tests assert
    about their inputs: the pair that won each round (winners), the rounds several pairs tied in (ties), nsf of the first
    raises (first_nsf), how the loop ended (end: "top" / "fit") and the samples clamped at either end of a quantiser."""
    sr, ch_n, br = cfg
    sblimit, high = table_select(sr, ch_n, br)
    size = frame_bytes(sr, br, n)
    S = np.stack([analysis(samples[c]) for c in range(ch_n)])             # [ch][36][32]
    pairs = [(sb, c) for sb in range(sblimit) for c in range(ch_n)]       # bitstream order
    idx, silent = {}, {}
    for sb, c in pairs:
        M = [int(np.abs(S[c, 12 * p:12 * p + 12, sb]).max()) for p in range(3)]
        idx[sb, c] = [scale_index(m) for m in M]
        silent[sb, c] = not any(M)
    sel, nsf = {}, {}
    for p in pairs:
        a, b, c3 = idx[p]
        sel[p] = 2 if a == b == c3 else (1 if a == b else (3 if b == c3 else 0))
        nsf[p] = {0: 3, 1: 2, 2: 1, 3: 2}[sel[p]]
    code = {p: 0 for p in pairs}
    left = 8 * size - 32 - sum(nbal(high, sb) for sb, _ in pairs)
    rounds = 0
    winners, ties, first_nsf = [], [], set()
    while True:
        best, best_key = None, None
        open_keys = []
        for p in pairs:
            sb, c = p
            if silent[p] or code[p] >= (1 << nbal(high, sb)) - 1:
                continue
            so, sn = steps_of(high, sb, code[p]), steps_of(high, sb, code[p] + 1)
            cost = 12 * (granule_bits(sn) - granule_bits(so)) + (2 + 6 * nsf[p] if code[p] == 0 else 0)
            if cost > left:
                continue
            key = (-8 * min(idx[p]) - gain(so), -sb, -c)
            open_keys.append((key[0], p))
            if best is None or key > best_key:
                best, best_key, best_cost = p, key, cost
        if best is None:
            break
        if info is not None:
            winners.append(best)
            tied = [p for noise, p in open_keys if noise == best_key[0]]
            if len(tied) > 1:                                  # the order (lower subband, then channel 0) decided this round
                ties.append(tied)
            if code[best] == 0:
                first_nsf.add(nsf[best])
        code[best] += 1
        left -= best_cost
        rounds += 1
    w = Bits()
    w.put(0xfffd, 16)
    w.put(br, 4); w.put(sr, 2); w.put(size - 144000 * KBPS[br - 1] // RATES[sr], 1); w.put(0, 1)
    w.put(3 if ch_n == 1 else 0, 2); w.put(0, 6)
    for p in pairs:
        w.put(code[p], nbal(high, p[0]))
    for p in pairs:
        if code[p]:
            w.put(sel[p], 2)
    for p in pairs:
        if code[p]:
            a, b, c3 = idx[p]
            for v in {0: (a, b, c3), 1: (a, c3), 2: (a,), 3: (a, b)}[sel[p]]:
                w.put(v, 6)
    coded = {}
    for p in pairs:
        if code[p]:
            sb, c = p
            st = steps_of(high, sb, code[p])
            coded[p] = (st, np.concatenate([quantise(S[c, 12 * part:12 * part + 12, sb], st, idx[p][part]) for part in range(3)]))
    for g in range(12):
        for p in pairs:
            if p in coded:
                st, q = coded[p]
                c0, c1, c2 = (int(v) for v in q[3 * g:3 * g + 3])
                if grouped(st):
                    w.put(c0 + st * (c1 + st * c2), code_bits(st))
                else:
                    for v in (c0, c1, c2):
                        w.put(v, code_bits(st))
    if info is not None:
        info.update(S=S, code=code, idx=idx, silent=silent, nsf=nsf, left=left, used=w.n, rounds=rounds, pairs=pairs, high=high,
                    codes={p: coded[p][1] for p in coded}, sel=sel, sblimit=sblimit, winners=winners, ties=ties, first_nsf=first_nsf)
        # how the loop ended: every loud pair at its top code with more bits left than the table's dearest raise, or a raise that does not fit
        loud = [p for p in pairs if not silent[p]]
        at_top = all(code[p] == (1 << nbal(high, p[0])) - 1 for p in loud)
        info["end"] = "top" if loud and at_top and left > dearest_raise(sblimit, high) else ("fit" if loud and not at_top else None)
        low = high_end = 0
        for (sb, c), (st, _) in coded.items():
            for part in range(3):
                c1 = np.searchsorted(-levels(st, idx[sb, c][part]), -S[c, 12 * part:12 * part + 12, sb], "left")
                low += int((c1 == 0).sum())
                high_end += int((c1 == st).sum())
        info["clamped"] = (low, high_end)                      # samples at or above the top level, samples below the lowest one
    assert left == 8 * size - w.n
    return w.bytes(size)


def encode(cfg, pcm, n0=0, history=None, infos=None):
    """pcm float32 [frames][2][1152] -> (the stream piece's bytes, the history for a chained continuation)"""
    sr, ch_n, br = cfg
    s16 = pcm_s16(pcm)                                                     # [frames][2][1152]
    hist = np.zeros((2, 480), np.int64) if history is None else history
    out = []
    for f in range(len(pcm)):
        samples = np.concatenate([hist, s16[f]], axis=1)
        info = {} if infos is not None else None
        out.append(encode_frame(cfg, samples, n0 + f, info))
        if infos is not None:
            infos.append(info)
        hist = samples[:, 1152:]
    return b"".join(out), hist
