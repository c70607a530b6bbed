"""TEST INFRASTRUCTURE ONLY -- what the tests and tools of the encoder's GOP pass (I + P pictures) share, beside
tests/enc_inputs.py: the CPU simulator of its kernels (sim_encode_p of tests/sim/sim_encode_pass.cpp, built on demand), the
inputs of the issue's list, and the oracle as judge of a stream."""
import ctypes

import numpy as np

import enc_inputs as ei
import enc_ref

ROOT = ei.ROOT
SCALES = (1, 8, 31)
GOPS = ((3, 0), (3, 7), (5, 15))       # (gop, search range)
KINDS = ("intra", "coded", "not_coded", "skipped")
_sim = None


def sim():
    global _sim
    if _sim is None:
        lib = ei.pass_sim()
        vp, u32, u64 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64
        lib.sim_encode_p.restype = ctypes.c_int64
        lib.sim_encode_p.argtypes = [vp, u32, u32, u32, vp, vp, u32, u32, u32, u32, u32, vp, u64, vp, vp, vp, vp, vp, vp, vp]
        lib.sim_encp_recip_div.restype = None
        lib.sim_encp_recip_div.argtypes = [vp, u32, u32, vp]
        _sim = lib
    return _sim


def sim_recip_div(n, q):
    """the non-intra quantiser's stand-in for n // q on an array of n"""
    n = np.ascontiguousarray(n, dtype=np.uint32)
    out = np.zeros_like(n)
    sim().sim_encp_recip_div(n.ctypes.data, n.size, q, out.ctypes.data)
    return out


def _s8(v):
    return ((v & 255) ^ 128) - 128


class Result:
    """what a call leaves: buffer bytes, [(offset, bytes)] per picture, {stream: (begin, end)}, the reconstructed frames
    (Y | Cr | Cb bytes each), per picture the macroblocks' vectors [(mvh, mvv) half-pels, None for an intra one] and the
    counts by kind (intra, coded, not coded, skipped)"""

    def __init__(self, buf, ranges, streams, recon, vectors, stats, table=None):
        self.buf, self.ranges, self.streams, self.recon, self.vectors, self.stats = buf, ranges, streams, recon, vectors, stats
        self.table = table              # [(begin, end)] of every stream number below max_streams, absent ones included

    def triple(self):
        return self.buf, self.ranges, self.streams

    def stream(self, s=0):
        b, e = self.streams[s]
        return np.frombuffer(self.buf[b:e], dtype=np.uint8)


def sim_encode_p(frames, width, height, gop, search, streams=None, qscale=8, frame_rate_code=5, end=True, max_streams=None, cap=None):
    """the simulator's call with a GOP: a Result, or None on overflow"""
    n = len(frames)
    fr = np.ascontiguousarray(np.stack(frames), dtype=np.uint8)
    q = np.ascontiguousarray([qscale] * n if np.isscalar(qscale) else qscale, dtype=np.uint8)
    s = None if streams is None else np.ascontiguousarray(streams, dtype=np.uint32)
    ms = max_streams or (int(max(streams)) + 1 if streams is not None else 1)
    fb = fr.shape[1]
    cap = cap if cap is not None else 64 + n * (fb * 4 + 4096)
    out = np.zeros(cap + 256 + 16, dtype=np.uint8)
    po, pb = np.zeros(n, np.uint64), np.zeros(n, np.uint32)
    sb, se = np.zeros(ms, np.uint64), np.zeros(ms, np.uint64)
    cw, ch = enc_ref.coded(width, height)
    mbs = (cw // 16) * (ch // 16)
    recon = np.zeros(n * fb + 16, dtype=np.uint8)
    info, stats = np.zeros(n * mbs, np.uint32), np.zeros(n * 4, np.uint32)
    total = sim().sim_encode_p(fr.ctypes.data, width, height, n, None if s is None else s.ctypes.data, q.ctypes.data, frame_rate_code,
                               1 if end else 0, ms, gop, search, out.ctypes.data, cap, po.ctypes.data, pb.ctypes.data, sb.ctypes.data,
                               se.ctypes.data, recon.ctypes.data, info.ctypes.data, stats.ctypes.data)
    if total < 0:
        return None
    assert np.all(out[total:total + 256] == 0xff)
    present = sorted(set([0] * n if streams is None else [int(v) for v in streams]))
    vectors = [[None if (v & 3) == 0 else (_s8(v >> 16), _s8(v >> 24)) for v in info[k * mbs:(k + 1) * mbs].tolist()]
               for k in range(n)]
    return Result(out[:total].tobytes(), [(int(po[k]), int(pb[k])) for k in range(n)], {i: (int(sb[i]), int(se[i])) for i in present},
                  [recon[k * fb:(k + 1) * fb].copy() for k in range(n)], vectors, [tuple(int(v) for v in stats[4 * k:4 * k + 4]) for k in range(n)],
                  [(int(sb[i]), int(se[i])) for i in range(ms)])


# ---------------------------------------------------------------------------------------------------- inputs

def smooth_picture(height, width, seed=5):
    """a smooth textured picture with room around it: [height + 64, width + 64] float"""
    yy, xx = np.mgrid[0:height + 64, 0:width + 64].astype(np.float64)
    return 120 + 60 * np.sin(xx / 9.0 + seed) * np.cos(yy / 11.0) + 35 * np.sin((xx - 2 * yy) / 13.0)


def pan_frames(width, height, n, step, half=False):
    """one smooth picture shifted by `step` = (dx, dy) whole pels per picture; half: by half a pel more in both directions,
    built by averaging the shifts with the decoder's rounding (a + b + c + d + 2) >> 2 -- picture t shows the source at
    t * (step + 1/2)"""
    cw, ch = enc_ref.coded(width, height)
    src = np.clip(np.rint(smooth_picture(ch, cw)), 0, 255).astype(np.int64)
    out = []
    for t in range(n):
        hx, hy = (2 * step[0] + (1 if half else 0)) * t, (2 * step[1] + (1 if half else 0)) * t     # half-pels
        x0, y0 = 32 + (hx >> 1), 32 + (hy >> 1)
        a = src[y0:y0 + ch, x0:x0 + cw]
        if hx & 1 and hy & 1:
            a = (a + src[y0:y0 + ch, x0 + 1:x0 + cw + 1] + src[y0 + 1:y0 + ch + 1, x0:x0 + cw] + src[y0 + 1:y0 + ch + 1, x0 + 1:x0 + cw + 1] + 2) >> 2
        elif hx & 1:
            a = (a + src[y0:y0 + ch, x0 + 1:x0 + cw + 1] + 1) >> 1
        elif hy & 1:
            a = (a + src[y0 + 1:y0 + ch + 1, x0:x0 + cw] + 1) >> 1
        c = np.full((ch // 2, cw // 2), 128, np.uint8)
        out.append(ei.frame_of(a, c, c))
    return out


def p_cases(libs):
    """name -> (frames, width, height): the issue's list"""
    out = {}
    out["content_176x144"] = (ei.content_frames(176, 144, 5), 176, 144)
    out["content_177x145"] = (ei.content_frames(177, 145, 3), 177, 145)
    out["enc_pan_176x144"] = ei.golden_frames(libs, "enc_pan_176x144", 13)
    out["whole_pel_pan"] = (pan_frames(64, 48, 3, (3, -2)), 64, 48)
    out["half_pel_pan"] = (pan_frames(64, 48, 3, (1, 0), half=True), 64, 48)
    out["flat_grey"] = ([ei.flat_frame(48, 32, 128)] * 3, 48, 32)
    out["flat_wide"] = ([ei.flat_frame(768, 16, 128)] * 2, 768, 16)
    y, cr, cb = enc_ref.planes(out["content_176x144"][0][0], 176, 144)
    one = ei.frame_of(y[48:64, 64:80], cr[24:32, 32:40], cb[24:32, 32:40])
    out["one_macroblock"] = ([one, one, ei.noise_frame(16, 16)], 16, 16)
    out["scene_cut"] = ([ei.frame_of(y[32:80, 48:112], cr[16:40, 24:56], cb[16:40, 24:56]), ei.stripe_frame(64, 48)], 64, 48)
    # uniform noise twice (intra macroblocks, escapes), then two-valued noise and the same 65 brighter: predicted with a zero
    # vector (its activity exceeds the SAD of 65 * 256), and the residual's DC coefficient, 8 * 65, is level 260 at q = 1: clipped
    two = (np.random.default_rng(7).integers(0, 2, 64 * 48 * 3 // 2, dtype=np.uint8) * 190).astype(np.uint8)
    out["noise"] = ([ei.noise_frame(64, 48, 1), ei.noise_frame(64, 48, 2), two, two + 65], 64, 48)
    return out


RADII = tuple(range(16))               # every search range the header accepts


def checker_picture(width, height, low=20, high=220):
    """a checkerboard of 2 x 2 cells: a shift by 2 pels in either direction is its inverse, a shift by 4 the picture itself --
    the candidates of a search tie by the dozen"""
    cw, ch = enc_ref.coded(width, height)
    yy, xx = np.mgrid[0:ch, 0:cw]
    return np.where(((yy >> 1) + (xx >> 1)) & 1, high, low).astype(np.uint8)


def threshold_frames():
    """64 x 16: flat 128, then four macroblocks of 130s whose first k pixels are 131, k = 127, 128, 129, 130.  Against the flat
    picture every candidate's SAD is 512 + k; the mean rounds to 130 for k = 127 (activity 127) and to 131 from k = 128 on
    (activity 256 - k): activity + 512 < SAD reads 639 < 639, 640 < 640 (the equality), 639 < 641, 638 < 642"""
    y = np.full((16, 64), 130, np.uint8)
    for col, k in enumerate((127, 128, 129, 130)):
        mb = np.full(256, 130, np.uint8)
        mb[:k] = 131
        y[:, col * 16:col * 16 + 16] = mb.reshape(16, 16)
    c = np.full((8, 32), 128, np.uint8)
    return [ei.flat_frame(64, 16, 128), ei.frame_of(y, c, c)]


def range_cases(libs, base=None):
    """name -> (frames, width, height): what every search range 0 .. 15 runs over -- five of p_cases (`base`, when the caller
    has them), a pan of (9.5, -5.5) pels per picture that every range below 10 cuts short, the checkerboard, its shift by
    2 pels and the checkerboard again, and the pair on the intra threshold"""
    base = base if base is not None else p_cases(libs)
    out = {name: base[name] for name in ("noise", "whole_pel_pan", "half_pel_pan", "content_177x145", "one_macroblock")}
    out["fast_pan"] = (pan_frames(64, 48, 3, (9, -6), half=True), 64, 48)
    y = checker_picture(64, 48)
    c = np.full((24, 32), 128, np.uint8)
    out["checker_ties"] = ([ei.frame_of(y, c, c), ei.frame_of(np.roll(y, 2, axis=1), c, c), ei.frame_of(y, c, c)], 64, 48)
    out["intra_threshold"] = (threshold_frames(), 64, 16)
    return out


LONG_STREAMS = [0] * 255 + [1] * 2 + [3] * 1 + [4] * 300 + [7] * 542
LONG_MAX_STREAMS = 9
LONG_GOPS = ((1024, 3), (300, 15), (7, 1))      # (gop, search range)


def long_call():
    """(frames, width, height, streams, scales): 1100 pictures of 48 x 32 (3 x 2 macroblocks: two slices, room for a skipped
    macroblock) in five streams whose numbers have gaps and whose boundaries -- pictures 255, 257, 258 and 558 -- lie on both
    sides of the 256-picture steps of the placement; a slow drift over one smooth picture with a rest now and then, noise at
    every 97th picture (intra macroblocks inside P pictures), a quantiser scale per picture"""
    w, h, n = 48, 32, len(LONG_STREAMS)
    src = np.clip(np.rint(smooth_picture(h, w)), 0, 255).astype(np.uint8)
    csrc = np.clip(np.rint(smooth_picture(h // 2, w // 2, seed=2)), 0, 255).astype(np.uint8)
    frames = []
    for t in range(n):
        if t % 97 == 96:
            frames.append(ei.noise_frame(w, h, 1000 + t))
            continue
        u = t - t % 5 if (t // 40) % 3 == 2 else t                  # a rest: the same picture five times
        x0, y0 = 32 + int(np.rint(14 * np.sin(u / 9.0))), 32 + int(np.rint(11 * np.cos(u / 13.0)))
        cx, cy = 32 + (x0 - 32) // 2, 32 + (y0 - 32) // 2
        frames.append(ei.frame_of(src[y0:y0 + h, x0:x0 + w], csrc[cy:cy + h // 2, cx:cx + w // 2], 255 - csrc[cy:cy + h // 2, cx:cx + w // 2]))
    return frames, w, h, list(LONG_STREAMS), [1 + t % 31 for t in range(n)]


# ---------------------------------------------------------------------------------------------------- the judge

def picture_types(es):
    """picture_coding_type of every picture start code in `es`"""
    b = np.asarray(es, dtype=np.uint8)
    at = np.flatnonzero((b[:-5] == 0) & (b[1:-4] == 0) & (b[2:-3] == 1) & (b[3:-2] == 0))
    return [int((b[i + 5] >> 3) & 7) for i in at]


def oracle_frames(libs, es):
    """the oracle's decode of a stream: [Y | Cr | Cb bytes] per picture"""
    from jsmpeg_amd import cabi
    frames, _, _ = cabi.decode_stream(libs["oracle"], np.ascontiguousarray(es, dtype=np.uint8), keep="planes")
    return [ei.frame_of(*f) for f in frames]


def expected_types(n, gop):
    return [1 if k % gop == 0 else 2 for k in range(n)]


def p_header(buf, off):
    """(temporal_reference, picture_coding_type, full_pel_forward_vector, forward_f_code) of the P picture header at `off`"""
    assert buf[off:off + 4] == b"\x00\x00\x01\x00", off
    v = int.from_bytes(buf[off + 4:off + 9], "big")         # 10 + 3 + 16 (vbv_delay) + 1 + 3 bits, 7 of padding
    return v >> 30, (v >> 27) & 7, (v >> 10) & 1, (v >> 7) & 7


def ordinals(streams):
    """each picture's number in its stream"""
    out = []
    for k, s in enumerate(streams):
        out.append(out[-1] + 1 if k and streams[k - 1] == s else 0)
    return out


def wrapped_differentials(vectors, mbw, rng):
    """how many vector components of a call (Result.vectors) differ from their predictor by less than -rng or by rng or more,
    so that the written differential is that difference +- 2 rng.  The predictor along a slice: the vector of the macroblock
    before -- zero at the slice's begin and after an intra macroblock; a skipped macroblock and one without motion
    compensation have a zero vector and leave a zero predictor, which is the same"""
    n = 0
    for pic in vectors:
        for first in range(0, len(pic), mbw):
            prev = (0, 0)
            for v in pic[first:first + mbw]:
                if v is not None:
                    n += sum(1 for a, b in zip(v, prev) if not -rng <= a - b < rng)
                prev = v if v is not None else (0, 0)
    return n
