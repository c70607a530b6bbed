"""TEST INFRASTRUCTURE ONLY -- an independent restatement of the intra encoder (jsmpeg_amd/csrc/enc_block.h) in numpy, in the
manner of tests/tensor_ref.py: the header's integer transform, quantiser and colour conversion written out from the formulas
the header states, the bits written with tests/enc/mpeg1_enc.py's Bits / put_coeffs (which read the Annex-B strings through
spec_tables, not through the encoder's table).  Nothing here includes or calls the code under test."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "enc"))
import mpeg1_enc  # noqa: E402
from mpeg1_enc import INV, ZZ, Bits, put_coeffs  # noqa: E402

W = np.array(mpeg1_enc.T["DEFAULT_INTRA_QUANT"], dtype=np.int64).reshape(8, 8)
_k, _n = np.mgrid[0:8, 0:8]
COS = np.rint(16384.0 * np.where(_k == 0, np.sqrt(1.0 / 8.0), 0.5) * np.cos((2 * _n + 1) * _k * np.pi / 16.0)).astype(np.int64)
FPS = {1: 24, 2: 24, 3: 25, 4: 30, 5: 30, 6: 50, 7: 60, 8: 60}


def coded(width, height):
    return (width + 15) & ~15, (height + 15) & ~15


def planes(frame, cw, ch):
    """Y | Cr | Cb bytes -> three 2-D arrays"""
    frame = np.asarray(frame, dtype=np.uint8)
    n = cw * ch
    return frame[:n].reshape(ch, cw), frame[n:n + n // 4].reshape(ch // 2, cw // 2), frame[n + n // 4:n + n // 2].reshape(ch // 2, cw // 2)


def blocks(plane):
    """[H, W] -> [H / 8, W / 8, 8, 8]"""
    h, w = plane.shape
    return plane.reshape(h // 8, 8, w // 8, 8).transpose(0, 2, 1, 3)


def c8_integer(x):
    """the header's transform: eight times the orthonormal DCT coefficient, one rounding"""
    a = COS @ x.astype(np.int64) @ COS.T
    return (a + (1 << 24)) >> 25


def c8_float(x):
    from scipy.fft import dctn
    return 8.0 * dctn(x.astype(np.float64), axes=(-2, -1), norm="ortho")


def quantise(c8, q, exact_float=False):
    """[..., 8, 8] coefficients times eight -> levels (raster), DC at [..., 0, 0]"""
    d = q * W
    if exact_float:
        mag = np.rint(np.abs(c8) / d)
        dc = np.rint(c8[..., 0, 0] / 64.0)
    else:
        mag = (2 * np.abs(c8) + d) // (2 * d)
        dc = (c8[..., 0, 0] + 32) >> 6
    lv = (np.sign(c8) * np.minimum(mag, 255)).astype(np.int64)
    lv[..., 0, 0] = np.clip(dc, 0, 255)
    return lv


def frame_levels(frame, width, height, q, exact_float=False):
    """levels[mb][block][64] in scan order ([0]: the DC level), blocks in syntax order Y0 Y1 Y2 Y3 Cb Cr"""
    cw, ch = coded(width, height)
    y, cr, cb = planes(frame, cw, ch)
    tr = c8_float if exact_float else c8_integer
    ly, lcr, lcb = (quantise(tr(blocks(p)), q, exact_float) for p in (y, cr, cb))
    mbh, mbw = ch // 16, cw // 16
    out = np.zeros((mbh, mbw, 6, 64), dtype=np.int64)
    zz = np.asarray(ZZ)
    for b in range(4):
        out[:, :, b] = ly[(b >> 1)::2, (b & 1)::2].reshape(mbh, mbw, 64)[..., zz]
    out[:, :, 4] = lcb.reshape(mbh, mbw, 64)[..., zz]
    out[:, :, 5] = lcr.reshape(mbh, mbw, 64)[..., zz]
    return out.reshape(mbh * mbw, 6, 64)


def picture_bytes(levels, width, height, q, frame_rate_code, ordinal):
    """sequence header, GOP header, picture header, one slice per macroblock row"""
    cw, ch = coded(width, height)
    mbw, mbh = cw // 16, ch // 16
    w = Bits()
    w.start_code(0xB3)
    w.put(width, 12); w.put(height, 12); w.put(1, 4); w.put(frame_rate_code, 4); w.put(0x3FFFF, 18); w.put(1, 1); w.put(20, 10)
    w.put(0, 1); w.put(0, 1); w.put(0, 1)
    w.start_code(0xB8)
    fps = FPS[frame_rate_code]
    s = ordinal // fps
    w.put(0, 1); w.put((s // 3600) % 24, 5); w.put((s // 60) % 60, 6); w.put(1, 1); w.put(s % 60, 6); w.put(ordinal % fps, 6)
    w.put(1, 1); w.put(0, 1)
    w.start_code(0x00)
    w.put(0, 10); w.put(1, 3); w.put(0xFFFF, 16); w.put(0, 1)
    for row in range(mbh):
        w.start_code(row + 1)
        w.put(q, 5); w.put(0, 1)
        pred = [128, 128, 128]
        for col in range(mbw):
            w.code(INV["MBA"][1])
            w.code(INV["MBTYPE_I"][0x01])
            for b in range(6):
                lv = levels[row * mbw + col][b]
                comp = 0 if b < 4 else b - 3
                diff = int(lv[0]) - pred[comp]
                size = 0 if diff == 0 else abs(diff).bit_length()
                w.code(INV["DCSIZE_LUMA" if b < 4 else "DCSIZE_CHROMA"][size])
                if size:
                    w.put(diff if diff > 0 else diff + (1 << size) - 1, size)
                pred[comp] = int(lv[0])
                put_coeffs(w, [int(v) for v in lv[1:]], False)
    w.align()
    return bytes(w.out)


def encode(frames, width, height, streams=None, qscale=8, frame_rate_code=5, end=True, exact_float=False):
    """The whole call: (buffer bytes with the 0xff gaps, [(offset, bytes)] per picture, {stream: (begin, end)})"""
    n = len(frames)
    streams = [0] * n if streams is None else [int(s) for s in streams]
    qs = [int(qscale)] * n if np.isscalar(qscale) else [int(v) for v in qscale]
    out = bytearray(b"\xff" * 16)
    ranges, sr = [], {}
    ordinal = 0
    for k in range(n):
        ordinal = ordinal + 1 if k and streams[k] == streams[k - 1] else 0
        if not k or streams[k] != streams[k - 1]:
            sr[streams[k]] = [len(out), None]
        pic = picture_bytes(frame_levels(frames[k], width, height, qs[k], exact_float), width, height, qs[k], frame_rate_code, ordinal)
        ranges.append((len(out), len(pic)))
        out += pic
        if k + 1 == n or streams[k + 1] != streams[k]:
            if end:
                out += b"\x00\x00\x01\xb7"
            sr[streams[k]][1] = len(out)
            # to the next 16-byte aligned begin, at least 8 bytes away; behind the call's last stream, to the next multiple of 16
            out += b"\xff" * (-len(out) % 16 if k + 1 == n else 8 + -(len(out) + 8) % 16)
    return bytes(out), ranges, {s: tuple(v) for s, v in sr.items()}


# ---------------------------------------------------------------------------------------------------- RGB in

def pad_rgb(rgb, cw, ch):
    """[H, W, 3] -> [ch, cw, 3] by edge replication"""
    h, w = rgb.shape[:2]
    return np.pad(rgb, ((0, ch - h), (0, cw - w), (0, 0)), mode="edge")


def rgb_to_frame(rgb):
    """the header's integer conversion: [H, W, 3] uint8 RGB -> Y | Cr | Cb bytes of the coded size"""
    h, w = rgb.shape[:2]
    cw, ch = coded(w, h)
    p = pad_rgb(rgb, cw, ch).astype(np.int64)
    r, g, b = p[..., 0], p[..., 1], p[..., 2]
    y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16
    rs, gs, bs = (c.reshape(ch // 2, 2, cw // 2, 2).sum(axis=(1, 3)) for c in (r, g, b))
    cr = np.clip((32768 * rs - 27439 * gs - 5329 * bs + (128 << 18) + (1 << 17)) >> 18, 0, 255)
    cb = np.clip((-11059 * rs - 21709 * gs + 32768 * bs + (128 << 18) + (1 << 17)) >> 18, 0, 255)
    return np.concatenate([y.ravel(), cr.ravel(), cb.ravel()]).astype(np.uint8)


def rgb_to_frame_float(rgb):
    """float64 JFIF (full-range BT.601) of the same, unrounded: (Y, Cr, Cb) float planes"""
    h, w = rgb.shape[:2]
    cw, ch = coded(w, h)
    p = pad_rgb(rgb, cw, ch).astype(np.float64)
    r, g, b = p[..., 0], p[..., 1], p[..., 2]
    y = 0.299 * r + 0.587 * g + 0.114 * b
    rm, gm, bm = (c.reshape(ch // 2, 2, cw // 2, 2).mean(axis=(1, 3)) for c in (r, g, b))
    cr = 128 + 0.5 * rm - 0.418688 * gm - 0.081312 * bm
    cb = 128 - 0.168736 * rm - 0.331264 * gm + 0.5 * bm
    return y, cr, cb
