"""TEST INFRASTRUCTURE ONLY -- an independent restatement in numpy of the encoder's GOP pass (I + P pictures; the rules of
jsmpeg_amd/csrc/enc_motion.h), beside tests/enc_ref.py: brute-force motion search by the stated order, the mode decision, the
residual through enc_ref's integer transform, the reference decoder's dequantiser and IDCT written out from oracle/mpeg1_oracle.c's
formulas, and the bits written with tests/enc/mpeg1_enc.py's Bits / put_coeffs / put_motion / mv_ok (which read the Annex-B strings
through spec_tables).  Nothing here includes or calls the code under test."""
import functools

import numpy as np

import enc_ref
import mpeg1_enc
from enc_ref import COS, FPS, W, blocks, c8_integer, coded, planes
from mpeg1_enc import INV, ZZ, Bits, mv_ok, put_coeffs, put_motion

INTRA_BIAS = 512
PREMULT = np.array(mpeg1_enc.T["PREMULTIPLIER"], dtype=np.int64).reshape(8, 8)
ZZA = np.asarray(ZZ)
STUFFING = "00000001111"


# ---------------------------------------------------------------------------------------------------- 1. search

@functools.lru_cache(maxsize=None)
def valid_full(cw, ch, R):
    """[2R+1, 2R+1, mbh, mbw] bool: full-pel vector (dy, dx) is a candidate of macroblock (row, col)"""
    mbw, mbh = cw // 16, ch // 16
    out = np.zeros((2 * R + 1, 2 * R + 1, mbh, mbw), dtype=bool)
    for dy in range(-R, R + 1):
        for dx in range(-R, R + 1):
            for row in range(mbh):
                for col in range(mbw):
                    out[dy + R, dx + R, row, col] = mv_ok(cw, ch, col, row, 2 * dx, 2 * dy)
    return out


def predict(plane, x, y, mh, mv, n):
    """the decoder's n x n prediction at (x, y) for (mh, mv) half-pels, integer roundings"""
    H, V, oh, ov = mh >> 1, mv >> 1, mh & 1, mv & 1
    p = plane.astype(np.int64)
    a = p[y + V:y + V + n, x + H:x + H + n]
    if oh and ov:
        return (a + p[y + V:y + V + n, x + H + 1:x + H + n + 1] + p[y + V + 1:y + V + n + 1, x + H:x + H + n] +
                p[y + V + 1:y + V + n + 1, x + H + 1:x + H + n + 1] + 2) >> 2
    if oh:
        return (a + p[y + V:y + V + n, x + H + 1:x + H + n + 1] + 1) >> 1
    if ov:
        return (a + p[y + V + 1:y + V + n + 1, x + H:x + H + n] + 1) >> 1
    return a


def search(cur, ref, cw, ch, R):
    """per macroblock [mbh, mbw]: best SAD and vector in half-pels"""
    mbw, mbh = cw // 16, ch // 16
    c = cur.astype(np.int64)
    pad = np.zeros((ch + 32, cw + 32), dtype=np.int64)
    pad[16:16 + ch, 16:16 + cw] = ref
    ok = valid_full(cw, ch, R)
    big = 1 << 40
    best = [np.full((mbh, mbw), big, dtype=np.int64) for _ in range(4)]          # (SAD, dx^2 + dy^2, dy, dx)
    for dy in range(-R, R + 1):
        for dx in range(-R, R + 1):
            sad = np.abs(c - pad[16 + dy:16 + dy + ch, 16 + dx:16 + dx + cw]).reshape(mbh, 16, mbw, 16).sum(axis=(1, 3))
            cand = (sad, np.full_like(sad, dx * dx + dy * dy), np.full_like(sad, dy), np.full_like(sad, dx))
            less = np.zeros((mbh, mbw), dtype=bool)
            equal = np.ones((mbh, mbw), dtype=bool)
            for a, b in zip(cand, best):
                less |= equal & (a < b)
                equal &= a == b
            take = less & ok[dy + R, dx + R]
            best = [np.where(take, a, b) for a, b in zip(cand, best)]
    sad, mvh, mvv = best[0], 2 * best[3], 2 * best[2]
    if R:
        rng = 16 if R <= 7 else 32
        for row in range(mbh):
            for col in range(mbw):
                blk = c[row * 16:row * 16 + 16, col * 16:col * 16 + 16]
                bh, bv = int(mvh[row, col]), int(mvv[row, col])
                found = None
                for hv in (-1, 0, 1):
                    for hh in (-1, 0, 1):
                        mh, mv = bh + hh, bv + hv
                        if (hh or hv) and -rng <= mh < rng and -rng <= mv < rng and mv_ok(cw, ch, col, row, mh, mv):
                            t = (int(np.abs(blk - predict(ref, col * 16, row * 16, mh, mv, 16)).sum()), hv, hh)
                            if found is None or t < found:
                                found = t
                if found is not None and found[0] < sad[row, col]:
                    sad[row, col], mvh[row, col], mvv[row, col] = found[0], bh + found[2], bv + found[1]
    return sad, mvh, mvv


def activity(cur, cw, ch):
    b = cur.astype(np.int64).reshape(ch // 16, 16, cw // 16, 16)
    mean = (b.sum(axis=(1, 3)) + 128) >> 8
    return np.abs(b - mean[:, None, :, None]).sum(axis=(1, 3))


# ---------------------------------------------------------------------------------------------------- 4. the decoder's side

def dequant(level, intra, q, weight):
    """oracle_dequant (mpeg1.c:1535-1551) on arrays; 0 where the level is 0"""
    lv = level.astype(np.int64)
    v = lv * 2
    if not intra:
        v = v + np.sign(lv)
    v = (v * q * weight) >> 4
    v = np.where((v & 1) == 0, np.where(v > 0, v - 1, v + 1), v)
    v = np.clip(v, -2048, 2047) * PREMULT
    return np.where(lv == 0, 0, v)


def _idct_1d(s, final):
    s0, s1, s2, s3, s4, s5, s6, s7 = s
    b1, b3, b4, tmp1, tmp2, b6 = s4, s2 + s6, s5 - s3, s1 + s7, s3 + s5, s1 - s7
    b7, m0 = tmp1 + tmp2, s0
    x4 = ((b6 * 473 - b4 * 196 + 128) >> 8) - b7
    x0 = x4 - (((tmp1 - tmp2) * 362 + 128) >> 8)
    x1 = m0 - b1
    x2 = (((s2 - s6) * 362 + 128) >> 8) - b3
    x3 = m0 + b1
    y3, y4, y5, y6 = x1 + x2, x3 + b3, x1 - x2, x3 - b3
    y7 = -x0 - ((b4 * 473 + b6 * 196 + 128) >> 8)
    o = [b7 + y4, x4 + y3, y5 - x0, y6 - y7, y6 + y7, x0 + y5, y3 - x4, y4 - b7]
    return [(v + 128) >> 8 for v in o] if final else o


def idct(coef):
    """[..., 8, 8] premultiplied coefficients -> residual (mpeg1.c:1673-1740): columns, then rows with the final rounding"""
    c = np.stack(_idct_1d([coef[..., k, :] for k in range(8)], False), axis=-2)
    return np.stack(_idct_1d([c[..., :, k] for k in range(8)], True), axis=-1)


def decode_blocks(levels, intra, q, dc=None):
    """what the decoder adds (or, intra, shows) for blocks of raster levels [..., 8, 8]; intra: `dc` [...] apart, levels[..., 0, 0] ignored"""
    lv = levels.copy()
    if intra:
        lv[..., 0, 0] = 0
    coef = dequant(lv, intra, q, W if intra else 16)
    if intra:
        coef[..., 0, 0] = dc * 256
    n_ac = np.count_nonzero(lv.reshape(lv.shape[:-2] + (64,))[..., 1:], axis=-1)
    single = n_ac == 0 if intra else (n_ac == 0) & (lv[..., 0, 0] != 0)
    short = np.broadcast_to(((coef[..., 0, 0] + 128) >> 8)[..., None, None], coef.shape)
    return np.where(single[..., None, None], short, idct(coef))


# ---------------------------------------------------------------------------------------------------- pictures

def mb_blocks(y, cr, cb):
    """planes -> [mbh, mbw, 6, 8, 8] in syntax order Y0 Y1 Y2 Y3 Cb Cr"""
    by, bcr, bcb = blocks(y), blocks(cr), blocks(cb)
    mbh, mbw = bcr.shape[:2]
    out = np.zeros((mbh, mbw, 6, 8, 8), dtype=np.int64)
    for b in range(4):
        out[:, :, b] = by[(b >> 1)::2, (b & 1)::2]
    out[:, :, 4], out[:, :, 5] = bcb, bcr
    return out


def from_mb_blocks(m):
    """the inverse: (Y, Cr, Cb)"""
    mbh, mbw = m.shape[:2]
    y = np.zeros((mbh * 16, mbw * 16), dtype=np.int64)
    for b in range(4):
        y.reshape(mbh, 2, 8, mbw, 2, 8)[:, b >> 1, :, :, b & 1, :] = m[:, :, b].transpose(0, 2, 1, 3)
    un = lambda p: p.transpose(0, 2, 1, 3).reshape(mbh * 8, mbw * 8)
    return y, un(m[:, :, 5]), un(m[:, :, 4])


def scan_order(raster):
    return raster.reshape(raster.shape[:-2] + (64,))[..., ZZA]


class Picture:
    """one picture's decisions: per macroblock kind ('I', 'C' coded, 'N' not coded, 'S' skipped), vector, levels, and its reconstruction"""


def code_picture(frame, ref, cw, ch, q, R, p_picture):
    y, cr, cb = planes(frame, cw, ch)
    mbh, mbw = ch // 16, cw // 16
    src = mb_blocks(y, cr, cb)
    # intra, every macroblock: enc_ref's quantiser
    c8 = c8_integer(src)
    li = enc_ref.quantise(c8, q)
    rec_i = np.clip(decode_blocks(li, True, q, dc=li[..., 0, 0]), 0, 255)
    pic = Picture()
    pic.kind = np.full((mbh, mbw), "I", dtype="<U1")
    pic.mv = np.zeros((mbh, mbw, 2), dtype=np.int64)
    pic.levels = scan_order(li)
    rec = rec_i
    if p_picture:
        ry, rcr, rcb = planes(ref, cw, ch)
        sad, mvh, mvv = search(y, ry, cw, ch, R)
        inter = ~(activity(y, cw, ch) + INTRA_BIAS < sad)
        pred = np.zeros_like(src)
        for row in range(mbh):
            for col in range(mbw):
                mh, mv = int(mvh[row, col]), int(mvv[row, col])
                py = predict(ry, col * 16, row * 16, mh, mv, 16)
                for b in range(4):
                    pred[row, col, b] = py[(b >> 1) * 8:(b >> 1) * 8 + 8, (b & 1) * 8:(b & 1) * 8 + 8]
                c_h, c_v = int(mh / 2), int(mv / 2)
                pred[row, col, 4] = predict(rcb, col * 8, row * 8, c_h, c_v, 8)
                pred[row, col, 5] = predict(rcr, col * 8, row * 8, c_h, c_v, 8)
        c8p = c8_integer(src - pred)
        lp = np.sign(c8p) * np.minimum(255, np.abs(c8p) // (16 * q))
        rec_p = np.clip(pred + decode_blocks(lp, False, q), 0, 255)
        coded_any = lp.reshape(mbh, mbw, -1).any(axis=-1)
        moved = (mvh != 0) | (mvv != 0)
        edge = np.zeros((mbh, mbw), dtype=bool)
        edge[:, 0] = edge[:, -1] = True
        kind = np.where(coded_any, "C", np.where(moved | edge, "N", "S"))
        pic.kind = np.where(inter, kind, "I")
        pic.mv = np.where(inter[..., None], np.stack([mvh, mvv], axis=-1), 0)
        pic.levels = np.where(inter[..., None, None], scan_order(lp), pic.levels)
        rec = np.where(inter[..., None, None, None], rec_p, rec_i)
    ry2, rcr2, rcb2 = from_mb_blocks(rec)
    pic.recon = np.concatenate([ry2.ravel(), rcr2.ravel(), rcb2.ravel()]).astype(np.uint8)
    return pic


def picture_bytes(pic, width, height, q, frame_rate_code, ordinal, gop, R):
    """the picture's bytes; pic.stuffed: the slices whose last macroblock got a stuffing code"""
    pic.stuffed = 0
    cw, ch = coded(width, height)
    mbw, mbh = cw // 16, ch // 16
    p_picture = ordinal % gop != 0
    r_size = 0 if R <= 7 else 1
    rng = 16 << r_size
    w = Bits()
    if not p_picture:
        w.start_code(0xB3)
        w.put(width, 12); w.put(height, 12); w.put(1, 4); w.put(frame_rate_code, 4); w.put(0x3FFFF, 18); w.put(1, 1); w.put(20, 10)
        w.put(0, 1); w.put(0, 1); w.put(0, 1)
        w.start_code(0xB8)
        fps = FPS[frame_rate_code]
        s = ordinal // fps
        w.put(0, 1); w.put((s // 3600) % 24, 5); w.put((s // 60) % 60, 6); w.put(1, 1); w.put(s % 60, 6); w.put(ordinal % fps, 6)
        w.put(1, 1); w.put(0, 1)
    w.start_code(0x00)
    w.put(ordinal % gop, 10); w.put(2 if p_picture else 1, 3); w.put(0xFFFF, 16)
    if p_picture:
        w.put(0, 1); w.put(r_size + 1, 3)
    w.put(0, 1)
    for row in range(mbh):
        w.start_code(row + 1)
        w.put(q, 5); w.put(0, 1)
        dc_pred, pmh, pmv, last = [128, 128, 128], 0, 0, -1
        for col in range(mbw):
            kind = pic.kind[row, col]
            if kind == "S":
                dc_pred, pmh, pmv = [128, 128, 128], 0, 0
                continue
            m = Bits()                                  # the macroblock apart: its length decides about stuffing
            inc = col - last
            last = col
            while inc > 33:
                m.code(INV["MBA"][35]); inc -= 33
            m.code(INV["MBA"][inc])
            lv = pic.levels[row, col]
            mvh, mvv = int(pic.mv[row, col, 0]), int(pic.mv[row, col, 1])
            cbp = 0
            if kind == "I":
                m.code(INV["MBTYPE_P" if p_picture else "MBTYPE_I"][0x01])
                pmh = pmv = 0
                for b in range(6):
                    comp = 0 if b < 4 else b - 3
                    diff = int(lv[b][0]) - dc_pred[comp]
                    size = 0 if diff == 0 else abs(diff).bit_length()
                    m.code(INV["DCSIZE_LUMA" if b < 4 else "DCSIZE_CHROMA"][size])
                    if size:
                        m.put(diff if diff > 0 else diff + (1 << size) - 1, size)
                    dc_pred[comp] = int(lv[b][0])
                    put_coeffs(m, [int(v) for v in lv[b][1:]], False)
            else:
                dc_pred = [128, 128, 128]
                for b in range(6):
                    if np.any(lv[b]):
                        cbp |= 0x20 >> b
                with_vector = kind == "N" or mvh != 0 or mvv != 0
                m.code(INV["MBTYPE_P"][(0x0A if with_vector else 0x02) if cbp else 0x08])
                if with_vector:
                    for cur_mv, prev in ((mvh, pmh), (mvv, pmv)):
                        d = cur_mv - prev
                        d = d + 2 * rng if d < -rng else (d - 2 * rng if d >= rng else d)
                        put_motion(m, d, r_size)
                    pmh, pmv = mvh, mvv
                else:
                    pmh = pmv = 0
                if cbp:
                    m.code(INV["CBP"][cbp])
                    for b in range(6):
                        if cbp & (0x20 >> b):
                            put_coeffs(m, [int(v) for v in lv[b]], True)
            nbits = len(m.out) * 8 + m.n
            if col == mbw - 1 and w.n and w.n + nbits <= 8:
                w.code(STUFFING)
                pic.stuffed += 1
            for byte in m.out:
                w.put(byte, 8)
            if m.n:
                w.put(m.acc, m.n)
    w.align()
    return bytes(w.out)


class Result:
    pass


def encode(frames, width, height, gop, search_range, streams=None, qscale=8, frame_rate_code=5, end=True):
    """The whole call with a GOP: .buf (with the 0xff gaps), .ranges [(offset, bytes)], .streams {stream: (begin, end)},
    .recon [frame bytes], .vectors [[(mvh, mvv) or None]], .stats [(intra, coded, not coded, skipped)], .stuffed [slices per
    picture whose last macroblock got a stuffing code]"""
    n = len(frames)
    cw, ch = coded(width, height)
    streams = [0] * n if streams is None else [int(s) for s in streams]
    qs = [int(qscale)] * n if np.isscalar(qscale) else [int(v) for v in qscale]
    out = bytearray(b"\xff" * 16)
    r = Result()
    r.ranges, sr, r.recon, r.vectors, r.stats, r.stuffed = [], {}, [], [], [], []
    ordinal = 0
    for k in range(n):
        ordinal = ordinal + 1 if k and streams[k] == streams[k - 1] else 0
        if not k or streams[k] != streams[k - 1]:
            sr[streams[k]] = [len(out), None]
        p_picture = ordinal % gop != 0
        pic = code_picture(frames[k], r.recon[-1] if p_picture else None, cw, ch, qs[k], search_range, p_picture)
        data = picture_bytes(pic, width, height, qs[k], frame_rate_code, ordinal, gop, search_range)
        r.ranges.append((len(out), len(data)))
        out += data
        r.recon.append(pic.recon)
        r.stuffed.append(pic.stuffed)
        r.vectors.append([None if kd == "I" else (int(v[0]), int(v[1])) for kd, v in zip(pic.kind.ravel(), pic.mv.reshape(-1, 2))])
        r.stats.append(tuple(int(np.count_nonzero(pic.kind == kd)) for kd in "ICNS"))
        if k + 1 == n or streams[k + 1] != streams[k]:
            if end:
                out += b"\x00\x00\x01\xb7"
            sr[streams[k]][1] = len(out)
            # to the next 16-byte aligned begin, at least 8 bytes away; behind the call's last stream, to the next multiple of 16
            out += b"\xff" * (-len(out) % 16 if k + 1 == n else 8 + -(len(out) + 8) % 16)
    r.buf, r.streams = bytes(out), {s: tuple(v) for s, v in sr.items()}
    return r
