"""TEST INFRASTRUCTURE ONLY -- a writer of EXACT macroblocks: an MPEG-1 video elementary stream from a plain description
(which macroblock has which type, quantiser scale and vector; which block holds which levels), and on top of it the
streams the reconstruct's tests are built from:

  sweep_stream()    every tile of every picture holds a chosen number A of low-frequency transform blocks and B of other
                    transform blocks, at chosen lanes -- the two counts that decide every branch of the slot packing in
                    kernels.hip jm_recon_tile (tests/test_craft_es.py holds the accounting, tests/test_gpu_recon_slots.py
                    the GPU side)
  bounds_stream()   the integer transform at the bounds tools/idct_bounds.py states: per output pixel and per
                    multiplication operand the sign pattern of full-amplitude levels that drives it furthest, a ladder of
                    intra DC values up to 3953 and down to -3952, random full-amplitude blocks
                    (tests/golden/craft_bounds_192x192.m1v, registered in tests/golden/make_golden.py)

The writer also places skipped macroblocks, increments with escapes and stuffing, slice breaks anywhere, forced escapes and user
data: the slice parse's inputs are built on it in tests/parse_inputs.py.

Nothing here includes or calls the code under test: the syntax is ISO 11172-2 as tests/enc/mpeg1_enc.py states it (its
bit writer helpers and VLC tables are reused), the tile geometry is restated from the design (recon_block.h JmTiles:
which block of a plane sits in which lane of which workgroup).

    python tests/craft_es.py      # regenerates tests/golden/craft_bounds_192x192.m1v (then tests/golden/make_golden.py)
"""
import os
import random
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (ROOT, os.path.join(HERE, "enc"), os.path.join(ROOT, "tools")):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import idct_bounds  # noqa: E402
import mpeg1_enc as E  # noqa: E402

DC_LIMIT = 3953                 # 128 + 15 * 255: what the ladder reaches; the contract allows +-4095


# ----------------------------------------------------------------------------------------------------------------
# the writer

class _StrBits:
    """mpeg1_enc.Bits' put / code on a string of '0' and '1' (what put_coeffs and put_motion need)"""
    def __init__(self):
        self.parts = []

    def put(self, value, nbits):
        if nbits:
            self.parts.append(format(int(value) & ((1 << nbits) - 1), "0%db" % nbits))

    def code(self, bits):
        self.parts.append(bits)

    def text(self):
        return "".join(self.parts)


_coef_cache = {}


def _coef_bits(levels, first_is_special):
    key = (tuple(levels), first_is_special)
    s = _coef_cache.get(key)
    if s is None:
        w = _StrBits()
        E.put_coeffs(w, key[0], first_is_special)
        s = _coef_cache[key] = w.text()
    return s


_dc_cache = {}


def _dc_bits(diff, luma):
    key = (diff, luma)
    s = _dc_cache.get(key)
    if s is None:
        assert -255 <= diff <= 255
        size = 0 if diff == 0 else abs(diff).bit_length()
        s = E.INV["DCSIZE_LUMA" if luma else "DCSIZE_CHROMA"][size]
        if size:
            s += format(diff if diff > 0 else diff + (1 << size) - 1, "0%db" % size)
        _dc_cache[key] = s
    return s


_mv_cache = {}


def _mv_bits(d, r_size):
    key = (d, r_size)
    s = _mv_cache.get(key)
    if s is None:
        w = _StrBits()
        E.put_motion(w, d, r_size)
        s = _mv_cache[key] = w.text()
    return s


def _bytes_of(bits):
    bits += "0" * (-len(bits) % 8)
    return int(bits, 2).to_bytes(len(bits) // 8, "big") if bits else b""


def coef_symbols(levels, first_is_special, esc=()):
    """the DCT symbols of one block, in order: [(run, level, form, bits)] with form "first" (the non-intra first coefficient's
    `1s`), "vlc" or "esc20" / "esc28"; esc: the scan INDICES into `levels` whose coefficient takes the escape whatever shorter code
    exists (True: all of them).  The end_of_block is not in the list."""
    out = []
    run, first = 0, first_is_special
    for i, lv in enumerate(levels):
        if lv == 0:
            run += 1
            continue
        assert -255 <= lv <= 255
        mag = abs(lv)
        forced = esc is True or i in esc
        if not forced and run == 0 and mag == 1:
            out.append((run, lv, "first" if first else "vlc", ("1" if first else "11") + ("1" if lv < 0 else "0")))
        elif not forced and (run, mag) in E.COEFF:
            out.append((run, lv, "vlc", E.COEFF[(run, mag)] + ("1" if lv < 0 else "0")))
        else:
            s = E.T["DCT_ESCAPE"] + format(run, "06b")
            if -127 <= lv <= 127:
                out.append((run, lv, "esc20", s + format(lv & 0xFF, "08b")))
            else:
                out.append((run, lv, "esc28", s + ("00000000" if lv > 0 else "10000000") + format(lv & 0xFF, "08b")))
        run, first = 0, False
    return out


def _coef_bits_forms(levels, first_is_special, esc):
    return "".join(s[3] for s in coef_symbols(levels, first_is_special, esc)) + "10"


def _mba_bits(inc, stuffing=0):
    """macroblock_address_increment: `stuffing` macroblock_stuffing codes, a macroblock_escape per 33, the code of the rest"""
    parts = [E.INV["MBA"][34]] * stuffing
    while inc > 33:
        parts.append(E.INV["MBA"][35])
        inc -= 33
    parts.append(E.INV["MBA"][inc])
    return "".join(parts)


USER_DATA_BYTE = 0xA5


def write_stream(desc):
    """desc: dict(width, height, frame_rate_code=5, intra_matrix=None, non_intra_matrix=None (64 values in scan order, as the
    header carries them), pictures=[...]); a picture: dict(type="I" | "P", full_pel=0, f_code=1, mbs=[...]) with one entry per
    macroblock in raster order; a macroblock: (q, kind, mv, blocks) with kind "intra" | "coded" (P, no vector) |
    "coded_mv" | "mv" (vector only), mv = (h, v) in the units the stream codes (half-pels, or pels with full_pel), blocks = six
    entries: intra (dc_differential, levels of scan positions 1..) ; else None (not coded) or the levels of scan positions 0..
    (trailing zeros may be left out).  One slice per macroblock row.  -> (es: np.uint8[], pic_offsets: np.uint32[n + 1])

    Beyond that (the slice parse's inputs, tests/parse_inputs.py), all optional:
      a macroblock (q, "skip", None, None) of a P picture is left out of the stream (the next coded one's increment covers it);
      a fifth entry of a macroblock, a dict: stuffing=n (macroblock_stuffing codes in front of its increment), esc={block: scan
      indices into that block's levels, or True} (coefficients that take the escape although a shorter code exists), mv_d=(dh, dv)
      (a motion differential as given -- None: as computed --, where two land on the same vector: +16 f and -16 f);
      a picture's slices=[start, ...] or [dict(start=macroblock, row=the row its start code names (default: the macroblock's own;
      an earlier one makes the first increment that much larger), extra=n extra_information_slice bytes), ...]: a slice runs from
      its start to the next one's, over row ends if need be (default: one per row); user_data=n: a user-data start code and n
      bytes in front of the picture's start code (pic_offsets points at it)."""
    width, height = desc["width"], desc["height"]
    mbw, mbh = (width + 15) >> 4, (height + 15) >> 4
    cw, ch = mbw * 16, mbh * 16
    out = bytearray()
    h = _StrBits()
    h.put(width, 12); h.put(height, 12); h.put(1, 4); h.put(desc.get("frame_rate_code", 5), 4); h.put(0x3FFFF, 18); h.put(1, 1)
    h.put(20, 10); h.put(0, 1)
    for m in (desc.get("intra_matrix"), desc.get("non_intra_matrix")):
        h.put(m is not None, 1)
        for v in (m or ()):
            assert 1 <= v <= 255
            h.put(v, 8)
    out += b"\x00\x00\x01\xb3" + _bytes_of(h.text())
    g = _StrBits()
    g.put(0, 1); g.put(0, 5); g.put(0, 6); g.put(1, 1); g.put(0, 6); g.put(0, 6); g.put(1, 1); g.put(0, 1)
    out += b"\x00\x00\x01\xb8" + _bytes_of(g.text())
    n_codes = 2
    pic_offsets = []
    for t, pic in enumerate(desc["pictures"]):
        is_p = pic["type"] == "P"
        assert pic["type"] in ("I", "P") and (t > 0 or not is_p)
        full_pel, f_code = pic.get("full_pel", 0), pic.get("f_code", 1)
        r_size = f_code - 1
        span = 16 << r_size
        pic_offsets.append(len(out))
        if pic.get("user_data") is not None:
            out += b"\x00\x00\x01\xb2" + bytes([USER_DATA_BYTE]) * pic["user_data"]
            n_codes += 1
        ph = _StrBits()
        ph.put(t & 1023, 10); ph.put(2 if is_p else 1, 3); ph.put(0xFFFF, 16)
        if is_p:
            assert 1 <= f_code <= 7
            ph.put(full_pel, 1); ph.put(f_code, 3)
        ph.put(0, 1)
        out += b"\x00\x00\x01\x00" + _bytes_of(ph.text())
        n_codes += 1
        mbs = pic["mbs"]
        assert len(mbs) == mbw * mbh
        mbtype = E.INV["MBTYPE_P" if is_p else "MBTYPE_I"]
        slices = [s if isinstance(s, dict) else dict(start=s) for s in pic.get("slices", range(0, mbw * mbh, mbw))]
        assert slices and slices[0]["start"] == 0 and all(a["start"] < b["start"] for a, b in zip(slices, slices[1:]))
        for si, sl in enumerate(slices):
            start = sl["start"]
            stop = slices[si + 1]["start"] if si + 1 < len(slices) else mbw * mbh
            code_row = sl.get("row", start // mbw)
            assert 0 <= code_row <= start // mbw and code_row < 175
            assert mbs[start][1] != "skip" and mbs[stop - 1][1] != "skip", "a slice begins and ends with a coded macroblock"
            q = mbs[start][0]
            parts = [format(q, "05b")] + ["1" + format(USER_DATA_BYTE, "08b")] * sl.get("extra", 0) + ["0"]
            dc = [128, 128, 128]
            pmh = pmv = 0
            last_len = 0
            inc = start - code_row * mbw + 1
            for addr in range(start, stop):
                row, col = divmod(addr, mbw)
                entry = mbs[addr]
                new_q, kind, mv, blocks = entry[:4]
                opts = entry[4] if len(entry) > 4 else {}
                if kind == "skip":
                    # left out: the decoder's resets (mpeg1.c:1060-1082)
                    assert is_p, "intra pictures skip nothing"
                    inc += 1
                    dc = [128, 128, 128]
                    pmh = pmv = 0
                    continue
                esc = opts.get("esc", {})
                assert 1 <= new_q <= 31 and len(blocks) == 6
                mb = [_mba_bits(inc, opts.get("stuffing", 0))]
                inc = 1
                use_q = new_q != q
                if kind == "intra":
                    mb.append(mbtype[0x11 if use_q else 0x01])
                    if use_q:
                        mb.append(format(new_q, "05b"))
                    pmh = pmv = 0
                    for b, (diff, levels) in enumerate(blocks):
                        comp = 0 if b < 4 else b - 3
                        dc[comp] += diff
                        assert abs(dc[comp]) <= DC_LIMIT, "intra DC %d" % dc[comp]
                        mb.append(_dc_bits(diff, b < 4))
                        mb.append(_coef_bits_forms(levels, False, esc[b]) if b in esc else _coef_bits(levels, False))
                else:
                    assert is_p and kind in ("coded", "coded_mv", "mv")
                    cbp = 0
                    for b in range(6):
                        if blocks[b] is not None:
                            assert any(blocks[b]), "a coded block holds a coefficient"
                            cbp |= 0x20 >> b
                    assert (cbp != 0) == (kind != "mv") and not (kind == "mv" and use_q), "vector-only macroblocks carry neither pattern nor quantiser"
                    mb.append(mbtype[{"coded": 0x02, "coded_mv": 0x0A, "mv": 0x08}[kind] | (0x10 if use_q else 0)])
                    if use_q:
                        mb.append(format(new_q, "05b"))
                    dc = [128, 128, 128]
                    if kind == "coded":
                        pmh = pmv = 0
                    else:
                        mh, mvv = (mv[0] << 1, mv[1] << 1) if full_pel else mv
                        assert E.mv_ok(cw, ch, col, row, mh, mvv), "vector (%d, %d) leaves the picture at macroblock (%d, %d)" % (mh, mvv, col, row)
                        for cur, prev, given in ((mv[0], pmh, opts.get("mv_d", (None, None))[0]), (mv[1], pmv, opts.get("mv_d", (None, None))[1])):
                            assert -span <= cur < span
                            d = cur - prev
                            d = d + 2 * span if d < -span else (d - 2 * span if d >= span else d)
                            if given is not None:                      # the other differential that lands on the same vector: +16 f for -16 f
                                assert (given - d) % (2 * span) == 0 and -span <= given <= span
                                d = given
                            mb.append(_mv_bits(d, r_size))
                        pmh, pmv = mv
                    if cbp:
                        mb.append(E.INV["CBP"][cbp])
                        for b in range(6):
                            if blocks[b] is not None:
                                mb.append(_coef_bits_forms(blocks[b], True, esc[b]) if b in esc else _coef_bits(blocks[b], True))
                q = new_q
                s = "".join(mb)
                last_len = len(s)
                parts.append(s)
            # the reference finds "next bytes are a start code" true one macroblock early when the last one fits into the slack of
            # the slice's last byte (fixture uncovered_last_mb_*): not what these streams are about
            assert last_len > 8, "the last macroblock of a slice is %d bits" % last_len
            payload = _bytes_of("".join(parts))
            assert payload.find(b"\x00\x00\x01") < 0, "start code emulated inside a slice"
            out += bytes([0, 0, 1, code_row + 1]) + payload
            n_codes += 1
    out += b"\x00\x00\x01\xb7"
    n_codes += 1
    pic_offsets.append(len(out) - 4)
    pic_offsets[0] = 0
    es = np.frombuffer(bytes(out), dtype=np.uint8).copy()
    found = int(np.count_nonzero((es[:-3] == 0) & (es[1:-2] == 0) & (es[2:-1] == 1)))
    assert found == n_codes, "start code emulated (%d codes, %d written)" % (found, n_codes)
    return es, np.array(pic_offsets, dtype=np.uint32)


# ----------------------------------------------------------------------------------------------------------------
# tile geometry, restated from the design (recon_block.h JmTiles): a reconstruct workgroup of 256 lanes
# takes one tile of one plane; the packing ranks a tile's transform blocks in lane order.

WG = 256


def tiles_of(width, height):
    """-> [dict(kind, plane (0 luma, 1 the plane of block 4, 2 of block 5; linear chroma tiles: 1), lanes=[(lane, mb, block)] in
    lane order -- the lanes that hold a block]"""
    mbw, mbh = (width + 15) >> 4, (height + 15) >> 4
    mbs = mbw * mbh
    out = []
    if 2 * mbw < 64:                                        # narrow pictures: consecutive blocks of the plane's block raster
        bw = 2 * mbw
        for t in range((4 * mbs + WG - 1) // WG):
            lanes = []
            for lane in range(WG):
                g = t * WG + lane
                if g < 4 * mbs:
                    by, bx = divmod(g, bw)
                    lanes.append((lane, (by >> 1) * mbw + (bx >> 1), ((by & 1) << 1) | (bx & 1)))
            out.append(dict(kind="linear luma, %d blocks" % len(lanes), plane=0, lanes=lanes))
        for t in range((2 * mbs + WG - 1) // WG):
            lanes = []
            for lane in range(WG):
                g = t * WG + lane
                if g < 2 * mbs:
                    lanes.append((lane, g % mbs, 4 + g // mbs))
            out.append(dict(kind="linear chroma, %d blocks" % len(lanes), plane=1, lanes=lanes))
        return out
    for plane in range(3):
        bw, bh = (2 * mbw, 2 * mbh) if plane == 0 else (mbw, mbh)
        full, rem = divmod(bw, 32)
        rem16 = 0 < rem <= 16
        specs = [(tx * 32, 32, False, ty) for ty in range((bh + 7) // 8) for tx in range(full)]
        if rem:
            specs += [(full * 32, rem, rem16, ty) for ty in range((bh + 15) // 16 if rem16 else (bh + 7) // 8)]
        for x0, tw, narrow, ty in specs:
            lanes = []
            for lane in range(WG):
                wave, l = divmod(lane, 64)
                if narrow:
                    lx, by = l & 15, ty * 16 + 4 * wave + (l >> 4)
                else:
                    lx, by = l & 31, ty * 8 + 2 * wave + (l >> 5)
                if lx < tw and by < bh:
                    bx = x0 + lx
                    if plane == 0:
                        lanes.append((lane, (by >> 1) * mbw + (bx >> 1), ((by & 1) << 1) | (bx & 1)))
                    else:
                        lanes.append((lane, by * mbw + bx, 3 + plane))
            rows = len({(ln // 64, (ln % 64) >> (4 if narrow else 5)) for ln, _, _ in lanes})
            out.append(dict(kind="%s %d wide, %d rows, %s" % ("16-lane rows" if narrow else "32-lane rows", tw, rows, "luma" if plane == 0 else "chroma"),
                            plane=plane, lanes=lanes))
    return out


# block classes, as the packing sees a block (recon_block.h jm_recon_front)
NONE, LOWF, FULL = 0, 1, 2


def block_class(intra, block):
    """what a block of a description is to the packing: NONE (no transform: no tokens, an intra DC alone, the (0,0) coefficient
    alone), LOWF (at most 8 tokens -- an intra block's DC is one --, the last at a scan position <= 9) or FULL"""
    if intra:
        pos = [i + 1 for i, v in enumerate(block[1]) if v]
        if not pos:
            return NONE
        return LOWF if len(pos) + 1 <= 8 and pos[-1] <= 9 else FULL
    if block is None:
        return NONE
    pos = [i for i, v in enumerate(block) if v]
    if pos == [0]:
        return NONE
    return LOWF if len(pos) <= 8 and pos[-1] <= 9 else FULL


# ----------------------------------------------------------------------------------------------------------------
# the transform's bounds: block set derived from the network as tools/idct_bounds.py states it

def network(levels, intra_dc=None):
    """tools/idct_bounds.py's network on one block of dequantised levels (raster order); intra: position 0 holds dc << 8 instead
    of a premultiplied level (mpeg1.c:1489).  -> (64 outputs, the 96 multiplication operands by site: the first operand of each
    of the six mul() calls of a 1-D pass, 8 column passes then 8 row passes; b6 and b4 feed two sites each)"""
    blk = [int(levels[k]) * idct_bounds.PM[k] for k in range(64)]
    if intra_dc is not None:
        blk[0] = intra_dc << 8
    ops = []
    orig = idct_bounds.mul

    def rec(x, c):
        ops.append(x)
        return orig(x, c)

    idct_bounds.mul = rec
    try:
        res = idct_bounds.idct(blk)
    finally:
        idct_bounds.mul = orig
    assert len(ops) == 96
    return res, ops


_bounds_cache = {}


def bounds_blocks():
    """-> dict(pixel=[128 blocks], site=[192], ladder=[(dc, block) x 32], random=[512]); a block: 64 levels of +2047 / -2048 in raster
    order"""
    if _bounds_cache:
        return _bounds_cache
    outs, ops = [], []
    for k in range(64):
        lv = [0] * 64
        lv[k] = 2047
        o, p = network(lv)
        outs.append(o); ops.append(p)

    def pattern(resp, sign):
        return [2047 if (resp[k] >= 0) == (sign > 0) else -2048 for k in range(64)]

    pixel = [pattern([outs[k][p] for k in range(64)], s) for p in range(64) for s in (1, -1)]
    site = [pattern([ops[k][j] for k in range(64)], s) for j in range(96) for s in (1, -1)]
    # the ladder: a chain of 16 blocks up (+255 fifteen times from 128: 3953, then once more the same value) under the patterns that
    # drive a pixel highest, a chain of 16 down (-255 sixteen times: -3952) under the ones that drive it lowest
    # (an intra block's position 0 holds the DC, not a level: the pixels are ranked by what the other 63 inputs can add, and the
    # strongest go to the top of each chain)
    order = sorted(range(64), key=lambda p: sum(abs(outs[k][p]) for k in range(1, 64)))[-16:]
    ladder = [(min(128 + 255 * (i + 1), DC_LIMIT), pixel[2 * order[i]]) for i in range(16)]
    ladder += [(128 - 255 * (i + 1), pixel[2 * order[i] + 1]) for i in range(16)]
    rng = random.Random(0xB0D5)
    rnd = [[2047 if rng.getrandbits(1) else -2048 for _ in range(64)] for _ in range(512)]
    _bounds_cache.update(pixel=pixel, site=site, ladder=ladder, random=rnd)
    return _bounds_cache


def bounds_figures():
    """what the tool's network gives for the set: the four figures the fixture records"""
    S = bounds_blocks()
    hi = lo = op = dc_hi = 0
    for blk in S["pixel"] + S["site"] + S["random"] + [b for _, b in S["ladder"]]:
        o, p = network(blk)
        hi, lo, op = max(hi, max(o)), min(lo, min(o)), max(op, max(abs(x) for x in p))
    for dc, blk in S["ladder"]:
        o, p = network(blk, intra_dc=dc)
        dc_hi, op = max(dc_hi, max(abs(x) for x in o)), max(op, max(abs(x) for x in p))
    return dict(max_output_non_intra=hi, min_output_non_intra=lo, max_abs_output_dc_ladder=dc_hi, max_operand=op)


def _level_of(v):
    return 255 if v > 0 else -255              # escape level +-255 at quantiser scale 31 under a matrix of 255: +2047, and -2048 by the clip


def _scan(raster):
    return [raster[E.ZZ[i]] for i in range(64)]


BOUNDS_NAME = "craft_bounds_192x192"


def bounds_desc():
    """192x192, two pictures: the set as intra blocks, then the same set as residuals over picture 0"""
    S = bounds_blocks()
    mbw = 12
    others = S["pixel"] + S["site"] + S["random"]
    assert len(others) + len(S["ladder"]) == 864
    ladder_at = {}                       # (macroblock, block) -> ladder index: the last four macroblocks of rows 0 (up) and 1 (down)
    for chain in range(2):
        for i in range(16):
            ladder_at[(chain * mbw + 8 + i // 4, i % 4)] = chain * 16 + i
    nxt = iter(others)
    intra, inter = [], []
    for mb in range(144):
        row, col = divmod(mb, mbw)
        bi, bp = [], []
        for b in range(6):
            if (mb, b) in ladder_at:
                k = ladder_at[(mb, b)]
                diff = (255 if k < 15 else 0) if k < 16 else -255
                raster = S["ladder"][k][1]
            else:
                diff, raster = 0, next(nxt)
            zz = [_level_of(v) for v in _scan(raster)]
            bi.append((diff, zz[1:]))
            bp.append(zz)
        intra.append((31, "intra", None, bi))
        mv = (1, 1) if (row + col) % 2 and col < mbw - 1 and row < mbw - 1 else (0, 0)
        inter.append((31, "coded_mv", mv, bp))
    return dict(width=192, height=192, intra_matrix=[255] * 64, non_intra_matrix=[255] * 64,
                pictures=[dict(type="I", mbs=intra), dict(type="P", full_pel=0, f_code=1, mbs=inter)])


def bounds_stream():
    return write_stream(bounds_desc())


# ----------------------------------------------------------------------------------------------------------------
# the slot-packing sweep

SWEEP_SHAPES = [(128, 128), (176, 144), (512, 64), (640, 64), (656, 64)]
TOTALS = (0, 1, 31, 32, 33, 127, 128, 129, 219, 220, 221, 255, 256)
# both sides of each condition of the rule that moves the second class up to a multiple of 32 (up = A rounded up; the rule:
# ceil(B / 32) < ceil((A + B) / 32) - floor(A / 32), and up + B <= slots), for 220 slots and for the dense form's 256
RULE_PAIRS = ((20, 20), (20, 12), (20, 13), (1, 32), (32, 20), (33, 64), (5, 188), (5, 189), (31, 188), (31, 189), (37, 156), (37, 157),
              (4, 188), (1, 31), (40, 30), (40, 24), (40, 25), (70, 124), (70, 125), (5, 224), (5, 225), (31, 224), (31, 225), (100, 121),
              (3, 10), (30, 3), (29, 3), (65, 155), (65, 156), (97, 123), (97, 124), (129, 91), (129, 92), (161, 59), (161, 60))


def ab_grid(cap):
    """the (A, B) pairs a tile of `cap` blocks takes, by their edges"""
    pairs = []
    for t in TOTALS:
        if t > cap:
            continue
        for a in (0, 1, 31, 32, 33, 64, 96, t - 33, t - 32, t - 31, t - 1, t):
            if 0 <= a <= t and (a, t - a) not in pairs:
                pairs.append((a, t - a))
    for a, b in RULE_PAIRS:
        if a + b <= cap and (a, b) not in pairs:
            pairs.append((a, b))
    return pairs


PLACEMENTS = ("first", "last", "shuffled")


def _pools(rng):
    """short blocks of each class: [intra: (AC levels of scan 1..)], [non-intra: levels of scan 0..]"""
    def lv():
        m = rng.choice((1, 1, 2, 3, 5, 9, 17, 40, 41, 127, 128, 255))
        return m if rng.getrandbits(1) else -m

    def make(positions, base):
        out = [0] * (max(positions) - base + 1)
        for p in positions:
            out[p - base] = lv()
        return out
    P = {}
    for intra in (True, False):
        base = 1 if intra else 0
        low = list(range(base, 10))
        a, b = [], []
        for _ in range(96):
            n = rng.randint(1, 3)
            pos = rng.sample(low, n)
            if not intra and pos == [0]:
                pos = [0, rng.randint(1, 9)]
            a.append(make(pos, base))
        a.append(make(rng.sample(low, 7 if intra else 8), base))          # eight tokens: the most a low-frequency block holds
        for i in range(96):
            pos = [rng.randint(10, 63)] + rng.sample(range(base, 64), rng.choice((0, 0, 1, 2, 3, 7, 8, 9, 17)))
            b.append(make(sorted(set(pos)), base))
        b.append(make(low[:8 if intra else 9], base))                       # nine tokens, all at low positions: past the eight looked at
        b.append(make(low, base))
        b.append(make([10], base)); b.append(make([63], base))
        P[intra] = {LOWF: a, FULL: b}
    P["k00"] = [[v] for v in (1, -1, 2, -3, 17, -128, 255, -255)]
    return P


def sweep_desc(width, height, predicted, seed=1):
    """-> (desc, plan): plan[picture] = None (a picture that only serves as a reference) or [(A, B, placement) per tile]"""
    rng = random.Random(seed * 7919 + width * 31 + height + (1 << 20) * predicted)
    mbw, mbh = (width + 15) >> 4, (height + 15) >> 4
    n_mb = mbw * mbh
    cw, ch = mbw * 16, mbh * 16
    tiles = tiles_of(width, height)
    pools = _pools(rng)
    S = bounds_blocks()
    full_amp = [[_level_of(v) for v in _scan(r)] for r in (S["pixel"][::9] + S["site"][::13] + S["random"][:16])]
    # tiles of one kind share the kind's cases between them
    by_kind = {}
    for i, t in enumerate(tiles):
        by_kind.setdefault(t["kind"], []).append(i)
    cases = {}
    n_sweep = 0
    for kind, idx in by_kind.items():
        cap = len(tiles[idx[0]]["lanes"])
        cs = [(a, b, p) for (a, b) in ab_grid(cap) for p in PLACEMENTS]
        rng.shuffle(cs)
        cases[kind] = cs
        n_sweep = max(n_sweep, (len(cs) + len(idx) - 1) // len(idx))
    pictures, plan = [], []
    for s in range(n_sweep):
        for ptype in (("I", "P") if predicted else ("I",)):
            sweep_here = (ptype == "P") == bool(predicted)
            cls = [[NONE] * 6 for _ in range(n_mb)]
            row_plan = []
            for kind, idx in by_kind.items():
                for j, ti in enumerate(idx):
                    cs = cases[kind]
                    if sweep_here:
                        a, b, place = cs[(s * len(idx) + j) % len(cs)]
                    else:                                                  # the noisy picture underneath: any counts
                        cap = len(tiles[ti]["lanes"])
                        a = rng.randint(0, cap); b = rng.randint(0, cap - a); place = "shuffled"
                    lanes = tiles[ti]["lanes"]
                    n = a + b
                    chosen = lanes[:n] if place == "first" else (lanes[len(lanes) - n:] if place == "last" else rng.sample(lanes, n))
                    # "first": the other class in the lowest lanes (its ranks come behind every low-frequency block's: a tile's first
                    # wavefront holds the blocks that wait), "last": in the highest, "shuffled": the classes mixed lane by lane
                    which = [FULL] * b + [LOWF] * a if place == "first" else [LOWF] * a + [FULL] * b
                    if place == "shuffled":
                        rng.shuffle(which)
                    for (_, mb, blk), c in zip(chosen, which):
                        cls[mb][blk] = c
                    row_plan.append((ti, a, b, place))
            row_plan.sort()
            plan.append([(a, b, p) for _, a, b, p in row_plan] if sweep_here else None)
            is_p = ptype == "P"
            loud = s % 8 == 7                                              # every eighth: the full-amplitude blocks of the bounds set
            f_code = 2 if is_p and s % 5 == 4 else 1
            full_pel = int(is_p and s % 7 == 6)
            reach = 6 if full_pel else (16 << (f_code - 1)) - 1
            mbs = []
            q = rng.randint(1, 31)
            dc = [128, 128, 128]
            for mb in range(n_mb):
                row, col = divmod(mb, mbw)
                if col == 0:
                    dc = [128, 128, 128]
                c6 = cls[mb]
                has_full = FULL in c6
                if rng.randrange(4) == 0:
                    q = rng.randint(1, 31)
                if loud and has_full:
                    q = 31
                if not is_p or rng.randrange(6) == 0:
                    blocks = []
                    for b in range(6):
                        comp = 0 if b < 4 else b - 3
                        diff = rng.randint(-24, 24)
                        if not 4 <= dc[comp] + diff <= 251:
                            diff = -diff
                        dc[comp] += diff
                        if c6[b] == NONE:
                            blocks.append((diff, ()))
                        elif c6[b] == FULL and loud:
                            blocks.append((diff, rng.choice(full_amp)[1:]))
                        else:
                            blocks.append((diff, rng.choice(pools[True][c6[b]])))
                    mbs.append((q, "intra", None, blocks))
                    continue
                dc = [128, 128, 128]
                blocks = []
                for b in range(6):
                    if c6[b] == NONE:
                        blocks.append(rng.choice(pools["k00"]) if rng.randrange(3) == 0 else None)
                    elif c6[b] == FULL and loud:
                        blocks.append(rng.choice(full_amp))
                    else:
                        blocks.append(rng.choice(pools[False][c6[b]]))
                coded = any(x is not None for x in blocks)
                if not coded and (col == mbw - 1 or rng.randrange(2)):
                    blocks[rng.randrange(6)] = rng.choice(pools["k00"])    # (a slice's last macroblock is longer than a vector alone)
                    coded = True
                kind = "mv" if not coded else ("coded" if rng.randrange(3) == 0 else "coded_mv")
                mv = None
                if kind != "coded":
                    for _ in range(64):
                        mv = (rng.randint(-reach, reach), rng.randint(-reach, reach))
                        if E.mv_ok(cw, ch, col, row, mv[0] << full_pel, mv[1] << full_pel):
                            break
                    else:
                        mv = (0, 0)
                mq = mbs[-1][0] if kind == "mv" and col > 0 else q         # a vector alone carries no quantiser: the one in force
                if kind == "mv" and col == 0:
                    mq = q
                mbs.append((mq, kind, mv, blocks))
                q = mq
            pictures.append(dict(type=ptype, full_pel=full_pel, f_code=f_code, mbs=mbs))
    return dict(width=width, height=height, pictures=pictures), plan


def tile_counts(desc, picture, tiles=None):
    """[(A, B, classes in lane order)] per tile of one picture of a description: what the packing is given"""
    tiles = tiles or tiles_of(desc["width"], desc["height"])
    mbs = desc["pictures"][picture]["mbs"]
    out = []
    for t in tiles:
        cl = []
        for lane, mb, blk in t["lanes"]:
            intra = mbs[mb][1] == "intra"
            cl.append((lane, block_class(intra, mbs[mb][3][blk])))
        out.append((sum(1 for _, c in cl if c == LOWF), sum(1 for _, c in cl if c == FULL), cl))
    return out


_sweep_cache = {}


def sweep_stream(width, height, predicted):
    """-> dict(es, offsets, desc, plan, seconds)"""
    key = (width, height, predicted)
    if key not in _sweep_cache:
        import time
        t0 = time.time()
        desc, plan = sweep_desc(width, height, predicted)
        es, offs = write_stream(desc)
        _sweep_cache[key] = dict(es=es, offsets=offs, desc=desc, plan=plan, seconds=time.time() - t0)
    return _sweep_cache[key]


if __name__ == "__main__":
    es, offs = bounds_stream()
    assert len(es) < 512 * 1024
    es.tofile(os.path.join(HERE, "golden", BOUNDS_NAME + ".m1v"))
    np.save(os.path.join(HERE, "golden", BOUNDS_NAME + ".offsets.npy"), offs)
    print("%-30s %d pictures, %d bytes" % (BOUNDS_NAME, len(offs) - 1, len(es)))
    print(bounds_figures())
