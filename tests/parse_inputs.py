"""TEST INFRASTRUCTURE ONLY -- the slice parse's inputs: crafted streams (tests/craft_es.py write_stream) that place chosen
symbols at chosen places, for the parts of jsmpeg_amd/csrc/slice_parse.h that exist on the device only (the 64-bit window over
the LDS ring, the refill and its hold-back, the token ring and its tail, the start phase).  Five sets, each a function that
returns dict(streams=[(name, desc)], claims={...}): `claims` says what the set holds; tests/test_parse_edges.py counts every
claim again over the descriptions and over the simulator's records, and states what the sets REACH in the walk (bits per
turn, head-room, ring occupancy, bit phases); tests/test_gpu_parse_edges.py decodes them on the device.

Everything is deterministic; nothing here includes or calls the code under test."""
import random

import craft_es as C
from craft_es import E

SMALL = (176, 144)              # 11 x 9 macroblocks
WIDE = (1136, 32)               # 71 x 2: room for two macroblock_escapes in a row, and for vectors of +-1024
TALL = (1136, 704)              # 71 x 44: room for the longest motion codes in both components (worst_turns)

ESC_RUNS = (0, 1, 31, 32, 62, 63)
ESC_LEVELS = (1, -1, 127, -127, 128, -128, 129, -129, 255, -255)
CODES = sorted(E.COEFF)         # (run, magnitude) of every DCT run/level code but (0, 1), which is "11s" / the first "1s"


def mbs_of(size):
    return ((size[0] + 15) >> 4) * ((size[1] + 15) >> 4)


def intra_flat(q=8):
    """an intra macroblock of DC differentials 0: the cheapest there is (30 bits)"""
    return (q, "intra", None, [(0, ())] * 6)


def intra_picture(size, q=8, seed=0):
    """a reference picture with some texture, so that a wrong vector shows"""
    rng = random.Random(seed)
    mbs = []
    mbw = (size[0] + 15) >> 4
    dc = [128, 128, 128]
    for mb in range(mbs_of(size)):
        if mb % mbw == 0:
            dc = [128, 128, 128]
        blocks = []
        for b in range(6):
            comp = 0 if b < 4 else b - 3
            d = rng.randint(-20, 20)
            if not 40 <= dc[comp] + d <= 215:
                d = -d
            dc[comp] += d
            blocks.append((d, (rng.choice((0, 3, -3, 5)), rng.choice((0, 0, 2, -2)))))
        mbs.append((q, "intra", None, blocks))
    return dict(type="I", mbs=mbs)


def nblock(n, sign=1):
    """a non-intra block of exactly n tokens: +-1 at scan positions 0 .. n - 1 (`1s`, then `11s` each: the shortest codes)"""
    return [sign if i % 3 else -sign for i in range(n)]


def iblock(n, diff=0, sign=1):
    """an intra block of exactly n tokens: the DC and n - 1 of +-1 at scan positions 1 .. n - 1"""
    return (diff, [sign if i % 3 else -sign for i in range(n - 1)])


def symbol_blocks(symbols, intra):
    """(run, level) symbols packed into as few blocks as hold them -> [levels] (non-intra: from scan position 0; intra: from 1)"""
    out, cur, pos = [], [], (1 if intra else 0)
    for run, lv in symbols:
        if pos + run > 63:
            out.append(cur)
            cur, pos = [], (1 if intra else 0)
        cur += [0] * run + [lv]
        pos += run + 1
    if cur:
        out.append(cur)
    return out


def pack_p(size, items, f_code=1, full_pel=0, slices=None, user_data=None, filler=None):
    """P pictures from a list of macroblock entries, in order; the last picture is filled up with `filler` (default: a coded
    macroblock of one coefficient)"""
    n = mbs_of(size)
    filler = filler or (8, "coded", None, [[2], None, None, None, None, None])
    pics = []
    for i in range(0, len(items), n):
        mbs = list(items[i:i + n])
        mbs += [filler] * (n - len(mbs))
        p = dict(type="P", f_code=f_code, full_pel=full_pel, mbs=mbs)
        p["slices"] = slices if slices is not None else [0]        # one slice over the whole picture: it runs over every row end
        if user_data is not None:
            p["user_data"] = user_data
        pics.append(p)
    return pics


# ----------------------------------------------------------------------------------------------------------------
# symbols()

def _dct_symbols():
    syms = [(0, 1), (0, -1)]
    for run, mag in CODES:
        syms += [(run, mag), (run, -mag)]
    return syms


def _intra_mbs(blocks, q=8):
    """intra macroblocks from AC level lists, six per macroblock, DC differentials 0"""
    out = []
    for i in range(0, len(blocks), 6):
        six = [(0, b) for b in blocks[i:i + 6]]
        six += [(0, ())] * (6 - len(six))
        out.append((q, "intra", None, six))
    return out


def _coded_mbs(blocks, q=8, esc=None):
    out = []
    for i in range(0, len(blocks), 6):
        six = list(blocks[i:i + 6])
        six += [None] * (6 - len(six))
        entry = (q, "coded", None, six)
        if esc:
            entry += (dict(esc={b: True for b in range(len(blocks[i:i + 6]))}),)
        out.append(entry)
    return out


DC_DIFFS = [0] + [d for s in range(1, 9) for d in ((1 << s) - 1, -((1 << s) - 1), 1 << (s - 1), -(1 << (s - 1)))]


def _dc_mbs(q=8):
    """intra macroblocks whose blocks walk DC_DIFFS in both tables: every dct_dc_size with its extreme differentials (each size's
    largest and smallest magnitude, both signs); a +d is followed by its -d within a component, so the DC stays near 128"""
    out = []
    for d in sorted({abs(x) for x in DC_DIFFS}):
        out.append((q, "intra", None, [(d, ()), (-d, ()), (d, ()), (-d, ()), (d, ()), (d, ())]))
        out.append((q, "intra", None, [(-d, ()), (d, ()), (-d, ()), (d, ()), (-d, ()), (-d, ())]))
    return out


def _types_and_patterns():
    """P macroblocks: all seven types, every coded block pattern 1 .. 63, quantiser changes to 1 and 31, and an intra macroblock
    with six non-zero DC differentials behind an intra, a non-intra and a skipped neighbour"""
    one = [3, 0, -1]
    dc6 = [(9, ()), (-5, (1,)), (7, ()), (-3, ()), (11, (2,)), (-13, ())]
    out = [(8, "coded", None, [one] + [None] * 5)]
    for cbp in range(1, 64):
        out.append((8, "coded_mv" if cbp % 3 == 0 else "coded", (0, 0) if cbp % 3 == 0 else None,
                    [list(one) if cbp & (0x20 >> b) else None for b in range(6)]))
    out += [
        (8, "mv", (0, 0), [None] * 6),                                   # 0x08
        (8, "coded", None, [one] + [None] * 5),                          # 0x02
        (8, "coded_mv", (0, 0), [None, one] + [None] * 4),               # 0x0A
        (8, "intra", None, dc6),                                         # 0x01, after a non-intra neighbour
        (8, "intra", None, dc6),                                         # ... after an intra one
        (1, "coded_mv", (0, 0), [one] + [None] * 5),                     # 0x1A, to quantiser scale 1
        (31, "coded", None, [one] + [None] * 5),                         # 0x12, to 31
        (1, "intra", None, dc6),                                         # 0x11, to 1
        (31, "intra", None, dc6),                                        # 0x11, to 31
        (31, "skip", None, None),
        (31, "intra", None, dc6),                                        # after a skipped neighbour
        (8, "coded", None, [one] + [None] * 5),
    ]
    return out


def _increment_pictures():
    """WIDE P pictures, each ONE slice over both rows: a coded macroblock after 0 .. 32 skipped ones (every increment code), after
    33, 65 (one escape), 66 and 98 (two in a row); macroblock_stuffing in front of some; and slices whose start code names an earlier
    row, so that their FIRST increment is large (the other path through the increment)"""
    n = mbs_of(WIDE)
    coded = (8, "coded", None, [[1, 2], None, None, None, None, None])
    skip = (8, "skip", None, None)
    incs = list(range(1, 34)) + [34, 66, 67, 99, 33, 35]
    pics, cur, k = [], [coded], 0
    for inc in incs:
        if len(cur) + inc > n:
            cur += [coded] * (n - len(cur))
            pics.append(dict(type="P", mbs=cur, slices=[0]))
            cur = [coded]
        mb = coded
        if k % 4 == 1:
            mb = coded + (dict(stuffing=1 + k % 3),)
        cur += [skip] * (inc - 1) + [mb]
        k += 1
    cur += [coded] * (n - len(cur))
    pics.append(dict(type="P", mbs=cur, slices=[0]))
    # first increments: slices at macroblocks 0 (stuffed), 5, 40 and 71 + 29, all named row 0 (increments 1, 6, 41 = escape + 8,
    # 101 = three escapes + 2), and one at 71 + 50 named row 1 (increment 51)
    mbs = [coded + (dict(stuffing=2),)] + [coded] * (n - 1)
    pics.append(dict(type="P", mbs=mbs, slices=[dict(start=0, extra=1), dict(start=5, row=0), dict(start=40, row=0, extra=3),
                                                dict(start=100, row=0), dict(start=121, row=1)]))
    return pics, incs


def motion_wanted(f_code):
    """the differentials to place: every motion code -16 .. 16 with residual bits all zero and all one (f_code 1 has none), and
    the two wraps: +16 f (code 16, residual all one) from any predictor p >= 0 lands on p - 16 f, and -16 f on a predictor of -1
    lands on 16 f - 1 -> [(pred or None, d)]"""
    r_size = f_code - 1
    f = 1 << r_size
    out = [(None, 0)]
    for code in range(1, 17):
        for r in sorted({0, f - 1}):
            d = ((code - 1) << r_size) + r + 1
            out += [(None, d), (None, -d)]
    out += [(-1, -16 * f)]
    return out


def motion_pictures(f_code, full_pel, seed=0):
    """WIDE P pictures that hold motion_wanted(f_code) as HORIZONTAL differentials (the vertical component, the same function of the
    parse, walks small values): macroblocks in raster order, each taking the first wanted differential whose vector stays inside
    the picture at that place, else a step of the predictor toward one that is wanted, else a coded macroblock without vector
    (the predictor's reset)"""
    mbw = WIDE[0] // 16
    cw, ch = WIDE
    span = 16 << (f_code - 1)
    sh = 1 if full_pel else 0
    wanted = motion_wanted(f_code)
    one = [2]
    reset = (8, "coded", None, [one] + [None] * 5)
    vseq = [0, 1, -1, 2, 0, -2, 3, -3] if not full_pel else [0, 1, -1, 0, 2, -2]
    pics, mbs, placed = [], [], []
    pmh = pmv = 0
    addr = 0
    guard = 0

    def wrap(v):
        return v + 2 * span if v < -span else (v - 2 * span if v >= span else v)

    def ok(col, row, h, v):
        return E.mv_ok(cw, ch, col, row, h << sh, v << sh)

    while wanted:
        guard += 1
        assert guard < 20000, (f_code, full_pel, wanted[:4])
        row, col = divmod(addr % (2 * mbw), mbw)
        if col == 0:
            pmh = pmv = 0                                                # a slice per row
        # vertical: the next small value that fits (row 0 may point down, row 1 up)
        v = next(x for x in vseq[len(mbs) % len(vseq):] + vseq if (x >= 0 if row == 0 else x <= 0))
        if abs(v - pmv) > span:
            v = pmv
        choice = None
        for i, (need, d) in enumerate(wanted):
            if need is not None and need != pmh:
                continue
            h = wrap(pmh + d)
            if ok(col, row, h, v):
                choice = (i, h)
                break
        last_of_row = col == mbw - 1
        if choice is not None:
            i, h = choice
            placed.append((pmh, wanted[i][1], h))
            opts = dict(mv_d=(wanted[i][1], None))
            del wanted[i]
            mbs.append((8, "coded_mv", (h, v), [one] + [None] * 5, opts) if last_of_row or len(mbs) % 5 == 0 else (8, "mv", (h, v), [None] * 6, opts))
            pmh, pmv = h, v
        else:
            needs = [need for need, _ in wanted if need is not None and need != pmh]
            step = None
            if needs and abs(needs[0] - pmh) <= span and ok(col, row, needs[0], v):
                step = needs[0]
            elif pmh != 0 and ok(col, row, 0, v) and abs(pmh) <= span:
                step = 0                                                 # back to 0, where every place takes some differential
            if step is not None:
                mbs.append((8, "coded_mv", (step, v), [one] + [None] * 5))
                pmh, pmv = step, v
            else:
                mbs.append(reset)
                pmh = pmv = 0
        addr += 1
        if len(mbs) == 2 * mbw:
            pics.append(dict(type="P", f_code=f_code, full_pel=full_pel, mbs=mbs))
            mbs = []
    if mbs:
        while len(mbs) < 2 * mbw:
            mbs.append(reset)
        pics.append(dict(type="P", f_code=f_code, full_pel=full_pel, mbs=mbs))
    return pics, placed


_cache = {}


def _cached(fn):
    def run():
        if fn.__name__ not in _cache:
            _cache[fn.__name__] = fn()
        return _cache[fn.__name__]
    run.__name__ = fn.__name__
    run.__doc__ = fn.__doc__
    return run


@_cached
def symbols():
    """every symbol of the slice layer at least once: three streams (small pictures: coefficients, types, patterns, DC; wide ones:
    increments; wide ones: motion)"""
    syms = _dct_symbols()
    # --- coefficients, DC, types, patterns: SMALL
    intra_blocks = symbol_blocks(syms, True) + [iblock(n)[1] for n in range(1, 65)]
    i_mbs = _intra_mbs(intra_blocks) + _dc_mbs()
    n = mbs_of(SMALL)
    i_pics = []
    for i in range(0, len(i_mbs), n):
        mbs = i_mbs[i:i + n]
        mbs += [intra_flat()] * (n - len(mbs))
        i_pics.append(dict(type="I", mbs=mbs))
    # quantiser scale changes inside an I picture: intra + quantiser (the second I type)
    i_pics[-1]["mbs"][-3] = (1, "intra", None, [(0, (1,))] * 6)
    i_pics[-1]["mbs"][-2] = (31, "intra", None, [(0, (1,))] * 6)
    i_pics[-1]["mbs"][-1] = (8, "intra", None, [(0, (1,))] * 6)
    p_items = _coded_mbs(symbol_blocks(syms, False)) + _coded_mbs([nblock(k) for k in range(1, 65)])
    esc_blocks = [[0] * run + [lv] for run in ESC_RUNS for lv in ESC_LEVELS]
    p_items += _coded_mbs(esc_blocks, esc=True)
    # the same escapes inside intra blocks (run 63 does not fit behind a DC)
    p_items += [(8, "intra", None, [(0, [0] * run + [lv]) for lv in ESC_LEVELS[j:j + 6]], dict(esc={b: True for b in range(6)}))
                for run in ESC_RUNS[:-1] for j in (0, 4)]
    p_items += _types_and_patterns()
    small = dict(width=SMALL[0], height=SMALL[1], pictures=i_pics + pack_p(SMALL, p_items))
    # --- increments: WIDE
    inc_pics, incs = _increment_pictures()
    wide = dict(width=WIDE[0], height=WIDE[1], pictures=[intra_picture(WIDE, seed=1)] + inc_pics)
    # --- motion: WIDE, a reference picture in front of every (f_code, full_pel)
    m_pics, placed = [], {}
    for full_pel in (0, 1):
        for f_code in range(1, 8):
            pics, got = motion_pictures(f_code, full_pel)
            m_pics += [intra_picture(WIDE, seed=2)] + pics
            placed[(f_code, full_pel)] = got
    motion = dict(width=WIDE[0], height=WIDE[1], pictures=m_pics)
    claims = dict(
        dct_codes=len(CODES) * 2 + 2, eob_after=list(range(1, 65)), esc_runs=list(ESC_RUNS), esc_levels=sorted(ESC_LEVELS),
        increments=sorted(set(incs)), stuffing=True, first_increments=[1, 6, 41, 51, 101],
        types_i=[0x01, 0x11], types_p=[0x01, 0x02, 0x08, 0x0A, 0x11, 0x12, 0x1A], patterns=list(range(1, 64)),
        motion={k: sorted({d for _, d, _ in v}) for k, v in placed.items()}, dc_sizes=list(range(9)), dc_diffs=sorted(set(DC_DIFFS)),
        quantisers=[1, 31], dc_after=["intra", "non-intra", "skipped"])
    return dict(streams=[("symbols_small", small), ("symbols_increments", wide), ("symbols_motion", motion)], claims=claims)


# ----------------------------------------------------------------------------------------------------------------
# phases()

def _rich_sequence():
    """one I and one P picture (SMALL) whose macroblocks mix every step kind: headers of every type, DCs of every size, pairs, long
    codes, escapes of both lengths, skipped runs, vectors"""
    rng = random.Random(0x9A5E)
    n = mbs_of(SMALL)
    mbw = SMALL[0] // 16

    def levels(intra):
        out = []
        for _ in range(rng.choice((1, 2, 3, 5, 8, 13))):
            out += [0] * rng.choice((0, 0, 0, 1, 2, 5)) + [rng.choice((1, -1, 1, -1, 2, -2, 3, 5, -7, 12, -19, 40, -41, 100, -130, 200, 255, -255))]
        return out[:63 if intra else 64]

    i_mbs, dc = [], [128, 128, 128]
    q = 8
    for mb in range(n):
        if mb % mbw == 0:
            dc = [128, 128, 128]
        blocks = []
        for b in range(6):
            comp = 0 if b < 4 else b - 3
            d = rng.choice((0, 1, -2, 3, -5, 9, -17, 33, -64, 100, -128, 255))
            if not 0 <= dc[comp] + d <= 400:
                d = -d if 0 <= dc[comp] - d <= 400 else 0
            dc[comp] += d
            blocks.append((d, levels(True) if rng.randrange(3) else ()))
        if rng.randrange(5) == 0:
            q = rng.choice((1, 2, 8, 31))
        i_mbs.append((q, "intra", None, blocks))
    p_mbs = []
    for mb in range(n):
        row, col = divmod(mb, mbw)
        edge = col in (0, mbw - 1)
        kind = rng.choice(("coded", "coded_mv", "mv", "intra", "skip", "skip", "coded_mv"))
        if edge and kind in ("skip", "mv"):
            kind = "coded_mv"
        if kind != "mv" and kind != "skip" and rng.randrange(4) == 0:
            q = rng.choice((1, 3, 8, 31))
        if mb % 9 == 4:                                                  # every row: a vector, a pattern and a new quantiser
            kind, q = "coded_mv", (31 if q != 31 else 2)
        mv = None
        if kind in ("coded_mv", "mv"):
            for _ in range(32):
                mv = (rng.randint(-30, 30), rng.randint(-30, 30))
                if E.mv_ok(SMALL[0], SMALL[1], col, row, mv[0], mv[1]):
                    break
            else:
                mv = (0, 0)
        if kind == "intra":
            p_mbs.append((q, kind, None, [(rng.choice((0, 4, -9, 30)), levels(True) if rng.randrange(2) else ()) for b in range(6)]))
        elif kind == "skip":
            p_mbs.append((q, "skip", None, None))
        elif kind == "mv":
            p_mbs.append((q, kind, mv, [None] * 6))
        else:
            blocks = [levels(False) if rng.randrange(2) else None for b in range(6)]
            if not any(b is not None for b in blocks):
                blocks[rng.randrange(6)] = levels(False)
            opts = dict(stuffing=1) if rng.randrange(9) == 0 else {}
            p_mbs.append((q, kind, mv, blocks, opts))
    return i_mbs, p_mbs


@_cached
def phases():
    """ONE macroblock sequence behind 0 .. 15 bytes of user data in front of the first picture: sixteen streams, in which every
    slice begins at every payload_off & 15 -- every chunk, row and wrap boundary of the ring passes over every part of the
    sequence.  Bit phases: the slices of a picture carry 0 .. 7 extra_information_slice bytes (9 bits each), which moves the
    slice's content through every bit offset of a byte"""
    i_mbs, p_mbs = _rich_sequence()
    mbh = SMALL[1] // 16
    mbw = SMALL[0] // 16
    streams = []
    for n in range(16):
        sl = [dict(start=r * mbw, extra=r % 8) for r in range(mbh)]
        pics = [dict(type="I", mbs=i_mbs, slices=sl, user_data=n),
                dict(type="P", f_code=2, mbs=p_mbs, slices=sl)]
        streams.append(("phases_%02d" % n, dict(width=SMALL[0], height=SMALL[1], pictures=pics)))
    return dict(streams=streams, claims=dict(user_data=list(range(16)), start_phases=list(range(16)), extra_bytes=list(range(8))))


# ----------------------------------------------------------------------------------------------------------------
# worst_turns()

WORST_D = 641          # |code| 11 with residual 0 at f_code 7: the shortest differential with an 11-bit code and 6 residual bits


def _longest_cbp():
    best = max(range(1, 64), key=lambda c: (len(E.INV["CBP"][c]), bin(c).count("1")))
    assert len(E.INV["CBP"][best]) == 9
    return best


def worst_mb_p(col, row, q, cbp):
    """the non-intra worst case at (col, row) of TALL, behind 21 skipped macroblocks (predictors 0): increment 22 (11 bits), type
    pattern + vector + quantiser (5 + 5), two 11-bit motion codes with 6 residual bits, a 9-bit pattern, and in every block a
    28-bit escape first and then (0, +-2) (0, +-1) end_of_block -- ten bits, one full pair look"""
    h = WORST_D if col <= 40 else -WORST_D
    v = WORST_D if row <= 21 else -WORST_D
    blocks = [[255 if (col + b) % 2 else -255, 2, -1] if cbp & (0x20 >> b) else None for b in range(6)]
    return (q, "coded_mv", (h, v), blocks)


def worst_mb_i(q):
    """the intra worst case: increment 22, type intra + quantiser (6 + 5), luma DCs of size 8 (15 bits; the chroma ones 16), and in
    every block a 28-bit escape and a full pair look"""
    ac = [-255, 2, -1]
    return (q, "intra", None, [(255, ac), (-255, ac), (255, ac), (-255, ac), (255, ac), (-255, ac)])


@_cached
def worst_turns():
    """TALL: one P picture that is ONE slice of worst-case macroblocks, each behind 21 skipped ones (alternately the non-intra and
    the intra form, the quantiser changing every time), and SMALL: the densest token producers (blocks of 64 tokens of 2 and 3
    bits) as an I and a P picture"""
    mbw = TALL[0] // 16
    n = mbs_of(TALL)
    cbp = _longest_cbp()
    mbs = []
    k = 0
    for addr in range(n):
        row, col = divmod(addr, mbw)
        if addr % 22 == 0 or addr == n - 1:
            q = 1 + (k * 7) % 31
            prev_q = mbs[-1][0] if mbs else q
            if q == prev_q:
                q = q % 31 + 1
            mbs.append(worst_mb_i(q) if k % 4 == 3 else worst_mb_p(col, row, q, cbp))
            k += 1
        else:
            mbs.append((mbs[-1][0], "skip", None, None))
    tall = dict(width=TALL[0], height=TALL[1], pictures=[dict(type="I", mbs=[intra_flat()] * n),
                                                         dict(type="P", f_code=7, full_pel=0, mbs=mbs, slices=[0])])
    # the first macroblock of the slice has increment 1 and the slice's quantiser: not a worst turn, by construction
    ns = mbs_of(SMALL)
    dense_i = [(8, "intra", None, [iblock(64, 0, 1 if (m + b) % 2 else -1) for b in range(6)]) for m in range(ns)]
    dense_p = [(8, "coded", None, [nblock(64, 1 if (m + b) % 2 else -1) for b in range(6)]) for m in range(ns)]
    dense = dict(width=SMALL[0], height=SMALL[1], pictures=[dict(type="I", mbs=dense_i), dict(type="P", mbs=dense_p)])
    claims = dict(worst_p=sum(1 for m in mbs[1:] if m[1] == "coded_mv"), worst_i=sum(1 for m in mbs[1:] if m[1] == "intra"),
                  cbp=cbp, dense_blocks=2 * 6 * ns, turn_bits_p=11 + 5 + 5 + 17 + 17 + 9 + 28 + 10, turn_bits_i=11 + 6 + 5 + 15 + 28 + 10)
    return dict(streams=[("worst_tall", tall), ("worst_dense", dense)], claims=claims)


# ----------------------------------------------------------------------------------------------------------------
# tails()

def _tail_slice_p(tokens):
    """macroblocks of a P slice (one SMALL row, 11 macroblocks) holding exactly `tokens` tokens; 0: vector-only and skipped ones"""
    mbw = SMALL[0] // 16
    if tokens == 0:
        row = [(8, "mv", (3, 0), [None] * 6)] + [(8, "skip", None, None)] * (mbw - 2) + [(8, "mv", (-8, 0), [None] * 6)]
        return row
    # spread over the macroblocks' first blocks, the rest in the last one
    counts = []
    left = tokens
    for i in range(mbw):
        c = min(left - (mbw - 1 - i), 1 + (i * 5 + tokens) % 7) if i < mbw - 1 else left
        c = max(1, c)
        counts.append(c)
        left -= c
    assert sum(counts) == tokens and all(c >= 1 for c in counts), (tokens, counts)
    row = []
    for c in counts:
        blocks = [None] * 6
        b = 0
        while c > 0:
            take = min(c, 64)
            blocks[b] = nblock(take)
            c -= take
            b += 1
        row.append((8, "coded", None, blocks))
    return row


@_cached
def tails():
    """the edges of a slice's end (SMALL): P slices of 0, 11 .. 58 tokens (every residue modulo 16; exactly 16 and 32), blocks of
    every token count 1 .. 64, slices of one macroblock (the shortest: 2 bytes), one slice of a row of escapes (14 KB); the written stream is measured for the rest (payload lengths modulo 16, slack bits, an end on a chunk boundary)"""
    mbw, mbh = SMALL[0] // 16, SMALL[1] // 16
    n = mbw * mbh
    totals = [0, 16, 32] + list(range(11, 11 + 48))
    rows = [_tail_slice_p(t) for t in totals]
    while len(rows) % mbh:
        rows.append(_tail_slice_p(0))
    pics = [intra_picture(SMALL, seed=3)]
    for i in range(0, len(rows), mbh):
        pics.append(dict(type="P", mbs=[m for r in rows[i:i + mbh] for m in r]))
    # blocks of every count: P macroblocks of one block each, a slice per macroblock in the first rows (the shortest slices)
    one_block = [(8, "coded", None, [nblock(k)] + [None] * 5) for k in range(1, 65)]
    one_block += [(8, "coded", None, [[1]] + [None] * 5)] * (n - len(one_block))
    one_block[n - mbw] = (8, "mv", (2, 0), [None] * 6)                    # the shortest legal slice: 6 bits of header, 9 of macroblock (at a row's start)
    pics.append(dict(type="P", mbs=one_block, slices=list(range(0, 2 * mbw)) + list(range(2 * mbw, n, mbw)) + [n - mbw + 1]))
    # intra slices whose totals step by one token (DC + k - 1): odd and even runs, every alignment
    im = []
    for r in range(mbh):
        for c in range(mbw):
            im.append((8, "intra", None, [iblock(1 + (r + b + c) % 5 if c else 1 + r) for b in range(6)]))
    pics.append(dict(type="I", mbs=im))
    # several kilobytes in one slice: every coefficient a 28-bit escape, the picture one slice
    big = [(31, "coded", None, [[255 if (m + i) % 2 else -255 for i in range(64)] for b in range(6)]) for m in range(mbw)]
    big += [(31, "coded", None, [[1]] + [None] * 5)] * (n - mbw)
    pics.append(dict(type="P", mbs=big))
    desc = dict(width=SMALL[0], height=SMALL[1], pictures=pics)
    claims = dict(slice_tokens=sorted(totals), token_residues=list(range(16)), slot_residues=list(range(0, 16, 2)),
                  block_counts=list(range(1, 65)), payload_residues=list(range(16)), slack_bits=list(range(8)),
                  ends_on_chunk=True, shortest_bytes=2, longest_bytes_at_least=4096)
    return dict(streams=[("tails", desc)], claims=claims)


# ----------------------------------------------------------------------------------------------------------------
# company()

@_cached
def company():
    """two streams of one picture size whose slices differ as much as slices can: `headers` (P pictures of short slices -- a slice
    per one or two macroblocks, vectors, skipped runs, hardly a coefficient) and `coefficients` (one long slice per row, every
    block full of long codes and escapes): in one batch they share wavefronts"""
    mbw, mbh = SMALL[0] // 16, SMALL[1] // 16
    n = mbw * mbh
    rng = random.Random(0xC0)
    hp = []
    for t in range(3):
        mbs, starts = [], []
        for mb in range(n):
            new = mb % mbw == 0 or rng.randrange(2) == 0
            if new:
                starts.append(mb)
            kind = rng.choice(("mv", "coded_mv", "skip", "coded"))
            mbs.append(kind)
        # a slice begins and ends with a coded macroblock
        out = []
        for mb in range(n):
            row, col = divmod(mb, mbw)
            kind = mbs[mb]
            last = mb + 1 == n or (mb + 1) in starts
            if kind == "skip" and (mb in starts or last):
                kind = "coded"
            if kind == "mv" and last:
                kind = "coded_mv"                                      # (a slice's last macroblock is longer than 8 bits)
            mv = None
            if kind in ("mv", "coded_mv"):
                for _ in range(32):
                    mv = (rng.randint(-15, 15), rng.randint(-15, 15))
                    if E.mv_ok(SMALL[0], SMALL[1], col, row, mv[0], mv[1]):
                        break
                else:
                    mv = (0, 0)
            if kind == "skip":
                out.append((8, "skip", None, None))
            elif kind == "mv":
                out.append((8, "mv", mv, [None] * 6))
            else:
                out.append((8, kind, mv, [[rng.choice((1, -1, 2))]] + [None] * 5))
        hp.append(dict(type="P", mbs=out, slices=starts))
    headers = dict(width=SMALL[0], height=SMALL[1], pictures=[intra_picture(SMALL, seed=4)] + hp)

    def heavy(intra):
        out = []
        for _ in range(20):
            out += [0] * rng.choice((0, 0, 1, 3)) + [rng.choice((1, -2, 7, -19, 40, -100, 129, -255, 3, -1))]
        return out[:63 if intra else 64]
    ci = [(8, "intra", None, [(0, heavy(True)) for b in range(6)]) for _ in range(n)]
    cp = [(8, "coded", None, [heavy(False) for b in range(6)]) for _ in range(n)]
    coefficients = dict(width=SMALL[0], height=SMALL[1], pictures=[dict(type="I", mbs=ci), dict(type="P", mbs=cp),
                                                                    dict(type="P", mbs=cp), dict(type="P", mbs=cp)])
    return dict(streams=[("company_headers", headers), ("company_coefficients", coefficients)],
                claims=dict(pictures=[4, 4], size=SMALL))


SETS = (symbols, phases, worst_turns, tails, company)

_written = {}


def written(name_desc):
    """(name, desc) -> dict(name, desc, es, offsets), written once"""
    name, desc = name_desc
    if name not in _written:
        es, offs = C.write_stream(desc)
        _written[name] = dict(name=name, desc=desc, es=es, offsets=offs)
    return _written[name]


def all_streams():
    return [written(s) for fn in SETS for s in fn()["streams"]]
