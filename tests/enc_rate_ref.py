"""TEST INFRASTRUCTURE ONLY -- rule RATE of jsmpeg_amd/csrc/enc_rate.h restated by brute force, beside tests/enc_p_ref.py: every
picture is coded at every scale of the range through enc_p_ref.code_picture / picture_bytes, against the reconstruction of the
picture before as chosen, and the smallest scale whose picture fits the budget is taken.  The whole call is then
enc_p_ref.encode with the chosen scales.  Nothing here includes or calls the code under test.

code_picture is a pure function of its arguments, and the tests run the same pictures under many targets: its results, and
the motion search inside it (which does not depend on the scale), are kept by the bytes of their arguments."""
import enc_p_ref
from enc_ref import coded

_search, _coded = {}, {}
_plain_search = enc_p_ref.search


def _kept_search(cur, ref, cw, ch, R):
    key = (cur.tobytes(), ref.tobytes(), cw, ch, R)
    if key not in _search:
        if len(_search) > 4096:
            _search.clear()
        _search[key] = _plain_search(cur, ref, cw, ch, R)
    sad, mvh, mvv = _search[key]
    return sad.copy(), mvh.copy(), mvv.copy()


def picture_at(frame, ref, width, height, q, R, ordinal, gop, frame_rate_code):
    """(reconstruction, bytes) of one picture coded at q"""
    cw, ch = coded(width, height)
    p_picture = ordinal % gop != 0
    key = (frame.tobytes(), ref.tobytes() if p_picture else None, width, height, q, R, p_picture)
    if key not in _coded:
        if len(_coded) > 65536:
            _coded.clear()
        enc_p_ref.search = _kept_search
        try:
            pic = enc_p_ref.code_picture(frame, ref if p_picture else None, cw, ch, q, R, p_picture)
        finally:
            enc_p_ref.search = _plain_search
        _coded[key] = (pic.recon, len(enc_p_ref.picture_bytes(pic, width, height, q, frame_rate_code, ordinal, gop, R)))
    return _coded[key]


def gops(streams, gop):
    """per picture of a call: (level in its GOP, pictures of its GOP in the call)"""
    n = len(streams)
    ordinal = [0] * n
    for k in range(1, n):
        ordinal[k] = ordinal[k - 1] + 1 if streams[k] == streams[k - 1] else 0
    out = [None] * n
    length = 0
    for k in reversed(range(n)):
        if k + 1 == n or streams[k + 1] != streams[k]:
            length = ordinal[k] + 1
        first = ordinal[k] - ordinal[k] % gop
        out[k] = (ordinal[k] % gop, min(gop, length - first), ordinal[k])
    return out


def budget(T, m, level, W, spent):
    left = max(0, m * T - spent)
    w, S = (W, W + m - 1) if level == 0 else (1, m - level)
    return left * w // S


class Rate:
    """q, budget, bytes: per picture what the rule chose; table: per picture {q: bytes} over the whole range"""


def choose(frames, width, height, gop, search_range, T, q_min=1, q_max=31, W=4, streams=None, frame_rate_code=5):
    n = len(frames)
    streams = [0] * n if streams is None else [int(s) for s in streams]
    r = Rate()
    r.q, r.budget, r.bytes, r.table = [], [], [], []
    recon = []
    for k, (level, m, ordinal) in enumerate(gops(streams, gop)):
        b = budget(T, m, level, W, sum(r.bytes[k - level:k]))
        at = {q: picture_at(frames[k], recon[k - 1] if level else None, width, height, q, search_range, ordinal, gop, frame_rate_code)
              for q in range(q_min, q_max + 1)}
        fits = [q for q in range(q_min, q_max + 1) if at[q][1] <= b]
        q = fits[0] if fits else q_max
        r.q.append(q); r.budget.append(b); r.bytes.append(at[q][1]); r.table.append({v: at[v][1] for v in at})
        recon.append(at[q][0])
    return r


def encode(frames, width, height, gop, search_range, T, q_min=1, q_max=31, W=4, streams=None, frame_rate_code=5, end=True):
    """enc_p_ref.encode's Result of the call at the chosen scales, the choice in .rate"""
    rate = choose(frames, width, height, gop, search_range, T, q_min, q_max, W, streams, frame_rate_code)
    out = enc_p_ref.encode(frames, width, height, gop, search_range, streams=streams, qscale=rate.q, frame_rate_code=frame_rate_code, end=end)
    out.rate = rate
    return out
