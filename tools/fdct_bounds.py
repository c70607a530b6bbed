"""The forward DCT of the intra encoder (jsmpeg_amd/csrc/enc_block.h) in integers: the largest magnitudes its two passes can
reach, added up from the header's own cosine table the way tools/idct_bounds.py does for the inverse.  No GPU.

    t[y][v] = sum_n C[v][n] x[y][n],  x in 0 .. 255         |t| <= 255 * max_v sum_n |C[v][n]|
    a[u][v] = sum_y C[u][y] t[y][v]                         |a| <= max_u sum_y |C[u][y]| * max |t|

    python tools/fdct_bounds.py [--signed]

--signed: the residual of a predicted block (jsmpeg_amd/csrc/enc_motion.h), x in -255 .. 255: the bounds are sums of |C| * 255
and so the same; what changes is the value reached (every term can take its sign) and the range of the 24-bit multiplications'
operands, printed as well.
"""
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def table():
    text = open(os.path.join(ROOT, "jsmpeg_amd", "csrc", "enc_block.h")).read()
    body = text[text.index("JmEncConst c = {"):text.index("MPEG1_DEFAULT_INTRA_QUANT_INIT, {}")]
    return np.array([int(v) for v in re.findall(r"-?\d+", body)], dtype=np.int64).reshape(8, 8)


if __name__ == "__main__":
    C = table()
    signed = "--signed" in sys.argv[1:]
    rows = np.abs(C).sum(axis=1)
    # the true maximum of each pass: pixels 255 where the cosine is positive, 0 elsewhere (and the other way round)
    t_max = int(max(255 * np.maximum(C, 0).sum(axis=1).max(), 255 * np.maximum(-C, 0).sum(axis=1).max()))
    if signed:
        t_max = int(255 * rows.max())                    # x = 255 * sign(C): the bound itself is reached
    t_bound = int(255 * rows.max())
    a_bound = int(rows.max() * t_bound)
    print("largest row sum of |C|: %d" % rows.max())
    print("|t| <= %d (reached: %d) < 2^24 = %d: %s" % (t_bound, t_max, 1 << 24, t_bound < 1 << 24))
    print("|a| <= %d < 2^39 = %d: %s; + 2^24 for the rounding still below 2^63" % (a_bound, 1 << 39, a_bound < 1 << 39))
    if signed:
        th, tl = (t_bound >> 12) + 1, 4095
        print("x in -255 .. 255 (9 bits signed), C in 16 bits signed, th = t >> 12 in +-%d, tl = t & 4095 in 0 .. %d: all within 24 bits signed" % (th, tl))
        print("Sh = sum C th: |Sh| <= %d, Sl = sum C tl: |Sl| <= %d, both < 2^28 = %d: %s" % (rows.max() * th, rows.max() * tl, 1 << 28, rows.max() * max(th, tl) < 1 << 28))
        print("non-intra level: (|c8| >> 4) / q <= %d < 2^31 / 31: the reciprocal of jm_encp_recip is exact" % (((a_bound + (1 << 24)) >> 25) >> 4))
    print("largest |c8| = (|a| + 2^24) >> 25 <= %d: fits int32, 2 |c8| + q W fits uint32" % ((a_bound + (1 << 24)) >> 25))
