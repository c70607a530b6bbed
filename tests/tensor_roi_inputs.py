"""The box lists of the region-of-interest tests, once for both suites: tests/test_tensor_roi_plan.py runs them through the
CPU simulator against tensor_ref.reference, tests/test_gpu_tensor_roi.py through k_tensor_roi -- so a GPU failure cannot be
the reference disagreeing with itself.  Also the clip rule (include/jsmpeg_hip.h, jsmpeg_hip_roi_t) restated in Python."""

I32_MAX, I32_MIN = (1 << 31) - 1, -(1 << 31)
EMPTY, INSIDE, CLIPPED = 0, 1, 2

W, H = 352, 288                        # the display size of the fixture the lists are made for (coherent_pan_352x288)
SIZES = ((20, 70), (48, 64))           # (height, width): partial tiles in both directions; one tile wide, three high
U8_CHECK_SIZE = (48, 64)               # tensor_ref.check's u8 rule allows 0.1 % of a row off by one: held to it only from here up


def clip(roi, count, w, h):
    """(status, (x, y, width, height) of the clipped box or None).  Python integers: no width to overflow."""
    row, x, y, bw, bh = (int(v) for v in roi)
    if row < 0 or row >= count or bw <= 0 or bh <= 0:
        return EMPTY, None
    x0, y0, x1, y1 = max(x, 0), max(y, 0), min(x + bw, w), min(y + bh, h)
    if x1 <= x0 or y1 <= y0:
        return EMPTY, None
    box = (x0, y0, x1 - x0, y1 - y0)
    return (INSIDE if box == (x, y, bw, bh) else CLIPPED), box


# (x, y, width, height) inside 352 x 288
BOXES12 = (
    (100, 50, 1, 1),                   # one pixel
    (0, 0, W, H),                      # the whole picture
    (33, 21, 121, 91),                 # odd x and odd y: chroma parity
    (15, 41, 2, 101),                  # straddles a 16-pixel span
    (249, 97, 103, 83),                # flush with the right edge
    (43, 205, 147, 83),                # flush with the bottom edge
    (299, 235, 53, 53),                # flush with both
    (21, 131, 301, 7),                 # slivers
    (171, 11, 7, 251),
    (17, 9, 64, 48),                   # the size of one output and of the other: an identity axis is a copy
    (101, 37, 70, 20),
    (64, 32, 130, 99),                 # a 16-aligned origin
)
# The u8 rows are held to tensor_ref.check at 64 x 48, whose cap is 9 values of a row off by one.  A u8 value can differ from
# torch's only where the exact result is a tie (x.5) that the two fp32 sums round apart.  The fixture is synthetic, with
# sharp edges and flat areas, and there a tie is no accident: a neighbourhood of two values a, a + 1 sums to a + (the weight
# on the a + 1 side), a tie wherever a filter window is centred on the edge.  With dyadic weights (plain 2 : 1, the whole
# picture's 5.5 : 1 and 6 : 1 in plain mode) such a sum is exact in fp32 and both round it alike; with the normalised
# weights of other ratios it is not.  So the boxes have odd sides that share no small factor with 64 and 48 (121 x 91,
# 103 x 83, 147 x 83, 53 x 53, 301 x 7, 7 x 251, 130 x 99): few windows are centred on a pixel boundary.  Measured on
# the reference alone (torch on the fixture's pictures, values within 2e-4 of x.5, worst of the pictures used): 120 x 90
# has 64 such values, 100 x 80 has 121, 128 x 96 has 487; 121 x 91 has 18, 103 x 83 has 9, 147 x 83 has 14.  The 1- and
# 2-wide boxes repeat one source value over up to 64 output columns, a tie with it: they go to pictures where the
# reference has none in those columns.

# test 1: the 12 boxes spread over three pictures, with repeats, in reverse order
MIXED_PICTURES = (7, 2, 11)
MIXED = tuple(reversed([(i % 3,) + b for i, b in enumerate(BOXES12)] +
                       [(2,) + BOXES12[1], (0,) + BOXES12[3], (0,) + BOXES12[3], (1,) + BOXES12[10]]))

# test 4: bad boxes beside good ones, over three pictures; the expected status follows from clip()
BAD = (
    (0, 33, 21, 121, 91),                                   # good
    (1, -10, 50, 100, 60),                                  # overhangs the left side,
    (2, 50, -7, 100, 60),                                   # the top,
    (0, 300, 50, 100, 60),                                  # the right,
    (1, 50, 250, 100, 60),                                  # the bottom,
    (2, -5, -5, 400, 300),                                  # every side
    (1, 64, 32, 130, 99),                                   # good
    (0, -100, 50, 100, 60),                                 # outside: left (its end is column 0),
    (0, W, 50, 10, 10),                                     # right,
    (1, 50, -60, 100, 60),                                  # above,
    (2, 50, H, 10, 10),                                     # below
    (0, 10, 10, 0, 10), (0, 10, 10, 10, 0),                 # size 0
    (1, 10, 10, -5, 10), (1, 10, 10, 10, -1), (2, 10, 10, I32_MIN, I32_MIN),      # negative size
    (2, 17, 9, 64, 48),                                     # good
    (-1, 0, 0, 64, 48), (3, 0, 0, 64, 48), (I32_MIN, 0, 0, 64, 48), (I32_MAX, 0, 0, 64, 48),      # row out of range
    (0, I32_MAX, I32_MAX, I32_MAX, I32_MAX),                # the INT32 extremes: far outside,
    (1, I32_MIN, I32_MIN, I32_MAX, I32_MAX),                # ends at -1: outside
    (2, -1, -1, I32_MAX, I32_MAX),                          # covers the picture: clipped to all of it
    (0, 0, 0, I32_MAX, I32_MAX),
    (1, I32_MIN, 100, I32_MAX, 50),                         # ends at column -1
    (2, -I32_MAX, 100, I32_MAX, 50),                        # ends at column 0: outside
    (1, -I32_MAX + 1, 100, I32_MAX, 50),                    # ends at column 1: one column wide
    (0, 101, 37, 70, 20),                                   # good
)
BAD_PICTURES = (5, 0, 7)

# test 5: 16 boxes that 65539 rows cycle through, 8 x 8 u8
CYCLE16 = tuple((i % 3,) + b for i, b in enumerate(BOXES12)) + (
    (0, 3, 5, 8, 8), (1, 200, 100, 16, 16), (2, 11, 13, 99, 77), (0, 340, 276, 12, 12))
CYCLE_PICTURES = (1, 4, 8)
CYCLE_ROWS = 65539
CYCLE_SIZE = (8, 8)

# test 3: many taps, narrow chunks.  (fixture, box, (height, width))
MANY_TAPS = {
    "352x288_to_3x2": ("coherent_pan_352x288", (0, 0, 352, 288), (2, 3)),
    "1080p_to_7x1": ("cfg2_1080p", (0, 0, 1920, 1080), (7, 1)),                # 1920 -> 1: 1920 taps, chunks of 4 source rows
    "crop_up_to_4096_wide": ("cfg2_1080p", (333, 101, 64, 17), (40, 4096)),
}
