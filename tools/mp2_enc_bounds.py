#!/usr/bin/env python3
"""Adds up the bounds of the MP2 encoder's integer analysis filterbank (jsmpeg_amd/csrc/mp2_enc.h), as tools/fdct_bounds.py
does for the video transform: how wide Y, the accumulator and S can get, and how far S can lie from the real-valued filterbank
with the same window.  Everything here follows from the committed window integers, |x| <= 32767 and the rounding of the
cosine table; nothing is measured.  tests/test_mp2_enc_sim.py holds the code to these figures.

    python tools/mp2_enc_bounds.py
"""
import json
import math
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def window_half():
    text = open(os.path.join(ROOT, "jsmpeg_amd", "csrc", "mp2_window.h")).read()
    body = text[text.index("MP2_WINDOW_HALF_X2[257]"):]
    return [int(v) for v in re.findall(r"-?\d+", body[body.index("{") + 1:body.index("}")])]


def bounds():
    half = window_half()
    w = [abs(half[i if i <= 256 else 512 - i]) for i in range(512)]
    x_max = 32767
    tap_sum = max(sum(w[i + 64 * j] for j in range(8)) for i in range(64))      # largest sum_j |W[i + 64 j]|
    w_sum = sum(w)
    y_max = tap_sum * x_max
    cos_q = [int(math.floor(32768.0 * math.cos(m * math.pi / 64.0) + 0.5)) for m in range(128)]
    cos_err = max(abs(cos_q[m] - 32768.0 * math.cos(m * math.pi / 64.0)) for m in range(128))
    acc_max = 32768 * x_max * w_sum                                               # sum_i |COS| |Y_i| <= 2^15 * 32767 * sum |W|
    s_max = (acc_max + (1 << 27)) >> 28
    # S against the real filterbank, in units of S: the cosines' rounding times sum_i |Y_i|, plus the final shift's half unit
    s_err = cos_err * x_max * w_sum / float(1 << 28) + 0.5
    return dict(window_tap_sum=tap_sum, window_sum=w_sum, y_max=y_max, y_bits=y_max.bit_length() + 1, acc_max=acc_max,
                acc_below_2_53=acc_max < (1 << 53), s_max=s_max, s_below_2_25=s_max < (1 << 25), cos_rounding=cos_err,
                s_error_units=s_err, s_error_of_full_scale=s_err / float(1 << 23),
                # the kernel's split: Z = Y + Y (folded, 34 bits) in a low half of 16 bits and the rest; 32 terms per half
                z_max=2 * y_max, z_bits=(2 * y_max).bit_length() + 1, z_hi_max=((2 * y_max) >> 16) + 1,
                half_sum_max=32 * 32768 * (((2 * y_max) >> 16) + 1))


if __name__ == "__main__":
    print(json.dumps(bounds(), indent=1))
