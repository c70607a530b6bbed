"""Nothing the encoder emits has moved: tests/golden/enc_pass_pin.json holds an md5 per call of the CPU simulator -- output
buffer, ranges, reconstructions, vectors, counts by kind, rate triples, ordinals -- written by tests/golden/make_enc_pass_pin.py
from the simulators as they were BEFORE the kernels and the simulator came to share their lane bodies (enc_pass.h).  Since then
"GPU == simulator" alone no longer shows that neither moved; this does.  Every entry is recomputed here with the writer's own
functions, which use nothing but the helpers' public calls."""
import importlib.util
import json
import os

import pytest

import enc_chain_inputs as ec
import enc_inputs as ei

_spec = importlib.util.spec_from_file_location("make_enc_pass_pin", os.path.join(ei.ROOT, "tests", "golden", "make_enc_pass_pin.py"))
pin = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(pin)


@pytest.fixture(scope="module")
def pinned():
    with open(pin.PIN) as f:
        return json.load(f)


def test_the_pin_holds_exactly_the_listed_calls(pinned):
    """an entry cannot be dropped quietly: the names are spelled out here, not taken from the file or from the cases"""
    small = ("enc_pan_176x144", "enc_wide_search_208x160", "content_176x144", "content_177x145", "flat", "stripes", "one_macroblock")
    want = {"intra/%s/q%d" % (n, q) for n in small for q in (1, 8, 31)}
    want |= {"intra/streams_176x144/end%d/rate_code%d" % (e, c) for e in (0, 1) for c in (3, 5)}
    p_names = ("content_176x144", "content_177x145", "enc_pan_176x144", "whole_pel_pan", "half_pel_pan", "flat_grey", "flat_wide", "one_macroblock",
               "scene_cut", "noise")
    want |= {"p/%s/%s/q%d" % (n, c, q) for n in p_names for c in ("gop3_R7", "gop4_R0") for q in (1, 8)}
    ranged = ("noise", "whole_pel_pan", "half_pel_pan", "content_177x145", "one_macroblock", "fast_pan", "checker_ties", "intra_threshold")
    want |= {"p/range/%s/R%d" % (n, R) for n in ranged for R in (0, 15)}
    want |= {"p/long_call/gop7_R1/end0", "p/long_call/gop7_R1/end1"}
    rated = ("pan_gop3_T150", "pan_gop4_T100", "pan_T20", "pan_T1500", "pan_gop1", "noise_T1500", "noise_T4000", "flat_grey", "flat_wide",
             "content_177x145", "content_177x145_R0", "one_macroblock", "range_4_16", "range_8_8", "streams_W1", "streams_W16")
    want |= {"rate/%s" % n for n in rated} | {"rate/long_call"}
    cuts = ["-".join(map(str, c)) for c in ec.splits(7)]
    assert len(set(cuts)) == 64
    want |= {"chain/pan7/%s/%s/cuts_%s" % (c, r, s) for c in ("gop3_R7", "gop4_R0") for r in ("no_rule", "T150") for s in cuts}
    want |= {"chain/streams_come_and_go", "chain/unchained_between_chained"}
    assert len(want) == 21 + 4 + 40 + 16 + 2 + 17 + 256 + 2
    assert set(pinned) == want
    assert set(pin.names()) == want


@pytest.mark.parametrize("group", pin.GROUPS)
def test_every_pinned_call_is_what_it_was(libs, pinned, group):
    got = pin.entries(libs, group)
    assert got, group
    assert set(got) == {n for n in pinned if n.startswith(group + "/")}
    moved = sorted(n for n in got if got[n] != pinned[n])
    assert not moved, moved
