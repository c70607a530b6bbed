"""The edges of k_enc_scale on the device (jsmpeg_amd/csrc/encode.hip; the rule: enc_scale.h): the named inputs of
tests/enc_scale_inputs.py -- EDGES (each reaches the tile, chunk or stride edge it is named for: tests/test_enc_scale_edges.py
proves that from the simulator's tile walker), CROPS, TINY, RATIOS (the weights' second form) -- the first geometries of the
seeded sweep and a mosaic cell at the largest ratios.  The planes in the handle's frame store equal the numpy restatement's
(tests/enc_scale_ref.py) and the CPU simulator's (tests/sim/sim_encode_scale.cpp) bit for bit: integers, no tolerance.
Nothing is asserted about time."""
import numpy as np
import pytest

import enc_inputs as ei
import enc_mosaic_inputs as mi
import enc_mosaic_ref as em
import enc_scale_inputs as si
import enc_scale_ref as es
from test_gpu_encode_mosaic import Device, cells_of
from test_gpu_encode_scale import capacity, on_device, result_of, source_bytes, torch  # noqa: F401  (torch: the fixture)

pytestmark = pytest.mark.gpu

SWEEP = 60          # the first geometries of si.sweep(), an encoder each (profiles/enc_scale_edges_notes.md has the time)


def planes_of(frame, ow, oh):
    """(luma, Cr, Cb) of the coded size and the scaled size of each: [(plane, pw, ph)]"""
    y, cr, cb = es.source_planes(frame, ow, oh)
    return [(y, ow, oh), (cr, (ow + 1) >> 1, (oh + 1) >> 1), (cb, (ow + 1) >> 1, (oh + 1) >> 1)]


def assert_both(got, frame, geo, want, what):
    w, h, crop, ow, oh, aa = geo
    assert np.array_equal(got, want), (what, int(np.count_nonzero(got != want)))
    assert np.array_equal(got, si.sim_frame(frame, w, h, ow, oh, crop, aa)), what


@pytest.mark.parametrize("name", sorted(si.EDGES))
def test_edges(torch, hip_lib, name):
    """two pictures from different frames on two streams; then the pointers swapped: the planes swap (the picture index is not
    mixed into the tile index)"""
    from jsmpeg_amd import encode
    geo = si.EDGES[name]
    w, h, crop, ow, oh, aa = geo
    frames, want = si.geometry_frames(w, h), si.geometry_want(geo)
    with encode.Encoder(ow, oh, 2, 2, capacity(want)) as enc:
        t, ptrs = on_device(torch, frames)
        enc.encode_scaled(ptrs, (w, h), crop, bool(aa), streams=[0, 1], qscale=5)
        for k in range(2):
            assert_both(source_bytes(enc, k), frames[k], geo, want[k], (name, k))
        enc.encode_scaled(ptrs[::-1], (w, h), crop, bool(aa), streams=[0, 1], qscale=5)
        assert np.array_equal(source_bytes(enc, 0), want[1]) and np.array_equal(source_bytes(enc, 1), want[0]), name
        assert not np.array_equal(want[0], want[1])


def test_crops_on_one_handle(torch, hip_lib):
    """every crop with both antialias values in turn on one encoder, then the first again: the descriptor differs from call to
    call, so each call has to replace the kept table -- a stale one shows as planes of the geometry before"""
    from jsmpeg_amd import encode
    (w, h), (ow, oh) = si.CROP_SOURCE, si.CROP_OUT
    frames = si.geometry_frames(w, h)
    geos = [(w, h, c, ow, oh, aa) for c in si.CROPS for aa in (1, 0)]
    geos.append(geos[0])
    with encode.Encoder(ow, oh, 2, 2, capacity(si.geometry_want(geos[0]))) as enc:
        t, ptrs = on_device(torch, frames)
        last, changed = None, 0
        for n, geo in enumerate(geos):
            want = si.geometry_want(geo)
            enc.encode_scaled(ptrs, (w, h), geo[2], bool(geo[5]), streams=[0, 1], qscale=5)
            for k in range(2):
                assert_both(source_bytes(enc, k), frames[k], geo, want[k], (n, geo, k))
            changed += last is not None and not np.array_equal(want[0], last)
            last = want[0]
        # (antialias changes nothing where both axes of a crop are enlarged: the 1 x 1 and the 2 x 2 crop)
        assert changed >= len(geos) - 3, "the call before left other planes nearly every time"
        # the same geometry twice in a row: the table is kept, the planes are the same
        enc.encode_scaled(ptrs[::-1], (w, h), geos[0][2], True, streams=[0, 1], qscale=5)
        assert np.array_equal(source_bytes(enc, 0), si.geometry_want(geos[0])[1])


@pytest.mark.parametrize("size", si.TINY, ids=["%dx%d" % s for s in si.TINY])
def test_tiny_outputs(torch, hip_lib, size):
    """outputs 1 and 2 across: beyond the scaled samples the coded plane is their replication -- for 1 x 1 the whole plane is
    one sample, and the stream is the intra pass's over that frame"""
    from jsmpeg_amd import encode
    (w, h), (ow, oh) = si.TINY_SOURCE, size
    frames = si.geometry_frames(w, h)
    with encode.Encoder(ow, oh, 2, 2, 1 << 16) as enc:
        t, ptrs = on_device(torch, frames)
        for aa in (1, 0):
            geo = (w, h, None, ow, oh, aa)
            want = si.geometry_want(geo)
            enc.encode_scaled(ptrs, (w, h), None, bool(aa), streams=[0, 1], qscale=5)
            for k in range(2):
                got = source_bytes(enc, k)
                assert_both(got, frames[k], geo, want[k], (size, aa, k))
                for p, pw, ph in planes_of(got, ow, oh):
                    assert np.array_equal(p, np.pad(p[:ph, :pw], ((0, p.shape[0] - ph), (0, p.shape[1] - pw)), mode="edge")), (size, aa, k)
                    if (ow, oh) == (1, 1):
                        assert p.shape in ((16, 16), (8, 8)) and np.all(p == p[0, 0])
            if (ow, oh) == (1, 1):
                assert result_of(enc, [0, 1]) == ei.sim_encode(want, 1, 1, streams=[0, 1], qscale=5)


@pytest.mark.parametrize("name", sorted(si.RATIOS))
def test_ratios(torch, hip_lib, name):
    """the ratios at which the first form of the weights left a tap below 0, which the 16-bit table stored as a weight near
    65 500: on the second form the device's planes are the simulator's and the restatement's"""
    from jsmpeg_amd import encode
    geo = si.RATIOS[name]
    w, h, crop, ow, oh, aa = geo
    frames, want = si.geometry_frames(w, h), si.geometry_want(geo)
    with encode.Encoder(ow, oh, 2, 2, 1 << 16) as enc:
        t, ptrs = on_device(torch, frames)
        enc.encode_scaled(ptrs, (w, h), crop, bool(aa), streams=[0, 1], qscale=5)
        for k in range(2):
            assert_both(source_bytes(enc, k), frames[k], geo, want[k], (name, k))


def test_sweep(torch, hip_lib):
    """the first SWEEP geometries of the CPU suite's seeded sweep, each on an encoder of its own"""
    from jsmpeg_amd import encode
    geos = si.sweep()[:SWEEP]
    assert len(geos) == SWEEP
    for n, geo in enumerate(geos):
        w, h, crop, ow, oh, aa = geo
        f = ei.noise_frame(w, h, seed=n)
        with encode.Encoder(ow, oh, 1, 1, 1 << 17) as enc:
            t, ptrs = on_device(torch, [f])
            enc.encode_scaled(ptrs, (w, h), crop, bool(aa), qscale=5)
            assert_both(source_bytes(enc, 0), f, geo, es.scale_frame(f, w, h, ow, oh, crop, bool(aa)), (n, geo))


def test_mosaic_cells_of_the_largest_ratios(torch, hip_lib):
    """k_enc_mosaic reads the same table: cells 1 and 2 pixels wide at even x from sources 3120 and 3418 wide (the CPU half:
    tests/test_enc_mosaic_sim.py)"""
    from jsmpeg_amd import encode
    w, h, fill, cells, _ = mi.RATIO_LAYOUT
    frames = mi.ratio_layout_frames()
    want = [em.compose(cells, fr, w, h, fill) for fr in frames]
    dev = Device(torch)
    with encode.Encoder(w, h, 2, 2, capacity(want)) as enc:
        enc.set_mosaic(cells_of(cells), fill)
        enc.encode_mosaic(dev.pictures(frames), streams=[0, 1], qscale=5)
        for k in range(2):
            got = source_bytes(enc, k)
            assert np.array_equal(got, want[k]), (k, int(np.count_nonzero(got != want[k])))
            assert np.array_equal(got, mi.sim_frame(cells, frames[k], w, h, fill)), k
