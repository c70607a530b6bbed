"""The lifecycle of the four pass handles -- Resampler, LogMel, Mp2Encoder, TsProgram (C ABI parts 11, 12, 9, 10) -- held to ONE
script: a fresh handle, the refusals the host makes before anything is enqueued, a pass in flight, the same bits from a second
call, close() with a pass in flight.  Every message is a literal string and is compared whole with jsmpeg_hip_last_error()
through the RuntimeError's text.  The smallest call each kind can make; bits and messages are asserted, never times.

Where the mux differs from the three chained handles the script says so per kind: its stream numbers may repeat (the equal
pair is refused by its PTS), it has no flags per call (the unknown bit is the config's), its alignment refusal is
set_output's, its per-stream state is five words read by state(), which settles, and none of its readers is closed form.
Needs an MI355X."""
import ctypes
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FRAME = 1152


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


def refused(call, text):
    with pytest.raises(RuntimeError) as e:
        call()
    assert str(e.value) == text


def noise(n, seed):
    return np.random.default_rng(seed).uniform(-0.5, 0.5, n).astype(np.float32)


class Kind:
    """one handle kind: how the script makes it, calls it and reads it.  p: the device address of the kind's input"""
    keys = {"kernel_ms", "total_ms"}
    zero = (False, 0, 0)

    def __init__(self, torch):
        self.x = torch.from_numpy(self.input()).cuda()
        self.p = self.x.data_ptr()
        torch.cuda.synchronize()

    def rewind(self, h):
        """in front of a call that has to repeat the first one: nothing for a handle whose unchained calls start from zeros"""

    def info(self, h):
        return [h.chain_info(s) for s in range(2)]

    def mutators(self, h):
        return [h.chain_reset, lambda: h.chain_reset(0)]

    def numbers(self, h, streams, counts=(1, 0)):
        """a call over two streams with these stream numbers; counts in units of the kind's smallest input"""
        return self.call(h, ptrs=[self.p] * len(streams), counts=counts[:len(streams)], streams=streams)

    def refusals(self, h):
        w = self.who
        return [(lambda: self.numbers(h, [2]), "%s: stream_numbers[0] = 2 >= max_streams 2" % w),
                (lambda: self.numbers(h, [1, 0]), "%s: stream_numbers[] must ascend (stream_numbers[1] = 0 after 1)" % w),
                (lambda: self.numbers(h, [1, 1]), "%s: stream_numbers[] must ascend (stream_numbers[1] = 1 after 1)" % w),
                (lambda: self.call(h, ptrs=[0]), "%s: pcm[0] is NULL" % w),
                (lambda: self.call(h, ptrs=[self.p + 2]), "%s: pcm[0] is not 4-byte aligned" % w),
                (lambda: h._ok(self.raw(h)(h.h, None, None, None, 0, 4, None)), "%s: unknown flags 0x4" % w)]


class ResamplerKind(Kind):
    who = "resampler"
    in_flight = "resampler: a pass is in flight: jsmpeg_hip_resampler_sync (or a reader) settles it first"
    nothing_yet = "resampler: nothing was resampled yet"

    def input(self):
        return noise(2 * FRAME, 1).reshape(1, 2, FRAME)

    def make(self):
        from jsmpeg_amd import resample
        return resample.Resampler(48000, 16000, max_streams=2, max_frames=1)

    def call(self, h, chain=False, ptrs=None, counts=(1,), streams=None):
        h.resample([self.p] if ptrs is None else ptrs, list(counts), streams, chain=chain, end=not chain)

    def raw(self, h):
        return h.L.jsmpeg_hip_resampler_resample

    def bits(self, h):
        return h.counts(), h.read().tobytes()

    def readers(self, h):
        return [h.device_out, lambda: h.stream_out(0), h.read, h.waveform]

    def closed_form(self, h):
        out = h.stream_out(0), h.counts(), h.device_out()
        assert out[0] == (0, out[1][0]) and out[1][0] > 0 and out[2][0] and out[2][1] == 2 * h.row * 4
        return out

    def moved(self, h):
        info = h.chain_info(0)
        assert info[0] is True and info[1] == FRAME and info[2] > 0 and h.chain_info(1) == self.zero


class LogMelKind(Kind):
    who = "logmel"
    in_flight = "logmel: a pass is in flight: jsmpeg_hip_logmel_sync (or a reader) settles it first"
    nothing_yet = "logmel: no features were computed yet"

    def input(self):
        return noise(400, 2)

    def make(self):
        from jsmpeg_amd import logmel
        return logmel.LogMel(max_streams=2, max_samples=400)

    def call(self, h, chain=False, ptrs=None, counts=(1,), streams=None):
        h.features([self.p] if ptrs is None else ptrs, [400 * c for c in counts], streams, chain=chain)

    def raw(self, h):
        return h.L.jsmpeg_hip_logmel_features

    def bits(self, h):
        return h.counts(), h.read().tobytes()

    def readers(self, h):
        return [h.device_out, lambda: h.stream_out(0), h.read, h.tensor]

    def closed_form(self, h):
        from jsmpeg_amd import logmel
        out = h.stream_out(0), h.counts(), h.device_out()
        assert out[0] == (0, logmel.frames(400, False)) and out[1] == [out[0][1]] and out[2][0] and out[2][1] == 80 * h.row * 4
        return out

    def moved(self, h):
        from jsmpeg_amd import logmel
        assert h.chain_info(0) == (True, 400, logmel.frames(400, False)) and h.chain_info(1) == self.zero


class Mp2EncoderKind(Kind):
    who = "MP2 encoder"
    in_flight = "MP2 encoder: an encode is in flight: jsmpeg_hip_mp2_encoder_sync (or a reader) settles it first"
    nothing_yet = "MP2 encoder: nothing was encoded yet"
    zero = (False, 0)

    def input(self):
        return noise(2 * FRAME, 3).reshape(1, 2, FRAME)

    def make(self):
        from jsmpeg_amd import mp2_encode
        return mp2_encode.Mp2Encoder(1, 2, 8, max_streams=2, max_frames=1, max_es_bytes=4096)

    def call(self, h, chain=False, ptrs=None, counts=(1,), streams=None):
        h.encode([self.p] if ptrs is None else ptrs, list(counts), streams, chain=chain)

    def raw(self, h):
        return h.L.jsmpeg_hip_mp2_encoder_encode

    def bits(self, h):
        return h.es(0)

    def readers(self, h):
        return [h.device_es, lambda: h.stream_range(0), lambda: h.es(0), lambda: h.frame_stats(0),
                lambda: h._ok(h.L.jsmpeg_hip_mp2_encoder_frame_range(h.h, 0, None, None))]

    def closed_form(self, h):
        out = h.stream_range(0), h.frame_ranges()
        assert out == ((0, 384), [(0, 384)])                      # 128 kbit/s at 48 kHz: 384 bytes a frame, no padding
        return out

    def moved(self, h):
        assert h.chain_info(0) == (True, 1) and h.chain_info(1) == self.zero


class TsProgramKind(Kind):
    who = "ts_program"
    in_flight = "ts_program: a pass is in flight: jsmpeg_hip_ts_program_sync (or a reader) settles it first"
    nothing_yet = "ts_program: nothing was muxed yet"
    keys = {"mux_ms", "total_ms"}
    zero = [0] * 5
    UNIT = [(0, 300)]

    def __init__(self, torch):
        Kind.__init__(self, torch)
        self.out = torch.zeros(4096, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()

    def input(self):
        return np.random.default_rng(4).integers(0, 256, 320, dtype=np.uint8)      # one audio unit of 300 bytes, whole dwords behind it

    def cfg(self, **kw):
        from jsmpeg_amd import ts_program
        return ts_program.config(2, 1, 2, 4096, **kw)

    def make(self):
        from jsmpeg_amd import ts_program
        return ts_program.TsProgram(self.cfg())

    def call(self, h, chain=False, ranges=None, pts=(0,), streams=(0,), base=True):
        h.mux(None, (), (), None, self.p if base else None, self.UNIT if ranges is None else ranges, list(pts), list(streams))

    def rewind(self, h):
        h.reset()                                                 # the counters and `started` go on from call to call

    def bits(self, h):
        return h.ts(0)

    def info(self, h):
        return [h.state(s) for s in range(2)]

    def readers(self, h):
        return [h.device_ts, lambda: h.stream_range(0), lambda: h.ts(0), h.ts_all,
                lambda: h._ok(h.L.jsmpeg_hip_ts_program_unit_range(h.h, 1, 0, None, None, None))]

    def closed_form(self, h):
        return None                                               # every reader of the mux settles

    def mutators(self, h):
        return [h.reset, lambda: h.reset(0), lambda: h.set_state(0, [0] * 5), lambda: h.set_output(self.out.data_ptr(), 4096)]

    def refusals(self, h):
        def bad_flags():
            c = self.cfg()
            c.flags = 4
            if not h.L.jsmpeg_hip_ts_program_create(ctypes.byref(c)):
                from jsmpeg_amd import batch
                raise RuntimeError(batch.last_error())
        two = self.UNIT * 2
        return [(lambda: self.call(h, streams=[2]), "ts_program: audio stream[0] = 2 >= max_streams 2"),
                (lambda: self.call(h, ranges=two, pts=[0, 0], streams=[1, 0]), "ts_program: audio stream[] must ascend (stream[1] = 0 after 1)"),
                (lambda: self.call(h, ranges=two, pts=[10, 5], streams=[1, 1]), "ts_program: audio pts[1] is below pts[0] of the same stream"),
                (lambda: self.call(h, base=False), "ts_program: NULL audio argument"),
                (lambda: h.set_output(self.out.data_ptr() + 2, 1000), "ts_program: dev_ts is not 4-byte aligned"),
                (bad_flags, "ts_program: unknown flags 0x4")]

    def moved(self, h):
        """state() settles; the words are those of the one call, so the refused reset and set_state moved nothing"""
        from jsmpeg_amd import ts_program
        want = ts_program.program_mux_host(self.cfg(), audio=self.input(), a_ranges=self.UNIT, a_pts=[0], a_streams=[0])[2]
        assert self.info(h) == want and want[0][4] == 1 and want[1] == self.zero


KINDS = {"resampler": ResamplerKind, "logmel": LogMelKind, "mp2_encoder": Mp2EncoderKind, "ts_program": TsProgramKind}


@pytest.mark.parametrize("kind", list(KINDS))
def test_the_lifecycle_of_a_pass_handle(kind, torch, hip_lib):
    k = KINDS[kind](torch)
    h = k.make()
    # ---- a fresh handle
    assert h.query() is True
    h.sync()
    for reader in k.readers(h) + [h.timings]:
        refused(reader, k.nothing_yet)
    for m in k.mutators(h)[:2]:
        m()
    assert k.info(h) == [k.zero] * 2
    # ---- what the host refuses before anything is enqueued; the handle stays usable
    for call, text in k.refusals(h):
        refused(call, text)
    assert k.info(h) == [k.zero] * 2 and h.query() is True
    refused(h.timings, k.nothing_yet)
    # ---- one call, not synced
    k.call(h, chain=True)
    closed = k.closed_form(h)                                     # answered from the plan: the pass stays in flight, or the next line is not refused
    refused(lambda: k.call(h, chain=True), k.in_flight)
    for m in k.mutators(h):
        refused(m, k.in_flight)
    assert h.query() in (False, True)
    k.moved(h)
    h.sync()
    assert h.query() is True and k.closed_form(h) == closed
    k.moved(h)
    t = h.timings()
    assert set(t) == k.keys and all(math.isfinite(v) and v >= 0 for v in t.values())
    # ---- a second call gives the bits of the first
    k.rewind(h)
    k.call(h)
    first = k.bits(h)
    k.rewind(h)
    k.call(h)
    assert k.bits(h) == first and len(first)
    # ---- close() with a pass in flight; a new handle repeats the bits
    k.rewind(h)
    k.call(h)
    h.close()
    h.close()
    with k.make() as again:
        k.call(again)
        assert k.bits(again) == first
