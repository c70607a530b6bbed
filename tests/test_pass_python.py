"""jsmpeg_amd/_pass.py without a device: the marshalling of a call's streams and the walkers over Mp2Batch and Mp2Live that
Resampler and Mp2Encoder share, against small fakes.  The refusal texts are the ones the four modules raised before the
helpers were shared."""
import ctypes

import pytest

from jsmpeg_amd import _pass

FRAME_BYTES = 2 * 1152 * 4


def refused(call, text):
    with pytest.raises(ValueError) as e:
        call()
    assert str(e.value) == text


def test_marshal():
    arr, cnt, st, numbers = _pass.marshal([4096, 0, 8192], [2, 0, 1], None, "frames: one count per stream")
    assert isinstance(arr, ctypes.c_void_p * 3) and list(arr) == [4096, None, 8192]
    assert cnt.dtype == "uint32" and cnt.tolist() == [2, 0, 1] and st is None and numbers == [0, 1, 2]
    arr, cnt, st, numbers = _pass.marshal([4096, 8192], [1, 1], [3, 7], "frames: one count per stream")
    assert st.dtype == "uint32" and st.tolist() == [3, 7] and numbers == [3, 7] and all(type(v) is int for v in numbers)
    arr, cnt, st, numbers = _pass.marshal([], [], None, "frames: one count per stream")
    assert isinstance(arr, ctypes.c_void_p * 1) and list(arr) == [None] and cnt.shape == (0,) and numbers == []
    for text in ("frames: one count per stream", "counts: one sample count per stream"):
        refused(lambda: _pass.marshal([4096, 8192], [1], None, text), text)
        refused(lambda: _pass.marshal([4096], [[1]], None, text), text)
    refused(lambda: _pass.marshal([4096, 8192], [1, 1], [0], "frames: one count per stream"), "streams: one stream number per stream")
    refused(lambda: _pass.marshal([4096], [1], [0, 1], "counts: one sample count per stream"), "streams: one stream number per stream")


class FakeBatch:
    """three streams of 2, 0 and 3 frames; stream 2 at another rate when asked"""

    def __init__(self, rates=(48000, 48000, 48000)):
        self.n_streams, self.counts, self.rates = 3, [2, 0, 3], rates

    def frame_count(self, s):
        return self.counts[s]

    def frame_info(self, s, k):
        assert k < self.counts[s]                                 # a stream without frames is never asked
        return (0, 0, self.rates[s])

    def pcm_device_pointer(self):
        return 1 << 20


def test_batch_frames():
    base = 1 << 20
    assert _pass.batch_frames(FakeBatch(), 48000, "resample_batch", "the resampler takes") == ([base, base + 2 * FRAME_BYTES, base + 2 * FRAME_BYTES], [2, 0, 3])
    assert _pass.batch_frames(FakeBatch((48000, 1, 48000)), 48000, "encode_batch", "the encoder at")[1] == [2, 0, 3]
    refused(lambda: _pass.batch_frames(FakeBatch((48000, 48000, 44100)), 48000, "resample_batch", "the resampler takes"),
            "resample_batch: stream 2 is sampled at 44100 Hz, the resampler takes 48000")
    refused(lambda: _pass.batch_frames(FakeBatch((32000, 48000, 48000)), 48000, "encode_batch", "the encoder at"),
            "encode_batch: stream 0 is sampled at 32000 Hz, the encoder at 48000")


class FakeLive:
    """a tick of live streams 5 (two frames) and 2 (one frame), handed over out of order"""

    def __init__(self, rate5=44100):
        self.list = [dict(stream=5, sample_rate=rate5, device_pcm=5000), dict(stream=2, sample_rate=44100, device_pcm=2000),
                     dict(stream=5, sample_rate=rate5, device_pcm=5000 + FRAME_BYTES)]

    def frames(self):
        return list(self.list)


def test_live_frames():
    live = FakeLive()
    frames, ptrs, counts, numbers = _pass.live_frames(live, 44100, 6, True, "resample_live", "the resampler takes")
    assert [f["device_pcm"] for f in frames] == [2000, 5000, 5000 + FRAME_BYTES]
    assert (ptrs, counts, numbers) == ([2000, 5000], [1, 2], [2, 5])           # chained: the live id is the stream number
    assert _pass.live_frames(live, 44100, 1, False, "encode_live", "the encoder at")[1:] == ([2000, 5000], [1, 2], None)
    refused(lambda: _pass.live_frames(live, 44100, 5, True, "resample_live", "the resampler takes"), "resample_live: live stream id 5 >= max_streams 5")
    refused(lambda: _pass.live_frames(live, 44100, 5, True, "encode_live", "the encoder at"), "encode_live: live stream id 5 >= max_streams 5")
    refused(lambda: _pass.live_frames(FakeLive(48000), 44100, 6, True, "resample_live", "the resampler takes"),
            "resample_live: stream 5 is sampled at 48000 Hz, the resampler takes 44100")
    refused(lambda: _pass.live_frames(FakeLive(48000), 44100, 6, False, "encode_live", "the encoder at"),
            "encode_live: stream 5 is sampled at 48000 Hz, the encoder at 44100")

    class Empty:
        def frames(self):
            return []
    assert _pass.live_frames(Empty(), 44100, 1, True, "encode_live", "the encoder at") == ([], [], [], [])
