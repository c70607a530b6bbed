"""The host runtime's messages, word for word: one refusal per file that reports through the shared fail() (csrc/host_common.h)
-- shard.hip, live.hip, engine.hip, mp2_stage.hip, mp2_live.hip -- with its numbers, compared with == against the text.  A
conversion that prints an argument with the wrong type or width changes a number here."""
import ctypes

import numpy as np
import pytest

import ts_craft


def _L():
    from jsmpeg_amd import batch as jb, distributed as jd
    jd._lib()                                     # the argument types of the shard entry points
    return jb.lib()


def _last(L):
    from jsmpeg_amd import batch as jb
    return jb.last_error()


def test_shard_plan_messages(hip_lib):
    from jsmpeg_amd import distributed as jd
    with pytest.raises(RuntimeError) as e:
        jd.plan_shards_c([1, 2], 0)
    assert str(e.value) == "bad shard plan arguments"
    with pytest.raises(RuntimeError) as e:
        jd.plan_rebalance_c([1, 1], [0, 5], 2)
    assert str(e.value) == "unit 1: home rank 5 outside the job"


def test_null_buffer_messages(hip_lib):
    L = _L()
    ho, hb = ctypes.c_uint64(), ctypes.c_uint64()
    assert L.jsmpeg_hip_split_gops(None, 8, None, 0, ctypes.byref(ho), ctypes.byref(hb)) < 0
    assert _last(L) == "null elementary stream"
    assert L.jsmpeg_hip_ts_packet_runs(None, 8, None, 0, None, None, 0, None, None) < 0
    assert _last(L) == "null buffer"


def test_host_demux_stream_id_message(hip_lib):
    L = _L()
    ts = np.ascontiguousarray(ts_craft.CASES["negative_total"]())
    fn = L.jsmpeg_hip_ts_demux_host
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint64), ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint64,
                   ctypes.POINTER(ctypes.c_uint64), ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32]
    assert fn(ts.ctypes.data, len(ts), None, 0, 0, None, 0, None, None, None, None, 0) < 0
    assert _last(L) == "stream id 0 out of range"


def test_audio_handles_without_a_device(hip_lib):
    from jsmpeg_amd import mp2
    L = _L()
    L.jsmpeg_hip_device_count.restype = ctypes.c_int
    if L.jsmpeg_hip_device_count() > 0:
        pytest.skip("the text of a machine without a device")
    with pytest.raises(RuntimeError) as e:
        mp2.Mp2Batch(2, 1 << 16)
    assert str(e.value) == "jsmpeg_hip_mp2_batch_create failed: no HIP device available: the MP2 decode stage has no CPU fallback"
    with pytest.raises(RuntimeError) as e:
        mp2.Mp2Live(2, store_bytes=1 << 16)
    assert str(e.value) == "jsmpeg_hip_mp2_live_create failed: no HIP device available: the MP2 decode stage has no CPU fallback"


@pytest.mark.gpu
def test_mp2_batch_messages(hip_lib):
    from jsmpeg_amd import mp2
    ts = ts_craft.CASES["sixteen_pids"]()
    some = np.zeros(40000, dtype=np.uint8)
    with mp2.Mp2Batch(2, 1 << 16) as b:
        with pytest.raises(RuntimeError) as e:
            b.ts_writes(0)
        assert str(e.value) == "jsmpeg_hip_mp2_batch_ts_writes failed: no TS upload for stream 0"
        with pytest.raises(RuntimeError) as e:
            b.upload([some[:10]] * 3)
        assert str(e.value) == "jsmpeg_hip_mp2_batch_upload failed: MP2 batch: 3 streams do not fit"
        with pytest.raises(RuntimeError) as e:
            b.upload([some, some])
        assert str(e.value) == "jsmpeg_hip_mp2_batch_upload failed: MP2 batch: 80000 bytes do not fit"
        for sid in (0, 300):
            with pytest.raises(RuntimeError) as e:
                b.upload_ts([ts], sid)
            assert str(e.value) == "jsmpeg_hip_mp2_batch_upload_ts failed: stream id %d out of range" % sid
        with pytest.raises(RuntimeError) as e:
            b.frame_info(0, 0)
        assert str(e.value) == "jsmpeg_hip_mp2_batch_frame_info failed: MP2 batch: not decoded"


@pytest.mark.gpu
def test_mp2_live_messages(hip_lib):
    from jsmpeg_amd import mp2
    with mp2.Mp2Live(2, store_bytes=1 << 16) as a:
        assert (a.open(), a.open()) == (0, 1)
        with pytest.raises(RuntimeError) as e:
            a.open()
        assert str(e.value) == "jsmpeg_hip_mp2_live_open failed: open: all 2 streams are in use"
        a.close_stream(1)
        with pytest.raises(RuntimeError) as e:
            a.close_stream(1)
        assert str(e.value) == "jsmpeg_hip_mp2_live_close failed: close: stream 1 is not open"
        with pytest.raises(RuntimeError) as e:
            a.write(0, 0.0, np.zeros((1 << 16) + 1, dtype=np.uint8))
        assert str(e.value) == ("jsmpeg_hip_mp2_live_write failed: write of 65537 bytes is larger than the stream's store "
                                "(the reference writes past its allocation there)")


@pytest.mark.gpu
def test_batch_messages(hip_lib):
    from jsmpeg_amd import batch as jb
    ts = ts_craft.CASES["negative_total"]()
    with jb.Batch(176, 144, 2, 64, 1 << 16) as b:
        with pytest.raises(RuntimeError) as e:
            b.upload_ts([ts, ts, ts])
        assert str(e.value) == "3 streams > max_streams 2"
