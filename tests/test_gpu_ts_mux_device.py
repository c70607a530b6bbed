"""The TS mux on the device over any device bytes (jsmpeg_hip_ts_mux_device, encode.ts_mux_device: k_ts_plan and k_ts_write of
jsmpeg_amd/csrc/encode.hip over a host-given unit list): the packets and the stream ranges equal the host mux
(jsmpeg_hip_ts_mux_host) and the CPU simulator's plan, counters included, on the rule's edges.  Bytes are asserted, never
times."""
import numpy as np
import pytest

import enc_ts_inputs as et

pytestmark = pytest.mark.gpu

CANARY = 64


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


def device_mux(torch, case, cap=None):
    """encode.ts_mux_device over the case, the output buffer `cap` bytes with a canary behind it: (total, the buffer on the
    host, ranges, counters out); RuntimeError on a refusal, after the canary and the buffer were checked untouched"""
    from jsmpeg_amd import encode
    cap = case.bound() if cap is None else cap
    es = torch.from_numpy(case.es).cuda()
    out = torch.full((cap + CANARY,), 0xA5, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    try:
        total, ranges, cc = encode.ts_mux_device(es.data_ptr(), case.ranges, [p / 90000.0 for p in case.pts], out.data_ptr(), cap,
                                                 streams=case.streams, n_streams=case.n_streams, continuity=case.counters())
    except RuntimeError:
        assert bool((out == 0xA5).all())
        raise
    host = out.cpu().numpy()
    assert np.all(host[cap:] == 0xA5)
    return total, host[:cap], ranges, cc


def held(torch, case, where):
    want = et.host_want(case)
    total, buf, ranges, cc = device_mux(torch, case)
    end = et.assert_equals_host(case, buf, ranges, cc, where, want)
    assert end == total
    sim = et.sim_mux(case)
    assert (total, ranges, cc) == (sim.total, sim.ranges, sim.cc), where
    return total, buf


def test_edge_sizes_first_unit_at_byte_5(torch, hip_lib):
    """(fails without the feature: jsmpeg_hip_ts_mux_device is missing)"""
    c = et.sizes_case(1, lead=5)
    assert c.ranges[0][0] == 5 and all(p < (1 << 33) for p in c.pts)       # (seconds and back: exact below 2^33 ticks)
    c.cc[0] = 15
    total, buf = held(torch, c, "sizes")
    assert buf[3] & 15 == 15 and buf[188 + 3] & 15 == 0                    # counter in 15: the first packet carries it
    assert np.all(buf[:total:188] == 0x47)


def test_every_size_1_to_400_in_one_call(torch, hip_lib):
    c = et.sweep_case()
    total, _ = held(torch, c, "sweep")
    assert 100_000 < total < 200_000
    with pytest.raises(RuntimeError, match="ts_cap"):
        device_mux(torch, c, cap=total - 1)
    total_exact, buf, _, _ = device_mux(torch, c, cap=total)
    assert total_exact == total


def test_three_streams(torch, hip_lib):
    c = et.three_stream_case()
    c.pts = [p & et.PTS_MASK for p in c.pts]
    total, _ = held(torch, c, "three streams")
    with pytest.raises(RuntimeError, match="ts_cap"):
        device_mux(torch, c, cap=total - 1)


def test_random_cases_and_no_units(torch, hip_lib):
    for i, c in enumerate(et.random_cases(24, seed=31)):
        c.pts = [p & et.PTS_MASK for p in c.pts]
        held(torch, c, ("random", i))
    empty = et.Case(np.zeros(16, np.uint8), [], [], [], {}, 3)
    total, _, ranges, cc = device_mux(torch, empty, cap=188)
    assert (total, ranges, cc) == (0, {}, [0, 0, 0])


def test_refusals(torch, hip_lib):
    from jsmpeg_amd import encode
    c = et.sizes_case(1, sizes=[300, 20])
    es = torch.from_numpy(c.es).cuda()
    out = torch.zeros(1024, dtype=torch.uint8, device="cuda")
    pts = [0.0, 0.1]
    for kw, why in ((dict(pid=0x2000), "pid"), (dict(stream_id=0x100), "stream id"), (dict(streams=[1, 0]), "ascend"),
                    (dict(streams=[0, 3], n_streams=3), "n_streams")):
        with pytest.raises(RuntimeError, match=why):
            encode.ts_mux_device(es.data_ptr(), c.ranges, pts, out.data_ptr(), 1024, **kw)
    with pytest.raises(RuntimeError, match="aligned"):
        encode.ts_mux_device(es.data_ptr(), c.ranges, pts, out.data_ptr() + 1, 1000)
    assert encode.ts_mux_device(es.data_ptr(), c.ranges, pts, out.data_ptr(), 1024)[0] == 188 * 3
