"""What the intra encoder (C ABI part 8) costs: ms per call, MEASURED (the tests assert bytes, never times).  Pool frames of a
decoded batch (bench.py's generator, cfg2: 64 streams x 120 pictures of 1080p) to streams at q = 8, for 64 pictures (the first of
every stream) and for all 7680: the call's span split by jsmpeg_hip_encoder_timings, the output bytes, the bytes the two passes
read and write per picture against a plain device copy's rate measured in the same process, and the whole pass of decode alone
against decode + encode (what a transcode costs).  A third step: Batch.tensor(uint8) -> encode_tensor -> decode, the luma PSNR
against the first decode.  A fourth step, `gop`: 64 streams x 12 pictures of 1080p with --gop and --search (gop 1: the intra
pass on the same pictures): ms per pass, the output bytes, and what Batch.decode takes on the encoder's streams; its figures go
to the bench_gop<N>_r<R> section of profiles/enc_p_notes.md.  A fifth step, `rate`: the same 768 pictures with --gop and --search
at a fixed scale, with rate control over 1 .. 31 and over 4 .. 16 (--rate bytes per picture): ms per pass each way, and the
registers, LDS and occupancy of the three rate kernels; its figures go to the bench section of profiles/enc_rate_notes.md.
A sixth step, `chain`: what a live relay runs -- 64 streams of 1080p, ONE picture per stream per call, 24 calls, with --gop and
--search, at a fixed scale and with rate control (--rate): bytes per picture and ms per call.  With chained calls
(Encoder.encode(chain=True)) the calls continue their streams; on a tree whose encoder has no chains the same calls are all I
pictures -- that is the figure to hold against.  Its figures go to the bench (or, without chains, bench_unchained) section of
profiles/enc_chain_notes.md.
A seventh step, `scale`: renditions -- 64 streams of 1080p, one picture per stream per call, 24 calls, scaled to 640x360 and to
1280x720 by Encoder.encode_scaled (chained, with --gop and --search, q = 8): the scale's "convert" time and the call's total,
against the route through RGB in the same run (Batch.tensor(size=..., dtype=uint8), then encode_tensor: k_tensor + k_enc_rgb) and
against a plain device copy of the bytes the scale moves.  Its figures go to the bench section of profiles/enc_scale_notes.md.
An eighth step, `ts`: what the relay's last step costs -- 64 streams of 1080p, one picture per stream per chained call, with
--gop and --search at q = 8: host time from the call to every stream's TS bytes on the host, (a) with TS on the device
(Encoder.set_ts) and ONE read_ts of the whole buffer, (b) with TS off, read_es per stream and jsmpeg_hip_ts_mux_host per stream;
and timings() with TS on and off, alternating, in one process.  Its figures go to the bench section of profiles/enc_ts_notes.md.

Every GPU step is a child process of this tool under its own `timeout`; the steps are chained and the tool stops at the first
one that fails.  The figures go into the bench section of profiles/enc_notes.md (nothing is written for a step that did not
run).
    python tools/encode_bench.py [--steps pool64,pool7680,tensor] [--reps 8]
    python tools/encode_bench.py --steps gop --gop 12 --search 7
    python tools/encode_bench.py --steps rate --gop 12 --search 7 --rate 40000
    python tools/encode_bench.py --steps chain --gop 12 --search 7 --rate 40000 --reps 3
    python tools/encode_bench.py --steps scale --gop 12 --search 7 --reps 3
    python tools/encode_bench.py --steps ts --gop 12 --search 7 --reps 3"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
W, H = 1920, 1080
STEPS = {"pool64": 300, "pool7680": 420, "tensor": 120, "gop": 300, "rate": 420, "chain": 420, "scale": 420, "ts": 420}          # seconds each step may take


def median(v):
    return round(float(np.median(v)), 3)


def copy_rate(L, nbytes, reps):
    """GB/s (read + written) of a plain device-to-device copy of nbytes"""
    import ctypes
    L.jsmpeg_hip_device_alloc.restype = ctypes.c_void_p
    L.jsmpeg_hip_device_alloc.argtypes = [ctypes.c_uint64, ctypes.c_int32, ctypes.c_int32]
    L.jsmpeg_hip_device_copy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64]
    L.jsmpeg_hip_device_free.argtypes = [ctypes.c_void_p]
    a, b = L.jsmpeg_hip_device_alloc(nbytes, 0, 1), L.jsmpeg_hip_device_alloc(nbytes, 0, 2)
    if not a or not b:
        raise RuntimeError("device_alloc failed")
    ms = []
    for r in range(reps + 2):
        L.jsmpeg_hip_device_synchronize()
        t0 = time.perf_counter()
        L.jsmpeg_hip_device_copy(b, a, nbytes)
        L.jsmpeg_hip_device_synchronize()
        if r >= 2:
            ms.append((time.perf_counter() - t0) * 1e3)
    L.jsmpeg_hip_device_free(a)
    L.jsmpeg_hip_device_free(b)
    return 2 * nbytes / (float(np.median(ms)) * 1e-3) / 1e9


def step_pool(all_pictures, reps):
    import bench
    from jsmpeg_amd import batch as jb
    from jsmpeg_amd import encode
    streams = [g[0] for g in bench.generate_streams(0, 64, 120)]
    total = sum(len(s) for s in streams)
    with jb.Batch(W, H, 64, 7680 + 8, total + 64 * 64 + 4096, device=0) as b:
        b.upload(streams)
        assert b.decode() == 7680
        infos = b.pictures()
        if all_pictures:
            pics = [p for p, i in enumerate(infos) if i.decoded]
        else:
            seen, pics = set(), []
            for p, i in enumerate(infos):
                if i.decoded and i.stream not in seen:
                    seen.add(i.stream)
                    pics.append(p)
        sn = [infos[p].stream for p in pics]
        # size the output from a call over the first pictures
        with encode.Encoder(W, H, 64, 64, 64 << 20, device=0) as probe:
            probe.encode_batch(b, pics[:64], [0] * 64 if all_pictures else sn[:64], 8)
            probe.sync()
            per_picture = probe.device_es()[1] / 64.0
        cap = int(per_picture * len(pics) * 1.5) + (1 << 20)
        with encode.Encoder(W, H, len(pics), 64, cap, device=0) as enc:
            ptrs = [b.frame_pool_ptr + p * b.frame_stride for p in pics]
            wall, split = [], []
            for r in range(reps + 2):
                t0 = time.perf_counter()
                enc.encode(ptrs, sn, 8)
                enc.sync()
                if r >= 2:
                    wall.append((time.perf_counter() - t0) * 1e3)
                    split.append(enc.timings())
            out_bytes = enc.device_es()[1]
            dec, both = [], []
            for r in range(reps + 2):
                t0 = time.perf_counter()
                b.decode()
                t1 = time.perf_counter()
                enc.encode(ptrs, sn, 8)
                enc.sync()
                t2 = time.perf_counter()
                if r >= 2:
                    dec.append((t1 - t0) * 1e3)
                    both.append((t2 - t0) * 1e3)
            rate = copy_rate(b.L, 1 << 30, reps)
            frame = b.frame_stride
            mbs = (W + 15) // 16 * ((H + 15) // 16)
            moved = 2 * frame + 2 * 12 * mbs + 2 * out_bytes / len(pics)       # both passes read the frame; records out and in; clear + write
            total_ms = median([s["total_ms"] for s in split])
            return dict(step="pool7680" if all_pictures else "pool64", pictures=len(pics), streams=len(set(sn)), q=8,
                        wall_ms=median(wall), convert_ms=median([s["convert_ms"] for s in split]), measure_scan_ms=median([s["measure_ms"] for s in split]),
                        write_ms=median([s["write_ms"] for s in split]), total_ms=total_ms, output_bytes=int(out_bytes),
                        output_bytes_per_picture=round(out_bytes / len(pics)), moved_bytes_per_picture=round(moved),
                        copy_GBps=round(rate, 1), copy_bound_ms=round(moved * len(pics) / (rate * 1e9) * 1e3, 3),
                        ratio_to_copy_bound=round(total_ms / (moved * len(pics) / (rate * 1e9) * 1e3), 2),
                        decode_alone_wall_ms=median(dec), decode_then_encode_wall_ms=median(both))


def step_gop(gop, search, reps):
    """64 streams x 12 pictures of 1080p from a batch's pool, q = 8, with a GOP (gop 1: the intra pass); then Batch.decode of
    the encoder's streams, uploaded to a second batch"""
    import bench
    from jsmpeg_amd import batch as jb
    from jsmpeg_amd import encode
    streams = [g[0] for g in bench.generate_streams(0, 64, 12)]
    total = sum(len(s) for s in streams)
    with jb.Batch(W, H, 64, 768 + 8, total + 64 * 64 + 4096, device=0) as b:
        b.upload(streams)
        assert b.decode() == 768
        infos = b.pictures()
        pics = [p for p, i in enumerate(infos) if i.decoded]
        sn = [infos[p].stream for p in pics]
        ptrs = [b.frame_pool_ptr + p * b.frame_stride for p in pics]
        with encode.Encoder(W, H, len(pics), 64, 768 << 20, device=0) as enc:
            if gop > 1:
                enc.set_gop(gop, search)
            wall, split = [], []
            for r in range(reps + 2):
                t0 = time.perf_counter()
                enc.encode(ptrs, sn, 8)
                enc.sync()
                if r >= 2:
                    wall.append((time.perf_counter() - t0) * 1e3)
                    split.append(enc.timings())
            ptr, out_bytes = enc.device_es()
            kinds = None
            if gop > 1:
                kinds = [sum(enc.picture_stats(k)[n] for k in range(len(pics))) for n in ("intra", "coded", "not_coded", "skipped")]
            dec = []
            # the streams go through the host: attach_device wants 8 bytes between streams, and the encoder's 16-byte aligned
            # begins leave fewer where a stream ends 9 .. 16 bytes into its last 16 (the intra encoder's layout, not changed here)
            es = [np.frombuffer(enc.es(s), dtype=np.uint8) for s in range(64)]
            with jb.Batch(W, H, 64, 768 + 8, out_bytes + 64 * 64 + 4096, device=0) as back:
                back.upload(es)
                for r in range(reps + 2):
                    t0 = time.perf_counter()
                    n = back.decode()
                    if r >= 2:
                        dec.append((time.perf_counter() - t0) * 1e3)
                assert n == len(pics)
            ms = [s["total_ms"] for s in split]
            return dict(step="gop", gop=gop, search=search, pictures=len(pics), streams=64, q=8, wall_ms=median(wall),
                        measure_scan_ms=median([s["measure_ms"] for s in split]), write_ms=median([s["write_ms"] for s in split]),
                        total_ms=median(ms), total_ms_min=round(min(ms), 3), total_ms_max=round(max(ms), 3), output_bytes=int(out_bytes),
                        kinds=kinds, decode_of_output_wall_ms=median(dec))


RATE_KERNELS = ("k_enc_rate_measure", "k_enc_rate_scan", "k_enc_rate_pick")


def step_rate(gop, search, target, reps):
    """64 streams x 12 pictures of 1080p from a batch's pool with a GOP: the pass at q = 8, with rate control over 1 .. 31 and
    over 4 .. 16; what the compiler gave the three rate kernels (no device needed for that part)"""
    import bench
    from jsmpeg_amd import batch as jb
    from jsmpeg_amd import build, encode
    usage = build.check_kernel_resources()
    kernels = {k: {n: v[n] for n in ("VGPRs", "LDS Size", "Occupancy", "ScratchSize")} for k in RATE_KERNELS for name, v in usage.items() if k in name}
    streams = [g[0] for g in bench.generate_streams(0, 64, 12)]
    total = sum(len(s) for s in streams)
    with jb.Batch(W, H, 64, 768 + 8, total + 64 * 64 + 4096, device=0) as b:
        b.upload(streams)
        assert b.decode() == 768
        infos = b.pictures()
        pics = [p for p, i in enumerate(infos) if i.decoded]
        sn = [infos[p].stream for p in pics]
        ptrs = [b.frame_pool_ptr + p * b.frame_stride for p in pics]
        ways = []
        with encode.Encoder(W, H, len(pics), 64, 768 << 20, device=0) as enc:
            enc.set_gop(gop, search)
            for name, rule in (("fixed scale 8", None), ("rate control, 1 .. 31", (target, 1, 31, 4)), ("rate control, 4 .. 16", (target, 4, 16, 4))):
                enc.set_rate(*(rule or (0,)))
                wall, split = [], []
                for r in range(reps + 2):
                    t0 = time.perf_counter()
                    enc.encode(ptrs, sn, 8)
                    enc.sync()
                    if r >= 2:
                        wall.append((time.perf_counter() - t0) * 1e3)
                        split.append(enc.timings())
                ms = [s["total_ms"] for s in split]
                way = dict(name=name, wall_ms=median(wall), measure_scan_ms=median([s["measure_ms"] for s in split]), write_ms=median([s["write_ms"] for s in split]),
                           total_ms=median(ms), total_ms_min=round(min(ms), 3), total_ms_max=round(max(ms), 3), output_bytes=int(enc.device_es()[1]))
                if rule:
                    chosen = [enc.picture_rate(k) for k in range(len(pics))]
                    way["picture_bytes"] = sum(c["bytes"] for c in chosen)
                    way["over_budget"] = sum(1 for c in chosen if c["bytes"] > c["budget"])
                    way["q_mean"] = round(float(np.mean([c["q"] for c in chosen])), 2)
                ways.append(way)
        return dict(step="rate", gop=gop, search=search, target=target, pictures=len(pics), streams=64, ways=ways, kernels=kernels)


CHAIN_CALLS = 24


def step_chain(gop, search, target, reps):
    """64 streams x 24 pictures of 1080p from a batch's pool, a picture per stream per call (24 calls a round, one round to warm
    up and `reps` measured), q = 8 and rate control over 1 .. 31; chained where the encoder has chains"""
    import bench
    from jsmpeg_amd import batch as jb
    from jsmpeg_amd import encode
    chained = hasattr(encode, "CHAIN")
    streams = [g[0] for g in bench.generate_streams(0, 64, CHAIN_CALLS)]
    total = sum(len(s) for s in streams)
    n = 64 * CHAIN_CALLS
    with jb.Batch(W, H, 64, n + 8, total + 64 * 64 + 4096, device=0) as b:
        b.upload(streams)
        assert b.decode() == n
        infos = b.pictures()
        by_stream = {}
        for p, i in enumerate(infos):
            if i.decoded:
                by_stream.setdefault(i.stream, []).append(p)
        assert sorted(by_stream) == list(range(64)) and all(len(v) == CHAIN_CALLS for v in by_stream.values())
        calls = [[b.frame_pool_ptr + by_stream[s][t] * b.frame_stride for s in range(64)] for t in range(CHAIN_CALLS)]
        sn = list(range(64))
        ways = []
        with encode.Encoder(W, H, 64, 64, 128 << 20, device=0) as enc:
            enc.set_gop(gop, search)
            for name, rule in (("fixed scale 8", None), ("rate control, 1 .. 31", (target, 1, 31, 4))):
                enc.set_rate(*(rule or (0,)))
                wall, dev, size, first = [], [], [], []
                for r in range(reps + 1):
                    if chained:
                        enc.chain_reset()
                    for t, ptrs in enumerate(calls):
                        t0 = time.perf_counter()
                        if chained:
                            enc.encode(ptrs, sn, 8, end=False, chain=True)
                        else:
                            enc.encode(ptrs, sn, 8, end=False)
                        enc.sync()
                        if r >= 1:
                            wall.append((time.perf_counter() - t0) * 1e3)
                            dev.append(enc.timings()["total_ms"])
                            first.append(t % gop == 0)
                            if r == 1:
                                size.append(sum(v for _, v in enc.picture_ranges()))
                i_calls = [k for k in range(CHAIN_CALLS) if k % gop == 0] if chained else list(range(CHAIN_CALLS))
                p_calls = [k for k in range(CHAIN_CALLS) if k not in i_calls]
                pick = lambda v, flag: [x for x, f in zip(v, first) if f == flag or not chained]
                ways.append(dict(name=name, calls=len(wall), wall_ms=median(wall), total_ms=median(dev), total_ms_min=round(min(dev), 3), total_ms_max=round(max(dev), 3),
                                 i_call_ms=median(pick(dev, True)), p_call_ms=median(pick(dev, False)) if p_calls else None,
                                 bytes_per_picture=round(sum(size) / n), i_bytes_per_picture=round(sum(size[k] for k in i_calls) / (64 * len(i_calls))),
                                 p_bytes_per_picture=round(sum(size[k] for k in p_calls) / (64 * len(p_calls))) if p_calls else None))
        return dict(step="chain", chained=chained, gop=gop, search=search, target=target, streams=64, calls=CHAIN_CALLS, reps=reps, ways=ways)


SCALE_SIZES = ((640, 360), (1280, 720))


def step_scale(gop, search, reps):
    """64 streams x 24 pictures of 1080p from a batch's pool, a picture per stream per call, chained, q = 8, into encoders of
    640x360 and 1280x720: through encode_scaled, and through Batch.tensor(uint8) + encode_tensor (one round to warm up, `reps`
    measured)"""
    import torch
    import bench
    from jsmpeg_amd import batch as jb
    from jsmpeg_amd import build, encode
    usage = build.check_kernel_resources()
    kernel = {n: v[n] for name, v in usage.items() if "k_enc_scale" in name for n in ("VGPRs", "LDS Size", "Occupancy", "ScratchSize")}
    streams = [g[0] for g in bench.generate_streams(0, 64, CHAIN_CALLS)]
    total = sum(len(s) for s in streams)
    n = 64 * CHAIN_CALLS
    with jb.Batch(W, H, 64, n + 8, total + 64 * 64 + 4096, device=0) as b:
        b.upload(streams)
        assert b.decode() == n
        by_stream = {}
        for p, i in enumerate(b.pictures()):
            if i.decoded:
                by_stream.setdefault(i.stream, []).append(p)
        assert sorted(by_stream) == list(range(64)) and all(len(v) == CHAIN_CALLS for v in by_stream.values())
        calls = [[by_stream[s][t] for s in range(64)] for t in range(CHAIN_CALLS)]
        sn = list(range(64))
        rate = copy_rate(b.L, 1 << 30, 8)
        sizes = []
        for ow, oh in SCALE_SIZES:
            ways = []
            with encode.Encoder(ow, oh, 64, 64, 64 << 20, device=0) as enc:
                enc.set_gop(gop, search)
                moved = 64 * (W * H * 3 // 2 + enc.frame_bytes)                # the source planes' display area read once, the coded frames written once
                for name in ("encode_scaled", "Batch.tensor(uint8) + encode_tensor"):
                    wall, convert, tensor_ms, dev, size = [], [], [], [], []
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    for r in range(reps + 1):
                        enc.chain_reset()
                        for pics in calls:
                            t0 = time.perf_counter()
                            if name == "encode_scaled":
                                enc.encode_scaled([b.frame_pool_ptr + p * b.frame_stride for p in pics], (W, H), streams=sn, qscale=8, end=False, chain=True)
                            else:
                                e0.record()
                                x = b.tensor(pictures=pics, size=(oh, ow), dtype=torch.uint8)
                                e1.record()
                                enc.encode_tensor(x, sn, 8, end=False, chain=True)
                            enc.sync()
                            if r >= 1:
                                ms = enc.timings()
                                wall.append((time.perf_counter() - t0) * 1e3)
                                tensor_ms.append(e0.elapsed_time(e1) if name != "encode_scaled" else 0.0)
                                convert.append(ms["convert_ms"] + tensor_ms[-1])
                                dev.append(ms["total_ms"] + tensor_ms[-1])
                                if r == 1:
                                    size.append(sum(v for _, v in enc.picture_ranges()))
                    ways.append(dict(name=name, calls=len(wall), wall_ms=median(wall), to_planes_ms=median(convert), to_planes_ms_min=round(min(convert), 3),
                                     to_planes_ms_max=round(max(convert), 3), k_tensor_ms=median(tensor_ms), total_ms=median(dev),
                                     bytes_per_picture=round(sum(size) / n)))
            sizes.append(dict(width=ow, height=oh, moved_bytes=moved, copy_bound_ms=round(moved / (rate * 1e9) * 1e3, 3), ways=ways))
        return dict(step="scale", gop=gop, search=search, streams=64, calls=CHAIN_CALLS, reps=reps, copy_GBps=round(rate, 1), sizes=sizes, kernel=kernel)


def step_ts(gop, search, reps):
    """64 streams x 24 pictures of 1080p from a batch's pool, a picture per stream per chained call, q = 8 (one round to warm
    up, `reps` measured): from the call to all streams' TS bytes on the host, with the mux on the device and with the host's"""
    import ctypes
    import bench
    from jsmpeg_amd import batch as jb
    from jsmpeg_amd import encode
    streams = [g[0] for g in bench.generate_streams(0, 64, CHAIN_CALLS)]
    total = sum(len(s) for s in streams)
    n = 64 * CHAIN_CALLS
    es_cap = 128 << 20
    ts_cap = encode.ts_bound(es_cap, 64, 64)
    with jb.Batch(W, H, 64, n + 8, total + 64 * 64 + 4096, device=0) as b:
        b.upload(streams)
        assert b.decode() == n
        by_stream = {}
        for p, i in enumerate(b.pictures()):
            if i.decoded:
                by_stream.setdefault(i.stream, []).append(p)
        assert sorted(by_stream) == list(range(64)) and all(len(v) == CHAIN_CALLS for v in by_stream.values())
        calls = [[b.frame_pool_ptr + by_stream[s][t] * b.frame_stride for s in range(64)] for t in range(CHAIN_CALLS)]
        sn = list(range(64))
        L = encode.lib()
        host_ts, host_es = np.empty(ts_cap, np.uint8), np.empty(es_cap, np.uint8)
        zero64, ln32, p64 = np.zeros(1, np.uint64), np.zeros(1, np.uint32), np.zeros(1, np.uint64)
        with encode.Encoder(W, H, 64, 64, es_cap, device=0) as on, encode.Encoder(W, H, 64, 64, es_cap, device=0) as off:
            on.set_ts(ts_cap)
            for e in (on, off):
                e.set_gop(gop, search)
            a_ms, b_ms, b_read_ms, b_mux_ms, es_bytes, ts_bytes = [], [], [], [], [], []
            t_on, t_off, first = [], [], []
            cc = [ctypes.c_uint8(0) for _ in sn]
            for r in range(reps + 1):
                for e in (on, off):
                    e.chain_reset()
                for t, ptrs in enumerate(calls):
                    # (a) the mux on the device, one copy
                    t0 = time.perf_counter()
                    on.encode(ptrs, sn, 8, end=False, chain=True)
                    got = L.jsmpeg_hip_encoder_read_ts(on.h, 0xffffffff, host_ts.ctypes.data, ts_cap)
                    ranges = [on.ts_range(s)[:2] for s in sn]
                    t1 = time.perf_counter()
                    assert got > 0 and ranges[-1][1] == got
                    # (b) what the parent offers: sync, a copy per stream, the host mux per stream
                    t2 = time.perf_counter()
                    off.encode(ptrs, sn, 8, end=False, chain=True)
                    off.sync()
                    at, sizes = 0, []
                    for s in sn:
                        k = L.jsmpeg_hip_encoder_read_es(off.h, s, host_es.ctypes.data + at, es_cap - at)
                        sizes.append(k)
                        at += k
                    t3 = time.perf_counter()
                    at = out = 0
                    for s in sn:
                        ln32[0], p64[0] = sizes[s], 3000 * (r * CHAIN_CALLS + t)
                        out += L.jsmpeg_hip_ts_mux_host(host_es.ctypes.data + at, zero64.ctypes.data, ln32.ctypes.data, p64.ctypes.data, 1, 0xE0, 0x100,
                                                        ctypes.byref(cc[s]), host_ts.ctypes.data + out, ts_cap - out)
                        at += sizes[s]
                    t4 = time.perf_counter()
                    if r >= 1:
                        a_ms.append((t1 - t0) * 1e3)
                        b_ms.append((t4 - t2) * 1e3)
                        b_read_ms.append((t3 - t2) * 1e3)
                        b_mux_ms.append((t4 - t3) * 1e3)
                        es_bytes.append(at)
                        ts_bytes.append(got)
                        t_on.append(on.timings())
                        t_off.append(off.timings())
                        first.append(t % gop == 0)
        med = lambda v, k: median([x[k] for x in v])
        kinds = []
        for name, flag in (("calls of I pictures", True), ("calls of P pictures", False)):
            pick = lambda v: [x for x, f in zip(v, first) if f == flag]
            if pick(a_ms):
                kinds.append(dict(name=name, calls=len(pick(a_ms)), device_mux_one_copy_ms=median(pick(a_ms)), host_mux_ms=median(pick(b_ms)),
                                  host_read_es_ms=median(pick(b_read_ms)), host_mux_only_ms=median(pick(b_mux_ms)),
                                  es_bytes=round(float(np.median(pick(es_bytes)))), ts_bytes=round(float(np.median(pick(ts_bytes)))),
                                  write_ms_ts_on=median([x["write_ms"] for x in pick(t_on)]), write_ms_ts_off=median([x["write_ms"] for x in pick(t_off)]),
                                  total_ms_ts_on=median([x["total_ms"] for x in pick(t_on)]), total_ms_ts_off=median([x["total_ms"] for x in pick(t_off)])))
        return dict(step="ts", gop=gop, search=search, streams=64, calls=CHAIN_CALLS, reps=reps, measured=len(a_ms),
                    device_mux_one_copy_ms=median(a_ms), device_mux_min_ms=round(min(a_ms), 3), device_mux_max_ms=round(max(a_ms), 3),
                    host_mux_ms=median(b_ms), host_mux_min_ms=round(min(b_ms), 3), host_mux_max_ms=round(max(b_ms), 3),
                    host_read_es_ms=median(b_read_ms), host_mux_only_ms=median(b_mux_ms),
                    es_bytes_per_call=round(float(np.mean(es_bytes))), ts_bytes_per_call=round(float(np.mean(ts_bytes))),
                    write_ms_ts_on=med(t_on, "write_ms"), write_ms_ts_off=med(t_off, "write_ms"),
                    total_ms_ts_on=med(t_on, "total_ms"), total_ms_ts_off=med(t_off, "total_ms"), kinds=kinds)


def step_tensor():
    import torch
    import enc_inputs as ei
    from jsmpeg_amd import batch as jb
    from jsmpeg_amd import build, cabi, encode
    es = np.fromfile(os.path.join(ROOT, "tests", "golden", "enc_pan_176x144.m1v"), dtype=np.uint8)
    oracle = build.build_oracle()
    first, _, _ = cabi.decode_stream(oracle, es, keep="planes")
    frames = [ei.frame_of(*f) for f in first]
    out = dict(step="tensor", content="enc_pan_176x144", pictures=len(frames))
    with jb.Batch(176, 144, 1, 16, 1 << 20, device=0) as b, encode.Encoder(176, 144, 16, 1, 4 << 20, device=0) as enc:
        b.upload([es])
        b.decode()
        x = b.tensor(dtype=torch.uint8)
        for q in (2, 8, 31):
            enc.encode_tensor(x, qscale=q)
            dec, _, _ = cabi.decode_stream(oracle, np.frombuffer(enc.es(0), dtype=np.uint8), keep="planes")
            out["psnr_q%d" % q] = round(ei.psnr(*ei.luma_sse(dec, frames, 176, 144)), 2)
    return out


def notes(results):
    lines = ["## Cost on the MI355X (measured by tools/encode_bench.py)", ""]
    for r in results:
        if r["step"] == "scale":
            lines = ["## Renditions: %d streams of 1080p, one picture per stream per call, %d chained calls, gop %d, search range %d, q = 8 (measured on an MI355X by tools/encode_bench.py)"
                     % (r["streams"], r["calls"], r["gop"], r["search"]), ""]
            for z in r["sizes"]:
                lines += ["**To %dx%d.**  The scale reads and writes %d bytes per call; a plain device copy ran at %.1f GB/s in the same process and would move them in %.3f ms."
                          % (z["width"], z["height"], z["moved_bytes"], r["copy_GBps"], z["copy_bound_ms"]), "",
                          "| | planes ready (convert), median (min .. max), ms per call | of that k_tensor, ms | call total on the device, ms | call + sync, host clock, ms | bytes per picture |",
                          "|---|---|---|---|---|---|"]
                for w in z["ways"]:
                    lines.append("| %s | %.3f (%.3f .. %.3f) | %s | %.3f | %.3f | %d |" % (
                        w["name"], w["to_planes_ms"], w["to_planes_ms_min"], w["to_planes_ms_max"], "%.3f" % w["k_tensor_ms"] if w["k_tensor_ms"] else "-",
                        w["total_ms"], w["wall_ms"], w["bytes_per_picture"]))
                a, c = z["ways"][0], z["ways"][1]
                lines += ["", "The fused scale takes %.2f times the copy's time and %.2f times the RGB route's (k_tensor + k_enc_rgb)."
                          % (a["to_planes_ms"] / z["copy_bound_ms"], a["to_planes_ms"] / c["to_planes_ms"]), ""]
            lines += ["Medians over %d measured calls each (%d rounds of %d behind one round to warm up).  k_enc_scale: %d VGPRs, %d bytes of LDS, occupancy %d, scratch %d."
                      % (r["sizes"][0]["ways"][0]["calls"], r["reps"], r["calls"], r["kernel"]["VGPRs"], r["kernel"]["LDS Size"], r["kernel"]["Occupancy"], r["kernel"]["ScratchSize"]), ""]
        elif r["step"] == "ts":
            lines = ["## TS for a relay tick: %d streams of 1080p, one picture per stream per chained call, %d calls, gop %d, search range %d, q = 8 (measured on an MI355X by tools/encode_bench.py)"
                     % (r["streams"], r["calls"], r["gop"], r["search"]), "",
                     "Host clock from the encode call to every stream's TS bytes on the host, median (min .. max) over %d calls (%d rounds of %d behind one round to warm up):"
                     % (r["measured"], r["reps"], r["calls"]), "",
                     "| way | ms per call |", "|---|---|",
                     "| (a) TS on the device, one `read_ts` of the whole buffer, 64 `ts_range` | %.3f (%.3f .. %.3f) |" % (r["device_mux_one_copy_ms"], r["device_mux_min_ms"], r["device_mux_max_ms"]),
                     "| (b) TS off: `sync`, 64 `read_es`, 64 `jsmpeg_hip_ts_mux_host` | %.3f (%.3f .. %.3f) |" % (r["host_mux_ms"], r["host_mux_min_ms"], r["host_mux_max_ms"]),
                     "| of (b): the call, `sync` and the 64 copies | %.3f |" % r["host_read_es_ms"],
                     "| of (b): the 64 host mux calls | %.3f |" % r["host_mux_only_ms"], "",
                     "A call's streams are %d bytes of ES and %d bytes of TS (%.4f times)." % (r["es_bytes_per_call"], r["ts_bytes_per_call"], r["ts_bytes_per_call"] / max(1, r["es_bytes_per_call"])), "",
                     "`timings()` of the same calls on two handles in one process, alternating, medians:", "",
                     "| | write, ms | total, ms |", "|---|---|---|",
                     "| TS on (write covers k_ts_units, k_ts_plan, k_ts_write) | %.3f | %.3f |" % (r["write_ms_ts_on"], r["total_ms_ts_on"]),
                     "| TS off | %.3f | %.3f |" % (r["write_ms_ts_off"], r["total_ms_ts_off"]), "",
                     "The same by the kind of call (the bytes above are a mean over all calls, the times medians), medians:", "",
                     "| | calls | ES bytes | TS bytes | (a), ms | (b), ms | of (b): call, sync, copies | of (b): host mux | write, TS on / off, ms | total, TS on / off, ms |",
                     "|---|---|---|---|---|---|---|---|---|---|"]
            lines += ["| %s | %d | %d | %d | %.3f | %.3f | %.3f | %.3f | %.3f / %.3f | %.3f / %.3f |" % (
                k["name"], k["calls"], k["es_bytes"], k["ts_bytes"], k["device_mux_one_copy_ms"], k["host_mux_ms"], k["host_read_es_ms"], k["host_mux_only_ms"],
                k["write_ms_ts_on"], k["write_ms_ts_off"], k["total_ms_ts_on"], k["total_ms_ts_off"]) for k in r["kinds"]] + [""]
        elif r["step"] == "chain":
            lines = ["## %s: %d streams of 1080p, one picture per stream per call, %d calls, gop %d, search range %d, target %d bytes per picture (measured on an MI355X by tools/encode_bench.py)"
                     % ("Chained calls" if r["chained"] else "The same calls WITHOUT chains (every picture an I picture)", r["streams"], r["calls"], r["gop"], r["search"], r["target"]), "",
                     "| | bytes per picture | of I pictures | of P pictures | call + sync, host clock, ms | device, median (min .. max), ms per call | calls with I pictures, ms | calls with P pictures, ms |",
                     "|---|---|---|---|---|---|---|---|"]
            for w in r["ways"]:
                lines.append("| %s | %d | %d | %s | %.3f | %.3f (%.3f .. %.3f) | %.3f | %s |" % (
                    w["name"], w["bytes_per_picture"], w["i_bytes_per_picture"], w["p_bytes_per_picture"] if w["p_bytes_per_picture"] is not None else "-", w["wall_ms"],
                    w["total_ms"], w["total_ms_min"], w["total_ms_max"], w["i_call_ms"], "%.3f" % w["p_call_ms"] if w["p_call_ms"] is not None else "-"))
            lines += ["", "Medians over %d measured calls each (%d rounds of %d behind one round to warm up)." % (r["ways"][0]["calls"], r["reps"], r["calls"]), ""]
        elif r["step"] == "rate":
            lines = ["## Cost on the MI355X: gop %d, search range %d, %d pictures of 1080p in %d streams, target %d bytes per picture (measured by tools/encode_bench.py)"
                     % (r["gop"], r["search"], r["pictures"], r["streams"], r["target"]), "",
                     "| | call + sync, host clock, ms | measure + scan (the level loop), ms | write, ms | total, median (min .. max), ms | output bytes | pictures' bytes of %d | over budget | mean q |" % (r["pictures"] * r["target"]),
                     "|---|---|---|---|---|---|---|---|---|"]
            for w in r["ways"]:
                lines.append("| %s | %.3f | %.3f | %.3f | %.3f (%.3f .. %.3f) | %d | %s | %s | %s |" % (
                    w["name"], w["wall_ms"], w["measure_scan_ms"], w["write_ms"], w["total_ms"], w["total_ms_min"], w["total_ms_max"], w["output_bytes"],
                    w.get("picture_bytes", ""), w.get("over_budget", ""), w.get("q_mean", "")))
            lines += ["", "| kernel | VGPRs | LDS bytes | occupancy (waves per SIMD) | scratch |", "|---|---|---|---|---|"]
            lines += ["| %s | %d | %d | %d | %d |" % (k, v["VGPRs"], v["LDS Size"], v["Occupancy"], v["ScratchSize"]) for k, v in r["kernels"].items()]
            lines.append("")
        elif r["step"] == "gop":
            lines = ["## gop %d, search range %d: %d pictures of 1080p in %d streams, q = %d (measured by tools/encode_bench.py)" % (r["gop"], r["search"], r["pictures"], r["streams"], r["q"]), "",
                     "| | ms |", "|---|---|",
                     "| call + sync, host clock | %.3f |" % r["wall_ms"],
                     "| timings: measure + scan (the level loop) | %.3f |" % r["measure_scan_ms"],
                     "| timings: write | %.3f |" % r["write_ms"],
                     "| timings: total, median (min .. max) | %.3f (%.3f .. %.3f) |" % (r["total_ms"], r["total_ms_min"], r["total_ms_max"]),
                     "| Batch.decode of the encoder's streams, host clock | %.3f |" % r["decode_of_output_wall_ms"], "",
                     "Output %d bytes.%s" % (r["output_bytes"], "  Macroblocks intra / coded / not coded / skipped: %s." % " / ".join(str(v) for v in r["kinds"]) if r["kinds"] else ""), ""]
        elif r["step"].startswith("pool"):
            lines += ["**%d pictures of 1080p into %d streams, q = %d, frames from a batch's pool** (cfg2 content)." % (r["pictures"], r["streams"], r["q"]), "",
                      "| | ms |", "|---|---|",
                      "| call + sync, host clock | %.3f |" % r["wall_ms"],
                      "| timings: convert | %.3f |" % r["convert_ms"],
                      "| timings: measure + scan | %.3f |" % r["measure_scan_ms"],
                      "| timings: write | %.3f |" % r["write_ms"],
                      "| timings: total | %.3f |" % r["total_ms"],
                      "| decode alone (whole pass, host clock) | %.3f |" % r["decode_alone_wall_ms"],
                      "| decode, then encode | %.3f |" % r["decode_then_encode_wall_ms"], "",
                      "Output %d bytes (%d per picture).  The two passes move %d bytes per picture (the frame read twice, 12 bytes per macroblock"
                      % (r["output_bytes"], r["output_bytes_per_picture"], r["moved_bytes_per_picture"]),
                      "out and in, the output cleared and written); a plain device copy ran at %.1f GB/s in the same process, which would move"
                      % r["copy_GBps"],
                      "them in %.3f ms: the call takes %.2f times that." % (r["copy_bound_ms"], r["ratio_to_copy_bound"]), ""]
        else:
            lines += ["**Tensor round trip** (`Batch.tensor(uint8)` -> `encode_tensor` -> decode, %s, %d pictures): luma PSNR against the first decode "
                      % (r["content"], r["pictures"]) + ", ".join("%.2f dB at q = %s" % (v, k[6:]) for k, v in r.items() if k.startswith("psnr_q")) + ".", ""]
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", default="pool64,pool7680,tensor")
    ap.add_argument("--reps", type=int, default=8)
    ap.add_argument("--gop", type=int, default=12, help="the gop step: GOP length (1: the intra pass)")
    ap.add_argument("--search", type=int, default=7, help="the gop step: full-pel search range 0 .. 15")
    ap.add_argument("--rate", type=int, default=40000, help="the rate step: target bytes per picture")
    ap.add_argument("--child")
    a = ap.parse_args()
    if a.child:
        r = step_ts(a.gop, a.search, a.reps) if a.child == "ts" else step_scale(a.gop, a.search, a.reps) if a.child == "scale" else step_chain(a.gop, a.search, a.rate, a.reps) if a.child == "chain" else step_rate(a.gop, a.search, a.rate, a.reps) if a.child == "rate" else step_gop(a.gop, a.search, a.reps) if a.child == "gop" else step_tensor() if a.child == "tensor" else step_pool(a.child == "pool7680", a.reps)
        print("RESULT " + json.dumps(r), flush=True)
        return 0
    results = []
    for step in a.steps.split(","):
        cmd = ["timeout", "-k", "10", str(STEPS[step]), sys.executable, os.path.abspath(__file__), "--child", step, "--reps", str(a.reps),
               "--gop", str(a.gop), "--search", str(a.search), "--rate", str(a.rate)]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
        if p.returncode != 0 or not line:
            print("step %s failed (exit status %d); stopping here\n%s" % (step, p.returncode, p.stdout[-3000:]), flush=True)
            break
        results.append(json.loads(line[-1][7:]))
        print(line[-1][7:], flush=True)
    done = len(results)
    from enc_quality import NOTES, replace_section
    for r in [r for r in results if r["step"] == "gop"]:
        replace_section(os.path.join(ROOT, "profiles", "enc_p_notes.md"), "bench_gop%d_r%d" % (r["gop"], r["search"]), notes([r]))
    for r in [r for r in results if r["step"] == "rate"]:
        replace_section(os.path.join(ROOT, "profiles", "enc_rate_notes.md"), "bench", notes([r]))
    for r in [r for r in results if r["step"] == "chain"]:
        replace_section(os.path.join(ROOT, "profiles", "enc_chain_notes.md"), "bench" if r["chained"] else "bench_unchained", notes([r]))
    for r in [r for r in results if r["step"] == "scale"]:
        replace_section(os.path.join(ROOT, "profiles", "enc_scale_notes.md"), "bench", notes([r]))
    for r in [r for r in results if r["step"] == "ts"]:
        replace_section(os.path.join(ROOT, "profiles", "enc_ts_notes.md"), "bench", notes([r]))
    results = [r for r in results if r["step"] not in ("gop", "rate", "chain", "scale", "ts")]
    if results:
        replace_section(NOTES, "bench", notes(results))
    return 0 if done == len(a.steps.split(",")) else 1


if __name__ == "__main__":
    sys.exit(main())
