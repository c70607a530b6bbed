"""One thread, N batches in flight through jsmpeg_hip_batch_enqueue, against the blocking decode one batch at a time and two
host threads (bench.py's two_batches_in_flight, imported, unchanged), on cfg2 (64 x 120 pictures of 1080p, bench.py's
generator) and on coded video (tools/enc_content_bench.py's encoder GOPs, 64 streams of 10).  Every pool of every run is gated
against the oracle's hashes.  Also: what the padding of the enqueued reconstruct's grid costs (the launch with the batch's
capacity at n + 8 pictures, as bench.py creates it, against 2 n: the slope per empty workgroup, times the n + 8 grid's empty
workgroups).  One JSON line per workload on stdout.
    python tools/enqueue_bench.py [--only cfg2|coded] [--passes 12]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def per_stream(b):
    dev, per = b.frame_hashes(), {}
    for p, i in enumerate(b.pictures()):
        per.setdefault(i.stream, []).append(int(dev[p]))
    return per


def gate(b, want, what):
    per = per_stream(b)
    bad = [s for s, w in enumerate(want) if per.get(s, []) != w]
    if bad:
        raise RuntimeError("PARITY FAILURE against the oracle (%s) on streams %s" % (what, bad[:8]))


def one_at_a_time(b, n_pictures, passes):
    b.decode()
    t0 = time.perf_counter()
    for _ in range(passes):
        b.decode()
    return n_pictures * passes / (time.perf_counter() - t0)


def in_flight(make_batch, streams, n_pictures, want, k, passes):
    """k batch objects on k HIP streams, ONE host thread: enqueue them all, then settle the oldest and enqueue it again"""
    import torch
    bs = [make_batch() for _ in range(k)]
    try:
        sts = [torch.cuda.Stream() for _ in range(k)]
        for bb, st in zip(bs, sts):
            bb.upload(streams)
            if bb.enqueue(stream=st.cuda_stream) != 0:
                raise RuntimeError("the batch was not planned on the device")
            bb.sync()
        info = bs[0].recon_info()
        for bb, st in zip(bs, sts):
            bb.enqueue(stream=st.cuda_stream)
        done, t0 = 0, None
        for i in range(passes * k + k):
            bb, st = bs[i % k], sts[i % k]
            bb.sync()
            if i == k - 1:
                t0 = time.perf_counter()          # (steady state: from the end of the first round of passes)
            elif i >= k:
                done += 1
            if i < passes * k:
                bb.enqueue(stream=st.cuda_stream)
        dt = time.perf_counter() - t0
        for bb in bs:
            gate(bb, want, "%d in flight" % k)
        return n_pictures * done / dt, info
    finally:
        for bb in bs:
            bb.close()


def padding_cost(make_batch_cap, streams, n_pictures, reps=6):
    """recon_ms of the enqueued launch at capacity n + 8 (bench.py's) and 2 n: 8 x rows_cap slots each, n_pictures of them pictures"""
    out = {}
    for cap in (n_pictures + 8, 2 * n_pictures):
        with make_batch_cap(cap) as b:
            b.upload(streams)
            ms = []
            for r in range(reps + 2):
                b.enqueue()
                b.sync()
                if r >= 2:
                    ms.append(b.timings()["recon_ms"])
            out[cap] = dict(recon_ms=float(np.median(ms)), slots=8 * (cap * 108 // 800), status=b.recon_info()["status"])
    return out[n_pictures + 8], out[2 * n_pictures]


def oracle_hashes(streams):
    from concurrent.futures import ThreadPoolExecutor
    from jsmpeg_amd import build, cabi, hashing
    olib = build.LIB_ORACLE if os.path.exists(build.LIB_ORACLE) else build.build_oracle()
    with ThreadPoolExecutor(16) as ex:
        return list(ex.map(lambda es: [hashing.frame_hash(*f) for f in cabi.decode_stream(olib, es, keep="planes")[0]], streams))


def workload(name, streams, want, width, height, passes):
    import bench
    from jsmpeg_amd import batch as jb
    n_pictures = sum(len(w) for w in want)
    total = sum(len(s) for s in streams)

    def make_batch_cap(cap):
        return jb.Batch(width, height, len(streams), cap, total + 64 * len(streams) + 4096, device=0)

    def make_batch():
        return make_batch_cap(n_pictures + 8)
    res = {"workload": name, "pictures_per_pass": n_pictures, "unit": "frames/s"}
    with make_batch() as b:
        b.upload(streams)
        res["one_at_a_time"] = round(one_at_a_time(b, n_pictures, passes), 1)
        gate(b, want, "decode")
        t = bench.two_batches_in_flight(b, make_batch, lambda bb, st: bb.upload(streams), n_pictures, want, passes=passes)
        res["two_threads"] = t["value"]
    for k in (2, 3):
        v, info = in_flight(make_batch, streams, n_pictures, want, k, passes)
        res["one_thread_%d_in_flight" % k] = round(v, 1)
        res["enqueued_recon_info"] = info
    lo, hi = padding_cost(make_batch_cap, streams, n_pictures)
    res["padding"] = {"capacity_n_plus_8": lo, "capacity_2n": hi,
                      "note": "recon_ms of the enqueued ordered launch; slots = 8 x rows_cap, of which n_pictures hold pictures"}
    if hi["slots"] > lo["slots"]:
        per_slot = (hi["recon_ms"] - lo["recon_ms"]) / (hi["slots"] - lo["slots"])
        pad = per_slot * (lo["slots"] - n_pictures)
        res["padding"]["ms_per_padding_slot"] = per_slot
        res["padding"]["share_of_recon_at_n_plus_8"] = round(pad / lo["recon_ms"], 5) if lo["recon_ms"] > 0 else None
    res["parity"] = "every pool of every run (decode, two threads, 2 / 3 in flight): device hash == oracle, every picture"
    return res


def cfg2(passes):
    import bench
    streams = [g[0] for g in bench.generate_streams(0, 64, 120)]
    return workload("cfg2_1080p 64 x 120", streams, oracle_hashes(streams), 1920, 1080, passes)


def coded(passes):
    import enc_content_bench as ecb
    files = ecb.gop_files()
    gops = [np.fromfile(files[k], dtype=np.uint8)[:-4] for k in sorted(files)]
    end = np.frombuffer(ecb.END, np.uint8)
    distinct = [np.concatenate([gops[(f + k) % len(gops)] for k in range(10)] + [end]) for f in range(len(gops))]
    want_d = oracle_hashes(distinct)
    streams = [distinct[s % len(distinct)] for s in range(64)]
    want = [want_d[s % len(distinct)] for s in range(64)]
    return workload("coded video 1080p 64 x 10 GOPs", streams, want, 1920, 1080, passes)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", choices=("cfg2", "coded"))
    ap.add_argument("--passes", type=int, default=12)
    a = ap.parse_args()
    for name, fn in (("coded", coded), ("cfg2", cfg2)):
        if a.only and a.only != name:
            continue
        print(json.dumps(fn(a.passes)), flush=True)


if __name__ == "__main__":
    main()
