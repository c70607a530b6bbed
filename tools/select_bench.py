"""What a pass over selected frames only (jsmpeg_hip_batch_select) is worth: ms per pass, MEASURED (the tests assert work done,
never times).  Two contents -- the headline's (64 x 120 pictures of 1080p, bench.py's generator, cfg2) and coded video (the
encoder GOPs of tests/golden/enc1080/ rotated into 64 streams of 10 GOPs, as bench.py rotates them) -- and on each
    whole        the whole pass, no selection
    last_of_gop  the last frame of one GOP per stream (the most a single frame can need)
    random_one   one random frame per stream
    eight_even   eight evenly spaced frames per stream (most GOPs are hit: little to gain)
through decode and enqueue: wall ms per pass (host clock around the call and its sync, median), the GPU's own span
(timings total_ms, median), needed / total pictures.  The selected pictures' device hashes are held against the whole pass's.

Two comparisons against code that is not the code under test (--baseline-lib: a library built from the parent commit, loaded
through JSMPEG_HIP_LIB in child processes of this tool):
    lower bound     the baseline library decoding a batch that holds ONLY the needed GOPs of the case: the selected pass should
                    come within the index's and the slice order's cost of it -- those still see all of the compressed data;
    no regression   the whole pass, baseline library against this tree's, in alternating processes (--alternate N).
k_select's own time: run the tool under `rocprofv3 --kernel-trace --stats` (a run of its own: --only cfg2 --cases last_of_gop
--reps 3) and hand the kernel_stats.csv it wrote to --kernel-stats.  One JSON line per content on stdout.
    python tools/select_bench.py [--only cfg2|coded] [--cases a,b] [--reps 12] [--baseline-lib variants/parent.so] [--alternate 3]
                                 [--kernel-stats file.csv]"""
import argparse
import csv
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
W, H = 1920, 1080
END = np.frombuffer(bytes([0, 0, 1, 0xB7]), np.uint8)
CASES = ("last_of_gop", "random_one", "eight_even")


def tolerate_older_library():
    """a baseline library has no selection symbols: the child process that loads it never calls them"""
    from jsmpeg_amd import build

    class Missing:
        def __init__(self, name):
            self.name = name

        def __call__(self, *a):
            raise RuntimeError("%s: not in the baseline library" % self.name)
    orig = build.load_hip_library

    def load(path=None):
        lib = orig(path)
        for name in ("jsmpeg_hip_batch_select", "jsmpeg_hip_batch_selected", "jsmpeg_hip_batch_select_info"):
            if not hasattr(lib, name):
                setattr(lib, name, Missing(name))
        return lib
    build.load_hip_library = load


def content(name):
    if name == "cfg2":
        import bench
        return [g[0] for g in bench.generate_streams(0, 64, 120)]
    import enc_content_bench as ecb
    files = ecb.gop_files()
    gops = [np.fromfile(files[k], dtype=np.uint8)[:-4] for k in sorted(files)]
    distinct = [np.concatenate([gops[(f + k) % len(gops)] for k in range(10)] + [END]) for f in range(len(gops))]
    return [distinct[s % len(distinct)] for s in range(64)]


def make_batch(streams, pictures):
    from jsmpeg_amd import batch as jb
    total = sum(len(s) for s in streams)
    return jb.Batch(W, H, len(streams), pictures + 8, total + 64 * len(streams) + 4096, device=0)


def measure(b, reps, enqueue):
    wall, gpu = [], []
    for r in range(reps + 2):
        t0 = time.perf_counter()
        if enqueue:
            if b.enqueue() != 0:
                raise RuntimeError("the batch was not planned on the device")
            b.sync()
        else:
            b.decode()
        t1 = time.perf_counter()
        if r >= 2:
            wall.append((t1 - t0) * 1e3)
            gpu.append(b.timings()["total_ms"])
    t = b.timings()
    return dict(wall_ms=round(float(np.median(wall)), 3), gpu_ms=round(float(np.median(gpu)), 3), wall_ms_min=round(min(wall), 3),
                phases_ms={k: round(float(v), 3) for k, v in t.items()})


def chains_of(info):
    """per stream: the GOP chains as lists of (frame number, picture, es_offset)"""
    out = {}
    frame = {}
    for p, i in enumerate(info):
        if not i.decoded:
            continue
        f = frame.get(i.stream, 0)
        frame[i.stream] = f + 1
        ch = out.setdefault(i.stream, [])
        if i.forward < 0 or not ch:
            ch.append([])
        ch[-1].append((f, p, i.es_offset))
    return out


def requests_of(case, chains, rng):
    reqs = []
    for s, ch in sorted(chains.items()):
        n = sum(len(c) for c in ch)
        if case == "last_of_gop":
            reqs.append((s, ch[int(rng.integers(0, len(ch)))][-1][0]))
        elif case == "random_one":
            reqs.append((s, int(rng.integers(0, n))))
        else:
            reqs += [(s, (2 * k + 1) * n // 16) for k in range(8)]
    return reqs


def needed_gops_only(streams, chains, reqs):
    """per stream: its bytes in front of the first picture (the sequence header) and the GOPs that hold a requested frame"""
    want = {}
    for s, f in reqs:
        want.setdefault(s, set()).add(f)
    out, pictures = [], 0
    for s, es in enumerate(streams):
        ch = chains.get(s, [])
        starts = [c[0][2] for c in ch] + [len(es)]
        pieces = [es[:starts[0]]] if ch else []
        for k, c in enumerate(ch):
            if any(f in want.get(s, ()) for f, _, _ in c):
                pieces.append(es[starts[k]:starts[k + 1]])
                pictures += len(c)
        if not pieces:
            continue
        out.append(np.concatenate(pieces + [END]))
    return out, pictures


def run_content(name, cases, reps, seed=20261016):
    """this tree: the whole pass, then every case selected; returns the JSON line's dict and what the baseline child needs"""
    streams = content(name)
    rng = np.random.default_rng(seed)
    res = {"content": "%s 1080p, %d streams" % ("cfg2 64 x 120" if name == "cfg2" else "coded video 64 x 10 GOPs", len(streams)), "cases": {}}
    sub = {}
    with make_batch(streams, 64 * 130) as b:
        b.upload(streams)
        b.decode()
        info = b.pictures()
        whole_hash = [int(h) for h in b.frame_hashes()]
        chains = chains_of(info)
        total = sum(i.decoded for i in info)
        res["pictures"] = total
        res["cases"]["whole"] = dict(needed=total, decode=measure(b, reps, False), enqueue=measure(b, reps, True))
        for case in cases:
            reqs = requests_of(case, chains, rng)
            b.select(reqs)
            row = dict(requests=len(reqs), decode=measure(b, reps, False))
            si = b.select_info()
            sel = b.selected()
            got = b.frame_hashes()
            bad = [p for p in sel if p is not None and int(got[p]) != whole_hash[p]]
            if bad:
                raise RuntimeError("PARITY FAILURE: selected pictures %s differ from the whole pass's" % bad[:8])
            row["enqueue"] = measure(b, reps, True)
            got = b.frame_hashes()
            if [p for p in sel if p is not None and int(got[p]) != whole_hash[p]]:
                raise RuntimeError("PARITY FAILURE (enqueue): selected pictures differ from the whole pass's")
            row.update(needed=si["needed"], selected=si["selected"], widened_streams=b.select_info()["widened_streams"],
                       recon_info=b.recon_info())
            res["cases"][case] = row
            sub[case] = needed_gops_only(streams, chains, reqs)
            b.select(None)
    return res, streams, sub


def baseline_child(name, cases, reps, seed):
    """(a child process with the baseline library loaded) the whole pass, and per case a batch of the needed GOPs only"""
    tolerate_older_library()
    # the same requests as the parent process drew: this tree's rules are not involved in cutting the streams
    streams = content(name)
    rng = np.random.default_rng(seed)
    out = {}
    with make_batch(streams, 64 * 130) as b:
        b.upload(streams)
        b.decode()
        chains = chains_of(b.pictures())
        out["whole"] = dict(decode=measure(b, reps, False), enqueue=measure(b, reps, True))
    for case in cases:
        sub, pictures = needed_gops_only(streams, chains, requests_of(case, chains, rng))
        with make_batch(sub, pictures) as b:
            b.upload(sub)
            b.decode()
            assert b.counters()["decoded"] == pictures, (b.counters(), pictures)
            out[case] = dict(pictures=pictures, decode=measure(b, reps, False), enqueue=measure(b, reps, True))
    print("BASELINE " + json.dumps(out), flush=True)


def whole_child(name, reps):
    tolerate_older_library()
    streams = content(name)
    with make_batch(streams, 64 * 130) as b:
        b.upload(streams)
        print("WHOLE " + json.dumps(dict(decode=measure(b, reps, False), enqueue=measure(b, reps, True))), flush=True)


def child(args, lib, tag):
    env = dict(os.environ)
    if lib:
        env["JSMPEG_HIP_LIB"] = os.path.abspath(lib)
    else:
        env.pop("JSMPEG_HIP_LIB", None)
    r = subprocess.run([sys.executable, os.path.abspath(__file__)] + args, env=env, capture_output=True, text=True, timeout=900)
    for ln in r.stdout.splitlines():
        if ln.startswith(tag + " "):
            return json.loads(ln[len(tag) + 1:])
    raise RuntimeError("child %r failed: %s" % (args, (r.stdout + r.stderr)[-1500:]))


def kernel_stats(path):
    rows = {}
    for row in csv.DictReader(open(path)):
        name = row.get("Name") or row.get("KernelName") or ""
        for k in ("k_select", "k_index", "k_order_count", "k_order_place", "k_scan", "k_plan", "k_to_host"):
            if k in name:
                rows[k] = dict(calls=int(row["Calls"]), avg_us=round(float(row["AverageNs"]) / 1e3, 2))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", choices=("cfg2", "coded"))
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--reps", type=int, default=12)
    ap.add_argument("--baseline-lib")
    ap.add_argument("--alternate", type=int, default=0)
    ap.add_argument("--kernel-stats")
    ap.add_argument("--role", choices=("baseline", "whole"))
    ap.add_argument("--seed", type=int, default=20261016)
    a = ap.parse_args()
    cases = [c for c in a.cases.split(",") if c]
    if a.role == "baseline":
        return baseline_child(a.only, cases, a.reps, a.seed)
    if a.role == "whole":
        return whole_child(a.only, a.reps)
    for name in ("cfg2", "coded"):
        if a.only and a.only != name:
            continue
        res, _, _ = run_content(name, cases, a.reps, a.seed)
        common = ["--only", name, "--reps", str(a.reps), "--seed", str(a.seed)]
        if a.baseline_lib:
            res["baseline_needed_gops_only"] = child(common + ["--role", "baseline", "--cases", ",".join(cases)], a.baseline_lib, "BASELINE")
            if a.alternate:
                res["whole_pass_alternating"] = [dict(baseline=child(common + ["--role", "whole"], a.baseline_lib, "WHOLE"),
                                                      this_tree=child(common + ["--role", "whole"], None, "WHOLE")) for _ in range(a.alternate)]
        if a.kernel_stats:
            res["kernel_stats_us"] = kernel_stats(a.kernel_stats)
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
