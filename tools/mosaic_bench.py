"""A wall of cameras on the device: 16 live 1080p streams composed into ONE 1920x1080 encoder, 4 x 4 cells of 480x270, one
picture per tick, chained, gop 12, search range 7, q = 8.  First one tick's Encoder.source(0) is held against the numpy
restatement (tests/enc_mosaic_ref.py) over the tick's pictures.  Then three ways are timed after every tick of the same
process, alternating, medians over `--reps` rounds of 12 ticks behind one round to warm up:
  (a) Encoder.encode_mosaic_latest: the planes composed by k_enc_mosaic;
  (b) what there was before: Live.latest_tensor(uint8, 480x270), the torch reshape into the wall, Encoder.encode_tensor;
  (c) Encoder.encode_scaled of the same 16 frames into a 480x270 encoder of 16 streams: the same source bytes read and the same
      number of plane bytes written as (a) by k_enc_scale -- only "convert" is compared.
(c) is the yardstick for the kernel, (b) for the feature.  A control, (a'): the same 16 sources in cells of 384x256 at multiples
of the kernel's 128 x 32 tile, so that no tile meets two cells -- what the cells' edges inside tiles cost (a).  With --loss (no device): what the wall loses on the route through
RGB, from the CPU restatements, in the way of tools/enc_scale_loss.py.  Writes the bench / loss sections of
profiles/enc_mosaic_notes.md.
    python tools/mosaic_bench.py [--reps 3]
    python tools/mosaic_bench.py --loss"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
W, H, COLS, ROWS, CW, CH = 1920, 1080, 4, 4, 480, 270
GOP, SEARCH, Q = 12, 7, 8
NOTES = os.path.join(ROOT, "profiles", "enc_mosaic_notes.md")


def bench(reps):
    import torch
    import bench as flagship
    import enc_mosaic_ref as em
    from encode_bench import copy_rate, median
    from enc_quality import replace_section
    from jsmpeg_amd import build, encode
    from jsmpeg_amd import live as jl
    usage = build.check_kernel_resources()
    figures = {k: {n: v[n] for n in ("VGPRs", "LDS Size", "Occupancy", "ScratchSize")} for k in ("k_enc_mosaic", "k_enc_scale")
               for name, v in usage.items() if k in name}
    n, ticks = COLS * ROWS, GOP * (reps + 1)
    made = flagship.generate_streams(0, n, ticks)
    cells = encode.grid(COLS, ROWS, (W, H), (W, H))
    as_tuples = [(W, H, None, 1, c.x, c.y, c.width, c.height) for c in cells]
    with jl.Live(W, H, n, pictures_per_tick=1, store_bytes=4 << 20, device=0) as lv, encode.Encoder(W, H, 1, 1, 16 << 20, device=0) as a, \
            encode.Encoder(W, H, 1, 1, 16 << 20, device=0) as b, encode.Encoder(CW, CH, n, n, 16 << 20, device=0) as c, \
            encode.Encoder(W, H, 1, 1, 16 << 20, device=0) as d:
        ids = [lv.open() for _ in range(n)]
        sources = [(lv, i) for i in ids]
        for enc in (a, b, c, d):
            enc.set_gop(GOP, SEARCH)
        a.set_mosaic(cells)
        d.set_mosaic([encode.cell((W, H), 384 * (k % COLS), 256 * (k // COLS), 384, 256) for k in range(n)])
        rate = copy_rate(lv.L, 1 << 30, 8)
        moved = n * (W * H * 3 // 2) + a.frame_bytes
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        rows = {k: dict(convert=[], total=[], wall=[], bytes=[]) for k in "abcd"}
        for t in range(ticks):
            for k, i in enumerate(ids):
                es, offs = made[k][0], made[k][1]
                lv.write(i, es[int(offs[t]):int(offs[t + 1])], pts=t / 30.0)
            assert lv.tick(flush=True) == n, "a picture per stream per tick"
            if t == 0:                                                      # the planes against the restatement, once
                host = lv.read_frames()
                by_stream = {p.stream: host[k] for k, p in enumerate(lv.pictures())}
                assert a.encode_mosaic_latest(sources, qscale=Q, end=False) == [True] * n
                got = np.concatenate([p.ravel() for p in a.source(0)])
                want = em.compose(as_tuples, [full_frame(by_stream[i], lv) for i in ids], W, H)
                assert np.array_equal(got, want), "the composed planes differ from the restatement in %d bytes" % int(np.count_nonzero(got != want))
                print("tick 0: source(0) equals the restatement (%d bytes)" % got.size, flush=True)
            keep = t >= GOP
            last = False                                                    # the chains go on: a relay never ends its streams
            # (a)
            t0 = time.perf_counter()
            a.encode_mosaic_latest(sources, qscale=Q, end=last, chain=True)
            a.sync()
            wa, ma = (time.perf_counter() - t0) * 1e3, a.timings()
            # (b)
            t0 = time.perf_counter()
            e0.record()
            x, have = lv.latest_tensor(ids, size=(CH, CW), dtype=torch.uint8)
            wall = x.view(ROWS, COLS, 3, CH, CW).permute(2, 0, 3, 1, 4).reshape(1, 3, ROWS * CH, COLS * CW).contiguous()
            e1.record()
            b.encode_tensor(wall, qscale=Q, end=last, chain=True)
            b.sync()
            wb, mb, render = (time.perf_counter() - t0) * 1e3, b.timings(), e0.elapsed_time(e1)
            # (c)
            t0 = time.perf_counter()
            c.encode_scaled(lv.latest_frames(ids), (W, H), streams=list(range(n)), qscale=Q, end=last, chain=True)
            c.sync()
            wc, mc = (time.perf_counter() - t0) * 1e3, c.timings()
            # (a'), the control
            t0 = time.perf_counter()
            d.encode_mosaic_latest(sources, qscale=Q, end=last, chain=True)
            d.sync()
            wd, md = (time.perf_counter() - t0) * 1e3, d.timings()
            if keep:
                for k, cv, tot, wl, enc in (("d", md["convert_ms"], md["total_ms"], wd, d),
                                            ("a", ma["convert_ms"], ma["total_ms"], wa, a), ("b", mb["convert_ms"] + render, mb["total_ms"] + render, wb, b),
                                            ("c", mc["convert_ms"], mc["total_ms"], wc, c)):
                    rows[k]["convert"].append(cv); rows[k]["total"].append(tot); rows[k]["wall"].append(wl)
                    rows[k]["bytes"].append(sum(v for _, v in enc.picture_ranges()))
    med = {k: {m: median(v[m]) for m in ("convert", "total", "wall")} for k, v in rows.items()}
    names = {"a": "(a) encode_mosaic_latest", "b": "(b) latest_tensor(uint8, 480x270) + reshape + encode_tensor", "c": "(c) encode_scaled, 16 x 480x270",
             "d": "(a') control: cells of 384x256 at multiples of the tile"}
    bound = moved / (rate * 1e9) * 1e3
    lines = ["## The wall: 16 live streams of 1080p into one 1920x1080 picture, 4 x 4 cells of 480x270, one picture per tick, chained, gop %d, search range %d, q = %d (measured on an MI355X by tools/mosaic_bench.py)" % (GOP, SEARCH, Q), "",
             "One tick's `source(0)` equalled the numpy restatement over the tick's pictures before anything was timed.  The composition reads and writes %d bytes per picture; a plain device copy ran at %.1f GB/s in the same process and would move them in %.3f ms." % (moved, rate, bound), "",
             "| | planes ready (convert), median (min .. max), ms | call total on the device, ms | call + sync, host clock, ms | bytes per picture |", "|---|---|---|---|---|"]
    for k in "abcd":
        lines.append("| %s | %.3f (%.3f .. %.3f) | %s | %.3f | %d |" % (names[k], med[k]["convert"], min(rows[k]["convert"]), max(rows[k]["convert"]),
                                                                     "-" if k in "cd" else "%.3f" % med[k]["total"], med[k]["wall"], round(float(np.mean(rows[k]["bytes"])))))
    lines += ["", "a / b: %.2f (convert), %.2f (call total).  a / c (convert): %.2f.  (a) takes %.2f times the copy's time.  a' / c (convert): %.2f."
              % (med["a"]["convert"] / med["b"]["convert"], med["a"]["total"] / med["b"]["total"], med["a"]["convert"] / med["c"]["convert"], med["a"]["convert"] / bound, med["d"]["convert"] / med["c"]["convert"]), "",
              "(b)'s convert is the device time of `latest_tensor` and the reshape (torch events) plus the encoder's own; (c) writes 16 pictures of 480x272, (a) one of 1920x1088 (the same display samples).",
              "Medians over %d measured ticks each (%d rounds of %d behind one round to warm up), the three ways after the same tick, alternating."
              % (len(rows["a"]["convert"]), reps, GOP),
              " ".join("%s: %d VGPRs, %d bytes of LDS, occupancy %d, scratch %d." % (k, v["VGPRs"], v["LDS Size"], v["Occupancy"], v["ScratchSize"]) for k, v in sorted(figures.items())), ""]
    replace_section(NOTES, "bench", "\n".join(lines))
    print("\n".join(lines))


def full_frame(planes, lv):
    """a tick's picture as read_frames hands it out (Y | Cr | Cb of the coded size)"""
    assert len(planes) == lv.luma_bytes + 2 * lv.chroma_bytes
    return np.array(planes)


def loss():
    """the two 1080p content frames as the wall's cells: every cell directly by the rule against the route through RGB"""
    import enc_scale_inputs as si
    import enc_scale_ref as es
    from enc_quality import replace_section
    from enc_scale_loss import rgb_route
    frames = si.case_frames("7_1080p_to_640x360")
    d = {"Y": [], "Cr": [], "Cb": []}
    for f in frames:
        x = es.source_planes(es.scale_frame(f, W, H, CW, CH), CW, CH)
        y = es.source_planes(rgb_route(f, CW, CH), CW, CH)
        for name, pa, pb, (pw, ph) in zip(("Y", "Cr", "Cb"), x, y, ((CW, CH), (CW // 2, CH // 2), (CW // 2, CH // 2))):
            d[name].append(np.abs(pa[:ph, :pw].astype(np.int32) - pb[:ph, :pw].astype(np.int32)))
    lines = ["## What the wall loses on the route through RGB (CPU restatements only, measured by tools/mosaic_bench.py --loss)", "",
             "A cell of the wall is 1080p scaled to 480x270; cell sizes and origins are even, so neither route mixes samples of two cells and the wall's",
             "loss is its cells'.  The two 1080p content frames, directly by the rule and through `latest_tensor(uint8)` + `encode_tensor` (integer BT.601",
             "to RGB, torch's antialiased resize, uint8, RGB back to Y | Cr | Cb with the chroma averaged 2x2).  Absolute difference over the cell:", "",
             "| plane | mean | max |", "|---|---|---|"]
    for name in ("Y", "Cr", "Cb"):
        v = np.concatenate([x.ravel() for x in d[name]])
        lines.append("| %s | %.3f | %d |" % (name, float(v.mean()), int(v.max())))
    replace_section(NOTES, "loss", "\n".join(lines + [""]))
    print("\n".join(lines))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--loss", action="store_true")
    args = ap.parse_args()
    if args.loss:
        loss()
    else:
        if args.reps < 3:
            ap.error("--reps: at least three rounds")
        bench(args.reps)
    return 0


if __name__ == "__main__":
    sys.exit(main())
