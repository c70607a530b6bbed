"""What one RELAY TICK costs from the calls to every stream's program on the host, MEASURED (the tests assert bytes, never
times): 64 streams, one picture (--size, gop 12, chained) and the tick's audio frames (--frames per stream, stereo 44.1 kHz
192 kbit/s, chained) per stream and tick.  Two ways, alternating tick by tick in one process:
  (a) Encoder.encode, Mp2Encoder.encode, TsProgram.mux_encoders on one HIP stream, then ONE read-back (TsProgram.ts_all);
  (b) what the library offered before part 10: Encoder.set_ts (TS on the device behind the pass), Mp2Encoder.encode, then
      jsmpeg_hip_ts_mux_device over the audio frames (synchronous), TWO read-backs, and an interleave by PES on the host (here
      in Python over numpy views: packets are self-contained, so whole PES are copied in PTS order).
(b) carries no PAT / PMT / PCR: it is the cheaper stream.  Host wall time per tick, median over --reps ticks after --warmup.
The figures go to profiles/ts_program_notes.md.
    python tools/ts_program_bench.py [--size 640x360] [--streams 64] [--frames 2] [--reps 20] [--warmup 4]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def pes_list(ts):
    """[(pts, first byte, end byte)] of the PES in one PID's packets: a PES begins at a packet with payload_unit_start"""
    starts = [p for p in range(0, len(ts), 188) if ts[p + 1] & 0x40] + [len(ts)]
    out = []
    for b, e in zip(starts[:-1], starts[1:]):
        h = b + 4 + (1 + ts[b + 4] if ts[b + 3] & 0x20 else 0)
        pts = ((ts[h + 9] >> 1) & 7) << 30 | ts[h + 10] << 22 | (ts[h + 11] >> 1) << 15 | ts[h + 12] << 7 | ts[h + 13] >> 1
        out.append((pts, b, e))
    return out


def interleave(video, audio):
    """one stream's two TS merged by PES in PTS order, video first at a tie"""
    units = [(pts, 0, video[b:e]) for pts, b, e in pes_list(video)] + [(pts, 1, audio[b:e]) for pts, b, e in pes_list(audio)]
    return b"".join(u[2] for u in sorted(units, key=lambda u: (u[0], u[1])))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="640x360")
    ap.add_argument("--streams", type=int, default=64)
    ap.add_argument("--frames", type=int, default=2)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=4)
    args = ap.parse_args()
    import torch

    import enc_p_inputs as ep
    import mp2_enc_inputs as minputs
    from jsmpeg_amd import encode, mp2_encode, ts_program
    w, h = (int(v) for v in args.size.split("x"))
    ns, nf, ticks = args.streams, args.frames, args.reps + args.warmup
    pictures = torch.from_numpy(np.ascontiguousarray(np.stack(ep.pan_frames(w, h, 8, (3, -2))))).cuda()      # eight pictures, shown in a cycle
    pcm = torch.from_numpy(np.ascontiguousarray(minputs.pcm("noise", 44100, nf * ticks, seed=3), dtype=np.float32)).cuda()
    torch.cuda.synchronize()
    streams = list(range(ns))
    es_cap = ns * (pictures.shape[1] * 2 + 4096)
    a_cap = mp2_encode.es_bytes([nf] * ns, 0, 10) + ns * (nf + 16)          # (a frame's padding byte depends on its ordinal)
    ts_cap = ts_program.program_bound(es_cap, ns, a_cap, ns * nf, ns)
    kw = dict(max_pictures=ns, max_streams=ns, max_es_bytes=es_cap)
    with encode.Encoder(w, h, **kw) as enc_a, encode.Encoder(w, h, **kw) as enc_b, \
            mp2_encode.Mp2Encoder(0, 2, 10, ns, ns * nf, a_cap) as aenc_a, mp2_encode.Mp2Encoder(0, 2, 10, ns, ns * nf, a_cap) as aenc_b, \
            ts_program.TsProgram(ts_program.config(ns, ns, ns * nf, ts_cap, pcr_lead_90k=9000)) as prog:
        for e in (enc_a, enc_b):
            e.set_gop(12, 7)
        enc_b.set_ts(encode.ts_bound(es_cap, ns, ns))
        a_ts_cap = encode.ts_bound(a_cap, ns * nf, ns)
        a_out = torch.zeros(a_ts_cap, dtype=torch.uint8, device="cuda")
        cc, ms_a, ms_b, bytes_a, bytes_b, mux_ms = None, [], [], 0, 0, []
        for k in range(ticks):
            frame = [pictures.data_ptr() + (k % 8) * pictures.shape[1]] * ns
            sound = [pcm.data_ptr() + k * nf * 2 * 1152 * 4] * ns
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            enc_a.encode(frame, streams, 8, end=False, chain=True)
            aenc_a.encode(sound, [nf] * ns, chain=True)
            prog.mux_encoders(enc_a, aenc_a)
            got_a = prog.ts_all()
            enc_a.sync()                                       # (done long since: the program ran behind them; frees the handles for the next tick)
            aenc_a.sync()
            t1 = time.perf_counter()
            enc_b.encode(frame, streams, 8, end=False, chain=True)
            aenc_b.encode(sound, [nf] * ns, chain=True)
            ranges, seconds, numbers = aenc_b.ts_units()
            dev_es, _ = aenc_b.device_es()
            n, where, cc = encode.ts_mux_device(dev_es, ranges, seconds, a_out.data_ptr(), a_ts_cap, numbers, ns, stream_id=0xC0, pid=0x101, continuity=cc)
            v_whole, v_ranges = enc_b.ts_all()
            a_whole = a_out[:n].cpu().numpy().tobytes()
            v_whole = bytes(v_whole)
            got_b = {s: interleave(v_whole[v_ranges[s][0]:v_ranges[s][1]], a_whole[where[s][0]:where[s][1]]) for s in streams}
            t2 = time.perf_counter()
            if k >= args.warmup:
                ms_a.append((t1 - t0) * 1e3)
                ms_b.append((t2 - t1) * 1e3)
                mux_ms.append(prog.timings()["mux_ms"])
                bytes_a, bytes_b = sum(len(v) for v in got_a.values()), sum(len(v) for v in got_b.values())
        print(json.dumps(dict(size=args.size, streams=ns, audio_frames_per_stream=nf, reps=args.reps,
                              a_mux_encoders_one_read_ms=round(float(np.median(ms_a)), 3), b_two_buffers_host_interleave_ms=round(float(np.median(ms_b)), 3),
                              a_mux_kernels_ms=round(float(np.median(mux_ms)), 4), a_bytes_per_tick=bytes_a, b_bytes_per_tick=bytes_b)))


if __name__ == "__main__":
    main()
