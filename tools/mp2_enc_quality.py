#!/usr/bin/env python3
"""The yardstick of the MP2 encoder's round trip: THIS encoder restated in float64 -- a real-valued analysis filterbank with the
same window, the same scalefactor and allocation rule, and an ideal nearest-level quantiser over the decoder's levels -- decoded
by the oracle decoder, SNR against the input.  Written apart from jsmpeg_amd/csrc/mp2_enc.h (it shares the table rules and the
bit writer with the numpy restatement tests/mp2_enc_ref.py, not a line with the header).  tests/test_mp2_enc_sim.py holds the
integer encoder to these figures minus 1 dB per (configuration, input).

The decoder returns HALF of ISO's level (include/jsmpeg_hip.h part 9), 481 samples late: the SNR is that of twice the decoded
signal, delayed input as the reference, over the channels the handle codes.

    python tools/mp2_enc_quality.py            # writes profiles/mp2_enc_bounds.json (with tools/mp2_enc_bounds.py's figures)
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import mp2_enc_ref as ref            # noqa: E402  (table rules, bit writer)
import mp2_enc_inputs as inputs      # noqa: E402
import mp2_enc_bounds                # noqa: E402

LAG = 481
GAIN = 2.0
OUT = os.path.join(ROOT, "profiles", "mp2_enc_bounds.json")


def clean(x):
    """the input as the encoder hears it, in float64: NaN -> 0, clamped to full scale"""
    return np.clip(np.nan_to_num(np.asarray(x, np.float64), nan=0.0, posinf=1.0, neginf=-1.0), -1.0, 1.0)


def snr_db(x, decoded, channels):
    """x, decoded: [frames][2][1152]; SNR of GAIN * decoded against x delayed by LAG, over the coded channels; None for silence"""
    num = den = 0.0
    for c in range(channels):
        a = clean(x[:, c, :]).reshape(-1)
        d = GAIN * np.asarray(decoded[:, c, :], np.float64).reshape(-1)
        a, d = a[:len(a) - LAG], d[LAG:]
        num += float((a * a).sum())
        den += float(((d - a) ** 2).sum())
    if num == 0.0:
        return None
    return 10.0 * np.log10(num / max(den, 1e-300))


def float_encode(cfg, pcm):
    """the float64 restatement: pcm float32 [frames][2][1152] -> bytes"""
    sr, ch_n, br = cfg
    sblimit, high = ref.table_select(sr, ch_n, br)
    W = ref.W.astype(np.float64)
    cosm = np.array([[np.cos((2 * k + 1) * (i - 16) * np.pi / 64.0) for i in range(64)] for k in range(32)])
    sf = ref.SCALEFACTORS.astype(np.float64)
    hist = np.zeros((2, 480))
    out = []
    for f in range(len(pcm)):
        x = np.concatenate([hist, clean(pcm[f]) * 32767.0], axis=1)
        hist = x[:, 1152:]
        size = ref.frame_bytes(sr, br, f)
        idx = 480 + 32 * np.arange(36)[:, None] + 31 - np.arange(512)[None, :]
        S = np.stack([((W[None, :] * x[c][idx]).reshape(36, 8, 64).sum(axis=1) @ cosm.T) / 8192.0 for c in range(ch_n)])
        pairs = [(sb, c) for sb in range(sblimit) for c in range(ch_n)]
        index, silent, sel, nsf = {}, {}, {}, {}
        for p in pairs:
            M = [float(np.abs(S[p[1], 12 * t:12 * t + 12, p[0]]).max()) for t in range(3)]
            index[p] = [int(np.nonzero(sf >= 2.0 * m)[0][-1]) if (sf >= 2.0 * m).any() else 0 for m in M]
            silent[p] = not any(M)
            a, b, c3 = index[p]
            sel[p] = 2 if a == b == c3 else (1 if a == b else (3 if b == c3 else 0))
            nsf[p] = {0: 3, 1: 2, 2: 1, 3: 2}[sel[p]]
        code = {p: 0 for p in pairs}
        left = 8 * size - 32 - sum(ref.nbal(high, sb) for sb, _ in pairs)
        while True:
            best = None
            for p in pairs:
                if silent[p] or code[p] >= (1 << ref.nbal(high, p[0])) - 1:
                    continue
                so, sn = ref.steps_of(high, p[0], code[p]), ref.steps_of(high, p[0], code[p] + 1)
                cost = 12 * (ref.granule_bits(sn) - ref.granule_bits(so)) + (2 + 6 * nsf[p] if code[p] == 0 else 0)
                key = (-8 * min(index[p]) - ref.gain(so), -p[0], -p[1])
                if cost <= left and (best is None or key > best[0]):
                    best = (key, p, cost)
            if best is None:
                break
            code[best[1]] += 1
            left -= best[2]
        w = ref.Bits()
        w.put(0xfffd, 16)
        w.put(br, 4); w.put(sr, 2); w.put(size - 144000 * ref.KBPS[br - 1] // ref.RATES[sr], 1); w.put(0, 1)
        w.put(3 if ch_n == 1 else 0, 2); w.put(0, 6)
        for p in pairs:
            w.put(code[p], ref.nbal(high, p[0]))
        for p in pairs:
            if code[p]:
                w.put(sel[p], 2)
        for p in pairs:
            if code[p]:
                a, b, c3 = index[p]
                for v in {0: (a, b, c3), 1: (a, c3), 2: (a,), 3: (a, b)}[sel[p]]:
                    w.put(v, 6)
        q = {}
        for p in pairs:
            if code[p]:
                st = ref.steps_of(high, p[0], code[p])
                codes = []
                for part in range(3):
                    lv = ref.levels(st, index[p][part]).astype(np.float64)
                    codes += [int(v) for v in np.abs(lv[None, :] - S[p[1], 12 * part:12 * part + 12, p[0]][:, None]).argmin(axis=1)]
                q[p] = (st, codes)
        for g in range(12):
            for p in pairs:
                if p in q:
                    st, c = q[p]
                    if ref.grouped(st):
                        w.put(c[3 * g] + st * (c[3 * g + 1] + st * c[3 * g + 2]), ref.code_bits(st))
                    else:
                        for v in c[3 * g:3 * g + 3]:
                            w.put(v, ref.code_bits(st))
        out.append(w.bytes(size))
    return b"".join(out)


def figures(oracle_path):
    from jsmpeg_amd import cabi
    out = {}
    for name, cfg in inputs.CONFIGS.items():
        for kind in inputs.KINDS:
            x = inputs.pcm(kind, inputs.RATES[cfg[0]], 3)
            data = float_encode(cfg, x)
            pcm = cabi.decode_mp2_stream(oracle_path, np.frombuffer(data, np.uint8))[0]
            v = snr_db(x, pcm, cfg[1])
            out["%s/%s" % (name, kind)] = None if v is None else round(v, 2)
    return out


if __name__ == "__main__":
    from jsmpeg_amd import build
    doc = {"filterbank": mp2_enc_bounds.bounds(), "lag_samples": LAG, "decoder_gain": 1.0 / GAIN,
           "float64_snr_db": figures(build.build_oracle())}
    with open(OUT, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print(OUT)
