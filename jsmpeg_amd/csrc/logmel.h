/*
 * LOG-MEL FEATURES of C ABI part 12 (include/jsmpeg_hip.h), stated once for the kernel (logmel.hip), the host runtime and the
 * test-only simulator (tests/sim/sim_logmel.cpp); tests/logmel_ref.py restates the tables and the values in numpy float64.
 *
 * INPUT: per stream a device address of float32 mono samples and a count.  h = n_fft / 2, bins = h + 1.
 *
 * FRAMING is torch.stft(center=True, pad_mode="reflect"): frame t covers samples [t hop - h, t hop + h) of the stream; an index
 * -i before the stream's first sample reads x[i]; with END an index n - 1 + i behind its last sample reads x[n - 1 - i].
 * COUNTS ARE CLOSED FORM.  A stream that has taken n samples in all has
 *     open:  n <= h ? 0 : (n - h) / hop + 1        (every sample of a frame exists, and so does x[h] for frame 0's reflection)
 *     END:   n <= h ? 0 : n / hop + 1              (torch refuses n <= h; here such a stream has no frame)
 * frames (integer division), so the host knows every count at enqueue time and a call is a pure enqueue.
 *
 * THE DFT IS A GEMM.  Window w (n_fft doubles: the periodic Hann 0.5 - 0.5 cos(2 pi k / n_fft), or the user's floats) is folded
 * into the basis: B[k][2 b] = w[k] cos(2 pi k b / n_fft), B[k][2 b + 1] = -w[k] sin(2 pi k b / n_fft), the angle taken from
 * (k b) mod n_fft, a multiple of a quarter turn exact, in double, rounded ONCE to float32.  The table is [n_fft][cols_pad],
 * cols_pad = 2 bins rounded up to LM_TILE columns, zeros behind column 2 bins.  re / im of frame t are each
 *     acc = fmaf(x[t hop - h + k], B[k][c], acc),  k ascending from acc = 0
 * -- on the device v_mfma_f32_32x32x2_f32 (frames on the rows, columns of B on the columns, two k per instruction, the lower k
 * first), in the simulator fmaf.  No symmetric-window fold: a user window need not be symmetric.
 * POWER: p[b] = fmaf(re, re, im * im).
 * MEL: mel[m] = sum over b in [lo_m, hi_m), b ascending, acc = fmaf(fb[m][b], p[b], acc) from acc = 0; fb and the ranges (the
 * nonzero span of the rounded row) are built on the host in double as torchaudio's melscale_fbanks / librosa's mel do: bin
 * frequencies b (sample_rate / 2) / (bins - 1), n_mels + 2 points evenly spaced on the mel scale from f_min to f_max, triangles
 * max(0, min(up, down)); mel_norm slaney multiplies row m by 2 / (f[m + 2] - f[m]).  HTK: 2595 log10(1 + f / 700).  SLANEY:
 * 3 f / 200 below 1000 Hz, 15 + 27 ln(f / 1000) / ln 6.4 above.
 * LOGARITHM: lm_log2 below -- the exponent from the bits, the mantissa brought to [sqrt(1/2), sqrt 2), a degree-10 polynomial in
 * fmaf -- then ONE multiply: ln 2 (log), log10 2 (log10, whisper), 10 log10 2 (db), each of max(mel, floor).  WHISPER:
 * (max(v, M - 8) + 4) * 0.25 with v the log10 value and M the stream's maximum v over the call's frames (log10 of floor for a
 * stream without frames).
 * OUTPUT: [stream of the call][n_mels][row] (mel_major) or [stream of the call][row][n_mels] (time_major) in f32, f16 or bf16
 * (rs_f16_bits / rs_bf16_bits of pcm_resample.h).  Columns at and behind a stream's count hold the PAD VALUE, what a frame of
 * zeros gets: 0 (power), the scale of floor (logs), the stream's lower clamp (M - 8 + 4) * 0.25 (whisper).
 *
 * CHAINS (flag CHAIN, as part 11's).  Per stream NUMBER the host keeps {has state, samples taken N, parity}; the frames made
 * so far are the open count of N.  The device keeps two carries per stream number.  THE RULE: after N samples the carry holds
 * x[keep0(N) .. N), keep0(N) = max(0, min(F hop - h, N - 1 - h)) with F the open count of N: everything the next frame (F) and
 * END's reflection (back to x[N - 1 - h]) can still read.  Frame F is the first whose last sample is missing, F hop + h > N, so
 * it starts behind N - n_fft: the carry holds at most n_fft - 1 samples (carry_cap = n_fft floats per carry).  keep0 == 0 means
 * the stream's first sample is still there, and only then can a frame reach before it (START).  A call reads carry[parity], block 0 of a stream with new samples writes carry[parity ^ 1], the record flips.  A stream without
 * samples in a call keeps its state.  END ends the chains of the call's streams; an END call with 0 new samples lets the tail
 * frames come out of the carry.  A call without CHAIN starts from nothing and stores nothing.  WHISPER with CHAIN is refused.
 *
 * THE KERNEL's view: workgroup = LM_F consecutive columns (frames) of one stream, LM_WG threads.  It stages the LM_F frames'
 * span of raw samples, (LM_F - 1) hop + n_fft floats, ONCE in LDS; sample i of the span lies at word i + (i >> sh).  Frames
 * hop apart are the MFMA's 32 rows, read by 32 lanes in one LDS cycle only if they fall into 32 different banks, that is if the
 * frame stride is odd: sh = ctz(hop) makes it hop + (hop >> sh), odd, when ctz(hop) >= 2 (hop = 160: 165 words instead of 2
 * banks for the wavefront); an odd hop needs nothing and hop = 2 mod 4 is left at its two-way conflict (sh = 31: no skew), since a
 * word in two would not fit the largest span.  Behind the span: p[LM_F][bins | 1].  LDS = lm_lds_floats(R) * 4 bytes, dynamic.
 */
#ifndef JSMPEG_AMD_LOGMEL_H
#define JSMPEG_AMD_LOGMEL_H

#include "pcm_resample.h"          /* RS_HD, rs_float_bits, rs_f16_bits, rs_bf16_bits; fp contract off */

#define LM_F 32                    /* frames (columns of the output) per workgroup: the rows of one 32x32 MFMA tile */
#define LM_TILE 32                 /* columns of B per MFMA tile */
#define LM_WG 256                  /* threads: 4 waves, each owns the tiles w, w + 4, .. */
#define LM_WAVES 4
#define LM_NT 4                    /* tiles a wave accumulates at once: 4 independent accumulators, one read of x */
#define LM_LDS_MAX (160 * 1024)

#define LM_POWER 0
#define LM_LOG 1
#define LM_LOG10 2
#define LM_DB 3
#define LM_WHISPER 4
#define LM_MEL_MAJOR 0
#define LM_TIME_MAJOR 1
#define LM_HTK 0
#define LM_SLANEY 1
#define LM_END 1u                  /* (= JSMPEG_HIP_LOGMEL_END) */
#define LM_CHAIN 2u                /* (= JSMPEG_HIP_LOGMEL_CHAIN) */

struct LmRule {
	int32_t sample_rate, n_fft, hop, n_mels;
	int32_t half, bins, cols_pad, tiles;
	int32_t scale, layout, dtype;
	int32_t sh, fstride;           /* the LDS map: sample i of the span at i + (i >> sh); words from frame to frame */
	int32_t span, span_lds;        /* (LM_F - 1) hop + n_fft samples; their words */
	int32_t pstride;               /* bins | 1 */
	int32_t carry_cap;             /* n_fft: a carry holds at most n_fft - 1 samples */
	uint32_t row;
	float floor_, pad, pad_log10;  /* pad: the pad value (whisper: unused); pad_log10: log10 of floor under the rule */
};

/* ------------------------------------------------------------------ the logarithm */
RS_HD float lm_bits_float(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }
/* log2 of a positive normal float */
RS_HD float lm_log2(float v) {
	const uint32_t bits = rs_float_bits(v), mant = bits & 0x7fffffu;
	int e = (int)(bits >> 23) - 127;
	uint32_t mb = mant | 0x3f800000u;
	if (mant > 0x3504f3u) { mb = mant | 0x3f000000u; e += 1; }                /* m in (sqrt(1/2), sqrt 2] */
	const float f = lm_bits_float(mb) - 1.0f;                                 /* exact */
	float p = 0x1.8e4c96p-4f;                                                 /* log2(1 + f) / f, fitted at Chebyshev nodes in double: 3.3e-10 */
	p = fmaf(p, f, -0x1.5a7f52p-3f);
	p = fmaf(p, f, 0x1.604f1cp-3f);
	p = fmaf(p, f, -0x1.6e5a2ep-3f);
	p = fmaf(p, f, 0x1.a3ee6ap-3f);
	p = fmaf(p, f, -0x1.ec7b06p-3f);
	p = fmaf(p, f, 0x1.278084p-2f);
	p = fmaf(p, f, -0x1.71548ep-2f);
	p = fmaf(p, f, 0x1.ec708p-2f);
	p = fmaf(p, f, -0x1.715476p-1f);
	p = fmaf(p, f, 0x1.715476p+0f);
	return fmaf(f, p, (float)e);
}
#define LM_LN2 0x1.62e43p-1f           /* ln 2 */
#define LM_LOG10_2 0x1.344136p-2f      /* log10 2 */
#define LM_DB_2 0x1.815182p+1f         /* 10 log10 2 */
RS_HD float lm_log_of(int scale, float floor_, float mel) {
	const float v = mel > floor_ ? mel : floor_;
	const float l2 = lm_log2(v);
	return l2 * (scale == LM_LOG ? LM_LN2 : scale == LM_DB ? LM_DB_2 : LM_LOG10_2);
}
RS_HD float lm_scale(const LmRule &R, float mel) { return R.scale == LM_POWER ? mel : lm_log_of(R.scale, R.floor_, mel); }

/* whisper's maximum: an order-preserving key of a float, so that an integer max over keys is the float max in any order */
RS_HD uint32_t lm_key(float v) { const uint32_t b = rs_float_bits(v); return (b & 0x80000000u) ? ~b : (b | 0x80000000u); }
RS_HD float lm_unkey(uint32_t k) { return lm_bits_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }
RS_HD float lm_whisper(float v, float M, bool valid) {
	const float low = M - 8.0f;
	const float c = (valid && v > low) ? v : low;
	return (c + 4.0f) * 0.25f;
}

/* ------------------------------------------------------------------ the rule */
RS_HD int lm_rule_make(int sample_rate, int n_fft, int hop, int n_mels, int scale, int layout, int dtype, float floor_, uint32_t row, LmRule *R) {
	if (sample_rate < 8000 || sample_rate > 48000) return -1;
	if (n_fft < 32 || n_fft > 1024 || (n_fft & 1)) return -2;
	if (hop < 1 || hop > n_fft / 2) return -3;
	if (n_mels < 1 || n_mels > 256) return -4;
	if (scale < 0 || scale > LM_WHISPER || layout < 0 || layout > 1 || dtype < 0 || dtype > 2) return -5;
	if (floor_ == 0.0f) floor_ = 1e-10f;
	if (!(floor_ >= 1.17549435e-38f) || !(floor_ <= 3.0e38f)) return -6;
	R->sample_rate = sample_rate; R->n_fft = n_fft; R->hop = hop; R->n_mels = n_mels;
	R->half = n_fft / 2; R->bins = n_fft / 2 + 1;
	R->cols_pad = (2 * R->bins + LM_TILE - 1) / LM_TILE * LM_TILE; R->tiles = R->cols_pad / LM_TILE;
	R->scale = scale; R->layout = layout; R->dtype = dtype;
	int z = 0;
	while (!((hop >> z) & 1)) z++;
	R->sh = z >= 2 ? z : 31;
	R->fstride = hop + (hop >> R->sh);
	R->span = (LM_F - 1) * hop + n_fft;
	R->span_lds = R->span + (R->span >> R->sh);
	R->pstride = R->bins | 1;
	R->carry_cap = n_fft;
	R->row = row;
	R->floor_ = floor_;
	R->pad_log10 = lm_log_of(LM_LOG10, floor_, 0.0f);
	R->pad = scale == LM_POWER ? 0.0f : lm_log_of(scale, floor_, 0.0f);
	return 0;
}
RS_HD uint32_t lm_lds_floats(const LmRule &R) { return (uint32_t)(R.span_lds + LM_F * R.pstride); }

RS_HD uint64_t lm_frames(const LmRule &R, uint64_t n, bool end) {
	if (n <= (uint64_t)R.half) return 0;
	return (end ? n : n - (uint64_t)R.half) / (uint64_t)R.hop + 1;
}
/* the first sample the carry holds after n samples */
RS_HD uint64_t lm_keep0(const LmRule &R, uint64_t n) {
	const int64_t a = (int64_t)(lm_frames(R, n, false) * (uint64_t)R.hop) - R.half, b = (int64_t)n - 1 - R.half;
	const int64_t m = a < b ? a : b;
	return m > 0 ? (uint64_t)m : 0;
}

/* ------------------------------------------------------------------ the tables (host, double) */
static inline void lm_window_make(int n_fft, const float *user, double *w) {
	const double pi = 3.14159265358979323846;
	for (int k = 0; k < n_fft; k++) w[k] = user ? (double)user[k] : 0.5 - 0.5 * cos(2.0 * pi * (double)k / (double)n_fft);
}
/* out: [n_fft][cols_pad] */
static inline void lm_basis_make(int n_fft, const double *w, int cols_pad, float *out) {
	const double pi = 3.14159265358979323846;
	const int bins = n_fft / 2 + 1;
	for (int k = 0; k < n_fft; k++) {
		float *row = out + (size_t)k * cols_pad;
		for (int c = 0; c < cols_pad; c++) row[c] = 0.0f;
		for (int b = 0; b < bins; b++) {
			const int j = (int)(((int64_t)k * b) % n_fft);
			double c, s;
			if ((4 * j) % n_fft == 0) { const int q = 4 * j / n_fft; c = q == 0 ? 1.0 : q == 2 ? -1.0 : 0.0; s = q == 1 ? 1.0 : q == 3 ? -1.0 : 0.0; }
			else { const double a = 2.0 * pi * (double)j / (double)n_fft; c = cos(a); s = sin(a); }
			row[2 * b] = (float)(w[k] * c);
			row[2 * b + 1] = (float)(-(w[k] * s));
		}
	}
}
static inline double lm_hz_to_mel(double f, int mel_scale) {
	if (mel_scale == LM_HTK) return 2595.0 * log10(1.0 + f / 700.0);
	if (f < 1000.0) return 3.0 * f / 200.0;
	return 15.0 + 27.0 * log(f / 1000.0) / log(6.4);
}
static inline double lm_mel_to_hz(double m, int mel_scale) {
	if (mel_scale == LM_HTK) return 700.0 * (pow(10.0, m / 2595.0) - 1.0);
	if (m < 15.0) return 200.0 * m / 3.0;
	return 1000.0 * exp(log(6.4) * (m - 15.0) / 27.0);
}
/* fb: [n_mels][bins]; range: [n_mels][2] = lo, hi of the rounded row's nonzero span (0, 0: an empty band); pts: n_mels + 2
 * doubles of room.  f_max == 0: sample_rate / 2.  Returns < 0 for f_min / f_max outside 0 <= f_min < f_max <= sample_rate / 2 */
static inline int lm_filters_make(int sample_rate, int n_fft, int n_mels, double f_min, double f_max, int mel_scale, int mel_norm, float *fb, int32_t *range, double *pts) {
	const int bins = n_fft / 2 + 1;
	const double nyq = 0.5 * (double)sample_rate;
	if (f_max == 0.0) f_max = nyq;
	if (!(f_min >= 0.0) || !(f_min < f_max) || !(f_max <= nyq) || mel_scale < 0 || mel_scale > 1 || mel_norm < 0 || mel_norm > 1) return -1;
	const double m0 = lm_hz_to_mel(f_min, mel_scale), m1 = lm_hz_to_mel(f_max, mel_scale), step = (m1 - m0) / (double)(n_mels + 1);
	for (int i = 0; i < n_mels + 2; i++) pts[i] = lm_mel_to_hz(i == n_mels + 1 ? m1 : m0 + (double)i * step, mel_scale);
	for (int m = 0; m < n_mels; m++) {
		const double d0 = pts[m + 1] - pts[m], d1 = pts[m + 2] - pts[m + 1], norm = mel_norm ? 2.0 / (pts[m + 2] - pts[m]) : 1.0;
		int lo = 0, hi = 0;
		for (int b = 0; b < bins; b++) {
			const double f = nyq * (double)b / (double)(bins - 1);
			const double up = (f - pts[m]) / d0, down = (pts[m + 2] - f) / d1;
			double v = up < down ? up : down;
			v = v > 0.0 ? v * norm : 0.0;
			const float r = (float)v;
			fb[(size_t)m * bins + b] = r;
			if (r != 0.0f) { if (hi == 0) lo = b; hi = b + 1; }
		}
		range[2 * m] = lo; range[2 * m + 1] = hi;
	}
	return 0;
}

/* ------------------------------------------------------------------ a stream of a call, planned by the host */
#define LM_S_START 1u              /* the stream's first sample is relative index -n0: indices before it reflect */
#define LM_S_END 2u                /* indices at or behind n_in reflect about n_in - 1 */
#define LM_S_CARRY_OUT 4u          /* block 0 writes carry[parity ^ 1]: the relative indices [n_in - keep, n_in) */
#define LM_S_PARITY 8u
struct LmStream {
	const float *pcm;
	uint32_t n_in;                 /* samples of the call */
	uint32_t frames;               /* frames of the call */
	int32_t first;                 /* the first of them starts at this index, relative to the call's first sample */
	uint32_t carry_len;            /* carry[parity] holds the relative indices [-carry_len, 0) */
	uint32_t keep;
	uint32_t stream;               /* stream number: which carry */
	uint32_t flags;
	uint32_t n0;                   /* START: samples in front of the call (= carry_len) */
	uint32_t index;                /* the stream's place in the call: its rows of the output */
	uint32_t maxkey;               /* WHISPER: lm_key of the largest log10 value so far; the host puts log10 of floor here */
};
struct LmChain { uint32_t have, parity; uint64_t n; };

RS_HD size_t lm_carry_at(const LmRule &R, uint32_t stream, uint32_t parity) { return (size_t)(stream * 2u + parity) * (size_t)R.carry_cap; }

/* Plans a call on the host: list[n_streams], count[i] = frames of stream i.  Reads the records, changes nothing.  Returns 0, or
 * -1 - i when stream i has more frames than row. */
static inline int lm_plan_call(const LmRule &R, const float *const *pcm, const uint32_t *samples, const uint32_t *numbers, uint32_t n_streams, uint32_t flags,
                               const LmChain *rec, LmStream *list, uint64_t *count) {
	const bool chain = (flags & LM_CHAIN) != 0, end = (flags & LM_END) != 0;
	for (uint32_t i = 0; i < n_streams; i++) {
		const uint32_t s = numbers ? numbers[i] : i;
		const bool have = chain && rec[s].have;
		const uint64_t N0 = have ? rec[s].n : 0, N1 = N0 + samples[i];
		const uint64_t F0 = lm_frames(R, N0, false), F1 = (samples[i] || end) ? lm_frames(R, N1, end) : F0;
		const uint64_t k0 = lm_keep0(R, N0);
		LmStream &S = list[i];
		S.pcm = samples[i] ? pcm[i] : nullptr;
		S.n_in = samples[i];
		S.frames = (uint32_t)(F1 - F0);
		S.first = (int32_t)((int64_t)(F0 * (uint64_t)R.hop) - R.half - (int64_t)N0);
		S.carry_len = (uint32_t)(N0 - k0);
		S.stream = s;
		S.flags = (k0 == 0 ? LM_S_START : 0u) | (end ? LM_S_END : 0u) | ((have && rec[s].parity) ? LM_S_PARITY : 0u);
		S.n0 = k0 == 0 ? (uint32_t)N0 : 0u;
		S.keep = 0;
		if (chain && !end && samples[i]) { S.flags |= LM_S_CARRY_OUT; S.keep = (uint32_t)(N1 - lm_keep0(R, N1)); }
		S.index = i;
		S.maxkey = lm_key(R.pad_log10);
		count[i] = S.frames;
		if (F1 - F0 > R.row) return -1 - (int)i;
	}
	return 0;
}
static inline void lm_plan_commit(const uint32_t *samples, const uint32_t *numbers, uint32_t n_streams, uint32_t flags, LmChain *rec) {
	if (!(flags & LM_CHAIN)) return;
	for (uint32_t i = 0; i < n_streams; i++) {
		LmChain &c = rec[numbers ? numbers[i] : i];
		if (flags & LM_END) { c = LmChain{ 0, 0, 0 }; continue; }
		if (!samples[i]) continue;
		c = LmChain{ 1u, c.have ? c.parity ^ 1u : 1u, (c.have ? c.n : 0) + samples[i] };
	}
}
/* a stream without state reads no carry and writes carry[1]: lm_plan_commit's first record has parity 1 */

/* ------------------------------------------------------------------ the per-lane bodies of k_logmel */
/* x of the call's stream at index i relative to the call's first sample; any i is answered, 0 where the stream has nothing */
RS_HD float lm_x(const LmRule &R, const LmStream &S, const float *carry, int64_t i) {
	if ((S.flags & LM_S_START) && i < -(int64_t)S.n0) i = -2 * (int64_t)S.n0 - i;
	if ((S.flags & LM_S_END) && i >= (int64_t)S.n_in) i = 2 * ((int64_t)S.n_in - 1) - i;
	if (i < 0) {
		if (i < -(int64_t)S.carry_len) return 0.0f;
		return carry[lm_carry_at(R, S.stream, (S.flags & LM_S_PARITY) ? 1u : 0u) + (size_t)((int64_t)S.carry_len + i)];
	}
	if (i >= (int64_t)S.n_in) return 0.0f;
	return S.pcm[i];
}
RS_HD int lm_pos(const LmRule &R, int i) { return i + (i >> R.sh); }

/* phase 1: the block's span into LDS (only a block that has frames); block 0 of a chained stream writes the next call's carry */
RS_HD void lm_wg_stage(const LmRule &R, const LmStream &S, uint32_t block, int tid, float *carry, float *xl) {
	if (block * LM_F < S.frames) {
		const int64_t base = (int64_t)S.first + (int64_t)block * LM_F * R.hop;
		for (int i = tid; i < R.span; i += LM_WG) xl[lm_pos(R, i)] = lm_x(R, S, carry, base + i);
	}
	if (block == 0 && (S.flags & LM_S_CARRY_OUT)) {
		float *out = carry + lm_carry_at(R, S.stream, (S.flags & LM_S_PARITY) ? 0u : 1u);
		for (int i = tid; i < (int)S.keep; i += LM_WG) out[i] = lm_x(R, S, carry, (int64_t)S.n_in - (int64_t)S.keep + i);
	}
}

/* phase 2 as the rule states it (the simulator's; the kernel does the same chains on the matrix unit): re, im of column pair b
 * of frame f of the block, and the power */
RS_HD void lm_dft_bin(const LmRule &R, const float *xl, const float *basis, int f, int b, float *re, float *im) {
	float a = 0.0f, c = 0.0f;
	for (int k = 0; k < R.n_fft; k++) {
		const float x = xl[lm_pos(R, f * R.hop + k)];
		a = fmaf(x, basis[(size_t)k * R.cols_pad + 2 * b], a);
		c = fmaf(x, basis[(size_t)k * R.cols_pad + 2 * b + 1], c);
	}
	*re = a; *im = c;
}
RS_HD float lm_power(float re, float im) { const float q = im * im; return fmaf(re, re, q); }

/* phase 3: the mel sums, the scale and the store of the block's LM_F columns; p: [LM_F][pstride].  WHISPER: the log10 values go
 * to tmp (float32, the output's layout); returns lm_key of the largest of them this lane has seen (0: none). */
RS_HD uint32_t lm_wg_mel(const LmRule &R, const LmStream &S, uint32_t block, int tid, const float *fb, const int32_t *range, const float *p, void *out, float *tmp) {
	uint32_t key = 0;
	const bool active = block * LM_F < S.frames;
	for (int idx = tid; idx < LM_F * R.n_mels; idx += LM_WG) {
		int f, m;
		if (R.layout == LM_MEL_MAJOR) { f = idx % LM_F; m = idx / LM_F; }
		else { m = idx % R.n_mels; f = idx / R.n_mels; }
		const uint32_t col = block * LM_F + (uint32_t)f;
		if (col >= R.row) continue;
		const size_t at = R.layout == LM_MEL_MAJOR ? ((size_t)S.index * (size_t)R.n_mels + (size_t)m) * R.row + col
		                                           : ((size_t)S.index * R.row + col) * (size_t)R.n_mels + (size_t)m;
		float v = R.pad;
		if (active && col < S.frames) {
			const float *w = fb + (size_t)m * R.bins, *q = p + (size_t)f * R.pstride;
			float acc = 0.0f;
			for (int b = range[2 * m]; b < range[2 * m + 1]; b++) acc = fmaf(w[b], q[b], acc);
			v = lm_scale(R, acc);
			if (R.scale == LM_WHISPER) { const uint32_t k = lm_key(v); key = k > key ? k : key; }
		}
		if (R.scale == LM_WHISPER) tmp[at] = v;
		else if (R.dtype == RS_F32) static_cast<float *>(out)[at] = v;
		else static_cast<uint16_t *>(out)[at] = R.dtype == RS_F16 ? rs_f16_bits(v) : rs_bf16_bits(v);
	}
	return key;
}

/* WHISPER's second pass: element e of the call's n_streams * n_mels * row */
RS_HD void lm_clamp_elem(const LmRule &R, const LmStream *list, size_t e, const float *tmp, void *out) {
	const size_t per = (size_t)R.n_mels * R.row;
	const LmStream &S = list[e / per];
	const uint32_t col = (uint32_t)(R.layout == LM_MEL_MAJOR ? e % R.row : (e % per) / (size_t)R.n_mels);
	const float v = lm_whisper(tmp[e], lm_unkey(S.maxkey), col < S.frames);
	if (R.dtype == RS_F32) static_cast<float *>(out)[e] = v;
	else static_cast<uint16_t *>(out)[e] = R.dtype == RS_F16 ? rs_f16_bits(v) : rs_bf16_bits(v);
}

#endif
