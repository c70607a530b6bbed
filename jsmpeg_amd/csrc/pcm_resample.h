/*
 * The PCM RESAMPLER of C ABI part 11 (include/jsmpeg_hip.h), stated once for the kernel (pcm_resample.hip), the host runtime
 * and the test-only simulator (tests/sim/sim_resample.cpp); tests/resample_ref.py restates it in numpy float64.
 *
 * RATES: input 32000, 44100 or 48000 Hz; output 8000, 16000, 22050, 24000, 32000, 44100 or 48000 Hz; output equal to input is
 * refused: 18 pairs.
 *
 * PLAN: g = gcd(in, out), L = out / g, M = in / g, s = min(1, L / M).  Half width H = 16 for s = 1, otherwise ceil(16 / s) =
 * ceil(16 M / L) input samples; cut-off c = 0.90 s.
 *
 * PROTOTYPE: w(t) = c sinc(c t) I0(9 sqrt(1 - (t / H)^2)) / I0(9) for |t| < H, 0 otherwise (sinc normalised: sin(pi x) / (pi x)).
 * TAPS: h[p][j] = w(H - 1 - j + p / L), p in 0 .. L - 1, j in 0 .. 2 H - 1, computed on the host in double and rounded ONCE to
 * float32; no per-phase normalisation.  The largest table is 32000 -> 22050: 441 x 48 floats.
 *
 * A SAMPLE: output ordinal m of a stream has n = floor(m M / L) and p = (m M) mod L;
 *     y[m] = gain * sum_j h[p][j] x[n - 2 H + 1 + j]
 * accumulated in float32 as acc = fmaf(h, x, acc), j ascending from acc = 0, then ONE multiply by gain.  x reads 0 before a
 * stream's first sample.  The result is the input delayed by H input samples.  That fixed order is what makes the GPU, the
 * simulator and pieces-versus-whole bit-exact: it is never reassociated.
 * MONO MIX (a handle with one output channel), before the filter: x = 0.5f * (left + right), one rounding.
 *
 * COUNTS ARE CLOSED FORM: after N input samples a stream has ceil(N L / M) outputs (output m exists once sample n of it does),
 * so the host knows every count and offset at enqueue time.
 * PER-CALL ARITHMETIC IN 32 BITS: a call continues a stream at N inputs and m0 outputs; o = m0 M - N L, 0 <= o < M, and the
 * k-th output of the call has n - N = (o + k M) div L and p = (o + k M) mod L.  The host refuses a call whose (inputs + H) L + M
 * does not fit 32 bits (more than about 8000 frames of one stream), so o + k M never wraps.
 *
 * FLAGS (as part 9's): CHAIN continues the call's streams -- per stream NUMBER the host keeps {has state, N, outputs so far,
 * parity}, the device two carries of the stream's last 2 H - 1 input samples per filter channel (after the mono mix); a call reads
 * carry[parity], its block 0 writes carry[parity ^ 1] from the input (a frame is longer than the carry), and the record flips.
 * A stream without frames in a call keeps its state.  A call without CHAIN starts from nothing and stores nothing.  END
 * continues every listed stream that has any input (in this call or in its chain) by H zero samples, so the filter's tail
 * comes out; with CHAIN it also ends the chain.
 *
 * FORMS.  WAVEFORM: [stream of the call][channels_out][row] in f32, f16 or bf16 (the f32 value rounded to nearest even:
 * rs_f16_bits / rs_bf16_bits, integers only); samples behind a stream's count are zero.  FRAMES: float32 [frame][2][1152] at
 * the output rate (a mono handle writes its mix to both channels); a call hands out the whole frames its outputs complete,
 * floor(m1 / 1152) - floor(m0 / 1152); the partial frame stays on the device in part[parity ^ 1] -- the samples in front of
 * it (lead = m0 mod 1152, from part[parity]) are carried along by the same kernel -- and the next chained call completes it;
 * with END the last partial frame is filled with zeros; a call with neither CHAIN nor END drops its partial tail.
 *
 * THE KERNEL's view: a "slot" q of a (stream, filter channel) is a place the call writes: q < lead is a sample of the partial
 * frame in front, lead <= q < lead + count output k = q - lead, anything behind a zero.  A workgroup is RS_WG consecutive
 * slots; it stages the input span its outputs read in LDS (at most (RS_WG - 1) M / L + 2 H + 1 <= RS_SPAN samples).
 */
#ifndef JSMPEG_AMD_PCM_RESAMPLE_H
#define JSMPEG_AMD_PCM_RESAMPLE_H

#include <math.h>
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define RS_HD __host__ __device__ __forceinline__
#else
#define RS_HD static inline
#endif

#pragma clang fp contract(off)     /* every product rounds as written: the only fused steps are the fmaf calls of the filter's sum */

#define RS_WG 256                  /* slots per workgroup, one per thread */
#define RS_SPAN 1792               /* floats of LDS: 48000 -> 8000 needs 255 * 6 + 192 + 1 = 1723 */
#define RS_FRAME 1152              /* samples per channel of a frame, in and (FRAMES form) out */
#define RS_MAX_TAPS (441 * 48)     /* 32000 -> 22050 */
#define RS_MAX_CARRY 191           /* 2 H - 1 at H = 96 (48000 -> 8000) */

#define RS_FORM_WAVEFORM 0
#define RS_FORM_FRAMES 1
#define RS_F32 0
#define RS_F16 1
#define RS_BF16 2
#define RS_END 1u                  /* (= JSMPEG_HIP_RESAMPLE_END) */
#define RS_CHAIN 2u                /* (= JSMPEG_HIP_RESAMPLE_CHAIN) */

/* the handle's settings and what follows from them */
struct RsRule {
	int32_t in_rate, out_rate;
	int32_t L, M, H;
	int32_t taps, carry;           /* 2 H, 2 H - 1 */
	int32_t channels;              /* filter channels = channels_out */
	int32_t form, dtype;
	uint32_t row;                  /* WAVEFORM: samples per (stream, channel) of the output */
	float gain;
};

RS_HD int rs_plan(int in_rate, int out_rate, int *L, int *M, int *H) {
	if (in_rate != 32000 && in_rate != 44100 && in_rate != 48000) return -1;
	if (out_rate != 8000 && out_rate != 16000 && out_rate != 22050 && out_rate != 24000 && out_rate != 32000 && out_rate != 44100 && out_rate != 48000) return -1;
	if (in_rate == out_rate) return -1;
	int a = in_rate, b = out_rate;
	while (b) { const int t = a % b; a = b; b = t; }
	const int l = out_rate / a, m = in_rate / a;
	*L = l; *M = m;
	*H = l >= m ? 16 : (16 * m + l - 1) / l;
	return 0;
}

RS_HD int rs_rule_make(int in_rate, int out_rate, int channels, int form, int dtype, float gain, uint32_t row, RsRule *R) {
	int L, M, H;
	if (rs_plan(in_rate, out_rate, &L, &M, &H) != 0) return -1;
	if (channels < 1 || channels > 2 || form < 0 || form > 1 || dtype < 0 || dtype > 2) return -2;
	if (form == RS_FORM_FRAMES && dtype != RS_F32) return -2;
	R->in_rate = in_rate; R->out_rate = out_rate; R->L = L; R->M = M; R->H = H; R->taps = 2 * H; R->carry = 2 * H - 1;
	R->channels = channels; R->form = form; R->dtype = dtype; R->row = row;
	R->gain = gain == 0.0f ? 1.0f : gain;
	return 0;
}

/* outputs of a stream after N input samples: ceil(N L / M) */
RS_HD uint64_t rs_outputs(const RsRule &R, uint64_t N) { return (N * (uint64_t)R.L + (uint64_t)R.M - 1) / (uint64_t)R.M; }

/* ------------------------------------------------------------------ the taps (host, double) */
static inline double rs_i0(double x) {                 /* the series sum ((x / 2)^2)^k / (k!)^2: all terms positive, x <= 9 here */
	const double q = 0.25 * x * x;
	double term = 1.0, sum = 1.0;
	for (int k = 1; k < 200; k++) {
		term *= q / ((double)k * (double)k);
		sum += term;
		if (term < sum * 1e-18) break;
	}
	return sum;
}
static inline double rs_prototype(double t, int H, double c) {
	if (!(fabs(t) < (double)H)) return 0.0;
	const double pi = 3.14159265358979323846;
	const double x = c * t, y = pi * (x == 0.0 ? 1.0e-20 : x);
	const double u = t / (double)H;
	return c * (sin(y) / y) * rs_i0(9.0 * sqrt(1.0 - u * u)) / rs_i0(9.0);
}
/* out: L * 2 H floats, [p][j] */
static inline int rs_taps_make(int in_rate, int out_rate, float *out) {
	int L, M, H;
	if (rs_plan(in_rate, out_rate, &L, &M, &H) != 0) return -1;
	const double s = L >= M ? 1.0 : (double)L / (double)M, c = 0.90 * s;
	for (int p = 0; p < L; p++)
		for (int j = 0; j < 2 * H; j++) out[p * 2 * H + j] = (float)rs_prototype((double)(H - 1 - j) + (double)p / (double)L, H, c);
	return 0;
}

/* ------------------------------------------------------------------ the narrow types: the f32 value rounded to nearest even */
RS_HD uint32_t rs_float_bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
RS_HD uint16_t rs_f16_bits(float f) {
	uint32_t x = rs_float_bits(f);
	const uint32_t sign = (x >> 16) & 0x8000u;
	x &= 0x7fffffffu;
	if (x > 0x7f800000u) return (uint16_t)(sign | 0x7e00u);
	if (x >= 0x47800000u) return (uint16_t)(sign | 0x7c00u);                 /* 65536 and above, infinity */
	if (x < 0x38800000u) {                                                   /* below 2^-14: a subnormal half, or zero */
		if (x < 0x33000000u) return (uint16_t)sign;                          /* below 2^-25 */
		const uint32_t shift = 126u - (x >> 23), m = (x & 0x7fffffu) | 0x800000u;
		uint32_t r = m >> shift;
		const uint32_t rem = m & ((1u << shift) - 1u), half = 1u << (shift - 1u);
		if (rem > half || (rem == half && (r & 1u))) r++;
		return (uint16_t)(sign | r);
	}
	uint32_t r = (x - 0x38000000u) >> 13;
	const uint32_t rem = x & 0x1fffu;
	if (rem > 0x1000u || (rem == 0x1000u && (r & 1u))) r++;                  /* (65520 and above carries into infinity) */
	return (uint16_t)(sign | r);
}
RS_HD uint16_t rs_bf16_bits(float f) {
	const uint32_t x = rs_float_bits(f);
	if ((x & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((x >> 16) | 0x0040u);
	return (uint16_t)((x + 0x7fffu + ((x >> 16) & 1u)) >> 16);
}

/* ------------------------------------------------------------------ a stream of a call, planned by the host */
#define RS_S_CARRY_IN 1u           /* indices before the call's first sample read carry[parity]; otherwise zeros */
#define RS_S_CARRY_OUT 2u          /* block 0 writes carry[parity ^ 1] from the call's last 2 H - 1 input samples */
#define RS_S_PARITY 4u
#define RS_S_PART_OUT 8u           /* FRAMES: slots behind the whole frames go to part[parity ^ 1]; otherwise nowhere */
struct RsStream {
	const float *pcm;              /* [frames][2][1152] */
	uint32_t in;                   /* input samples in pcm: 1152 per frame; indices at or above it read 0 (END's tail) */
	uint32_t o;                    /* m0 M - N L */
	uint32_t count;                /* outputs of the call */
	uint32_t stream;               /* stream number: which carry */
	uint32_t flags;
	uint32_t lead;                 /* FRAMES: samples of the partial frame in front (part[parity]); WAVEFORM: 0 */
	uint32_t slots;                /* what the call writes per channel: WAVEFORM row; FRAMES lead + count, padded or cut to frames */
	uint32_t whole;                /* FRAMES: whole frames handed out */
	uint32_t frame0;               /* FRAMES: the first of them in the output; WAVEFORM: the stream's index in the call */
	uint32_t pad_;
};

/* THE CHAIN: the host's record per stream number */
struct RsChain { uint32_t have, parity; uint64_t n_in, n_out; };

/* Plans a call on the host.  Fills list[n_streams], offset[i] / count[i] (WAVEFORM: the element index of the stream's first
 * row and its samples; FRAMES: its first frame and its whole frames) and *total (WAVEFORM: n_streams * channels * row
 * elements; FRAMES: frames).  Reads the records, changes nothing.  Returns 0, -1 - i when stream i has more outputs than row,
 * -1000001 - i when its inputs do not fit the 32-bit arithmetic. */
static inline int rs_plan_call(const RsRule &R, const float *const *pcm, const uint32_t *frames, const uint32_t *numbers, uint32_t n_streams, uint32_t flags,
                               const RsChain *rec, RsStream *list, uint64_t *offset, uint64_t *count, uint64_t *total) {
	const bool chain = (flags & RS_CHAIN) != 0, end = (flags & RS_END) != 0;
	uint64_t at = 0;
	for (uint32_t i = 0; i < n_streams; i++) {
		const uint32_t s = numbers ? numbers[i] : i;
		const bool have = chain && rec[s].have;
		const uint64_t N = have ? rec[s].n_in : 0, m0 = have ? rec[s].n_out : 0;
		const uint64_t in = (uint64_t)frames[i] * RS_FRAME;
		const uint64_t tail = (end && (in || N)) ? (uint64_t)R.H : 0;
		if ((in + tail) * (uint64_t)R.L + (uint64_t)R.M > 0xffffffffull) return -1000001 - (int)i;
		const uint64_t m1 = rs_outputs(R, N + in + tail);
		RsStream &S = list[i];
		S.pcm = frames[i] ? pcm[i] : nullptr;
		S.in = (uint32_t)in;
		S.o = (uint32_t)(m0 * (uint64_t)R.M - N * (uint64_t)R.L);
		S.count = (uint32_t)(m1 - m0);
		S.stream = s;
		S.flags = (have ? RS_S_CARRY_IN | (rec[s].parity ? RS_S_PARITY : 0u) : 0u) | ((chain && !end && in) ? RS_S_CARRY_OUT : 0u);
		S.pad_ = 0;
		if (R.form == RS_FORM_WAVEFORM) {
			if (S.count > R.row) return -1 - (int)i;
			S.lead = 0; S.slots = R.row; S.whole = 0; S.frame0 = i;
			offset[i] = (uint64_t)i * (uint64_t)R.channels * R.row; count[i] = S.count;
		} else {
			S.lead = (uint32_t)(m0 % RS_FRAME);
			const uint32_t filled = S.lead + S.count;
			const bool active = in || tail;
			if (!active) { S.slots = 0; S.whole = 0; }                      /* the stream keeps its state, its partial frame included */
			else if (end) { S.whole = (filled + RS_FRAME - 1) / RS_FRAME; S.slots = S.whole * RS_FRAME; }
			else if (chain) { S.whole = filled / RS_FRAME; S.slots = filled; S.flags |= RS_S_PART_OUT; }
			else { S.whole = filled / RS_FRAME; S.slots = S.whole * RS_FRAME; }
			S.frame0 = (uint32_t)at;
			offset[i] = at; count[i] = S.whole;
			at += S.whole;
		}
	}
	*total = R.form == RS_FORM_WAVEFORM ? (uint64_t)n_streams * (uint64_t)R.channels * R.row : at;
	return 0;
}
/* the records behind a planned call */
static inline void rs_plan_commit(const RsRule &R, const uint32_t *frames, const uint32_t *numbers, uint32_t n_streams, uint32_t flags, RsChain *rec) {
	if (!(flags & RS_CHAIN)) return;
	for (uint32_t i = 0; i < n_streams; i++) {
		RsChain &c = rec[numbers ? numbers[i] : i];
		if (flags & RS_END) { c = RsChain{ 0, 0, 0, 0 }; continue; }
		if (!frames[i]) continue;
		const uint64_t N = (c.have ? c.n_in : 0) + (uint64_t)frames[i] * RS_FRAME;
		c = RsChain{ 1u, c.have ? c.parity ^ 1u : 1u, N, rs_outputs(R, N) };
	}
}
/* a stream without state reads no carry and writes carry[1] / part[1] (parity 0 ^ 1): rs_plan_commit's first record has parity 1 */

/* the device's state per stream number: float carry[stream][parity][2][RS_MAX_CARRY] and part[stream][parity][2][1152] */
#define RS_CARRY_FLOATS (2 * 2 * RS_MAX_CARRY)
#define RS_PART_FLOATS (2 * 2 * RS_FRAME)
RS_HD size_t rs_carry_at(uint32_t stream, uint32_t parity, int ch) { return ((size_t)(stream * 2u + parity) * 2u + (uint32_t)ch) * RS_MAX_CARRY; }
RS_HD size_t rs_part_at(uint32_t stream, uint32_t parity, int ch) { return ((size_t)(stream * 2u + parity) * 2u + (uint32_t)ch) * RS_FRAME; }

/* ------------------------------------------------------------------ the per-lane bodies of k_resample */
struct RsLds { float x[RS_SPAN]; };

/* x of the call's stream at index i relative to the call's first sample, -(2 H - 1) <= i, of filter channel ch */
RS_HD float rs_x(const RsRule &R, const RsStream &S, const float *carry, int ch, int i) {
	if (i < 0) return (S.flags & RS_S_CARRY_IN) ? carry[rs_carry_at(S.stream, (S.flags & RS_S_PARITY) ? 1u : 0u, ch) + (size_t)(R.carry + i)] : 0.0f;
	if ((uint32_t)i >= S.in) return 0.0f;
	const float *f = S.pcm + (size_t)((uint32_t)i / RS_FRAME) * (2 * RS_FRAME) + (uint32_t)i % RS_FRAME;
	if (R.channels == 1) { const float sum = f[0] + f[RS_FRAME]; return 0.5f * sum; }
	return f[ch * RS_FRAME];
}

/* the outputs [k0, k1) of workgroup `block` and the first input index they read; false: the block has no slot */
RS_HD bool rs_block(const RsRule &R, const RsStream &S, uint32_t block, uint32_t *k0, uint32_t *k1, int *first, int *span) {
	const uint32_t q0 = block * RS_WG;
	if (q0 >= S.slots) return false;
	const uint32_t q1 = q0 + RS_WG;
	*k0 = q0 > S.lead ? q0 - S.lead : 0u;
	*k1 = q1 > S.lead ? (q1 - S.lead < S.count ? q1 - S.lead : S.count) : 0u;
	if (*k1 > *k0) {
		*first = (int)((S.o + *k0 * (uint32_t)R.M) / (uint32_t)R.L) - R.taps + 1;
		*span = (int)((S.o + (*k1 - 1u) * (uint32_t)R.M) / (uint32_t)R.L) - *first + 1;
	} else { *k1 = *k0; *first = 0; *span = 0; }
	return true;
}

/* phase 1: the block's input span into LDS; block 0 of a chained stream also writes the carry the next call reads */
RS_HD void rs_wg_stage(const RsRule &R, const RsStream &S, uint32_t block, int ch, int tid, float *carry, RsLds &L) {
	uint32_t k0, k1; int first, span;
	if (!rs_block(R, S, block, &k0, &k1, &first, &span)) return;
	for (int i = tid; i < span; i += RS_WG) L.x[i] = rs_x(R, S, carry, ch, first + i);
	if (block == 0 && (S.flags & RS_S_CARRY_OUT)) {
		float *out = carry + rs_carry_at(S.stream, (S.flags & RS_S_PARITY) ? 0u : 1u, ch);
		for (int i = tid; i < R.carry; i += RS_WG) out[i] = rs_x(R, S, carry, ch, (int)S.in - R.carry + i);      /* (in >= 1152 > 2 H - 1) */
	}
}

/* phase 2: slot q = block * RS_WG + tid */
RS_HD void rs_wg_slot(const RsRule &R, const RsStream &S, uint32_t block, int ch, int tid, const float *taps, float *part, void *out, const RsLds &L) {
	uint32_t k0, k1; int first, span;
	if (!rs_block(R, S, block, &k0, &k1, &first, &span)) return;
	const uint32_t q = block * RS_WG + (uint32_t)tid;
	if (q >= S.slots) return;
	const uint32_t parity = (S.flags & RS_S_PARITY) ? 1u : 0u;
	float v = 0.0f;
	if (q < S.lead) v = part[rs_part_at(S.stream, parity, ch) + q];
	else if (q - S.lead < S.count) {
		const uint32_t a = S.o + (q - S.lead) * (uint32_t)R.M;
		const float *h = taps + (size_t)(a % (uint32_t)R.L) * (size_t)R.taps;
		const float *x = L.x + ((int)(a / (uint32_t)R.L) - R.taps + 1 - first);
		float acc = 0.0f;
		for (int j = 0; j < R.taps; j++) acc = fmaf(h[j], x[j], acc);
		v = R.gain * acc;
	}
	if (R.form == RS_FORM_WAVEFORM) {
		const size_t at = ((size_t)S.frame0 * (size_t)R.channels + (size_t)ch) * R.row + q;
		if (R.dtype == RS_F32) static_cast<float *>(out)[at] = v;
		else static_cast<uint16_t *>(out)[at] = R.dtype == RS_F16 ? rs_f16_bits(v) : rs_bf16_bits(v);
		return;
	}
	const uint32_t fr = q / RS_FRAME, pos = q % RS_FRAME;
	if (fr < S.whole) {
		float *f = static_cast<float *>(out) + (size_t)(S.frame0 + fr) * (2 * RS_FRAME) + pos;
		if (R.channels == 1) { f[0] = v; f[RS_FRAME] = v; }
		else f[ch * RS_FRAME] = v;
	} else if (S.flags & RS_S_PART_OUT) part[rs_part_at(S.stream, parity ^ 1u, ch) + pos] = v;
}

#endif
