/*
 * The MPEG-1 Audio Layer II ENCODER of C ABI part 9 (include/jsmpeg_hip.h), stated once for the kernel (mp2_encode.hip), the
 * host runtime and the test-only simulator (tests/sim/sim_mp2_enc.cpp); tests/mp2_enc_ref.py restates it in numpy integers.
 * The reference has no encoder: the contract is this header, the bit-exact decoder of oracle/mp2_oracle.c judging every
 * stream, and a quantiser that is closed-loop against that decoder's arithmetic (mp2_tables.h: mp2_requantise).
 * Integers only behind the input conversion.
 *
 * HANDLE: sample_rate_index 0..2, channels 1 (mode mono) or 2 (mode stereo), bitrate_index 1..14 minus what ISO 11172-3
 * forbids for Layer II (32 / 48 / 56 / 80 kbit/s with two channels, 224 .. 384 with one).  No joint or dual mode, no CRC;
 * copyright, original and emphasis are 0.  Table, sblimit and nbal: mp2_table_select / mp2_nbal as they are.
 *
 * FRAME LENGTH AND PLACE (closed form, constant bit rate): N = 144000 kbps, b = N / fs, r = N mod fs.  Frame n of a stream --
 * n is the stream's ordinal, it goes on across chained calls -- has pad(n) = floor((n + 1) r / fs) - floor(n r / fs) (64-bit
 * products), b + pad(n) bytes, and begins n b + floor(n r / fs) bytes after the stream's begin.  Streams of a call begin at
 * multiples of 16; the bytes between a stream's end and the next multiple of 16 are zero (jsmpeg_hip_mp2_batch_upload_device
 * takes any ranges [begin, end) inside the buffer, end >= begin: it insists on nothing about the gaps).  Default PTS of frame
 * n: floor(n 1152 90000 / fs) ticks of 90 kHz.
 *
 * INPUT: float32 [frame][2][1152] (a mono handle reads channel 0); s = clamp(rne(x * 32767.0f), -32767, 32767), NaN -> 0 --
 * one binary32 multiply, no FMA.
 *
 * ANALYSIS (exact): 480 samples of history per channel in front of a frame (zeros before a stream's first frame, or the
 * carry of a chained call).  Per sub-block (36 of 32 samples) X is the newest 512 samples, newest first (ISO C.1.3);
 * Y[i] = sum_{j<8} W[i + 64 j] X[i + 64 j], W = the 512 integers of MP2_WINDOW_HALF_X2 (ISO's C[i] * 2^21), a 33-bit value;
 * acc[k] = sum_{i<64} COS[(2 k + 1)(i - 16) mod 128] Y[i], COS = MP2E_COS_Q15, |acc| < 2^53; S[k] = (acc + 2^27) >> 28
 * (arithmetic): ISO's subband sample times 2^23, which is the decoder's requantised value times 256; |S| < 2^25.  The kernel
 * folds the 64 terms of acc into 32 by the cosine's symmetries (mp2e_window_fold) and sums them in two halves of the folded
 * Y (mp2e_y_lo / mp2e_y_hi): the same integer.  tools/mp2_enc_bounds.py adds up the bounds.
 *
 * SCALEFACTORS: per (subband, channel) pair and part (3 x 12 samples) M = max |S|; the index is the largest i in 0..62 with
 * mp2_scalefactor(i) >= 2 M, 0 if there is none (62 when M = 0).  scfsi merges nothing lossy: indices (a, b, c): a = b = c one
 * scalefactor (code 2), a = b two (code 1: a, c), b = c two (code 3: a, b), otherwise three (code 0) -- mp2_dev.h's reading.
 *
 * BIT ALLOCATION (no psychoacoustic model; a total order, so the shape of the reduction cannot matter): pairs q = 2 sb + ch,
 * sb < sblimit.  A pair with M = 0 in all three parts is silent and never gets bits.  level(q) = -8 min(a, b, c); noise(q) =
 * level(q) - G(steps), G(0) = 0, G(steps) = round(24 log2(steps + 1)): 4 -> 48, 6 -> 62, 8 -> 72, 10 -> 80, 2^n -> 24 n.
 * left = 8 (b + pad) - 32 - sum nbal.  Raising a pair's code by one costs 12 (mp2_granule_bits(new) - mp2_granule_bits(old)),
 * plus 2 + 6 nsf(q) when the old code was 0.  A pair is open while it is not silent, its code is below 2^nbal - 1 and its
 * raise fits in `left`; every round raises the open pair with the largest (noise, then lower subband, then channel 0) --
 * one integer key, mp2e_alloc_key -- until no pair is open.  At most 540 rounds (two channels, Table 3-B.2b).
 *
 * QUANTISER (closed loop): the code of a sample is the argmin over 0 .. steps - 1 of |256 mp2_requantise(code, steps,
 * mp2_scalefactor(i)) - S|, ties to the lower code.  mp2_requantise falls monotonically with the code, so two binary searches
 * find it (mp2e_quantise).  Groups (3, 5, 9 steps): v = c0 + steps c1 + steps^2 c2, as mp2_dev.h splits it.
 *
 * FRAME: header, allocation codes, scfsi, scalefactors, 12 granules of sample codes in the decoder's order; every field's bit
 * position is a prefix sum over the pairs, as in k_mp2_matrix; the rest of the frame is zero bits.
 */
#ifndef JSMPEG_AMD_MP2_ENC_H
#define JSMPEG_AMD_MP2_ENC_H

#include <math.h>

#include "mp2_dev.h"
#include "mp2_enc_cos.h"
#include "mp2_window.h"

#define MP2E_WG 256
#define MP2E_HIST 480                             /* samples in front of a frame that its first sub-block's window reaches */
#define MP2E_STAGED (MP2E_HIST + MP2_SAMPLES_PER_FRAME)
#define MP2E_MAX_FRAME_BYTES 1728                 /* 384 kbit/s at 32 kHz; a padded frame of another rate is shorter */
#define MP2E_IMG_WORDS (MP2E_MAX_FRAME_BYTES / 4 + 4)
#define MP2E_MAX_ROUNDS 540

/* the handle's settings and what follows from them */
struct Mp2EncRule {
	int32_t sample_rate_index, channels, bitrate_index;
	int32_t high, sblimit;                        /* mp2_table_select */
	int32_t fs, b, r;                             /* frame length: b + pad(n) */
	int32_t nbal_bits;                            /* allocation bits of a frame */
};

MP2_HD int mp2e_rule_make(int sample_rate_index, int channels, int bitrate_index, Mp2EncRule *R) {
	if (sample_rate_index < 0 || sample_rate_index > 2 || bitrate_index < 1 || bitrate_index > 14 || channels < 1 || channels > 2) return -1;
	const int kbps = mp2_bitrate_kbps(bitrate_index);
	if (channels == 2 && (kbps == 32 || kbps == 48 || kbps == 56 || kbps == 80)) return -1;     /* ISO 11172-3 2.4.2.3, Layer II */
	if (channels == 1 && kbps >= 224) return -1;
	int high = 0;
	R->sample_rate_index = sample_rate_index; R->channels = channels; R->bitrate_index = bitrate_index;
	R->sblimit = mp2_table_select(bitrate_index, sample_rate_index, channels == 1, &high);
	R->high = high;
	R->fs = mp2_sample_rate(sample_rate_index);
	R->b = 144000 * kbps / R->fs;
	R->r = 144000 * kbps % R->fs;
	R->nbal_bits = channels * mp2_nbal_before(high, R->sblimit);
	return 0;
}
/* where frame n of a stream begins, counted from the stream's ordinal 0, and its length */
MP2_HD uint64_t mp2e_frame_offset(const Mp2EncRule &R, uint64_t n) { return n * (uint64_t)R.b + n * (uint64_t)R.r / (uint64_t)R.fs; }
MP2_HD uint32_t mp2e_frame_bytes(const Mp2EncRule &R, uint64_t n) { return (uint32_t)(mp2e_frame_offset(R, n + 1) - mp2e_frame_offset(R, n)); }
MP2_HD uint64_t mp2e_default_pts(const Mp2EncRule &R, uint64_t n) { return n * 1152ull * 90000ull / (uint64_t)R.fs; }

/* the input conversion: the one place with a float in it */
MP2_HD int mp2e_pcm_s16(float x) {
	if (x != x) return 0;
	const float v = x * 32767.0f;
	if (v >= 32767.0f) return 32767;
	if (v <= -32767.0f) return -32767;
	return (int)rintf(v);
}

/* the constants the kernel stages in LDS: the analysis window times 2^21 and the matrixing cosines times 2^15 */
struct Mp2EncTables { int32_t win[512]; int32_t cosq[128]; };
static inline void mp2e_tables_make(Mp2EncTables *T) {            /* host: the kernel gets them in device memory */
	for (int i = 0; i < 512; i++) {                /* mp2_window_at's symmetry, in integers */
		const int m = i <= 256 ? i : 512 - i;
		T->win[i] = (i <= 256 || (m & 63) == 0) ? MP2_WINDOW_HALF_X2[m] : -MP2_WINDOW_HALF_X2[m];
	}
	for (int m = 0; m < 128; m++) T->cosq[m] = MP2E_COS_Q15[m];
}

/* One frame of a call, planned by the host from the handle's records alone. */
#define MP2E_F_FIRST 1u        /* the stream's first frame of the call: its history is not in the input */
#define MP2E_F_CARRY_IN 2u     /* ... but in carry[parity] (chained, the stream has state); otherwise zeros */
#define MP2E_F_CARRY_OUT 4u    /* the stream's last frame of a chained call: writes carry[parity ^ 1] */
#define MP2E_F_PARITY 8u
struct Mp2EncFrame {
	const float *pcm;          /* [2][1152]; without MP2E_F_FIRST the frame before lies right in front of it */
	uint64_t out;              /* byte offset of the frame in the call's output */
	uint32_t bytes;            /* b + pad(n) */
	uint32_t tail;             /* zero bytes behind it: up to the next multiple of 16 behind a stream's last frame */
	uint32_t stream;           /* stream number: which carry */
	uint32_t flags;
};
#define MP2E_CARRY_WORDS (2 * 2 * MP2E_HIST)      /* int16 per stream: [parity][channel][480] */

/* THE CHAIN: the host's record per stream number.  A chained call continues stream s at ordinal n with the history in
 * carry[parity]; the workgroup of its first frame reads that buffer, the workgroup of its last frame writes carry[parity ^ 1]
 * from the input (a frame is longer than the history), and the record then flips: nothing reads and writes one buffer in one
 * call.  A stream without frames in a call keeps its record; an unchained call touches neither records nor carries. */
struct Mp2EncChain { uint32_t have, parity; uint64_t n; };
#define MP2E_CHAIN 2u          /* (= JSMPEG_HIP_MP2_ENC_CHAIN) */

/* Plans a call on the host: stream i has frames[i] contiguous frames from pcm[i] and the number numbers[i] (NULL: i).  Fills
 * list[] (sum of frames), begin[i] / end[i] (byte ranges of the streams in the output) and returns the call's bytes: every
 * stream begins at a multiple of 16, zeros fill up to the next one behind it.  Reads the records, changes nothing. */
static inline uint64_t mp2e_plan(const Mp2EncRule &R, const float *const *pcm, const uint32_t *frames, const uint32_t *numbers, uint32_t n_streams,
                                 uint32_t flags, const Mp2EncChain *rec, Mp2EncFrame *list, uint64_t *begin, uint64_t *end) {
	uint64_t at = 0;
	uint32_t k = 0;
	for (uint32_t i = 0; i < n_streams; i++) {
		const uint32_t s = numbers ? numbers[i] : i;
		const bool cont = (flags & MP2E_CHAIN) && rec[s].have;
		const uint64_t n0 = cont ? rec[s].n : 0;
		const uint32_t parity = (flags & MP2E_CHAIN) ? rec[s].parity : 0;
		begin[i] = at;
		for (uint32_t f = 0; f < frames[i]; f++, k++) {
			Mp2EncFrame &F = list[k];
			F.pcm = pcm[i] + (size_t)f * 2 * MP2_SAMPLES_PER_FRAME;
			F.out = begin[i] + mp2e_frame_offset(R, n0 + f) - mp2e_frame_offset(R, n0);
			F.bytes = mp2e_frame_bytes(R, n0 + f);
			F.tail = 0;
			F.stream = s;
			F.flags = (f == 0 ? MP2E_F_FIRST | (cont ? MP2E_F_CARRY_IN : 0u) : 0u) | (parity ? MP2E_F_PARITY : 0u) |
			          ((flags & MP2E_CHAIN) && f + 1 == frames[i] ? MP2E_F_CARRY_OUT : 0u);
			at = F.out + F.bytes;
		}
		end[i] = at;
		at = (at + 15) & ~15ull;
		if (frames[i]) list[k - 1].tail = (uint32_t)(at - end[i]);
	}
	return at;
}
/* ... and, once the call is enqueued, moves the records of a chained call on */
static inline void mp2e_plan_commit(const uint32_t *frames, const uint32_t *numbers, uint32_t n_streams, uint32_t flags, Mp2EncChain *rec) {
	if (!(flags & MP2E_CHAIN)) return;
	for (uint32_t i = 0; i < n_streams; i++) {
		Mp2EncChain &c = rec[numbers ? numbers[i] : i];
		if (!frames[i]) continue;
		c.n = (c.have ? c.n : 0) + frames[i]; c.have = 1; c.parity ^= 1u;
	}
}

/* what a frame's workgroup keeps in LDS */
struct Mp2EncLds {
	int16_t x[2][MP2E_STAGED];                    /* [channel] history, then the frame */
	Mp2EncTables T;
	int32_t y[2][12][32][2];                      /* one part's folded Y (mp2e_window_fold): low 16 bits, the rest (mp2e_y_lo / _hi) */
	int32_t S[2][36][32];                         /* [channel][sub-block][subband] */
	uint32_t img[MP2E_IMG_WORDS];                 /* the frame's bits, word w = bits 32 w .. 32 w + 31, first bit highest */
	uint8_t sfi[64][4];                           /* [q] scalefactor index per part */
	uint8_t loud[64][4];                          /* [q] M != 0 per part */
	uint32_t key[16][64];                         /* [code][q] the pair's allocation key at that code (mp2e_alloc_table) */
	uint8_t code[64], sel[64], nsf[64];
	uint16_t steps[64], gbits[64], bit_in_granule[64];
	uint64_t coded_mask, nsf_plane[2], gbits_plane[6];    /* prefix sums over the pairs as bit planes (mp2_dev.h) */
	int32_t left, sample_bit, granule_bits;
};

#if defined(__HIP_DEVICE_COMPILE__)
#define MP2E_LDS_OR(word, v) atomicOr(&(word), (v))
#else
#define MP2E_LDS_OR(word, v) ((word) |= (v))
#endif

/* n <= 32 bits of `value` at bit `pos` of the image; fields of different lanes share words, never bits */
MP2_HD void mp2e_put(Mp2EncLds &L, uint32_t pos, int n, uint32_t value) {
	if (n == 0) return;
	const uint32_t idx = pos >> 5;
	const uint64_t v = (uint64_t)value << (64 - (int)(pos & 31) - n);
	const uint32_t hi = (uint32_t)(v >> 32), lo = (uint32_t)v;
	if (hi) MP2E_LDS_OR(L.img[idx], hi);
	if (lo) MP2E_LDS_OR(L.img[idx + 1], lo);
}
/* byte k of the frame, zero behind its bits */
MP2_HD uint32_t mp2e_img_byte(const Mp2EncLds &L, uint32_t k, uint32_t bytes) {
	return k < bytes ? (L.img[k >> 2] >> (24 - 8 * (int)(k & 3))) & 255u : 0u;
}

/* ---- analysis */
MP2_HD int32_t mp2e_y_lo(int64_t y) { return (int32_t)(y & 0xffff); }
MP2_HD int32_t mp2e_y_hi(int64_t y) { return (int32_t)(y >> 16); }
/* Y[i] of the sub-block whose newest sample is *newest */
MP2_HD int64_t mp2e_window_sum(const int16_t *newest, const int32_t *win, int i) {
	int64_t y = 0;
#pragma unroll
	for (int j = 0; j < 8; j++) y += (int64_t)win[i + 64 * j] * (int64_t)newest[-(i + 64 * j)];
	return y;
}
/* The cosine of (2 k + 1)(i - 16) pi / 64 is even in t = i - 16 and changes sign under t -> 64 - t, so the 64 terms are 32:
 * Z[0] = Y[16], Z[t] = Y[16 + t] + Y[16 - t] (t = 1 .. 16), Z[t] = Y[16 + t] - Y[80 - t] (t = 17 .. 31); Y[48] meets a zero.
 * acc[k] = sum_{t<32} COS[(2 k + 1) t mod 128] Z[t]: the same integer (the products are exact), a 34-bit Z. */
MP2_HD int64_t mp2e_window_fold(const int16_t *newest, const int32_t *win, int t) {
	const int64_t a = mp2e_window_sum(newest, win, 16 + t);
	if (t == 0) return a;
	return t <= 16 ? a + mp2e_window_sum(newest, win, 16 - t) : a - mp2e_window_sum(newest, win, 80 - t);
}
/* S[k] from the 32 Z of a sub-block, z[t][0] = low half, z[t][1] = high half */
MP2_HD int32_t mp2e_matrix_sum(const int32_t (*z)[2], const int32_t *cosq, int k) {
	int64_t lo = 0, hi = 0;
	for (int t = 0; t < 32; t++) {
		const int32_t c = cosq[((2 * k + 1) * t) & 127];
		lo += (int64_t)c * (int64_t)z[t][0];
		hi += (int64_t)c * (int64_t)z[t][1];
	}
	const int64_t acc = hi * 65536 + lo;
	return (int32_t)((acc + ((int64_t)1 << 27)) >> 28);
}

/* ---- scalefactor index of a part's largest magnitude */
MP2_HD int mp2e_scale_index(int M) {
	for (int i = 62; i > 0; i--) if (mp2_scalefactor(i) >= 2 * M) return i;
	return 0;
}
/* scfsi of the three indices, and how many are transmitted */
MP2_HD int mp2e_scfsi(int a, int b, int c) { return (a == b && b == c) ? 2 : (a == b ? 1 : (b == c ? 3 : 0)); }
MP2_HD int mp2e_nsf(int sel) { return sel == 0 ? 3 : (sel == 2 ? 1 : 2); }

/* ---- allocation */
MP2_HD int mp2e_gain(int steps) {
	if (steps == 0) return 0;
	if (steps == 3) return 48;
	if (steps == 5) return 62;
	if (steps == 9) return 80;
	return 24 * mp2_code_bits(steps);
}
struct Mp2EncPair { int open, code, top, nsf, level; };       /* a lane's pair during the loop */
/* 0: the pair is closed.  Otherwise (noise + 1024) << 16 | (63 - q) << 10 | the raise's cost in bits: the largest key is the
 * round's pair, and its low ten bits are what the round takes from `left` */
MP2_HD uint32_t mp2e_alloc_key(const Mp2EncRule &R, const Mp2EncPair &P, int q, int left) {
	if (!P.open || P.code >= P.top) return 0;
	const int so = mp2_steps(R.high, q >> 1, P.code), sn = mp2_steps(R.high, q >> 1, P.code + 1);
	const int cost = 12 * (mp2_granule_bits(sn) - mp2_granule_bits(so)) + (P.code == 0 ? 2 + 6 * P.nsf : 0);
	if (cost > left) return 0;
	const int noise = P.level - mp2e_gain(so);
	return ((uint32_t)(noise + 1024) << 16) | ((uint32_t)(63 - q) << 10) | (uint32_t)cost;
}
/* A pair's key depends on its code alone until `left` runs short of its cost: lane q writes its sixteen keys down once
 * (mp2e_alloc_table), and a round is a look-up, a compare with `left` and the maximum (mp2e_alloc_pick) */
#define MP2E_KEY_COST 1023u
#define MP2E_KEY_PAIR(key) (63 - (int)(((key) >> 10) & 63u))

/* ---- quantiser */
/* the smallest code of 0 .. steps - 1 whose requantised value is <= target; steps if there is none.  The search begins in
 * [lo, hi] when the values there bracket the target and in 0 .. steps otherwise: a guess saves steps, it decides nothing */
MP2_HD int mp2e_first_le(int steps, int sf, int target, int lo, int hi) {
	if (lo < 0 || (lo > 0 && mp2_requantise(lo - 1, steps, sf) <= target)) lo = 0;
	if (hi > steps || (hi < steps && mp2_requantise(hi, steps, sf) > target)) hi = steps;
	while (lo < hi) {
		const int mid = (lo + hi) >> 1;
		if (mp2_requantise(mid, steps, sf) <= target) hi = mid; else lo = mid + 1;
	}
	return lo;
}
MP2_HD int mp2e_quantise(int S, int steps, int sf) {
	/* where the code would lie if the requantiser were exact: 256 (mid - code) scale sf / 2^24 = S */
	const float guess = (float)(((steps + 1) >> 1) - 1) - (float)S * 65536.0f / ((float)mp2_requantise_scale(steps) * (float)(sf > 0 ? sf : 1));
	const int g = guess <= 0.0f ? 0 : (guess >= (float)steps ? steps : (int)guess);
	const int c1 = mp2e_first_le(steps, sf, S >> 8, g - 2, g + 3);   /* the first code at or below S; the codes before it lie above */
	if (c1 == 0) return 0;
	const int r0 = mp2_requantise(c1 - 1, steps, sf);
	const int c0 = mp2e_first_le(steps, sf, r0, c1 - 3, c1 - 1);     /* the lowest code with the value just above S */
	if (c1 == steps) return c0;
	const int e0 = 256 * r0 - S, e1 = S - 256 * mp2_requantise(c1, steps, sf);
	return e1 < e0 ? c1 : c0;
}

/* ---------------------------------------------------------------------------------------------------------
 * Workgroup bodies of k_mp2e_frame (workgroup = frame, MP2E_WG lanes), a barrier between each; the simulator calls them in
 * plain loops. */

/* tables, the frame's samples behind their history, an empty image */
MP2_HD void mp2e_wg_stage(const Mp2EncRule &R, const Mp2EncFrame &F, const Mp2EncTables *tables, const int16_t *carry, int tid, Mp2EncLds &L) {
	const int32_t *t = reinterpret_cast<const int32_t *>(tables);
	int32_t *lt = reinterpret_cast<int32_t *>(&L.T);
	for (int i = tid; i < (int)(sizeof(Mp2EncTables) / 4); i += MP2E_WG) lt[i] = t[i];
	for (int i = tid; i < MP2E_IMG_WORDS; i += MP2E_WG) L.img[i] = 0;
	const int16_t *cin = carry + (size_t)F.stream * MP2E_CARRY_WORDS + ((F.flags & MP2E_F_PARITY) ? 2 * MP2E_HIST : 0);
	for (int i = tid; i < R.channels * MP2E_STAGED; i += MP2E_WG) {
		const int ch = i >= MP2E_STAGED, k = i - ch * MP2E_STAGED;
		int s;
		if (k >= MP2E_HIST) s = mp2e_pcm_s16(F.pcm[ch * MP2_SAMPLES_PER_FRAME + k - MP2E_HIST]);
		else if (!(F.flags & MP2E_F_FIRST)) s = mp2e_pcm_s16(F.pcm[(ch - 2) * MP2_SAMPLES_PER_FRAME + MP2_SAMPLES_PER_FRAME - MP2E_HIST + k]);
		else s = (F.flags & MP2E_F_CARRY_IN) ? cin[ch * MP2E_HIST + k] : 0;
		L.x[ch][k] = (int16_t)s;
	}
	if (tid == 0) {
		L.coded_mask = 0; L.nsf_plane[0] = L.nsf_plane[1] = 0;
		for (int k = 0; k < 6; k++) L.gbits_plane[k] = 0;
	}
}
/* the last 480 samples of the frame into the stream's other carry */
MP2_HD void mp2e_wg_carry_out(const Mp2EncRule &R, const Mp2EncFrame &F, int16_t *carry, int tid, const Mp2EncLds &L) {
	if (!(F.flags & MP2E_F_CARRY_OUT)) return;
	int16_t *cout = carry + (size_t)F.stream * MP2E_CARRY_WORDS + ((F.flags & MP2E_F_PARITY) ? 0 : 2 * MP2E_HIST);
	for (int i = tid; i < R.channels * MP2E_HIST; i += MP2E_WG) {
		const int ch = i >= MP2E_HIST, k = i - ch * MP2E_HIST;
		cout[ch * MP2E_HIST + k] = L.x[ch][MP2_SAMPLES_PER_FRAME + k];
	}
}
/* part 0..2: the Y of its 12 sub-blocks, then their S */
MP2_HD void mp2e_wg_window(const Mp2EncRule &R, int part, int tid, Mp2EncLds &L) {
	for (int item = tid; item < R.channels * 12 * 32; item += MP2E_WG) {
		const int t = item & 31, pp = (item >> 5) % 12, ch = item / (12 * 32);
		const int64_t z = mp2e_window_fold(&L.x[ch][MP2E_HIST + 32 * (part * 12 + pp) + 31], L.T.win, t);
		L.y[ch][pp][t][0] = mp2e_y_lo(z); L.y[ch][pp][t][1] = mp2e_y_hi(z);
	}
}
MP2_HD void mp2e_wg_matrix(const Mp2EncRule &R, int part, int tid, Mp2EncLds &L) {
	for (int item = tid; item < R.channels * 12 * 32; item += MP2E_WG) {
		const int k = item & 31, pp = (item >> 5) % 12, ch = item / (12 * 32);
		L.S[ch][part * 12 + pp][k] = mp2e_matrix_sum(L.y[ch][pp], L.T.cosq, k);
	}
}
/* lanes over (pair, part): the scalefactor index */
MP2_HD void mp2e_wg_scale(const Mp2EncRule &R, int tid, Mp2EncLds &L) {
	for (int item = tid; item < 192; item += MP2E_WG) {
		const int q = item & 63, part = item >> 6, sb = q >> 1, ch = q & 1;
		int M = 0;
		if (sb < R.sblimit && ch < R.channels)
			for (int t = 0; t < 12; t++) {
				const int v = L.S[ch][part * 12 + t][sb];
				const int a = v < 0 ? -v : v;
				M = a > M ? a : M;
			}
		L.sfi[q][part] = (uint8_t)mp2e_scale_index(M);
		L.loud[q][part] = (uint8_t)(M != 0);
	}
}
/* lane q < 64: its pair before the allocation loop; scfsi and nsf into LDS */
MP2_HD Mp2EncPair mp2e_pair_begin(const Mp2EncRule &R, int q, Mp2EncLds &L) {
	const int sb = q >> 1, ch = q & 1;
	const int a = L.sfi[q][0], b = L.sfi[q][1], c = L.sfi[q][2];
	const int sel = mp2e_scfsi(a, b, c);
	Mp2EncPair P;
	P.open = sb < R.sblimit && ch < R.channels && (L.loud[q][0] | L.loud[q][1] | L.loud[q][2]);
	P.code = 0;
	P.top = (1 << mp2_nbal(R.high, sb)) - 1;
	P.nsf = mp2e_nsf(sel);
	const int m = a < b ? a : b;
	P.level = -8 * (m < c ? m : c);
	L.sel[q] = (uint8_t)sel; L.nsf[q] = (uint8_t)P.nsf;
	return P;
}
MP2_HD int mp2e_left_begin(const Mp2EncRule &R, const Mp2EncFrame &F) { return 8 * (int)F.bytes - 32 - R.nbal_bits; }
MP2_HD void mp2e_alloc_table(const Mp2EncRule &R, Mp2EncPair P, int q, Mp2EncLds &L) {
	for (int code = 0; code < 16; code++) {
		P.code = code;
		L.key[code][q] = mp2e_alloc_key(R, P, q, 1 << 30);
	}
}
MP2_HD uint32_t mp2e_alloc_pick(const Mp2EncLds &L, int q, int code, int left) {
	const uint32_t key = L.key[code][q];
	return (int)(key & MP2E_KEY_COST) > left ? 0u : key;
}
/* lane q < 64 after the loop: what the pair got, and its share of the prefix sums */
MP2_HD void mp2e_pair_end(const Mp2EncRule &R, const Mp2EncPair &P, int q, int left, Mp2EncLds &L) {
	const int steps = mp2_steps(R.high, q >> 1, P.code), gbits = mp2_granule_bits(steps);
	L.code[q] = (uint8_t)P.code; L.steps[q] = (uint16_t)steps; L.gbits[q] = (uint16_t)gbits;
	mp2_plane_set(L.coded_mask, q, P.code != 0);
	mp2_plane_set(L.nsf_plane[0], q, P.code != 0 && (P.nsf & 1));
	mp2_plane_set(L.nsf_plane[1], q, P.code != 0 && (P.nsf >> 1));
#pragma unroll
	for (int k = 0; k < 6; k++) mp2_plane_set(L.gbits_plane[k], q, (gbits >> k) & 1);
	if (q == 0) L.left = left;
}
MP2_HD int mp2e_gbits_before(const Mp2EncLds &L, int q) {
	int g = 0;
#pragma unroll
	for (int k = 0; k < 6; k++) g += mp2_plane_before(L.gbits_plane[k], q) << k;
	return g;
}
/* lane q < 64: header (lane 0), the pair's allocation code, scfsi and scalefactors, each at its prefix sum */
MP2_HD void mp2e_wg_side(const Mp2EncRule &R, const Mp2EncFrame &F, int q, Mp2EncLds &L) {
	const int sb = q >> 1, ch = q & 1;
	const uint32_t scfsi_bit = 32u + (uint32_t)R.nbal_bits;
	const uint32_t sf_bit = scfsi_bit + 2u * (uint32_t)(mp2_plane_before(L.coded_mask, 63) + (int)(L.coded_mask >> 63));
	const uint64_t n0 = L.nsf_plane[0], n1 = L.nsf_plane[1];
	if (q == 0) {
		const uint32_t pad = F.bytes - (uint32_t)R.b;
		/* sync, MPEG-1, Layer II, no CRC | bit rate, sampling frequency, padding, private 0 | mode, mode extension 0, copyright 0,
		 * original 0, emphasis 0 */
		mp2e_put(L, 0, 32, 0xfffd0000u | ((uint32_t)R.bitrate_index << 12) | ((uint32_t)R.sample_rate_index << 10) | (pad << 9) |
		                   ((uint32_t)(R.channels == 1 ? MP2_MODE_MONO : MP2_MODE_STEREO) << 6));
		L.sample_bit = (int32_t)(sf_bit + 6u * (uint32_t)(mp2_plane_before(n0, 63) + (int)(n0 >> 63) + 2 * (mp2_plane_before(n1, 63) + (int)(n1 >> 63))));
		L.granule_bits = mp2e_gbits_before(L, 63) + (int)L.gbits[63];
	}
	L.bit_in_granule[q] = (uint16_t)mp2e_gbits_before(L, q);
	if (sb >= R.sblimit || ch >= R.channels) return;
	const int nbal = mp2_nbal(R.high, sb), code = L.code[q];
	mp2e_put(L, 32u + (uint32_t)(R.channels * mp2_nbal_before(R.high, sb) + ch * nbal), nbal, (uint32_t)code);
	if (!code) return;
	const int sel = L.sel[q], a = L.sfi[q][0], b = L.sfi[q][1], c = L.sfi[q][2];
	mp2e_put(L, scfsi_bit + 2u * (uint32_t)mp2_plane_before(L.coded_mask, q), 2, (uint32_t)sel);
	const uint32_t at = sf_bit + 6u * (uint32_t)(mp2_plane_before(n0, q) + 2 * mp2_plane_before(n1, q));
	if (sel == 0) mp2e_put(L, at, 18, (uint32_t)((a << 12) | (b << 6) | c));
	else if (sel == 1) mp2e_put(L, at, 12, (uint32_t)((a << 6) | c));
	else if (sel == 3) mp2e_put(L, at, 12, (uint32_t)((a << 6) | b));
	else mp2e_put(L, at, 6, (uint32_t)a);
}
/* lanes over (granule, pair): three samples quantised and packed */
MP2_HD void mp2e_wg_quantise(int tid, Mp2EncLds &L) {
	for (int item = tid; item < 768; item += MP2E_WG) {
		const int g = item >> 6, q = item & 63, sb = q >> 1, ch = q & 1;
		const int steps = L.steps[q];
		if (!steps) continue;
		const int sf = mp2_scalefactor(L.sfi[q][g >> 2]);
		const uint32_t c0 = (uint32_t)mp2e_quantise(L.S[ch][3 * g][sb], steps, sf);
		const uint32_t c1 = (uint32_t)mp2e_quantise(L.S[ch][3 * g + 1][sb], steps, sf);
		const uint32_t c2 = (uint32_t)mp2e_quantise(L.S[ch][3 * g + 2][sb], steps, sf);
		const uint32_t at = (uint32_t)L.sample_bit + (uint32_t)g * (uint32_t)L.granule_bits + L.bit_in_granule[q];
		const int nb = mp2_code_bits(steps);
		if (mp2_grouped(steps)) mp2e_put(L, at, nb, c0 + (uint32_t)steps * (c1 + (uint32_t)steps * c2));
		else { mp2e_put(L, at, nb, c0); mp2e_put(L, at + (uint32_t)nb, nb, c1); mp2e_put(L, at + 2u * (uint32_t)nb, nb, c2); }
	}
}
/* the frame and the zeros behind it: one owner per output byte, whole dwords inside, bytes at the unaligned ends (frames of a
 * stream share dwords, never bytes) */
MP2_HD void mp2e_wg_store(const Mp2EncFrame &F, uint8_t *out, int tid, const Mp2EncLds &L) {
	const uint64_t begin = F.out, end = F.out + F.bytes + F.tail, w0 = begin & ~3ull;
	const int words = (int)((end - w0 + 3) >> 2);
	for (int i = tid; i < words; i += MP2E_WG) {
		const uint64_t w = w0 + 4ull * (uint64_t)i;
		uint32_t b[4];
#pragma unroll
		for (int k = 0; k < 4; k++) b[k] = (w + k >= begin && w + k < end) ? mp2e_img_byte(L, (uint32_t)(w + k - begin), F.bytes) : 0u;
		if (w >= begin && w + 4 <= end) *reinterpret_cast<uint32_t *>(out + w) = b[0] | (b[1] << 8) | (b[2] << 16) | (b[3] << 24);
		else {
#pragma unroll
			for (int k = 0; k < 4; k++) if (w + k >= begin && w + k < end) out[w + k] = (uint8_t)b[k];
		}
	}
}
/* lane 0: coded pairs, bits used, bits left over, the largest allocation code */
MP2_HD void mp2e_wg_stats(const Mp2EncFrame &F, uint32_t *stats, const Mp2EncLds &L) {
	uint32_t top = 0;
	for (int q = 0; q < 64; q++) top = L.code[q] > top ? L.code[q] : top;
	const uint32_t used = (uint32_t)L.sample_bit + 12u * (uint32_t)L.granule_bits;
	stats[0] = (uint32_t)mp2_plane_before(L.coded_mask, 63) + (uint32_t)(L.coded_mask >> 63);
	stats[1] = used; stats[2] = 8u * F.bytes - used; stats[3] = top;
}

#endif
