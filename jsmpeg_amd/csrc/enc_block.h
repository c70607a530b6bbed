/*
 * MPEG-1 INTRA ENCODER, the per-macroblock device functions (include/jsmpeg_hip.h part 8): what the lane bodies of enc_pass.h --
 * and through them the kernels of encode.hip and the CPU simulator (tests/sim/sim_encode_pass.cpp) -- share.  Host + device; on
 * the CPU an atomic OR is a plain OR and a lane's slot of LDS is a local array, nothing else differs. tests/enc_ref.py restates
 * every formula below in numpy.
 *
 * I pictures here, one quantiser scale per picture, the default intra matrix, one slice per macroblock row; P pictures and the
 * closed loop they need (the encoder's reference must be the decoder's reconstruction) are enc_motion.h's, built on what is
 * below.  OUT OF SCOPE (say so to whoever asks): B pictures, a VBV model (rate control by a budget per GOP: enc_rate.h), custom matrices, a Node binding.
 * (Scaled and cropped YCbCr input: enc_scale.h.)
 *
 * FORWARD DCT, exactly:  with C[k][n] = round(2^14 * c_k * cos((2n + 1) k pi / 16)), c_0 = sqrt(1/8), c_k = 1/2
 * (jm_enc_make_const below, 16-bit signed), and the block's pixels x[y][n] in 0 .. 255 (MPEG-1 intra blocks are not level-shifted),
 *     t[y][v]  = sum_n C[v][n] * x[y][n]                         32-bit
 *     a[u][v]  = sum_y C[u][y] * t[y][v]                         below 2^39 (computed as two 32-bit sums: jm_enc_block_levels)
 *     c8[u][v] = (a[u][v] + 2^24) >> 25                          arithmetic shift: ONE rounding, at the end
 * c8 is EIGHT TIMES the orthonormal DCT coefficient (2^28 / 8 = 2^25): three fractional bits go into the quantiser.
 * Bounds (tools/fdct_bounds.py adds up the table, as tools/idct_bounds.py does for the inverse): sum_n |C[k][n]| <= 46344,
 * so |t| <= 255 * 46344 = 11 817 720 < 2^24 and |a| <= 46344 * 11 817 720 < 2^39: int32 and int64 hold them with room.
 * The same sums bound the residual of a predicted block, x in -255 .. 255 (enc_motion.h; tools/fdct_bounds.py --signed): there
 * |t| reaches 11 817 720 itself, the high and low halves of t stay within +-2886 and 0 .. 4095, their sums below 2^28.
 *
 * QUANTISER, for the reference's dequantiser (mpeg1.c decode_block, oracle/mpeg1_oracle.c), W = the default intra matrix:
 *     DC level = clamp((c8[0][0] + 32) >> 6, 0, 255)             round(dc / 8)
 *     AC level = sign(c8) * min(255, (2 |c8| + d) / (2 d)), d = q * W[i]      round-to-nearest of 8 c / (q W[i]), halves away
 *                                                                             from zero; integer division
 * SYNTAX of a macroblock of an I picture (ISO 11172-2 as the reference reads it): increment "1", type
 * "1" (intra, no quantiser change), then per block dct_dc_size + differential against the component's predictor (128 at the
 * slice start), run / level pairs (table B.14, "11s" for (0, 1), escape: 8-bit level for |level| <= 127, else 0x00 / 0x80 +
 * 8 bits), end_of_block "10".
 *
 * TWO PASSES, no serial walk over macroblocks: jm_enc_measure gives a macroblock's bits WITHOUT its six DC codes and its six DC
 * levels; jm_enc_dc_bits gives the DC codes' bits once the predecessor's levels are known (the scan: jm_enc_scan_slice);
 * jm_enc_write writes the macroblock at its bit offset into a zeroed range: its first and last word by an atomic OR
 * (neighbours share them), the words between by plain stores.
 *
 * RGB IN (tensor input), full-range BT.601 -- the inverse of the renderer the project matches (canvas2d.js) --, 16-bit fixed point:
 *     Y  = (19595 R + 38470 G + 7471 B + 2^15) >> 16
 *     Cr = clamp((32768 Rs - 27439 Gs -  5329 Bs + 128 * 2^18 + 2^17) >> 18)     Rs, Gs, Bs: sums over the 2x2 pixels
 *     Cb = clamp((-11059 Rs - 21709 Gs + 32768 Bs + 128 * 2^18 + 2^17) >> 18)    (the rounded mean, one rounding)
 * over the picture extended to the coded size by edge replication (source coordinates clamped to the display size).
 */
#pragma once
#include <stdint.h>
#include <string.h>

#include "mpeg1_dev.h"
#include "mpeg1_vlc_codes.h"

#define JM_ENC_MAX_RUN 32u       /* table B.14 holds runs 0 .. 31 */
#define JM_ENC_MAX_LEVEL 41u     /* ... and levels 1 .. 40 */
#define JM_ENC_SLICE_HEAD_BITS 38u   /* 00 00 01 row | quantiser_scale (5) | extra_bit_slice (1) */
#define JM_ENC_PIC_HEAD_BYTES 28u    /* sequence header 12, GOP header 8, picture header 8 */
#define JM_ENC_LEAD_GAP 16u      /* 0xff bytes in front of the first stream (jsmpeg_hip_batch_attach_device's rule) */
#define JM_ENC_TAIL 256u         /* 0xff bytes behind the total (readable, the same rule) */

/* the encoder's code tables, built from the Annex-B strings at compile time (jm_enc_make_tables), uploaded once per handle */
struct JmEncTables {
	uint32_t coeff[JM_ENC_MAX_RUN][JM_ENC_MAX_LEVEL];   /* [run][|level|]: (length << 16) | bits, WITHOUT the sign bit; 0: no code (escape) */
	uint16_t dc_luma[9], dc_chroma[9];                  /* [size]: (length << 8) | bits */
	uint32_t recip[32][64];                             /* [q][i]: floor(2^32 / (2 q W[i])) + 1 -- the quantiser's division, see jm_enc_block_levels */
};

constexpr uint32_t jm_enc_code(const char *s) {
	uint32_t v = 0, n = 0;
	while (s[n]) { v = v * 2 + (uint32_t)(s[n] - '0'); n++; }
	return (n << 16) | v;
}
constexpr uint16_t jm_enc_code8(const char *s) { return (uint16_t)(((jm_enc_code(s) >> 16) << 8) | (jm_enc_code(s) & 0xffu)); }
constexpr JmEncTables jm_enc_make_tables() {
	JmEncTables t{};
#define X(bits, run, level) t.coeff[run][level] = jm_enc_code(bits);
	MPEG1_VLC_DCT_COEFF(X)
#undef X
#define X(bits, size) t.dc_luma[size] = jm_enc_code8(bits);
	MPEG1_VLC_DCSIZE_LUMA(X)
#undef X
#define X(bits, size) t.dc_chroma[size] = jm_enc_code8(bits);
	MPEG1_VLC_DCSIZE_CHROMA(X)
#undef X
	const uint8_t w[64] = MPEG1_DEFAULT_INTRA_QUANT_INIT;
	for (uint32_t q = 1; q < 32; q++)
		for (uint32_t i = 0; i < 64; i++) t.recip[q][i] = (uint32_t)((1ull << 32) / (2u * q * w[i])) + 1u;
	return t;
}

struct JmEncConst {
	int16_t cos[8][8];
	uint8_t w[64];       /* default intra matrix, raster */
	uint8_t izz[64];     /* raster position -> scan index */
};
constexpr JmEncConst jm_enc_make_const() {
	JmEncConst c = { {
		{ 5793,  5793,  5793,  5793,  5793,  5793,  5793,  5793 },
		{ 8035,  6811,  4551,  1598, -1598, -4551, -6811, -8035 },
		{ 7568,  3135, -3135, -7568, -7568, -3135,  3135,  7568 },
		{ 6811, -1598, -8035, -4551,  4551,  8035,  1598, -6811 },
		{ 5793, -5793, -5793,  5793,  5793, -5793, -5793,  5793 },
		{ 4551, -8035,  1598,  6811, -6811, -1598,  8035, -4551 },
		{ 3135, -7568,  7568, -3135, -3135,  7568, -7568,  3135 },
		{ 1598, -4551,  6811, -8035,  8035, -6811,  4551, -1598 } },
		MPEG1_DEFAULT_INTRA_QUANT_INIT, {} };
	const uint8_t zz[64] = MPEG1_ZIGZAG_INIT;
	for (int i = 0; i < 64; i++) c.izz[zz[i]] = (uint8_t)i;
	return c;
}

/* ------------------------------------------------------------------ bits out
 * The output is a big-endian bit string in a buffer of 32-bit words (16-byte aligned base); a writer starts at any bit and
 * ORs its first and its last word in -- they belong to its neighbours too -- and stores the words between. */
struct JmEncBits {
	uint32_t *words;
	uint64_t acc;        /* pending bits, from bit 63 down */
	uint64_t w;          /* word the top 32 bits of acc go to */
	uint32_t fill;       /* bits of acc in use (the bits in front of the start included), < 32 between calls */
	uint32_t shared;     /* the next word out is the writer's first: a neighbour may own bits of it */
};
JM_HD void jm_enc_or(uint32_t *p, uint32_t v) {
	if (!v) return;
#if defined(__HIP_DEVICE_COMPILE__)
	atomicOr(p, v);
#else
	*p |= v;
#endif
}
JM_HD JmEncBits jm_enc_bits_at(uint32_t *words, uint64_t bitpos) {
	JmEncBits b;
	b.words = words; b.acc = 0; b.w = bitpos >> 5; b.fill = (uint32_t)(bitpos & 31u); b.shared = 1;
	return b;
}
/* n in 1 .. 32, v < 2^n */
JM_HD void jm_enc_put(JmEncBits &b, uint32_t v, uint32_t n) {
	b.acc |= (uint64_t)v << (64u - b.fill - n);
	b.fill += n;
	if (b.fill >= 32u) {
		/* a word between the writer's first and last is all its own: a plain store; the first and the last are ORed in */
		const uint32_t word = __builtin_bswap32((uint32_t)(b.acc >> 32));
		if (b.shared) jm_enc_or(b.words + b.w, word); else b.words[b.w] = word;
		b.shared = 0;
		b.w++; b.acc <<= 32; b.fill -= 32u;
	}
}
JM_HD void jm_enc_flush(JmEncBits &b) {
	if (b.fill) jm_enc_or(b.words + b.w, __builtin_bswap32((uint32_t)(b.acc >> 32)));
	b.acc = 0; b.fill = 0;
}

/* ------------------------------------------------------------------ one block
 * Rows of 8 pixels at px + y * stride (8-byte aligned) -> the DC level (returned) and the AC levels in SCAN order at
 * zz[z * zs], z = 1 .. 63 (zs: 1 on the CPU, the lanes of a wavefront side by side in LDS on the device). */

JM_HD int32_t jm_enc_mad24(int32_t a, int32_t b, int32_t acc) {        /* a, b within 24 bits signed */
#if defined(__HIP_DEVICE_COMPILE__)
	return __mul24(a, b) + acc;
#else
	return a * b + acc;
#endif
}
JM_HD uint32_t jm_enc_mulhi(uint32_t a, uint32_t b) { return (uint32_t)(((uint64_t)a * b) >> 32); }

/* How the two exact formulas of the header are computed in 32 bits:
 *   column pass   t = th * 2^12 + tl (tl = t & 4095): a = 2^12 Sh + Sl with Sh = sum C th, Sl = sum C tl, both below 2^28;
 *                 (a + 2^24) >> 25 == (Sh + (Sl >> 12) + 2^12) >> 13 -- the 12 low bits of Sl cannot carry across a multiple of 2^13;
 *   division      n / D for n = 2 |c8| + d <= 35217 and D = 2 d <= 5146 is (n * (floor(2^32 / D) + 1)) >> 32: the factor
 *                 exceeds 2^32 / D by less than 1, so the product exceeds n / D * 2^32 by less than n < 2^32 / D.
 * *nz: bit z set where zz[z * zs] was written (a level that is not 0); the other slots are left as they were. */
JM_HD int jm_enc_block_levels(const uint8_t *px, uint32_t stride, uint32_t q, const JmEncTables *T, int16_t *zz, uint32_t zs, uint64_t *nz) {
	constexpr JmEncConst K = jm_enc_make_const();
	/* row by row: the row's eight t values, then their share of all 64 sums (the sums stay in registers: every index into
	 * them is a constant once the u / v loops are unrolled; the row loop is a real loop) */
	int32_t sh[64], sl[64];
#pragma unroll
	for (int i = 0; i < 64; i++) { sh[i] = 0; sl[i] = 0; }
#pragma unroll 1
	for (int y = 0; y < 8; y++) {
		uint64_t row;
		memcpy(&row, __builtin_assume_aligned(px + (size_t)y * stride, 8), 8);
		int32_t cy[8];
#pragma unroll
		for (int u = 0; u < 8; u++) cy[u] = K.cos[u][y];
#pragma unroll
		for (int v = 0; v < 8; v++) {
			int32_t t = 0;
#pragma unroll
			for (int n = 0; n < 8; n++) t = jm_enc_mad24((int32_t)K.cos[v][n], (int32_t)((row >> (8 * n)) & 255u), t);
			const int32_t th = t >> 12, tl = t & 4095;
#pragma unroll
			for (int u = 0; u < 8; u++) {
				sh[u * 8 + v] = jm_enc_mad24(cy[u], th, sh[u * 8 + v]);
				sl[u * 8 + v] = jm_enc_mad24(cy[u], tl, sl[u * 8 + v]);
			}
		}
	}
	int dc = 0;
	uint64_t mask = 0;
	const uint32_t *recip = T->recip[q];
#pragma unroll
	for (int i = 0; i < 64; i++) {
		const int32_t c8 = (sh[i] + (sl[i] >> 12) + 4096) >> 13;
		if (i == 0) {
			const int l = (c8 + 32) >> 6;
			dc = l < 0 ? 0 : (l > 255 ? 255 : l);
		} else {
			const uint32_t d = q * (uint32_t)K.w[i];
			const uint32_t mag = jm_enc_mulhi(2u * (uint32_t)(c8 < 0 ? -c8 : c8) + d, recip[i]);
			if (mag) {
				const int m = (int)(mag > 255u ? 255u : mag);
				zz[(uint32_t)K.izz[i] * zs] = (int16_t)(c8 < 0 ? -m : m);
				mask |= 1ull << K.izz[i];
			}
		}
	}
	*nz = mask;
	return dc;
}

/* the run / level pairs of the levels nz marks (scan order) and end_of_block: their bits, written too when WRITE */
template <bool WRITE>
JM_HD uint32_t jm_enc_ac(const int16_t *zz, uint32_t zs, uint64_t nz, const JmEncTables *T, JmEncBits *bw) {
	uint32_t bits = 0, prev = 0;
	while (nz) {
		const uint32_t z = (uint32_t)__builtin_ctzll(nz);
		nz &= nz - 1;
		const uint32_t run = z - prev - 1u;
		prev = z;
		const int lv = zz[z * zs];
		const uint32_t mag = (uint32_t)(lv < 0 ? -lv : lv), sign = lv < 0 ? 1u : 0u;
		uint32_t e = (run < JM_ENC_MAX_RUN && mag < JM_ENC_MAX_LEVEL) ? T->coeff[run][mag] : 0u;
		if (run == 0 && mag == 1) e = (2u << 16) | 3u;                      /* "11" s: not the first coefficient of the block */
		uint32_t len, code;
		if (e) { len = (e >> 16) + 1u; code = ((e & 0xffffu) << 1) | sign; }
		else if (mag <= 127u) { len = 20u; code = (1u << 14) | (run << 8) | ((uint32_t)lv & 255u); }
		else { len = 28u; code = (1u << 22) | (run << 16) | (sign << 15) | ((uint32_t)lv & 255u); }
		bits += len;
		if (WRITE) jm_enc_put(*bw, code, len);
	}
	if (WRITE) jm_enc_put(*bw, 2u, 2u);
	return bits + 2u;
}

/* dct_dc_size + differential of level `dc` against `pred` */
template <bool WRITE>
JM_HD uint32_t jm_enc_dc(int dc, int pred, bool luma, const JmEncTables *T, JmEncBits *bw) {
	const int diff = dc - pred;
	const uint32_t mag = (uint32_t)(diff < 0 ? -diff : diff);
	const uint32_t size = mag ? 32u - (uint32_t)__builtin_clz(mag) : 0u;
	const uint32_t e = luma ? T->dc_luma[size] : T->dc_chroma[size];
	if (WRITE) {
		jm_enc_put(*bw, e & 255u, e >> 8);
		if (size) jm_enc_put(*bw, (uint32_t)(diff > 0 ? diff : diff + (1 << size) - 1), size);
	}
	return (e >> 8) + size;
}

/* ------------------------------------------------------------------ one macroblock
 * y, cr, cb: the macroblock's top-left sample in each plane; cw: coded width.  Blocks and dc[0 .. 5] in the order of the
 * syntax: Y0 Y1 Y2 Y3 Cb Cr (the frame store is Y | Cr | Cb: block 4 is the LAST plane, as in the reference, mpeg1.c:1571). */
JM_HD const uint8_t *jm_enc_block_px(const uint8_t *y, const uint8_t *cr, const uint8_t *cb, uint32_t cw, int b, uint32_t *stride) {
	*stride = b < 4 ? cw : cw >> 1;
	return b < 4 ? y + (size_t)(b >> 1) * 8u * cw + (size_t)(b & 1) * 8u : (b == 4 ? cb : cr);
}

/* bits of the macroblock WITHOUT its six DC codes (increment, type, the blocks' pairs and end_of_block); *dcs: the six DC
 * levels, block b's in byte b */
JM_HD uint32_t jm_enc_measure(const uint8_t *y, const uint8_t *cr, const uint8_t *cb, uint32_t cw, uint32_t q, const JmEncTables *T,
                              int16_t *zz, uint32_t zs, uint64_t *dcs) {
	uint32_t bits = 2;
	uint64_t d = 0;
#pragma unroll 1
	for (int b = 0; b < 6; b++) {
		uint32_t stride;
		const uint8_t *px = jm_enc_block_px(y, cr, cb, cw, b, &stride);
		uint64_t nz;
		d |= (uint64_t)(uint32_t)jm_enc_block_levels(px, stride, q, T, zz, zs, &nz) << (8 * b);
		bits += jm_enc_ac<false>(zz, zs, nz, T, nullptr);
	}
	*dcs = d;
	return bits;
}
/* what a macroblock's successor predicts from: (Y3, Cb, Cr) in bytes 0 .. 2; the slice's first macroblock predicts from JM_ENC_PRED0 */
#define JM_ENC_PRED0 0x808080u
JM_HD uint32_t jm_enc_pred_of(uint64_t dcs) { return (uint32_t)(dcs >> 24) & 0xffffffu; }
/* bits of the six DC codes, given the predecessor's levels */
JM_HD uint32_t jm_enc_dc_bits(uint64_t dcs, uint32_t pred, const JmEncTables *T) {
	const int d0 = (int)(dcs & 255u), d1 = (int)((dcs >> 8) & 255u), d2 = (int)((dcs >> 16) & 255u), d3 = (int)((dcs >> 24) & 255u);
	return jm_enc_dc<false>(d0, (int)(pred & 255u), true, T, nullptr) + jm_enc_dc<false>(d1, d0, true, T, nullptr) +
	       jm_enc_dc<false>(d2, d1, true, T, nullptr) + jm_enc_dc<false>(d3, d2, true, T, nullptr) +
	       jm_enc_dc<false>((int)((dcs >> 32) & 255u), (int)((pred >> 8) & 255u), false, T, nullptr) +
	       jm_enc_dc<false>((int)((dcs >> 40) & 255u), (int)((pred >> 16) & 255u), false, T, nullptr);
}
/* the macroblock's bits from bw's position on (bw is flushed by the caller) */
JM_HD void jm_enc_write(const uint8_t *y, const uint8_t *cr, const uint8_t *cb, uint32_t cw, uint32_t q, const JmEncTables *T,
                        int16_t *zz, uint32_t zs, uint32_t pred, JmEncBits &bw) {
	jm_enc_put(bw, 3u, 2u);                                     /* increment 1, type intra */
	int py = (int)(pred & 255u);
#pragma unroll 1
	for (int b = 0; b < 6; b++) {
		uint32_t stride;
		const uint8_t *px = jm_enc_block_px(y, cr, cb, cw, b, &stride);
		uint64_t nz;
		const int dc = jm_enc_block_levels(px, stride, q, T, zz, zs, &nz);
		jm_enc_dc<true>(dc, b < 4 ? py : (int)((pred >> (8 * (b - 3))) & 255u), b < 4, T, &bw);
		if (b < 4) py = dc;
		jm_enc_ac<true>(zz, zs, nz, T, &bw);
	}
}

/* ------------------------------------------------------------------ the scan
 * One macroblock's record between the passes: `bits` is jm_enc_measure's count, then -- after jm_enc_scan_slice -- the
 * macroblock's bit offset from the first byte of its slice. */
struct JmEncMb {
	uint32_t bits;
	uint32_t dc[2];      /* the six DC levels: Y0 Y1 Y2 Y3 | Cb Cr 0 0 */
};
JM_HD uint64_t jm_enc_mb_dcs(const JmEncMb &m) { return (uint64_t)m.dc[0] | ((uint64_t)m.dc[1] << 32); }
/* a slice of mbw macroblocks: bit offsets in place; returns the slice's bytes, padded to a whole byte */
JM_HD uint32_t jm_enc_scan_slice(JmEncMb *mb, uint32_t mbw, const JmEncTables *T) {
	uint32_t pred = JM_ENC_PRED0;
	uint32_t at = JM_ENC_SLICE_HEAD_BITS;
	for (uint32_t i = 0; i < mbw; i++) {
		const uint64_t dcs = jm_enc_mb_dcs(mb[i]);
		const uint32_t n = mb[i].bits + jm_enc_dc_bits(dcs, pred, T);
		mb[i].bits = at;
		at += n;
		pred = jm_enc_pred_of(dcs);
	}
	return (at + 7u) >> 3;
}
/* a picture's slices: each one's byte offset from the picture's sequence header (in place of its length); returns the picture's bytes */
JM_HD uint32_t jm_enc_scan_picture(uint32_t *slice_bytes, uint32_t mbh) {
	uint32_t at = JM_ENC_PIC_HEAD_BYTES;
	for (uint32_t r = 0; r < mbh; r++) { const uint32_t n = slice_bytes[r]; slice_bytes[r] = at; at += n; }
	return at;
}

/* The pictures of a call in order: streams ascend, each stream's pictures back to back from a 16-byte aligned begin, a
 * sequence end code behind the stream's last picture when `end`, and at least JM_STREAM_GAP bytes of 0xff up to the next
 * stream's begin (jsmpeg_hip_batch_attach_device refuses ranges that lie closer); the total is the last stream's end
 * rounded up to 16 (0xff from there on anyway).  One step per picture. */
struct JmEncPlace {
	uint64_t at;         /* next free byte */
	uint32_t stream;     /* of the previous picture, JM_NONE before the first */
};
JM_HD uint64_t jm_enc_align16(uint64_t v) { return (v + 15u) & ~(uint64_t)15u; }
JM_HD uint64_t jm_enc_next_begin(uint64_t stream_end) { return jm_enc_align16(stream_end + JM_STREAM_GAP); }
JM_HD JmEncPlace jm_enc_place_begin() { JmEncPlace p; p.at = JM_ENC_LEAD_GAP; p.stream = JM_NONE; return p; }
/* the current stream ends; `another` follows it (else: the call ends) */
JM_HD void jm_enc_place_end_stream(JmEncPlace &p, bool end, uint64_t *stream_end, bool another) {
	if (p.stream == JM_NONE) return;
	if (end) p.at += 4;
	stream_end[p.stream] = p.at;
	p.at = another ? jm_enc_next_begin(p.at) : jm_enc_align16(p.at);
}
JM_HD void jm_enc_place_close(JmEncPlace &p, bool end, uint64_t *stream_end) { jm_enc_place_end_stream(p, end, stream_end, false); }
/* returns the picture's byte offset */
JM_HD uint64_t jm_enc_place_picture(JmEncPlace &p, uint32_t stream, uint32_t bytes, bool end, uint64_t *stream_begin, uint64_t *stream_end) {
	if (stream != p.stream) {
		jm_enc_place_end_stream(p, end, stream_end, true);
		stream_begin[stream] = p.at;
		p.stream = stream;
	}
	const uint64_t off = p.at;
	p.at += bytes;
	return off;
}

/* ------------------------------------------------------------------ headers */
JM_HD uint32_t jm_enc_fps(uint32_t frame_rate_code) {          /* pictures per second of the time code */
	return frame_rate_code <= 2 ? 24u : (frame_rate_code == 3 ? 25u : (frame_rate_code <= 5 ? 30u : (frame_rate_code == 6 ? 50u : 60u)));
}
/* sequence header (no matrices), GOP header (closed, the time code of the picture's ordinal in its stream), picture header
 * (temporal reference 0, type I, vbv_delay 0xFFFF): 28 bytes at byte offset `at` */
JM_HD void jm_enc_put_picture_headers(uint32_t *words, uint64_t at, uint32_t width, uint32_t height, uint32_t frame_rate_code, uint32_t ordinal) {
	JmEncBits b = jm_enc_bits_at(words, at * 8u);
	jm_enc_put(b, 0x000001B3u, 32);
	jm_enc_put(b, width, 12); jm_enc_put(b, height, 12);
	jm_enc_put(b, 1, 4); jm_enc_put(b, frame_rate_code, 4);
	jm_enc_put(b, 0x3FFFFu, 18); jm_enc_put(b, 1, 1); jm_enc_put(b, 20, 10); jm_enc_put(b, 0, 3);
	const uint32_t fps = jm_enc_fps(frame_rate_code), s = ordinal / fps;
	jm_enc_put(b, 0x000001B8u, 32);
	jm_enc_put(b, 0, 1); jm_enc_put(b, (s / 3600u) % 24u, 5); jm_enc_put(b, (s / 60u) % 60u, 6); jm_enc_put(b, 1, 1);
	jm_enc_put(b, s % 60u, 6); jm_enc_put(b, ordinal % fps, 6); jm_enc_put(b, 1, 1); jm_enc_put(b, 0, 1 + 5);
	jm_enc_put(b, 0x00000100u, 32);
	jm_enc_put(b, 0, 10); jm_enc_put(b, 1, 3); jm_enc_put(b, 0xFFFFu, 16); jm_enc_put(b, 0, 1 + 2);
	jm_enc_flush(b);
}
JM_HD void jm_enc_put_slice_header(uint32_t *words, uint64_t at, uint32_t row, uint32_t q) {
	JmEncBits b = jm_enc_bits_at(words, at * 8u);
	jm_enc_put(b, 0x00000101u + row, 32);
	jm_enc_put(b, q, 5); jm_enc_put(b, 0, 1);
	jm_enc_flush(b);
}
/* behind a stream's last picture: the sequence end code when `end`, then 0xff up to where the next stream begins (behind the call's last stream
 * these bytes lie in the 0xff tail or are the total's rounding) */
JM_HD void jm_enc_put_stream_tail(uint32_t *words, uint64_t at, bool end) {
	JmEncBits b = jm_enc_bits_at(words, at * 8u);
	if (end) { jm_enc_put(b, 0x000001B7u, 32); at += 4; }
	for (uint64_t i = at; i < jm_enc_next_begin(at); i++) jm_enc_put(b, 0xffu, 8);
	jm_enc_flush(b);
}

/* ------------------------------------------------------------------ RGB in */
JM_HD uint32_t jm_enc_clamp255(int32_t v) { return (uint32_t)(v < 0 ? 0 : (v > 255 ? 255 : v)); }
JM_HD uint32_t jm_enc_luma(uint32_t r, uint32_t g, uint32_t b) { return (19595u * r + 38470u * g + 7471u * b + 32768u) >> 16; }
JM_HD uint32_t jm_enc_cr(int32_t rs, int32_t gs, int32_t bs) { return jm_enc_clamp255((32768 * rs - 27439 * gs - 5329 * bs + (128 << 18) + (1 << 17)) >> 18); }
JM_HD uint32_t jm_enc_cb(int32_t rs, int32_t gs, int32_t bs) { return jm_enc_clamp255((-11059 * rs - 21709 * gs + 32768 * bs + (128 << 18) + (1 << 17)) >> 18); }
/* One 2x2 of the coded picture, chroma sample (cx, cy): picture `pic` of display size w x h (layout 0: [3][h][w], 1: [h][w][3];
 * order 0: RGB, 1: BGR) -> four luma samples and one of each chroma in `frame` (Y | Cr | Cb of cw x ch) */
JM_HD void jm_enc_rgb_quad(const uint8_t *pic, uint32_t layout, uint32_t order, uint32_t w, uint32_t h, uint32_t cx, uint32_t cy,
                           uint8_t *frame, uint32_t cw, uint32_t ch) {
	int32_t sum[3] = { 0, 0, 0 };
	uint8_t *Y = frame, *Cr = frame + (size_t)cw * ch, *Cb = Cr + (size_t)(cw >> 1) * (ch >> 1);
#pragma unroll
	for (uint32_t j = 0; j < 4; j++) {
		const uint32_t x = 2 * cx + (j & 1), y = 2 * cy + (j >> 1);
		const uint32_t sx = x < w ? x : w - 1, sy = y < h ? y : h - 1;
		uint32_t c[3];
#pragma unroll
		for (uint32_t k = 0; k < 3; k++) {
			const uint32_t plane = order ? 2 - k : k;        /* where colour k (R, G, B) lies */
			c[k] = layout ? pic[((size_t)sy * w + sx) * 3 + plane] : pic[((size_t)plane * h + sy) * w + sx];
			sum[k] += (int32_t)c[k];
		}
		Y[(size_t)y * cw + x] = (uint8_t)jm_enc_luma(c[0], c[1], c[2]);
	}
	Cr[(size_t)cy * (cw >> 1) + cx] = (uint8_t)jm_enc_cr(sum[0], sum[1], sum[2]);
	Cb[(size_t)cy * (cw >> 1) + cx] = (uint8_t)jm_enc_cb(sum[0], sum[1], sum[2]);
}
