/*
 * MPEG-1 ENCODER, P PICTURES (include/jsmpeg_hip.h part 8, jsmpeg_hip_encoder_set_gop): the rules of the closed loop, stated
 * once, host + device -- what the lane bodies of enc_pass.h, k_enc_motion of encode.hip and the CPU simulator
 * (tests/sim/sim_encode_pass.cpp) share.
 * tests/enc_p_ref.py restates every rule below in numpy.  enc_block.h stays what the gop-1 pass compiles.
 *
 * 1. MOTION SEARCH, on luma, against the encoder's own reconstruction of the stream's previous picture.  Candidates: the
 *    full-pel vectors in [-R, R]^2 for which every luma and chroma pixel a decoder reads lies inside the coded picture
 *    (jm_encp_mv_ok; the chroma vector is the luma vector halved toward zero).  The winner is the minimum of the tuple
 *    (SAD, dx^2 + dy^2, dy, dx), packed into one integer (jm_encp_key): a total order, so any shape of reduction finds it.
 *    R > 0: the eight half-pel neighbours of the winner, where valid by the same rule and inside the f_code's range,
 *    predicted with the decoder's roundings (a + b + 1) >> 1 and (a + b + c + d + 2) >> 2; one replaces the full-pel winner
 *    only with a strictly smaller SAD, among several the order is (SAD, vertical half step, horizontal half step).
 *    forward_f_code is 1 for R <= 7 and 2 above: 2 R + 1 <= 15 resp. 31 half-pels always lies inside [-16 f, 16 f - 1].
 * 2. MODE: intra when activity + JM_ENC_INTRA_BIAS < best SAD, activity = sum |x - mean| over the 16 x 16 luma,
 *    mean = (sum x + 128) >> 8.
 * 3. RESIDUAL: source minus prediction, in -255 .. 255, through the forward DCT of enc_block.h.  Its bounds hold unchanged:
 *    they were taken over |x| <= 255 (tools/fdct_bounds.py --signed: |t| <= 255 * 46344 = 11 817 720 < 2^24, |a| < 2^39).
 *    Quantiser, default non-intra matrix (16 everywhere), truncating toward zero, for the reference's dequantiser:
 *        level = sign(c8) * min(255, |c8| / (16 q))          integer division, as (|c8| >> 4) / q
 *    Macroblock types in use: intra, MC + coded, no MC + coded (zero vector with a pattern), MC not coded.  Zero vector and
 *    empty pattern: skipped -- but the first and the last macroblock of a slice are written as "MC, not coded" with a zero vector.
 * 4. RECONSTRUCTION, what the reference decoder makes of the bits (mpeg1.c decode_block): dequantise + oddify + clip
 *    (jm_dequant of recon_block.h), premultiply, the reference's IDCT network (JM_IDCT_1D) or -- a block whose only coefficient
 *    is (0, 0), an intra block without AC levels -- the single-coefficient shortcut, add the prediction, clamp.  I pictures
 *    of a GOP go the same way: the first P predicts from them.
 * 5. BITS.  jm_encp_measure_* give what is local to a macroblock (pattern code and run / level pairs; an intra macroblock's
 *    pairs and DC levels); jm_encp_scan_slice walks a row and adds what depends on the predecessor -- the address increment
 *    over a skipped run (escapes above 33), the differential vector against the vector predictor (reset after intra, after
 *    "no MC" and after a skip), the DC codes against the DC predictors (reset after a non-intra or skipped macroblock) --
 *    and leaves every macroblock's inherited state in its record, so that jm_encp_write_* need no walk.
 *    STUFFING: the reference ends a slice when the next WHOLE bytes are a start code (buffer.c next_bytes_are_start_code), so it
 *    would never read a slice's last macroblock that begins inside a byte and ends in the same byte ("MC, not coded", increment
 *    1, zero differentials: 6 bits).  Such a macroblock gets one macroblock_stuffing code (11 bits) in front of its increment.
 */
#pragma once
#include "enc_block.h"
#include "recon_block.h"

/* 512: a predicted macroblock also pays for a vector and a pattern and inherits the reference's noise, an intra one pays a few hundred
 * bits of DC and low frequencies -- the test encoder's neighbourhood (tests/enc/mpeg1_enc.py: 500).  A content decision, not a measured optimum. */
#define JM_ENC_INTRA_BIAS 512u
#define JM_ENC_MAX_SEARCH 15u
#define JM_ENC_P_HEAD_BYTES 9u       /* picture header of a P picture: 32 + 10 + 3 + 16 + 1 + 3 + 1 bits, padded */

/* the search window of a macroblock in dwords: 48 rows x 52 bytes of the reference's luma from (16 col - 16, 16 row - 16), zero outside the picture */
#define JM_ENCP_WIN_DW 13u
#define JM_ENCP_WIN_ROWS 48u
#define JM_ENCP_WIN_WORDS (JM_ENCP_WIN_DW * JM_ENCP_WIN_ROWS)

enum { JM_ENCP_INTRA = 0, JM_ENCP_CODED = 1, JM_ENCP_NOT_CODED = 2, JM_ENCP_SKIPPED = 3 };

/* One macroblock between the passes (gop > 1).
 * info: kind (bits 0 .. 1) | vector transmitted (bit 2) | pattern (bits 3 .. 8, block b at 0x20 >> b) | mvh (16 .. 23) | mvv (24 .. 31), half-pels.
 *       After the motion kernel and before the measure kernel: bit 0 = predicted (not intra) and the vector.
 * bits: the local count, then -- after jm_encp_scan_slice -- the bit offset from the first byte of the slice.
 * inh : what the macroblock inherits along the slice: address increment (bits 0 .. 11) | stuffing in front (bit 12) | vector predictor h (16 .. 23) | v (24 .. 31)
 * pred: the DC predictors it inherits (jm_enc_pred_of's layout) */
struct JmEncPMb {
	uint32_t bits;
	uint32_t dc[2];
	uint32_t info, inh, pred;
};
JM_HD uint32_t jm_encp_info(uint32_t kind, bool mc, uint32_t cbp, int mvh, int mvv) {
	return kind | (mc ? 4u : 0u) | (cbp << 3) | (((uint32_t)mvh & 255u) << 16) | (((uint32_t)mvv & 255u) << 24);
}
JM_HD uint32_t jm_encp_kind(uint32_t info) { return info & 3u; }
JM_HD uint32_t jm_encp_cbp(uint32_t info) { return (info >> 3) & 63u; }
JM_HD int jm_encp_mvh(uint32_t info) { return (int)(int8_t)(info >> 16); }
JM_HD int jm_encp_mvv(uint32_t info) { return (int)(int8_t)(info >> 24); }

struct JmEncPTables {
	uint32_t mba[35];        /* [increment 1 .. 33]: (length << 16) | bits; [0]: macroblock_escape, [34]: macroblock_stuffing */
	uint32_t cbp[64];
	uint32_t motion[17];     /* [|code|]: the positive code, its sign bit (0) included */
};
constexpr JmEncPTables jm_encp_make_tables() {
	JmEncPTables t{};
#define X(bits, v) if ((v) == 35) t.mba[0] = jm_enc_code(bits); else t.mba[(v) <= 34 ? (v) : 0] = jm_enc_code(bits);
	MPEG1_VLC_MBA(X)
#undef X
#define X(bits, v) t.cbp[v] = jm_enc_code(bits);
	MPEG1_VLC_CBP(X)
#undef X
#define X(bits, v) if ((v) >= 0) t.motion[(v) >= 0 ? (v) : 0] = jm_enc_code(bits);
	MPEG1_VLC_MOTION(X)
#undef X
	return t;
}

JM_HD uint32_t jm_encp_r_size(uint32_t search) { return search <= 7u ? 0u : 1u; }     /* forward_f_code - 1 */

/* ------------------------------------------------------------------ 1. motion search */

JM_HD bool jm_encp_mv_ok(uint32_t cw, uint32_t ch, uint32_t col, uint32_t row, int mh, int mv) {
	const int H = mh >> 1, V = mv >> 1, oh = mh & 1, ov = mv & 1;
	const int x0 = (int)col * 16 + H, y0 = (int)row * 16 + V;
	if (x0 < 0 || y0 < 0 || x0 + 15 + oh > (int)cw - 1 || y0 + 15 + ov > (int)ch - 1) return false;
	const int c_h = mh / 2, c_v = mv / 2;                      /* toward zero, like the decoder */
	const int cx0 = (int)col * 8 + (c_h >> 1), cy0 = (int)row * 8 + (c_v >> 1);
	return !(cx0 < 0 || cy0 < 0 || cx0 + 7 + (c_h & 1) > (int)(cw >> 1) - 1 || cy0 + 7 + (c_v & 1) > (int)(ch >> 1) - 1);
}

/* (SAD, dx^2 + dy^2, dy, dx) as one integer: 16 + 9 + 5 + 5 bits */
JM_HD uint64_t jm_encp_key(uint32_t sad, int dx, int dy) {
	return ((uint64_t)sad << 19) | ((uint64_t)(uint32_t)(dx * dx + dy * dy) << 10) | ((uint64_t)(uint32_t)(dy + 16) << 5) | (uint64_t)(uint32_t)(dx + 16);
}
#define JM_ENCP_NO_KEY (~0ull)
JM_HD uint32_t jm_encp_key_sad(uint64_t key) { return (uint32_t)(key >> 19); }
JM_HD int jm_encp_key_dx(uint64_t key) { return (int)(key & 31u) - 16; }
JM_HD int jm_encp_key_dy(uint64_t key) { return (int)((key >> 5) & 31u) - 16; }

/* sum of the four absolute byte differences, plus acc */
JM_HD uint32_t jm_encp_sad4(uint32_t a, uint32_t b, uint32_t acc) {
#if defined(__HIP_DEVICE_COMPILE__)
	return __builtin_amdgcn_sad_u8(a, b, acc);
#else
	for (int i = 0; i < 32; i += 8) { const int d = (int)((a >> i) & 255u) - (int)((b >> i) & 255u); acc += (uint32_t)(d < 0 ? -d : d); }
	return acc;
#endif
}

/* dword i of the window of macroblock (col, row): four luma bytes of the reference, 0 where they leave the picture */
JM_HD uint32_t jm_encp_window_dword(JM_GLOBAL const uint8_t *ref, uint32_t cw, uint32_t ch, uint32_t col, uint32_t row, uint32_t i) {
	const int y = (int)row * 16 - 16 + (int)(i / JM_ENCP_WIN_DW), x = (int)col * 16 - 16 + 4 * (int)(i % JM_ENCP_WIN_DW);
	if (y < 0 || y >= (int)ch || x < 0 || x + 4 > (int)cw) return 0u;
	return *reinterpret_cast<JM_GLOBAL const uint32_t *>(ref + (size_t)y * cw + (size_t)x);
}

/* The items of a full-pel search: item = (dy, a group of four dx that share their reference dwords).  The byte offset of
 * dx in a window row is 16 + dx; group `gi` holds the offsets 4 gi .. 4 gi + 3, so the shifts are constants. */
struct JmEncSearch { uint32_t g0, ng, items; };
JM_HD JmEncSearch jm_encp_search_shape(uint32_t R) {
	JmEncSearch s;
	s.g0 = (16u - R) >> 2; s.ng = ((16u + R) >> 2) - s.g0 + 1u; s.items = (2u * R + 1u) * s.ng;
	return s;
}
/* the best key among the (up to) four candidates of item `it`; win, cur: the window and the macroblock's 64 dwords */
JM_HD uint64_t jm_encp_search_item(const uint32_t *win, const uint32_t *cur, uint32_t R, JmEncSearch s, uint32_t it,
                                   uint32_t cw, uint32_t ch, uint32_t col, uint32_t row) {
	const int dy = (int)(it / s.ng) - (int)R;
	const uint32_t gi = s.g0 + it % s.ng;
	const uint32_t *w = win + (uint32_t)(16 + dy) * JM_ENCP_WIN_DW + gi;
	uint32_t sad[4] = { 0, 0, 0, 0 };
#pragma unroll 4
	for (uint32_t r = 0; r < 16; r++, w += JM_ENCP_WIN_DW) {
		const uint32_t W[5] = { w[0], w[1], w[2], w[3], w[4] };
#pragma unroll
		for (uint32_t k = 0; k < 4; k++) {
			const uint32_t c = cur[r * 4 + k];
			sad[0] = jm_encp_sad4(W[k], c, sad[0]);
#pragma unroll
			for (uint32_t j = 1; j < 4; j++) sad[j] = jm_encp_sad4(jm_alignbyte(W[k + 1], W[k], j), c, sad[j]);
		}
	}
	uint64_t best = JM_ENCP_NO_KEY;
#pragma unroll
	for (uint32_t j = 0; j < 4; j++) {
		const int dx = (int)(gi * 4 + j) - 16;
		const bool ok = dx >= -(int)R && dx <= (int)R && jm_encp_mv_ok(cw, ch, col, row, 2 * dx, 2 * dy);
		const uint64_t key = ok ? jm_encp_key(sad[j], dx, dy) : JM_ENCP_NO_KEY;
		best = key < best ? key : best;
	}
	return best;
}

/* half-pel neighbour n = 0 .. 7 in the order (vertical half step, horizontal half step) */
JM_HD void jm_encp_half_step(uint32_t n, int *hh, int *hv) {
	const uint32_t i = n < 4 ? n : n + 1;
	*hv = (int)(i / 3) - 1; *hh = (int)(i % 3) - 1;
}
JM_HD bool jm_encp_half_ok(uint32_t cw, uint32_t ch, uint32_t col, uint32_t row, int mh, int mv, uint32_t r_size) {
	const int range = 16 << r_size;
	return mh >= -range && mh < range && mv >= -range && mv < range && jm_encp_mv_ok(cw, ch, col, row, mh, mv);
}
/* The SAD of luma rows 2 part, 2 part + 1 of the macroblock against the prediction a decoder forms for (mh, mv) half-pels --
 * recon_block.h's branch-free form: u = (A + B + 1) >> 1 per row, P = (u_r + u_r' + [A + B even in both rows]) >> 1 */
JM_HD uint32_t jm_encp_halfpel_part(const uint32_t *win, const uint32_t *cur, int mh, int mv, uint32_t part) {
	const uint32_t oh = (uint32_t)(mh & 1), ov = (uint32_t)(mv & 1);
	const uint32_t bx = (uint32_t)(16 + (mh >> 1)), m = bx & 3u;
	const uint32_t *w = win + (uint32_t)(16 + (mv >> 1) + 2 * (int)part) * JM_ENCP_WIN_DW + (bx >> 2);
	uint32_t u[3][4], e[3][4];
#pragma unroll
	for (uint32_t r = 0; r < 3; r++, w += JM_ENCP_WIN_DW) {
		uint32_t a[5];
#pragma unroll
		for (uint32_t k = 0; k < 4; k++) a[k] = jm_alignbyte(w[k + 1], w[k], m);
		a[4] = w[4] >> (8u * m);
#pragma unroll
		for (uint32_t k = 0; k < 4; k++) {
			const uint32_t b = jm_alignbyte(a[k + 1], a[k], oh);
			u[r][k] = jm_lerp(a[k], b, 0x01010101u);
			e[r][k] = ~(a[k] ^ b);
		}
	}
	uint32_t sad = 0;
#pragma unroll
	for (uint32_t r = 0; r < 2; r++)
#pragma unroll
		for (uint32_t k = 0; k < 4; k++)
			sad = jm_encp_sad4(jm_lerp(u[r][k], ov ? u[r + 1][k] : u[r][k], e[r][k] & e[r + 1][k]), cur[(2 * part + r) * 4 + k], sad);
	return sad;
}

/* what the search leaves in a macroblock's record: predicted (bit 0) and the vector */
JM_HD uint32_t jm_encp_decide(uint32_t sad, uint32_t activity, int mvh, int mvv) {
	const bool intra = activity + JM_ENC_INTRA_BIAS < sad;
	return intra ? 0u : (1u | (((uint32_t)mvh & 255u) << 16) | (((uint32_t)mvv & 255u) << 24));
}

/* ------------------------------------------------------------------ 3. residual -> levels */

/* the 8 x 8 prediction of a decoder: block at (x0, y0) of `plane` (stride x ph), vector (mh, mv) half-pels of that plane, valid by
 * jm_encp_mv_ok; rows as packed bytes in P[16].  Reads 12 bytes per row from a dword boundary: up to 4 bytes behind the
 * plane's last row (the reconstruction store has that slack). */
JM_HD void jm_encp_predict8(JM_GLOBAL const uint8_t *plane, uint32_t stride, uint32_t ph, int x0, int y0, int mh, int mv, uint32_t P[16]) {
	JmBlk B;
	B.pred = true;
	B.oh = (uint32_t)(mh & 1); B.ov = (uint32_t)(mv & 1);
	const int sx = x0 + (mh >> 1), sy = y0 + (mv >> 1);
	const uint32_t off = (uint32_t)sy * stride + (uint32_t)sx;
	B.m = off & 3u;
	const uint32_t last = (sy + 8 < (int)ph) ? 8u : 7u;        /* row 8 is only used when ov == 1 (then it is inside) */
#pragma unroll
	for (uint32_t r = 0; r < 9; r++) {
		JM_GLOBAL const uint32_t *wr = reinterpret_cast<JM_GLOBAL const uint32_t *>(plane + ((off & ~3u) + (r < 8 ? r : last) * stride));
		B.R[3 * r] = wr[0]; B.R[3 * r + 1] = wr[1]; B.R[3 * r + 2] = wr[2];
	}
	jm_recon_predict(B);
#pragma unroll
	for (int i = 0; i < 16; i++) P[i] = B.P[i];
}

/* enc_block.h's forward DCT (the same two formulas, the same 32-bit arithmetic) of the block's pixels minus the prediction
 * rows pp[(2 y) * ps], pp[(2 y + 1) * ps] (SUB; else of the pixels as they are, what jm_enc_block_levels transforms): c8[64],
 * raster.  The pixels come through a JM_GLOBAL pointer: frames are addresses out of JmEncPic (mpeg1_dev.h says why that matters). */
template <bool SUB>
JM_HD void jm_encp_fdct(JM_GLOBAL const uint8_t *px, uint32_t stride, const uint32_t *pp, uint32_t ps, int32_t c8[64]) {
	constexpr JmEncConst K = jm_enc_make_const();
	int32_t sh[64], sl[64];
#pragma unroll
	for (int i = 0; i < 64; i++) { sh[i] = 0; sl[i] = 0; }
#pragma unroll 1
	for (int y = 0; y < 8; y++) {
		const uint64_t row = *reinterpret_cast<JM_GLOBAL const uint64_t *>(px + (size_t)y * stride);
		const uint64_t prow = SUB ? (uint64_t)pp[(uint32_t)(2 * y) * ps] | ((uint64_t)pp[(uint32_t)(2 * y + 1) * ps] << 32) : 0ull;
		int32_t cy[8];
#pragma unroll
		for (int u = 0; u < 8; u++) cy[u] = K.cos[u][y];
#pragma unroll
		for (int v = 0; v < 8; v++) {
			int32_t t = 0;
#pragma unroll
			for (int n = 0; n < 8; n++)
				t = jm_enc_mad24((int32_t)K.cos[v][n], (int32_t)((row >> (8 * n)) & 255u) - (int32_t)((prow >> (8 * n)) & 255u), t);
			const int32_t th = t >> 12, tl = t & 4095;
#pragma unroll
			for (int u = 0; u < 8; u++) {
				sh[u * 8 + v] = jm_enc_mad24(cy[u], th, sh[u * 8 + v]);
				sl[u * 8 + v] = jm_enc_mad24(cy[u], tl, sl[u * 8 + v]);
			}
		}
	}
#pragma unroll
	for (int i = 0; i < 64; i++) c8[i] = (sh[i] + (sl[i] >> 12) + 4096) >> 13;
}

/* n / q for n < 2^31 / q: mulhi(2 n, floor(2^31 / q) + 1) -- the factor exceeds 2^31 / q by at most 1, so the quotient's
 * excess 2 n / 2^32 stays below 1 / q */
JM_HD uint32_t jm_encp_recip(uint32_t q) { return 0x80000000u / q + 1u; }

/* non-intra levels in scan order at zz[z * zs], z = 0 .. 63; returns the mask of the levels that are not 0 */
JM_HD uint64_t jm_encp_quant_inter(const int32_t c8[64], uint32_t rq, int16_t *zz, uint32_t zs) {
	constexpr JmEncConst K = jm_enc_make_const();
	uint64_t mask = 0;
#pragma unroll
	for (int i = 0; i < 64; i++) {
		const uint32_t mag = jm_enc_mulhi(2u * ((uint32_t)(c8[i] < 0 ? -c8[i] : c8[i]) >> 4), rq);
		if (mag) {
			const int m = (int)(mag > 255u ? 255u : mag);
			zz[(uint32_t)K.izz[i] * zs] = (int16_t)(c8[i] < 0 ? -m : m);
			mask |= 1ull << K.izz[i];
		}
	}
	return mask;
}

/* jm_enc_block_levels' quantiser (the same two formulas, the same reciprocal table) on c8: the DC level (returned) and the AC
 * levels in scan order at zz[z * zs], z = 1 .. 63, *nz their mask */
JM_HD int jm_encp_quant_intra(const int32_t c8[64], uint32_t q, const JmEncTables *T, int16_t *zz, uint32_t zs, uint64_t *nz) {
	constexpr JmEncConst K = jm_enc_make_const();
	const uint32_t *recip = T->recip[q];
	uint64_t mask = 0;
#pragma unroll
	for (int i = 1; i < 64; i++) {
		const uint32_t d = q * (uint32_t)K.w[i];
		const uint32_t mag = jm_enc_mulhi(2u * (uint32_t)(c8[i] < 0 ? -c8[i] : c8[i]) + d, recip[i]);
		if (mag) {
			const int m = (int)(mag > 255u ? 255u : mag);
			zz[(uint32_t)K.izz[i] * zs] = (int16_t)(c8[i] < 0 ? -m : m);
			mask |= 1ull << K.izz[i];
		}
	}
	*nz = mask;
	const int l = (c8[0] + 32) >> 6;
	return l < 0 ? 0 : (l > 255 ? 255 : l);
}
JM_HD int jm_encp_intra_block(JM_GLOBAL const uint8_t *px, uint32_t stride, uint32_t q, const JmEncTables *T, int16_t *zz, uint32_t zs, uint64_t *nz) {
	int32_t c8[64];
	jm_encp_fdct<false>(px, stride, nullptr, 0, c8);
	return jm_encp_quant_intra(c8, q, T, zz, zs, nz);
}

/* a non-intra block's run / level pairs from scan position 0 on ("1s" for a first coefficient (0, +-1)) and end_of_block */
template <bool WRITE>
JM_HD uint32_t jm_encp_ac(const int16_t *zz, uint32_t zs, uint64_t nz, const JmEncTables *T, JmEncBits *bw) {
	uint32_t bits = 0, prev = 0xffffffffu;
	while (nz) {
		const uint32_t z = (uint32_t)__builtin_ctzll(nz);
		nz &= nz - 1;
		const uint32_t run = z - prev - 1u;
		const bool first = prev == 0xffffffffu;
		prev = z;
		const int lv = zz[z * zs];
		const uint32_t mag = (uint32_t)(lv < 0 ? -lv : lv), sign = lv < 0 ? 1u : 0u;
		uint32_t e = (run < JM_ENC_MAX_RUN && mag < JM_ENC_MAX_LEVEL) ? T->coeff[run][mag] : 0u;
		if (run == 0 && mag == 1) e = first ? ((1u << 16) | 1u) : ((2u << 16) | 3u);
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

/* ------------------------------------------------------------------ 4. reconstruction */

/* What the reference decoder makes of a block's levels: INTRA: dc and the AC levels nz marks (scan 1 .. 63), the pixels
 * are the clamped transform; else the levels nz marks (scan 0 .. 63), added to the prediction rows at pp.  8 rows to out. */
template <bool INTRA>
JM_HD void jm_encp_recon_block(const int16_t *zz, uint32_t zs, uint64_t nz, int dc, uint32_t q, const uint32_t *pp, uint32_t ps,
                               JM_GLOBAL uint8_t *out, uint32_t stride) {
	constexpr JmEncConst K = jm_enc_make_const();
	int v[64];
	if (INTRA ? nz == 0 : nz <= 1) {
		/* nothing, or only the (0, 0) coefficient: every pixel gets (coefficient + 128) >> 8 (mpeg1.c:1578-1581) */
		int k = 0;
		if (INTRA) k = dc;
		else if (nz) k = (jm_mul24(jm_dequant((int)zz[0], false, (int)q * 16), JM_PREMULT[0]) + 128) >> 8;
#pragma unroll
		for (int i = 0; i < 64; i++) v[i] = k;
	} else {
#pragma unroll
		for (int i = 0; i < 64; i++) {
			const uint32_t z = K.izz[i];
			const int lv = ((nz >> z) & 1u) ? (int)zz[z * zs] : 0;
			const int d = jm_mul24(jm_dequant(lv, INTRA, (int)q * (INTRA ? (int)K.w[i] : 16)), JM_PREMULT[i]);
			v[i] = lv ? d : 0;
		}
		if (INTRA) v[0] = dc << 8;
		const int c128 = 128;
#pragma unroll
		for (int c = 0; c < 8; c++)
			JM_IDCT_1D(v[c], v[8 + c], v[16 + c], v[24 + c], v[32 + c], v[40 + c], v[48 + c], v[56 + c], 0, JM_FIN_NONE)
#pragma unroll
		for (int r = 0; r < 8; r++)
			JM_IDCT_1D(v[8 * r], v[8 * r + 1], v[8 * r + 2], v[8 * r + 3], v[8 * r + 4], v[8 * r + 5], v[8 * r + 6], v[8 * r + 7], 128, JM_FIN_SHIFT)
	}
#pragma unroll
	for (int r = 0; r < 8; r++) {
		uint32_t o[2];
#pragma unroll
		for (int h = 0; h < 2; h++) {
			const uint32_t p = INTRA ? 0u : pp[(uint32_t)(2 * r + h) * ps];
			o[h] = 0;
#pragma unroll
			for (int n = 0; n < 4; n++) o[h] |= (uint32_t)jm_clamp255((int)((p >> (8 * n)) & 255u) + v[8 * r + 4 * h + n]) << (8 * n);
		}
		JM_GLOBAL uint32_t *w = reinterpret_cast<JM_GLOBAL uint32_t *>(out + (size_t)r * stride);
		w[0] = o[0]; w[1] = o[1];
	}
}

/* ------------------------------------------------------------------ one macroblock
 * A frame's planes; block b (syntax order Y0 Y1 Y2 Y3 Cb Cr) of macroblock (col, row): plane pointer, stride, rows, position */
struct JmEncPlane { uint32_t off, stride, ph; int x0, y0; };
JM_HD JmEncPlane jm_encp_plane(uint32_t cw, uint32_t ch, uint32_t col, uint32_t row, int b) {
	JmEncPlane p;
	const uint32_t luma = cw * ch;
	if (b < 4) { p.off = 0; p.stride = cw; p.ph = ch; p.x0 = (int)col * 16 + (b & 1) * 8; p.y0 = (int)row * 16 + (b >> 1) * 8; }
	else { p.off = luma + (b == 4 ? luma >> 2 : 0u); p.stride = cw >> 1; p.ph = ch >> 1; p.x0 = (int)col * 8; p.y0 = (int)row * 8; }
	return p;
}

/* an intra macroblock of a GOP: jm_enc_measure's bits (without increment and type) and DC levels, and its reconstruction */
JM_HD uint32_t jm_encp_measure_intra(JM_GLOBAL const uint8_t *frame, JM_GLOBAL uint8_t *recon, uint32_t cw, uint32_t ch, uint32_t col, uint32_t row,
                                     uint32_t q, const JmEncTables *T, int16_t *zz, uint32_t zs, uint64_t *dcs) {
	uint32_t bits = 0;
	uint64_t d = 0;
#pragma unroll 1
	for (int b = 0; b < 6; b++) {
		const JmEncPlane p = jm_encp_plane(cw, ch, col, row, b);
		const size_t at = p.off + (size_t)p.y0 * p.stride + (size_t)p.x0;
		uint64_t nz;
		const int dc = jm_encp_intra_block(frame + at, p.stride, q, T, zz, zs, &nz);
		d |= (uint64_t)(uint32_t)dc << (8 * b);
		bits += jm_enc_ac<false>(zz, zs, nz, T, nullptr);
		jm_encp_recon_block<true>(zz, zs, nz, dc, q, nullptr, 0, recon + at, p.stride);
	}
	*dcs = d;
	return bits;
}
/* its blocks' bits from bw's position on: jm_enc_write without the increment and the type */
JM_HD void jm_encp_write_intra(JM_GLOBAL const uint8_t *frame, uint32_t cw, uint32_t ch, uint32_t col, uint32_t row, uint32_t q, const JmEncTables *T,
                               int16_t *zz, uint32_t zs, uint32_t pred, JmEncBits &bw) {
	int py = (int)(pred & 255u);
#pragma unroll 1
	for (int b = 0; b < 6; b++) {
		const JmEncPlane p = jm_encp_plane(cw, ch, col, row, b);
		uint64_t nz;
		const int dc = jm_encp_intra_block(frame + (p.off + (size_t)p.y0 * p.stride + (size_t)p.x0), p.stride, q, T, zz, zs, &nz);
		jm_enc_dc<true>(dc, b < 4 ? py : (int)((pred >> (8 * (b - 3))) & 255u), b < 4, T, &bw);
		if (b < 4) py = dc;
		jm_enc_ac<true>(zz, zs, nz, T, &bw);
	}
}

/* block b of a predicted macroblock: prediction into pp, the transformed residual into c8 */
JM_HD void jm_encp_inter_c8(JM_GLOBAL const uint8_t *frame, JM_GLOBAL const uint8_t *ref, const JmEncPlane &p, int b, int mvh, int mvv,
                            uint32_t *pp, uint32_t ps, int32_t c8[64]) {
	uint32_t P[16];
	jm_encp_predict8(ref + p.off, p.stride, p.ph, p.x0, p.y0, b < 4 ? mvh : mvh / 2, b < 4 ? mvv : mvv / 2, P);
#pragma unroll
	for (uint32_t i = 0; i < 16; i++) pp[i * ps] = P[i];
	jm_encp_fdct<true>(frame + (p.off + (size_t)p.y0 * p.stride + (size_t)p.x0), p.stride, pp, ps, c8);
}
/* ... and its levels into zz; returns their mask */
JM_HD uint64_t jm_encp_inter_block(JM_GLOBAL const uint8_t *frame, JM_GLOBAL const uint8_t *ref, const JmEncPlane &p, int b, int mvh, int mvv,
                                   uint32_t rq, int16_t *zz, uint32_t zs, uint32_t *pp, uint32_t ps) {
	int32_t c8[64];
	jm_encp_inter_c8(frame, ref, p, b, mvh, mvv, pp, ps, c8);
	return jm_encp_quant_inter(c8, rq, zz, zs);
}

/* a predicted macroblock with vector (mvh, mvv) against `ref` (the reconstruction of the picture before): its reconstruction,
 * its local bits (the pattern's code and the blocks' pairs), *info: kind, pattern, vector */
JM_HD uint32_t jm_encp_measure_inter(JM_GLOBAL const uint8_t *frame, JM_GLOBAL const uint8_t *ref, JM_GLOBAL uint8_t *recon, uint32_t cw, uint32_t ch,
                                     uint32_t mbw, uint32_t col, uint32_t row, int mvh, int mvv, uint32_t q, const JmEncTables *T, const JmEncPTables *PT,
                                     int16_t *zz, uint32_t zs, uint32_t *pp, uint32_t ps, uint32_t *info) {
	uint32_t bits = 0, cbp = 0;
	const uint32_t rq = jm_encp_recip(q);
#pragma unroll 1
	for (int b = 0; b < 6; b++) {
		const JmEncPlane p = jm_encp_plane(cw, ch, col, row, b);
		const uint64_t nz = jm_encp_inter_block(frame, ref, p, b, mvh, mvv, rq, zz, zs, pp, ps);
		if (nz) { cbp |= 0x20u >> b; bits += jm_encp_ac<false>(zz, zs, nz, T, nullptr); }
		jm_encp_recon_block<false>(zz, zs, nz, 0, q, pp, ps, recon + (p.off + (size_t)p.y0 * p.stride + (size_t)p.x0), p.stride);
	}
	const bool moved = mvh != 0 || mvv != 0;
	if (cbp) { *info = jm_encp_info(JM_ENCP_CODED, moved, cbp, mvh, mvv); bits += PT->cbp[cbp] >> 16; }
	else if (moved || col == 0 || col + 1 == mbw) *info = jm_encp_info(JM_ENCP_NOT_CODED, true, 0, mvh, mvv);
	else *info = jm_encp_info(JM_ENCP_SKIPPED, false, 0, 0, 0);
	return bits;
}

/* ------------------------------------------------------------------ 5. the neighbour-dependent codes */

JM_HD int jm_encp_wrap(int d, uint32_t r_size) {
	const int range = 16 << r_size;
	return d < -range ? d + 2 * range : (d >= range ? d - 2 * range : d);
}
template <bool WRITE>
JM_HD uint32_t jm_encp_motion(int d, uint32_t r_size, const JmEncPTables *PT, JmEncBits *bw) {
	if (d == 0) { if (WRITE) jm_enc_put(*bw, PT->motion[0] & 0xffffu, PT->motion[0] >> 16); return PT->motion[0] >> 16; }
	const uint32_t ad = (uint32_t)(d < 0 ? -d : d) - 1u, e = PT->motion[(ad >> r_size) + 1u];
	if (WRITE) {
		jm_enc_put(*bw, (e & 0xffffu) | (d < 0 ? 1u : 0u), e >> 16);
		if (r_size) jm_enc_put(*bw, ad & ((1u << r_size) - 1u), r_size);
	}
	return (e >> 16) + r_size;
}
template <bool WRITE>
JM_HD uint32_t jm_encp_mba(uint32_t inc, const JmEncPTables *PT, JmEncBits *bw) {
	uint32_t bits = 0;
	while (inc > 33u) { if (WRITE) jm_enc_put(*bw, PT->mba[0] & 0xffffu, PT->mba[0] >> 16); bits += PT->mba[0] >> 16; inc -= 33u; }
	if (WRITE) jm_enc_put(*bw, PT->mba[inc] & 0xffffu, PT->mba[inc] >> 16);
	return bits + (PT->mba[inc] >> 16);
}
/* macroblock_type: (length << 16) | bits */
JM_HD uint32_t jm_encp_type(uint32_t info, bool p_picture) {
	const uint32_t kind = jm_encp_kind(info);
	if (kind == JM_ENCP_INTRA) return p_picture ? ((5u << 16) | 3u) : ((1u << 16) | 1u);
	if (kind == JM_ENCP_CODED) return (info & 4u) ? ((1u << 16) | 1u) : ((2u << 16) | 1u);
	return (3u << 16) | 1u;
}

/* THE WALK along a slice of mbw macroblocks, whatever holds them.  `mb` gives macroblock i's info(i) (kind, vector transmitted,
 * vector), its local bits(i) and -- intra -- its DC levels dcs(i), and takes what the walk finds: count(kind), skipped(i, at),
 * placed(i, at, inh, pred) with `at` the bit offset from the first byte of the slice.  Returns the slice's bytes. */
template <class Row>
JM_HD uint32_t jm_encp_walk_slice(Row &mb, uint32_t mbw, bool p_picture, uint32_t r_size, const JmEncTables *T, const JmEncPTables *PT) {
	uint32_t pred = JM_ENC_PRED0, at = JM_ENC_SLICE_HEAD_BITS;
	int pmh = 0, pmv = 0, last = -1;
	for (uint32_t i = 0; i < mbw; i++) {
		const uint32_t info = mb.info(i), kind = jm_encp_kind(info);
		mb.count(kind);
		if (kind == JM_ENCP_SKIPPED) {
			mb.skipped(i, at);
			pred = JM_ENC_PRED0; pmh = pmv = 0;
			continue;
		}
		const uint32_t inc = (uint32_t)((int)i - last);
		last = (int)i;
		uint32_t n = jm_encp_mba<false>(inc, PT, nullptr) + (jm_encp_type(info, p_picture) >> 16) + mb.bits(i);
		uint32_t inh = inc | (((uint32_t)pmh & 255u) << 16) | (((uint32_t)pmv & 255u) << 24);
		const uint32_t inherited = pred;
		if (kind == JM_ENCP_INTRA) {
			const uint64_t dcs = mb.dcs(i);
			n += jm_enc_dc_bits(dcs, pred, T);
			pred = jm_enc_pred_of(dcs);
			pmh = pmv = 0;
		} else {
			pred = JM_ENC_PRED0;
			if (info & 4u) {
				const int mvh = jm_encp_mvh(info), mvv = jm_encp_mvv(info);
				n += jm_encp_motion<false>(jm_encp_wrap(mvh - pmh, r_size), r_size, PT, nullptr) + jm_encp_motion<false>(jm_encp_wrap(mvv - pmv, r_size), r_size, PT, nullptr);
				pmh = mvh; pmv = mvv;
			} else pmh = pmv = 0;
		}
		if (i + 1 == mbw && (at & 7u) && (at & 7u) + n <= 8u) { inh |= 1u << 12; n += PT->mba[34] >> 16; }     /* STUFFING, above */
		mb.placed(i, at, inh, inherited);
		at += n;
	}
	return (at + 7u) >> 3;
}

/* a slice of mbw macroblocks of a picture of a GOP: bit offsets and inherited state in place, the slice's kinds added to
 * kinds[4]; returns the slice's bytes */
struct JmEncPRow {
	JmEncPMb *mb;
	uint32_t *kinds;
	JM_HD uint32_t info(uint32_t i) const { return mb[i].info; }
	JM_HD uint32_t bits(uint32_t i) const { return mb[i].bits; }
	JM_HD uint64_t dcs(uint32_t i) const { return (uint64_t)mb[i].dc[0] | ((uint64_t)mb[i].dc[1] << 32); }
	JM_HD void count(uint32_t kind) { kinds[kind]++; }
	JM_HD void skipped(uint32_t i, uint32_t at) { mb[i].bits = at; mb[i].inh = 0; mb[i].pred = JM_ENC_PRED0; }
	JM_HD void placed(uint32_t i, uint32_t at, uint32_t inh, uint32_t pred) { mb[i].bits = at; mb[i].inh = inh; mb[i].pred = pred; }
};
JM_HD uint32_t jm_encp_scan_slice(JmEncPMb *mb, uint32_t mbw, bool p_picture, uint32_t r_size, const JmEncTables *T, const JmEncPTables *PT, uint32_t kinds[4]) {
	JmEncPRow row = { mb, kinds };
	return jm_encp_walk_slice(row, mbw, p_picture, r_size, T, PT);
}
JM_HD uint32_t jm_encp_scan_picture(uint32_t *slice_bytes, uint32_t mbh, uint32_t head_bytes) {
	uint32_t at = head_bytes;
	for (uint32_t r = 0; r < mbh; r++) { const uint32_t n = slice_bytes[r]; slice_bytes[r] = at; at += n; }
	return at;
}

/* a macroblock of a picture of a GOP from bw's position on (nothing for a skipped one): increment, type, then the vector and
 * the pattern and the coded blocks, or the intra blocks */
JM_HD void jm_encp_write(const JmEncPMb &rec, JM_GLOBAL const uint8_t *frame, JM_GLOBAL const uint8_t *ref, uint32_t cw, uint32_t ch, uint32_t col, uint32_t row,
                         bool p_picture, uint32_t r_size, uint32_t q, const JmEncTables *T, const JmEncPTables *PT,
                         int16_t *zz, uint32_t zs, uint32_t *pp, uint32_t ps, JmEncBits &bw) {
	const uint32_t info = rec.info, kind = jm_encp_kind(info);
	if (kind == JM_ENCP_SKIPPED) return;
	if (rec.inh & (1u << 12)) jm_enc_put(bw, PT->mba[34] & 0xffffu, PT->mba[34] >> 16);
	jm_encp_mba<true>(rec.inh & 0xfffu, PT, &bw);
	const uint32_t type = jm_encp_type(info, p_picture);
	jm_enc_put(bw, type & 0xffffu, type >> 16);
	if (kind == JM_ENCP_INTRA) { jm_encp_write_intra(frame, cw, ch, col, row, q, T, zz, zs, rec.pred, bw); return; }
	const int mvh = jm_encp_mvh(info), mvv = jm_encp_mvv(info);
	if (info & 4u) {
		jm_encp_motion<true>(jm_encp_wrap(mvh - (int)(int8_t)(rec.inh >> 16), r_size), r_size, PT, &bw);
		jm_encp_motion<true>(jm_encp_wrap(mvv - (int)(int8_t)(rec.inh >> 24), r_size), r_size, PT, &bw);
	}
	const uint32_t cbp = jm_encp_cbp(info);
	if (!cbp) return;
	jm_enc_put(bw, PT->cbp[cbp] & 0xffffu, PT->cbp[cbp] >> 16);
	const uint32_t rq = jm_encp_recip(q);
#pragma unroll 1
	for (int b = 0; b < 6; b++) {
		if (!(cbp & (0x20u >> b))) continue;
		const JmEncPlane p = jm_encp_plane(cw, ch, col, row, b);
		const uint64_t nz = jm_encp_inter_block(frame, ref, p, b, mvh, mvv, rq, zz, zs, pp, ps);
		jm_encp_ac<true>(zz, zs, nz, T, &bw);
	}
}

/* the picture header of a P picture (full_pel_forward_vector 0): 9 bytes at byte offset `at` */
JM_HD void jm_encp_put_picture_header(uint32_t *words, uint64_t at, uint32_t temporal, uint32_t r_size) {
	JmEncBits b = jm_enc_bits_at(words, at * 8u);
	jm_enc_put(b, 0x00000100u, 32);
	jm_enc_put(b, temporal & 1023u, 10); jm_enc_put(b, 2, 3); jm_enc_put(b, 0xFFFFu, 16);
	jm_enc_put(b, 0, 1); jm_enc_put(b, r_size + 1u, 3); jm_enc_put(b, 0, 1 + 6);
	jm_enc_flush(b);
}
