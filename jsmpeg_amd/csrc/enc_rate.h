/*
 * MPEG-1 ENCODER, RATE CONTROL (include/jsmpeg_hip.h part 8, jsmpeg_hip_encoder_set_rate): the quantiser scale of a picture
 * chosen on the device from a budget in bytes, stated once, host + device -- what the lane bodies of enc_pass.h, k_enc_rate_pick
 * of encode.hip and the CPU simulator's pick (tests/sim/sim_encode_pass.cpp) share.  tests/enc_rate_ref.py restates the rule in
 * numpy by brute force.
 * enc_motion.h's rules 1 .. 5 stand as they are: this one only says which scale they run at.
 *
 * RATE.  The handle carries T, the target bytes per picture (0: off), a range q_min <= q_max within 1 .. 31 and W, the weight of
 *    an I picture, 1 .. 255.  A GOP of a call is the m <= gop pictures of one stream from an ordinal that is a multiple of gop
 *    onwards (the last GOP of a stream in a call may be short; gop 1: every picture is a GOP of its own).  For the picture at
 *    level l (0-based) of its GOP, in unsigned 64-bit integers:
 *        G      = m * T
 *        spent  = sum of the FINAL bytes of the GOP's pictures at levels < l
 *        left   = G > spent ? G - spent : 0
 *        w, S   = (W, W + m - 1) if l == 0 else (1, m - l)
 *        budget = left * w / S                                  floor
 *        q      = the smallest q in [q_min, q_max] whose picture is at most `budget` bytes; q_max if none is
 *    "The picture's bytes at q" is exact: what jsmpeg_hip_encoder_picture_range reports for the picture coded at q with every
 *    earlier picture as chosen -- headers, per-slice padding, increments over skipped runs, vector differentials, DC codes and
 *    the STUFFING code included; the stream's end code and the gaps are not.  Sizes need not fall with q: every q of the range is
 *    measured, nothing is bisected.  Budgets do not carry from GOP to GOP; there is no VBV model and the
 *    headers (bit_rate, vbv_delay) stay as they are.
 *    ACROSS CALLS (JSMPEG_HIP_ENC_CHAIN; enc_chain.h): in a chained call m = gop for every picture -- a GOP is assumed to be
 *    completed by later calls, the call's last GOP is not cut short -- and `spent` is the final bytes of the GOP's earlier levels
 *    WHICHEVER CALL CODED THEM: a uint64 per stream on the device, written by the pick of the stream's last picture of a call
 *    (its spent + its bytes) and added by the pick of a picture whose GOP began in an earlier call; a level-0 picture ignores
 *    it.  An unchained call is as above: nothing carries from call to call.
 *
 * HOW.  The transform, the mode decision and the vectors do not depend on q, so per level, behind the motion search:
 *    jm_encr_measure   a macroblock: each block transformed ONCE, then quantised and counted at every q; per (macroblock, q) a
 *                      16-bit record: the kind the macroblock would have at q (bits 0 .. 1) | its local bits (2 .. 15; below
 *                      6 * 64 * 28 + 9 < 2^14).  An intra macroblock's DC levels (the same at every q) go to its JmEncPMb.
 *    jm_encr_scan      a (slice, q): enc_motion.h's walk (jm_encp_walk_slice) over those records and the search's vectors
 *    jm_encr_budget    and the choice, a picture: the rows' sum plus the header against the budget
 *    No reconstruction: the level's measure kernel runs afterwards, at the chosen q.
 */
#pragma once
#include "enc_motion.h"

#define JM_ENCR_MAX_Q 31u        /* records per macroblock the store has room for */

JM_HD uint16_t jm_encr_record(uint32_t kind, uint32_t bits) { return (uint16_t)(kind | (bits << 2)); }

JM_HD uint64_t jm_encr_budget(uint64_t T, uint32_t m, uint32_t l, uint32_t W, uint64_t spent) {
	const uint64_t G = (uint64_t)m * T, left = G > spent ? G - spent : 0;
	const uint64_t w = l == 0 ? W : 1u, S = l == 0 ? (uint64_t)W + m - 1u : (uint64_t)(m - l);
	return left * w / S;
}
JM_HD uint32_t jm_encr_saturate(uint64_t v) { return v > 0xffffffffull ? 0xffffffffu : (uint32_t)v; }
/* what a picture at level l of its GOP has in bytes before its slices: the headers */
JM_HD uint32_t jm_encr_head_bytes(uint32_t l) { return l ? JM_ENC_P_HEAD_BYTES : JM_ENC_PIC_HEAD_BYTES; }

/* block b of a macroblock at every q of [q_min, q_min + nq): acc[qi * as] += its pairs' bits | its pattern bit << 16 */
template <bool INTER>
JM_HD void jm_encr_block(const int32_t c8[64], int b, uint32_t q_min, uint32_t nq, const JmEncTables *T, int16_t *zz, uint32_t zs, uint32_t *acc, uint32_t as) {
#pragma unroll 1
	for (uint32_t qi = 0; qi < nq; qi++) {
		const uint32_t q = q_min + qi;
		if (INTER) {
			const uint64_t nz = jm_encp_quant_inter(c8, jm_encp_recip(q), zz, zs);
			if (nz) acc[qi * as] += jm_encp_ac<false>(zz, zs, nz, T, nullptr) | ((0x20u >> b) << 16);
		} else {
			uint64_t nz;
			jm_encp_quant_intra(c8, q, T, zz, zs, &nz);
			acc[qi * as] += jm_enc_ac<false>(zz, zs, nz, T, nullptr);
		}
	}
}

/* A macroblock of a picture of a GOP at every q of [q_min, q_min + nq): rec[qi] = jm_encr_record(kind, local bits) by the rules of
 * jm_encp_measure_inter / _intra.  found: what the search left (jm_encp_decide), 0 in an I picture.  Returns whether it is
 * intra; then *dcs are its DC levels.  zz, pp: as there; acc: nq words of the caller's at acc[qi * as]. */
JM_HD bool jm_encr_measure(JM_GLOBAL const uint8_t *frame, JM_GLOBAL const uint8_t *ref, uint32_t cw, uint32_t ch, uint32_t mbw, uint32_t col, uint32_t row,
                           uint32_t found, uint32_t q_min, uint32_t nq, const JmEncTables *T, const JmEncPTables *PT,
                           int16_t *zz, uint32_t zs, uint32_t *pp, uint32_t ps, uint32_t *acc, uint32_t as, uint16_t *rec, uint64_t *dcs) {
	for (uint32_t qi = 0; qi < nq; qi++) acc[qi * as] = 0;
	if (found & 1u) {
		const int mvh = jm_encp_mvh(found), mvv = jm_encp_mvv(found);
#pragma unroll 1
		for (int b = 0; b < 6; b++) {
			int32_t c8[64];
			jm_encp_inter_c8(frame, ref, jm_encp_plane(cw, ch, col, row, b), b, mvh, mvv, pp, ps, c8);
			jm_encr_block<true>(c8, b, q_min, nq, T, zz, zs, acc, as);
		}
		const bool kept = mvh != 0 || mvv != 0 || col == 0 || col + 1 == mbw;
		for (uint32_t qi = 0; qi < nq; qi++) {
			const uint32_t v = acc[qi * as], cbp = v >> 16;
			rec[qi] = cbp ? jm_encr_record(JM_ENCP_CODED, (v & 0xffffu) + (PT->cbp[cbp] >> 16)) : jm_encr_record(kept ? JM_ENCP_NOT_CODED : JM_ENCP_SKIPPED, 0);
		}
		return false;
	}
	uint64_t d = 0;
#pragma unroll 1
	for (int b = 0; b < 6; b++) {
		const JmEncPlane p = jm_encp_plane(cw, ch, col, row, b);
		int32_t c8[64];
		jm_encp_fdct<false>(frame + (p.off + (size_t)p.y0 * p.stride + (size_t)p.x0), p.stride, nullptr, 0, c8);
		const int l = (c8[0] + 32) >> 6;                       /* jm_encp_quant_intra's DC level */
		d |= (uint64_t)(uint32_t)(l < 0 ? 0 : (l > 255 ? 255 : l)) << (8 * b);
		jm_encr_block<false>(c8, b, q_min, nq, T, zz, zs, acc, as);
	}
	for (uint32_t qi = 0; qi < nq; qi++) rec[qi] = jm_encr_record(JM_ENCP_INTRA, acc[qi * as]);
	*dcs = d;
	return true;
}

/* a slice of mbw macroblocks at scale number qi: the records rec[i * JM_ENCR_MAX_Q + qi] of jm_encr_measure, the vectors the
 * search left in mb[i].info and an intra macroblock's DC levels in mb[i].dc; nothing is written.  Returns the slice's bytes. */
struct JmEncRRow {
	const uint16_t *rec;
	const JmEncPMb *mb;
	JM_HD uint32_t info(uint32_t i) const {
		const uint32_t kind = rec[(size_t)i * JM_ENCR_MAX_Q] & 3u;
		if (kind == JM_ENCP_INTRA) return jm_encp_info(JM_ENCP_INTRA, false, 0, 0, 0);
		if (kind == JM_ENCP_SKIPPED) return jm_encp_info(JM_ENCP_SKIPPED, false, 0, 0, 0);
		const uint32_t found = mb[i].info;
		const int mvh = jm_encp_mvh(found), mvv = jm_encp_mvv(found);
		return jm_encp_info(kind, kind == JM_ENCP_NOT_CODED || mvh != 0 || mvv != 0, 0, mvh, mvv);
	}
	JM_HD uint32_t bits(uint32_t i) const { return (uint32_t)rec[(size_t)i * JM_ENCR_MAX_Q] >> 2; }
	JM_HD uint64_t dcs(uint32_t i) const { return (uint64_t)mb[i].dc[0] | ((uint64_t)mb[i].dc[1] << 32); }
	JM_HD void count(uint32_t) {}
	JM_HD void skipped(uint32_t, uint32_t) {}
	JM_HD void placed(uint32_t, uint32_t, uint32_t, uint32_t) {}
};
JM_HD uint32_t jm_encr_scan(const uint16_t *rec, const JmEncPMb *mb, uint32_t qi, uint32_t mbw, bool p_picture, uint32_t r_size,
                            const JmEncTables *T, const JmEncPTables *PT) {
	JmEncRRow row = { rec + qi, mb };
	return jm_encp_walk_slice(row, mbw, p_picture, r_size, T, PT);
}
