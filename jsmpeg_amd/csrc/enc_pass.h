/*
 * MPEG-1 ENCODER, THE PASS (include/jsmpeg_hip.h part 8): what a LANE of each kernel of encode.hip does around the arithmetic
 * of enc_block.h, enc_motion.h, enc_rate.h and enc_chain.h, stated once, host + device.  The kernels of encode.hip are their
 * __shared__ declarations, their guards and one call of a body below; the CPU simulator (tests/sim/sim_encode_pass.cpp) fills
 * the same argument structs with host pointers and runs the same launches as loops over g.
 *
 *   jm_pass_lane      which picture, row and column lane g has, and where its macroblock lies in the picture's planes
 *   jm_pass_headers   which headers the lane of a macroblock puts in front of it: the slice header by column 0, the picture's
 *                     (I: sequence + GOP + picture, P: picture) by macroblock 0, with them the stream's tail behind the
 *                     stream's last picture and the lead gap in front of the call's first
 *   jm_pass_*         a body per kernel whose lanes work alone; zz (and pp, acc) are the lane's strided scratch, as in the
 *                     functions they are handed to
 * k_enc_motion, k_enc_rate_pick, k_enc_place, k_enc_clear, k_enc_rgb and k_enc_scale are wave- or workgroup-cooperative: they
 * stay in encode.hip, and the simulator restates them serially from the same enc_*.h functions.  So do k_enc_rate_measure and
 * k_enc_rate_scan, a call of jm_encr_measure / jm_encr_scan each: behind a body of this header the compiler scheduled them
 * differently, and a call of 64 I pictures under rate control measured 0.6 % slower (profiles/enc_pass_notes.md).
 */
#pragma once
#include "enc_block.h"
#include "enc_motion.h"
#include "enc_rate.h"
#include "enc_chain.h"

struct JmEncPic {
	const uint8_t *frame;    /* Y | Cr | Cb of the coded size */
	const uint8_t *ref;      /* a P picture's reference: the reconstruction of the picture before (enc_chain.h, WHERE); level loop only */
	uint8_t *recon;          /* where the picture is reconstructed; level loop only */
	uint32_t stream, ordinal, q;
	uint32_t last;           /* the last picture of its stream in this call */
	uint32_t m;              /* the pictures its GOP is budgeted for (rate control) */
	uint32_t before;         /* pictures of its GOP in front of it in this call (rate control) */
	uint32_t carry;          /* JM_ENCC_READ | JM_ENCC_WRITE | JM_ENCC_ODD (rate control across calls) */
};

struct JmEncArgs {
	uint32_t width, height, cw, ch, mbw, mbh, count, frame_rate_code, end;
	uint64_t cap;
	const JmEncPic *pics;
	const JmEncTables *tables;
	JmEncMb *mb;             /* [count][mbh][mbw] */
	uint32_t *slice;         /* [count][mbh]: bytes, then offset in the picture */
	uint64_t *result;        /* total | status | stream_begin[max_streams] | stream_end[max_streams] | pic_off[max_pictures] | pic_bytes (u32) */
	uint32_t max_streams, max_pictures;
	uint32_t *words;         /* the output */
};
JM_HD uint64_t *enc_stream_begin(const JmEncArgs &a) { return a.result + 2; }
JM_HD uint64_t *enc_stream_end(const JmEncArgs &a) { return a.result + 2 + a.max_streams; }
JM_HD uint64_t *enc_pic_off(const JmEncArgs &a) { return a.result + 2 + 2 * (size_t)a.max_streams; }
JM_HD uint32_t *enc_pic_bytes(const JmEncArgs &a) { return (uint32_t *)(a.result + 2 + 2 * (size_t)a.max_streams + a.max_pictures); }
JM_HD size_t enc_result_bytes(uint32_t max_streams, uint32_t max_pictures) {
	return 8 * (2 + 2 * (size_t)max_streams + max_pictures) + 4 * (size_t)max_pictures;
}

/* the level loop (gop > 1, or rate control) */
struct JmEncPArgs {
	JmEncPMb *pmb;               /* [count][mbh][mbw] */
	const JmEncPTables *ptables;
	const uint32_t *list;        /* the call's picture numbers, sorted by level (jm_encc_levels) */
	uint32_t *slice_kinds;       /* [count][mbh][4] */
	uint32_t *stats;             /* [count][4] */
	uint32_t gop, search, r_size;
};

/* rate control (enc_rate.h) */
struct JmEncRArgs {
	uint16_t *rec;               /* [count][mbh][mbw][JM_ENCR_MAX_Q]: jm_encr_record */
	uint32_t *slice;             /* [count][mbh][JM_ENCR_MAX_Q]: a slice's bytes at every scale */
	uint32_t *out;               /* [count][4]: q, budget (saturated), bytes, 0 */
	uint64_t *spent;             /* [2][max_streams]: the final bytes of a stream's unfinished GOP, from call to call (enc_chain.h, RATE); chained calls only */
	uint64_t T;
	uint32_t q_min, nq, W;
};

/* The macroblock of lane g: picture k and macroblock m = (row, col) of it.  LEVEL: the lanes run over the pictures
 * list[first ..] of a level; else over every picture of the call (list is not read). */
struct JmEncLane { uint32_t k, m, row, col; };
template <bool LEVEL>
JM_HD JmEncLane jm_pass_lane(const JmEncArgs &a, const uint32_t *list, uint32_t first, uint64_t g) {
	JmEncLane l;
	const uint32_t mbs = a.mbw * a.mbh;
	l.k = LEVEL ? list[first + (uint32_t)(g / mbs)] : (uint32_t)(g / mbs); l.m = (uint32_t)(g % mbs); l.row = l.m / a.mbw; l.col = l.m % a.mbw;
	return l;
}
/* where lane l's macroblock lies in the three planes of its picture's frame (the intra pass; the level loop's functions take
 * the frame and (col, row)) */
struct JmEncPlanes { const uint8_t *y, *cr, *cb; };
JM_HD JmEncPlanes jm_pass_planes(const JmEncArgs &a, const JmEncLane &l) {
	JmEncPlanes p;
	const uint8_t *f = a.pics[l.k].frame;
	const size_t luma = (size_t)a.cw * a.ch, coff = (size_t)l.row * 8u * (a.cw >> 1) + (size_t)l.col * 8u;
	p.y = f + (size_t)l.row * 16u * a.cw + (size_t)l.col * 16u;
	p.cr = f + luma + coff;
	p.cb = f + luma + (luma >> 2) + coff;
	return p;
}

/* What lane l puts in front of its macroblock.  level: the picture's ordinal mod gop, 0 for an I picture. */
JM_HD void jm_pass_headers(const JmEncArgs &a, const JmEncLane &l, const JmEncPic &pic, uint64_t pic_at, uint64_t slice_at, uint32_t level, uint32_t r_size) {
	if (l.col) return;
	jm_enc_put_slice_header(a.words, slice_at, l.row, pic.q);
	if (l.row) return;
	if (level) jm_encp_put_picture_header(a.words, pic_at, level, r_size);
	else jm_enc_put_picture_headers(a.words, pic_at, a.width, a.height, a.frame_rate_code, pic.ordinal);
	if (pic.last) jm_enc_put_stream_tail(a.words, pic_at + enc_pic_bytes(a)[l.k], a.end != 0);
	if (l.k == 0)
		for (uint32_t i = 0; i < JM_ENC_LEAD_GAP / 4; i++) jm_enc_or(a.words + i, 0xffffffffu);
}

/* ------------------------------------------------------------------ the intra pass (gop 1 without rate control) */

/* k_enc_measure: g < count * mbw * mbh */
JM_HD void jm_pass_measure(const JmEncArgs &a, uint64_t g, int16_t *zz, uint32_t zs) {
	const JmEncLane l = jm_pass_lane<false>(a, nullptr, 0, g);
	const JmEncPlanes f = jm_pass_planes(a, l);
	JmEncMb rec;
	uint64_t dcs;
	rec.bits = jm_enc_measure(f.y, f.cr, f.cb, a.cw, a.pics[l.k].q, a.tables, zz, zs, &dcs);
	rec.dc[0] = (uint32_t)dcs; rec.dc[1] = (uint32_t)(dcs >> 32);
	a.mb[g] = rec;
}

/* k_enc_scan_slices: s < count * mbh */
JM_HD void jm_pass_scan_slice(const JmEncArgs &a, uint32_t s) { a.slice[s] = jm_enc_scan_slice(a.mb + (size_t)s * a.mbw, a.mbw, a.tables); }

/* k_enc_scan_pictures: k < count */
JM_HD void jm_pass_scan_picture(const JmEncArgs &a, uint32_t k) { enc_pic_bytes(a)[k] = jm_enc_scan_picture(a.slice + (size_t)k * a.mbh, a.mbh); }

/* k_enc_write: g < count * mbw * mbh, the call did not overflow */
JM_HD void jm_pass_write(const JmEncArgs &a, uint64_t g, int16_t *zz, uint32_t zs) {
	const JmEncLane l = jm_pass_lane<false>(a, nullptr, 0, g);
	const JmEncPlanes f = jm_pass_planes(a, l);
	const JmEncPic pic = a.pics[l.k];
	const uint64_t pic_at = enc_pic_off(a)[l.k], slice_at = pic_at + a.slice[(size_t)l.k * a.mbh + l.row];
	jm_pass_headers(a, l, pic, pic_at, slice_at, 0, 0);
	const uint32_t pred = l.col ? jm_enc_pred_of(jm_enc_mb_dcs(a.mb[g - 1])) : JM_ENC_PRED0;
	JmEncBits bw = jm_enc_bits_at(a.words, slice_at * 8u + a.mb[g].bits);
	jm_enc_write(f.y, f.cr, f.cb, a.cw, pic.q, a.tables, zz, zs, pred, bw);
	jm_enc_flush(bw);
}

/* ------------------------------------------------------------------ the level loop */

/* k_enc_measure_p: g < n * mbw * mbh over the pictures list[first ..] of a level; the macroblock's record holds what the search
 * left (jm_encp_decide) and, with rate control, an intra macroblock's DC levels */
JM_HD void jm_pass_measure_p(const JmEncArgs &a, const JmEncPArgs &p, uint32_t first, uint64_t g, int16_t *zz, uint32_t zs, uint32_t *pp, uint32_t ps) {
	const JmEncLane l = jm_pass_lane<true>(a, p.list, first, g);
	const JmEncPic pic = a.pics[l.k];
	JmEncPMb *rec = p.pmb + ((size_t)l.k * a.mbw * a.mbh + l.m);
	JM_GLOBAL uint8_t *recon = (JM_GLOBAL uint8_t *)pic.recon;
	const uint32_t found = (pic.ordinal % p.gop) ? rec->info : 0u;
	JmEncPMb out;
	out.dc[0] = out.dc[1] = 0; out.inh = 0; out.pred = 0;
	if (found & 1u) {
		out.bits = jm_encp_measure_inter((JM_GLOBAL const uint8_t *)pic.frame, (JM_GLOBAL const uint8_t *)pic.ref, recon, a.cw, a.ch, a.mbw, l.col, l.row,
		                                 jm_encp_mvh(found), jm_encp_mvv(found), pic.q, a.tables, p.ptables, zz, zs, pp, ps, &out.info);
	} else {
		uint64_t dcs;
		out.bits = jm_encp_measure_intra((JM_GLOBAL const uint8_t *)pic.frame, recon, a.cw, a.ch, l.col, l.row, pic.q, a.tables, zz, zs, &dcs);
		out.dc[0] = (uint32_t)dcs; out.dc[1] = (uint32_t)(dcs >> 32);
		out.info = jm_encp_info(JM_ENCP_INTRA, false, 0, 0, 0);
	}
	*rec = out;
}

/* k_enc_scan_slices_p: s < count * mbh */
JM_HD void jm_pass_scan_slice_p(const JmEncArgs &a, const JmEncPArgs &p, uint32_t s) {
	uint32_t kinds[4] = { 0, 0, 0, 0 };
	a.slice[s] = jm_encp_scan_slice(p.pmb + (size_t)s * a.mbw, a.mbw, (a.pics[s / a.mbh].ordinal % p.gop) != 0, p.r_size, a.tables, p.ptables, kinds);
	for (int i = 0; i < 4; i++) p.slice_kinds[(size_t)s * 4 + i] = kinds[i];
}

/* k_enc_scan_pictures_p: k < count */
JM_HD void jm_pass_scan_picture_p(const JmEncArgs &a, const JmEncPArgs &p, uint32_t k) {
	enc_pic_bytes(a)[k] = jm_encp_scan_picture(a.slice + (size_t)k * a.mbh, a.mbh, jm_encr_head_bytes(a.pics[k].ordinal % p.gop));
	for (int i = 0; i < 4; i++) {
		uint32_t sum = 0;
		for (uint32_t r = 0; r < a.mbh; r++) sum += p.slice_kinds[((size_t)k * a.mbh + r) * 4 + i];
		p.stats[(size_t)k * 4 + i] = sum;
	}
}

/* k_enc_write_p: g < count * mbw * mbh, the call did not overflow */
JM_HD void jm_pass_write_p(const JmEncArgs &a, const JmEncPArgs &p, uint64_t g, int16_t *zz, uint32_t zs, uint32_t *pp, uint32_t ps) {
	const JmEncLane l = jm_pass_lane<false>(a, nullptr, 0, g);
	const JmEncPic pic = a.pics[l.k];
	const uint32_t level = pic.ordinal % p.gop;
	const uint64_t pic_at = enc_pic_off(a)[l.k], slice_at = pic_at + a.slice[(size_t)l.k * a.mbh + l.row];
	jm_pass_headers(a, l, pic, pic_at, slice_at, level, p.r_size);
	const JmEncPMb rec = p.pmb[g];
	JmEncBits bw = jm_enc_bits_at(a.words, slice_at * 8u + rec.bits);
	jm_encp_write(rec, (JM_GLOBAL const uint8_t *)pic.frame, (JM_GLOBAL const uint8_t *)pic.ref, a.cw, a.ch, l.col, l.row, level != 0, p.r_size, pic.q,
	              a.tables, p.ptables, zz, zs, pp, ps, bw);
	jm_enc_flush(bw);
}
