/* TEST-ONLY simulator of the encoder's pass (jsmpeg_amd/csrc/encode.hip): enc_pass.h's lane bodies -- what the kernels
 * themselves call -- compiled by g++ and driven launch by launch in the order of enc_run and enc_run_gop, every launch a loop
 * over g, with JmEncArgs / JmEncPArgs / JmEncRArgs that hold host pointers.  The kernels without a lane body are restated
 * serially from the same enc_*.h functions: k_enc_rgb (sim_enc_rgb), k_enc_motion (sim_motion: item by item, half-pel part by
 * part, as its lanes take them), k_enc_rate_measure and k_enc_rate_scan (sim_rate_measure, sim_rate_scan: the kernels' own
 * statements), k_enc_rate_pick (sim_rate_pick), k_enc_place and k_enc_clear.  The entry points:
 *   sim_encode          the intra pass (gop 1 without rate control)
 *   sim_encode_p        the level loop with a GOP
 *   sim_encode_rate     the level loop with rate control
 *     these three derive a call's plan plainly -- ordinals counted from stream[], a P picture's reference in the frame before
 *     its own, a short last GOP's m -- and NOT through enc_chain.h: they are the yardstick tests/test_enc_chain_sim.py holds
 *     chained calls against, what an unchained call always did
 *   sim_chain_*         a handle with the host's chain records, the carry frames and the GOPs' spent bytes, called again and
 *                       again, chained or not: the plan, the level lists and the addresses are enc_chain.h's, as in enc_run
 * so that the tests hold the streams against the reference decoder and the numpy restatements without a GPU, and the GPU
 * tests hold the device to the same calls. */
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "enc_pass.h"

static const JmEncTables g_tables = jm_enc_make_tables();
static const JmEncPTables g_ptables = jm_encp_make_tables();

extern "C" const uint32_t *sim_enc_coeff_table() { return &g_tables.coeff[0][0]; }
extern "C" const uint16_t *sim_enc_dc_table(int chroma) { return chroma ? g_tables.dc_chroma : g_tables.dc_luma; }

/* k_enc_rgb: count RGB pictures of w x h -> frames of the coded size */
extern "C" void sim_enc_rgb(const uint8_t *rgb, uint32_t layout, uint32_t order, uint32_t w, uint32_t h, uint32_t count, uint8_t *frames) {
	const uint32_t cw = (w + 15u) & ~15u, ch = (h + 15u) & ~15u;
	for (uint32_t k = 0; k < count; k++)
		for (uint32_t cy = 0; cy < ch / 2; cy++)
			for (uint32_t cx = 0; cx < cw / 2; cx++)
				jm_enc_rgb_quad(rgb + (size_t)k * w * h * 3, layout, order, w, h, cx, cy, frames + (size_t)k * cw * ch * 3 / 2, cw, ch);
}

/* jm_encp_quant_inter's division on its own: out[i] = mulhi(2 n[i], jm_encp_recip(q)), which stands in for n[i] / q */
extern "C" void sim_encp_recip_div(const uint32_t *n, uint32_t count, uint32_t q, uint32_t *out) {
	const uint32_t rq = jm_encp_recip(q);
	for (uint32_t i = 0; i < count; i++) out[i] = jm_enc_mulhi(2u * n[i], rq);
}

/* ------------------------------------------------------------------ a pass: the stores of a handle, the arguments of its launches */

struct Pass {
	JmEncArgs a;
	JmEncPArgs p;
	JmEncRArgs r;
	uint32_t mbs;
	size_t fb;
	std::vector<JmEncPic> pics;
	std::vector<JmEncMb> mb;
	std::vector<JmEncPMb> pmb;
	std::vector<uint32_t> slice, list, begin, kinds, rslice, rout;
	std::vector<uint64_t> result;
	std::vector<uint16_t> rec;
	int16_t zz[64];
	uint32_t pp[16], acc[JM_ENCR_MAX_Q];

	/* what enc_run puts into JmEncArgs; the pictures: frame, stream and q here, the plan's part by the caller */
	Pass(const uint8_t *frames, uint32_t w, uint32_t h, uint32_t count, const uint32_t *stream, const uint8_t *q, uint32_t frame_rate_code, bool end,
	     uint32_t max_streams, uint8_t *out, uint64_t cap) {
		a.width = w; a.height = h; a.mbw = (w + 15u) >> 4; a.mbh = (h + 15u) >> 4; a.cw = a.mbw * 16; a.ch = a.mbh * 16;
		a.count = count; a.frame_rate_code = frame_rate_code; a.end = end ? 1u : 0u; a.cap = cap;
		a.max_streams = max_streams; a.max_pictures = std::max(count, 1u);
		mbs = a.mbw * a.mbh; fb = (size_t)a.cw * a.ch * 3 / 2;
		pics.assign(count, JmEncPic());
		for (uint32_t k = 0; k < count; k++) { pics[k].frame = frames + k * fb; pics[k].stream = stream ? stream[k] : 0; pics[k].q = q ? q[k] : 0; }
		slice.assign((size_t)count * a.mbh, 0);
		result.assign(enc_result_bytes(a.max_streams, a.max_pictures) / 8 + 1, 0);
		a.pics = pics.data(); a.tables = &g_tables; a.mb = nullptr; a.slice = slice.data(); a.result = result.data();
		a.words = reinterpret_cast<uint32_t *>(out);
	}

	/* the plain plan of an unchained call: ordinal, last, and -- recon: the call's store -- a picture's reconstruction in its own
	 * frame, a P picture's reference in the frame before */
	void plain_plan(uint32_t gop, uint8_t *recon) {
		for (uint32_t k = 0; k < a.count; k++) {
			JmEncPic &c = pics[k];
			c.ordinal = (k && pics[k - 1].stream == c.stream) ? pics[k - 1].ordinal + 1 : 0;
			c.last = (k + 1 == a.count || pics[k + 1].stream != c.stream) ? 1u : 0u;
			if (!recon) continue;
			c.recon = recon + k * fb;
			c.ref = c.ordinal % gop ? c.recon - fb : c.recon;
		}
	}

	/* the stores and arguments of the level loop; list and begin: the caller's (levels()) */
	void level_stores(uint32_t gop, uint32_t R, uint32_t *stats) {
		pmb.assign((size_t)a.count * mbs, JmEncPMb());
		kinds.assign((size_t)a.count * a.mbh * 4, 0);
		list.assign(a.count, 0);
		begin.assign(gop + 1, 0);
		p.pmb = pmb.data(); p.ptables = &g_ptables; p.list = list.data(); p.slice_kinds = kinds.data(); p.stats = stats;
		p.gop = gop; p.search = R; p.r_size = jm_encp_r_size(R);
	}
	void rate_stores(uint64_t T, uint32_t q_min, uint32_t q_max, uint32_t W, uint64_t *spent) {
		rec.assign((size_t)a.count * mbs * JM_ENCR_MAX_Q, 0xffffu);         /* what the range does not cover is never read */
		rslice.assign((size_t)a.count * a.mbh * JM_ENCR_MAX_Q, 0);
		rout.assign((size_t)a.count * 4, 0);
		r.rec = rec.data(); r.slice = rslice.data(); r.out = rout.data(); r.spent = spent;
		r.T = T; r.q_min = q_min; r.nq = q_max - q_min + 1u; r.W = W;
	}
};

/* k_enc_motion for one macroblock */
static uint32_t sim_motion(const uint8_t *cur, const uint8_t *ref, uint32_t cw, uint32_t ch, uint32_t col, uint32_t row, uint32_t R) {
	uint32_t win[JM_ENCP_WIN_WORDS], mb[64];
	for (uint32_t i = 0; i < JM_ENCP_WIN_WORDS; i++) win[i] = 0xdeadbeefu;         /* rows the kernel does not stage are never read */
	for (uint32_t i = (15u - R) * JM_ENCP_WIN_DW; i < (33u + R) * JM_ENCP_WIN_DW; i++) win[i] = jm_encp_window_dword(ref, cw, ch, col, row, i);
	for (uint32_t l = 0; l < 64; l++) memcpy(&mb[l], cur + ((size_t)row * 16 + (l >> 2)) * cw + (size_t)col * 16 + (l & 3u) * 4u, 4);
	const JmEncSearch shape = jm_encp_search_shape(R);
	uint64_t best = JM_ENCP_NO_KEY;
	for (uint32_t it = 0; it < shape.items; it++) best = std::min(best, jm_encp_search_item(win, mb, R, shape, it, cw, ch, col, row));
	uint32_t sad = jm_encp_key_sad(best);
	int mvh = 2 * jm_encp_key_dx(best), mvv = 2 * jm_encp_key_dy(best);
	if (R) {
		uint64_t hk = JM_ENCP_NO_KEY;
		for (uint32_t n = 0; n < 8; n++) {
			int hh, hv;
			jm_encp_half_step(n, &hh, &hv);
			if (!jm_encp_half_ok(cw, ch, col, row, mvh + hh, mvv + hv, jm_encp_r_size(R))) continue;
			uint32_t s = 0;
			for (uint32_t part = 0; part < 8; part++) s += jm_encp_halfpel_part(win, mb, mvh + hh, mvv + hv, part);
			hk = std::min(hk, ((uint64_t)s << 3) | n);
		}
		if (hk != JM_ENCP_NO_KEY && (uint32_t)(hk >> 3) < sad) {
			int hh, hv;
			jm_encp_half_step((uint32_t)(hk & 7u), &hh, &hv);
			sad = (uint32_t)(hk >> 3); mvh += hh; mvv += hv;
		}
	}
	uint32_t sum = 0, activity = 0;
	for (uint32_t l = 0; l < 64; l++) sum = jm_encp_sad4(mb[l], 0u, sum);
	const uint32_t mean = (sum + 128u) >> 8;
	for (uint32_t l = 0; l < 64; l++) activity = jm_encp_sad4(mb[l], mean * 0x01010101u, activity);
	return jm_encp_decide(sad, activity, mvh, mvv);
}

/* k_enc_rate_measure for lane g < n * mbw * mbh, as the kernel has it; acc: JM_ENCR_MAX_Q words at acc[qi * as] */
static void sim_rate_measure(const JmEncArgs &a, const JmEncPArgs &p, const JmEncRArgs &r, uint32_t first, uint64_t g,
                                int16_t *zz, uint32_t zs, uint32_t *pp, uint32_t ps, uint32_t *acc, uint32_t as) {
	const JmEncLane l = jm_pass_lane<true>(a, p.list, first, g);
	const JmEncPic pic = a.pics[l.k];
	const size_t at = (size_t)l.k * a.mbw * a.mbh + l.m;
	JmEncPMb *rec = p.pmb + at;
	JM_GLOBAL const uint8_t *ref = (JM_GLOBAL const uint8_t *)pic.ref;    /* only read in a P picture */
	const uint32_t found = (pic.ordinal % p.gop) ? rec->info : 0u;
	uint64_t dcs;
	if (jm_encr_measure((JM_GLOBAL const uint8_t *)pic.frame, ref, a.cw, a.ch, a.mbw, l.col, l.row, found, r.q_min, r.nq, a.tables, p.ptables,
	                    zz, zs, pp, ps, acc, as, r.rec + at * JM_ENCR_MAX_Q, &dcs)) {
		rec->dc[0] = (uint32_t)dcs; rec->dc[1] = (uint32_t)(dcs >> 32);
	}
}

/* k_enc_rate_scan for lane g < n * mbh * nq, a (picture, slice, scale) each, as the kernel has it */
static void sim_rate_scan(const JmEncArgs &a, const JmEncPArgs &p, const JmEncRArgs &r, uint32_t first, uint64_t g) {
	const uint32_t qi = (uint32_t)(g % r.nq), row = (uint32_t)((g / r.nq) % a.mbh), k = p.list[first + (uint32_t)(g / ((uint64_t)r.nq * a.mbh))];
	const size_t s = (size_t)k * a.mbh + row;
	r.slice[s * JM_ENCR_MAX_Q + qi] = jm_encr_scan(r.rec + s * a.mbw * JM_ENCR_MAX_Q, p.pmb + s * a.mbw, qi, a.mbw, (a.pics[k].ordinal % p.gop) != 0, p.r_size, a.tables, p.ptables);
}

/* k_enc_rate_pick for picture k; budget[k]: the budget before it is saturated */
static void sim_rate_pick(Pass &P, uint32_t k, uint64_t *budget) {
	const JmEncArgs &a = P.a;
	const JmEncRArgs &r = P.r;
	JmEncPic &pic = P.pics[k];
	const uint32_t level = pic.ordinal % P.p.gop;
	uint64_t spent = 0;
	for (uint32_t j = 1; j <= pic.before; j++) spent += r.out[(size_t)(k - j) * 4 + 2];
	const uint32_t odd = jm_encc_spent_row(pic.carry);
	if (pic.carry & JM_ENCC_READ) spent += r.spent[(size_t)odd * a.max_streams + pic.stream];
	budget[k] = jm_encr_budget(r.T, pic.m, level, r.W, spent);
	uint32_t fit = r.nq - 1u, taken = 0;
	for (uint32_t qi = r.nq; qi-- > 0;) {
		uint32_t bytes = jm_encr_head_bytes(level);
		for (uint32_t row = 0; row < a.mbh; row++) bytes += r.slice[((size_t)k * a.mbh + row) * JM_ENCR_MAX_Q + qi];
		if (bytes <= budget[k] || qi == r.nq - 1u) { fit = qi; taken = bytes; }
	}
	pic.q = r.q_min + fit;
	r.out[(size_t)k * 4] = r.q_min + fit; r.out[(size_t)k * 4 + 1] = jm_encr_saturate(budget[k]); r.out[(size_t)k * 4 + 2] = taken; r.out[(size_t)k * 4 + 3] = 0;
	if (pic.carry & JM_ENCC_WRITE) r.spent[(size_t)(odd ^ 1u) * a.max_streams + pic.stream] = spent + taken;
}

/* enc_run's launches without a GOP: k_enc_measure, k_enc_scan_slices, k_enc_scan_pictures */
static void run_intra(Pass &P) {
	P.mb.assign((size_t)P.a.count * P.mbs, JmEncMb());
	P.a.mb = P.mb.data();
	for (uint64_t g = 0; g < (uint64_t)P.a.count * P.mbs; g++) jm_pass_measure(P.a, g, P.zz, 1);
	for (uint32_t s = 0; s < P.a.count * P.a.mbh; s++) jm_pass_scan_slice(P.a, s);
	for (uint32_t k = 0; k < P.a.count; k++) jm_pass_scan_picture(P.a, k);
}

/* enc_run_gop's launches up to the scans: per level k_enc_motion, with rate control k_enc_rate_measure, k_enc_rate_scan and
 * k_enc_rate_pick (budget: count, out), k_enc_measure_p; then k_enc_scan_slices_p, k_enc_scan_pictures_p.  P.list and P.begin
 * hold the `levels` levels. */
static void run_levels(Pass &P, uint32_t levels, bool rate, uint64_t *budget) {
	const JmEncArgs &a = P.a;
	for (uint32_t l = 0; l < levels; l++) {
		const uint32_t first = P.begin[l], n = P.begin[l + 1] - P.begin[l];
		if (!n) continue;
		if (l)
			for (uint64_t g = 0; g < (uint64_t)n * P.mbs; g++) {
				const JmEncLane ln = jm_pass_lane<true>(a, P.p.list, first, g);
				P.pmb[(size_t)ln.k * P.mbs + ln.m].info = sim_motion(a.pics[ln.k].frame, a.pics[ln.k].ref, a.cw, a.ch, ln.col, ln.row, P.p.search);
			}
		if (rate) {
			for (uint64_t g = 0; g < (uint64_t)n * P.mbs; g++) sim_rate_measure(a, P.p, P.r, first, g, P.zz, 1, P.pp, 1, P.acc, 1);
			for (uint64_t g = 0; g < (uint64_t)n * a.mbh * P.r.nq; g++) sim_rate_scan(a, P.p, P.r, first, g);
			for (uint32_t i = 0; i < n; i++) sim_rate_pick(P, P.list[first + i], budget);
		}
		for (uint64_t g = 0; g < (uint64_t)n * P.mbs; g++) jm_pass_measure_p(a, P.p, first, g, P.zz, 1, P.pp, 1);
	}
	for (uint32_t s = 0; s < a.count * a.mbh; s++) jm_pass_scan_slice_p(a, P.p, s);
	for (uint32_t k = 0; k < a.count; k++) jm_pass_scan_picture_p(a, P.p, k);
}

/* the rest of either pass: k_enc_place, k_enc_clear, k_enc_write or k_enc_write_p (gop != 0); the ranges out.  Returns the
 * total, or -1 when it exceeds the cap (nothing is written then) */
static int64_t run_place_and_write(Pass &P, bool gop, uint64_t *pic_off, uint32_t *pic_bytes, uint64_t *stream_begin, uint64_t *stream_end) {
	const JmEncArgs &a = P.a;
	uint64_t *sb = enc_stream_begin(a), *se = enc_stream_end(a);
	JmEncPlace place = jm_enc_place_begin();
	for (uint32_t k = 0; k < a.count; k++) enc_pic_off(a)[k] = jm_enc_place_picture(place, a.pics[k].stream, enc_pic_bytes(a)[k], a.end != 0, sb, se);
	jm_enc_place_close(place, a.end != 0, se);
	a.result[0] = place.at; a.result[1] = place.at > a.cap ? 1u : 0u;
	for (uint32_t k = 0; k < a.count; k++) { pic_off[k] = enc_pic_off(a)[k]; pic_bytes[k] = enc_pic_bytes(a)[k]; }
	for (uint32_t s = 0; s < a.max_streams; s++) { stream_begin[s] = sb[s]; stream_end[s] = se[s]; }
	if (a.result[1]) return -1;
	memset(a.words, 0, place.at);
	memset(reinterpret_cast<uint8_t *>(a.words) + place.at, 0xff, JM_ENC_TAIL);
	for (uint64_t g = 0; g < (uint64_t)a.count * P.mbs; g++) {
		if (gop) jm_pass_write_p(a, P.p, g, P.zz, 1, P.pp, 1);
		else jm_pass_write(a, g, P.zz, 1);
	}
	return (int64_t)place.at;
}

/* ------------------------------------------------------------------ unchained calls, the plan derived plainly */

/* the quantised levels of one frame: levels[mb][block][64] in scan order, [0] the DC level */
extern "C" void sim_enc_levels(const uint8_t *frame, uint32_t w, uint32_t h, uint32_t q, int16_t *levels) {
	const uint8_t q8 = (uint8_t)q;
	Pass P(frame, w, h, 1, nullptr, &q8, 5, true, 1, nullptr, 0);
	for (uint32_t m = 0; m < P.mbs; m++) {
		const JmEncPlanes l = jm_pass_planes(P.a, jm_pass_lane<false>(P.a, nullptr, 0, m));
		for (int b = 0; b < 6; b++) {
			uint32_t stride;
			const uint8_t *px = jm_enc_block_px(l.y, l.cr, l.cb, P.a.cw, b, &stride);
			int16_t *zz = levels + ((size_t)m * 6 + b) * 64;
			uint64_t nz;
			memset(zz, 0, 64 * sizeof(int16_t));
			zz[0] = (int16_t)jm_enc_block_levels(px, stride, q, &g_tables, zz, 1, &nz);
			for (int z = 1; z < 64; z++)
				if (!((nz >> z) & 1) != !zz[z]) zz[0] = -1;     /* the mask must name exactly the levels that are not 0 */
		}
	}
}

/* One call of the encoder: frames[k] = frames + k * frame_bytes.  Returns the total bytes (the 0xff tail behind them is written
 * too: out holds cap + 256 bytes), or -1 when the total exceeds cap (nothing is written then). */
extern "C" int64_t sim_encode(const uint8_t *frames, uint32_t w, uint32_t h, uint32_t count, const uint32_t *stream, const uint8_t *q,
                              uint32_t frame_rate_code, uint32_t end, uint32_t max_streams, uint8_t *out, uint64_t cap,
                              uint64_t *pic_off, uint32_t *pic_bytes, uint64_t *stream_begin, uint64_t *stream_end) {
	Pass P(frames, w, h, count, stream, q, frame_rate_code, end != 0, max_streams, out, cap);
	P.plain_plan(1, nullptr);
	run_intra(P);
	return run_place_and_write(P, false, pic_off, pic_bytes, stream_begin, stream_end);
}

/* the level lists of an unchained call from its ordinals */
static uint32_t plain_levels(Pass &P, uint32_t gop) {
	uint32_t levels = 0, at = 0;
	for (const JmEncPic &c : P.pics) levels = std::max(levels, c.ordinal % gop + 1);
	for (uint32_t l = 0; l < levels; l++) {
		P.begin[l] = at;
		for (uint32_t k = 0; k < P.a.count; k++)
			if (P.pics[k].ordinal % gop == l) P.list[at++] = k;
	}
	P.begin[levels] = at;
	return levels;
}

/* One call of the encoder with gop > 1: sim_encode's arguments, then gop and search_range; recon: count frames out (16 bytes
 * of slack behind them), info: count * macroblocks records' info words out, stats: count * 4.  Returns the total bytes or -1. */
extern "C" int64_t sim_encode_p(const uint8_t *frames, uint32_t w, uint32_t h, uint32_t count, const uint32_t *stream, const uint8_t *q,
                                uint32_t frame_rate_code, uint32_t end, uint32_t max_streams, uint32_t gop, uint32_t R, uint8_t *out, uint64_t cap,
                                uint64_t *pic_off, uint32_t *pic_bytes, uint64_t *stream_begin, uint64_t *stream_end,
                                uint8_t *recon, uint32_t *info, uint32_t *stats) {
	Pass P(frames, w, h, count, stream, q, frame_rate_code, end != 0, max_streams, out, cap);
	P.plain_plan(gop, recon);
	P.level_stores(gop, R, stats);
	run_levels(P, plain_levels(P, gop), false, nullptr);
	for (size_t i = 0; i < P.pmb.size(); i++) info[i] = P.pmb[i].info;
	return run_place_and_write(P, true, pic_off, pic_bytes, stream_begin, stream_end);
}

/* sim_encode_p's arguments with the rule's four values (T > 0) in place of the scales; chosen, budget, bytes: count each, out */
extern "C" int64_t sim_encode_rate(const uint8_t *frames, uint32_t w, uint32_t h, uint32_t count, const uint32_t *stream,
                                   uint32_t frame_rate_code, uint32_t end, uint32_t max_streams, uint32_t gop, uint32_t R,
                                   uint32_t T, uint32_t q_min, uint32_t q_max, uint32_t W, uint8_t *out, uint64_t cap,
                                   uint64_t *pic_off, uint32_t *pic_bytes, uint64_t *stream_begin, uint64_t *stream_end,
                                   uint8_t *recon, uint32_t *info, uint32_t *stats, uint8_t *chosen, uint64_t *budget, uint32_t *bytes) {
	Pass P(frames, w, h, count, stream, nullptr, frame_rate_code, end != 0, max_streams, out, cap);
	P.plain_plan(gop, recon);
	for (uint32_t k = count, len = 0; k-- > 0;) {                  /* a GOP is the pictures of its stream in the call: the last one may be short */
		JmEncPic &c = P.pics[k];
		if (c.last) len = c.ordinal + 1;
		c.m = std::min(gop, len - (c.ordinal - c.ordinal % gop));
		c.before = c.ordinal % gop;
	}
	P.level_stores(gop, R, stats);
	P.rate_stores(T, q_min, q_max, W, nullptr);
	run_levels(P, plain_levels(P, gop), true, budget);
	for (size_t i = 0; i < P.pmb.size(); i++) info[i] = P.pmb[i].info;
	for (uint32_t k = 0; k < count; k++) { chosen[k] = (uint8_t)P.pics[k].q; bytes[k] = P.rout[(size_t)k * 4 + 2]; }
	return run_place_and_write(P, true, pic_off, pic_bytes, stream_begin, stream_end);
}

/* ------------------------------------------------------------------ a handle that is called again and again (enc_chain.h) */

struct SimChain {
	uint32_t w, h, frame_rate_code, max_streams, gop, R, T, q_min, q_max, W;
	std::vector<JmEncChain> chain;
	std::vector<uint8_t> carry;
	std::vector<uint64_t> spent;
	size_t fb;
};

extern "C" SimChain *sim_chain_create(uint32_t w, uint32_t h, uint32_t frame_rate_code, uint32_t max_streams) {
	SimChain *c = new SimChain();
	const uint32_t mbw = (w + 15u) >> 4, mbh = (h + 15u) >> 4;
	c->w = w; c->h = h; c->frame_rate_code = frame_rate_code; c->max_streams = max_streams;
	c->gop = 1; c->R = 0; c->T = 0; c->q_min = 1; c->q_max = JM_ENCR_MAX_Q; c->W = 1;
	c->fb = (size_t)mbw * 16 * mbh * 16 * 3 / 2;
	c->chain.assign(max_streams, JmEncChain{ 0, 0, 0, 0 });
	c->carry.assign(2 * (size_t)max_streams * c->fb + 16, 0xa5);      /* a frame nobody wrote is never read */
	c->spent.assign(2 * (size_t)max_streams, 0);
	return c;
}
extern "C" void sim_chain_destroy(SimChain *c) { delete c; }
extern "C" void sim_chain_set_gop(SimChain *c, uint32_t gop, uint32_t R) {
	c->gop = gop; c->R = R;
	for (JmEncChain &r : c->chain) jm_encc_reset(r);
}
extern "C" void sim_chain_set_rate(SimChain *c, uint32_t T, uint32_t q_min, uint32_t q_max, uint32_t W) { c->T = T; c->q_min = q_min; c->q_max = q_max; c->W = W; }
extern "C" int sim_chain_reset(SimChain *c, uint32_t stream) {
	if (stream != 0xffffffffu && stream >= c->max_streams) return -1;
	for (uint32_t s = 0; s < c->max_streams; s++)
		if (stream == 0xffffffffu || s == stream) jm_encc_reset(c->chain[s]);
	return 0;
}
extern "C" int sim_chain_info(SimChain *c, uint32_t stream, uint32_t *out) {
	if (stream >= c->max_streams) return -1;
	out[0] = c->chain[stream].have; out[1] = c->chain[stream].n;
	return 0;
}
/* the record as it is, for the tests of the rule itself: have, n, parity, rated */
extern "C" void sim_chain_record(SimChain *c, uint32_t stream, uint32_t *out) {
	const JmEncChain &r = c->chain[stream];
	out[0] = r.have; out[1] = r.n; out[2] = r.parity; out[3] = r.rated;
}
extern "C" void sim_chain_set_record(SimChain *c, uint32_t stream, const uint32_t *in) { c->chain[stream] = JmEncChain{ in[0], in[1], in[2], in[3] }; }
extern "C" uint32_t sim_chain_next(uint32_t ordinal, uint32_t gop) { return jm_encc_next(ordinal, gop); }

/* One call.  flags: 1 END, 2 CHAIN.  q: the caller's scales, one per picture (with rate control: the chosen ones, out);
 * ordinal, budget, bytes: count each, out (the last two with rate control only); recon: count frames out, wherever the call
 * put them; the rest as in sim_encode_p.  Returns the total, -1 on overflow (a chained call's streams are reset, as when the
 * device's pass is settled), -2 for what this simulator does not cover: gop 1 without rate control is not the level loop. */
extern "C" int64_t sim_chain_encode(SimChain *c, const uint8_t *frames, uint32_t count, const uint32_t *stream, uint8_t *q, uint32_t flags,
                                    uint8_t *out, uint64_t cap, uint64_t *pic_off, uint32_t *pic_bytes, uint64_t *stream_begin, uint64_t *stream_end,
                                    uint8_t *recon_out, uint32_t *info, uint32_t *stats, uint32_t *ordinal, uint64_t *budget, uint32_t *bytes) {
	const bool chained = (flags & 2u) != 0, end = (flags & 1u) != 0, rate = c->T != 0;
	if ((c->gop == 1 && !rate) || (flags & ~3u)) return -2;
	Pass P(frames, c->w, c->h, count, stream, q, c->frame_rate_code, end, c->max_streams, out, cap);
	std::vector<JmEncPlan> plan(count);
	std::vector<uint8_t> store((size_t)count * c->fb + 16, 0x5a);
	jm_encc_plan_call(stream, count, c->chain.data(), rate, c->gop, chained, end, plan.data());
	for (uint32_t k = 0; k < count; k++) {
		const JmEncPlan &pl = plan[k];
		JmEncPic &pic = P.pics[k];
		pic.ordinal = ordinal[k] = pl.ordinal; pic.last = pl.last; pic.m = pl.m; pic.before = pl.before; pic.carry = pl.carry;
		pic.ref = jm_encc_frame(pl.ref, store.data(), c->carry.data(), c->fb);
		pic.recon = jm_encc_frame(pl.recon, store.data(), c->carry.data(), c->fb);
	}
	P.level_stores(c->gop, c->R, stats);
	if (rate) P.rate_stores(c->T, c->q_min, c->q_max, c->W, c->spent.data());
	run_levels(P, jm_encc_levels(plan.data(), count, c->gop, P.list.data(), P.begin.data()), rate, budget);
	for (size_t i = 0; i < P.pmb.size(); i++) info[i] = P.pmb[i].info;
	for (uint32_t k = 0; k < count; k++) {
		memcpy(recon_out + k * c->fb, P.pics[k].recon, c->fb);
		if (rate) { q[k] = (uint8_t)P.pics[k].q; bytes[k] = P.rout[(size_t)k * 4 + 2]; }
	}
	const int64_t total = run_place_and_write(P, true, pic_off, pic_bytes, stream_begin, stream_end);
	if (total < 0 && chained)
		for (uint32_t k = 0; k < count; k++) jm_encc_reset(c->chain[P.pics[k].stream]);
	return total;
}

#ifdef SIM_CHAIN_MAIN
/* A stand-alone program for sanitizer builds (g++ -fsanitize=address,undefined -DSIM_CHAIN_MAIN): argv[1] holds n frames of
 * w x h (argv[2..4]); every way of cutting them into chained calls, at (gop 3, R 7) and (gop 4, R 0), q 1 and 8, against one
 * unchained call (sim_encode_p).  Exit status 0: every cut gave the one call's stream and reconstructions. */
#include <stdio.h>
#include <stdlib.h>

int main(int argc, char **argv) {
	if (argc != 5) { fprintf(stderr, "usage: %s frames.bin width height count\n", argv[0]); return 2; }
	const uint32_t w = (uint32_t)atoi(argv[2]), h = (uint32_t)atoi(argv[3]), n = (uint32_t)atoi(argv[4]);
	const uint32_t mbw = (w + 15u) >> 4, mbh = (h + 15u) >> 4, mbs = mbw * mbh;
	const size_t fb = (size_t)mbw * 16 * mbh * 16 * 3 / 2, cap = 64 + n * (fb * 4 + 4096);
	std::vector<uint8_t> frames(n * fb);
	FILE *f = fopen(argv[1], "rb");
	if (!f || fread(frames.data(), 1, frames.size(), f) != frames.size()) { fprintf(stderr, "cannot read %zu bytes of %s\n", frames.size(), argv[1]); return 2; }
	fclose(f);
	if (n < 1 || n > 12) return 2;
	const uint32_t configs[2][2] = { { 3, 7 }, { 4, 0 } }, scales[2] = { 1, 8 };
	unsigned checked = 0;
	for (const auto &cfg : configs)
		for (const uint32_t qs : scales) {
			std::vector<uint8_t> q(n, (uint8_t)qs), one(cap + JM_ENC_TAIL + 16), one_recon(n * fb + 16), out(cap + JM_ENC_TAIL + 16), recon(n * fb + 16);
			std::vector<uint64_t> po(n), sb(1), se(1), budget(n);
			std::vector<uint32_t> pb(n), info((size_t)n * mbs), stats(n * 4), ordinal(n), bytes(n);
			if (sim_encode_p(frames.data(), w, h, n, nullptr, q.data(), 5, 1, 1, cfg[0], cfg[1], one.data(), cap, po.data(), pb.data(), sb.data(), se.data(),
			                 one_recon.data(), info.data(), stats.data()) < 0) return 3;
			const std::vector<uint8_t> want(one.begin() + sb[0], one.begin() + se[0]);
			for (uint32_t mask = 0; mask < (1u << (n - 1)); mask++) {
				SimChain *c = sim_chain_create(w, h, 5, 1);
				sim_chain_set_gop(c, cfg[0], cfg[1]);
				std::vector<uint8_t> got, got_recon;
				for (uint32_t at = 0; at < n;) {
					uint32_t len = 1;
					while (at + len < n && !(mask >> (at + len - 1) & 1u)) len++;
					const bool last = at + len == n;
					if (sim_chain_encode(c, frames.data() + at * fb, len, nullptr, q.data(), (last ? 1u : 0u) | 2u, out.data(), cap, po.data(), pb.data(), sb.data(), se.data(),
					                     recon.data(), info.data(), stats.data(), ordinal.data(), budget.data(), bytes.data()) < 0) return 3;
					got.insert(got.end(), out.begin() + sb[0], out.begin() + se[0]);
					got_recon.insert(got_recon.end(), recon.begin(), recon.begin() + len * fb);
					at += len;
				}
				uint32_t rec[2];
				sim_chain_info(c, 0, rec);
				sim_chain_destroy(c);
				if (got != want || memcmp(got_recon.data(), one_recon.data(), n * fb) != 0 || rec[0] != 0) {
					fprintf(stderr, "gop %u R %u q %u cut %u differs\n", cfg[0], cfg[1], qs, mask);
					return 1;
				}
				checked++;
			}
		}
	printf("%u cuts equal the one call\n", checked);
	return 0;
}
#endif
