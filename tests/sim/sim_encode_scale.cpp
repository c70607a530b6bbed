/* TEST-ONLY simulator of k_enc_scale (jsmpeg_amd/csrc/encode.hip): enc_scale.h's taps, weights and roundings run per output
 * sample in scalar loops on the CPU -- not through the table the kernel reads -- so that tests/test_enc_scale_sim.py holds
 * them against the numpy restatement (tests/enc_scale_ref.py) and torch without a GPU; and the table held against them. */
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "enc_scale.h"

/* "" or the descriptor check's message */
extern "C" const char *sim_es_check(const jsmpeg_hip_enc_source_t *s) {
	const char *m = jm_es_check(s);
	return m ? m : "";
}

/* the taps of output index i of an axis: out[0] = xmin, out[1] = xsize, weights[0 .. xsize) (at most cap) */
extern "C" void sim_es_taps(uint32_t n_in, uint32_t n_out, uint32_t aa, uint32_t i, uint32_t *out, uint32_t *weights, uint32_t cap) {
	const JmEsAxis a = { n_in, n_out, aa };
	const JmEsTaps t = jm_es_taps(a, i);
	out[0] = t.xmin; out[1] = t.xsize;
	for (uint32_t j = 0; j < t.xsize && j < cap; j++) weights[j] = jm_es_weight(a, t, j);
}

/* one plane: the crop n_in_x x n_in_y at (x0, y0) of `src` (row stride src_w) -> pw x ph scaled samples, extended by edge
 * replication to out_w x out_h */
static void scale_plane(const uint8_t *src, uint32_t src_w, uint32_t x0, uint32_t y0, const JmEsAxis &ax, const JmEsAxis &ay,
                        uint8_t *out, uint32_t out_w, uint32_t out_h) {
	for (uint32_t y = 0; y < out_h; y++) {
		const JmEsTaps vt = jm_es_taps(ay, y < ay.n_out ? y : ay.n_out - 1u);
		for (uint32_t x = 0; x < out_w; x++) {
			const JmEsTaps ht = jm_es_taps(ax, x < ax.n_out ? x : ax.n_out - 1u);
			uint32_t v = 0;
			for (uint32_t k = 0; k < vt.xsize; k++) {
				const uint8_t *row = src + (size_t)(y0 + vt.xmin + k) * src_w + x0 + ht.xmin;
				uint32_t h = 0;
				for (uint32_t j = 0; j < ht.xsize; j++) h += jm_es_weight(ax, ht, j) * row[j];
				v += jm_es_weight(ay, vt, k) * jm_es_round_h(h);
			}
			out[(size_t)y * out_w + x] = (uint8_t)jm_es_round_v(v);
		}
	}
}

/* One source frame (Y | Cr | Cb of the source's coded size) -> the encoder's frame (coded size of W x H).  0, or -1 for a
 * descriptor the check refuses. */
extern "C" int sim_es_frame(const uint8_t *frame, const jsmpeg_hip_enc_source_t *s, uint32_t W, uint32_t H, uint8_t *out) {
	if (jm_es_check(s) || W < 1 || W > JM_ES_MAX_SIDE || H < 1 || H > JM_ES_MAX_SIDE) return -1;
	const JmEsPlan p = jm_es_plan(s, W, H);
	for (int c = 0; c < 3; c++) {
		const JmEsPlane &q = p.pl[c ? 1 : 0];
		const size_t so = c == 0 ? 0 : c == 1 ? p.src_luma : (size_t)p.src_luma + p.src_chroma;
		const size_t oo = c == 0 ? 0 : c == 1 ? p.out_luma : (size_t)p.out_luma + p.out_chroma;
		scale_plane(frame + so, q.src_w, q.x0, q.y0, q.ax, q.ay, out + oo, q.out_w, q.out_h);
	}
	return 0;
}

/* The launch plan and the table the kernel reads, held against the functions and walked tile by tile as the kernel walks
 * them: 0, or the number of the first thing that is wrong.  out[0]: the table's words, out[1]: its bound, out[2]: the tiles,
 * out[3]: the fewest source rows a chunk holds. */
extern "C" int sim_es_plan_check(const jsmpeg_hip_enc_source_t *s, uint32_t W, uint32_t H, uint32_t *out) {
	if (jm_es_check(s)) return -1;
	const JmEsPlan p = jm_es_plan(s, W, H);
	out[0] = p.words; out[1] = jm_es_table_bound(W, H); out[2] = p.tiles; out[3] = JM_ES_CR;
	if (p.words > out[1]) return 1;
	std::vector<uint32_t> tab(p.words + 1u, 0xdeadbeefu);
	jm_es_table(p, tab.data());
	if (tab[p.words] != 0xdeadbeefu) return 2;
	const uint16_t *w = reinterpret_cast<const uint16_t *>(tab.data() + p.wts);
	const uint32_t scw = (s->width + 15u) & ~15u, sch = (s->height + 15u) & ~15u;
	for (int i = 0; i < 2; i++) {
		const JmEsPlane &q = p.pl[i];
		const uint32_t src_h = i ? sch >> 1 : sch, gran = i ? 8u : 16u;
		if (q.src_w != (i ? scw >> 1 : scw)) return 3;
		for (int v = 0; v < 2; v++) {
			const JmEsAxis &a = v ? q.ay : q.ax;
			const uint32_t *ent = tab.data() + (v ? q.ent_y : q.ent_x);
			for (uint32_t o = 0; o < a.n_out; o++) {
				const JmEsTaps t = jm_es_taps(a, o);
				if (ent[2u * o] != (t.xmin | (t.xsize << 16))) return 4;
				if (2u * p.wts + ent[2u * o + 1u] + t.xsize > 2u * p.words) return 5;
				for (uint32_t j = 0; j < t.xsize; j++)
					if (w[ent[2u * o + 1u] + j] != jm_es_weight(a, t, j)) return 6;
			}
		}
		/* the tiles: every real sample once; the staged span inside the source plane and inside the staging bytes */
		if (q.tiles_x * JM_ES_TW < q.out_w || q.tiles_y * JM_ES_TH < q.out_h || (q.tiles_x - 1u) * JM_ES_TW >= q.out_w || (q.tiles_y - 1u) * JM_ES_TH >= q.out_h) return 7;
		const uint32_t *ex = tab.data() + q.ent_x, *ey = tab.data() + q.ent_y;
		for (uint32_t tx = 0; tx < q.tiles_x; tx++) {
			const uint32_t ox0 = tx * JM_ES_TW, nw = q.out_w - ox0 < JM_ES_TW ? q.out_w - ox0 : JM_ES_TW;
			if (ox0 >= q.ax.n_out || (nw & 3u)) return 8;
			const uint32_t last = ox0 + nw - 1u < q.ax.n_out - 1u ? ox0 + nw - 1u : q.ax.n_out - 1u;
			const uint32_t ef = ex[2u * ox0], el = ex[2u * last];
			const uint32_t ax0 = (q.x0 + (ef & 0xffffu)) & ~(gran - 1u), ax1 = (q.x0 + (el & 0xffffu) + (el >> 16) + gran - 1u) & ~(gran - 1u);
			if (ax1 > q.src_w || ax1 <= ax0 || ax1 - ax0 > JM_ES_SRC) return 9;
			const uint32_t rows = JM_ES_SRC / (ax1 - ax0) < JM_ES_CR ? JM_ES_SRC / (ax1 - ax0) : JM_ES_CR;
			if (rows < out[3]) out[3] = rows;
			for (uint32_t o = ox0; o <= last; o++) {              /* every column's taps inside the staged span */
				const uint32_t b = q.x0 + (ex[2u * o] & 0xffffu);
				if (b < ax0 || b + (ex[2u * o] >> 16) > ax1) return 10;
			}
		}
		for (uint32_t ty = 0; ty < q.tiles_y; ty++) {
			const uint32_t oy0 = ty * JM_ES_TH, nh = q.out_h - oy0 < JM_ES_TH ? q.out_h - oy0 : JM_ES_TH;
			if (oy0 >= q.ay.n_out) return 11;
			const uint32_t last = oy0 + nh - 1u < q.ay.n_out - 1u ? oy0 + nh - 1u : q.ay.n_out - 1u;
			const uint32_t sy0 = ey[2u * oy0] & 0xffffu, sy1 = (ey[2u * last] & 0xffffu) + (ey[2u * last] >> 16);
			if (sy1 <= sy0 || q.y0 + sy1 > src_h) return 12;
			for (uint32_t o = oy0; o <= last; o++) {
				const uint32_t b = ey[2u * o] & 0xffffu;
				if (b < sy0 || b + (ey[2u * o] >> 16) > sy1) return 13;
			}
		}
	}
	if (out[3] < 2u) return 14;
	return 0;
}

/* One axis over all its output indices: out[0] the smallest weight (as a signed number: a weight that wrapped below 0 shows),
 * out[1] the largest, out[2] 1 when every output index's weights sum to exactly JM_ES_ONE and its taps lie inside 0 .. n_in,
 * out[3] how many output indices take the rule's second form (cumulative rounding). */
extern "C" void sim_es_axis_scan(uint32_t n_in, uint32_t n_out, uint32_t aa, int32_t *out) {
	const JmEsAxis a = { n_in, n_out, aa };
	int32_t lo = INT32_MAX, hi = INT32_MIN, exact = 1, second = 0;
	for (uint32_t i = 0; i < n_out; i++) {
		const JmEsTaps t = jm_es_taps(a, i);
		int64_t sum = 0;
		second += t.cum ? 1 : 0;
		if (t.xsize < 1 || (uint64_t)t.xmin + t.xsize > n_in) exact = 0;
		for (uint32_t j = 0; j < t.xsize; j++) {
			const int32_t w = (int32_t)jm_es_weight(a, t, j);
			sum += w;
			if (w < lo) lo = w;
			if (w > hi) hi = w;
		}
		if (sum != (int64_t)JM_ES_ONE) exact = 0;
	}
	out[0] = lo; out[1] = hi; out[2] = exact; out[3] = second;
}

/* One axis written out: ent[2 i] = xmin, ent[2 i + 1] = xsize of output index i, the weights (signed, as above) one index after
 * the other.  Returns the number of weights; nothing beyond `cap` of them is written. */
extern "C" uint32_t sim_es_axis(uint32_t n_in, uint32_t n_out, uint32_t aa, uint32_t *ent, int32_t *weights, uint32_t cap) {
	const JmEsAxis a = { n_in, n_out, aa };
	uint32_t at = 0;
	for (uint32_t i = 0; i < n_out; i++) {
		const JmEsTaps t = jm_es_taps(a, i);
		ent[2u * i] = t.xmin; ent[2u * i + 1u] = t.xsize;
		for (uint32_t j = 0; j < t.xsize; j++, at++)
			if (at < cap) weights[at] = (int32_t)jm_es_weight(a, t, j);
	}
	return at;
}

/* The workgroups of one picture as k_enc_scale walks them -- its own expressions (encode.hip, the lines between the tile index
 * and the chunk loop) over the table the host builds, the header's tile constants -- a record of SIM_ES_WALK_FIELDS words each
 * into rec (at most cap records are written).  Returns the number of workgroups, or -1 for a descriptor the check refuses.  It
 * takes no part in computing samples: the tests read from it which edge of the kernel an input reaches.
 *   0 plane kind (0 luma, 1 Cr, 2 Cb)   1 tile column   2 tile row   3 nw   4 nh   5 stride   6 cr_max   7 chunks
 *   8 source rows of the last chunk   9 rows of the tile whose vertical taps lie in more than one chunk
 *   10 (x0 + the first column's xmin) mod the load granule   11 bit 0: the tile reaches past n_out in x, bit 1: in y */
#define SIM_ES_WALK_FIELDS 12u
extern "C" int sim_es_walk(const jsmpeg_hip_enc_source_t *s, uint32_t W, uint32_t H, uint32_t *rec, uint32_t cap) {
	if (jm_es_check(s) || W < 1 || W > JM_ES_MAX_SIDE || H < 1 || H > JM_ES_MAX_SIDE) return -1;
	const JmEsPlan plan = jm_es_plan(s, W, H);
	std::vector<uint32_t> tab(plan.words);
	jm_es_table(plan, tab.data());
	const uint32_t nl = plan.pl[0].tiles_x * plan.pl[0].tiles_y, nc = plan.pl[1].tiles_x * plan.pl[1].tiles_y;
	for (uint32_t b = 0; b < plan.tiles; b++) {
		uint32_t tile = b, comp = 0;
		if (tile >= nl) { tile -= nl; comp = 1; if (tile >= nc) { tile -= nc; comp = 2; } }
		const JmEsPlane q = comp ? plan.pl[1] : plan.pl[0];
		const uint32_t ox0 = (tile % q.tiles_x) * JM_ES_TW, oy0 = (tile / q.tiles_x) * JM_ES_TH;
		const uint32_t nw = std::min(JM_ES_TW, q.out_w - ox0), nh = std::min(JM_ES_TH, q.out_h - oy0);
		const uint32_t *ex = tab.data() + q.ent_x, *ey = tab.data() + q.ent_y;
		const uint32_t ef = ex[2u * ox0], el = ex[2u * std::min(ox0 + nw - 1u, q.ax.n_out - 1u)];
		const uint32_t vf = ey[2u * oy0], vl = ey[2u * std::min(oy0 + nh - 1u, q.ay.n_out - 1u)];
		const uint32_t gran = comp ? 8u : 16u;
		const uint32_t ax0 = (q.x0 + (ef & 0xffffu)) & ~(gran - 1u), ax1 = (q.x0 + (el & 0xffffu) + (el >> 16) + gran - 1u) & ~(gran - 1u);
		const uint32_t stride = ax1 - ax0, cr_max = std::min(JM_ES_CR, JM_ES_SRC / stride);
		const uint32_t sy0 = vf & 0xffffu, sy1 = (vl & 0xffffu) + (vl >> 16);
		uint32_t chunks = 0, last_rows = 0, straddle = 0;
		for (uint32_t r0 = sy0; r0 < sy1; r0 += cr_max) { chunks++; last_rows = std::min(cr_max, sy1 - r0); }
		for (uint32_t ol = 0; ol < nh; ol++) {
			const uint32_t e = ey[2u * std::min(oy0 + ol, q.ay.n_out - 1u)], xmin = e & 0xffffu, xsize = e >> 16;
			if ((xmin - sy0) / cr_max != (xmin + xsize - 1u - sy0) / cr_max) straddle++;
		}
		if (b >= cap) continue;
		uint32_t *r = rec + (size_t)b * SIM_ES_WALK_FIELDS;
		r[0] = comp; r[1] = tile % q.tiles_x; r[2] = tile / q.tiles_x; r[3] = nw; r[4] = nh; r[5] = stride; r[6] = cr_max;
		r[7] = chunks; r[8] = last_rows; r[9] = straddle; r[10] = (q.x0 + (ef & 0xffffu)) % gran;
		r[11] = (ox0 + nw > q.ax.n_out ? 1u : 0u) | (oy0 + nh > q.ay.n_out ? 2u : 0u);
	}
	return (int)plan.tiles;
}

#ifdef SIM_ES_MAIN
/* A stand-alone program for the sanitizers (g++ -fsanitize=address,undefined): a seeded sweep of geometries through the frame
 * and the plan check, the frames in buffers of exactly their size, and the table's bound at the largest sources. */
#include <stdio.h>
#include <stdlib.h>

static uint32_t g_seed = 12345u;
static uint32_t rnd(uint32_t n) { g_seed = g_seed * 1664525u + 1013904223u; return (g_seed >> 8) % n; }

int main(int argc, char **argv) {
	const int n = argc > 1 ? atoi(argv[1]) : 150;
	uint32_t out[4];
	for (int k = 0; k < n; k++) {
		jsmpeg_hip_enc_source_t s;
		memset(&s, 0, sizeof(s));
		s.width = 1u + rnd(80); s.height = 1u + rnd(80); s.antialias = rnd(2);
		if (k & 1) {
			s.crop_x = 2u * rnd((s.width + 1u) / 2u); s.crop_y = 2u * rnd((s.height + 1u) / 2u);
			s.crop_width = 1u + rnd(s.width - s.crop_x); s.crop_height = 1u + rnd(s.height - s.crop_y);
		}
		const uint32_t W = 1u + rnd(80), H = 1u + rnd(80);
		const size_t sb = (size_t)((s.width + 15u) & ~15u) * ((s.height + 15u) & ~15u) * 3 / 2, ob = (size_t)((W + 15u) & ~15u) * ((H + 15u) & ~15u) * 3 / 2;
		std::vector<uint8_t> src(sb), dst(ob);
		for (size_t i = 0; i < sb; i++) src[i] = (uint8_t)rnd(256);
		if (sim_es_frame(src.data(), &s, W, H, dst.data()) != 0) { printf("geometry %d refused\n", k); return 1; }
		const int rc = sim_es_plan_check(&s, W, H, out);
		if (rc) { printf("geometry %d: plan check %d\n", k, rc); return 1; }
	}
	/* (from the fifth on: tests/enc_scale_inputs.py's RATIOS, whose weights take the rule's second form) */
	const uint32_t big[][4] = { { 4095, 4095, 1, 1 }, { 4095, 4095, 4095, 2800 }, { 1, 1, 4095, 2800 }, { 4095, 2, 2048, 1 },
	                            { 1280, 2, 1, 1 }, { 3120, 2, 1, 1 }, { 2870, 2, 2, 2 }, { 3418, 2, 2, 1 }, { 2, 3120, 1, 1 }, { 2560, 2, 2, 2 } };
	for (const auto &g : big) {
		jsmpeg_hip_enc_source_t s;
		memset(&s, 0, sizeof(s));
		s.width = g[0]; s.height = g[1]; s.antialias = 1;
		const int rc = sim_es_plan_check(&s, g[2], g[3], out);
		if (rc) { printf("%u x %u -> %u x %u: plan check %d\n", g[0], g[1], g[2], g[3], rc); return 1; }
		std::vector<uint32_t> rec((size_t)out[2] * SIM_ES_WALK_FIELDS);
		if (sim_es_walk(&s, g[2], g[3], rec.data(), out[2]) != (int)out[2]) { printf("%u x %u -> %u x %u: the walk\n", g[0], g[1], g[2], g[3]); return 1; }
		if (g[0] * g[1] > 8192u) continue;
		/* the small ones through the frame as well, in buffers of exactly their size */
		const size_t sb = (size_t)((s.width + 15u) & ~15u) * ((s.height + 15u) & ~15u) * 3 / 2, ob = (size_t)((g[2] + 15u) & ~15u) * ((g[3] + 15u) & ~15u) * 3 / 2;
		std::vector<uint8_t> src(sb), dst(ob);
		for (size_t i = 0; i < sb; i++) src[i] = (uint8_t)rnd(256);
		if (sim_es_frame(src.data(), &s, g[2], g[3], dst.data()) != 0) { printf("%u x %u -> %u x %u refused\n", g[0], g[1], g[2], g[3]); return 1; }
	}
	printf("%d geometries and the largest plans are clean\n", n);
	return 0;
}
#endif
