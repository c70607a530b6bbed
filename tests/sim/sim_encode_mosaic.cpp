/* TEST-ONLY simulator of k_enc_mosaic (jsmpeg_amd/csrc/encode.hip): enc_mosaic.h's rule run pixel by pixel in scalar loops on
 * the CPU -- the fill, every cell's samples from enc_scale.h's taps, weights and roundings (not through the table the kernel
 * reads) pasted in index order, the edge replication -- so that tests/test_enc_mosaic_sim.py holds it against the numpy
 * restatement (tests/enc_mosaic_ref.py) without a GPU; and the table and the tile walk held against the functions. */
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "enc_mosaic.h"

extern "C" uint32_t sim_em_sizeof_cell(void) { return (uint32_t)sizeof(jsmpeg_hip_enc_cell_t); }

/* 0 and "", or -1 and the layout check's message, with "cell k: " in front when it is about a cell */
extern "C" int sim_em_check(const jsmpeg_hip_enc_cell_t *cells, uint32_t n, uint32_t fill, uint32_t W, uint32_t H, char *msg, uint32_t cap) {
	uint32_t cell;
	const char *m = jm_em_check(cells, n, fill, W, H, &cell);
	if (!m) { if (cap) msg[0] = 0; return 0; }
	if (cell == 0xffffffffu) snprintf(msg, cap, "%s", m);
	else snprintf(msg, cap, "cell %u: %s", cell, m);
	return -1;
}

/* one plane of one cell: the crop at (x0, y0) of `src` (row stride src_w) scaled to ax.n_out x ay.n_out, pasted at (dx, dy)
 * of `out` (row stride out_w) */
static void paste_plane(const uint8_t *src, uint32_t src_w, uint32_t x0, uint32_t y0, const JmEsAxis &ax, const JmEsAxis &ay,
                        uint8_t *out, uint32_t out_w, uint32_t dx, uint32_t dy) {
	for (uint32_t y = 0; y < ay.n_out; y++) {
		const JmEsTaps vt = jm_es_taps(ay, y);
		for (uint32_t x = 0; x < ax.n_out; x++) {
			const JmEsTaps ht = jm_es_taps(ax, x);
			uint32_t v = 0;
			for (uint32_t k = 0; k < vt.xsize; k++) {
				const uint8_t *row = src + (size_t)(y0 + vt.xmin + k) * src_w + x0 + ht.xmin;
				uint32_t h = 0;
				for (uint32_t j = 0; j < ht.xsize; j++) h += jm_es_weight(ax, ht, j) * row[j];
				v += jm_es_weight(ay, vt, k) * jm_es_round_h(h);
			}
			out[(size_t)(dy + y) * out_w + dx + x] = (uint8_t)jm_es_round_v(v);
		}
	}
}

/* One picture: frames[c] (Y | Cr | Cb of cell c's source's coded size) or NULL per cell -> the encoder's frame (coded size of
 * W x H).  0, or -1 for a layout the check refuses. */
extern "C" int sim_em_frame(const uint8_t *const *frames, const jsmpeg_hip_enc_cell_t *cells, uint32_t n, uint32_t fill, uint32_t W, uint32_t H, uint8_t *out) {
	uint32_t cell;
	if (W < 1 || W > JM_ES_MAX_SIDE || H < 1 || H > JM_ES_MAX_SIDE || jm_em_check(cells, n, fill, W, H, &cell)) return -1;
	const JmEmPlan p = jm_em_plan(cells, n, fill, W, H);
	for (int c = 0; c < 3; c++) {
		const int i = c ? 1 : 0;
		uint8_t *O = out + (c == 0 ? 0 : c == 1 ? p.out_luma : (size_t)p.out_luma + p.out_chroma);
		const uint32_t ow = p.out_w[i], oh = p.out_h[i], pw = p.disp_w[i], ph = p.disp_h[i];
		for (uint32_t y = 0; y < ph; y++) memset(O + (size_t)y * ow, (int)((fill >> (8 * c)) & 0xffu), pw);
		for (uint32_t k = 0; k < n; k++) {
			if (!frames[k]) continue;
			const JmEsPlan s = jm_es_plan(&cells[k].source, cells[k].width, cells[k].height);
			const JmEsPlane &q = s.pl[i];
			const size_t so = c == 0 ? 0 : c == 1 ? s.src_luma : (size_t)s.src_luma + s.src_chroma;
			paste_plane(frames[k] + so, q.src_w, q.x0, q.y0, q.ax, q.ay, O, ow, i ? cells[k].x >> 1 : cells[k].x, i ? cells[k].y >> 1 : cells[k].y);
		}
		for (uint32_t y = 0; y < oh; y++)
			for (uint32_t x = 0; x < ow; x++)
				if (x >= pw || y >= ph) O[(size_t)y * ow + x] = O[(size_t)(y < ph ? y : ph - 1u) * ow + (x < pw ? x : pw - 1u)];
	}
	return 0;
}

/* The plan and the table the kernel reads, held against the functions and walked tile by tile and cell by cell as the kernel
 * walks them: 0, or the number of the first thing that is wrong.  out[0]: the table's words, out[1]: its bound, out[2]: the
 * tiles, out[3]: the fewest source rows a chunk holds. */
extern "C" int sim_em_plan_check(const jsmpeg_hip_enc_cell_t *cells, uint32_t n, uint32_t fill, uint32_t W, uint32_t H, uint32_t *out) {
	uint32_t cell;
	if (jm_em_check(cells, n, fill, W, H, &cell)) return -1;
	const JmEmPlan p = jm_em_plan(cells, n, fill, W, H);
	out[0] = p.words; out[1] = jm_em_table_bound(n, W, H); out[2] = p.tiles; out[3] = JM_ES_CR;
	if (p.words > out[1]) return 1;
	if (!jm_em_tiles_ok(p)) return 2;
	std::vector<uint32_t> tab(p.words + 1u, 0xdeadbeefu);
	jm_em_table(p, cells, tab.data());
	if (tab[p.words] != 0xdeadbeefu) return 3;
	for (int i = 0; i < 2; i++) {
		if (p.tiles_x[i] * JM_ES_TW < p.out_w[i] || p.tiles_y[i] * JM_ES_TH < p.out_h[i] || (p.tiles_x[i] - 1u) * JM_ES_TW >= p.out_w[i] ||
		    (p.tiles_y[i] - 1u) * JM_ES_TH >= p.out_h[i]) return 4;
		if (p.disp_w[i] > p.out_w[i] || p.disp_h[i] > p.out_h[i]) return 5;
	}
	for (uint32_t c = 0; c < n; c++) {
		JmEmCellRec r;
		memcpy(&r, tab.data() + c * JM_EM_REC, sizeof(r));
		const jsmpeg_hip_enc_source_t &s = cells[c].source;
		const uint32_t scw = (s.width + 15u) & ~15u, sch = (s.height + 15u) & ~15u;
		if (r.dx != cells[c].x || r.dy != cells[c].y || r.pl[0].ax.n_out != cells[c].width || r.pl[0].ay.n_out != cells[c].height) return 6;
		if (r.pl[1].ax.n_out != (cells[c].width + 1u) >> 1 || r.pl[1].ay.n_out != (cells[c].height + 1u) >> 1) return 6;
		if (r.src_luma != scw * sch || r.src_chroma != r.src_luma >> 2) return 7;
		const uint16_t *w = reinterpret_cast<const uint16_t *>(tab.data() + r.wts);
		for (int i = 0; i < 2; i++) {
			const JmEsPlane &q = r.pl[i];
			const uint32_t src_h = i ? sch >> 1 : sch, gran = i ? 8u : 16u;
			uint32_t rect[4];
			jm_em_rect(r, i, rect);
			if (q.src_w != (i ? scw >> 1 : scw)) return 8;
			if (rect[0] + rect[2] > p.disp_w[i] || rect[1] + rect[3] > p.disp_h[i]) return 9;
			for (int v = 0; v < 2; v++) {
				const JmEsAxis &a = v ? q.ay : q.ax;
				const uint32_t e0 = v ? q.ent_y : q.ent_x;
				if (e0 < n * JM_EM_REC || e0 + 2u * a.n_out > r.wts) return 10;
				const uint32_t *ent = tab.data() + e0;
				for (uint32_t o = 0; o < a.n_out; o++) {
					const JmEsTaps t = jm_es_taps(a, o);
					if (ent[2u * o] != (t.xmin | (t.xsize << 16))) return 11;
					if (2u * r.wts + ent[2u * o + 1u] + t.xsize > 2u * p.words) return 12;
					for (uint32_t j = 0; j < t.xsize; j++)
						if (w[ent[2u * o + 1u] + j] != jm_es_weight(a, t, j)) return 13;
				}
			}
			/* the tiles this cell meets: the staged span of the intersection inside the source plane and the staging bytes */
			const uint32_t *ex = tab.data() + q.ent_x, *ey = tab.data() + q.ent_y;
			for (uint32_t tx = 0; tx < p.tiles_x[i]; tx++) {
				const uint32_t ox0 = tx * JM_ES_TW, nw = p.out_w[i] - ox0 < JM_ES_TW ? p.out_w[i] - ox0 : JM_ES_TW;
				const uint32_t vw = p.disp_w[i] - ox0 < nw ? p.disp_w[i] - ox0 : nw;
				const uint32_t ix0 = rect[0] > ox0 ? rect[0] : ox0, ix1 = rect[0] + rect[2] < ox0 + vw ? rect[0] + rect[2] : ox0 + vw;
				if (ix0 >= ix1) continue;
				const uint32_t lx0 = ix0 - rect[0], lx1 = ix1 - rect[0];
				const uint32_t ef = ex[2u * lx0], el = ex[2u * (lx1 - 1u)];
				const uint32_t ax0 = (q.x0 + (ef & 0xffffu)) & ~(gran - 1u), ax1 = (q.x0 + (el & 0xffffu) + (el >> 16) + gran - 1u) & ~(gran - 1u);
				if (ax1 > q.src_w || ax1 <= ax0 || ax1 - ax0 > JM_ES_SRC) return 14;
				const uint32_t rows = JM_ES_SRC / (ax1 - ax0) < JM_ES_CR ? JM_ES_SRC / (ax1 - ax0) : JM_ES_CR;
				if (rows < out[3]) out[3] = rows;
				for (uint32_t o = lx0; o < lx1; o++) {
					const uint32_t b = q.x0 + (ex[2u * o] & 0xffffu);
					if (b < ax0 || b + (ex[2u * o] >> 16) > ax1) return 15;
				}
			}
			for (uint32_t ty = 0; ty < p.tiles_y[i]; ty++) {
				const uint32_t oy0 = ty * JM_ES_TH, nh = p.out_h[i] - oy0 < JM_ES_TH ? p.out_h[i] - oy0 : JM_ES_TH;
				const uint32_t vh = p.disp_h[i] - oy0 < nh ? p.disp_h[i] - oy0 : nh;
				const uint32_t iy0 = rect[1] > oy0 ? rect[1] : oy0, iy1 = rect[1] + rect[3] < oy0 + vh ? rect[1] + rect[3] : oy0 + vh;
				if (iy0 >= iy1) continue;
				const uint32_t ly0 = iy0 - rect[1], ly1 = iy1 - rect[1];
				const uint32_t sy0 = ey[2u * ly0] & 0xffffu, sy1 = (ey[2u * (ly1 - 1u)] & 0xffffu) + (ey[2u * (ly1 - 1u)] >> 16);
				if (sy1 <= sy0 || q.y0 + sy1 > src_h) return 16;
				for (uint32_t o = ly0; o < ly1; o++) {
					const uint32_t b = ey[2u * o] & 0xffffu;
					if (b < sy0 || b + (ey[2u * o] >> 16) > sy1) return 17;
				}
			}
		}
	}
	if (out[3] < 2u) return 18;
	return 0;
}

#ifdef SIM_EM_MAIN
/* A stand-alone program for the sanitizers (g++ -fsanitize=address,undefined): a seeded sweep of layouts through the frame
 * and the plan check, every frame in a buffer of exactly its size, and the table's bound at the extremes. */
#include <stdlib.h>

static uint32_t g_seed = 4711u;
static uint32_t rnd(uint32_t n) { g_seed = g_seed * 1664525u + 1013904223u; return (g_seed >> 8) % n; }

static jsmpeg_hip_enc_cell_t random_cell(uint32_t W, uint32_t H, uint32_t k) {
	jsmpeg_hip_enc_cell_t c;
	memset(&c, 0, sizeof(c));
	jsmpeg_hip_enc_source_t &s = c.source;
	s.width = 1u + rnd(96); s.height = 1u + rnd(96); s.antialias = rnd(2);
	if (k & 1) {
		s.crop_x = 2u * rnd((s.width + 1u) / 2u); s.crop_y = 2u * rnd((s.height + 1u) / 2u);
		s.crop_width = 1u + rnd(s.width - s.crop_x); s.crop_height = 1u + rnd(s.height - s.crop_y);
	}
	c.x = 2u * rnd((W + 1u) / 2u); c.y = 2u * rnd((H + 1u) / 2u);
	c.width = (k % 3u == 0) ? W - c.x : 1u + rnd(W - c.x);      /* every third flush with the right edge */
	c.height = (k % 3u == 1) ? H - c.y : 1u + rnd(H - c.y);     /* ... or the bottom edge */
	return c;
}

int main(int argc, char **argv) {
	const int n = argc > 1 ? atoi(argv[1]) : 150;
	uint32_t out[4];
	for (int k = 0; k < n; k++) {
		const uint32_t W = 1u + rnd(96), H = 1u + rnd(96), nc = 1u + rnd(6);
		std::vector<jsmpeg_hip_enc_cell_t> cells;
		std::vector<std::vector<uint8_t>> bufs;
		std::vector<const uint8_t *> frames;
		for (uint32_t c = 0; c < nc; c++) {
			cells.push_back(random_cell(W, H, (uint32_t)k + c));
			const jsmpeg_hip_enc_source_t &s = cells.back().source;
			bufs.emplace_back((size_t)((s.width + 15u) & ~15u) * ((s.height + 15u) & ~15u) * 3 / 2);
			for (uint8_t &b : bufs.back()) b = (uint8_t)rnd(256);
		}
		for (uint32_t c = 0; c < nc; c++) frames.push_back(rnd(5) == 0 ? nullptr : bufs[c].data());
		std::vector<uint8_t> dst((size_t)((W + 15u) & ~15u) * ((H + 15u) & ~15u) * 3 / 2);
		if (sim_em_frame(frames.data(), cells.data(), nc, 0x808010u, W, H, dst.data()) != 0) { printf("layout %d refused\n", k); return 1; }
		const int rc = sim_em_plan_check(cells.data(), nc, 0x808010u, W, H, out);
		if (rc) { printf("layout %d: plan check %d\n", k, rc); return 1; }
	}
	/* 64 cells of 4095-wide sources, and a 1 x 1 cell of the largest source */
	std::vector<jsmpeg_hip_enc_cell_t> wall(64);
	for (uint32_t c = 0; c < 64; c++) {
		memset(&wall[c], 0, sizeof(wall[c]));
		wall[c].source.width = 4095; wall[c].source.height = c & 1 ? 4095 : 16; wall[c].source.antialias = 1;
		wall[c].x = (c % 8u) * 64u; wall[c].y = (c / 8u) * 36u; wall[c].width = 64; wall[c].height = 36;
	}
	int rc = sim_em_plan_check(wall.data(), 64, 0, 512, 288, out);
	if (rc) { printf("the wall: plan check %d\n", rc); return 1; }
	wall[0].source.height = 4095; wall[0].x = 510; wall[0].y = 286; wall[0].width = 1; wall[0].height = 1;
	rc = sim_em_plan_check(wall.data(), 1, 0, 512, 288, out);
	if (rc) { printf("the 1 x 1 cell: plan check %d\n", rc); return 1; }
	printf("%d layouts and the largest plans are clean\n", n);
	return 0;
}
#endif
