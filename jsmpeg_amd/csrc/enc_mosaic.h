/*
 * Mosaic input of the encoder (include/jsmpeg_hip.h part 8, jsmpeg_hip_encoder_set_mosaic / _encode_mosaic): one coded picture
 * composed from many sources, plane to plane, on top of enc_scale.h -- what k_enc_mosaic (encode.hip), the CPU simulator
 * (tests/sim/sim_encode_mosaic.cpp) and the host side share: the layout check, the plan, the table and the tile plan.
 * Host + device.  tests/enc_mosaic_ref.py restates the rule in numpy by pasting enc_scale_ref's planes.
 *
 * LAYOUT    a fill colour (Y, Cr, Cb bytes: Y | Cr << 8 | Cb << 16) and n cells, 1 <= n <= 64.
 * CELL      a jsmpeg_hip_enc_source_t -- geometry, crop and antialias of that cell's frames, exactly as
 *           jsmpeg_hip_encoder_encode_scaled reads them -- and a destination x, y, width, height in the encoder's display
 *           pixels: x and y even, width and height at least 1, inside W x H.
 * SAMPLES   of a cell: the three scaled planes enc_scale.h defines (PLANES, TAPS, VALUE) for that source and crop at output
 *           size width x height:
 *             luma      width x height, pasted at (x, y)
 *             Cr, Cb    ((width + 1) >> 1) x ((height + 1) >> 1), pasted at (x >> 1, y >> 1)
 *           x is even and x + width <= W, so the chroma rectangle stays inside ((W + 1) >> 1) x ((H + 1) >> 1).
 * ORDER     each plane is filled with its byte of the fill colour; then the cells are pasted in index order, each plane
 *           independently: where cells overlap the later one wins (picture in picture).
 * ABSENT    a cell whose frame pointer is NULL for a picture is left out of that picture: what lies under it shows.  A picture
 *           whose cells are all absent is all fill.
 * CODED     the composed display planes extended by edge replication, as enc_scale.h CODED: output (x, y) of a plane of
 *           pw x ph composed samples is the composed sample (min(x, pw - 1), min(y, ph - 1)).
 * So one cell with the destination (0, 0, W, H) is bit for bit jsmpeg_hip_encoder_encode_scaled of that source.
 *
 * TABLE     what the kernel reads, in 32-bit words: n records JmEmCellRec, then per cell the table jm_es_table writes for the
 *           cell's source at output size width x height (entries at cell-local output indices, then its weights).  Cells that
 *           share an axis could share entries; this builder gives every cell its own.
 * TILES     a workgroup owns one JM_ES_TW x JM_ES_TH tile of one plane of the coded size of one picture, every byte of it:
 *           overlapping cells are ordered inside the workgroup.  Every tile holds at least one display column and one display
 *           row of its plane, so the edge replication never leaves the tile: a coded side is a multiple of 16 (luma) or 8
 *           (chroma), a tile's origin a multiple of JM_ES_TW / JM_ES_TH, both multiples of 16, so a luma tile begins at or
 *           below (coded - 16) < display, and a chroma tile at or below (coded - 16) / 2 < (display + 1) >> 1.
 *           jm_em_tiles_ok states that as a check.
 * OUT OF SCOPE: alpha blending; borders, labels and text; cells that change per picture within a call; rotation; a Node binding.
 */
#pragma once
#include <string.h>

#include "enc_scale.h"

#define JM_EM_MAX_CELLS 64u

/* One cell in the table: the cell's scale plan with its offsets made absolute, and where it goes */
struct JmEmCellRec {
	JmEsPlane pl[2];                 /* ax / ay: crop -> the cell's plane; x0, y0, src_w; ent_x / ent_y absolute in the table */
	uint32_t src_luma, src_chroma;   /* bytes of a source plane */
	uint32_t wts;                    /* where the cell's weights begin in the table, in 32-bit words */
	uint32_t dx, dy;                 /* the luma destination; chroma: dx >> 1, dy >> 1; the sizes are pl[i].ax.n_out x pl[i].ay.n_out */
};
#define JM_EM_REC ((uint32_t)(sizeof(JmEmCellRec) / 4u))

/* What a launch needs besides the frames and the table; index 0 luma, 1 chroma */
struct JmEmPlan {
	uint32_t n, fill;
	uint32_t disp_w[2], disp_h[2];   /* the composed planes */
	uint32_t out_w[2], out_h[2];     /* the planes of the coded size */
	uint32_t tiles_x[2], tiles_y[2];
	uint32_t out_luma, out_chroma;
	uint32_t tiles;                  /* of one picture: luma, Cr, Cb */
	uint32_t words;                  /* the table's size */
};

/* The layout check: 0, or a message (static text) of what the rule does not cover; *cell: the cell it is about, or
 * 0xffffffff for the layout as a whole */
JM_ES_FN const char *jm_em_check(const jsmpeg_hip_enc_cell_t *cells, uint32_t n, uint32_t fill, uint32_t W, uint32_t H, uint32_t *cell) {
	*cell = 0xffffffffu;
	if (n < 1 || n > JM_EM_MAX_CELLS) return "a layout has 1 .. 64 cells";
	if (!cells) return "null cells";
	if (fill > 0xffffffu) return "fill must be Y | Cr << 8 | Cb << 16";
	for (uint32_t c = 0; c < n; c++) {
		const jsmpeg_hip_enc_cell_t &q = cells[c];
		*cell = c;
		if (const char *why = jm_es_check(&q.source)) return why;
		if (q.width < 1 || q.height < 1) return "cell width and height must be at least 1";
		if ((q.x | q.y) & 1u) return "cell x and y must be even (the chroma samples would be sited half a sample off)";
		if ((uint64_t)q.x + q.width > W || (uint64_t)q.y + q.height > H) return "cell rectangle outside the picture";
	}
	*cell = 0xffffffffu;
	return 0;
}

/* the most 32-bit words the table of a layout of n cells takes in an encoder of W x H, whatever the sources: a cell is at most
 * W x H, and jm_es_table_bound does not decrease with the output size */
JM_ES_FN uint32_t jm_em_table_bound(uint32_t n, uint32_t W, uint32_t H) { return n * (JM_EM_REC + jm_es_table_bound(W, H)); }

JM_ES_FN JmEmPlan jm_em_plan(const jsmpeg_hip_enc_cell_t *cells, uint32_t n, uint32_t fill, uint32_t W, uint32_t H) {
	JmEmPlan p;
	const uint32_t ocw = (W + 15u) & ~15u, och = (H + 15u) & ~15u;
	p.n = n; p.fill = fill;
	p.disp_w[0] = W; p.disp_h[0] = H; p.disp_w[1] = (W + 1u) >> 1; p.disp_h[1] = (H + 1u) >> 1;
	p.out_w[0] = ocw; p.out_h[0] = och; p.out_w[1] = ocw >> 1; p.out_h[1] = och >> 1;
	for (int i = 0; i < 2; i++) {
		p.tiles_x[i] = (p.out_w[i] + JM_ES_TW - 1u) / JM_ES_TW; p.tiles_y[i] = (p.out_h[i] + JM_ES_TH - 1u) / JM_ES_TH;
	}
	p.out_luma = ocw * och; p.out_chroma = p.out_luma >> 2;
	p.tiles = p.tiles_x[0] * p.tiles_y[0] + 2u * p.tiles_x[1] * p.tiles_y[1];
	p.words = n * JM_EM_REC;
	for (uint32_t c = 0; c < n; c++) p.words += jm_es_plan(&cells[c].source, cells[c].width, cells[c].height).words;
	return p;
}

/* every tile holds a display column and a display row of its plane (TILES above) */
JM_ES_FN bool jm_em_tiles_ok(const JmEmPlan &p) {
	for (int i = 0; i < 2; i++)
		if ((p.tiles_x[i] - 1u) * JM_ES_TW >= p.disp_w[i] || (p.tiles_y[i] - 1u) * JM_ES_TH >= p.disp_h[i] || (p.out_w[i] & 3u)) return false;
	return true;
}

/* The table of a plan, p.words 32-bit words */
JM_ES_FN void jm_em_table(const JmEmPlan &p, const jsmpeg_hip_enc_cell_t *cells, uint32_t *tab) {
	uint32_t at = p.n * JM_EM_REC;
	for (uint32_t c = 0; c < p.n; c++) {
		const JmEsPlan s = jm_es_plan(&cells[c].source, cells[c].width, cells[c].height);
		JmEmCellRec r;
		for (int i = 0; i < 2; i++) { r.pl[i] = s.pl[i]; r.pl[i].ent_x += at; r.pl[i].ent_y += at; }
		r.src_luma = s.src_luma; r.src_chroma = s.src_chroma; r.wts = at + s.wts;
		r.dx = cells[c].x; r.dy = cells[c].y;
		memcpy(tab + c * JM_EM_REC, &r, sizeof(r));
		jm_es_table(s, tab + at);
		at += s.words;
	}
}

/* where cell record r lies in plane kind i (0 luma, 1 chroma): x, y, width, height */
JM_ES_FN void jm_em_rect(const JmEmCellRec &r, int i, uint32_t out[4]) {
	out[0] = i ? r.dx >> 1 : r.dx; out[1] = i ? r.dy >> 1 : r.dy; out[2] = r.pl[i].ax.n_out; out[3] = r.pl[i].ay.n_out;
}
