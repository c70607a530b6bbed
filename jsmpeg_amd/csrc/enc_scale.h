/*
 * Scaled and cropped YCbCr input of the encoder (include/jsmpeg_hip.h part 8, jsmpeg_hip_encoder_encode_scaled): what
 * k_enc_scale (encode.hip), the CPU simulator (tests/sim/sim_encode_scale.cpp) and the host side of the call share -- the
 * descriptor check, the per-axis taps with their integer weights, and the table and tile plan of a launch.  Host + device.
 * tests/enc_scale_ref.py restates every formula in numpy.
 *
 * SOURCE    a frame Y | Cr | Cb of the source's coded size (display size rounded up to 16s: a pool slot of a Batch or Live
 *           of that size), a crop (crop_x, crop_y, crop_width, crop_height) in display pixels, x / y even.
 * PLANES    scaled independently, the same half-pixel-centre mapping on each (MPEG-1's chroma is centred in its 2x2 luma):
 *             luma    crop_width x crop_height at (crop_x, crop_y) -> W x H, the encoder's display size
 *             chroma  ((crop_width + 1) >> 1) x ((crop_height + 1) >> 1) at (crop_x >> 1, crop_y >> 1)
 *                     -> ((W + 1) >> 1) x ((H + 1) >> 1)
 *           no tap reaches outside the crop.
 * TAPS      of one axis, n_in -> n_out, output index i: torch's bilinear, align_corners=False filter shapes as integer ratios.
 *             n_in == n_out                 one tap i
 *             antialias and n_in > n_out    c = (2i + 1) n_in; n_j = 2 n_in - |(2j + 1) n_out - c|; the j with n_j > 0
 *                                           (one contiguous run: the triangle filter widened by the scale)
 *             otherwise                     num = max(0, (2i + 1) n_in - n_out), i0 = num div 2 n_out, r = num mod 2 n_out:
 *                                           i0 >= n_in - 1: the single tap n_in - 1; r == 0: the single tap i0;
 *                                           else tap i0 with n = 2 n_out - r and tap i0 + 1 with n = r
 *           weights: N = sum n_j, W_j = (2 * 16384 n_j + N) div 2N, and the first tap of the largest W takes 16384 - sum W.
 *           An output index where that tap would go below 0 -- the roundings of very many small weights add up to more than
 *           the largest: only antialiased n_out = 1 with n_in from 1280 and n_out = 2 with n_in from 2870, within 1 .. 4095 --
 *           takes cumulative rounding instead: C_j = n_0 + .. + n_(j-1), R(c) = (2 * 16384 c + N) div 2N in 64 bits,
 *           W_j = R(C_(j+1)) - R(C_j), no remainder tap.  Either way every weight is 0 .. 16384 and they sum to exactly 16384.
 * VALUE     horizontal pass, then vertical:  t = (sum_j Wx_j p[x0 + j] + 32) >> 6   (<= 65280)
 *                                            out = (sum_k Wy_k t[y0 + k] + 2^21) >> 22   (0 .. 255 without a clamp)
 *           everything fits 32 bits.
 * CODED     the encoder's frame is the scaled picture extended by edge replication: output (x, y) of a plane of pw x ph
 *           scaled samples is the scaled sample (min(x, pw - 1), min(y, ph - 1)).
 */
#pragma once
#include <stdint.h>

#include "jsmpeg_hip.h"

#if defined(__HIPCC__)
#define JM_ES_FN __host__ __device__ inline
#else
#define JM_ES_FN static inline
#endif

#define JM_ES_ONE 16384u         /* the weights of an output sample sum to this */
#define JM_ES_MAX_SIDE 4095u

/* the tiles of k_enc_scale: output columns x rows of one plane, the source rows of a chunk, the staging bytes */
#define JM_ES_TW 128u
#define JM_ES_TH 32u
#define JM_ES_CR 32u
#define JM_ES_SRC 16384u

struct JmEsAxis { uint32_t n_in, n_out, aa; };

/* output index i's taps: source indices xmin .. xmin + xsize - 1 of the crop; the rest is what jm_es_weight needs */
struct JmEsTaps {
	uint32_t xmin, xsize;
	uint32_t N;                  /* sum of the n_j */
	uint32_t p;                  /* antialiased: the centre c; two plain taps: r */
	uint32_t fix_j, fix;         /* the tap that takes the remainder, and the remainder */
	uint32_t cum;                /* 1: that tap would go below 0, the weights are the cumulative roundings instead */
};

JM_ES_FN uint32_t jm_es_n(const JmEsAxis &a, const JmEsTaps &t, uint32_t j) {
	if (t.xsize == 1) return 1u;
	if (a.aa && a.n_in > a.n_out) {
		const int32_t d = (int32_t)((2u * (t.xmin + j) + 1u) * a.n_out) - (int32_t)t.p;
		return 2u * a.n_in - (uint32_t)(d < 0 ? -d : d);
	}
	return j == 0 ? 2u * a.n_out - t.p : t.p;
}

JM_ES_FN uint32_t jm_es_weight_raw(const JmEsTaps &t, uint32_t n) { return (2u * JM_ES_ONE * n + t.N) / (2u * t.N); }

/* C_j = n_0 + .. + n_(j-1) (0 <= j <= t.xsize) without a loop: the antialiased n_k = 2 n_in - |d_0 + 2 n_out k| is linear on
 * either side of the centre, the first m of the k < j lie below it */
JM_ES_FN uint64_t jm_es_cum(const JmEsAxis &a, const JmEsTaps &t, uint32_t j) {
	if (!(a.aa && a.n_in > a.n_out)) return j == 0 ? 0u : j == 1 ? jm_es_n(a, t, 0) : t.N;
	const int64_t d0 = (int64_t)(2u * t.xmin + 1u) * a.n_out - (int64_t)t.p, s = 2 * (int64_t)a.n_out;
	int64_t m = d0 < 0 ? (-d0 + s - 1) / s : 0;
	if (m > (int64_t)j) m = j;
	const int64_t tri_m = m * (m - 1) / 2, tri_j = (int64_t)j * ((int64_t)j - 1) / 2;
	const int64_t below = -(d0 * m + s * tri_m), above = d0 * ((int64_t)j - m) + s * (tri_j - tri_m);
	return (uint64_t)(2 * (int64_t)a.n_in * j - below - above);
}

JM_ES_FN uint32_t jm_es_round_cum(const JmEsTaps &t, uint64_t c) { return (uint32_t)((2u * (uint64_t)JM_ES_ONE * c + t.N) / (2u * (uint64_t)t.N)); }

JM_ES_FN JmEsTaps jm_es_taps(const JmEsAxis &a, uint32_t i) {
	JmEsTaps t;
	t.N = 1; t.p = 0; t.fix_j = 0; t.fix = 0; t.cum = 0;
	if (a.n_in == a.n_out) { t.xmin = i; t.xsize = 1; return t; }
	if (a.aa && a.n_in > a.n_out) {
		const uint32_t c = (2u * i + 1u) * a.n_in, lo = c - 2u * a.n_in, hi = c + 2u * a.n_in;    /* (lo as a signed number: i = 0 gives -n_in) */
		const uint32_t first = (i == 0 || lo < a.n_out) ? 0u : (lo - a.n_out) / (2u * a.n_out) + 1u;
		uint32_t last = (hi - a.n_out - 1u) / (2u * a.n_out);
		if (last > a.n_in - 1u) last = a.n_in - 1u;
		t.xmin = first; t.xsize = last - first + 1u; t.p = c;
		if (t.xsize == 1) return t;
	} else {
		const uint32_t c = (2u * i + 1u) * a.n_in, num = c > a.n_out ? c - a.n_out : 0u;
		const uint32_t i0 = num / (2u * a.n_out), r = num % (2u * a.n_out);
		if (i0 >= a.n_in - 1u) { t.xmin = a.n_in - 1u; t.xsize = 1; return t; }
		t.xmin = i0;
		if (r == 0) { t.xsize = 1; return t; }
		t.xsize = 2; t.p = r;
	}
	t.N = 0;
	for (uint32_t j = 0; j < t.xsize; j++) t.N += jm_es_n(a, t, j);
	uint32_t sum = 0, best = 0;
	for (uint32_t j = 0; j < t.xsize; j++) {
		const uint32_t w = jm_es_weight_raw(t, jm_es_n(a, t, j));
		sum += w;
		if (w > best) { best = w; t.fix_j = j; }
	}
	t.fix = JM_ES_ONE - sum;         /* (mod 2^32: the sum may exceed 16384 by the roundings) */
	t.cum = sum > JM_ES_ONE + best ? 1u : 0u;
	return t;
}

/* weight of tap j (0 <= j < t.xsize): 0 .. JM_ES_ONE */
JM_ES_FN uint32_t jm_es_weight(const JmEsAxis &a, const JmEsTaps &t, uint32_t j) {
	if (t.xsize == 1) return JM_ES_ONE;
	if (t.cum) return jm_es_round_cum(t, jm_es_cum(a, t, j + 1u)) - jm_es_round_cum(t, jm_es_cum(a, t, j));
	return jm_es_weight_raw(t, jm_es_n(a, t, j)) + (j == t.fix_j ? t.fix : 0u);
}

/* The descriptor check: 0, or a message (static text) of what the contract does not cover. */
JM_ES_FN const char *jm_es_check(const jsmpeg_hip_enc_source_t *s) {
	if (!s) return "null source descriptor";
	if (s->width < 1 || s->width > JM_ES_MAX_SIDE || s->height < 1 || s->height > JM_ES_MAX_SIDE)
		return "source width and height must be 1 .. 4095";
	if (s->antialias > 1) return "antialias must be 0 or 1";
	const bool whole = s->crop_width == 0 && s->crop_height == 0;
	if (whole ? (s->crop_x || s->crop_y)
	          : (s->crop_width == 0 || s->crop_height == 0 || (uint64_t)s->crop_x + s->crop_width > s->width ||
	             (uint64_t)s->crop_y + s->crop_height > s->height))
		return "crop rectangle outside the picture";
	if ((s->crop_x | s->crop_y) & 1u) return "crop_x and crop_y must be even (the chroma samples would be sited half a sample off)";
	return 0;
}

/* One plane kind of a launch: 0 luma, 1 chroma (Cr and Cb alike) */
struct JmEsPlane {
	JmEsAxis ax, ay;
	uint32_t x0, y0;             /* the crop's origin in the source plane */
	uint32_t src_w;              /* the source plane's coded width = its row stride */
	uint32_t out_w, out_h;       /* the plane of the encoder's coded size */
	uint32_t tiles_x, tiles_y;
	uint32_t ent_x, ent_y;       /* where the axes' entries begin in the table, in 32-bit words */
};

/* What a launch needs besides the frames, worked out on the host from a checked descriptor and the encoder's display size */
struct JmEsPlan {
	JmEsPlane pl[2];
	uint32_t src_luma, src_chroma;   /* bytes of a source plane */
	uint32_t out_luma, out_chroma;
	uint32_t tiles;                  /* of one picture: luma, Cr, Cb */
	uint32_t wts;                    /* where the weights (16 bits each) begin in the table, in 32-bit words */
	uint32_t words;                  /* the table's size */
};

JM_ES_FN JmEsPlan jm_es_plan(const jsmpeg_hip_enc_source_t *s, uint32_t W, uint32_t H) {
	JmEsPlan p;
	const bool whole = s->crop_width == 0 && s->crop_height == 0;
	const uint32_t cx = whole ? 0 : s->crop_x, cy = whole ? 0 : s->crop_y;
	const uint32_t cw = whole ? s->width : s->crop_width, ch = whole ? s->height : s->crop_height;
	const uint32_t scw = (s->width + 15u) & ~15u, sch = (s->height + 15u) & ~15u, ocw = (W + 15u) & ~15u, och = (H + 15u) & ~15u;
	JmEsPlane &l = p.pl[0], &c = p.pl[1];
	l.ax = JmEsAxis{ cw, W, s->antialias }; l.ay = JmEsAxis{ ch, H, s->antialias };
	l.x0 = cx; l.y0 = cy; l.src_w = scw; l.out_w = ocw; l.out_h = och;
	c.ax = JmEsAxis{ (cw + 1u) >> 1, (W + 1u) >> 1, s->antialias }; c.ay = JmEsAxis{ (ch + 1u) >> 1, (H + 1u) >> 1, s->antialias };
	c.x0 = cx >> 1; c.y0 = cy >> 1; c.src_w = scw >> 1; c.out_w = ocw >> 1; c.out_h = och >> 1;
	p.src_luma = scw * sch; p.src_chroma = p.src_luma >> 2;
	p.out_luma = ocw * och; p.out_chroma = p.out_luma >> 2;
	uint32_t at = 0;
	for (int i = 0; i < 2; i++) {
		JmEsPlane &q = p.pl[i];
		q.tiles_x = (q.out_w + JM_ES_TW - 1u) / JM_ES_TW; q.tiles_y = (q.out_h + JM_ES_TH - 1u) / JM_ES_TH;
		q.ent_x = at; at += 2u * q.ax.n_out;
		q.ent_y = at; at += 2u * q.ay.n_out;
	}
	p.tiles = l.tiles_x * l.tiles_y + 2u * c.tiles_x * c.tiles_y;
	p.wts = at;
	uint32_t taps = 0;
	for (int i = 0; i < 2; i++)
		for (int v = 0; v < 2; v++) {
			const JmEsAxis &a = v ? p.pl[i].ay : p.pl[i].ax;
			for (uint32_t o = 0; o < a.n_out; o++) taps += jm_es_taps(a, o).xsize;
		}
	p.words = at + ((taps + 1u) >> 1);
	return p;
}

/* the most 32-bit words a table takes for an encoder of W x H, whatever the source: an output sample has at most
 * 2 n_in / n_out + 1 taps (the odd numbers of an open interval 4 n_in / n_out long), or two */
JM_ES_FN uint32_t jm_es_table_bound(uint32_t W, uint32_t H) {
	const uint32_t cw = (W + 1u) >> 1, ch = (H + 1u) >> 1, in_l = JM_ES_MAX_SIDE, in_c = (JM_ES_MAX_SIDE + 1u) >> 1;
	const uint32_t taps = 2u * (2u * in_l + 2u * in_c) + 2u * (W + H + cw + ch);
	return 2u * (W + H + cw + ch) + ((taps + 1u) >> 1);
}

/* The table of a plan, p.words 32-bit words: per axis and output index two words, xmin | xsize << 16 and the index of its
 * first weight; then the weights */
JM_ES_FN void jm_es_table(const JmEsPlan &p, uint32_t *tab) {
	uint16_t *w = reinterpret_cast<uint16_t *>(tab + p.wts);
	uint32_t at = 0;
	for (int i = 0; i < 2; i++)
		for (int v = 0; v < 2; v++) {
			const JmEsAxis &a = v ? p.pl[i].ay : p.pl[i].ax;
			uint32_t *ent = tab + (v ? p.pl[i].ent_y : p.pl[i].ent_x);
			for (uint32_t o = 0; o < a.n_out; o++) {
				const JmEsTaps t = jm_es_taps(a, o);
				ent[2u * o] = t.xmin | (t.xsize << 16);
				ent[2u * o + 1u] = at;
				for (uint32_t j = 0; j < t.xsize; j++) w[at++] = (uint16_t)jm_es_weight(a, t, j);
			}
		}
	if (at & 1u) w[at] = 0;
}

/* the two passes' roundings */
JM_ES_FN uint32_t jm_es_round_h(uint32_t sum) { return (sum + 32u) >> 6; }
JM_ES_FN uint32_t jm_es_round_v(uint32_t sum) { return (sum + (1u << 21)) >> 22; }
