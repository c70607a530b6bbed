/* TEST-ONLY simulator of the intra encoder's kernels (jsmpeg_amd/csrc/encode.hip): enc_block.h's device functions compiled by
 * g++ and driven macroblock by macroblock in the kernels' two-pass order -- measure every macroblock, scan the slices, the
 * pictures and the call, clear, write every macroblock at its offset -- so that tests/test_enc_sim.py holds the streams against
 * the reference decoder and against tests/enc_ref.py without a GPU. */
#include <stdint.h>
#include <string.h>

#include <vector>

#include "enc_block.h"

static const JmEncTables g_tables = jm_enc_make_tables();

extern "C" const uint32_t *sim_enc_coeff_table() { return &g_tables.coeff[0][0]; }
extern "C" const uint16_t *sim_enc_dc_table(int chroma) { return chroma ? g_tables.dc_chroma : g_tables.dc_luma; }

struct Planes { const uint8_t *y, *cr, *cb; };
static Planes mb_planes(const uint8_t *f, uint32_t cw, uint32_t ch, uint32_t row, uint32_t col) {
	const size_t luma = (size_t)cw * ch, coff = (size_t)row * 8u * (cw >> 1) + (size_t)col * 8u;
	return { f + (size_t)row * 16u * cw + (size_t)col * 16u, f + luma + coff, f + luma + (luma >> 2) + coff };
}

/* k_enc_rgb: count RGB pictures of w x h -> frames of the coded size */
extern "C" void sim_enc_rgb(const uint8_t *rgb, uint32_t layout, uint32_t order, uint32_t w, uint32_t h, uint32_t count, uint8_t *frames) {
	const uint32_t cw = (w + 15u) & ~15u, ch = (h + 15u) & ~15u;
	for (uint32_t k = 0; k < count; k++)
		for (uint32_t cy = 0; cy < ch / 2; cy++)
			for (uint32_t cx = 0; cx < cw / 2; cx++)
				jm_enc_rgb_quad(rgb + (size_t)k * w * h * 3, layout, order, w, h, cx, cy, frames + (size_t)k * cw * ch * 3 / 2, cw, ch);
}

/* the quantised levels of one frame: levels[mb][block][64] in scan order, [0] the DC level */
extern "C" void sim_enc_levels(const uint8_t *frame, uint32_t w, uint32_t h, uint32_t q, int16_t *levels) {
	const uint32_t mbw = (w + 15u) >> 4, mbh = (h + 15u) >> 4, cw = mbw * 16, ch = mbh * 16;
	for (uint32_t m = 0; m < mbw * mbh; m++) {
		const Planes p = mb_planes(frame, cw, ch, m / mbw, m % mbw);
		for (int b = 0; b < 6; b++) {
			uint32_t stride;
			const uint8_t *px = jm_enc_block_px(p.y, p.cr, p.cb, cw, b, &stride);
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
	const uint32_t mbw = (w + 15u) >> 4, mbh = (h + 15u) >> 4, cw = mbw * 16, ch = mbh * 16, mbs = mbw * mbh;
	const size_t fb = (size_t)cw * ch * 3 / 2;
	std::vector<JmEncMb> mb((size_t)count * mbs);
	std::vector<uint32_t> slice((size_t)count * mbh);
	int16_t zz[64];
	/* k_enc_measure */
	for (size_t g = 0; g < mb.size(); g++) {
		const uint32_t k = (uint32_t)(g / mbs), m = (uint32_t)(g % mbs);
		const Planes p = mb_planes(frames + k * fb, cw, ch, m / mbw, m % mbw);
		uint64_t dcs;
		mb[g].bits = jm_enc_measure(p.y, p.cr, p.cb, cw, q[k], &g_tables, zz, 1, &dcs);
		mb[g].dc[0] = (uint32_t)dcs; mb[g].dc[1] = (uint32_t)(dcs >> 32);
	}
	/* k_enc_scan_slices, k_enc_scan_pictures, k_enc_place */
	for (size_t s = 0; s < slice.size(); s++) slice[s] = jm_enc_scan_slice(&mb[s * mbw], mbw, &g_tables);
	for (uint32_t k = 0; k < count; k++) pic_bytes[k] = jm_enc_scan_picture(&slice[(size_t)k * mbh], mbh);
	for (uint32_t s = 0; s < max_streams; s++) stream_begin[s] = stream_end[s] = 0;
	JmEncPlace place = jm_enc_place_begin();
	for (uint32_t k = 0; k < count; k++) pic_off[k] = jm_enc_place_picture(place, stream ? stream[k] : 0, pic_bytes[k], end != 0, stream_begin, stream_end);
	jm_enc_place_close(place, end != 0, stream_end);
	const uint64_t total = place.at;
	if (total > cap) return -1;
	/* k_enc_clear */
	memset(out, 0, total);
	memset(out + total, 0xff, JM_ENC_TAIL);
	/* k_enc_write */
	uint32_t *words = reinterpret_cast<uint32_t *>(out);
	for (size_t g = 0; g < mb.size(); g++) {
		const uint32_t k = (uint32_t)(g / mbs), m = (uint32_t)(g % mbs), row = m / mbw, col = m % mbw;
		const Planes p = mb_planes(frames + k * fb, cw, ch, row, col);
		const uint64_t slice_at = pic_off[k] + slice[(size_t)k * mbh + row];
		const uint32_t s = stream ? stream[k] : 0;
		if (col == 0) {
			jm_enc_put_slice_header(words, slice_at, row, q[k]);
			if (row == 0) {
				uint32_t ordinal = 0;
				for (uint32_t j = k; j > 0 && (stream ? stream[j - 1] : 0) == s; j--) ordinal++;
				jm_enc_put_picture_headers(words, pic_off[k], w, h, frame_rate_code, ordinal);
				if (k + 1 == count || (stream && stream[k + 1] != s)) jm_enc_put_stream_tail(words, pic_off[k] + pic_bytes[k], end != 0);
				if (k == 0) memset(out, 0xff, JM_ENC_LEAD_GAP);
			}
		}
		const uint32_t pred = col ? jm_enc_pred_of(jm_enc_mb_dcs(mb[g - 1])) : JM_ENC_PRED0;
		JmEncBits bw = jm_enc_bits_at(words, slice_at * 8u + mb[g].bits);
		jm_enc_write(p.y, p.cr, p.cb, cw, q[k], &g_tables, zz, 1, pred, bw);
		jm_enc_flush(bw);
	}
	return (int64_t)total;
}
