/* TEST-ONLY simulator of the encoder's GOP pass (jsmpeg_amd/csrc/encode.hip with jsmpeg_hip_encoder_set_gop, gop > 1):
 * enc_motion.h's device functions compiled by g++ and driven in the kernels' order -- level by level the search (item by item,
 * half-pel part by part, as the lanes of k_enc_motion take them) and the measure with its reconstruction, then the scans, place,
 * clear and the write of every macroblock at its offset -- so that tests/test_enc_p_sim.py holds the streams against the
 * reference decoder and against tests/enc_p_ref.py without a GPU. */
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "enc_motion.h"

static const JmEncTables g_tables = jm_enc_make_tables();
static const JmEncPTables g_ptables = jm_encp_make_tables();

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

/* jm_encp_quant_inter's division on its own: out[i] = mulhi(2 n[i], jm_encp_recip(q)), which stands in for n[i] / q */
extern "C" void sim_encp_recip_div(const uint32_t *n, uint32_t count, uint32_t q, uint32_t *out) {
	const uint32_t rq = jm_encp_recip(q);
	for (uint32_t i = 0; i < count; i++) out[i] = jm_enc_mulhi(2u * n[i], rq);
}

/* One call of the encoder with gop > 1: sim_encode's arguments, then gop and search_range; recon: count frames out (16 bytes
 * of slack behind them), info: count * macroblocks records' info words out, stats: count * 4.  Returns the total bytes or -1. */
extern "C" int64_t sim_encode_p(const uint8_t *frames, uint32_t w, uint32_t h, uint32_t count, const uint32_t *stream, const uint8_t *q,
                                uint32_t frame_rate_code, uint32_t end, uint32_t max_streams, uint32_t gop, uint32_t R, uint8_t *out, uint64_t cap,
                                uint64_t *pic_off, uint32_t *pic_bytes, uint64_t *stream_begin, uint64_t *stream_end,
                                uint8_t *recon, uint32_t *info, uint32_t *stats) {
	const uint32_t mbw = (w + 15u) >> 4, mbh = (h + 15u) >> 4, cw = mbw * 16, ch = mbh * 16, mbs = mbw * mbh;
	const size_t fb = (size_t)cw * ch * 3 / 2;
	const uint32_t r_size = jm_encp_r_size(R);
	std::vector<JmEncPMb> mb((size_t)count * mbs);
	std::vector<uint32_t> slice((size_t)count * mbh), ordinal(count), kinds((size_t)count * mbh * 4, 0);
	int16_t zz[64];
	uint32_t pp[16];
	uint32_t levels = 0;
	for (uint32_t k = 0; k < count; k++) {
		ordinal[k] = (k && (stream ? stream[k] == stream[k - 1] : true)) ? ordinal[k - 1] + 1 : 0;
		levels = std::max(levels, ordinal[k] % gop + 1);
	}
	/* the level loop: k_enc_motion, k_enc_measure_p */
	for (uint32_t l = 0; l < levels; l++)
		for (uint32_t k = 0; k < count; k++) {
			if (ordinal[k] % gop != l) continue;
			const uint8_t *f = frames + k * fb;
			uint8_t *rc = recon + k * fb;
			for (uint32_t m = 0; m < mbs; m++) {
				const uint32_t row = m / mbw, col = m % mbw;
				JmEncPMb &rec = mb[(size_t)k * mbs + m];
				rec = JmEncPMb();
				const uint32_t found = l ? sim_motion(f, rc - fb, cw, ch, col, row, R) : 0u;
				if (found & 1u)
					rec.bits = jm_encp_measure_inter(f, rc - fb, rc, cw, ch, mbw, col, row, jm_encp_mvh(found), jm_encp_mvv(found), q[k], &g_tables, &g_ptables,
					                                 zz, 1, pp, 1, &rec.info);
				else {
					uint64_t dcs;
					rec.bits = jm_encp_measure_intra(f, rc, cw, ch, col, row, q[k], &g_tables, zz, 1, &dcs);
					rec.dc[0] = (uint32_t)dcs; rec.dc[1] = (uint32_t)(dcs >> 32);
					rec.info = jm_encp_info(JM_ENCP_INTRA, false, 0, 0, 0);
				}
				info[(size_t)k * mbs + m] = rec.info;
			}
		}
	/* k_enc_scan_slices_p, k_enc_scan_pictures_p, k_enc_place */
	for (size_t s = 0; s < slice.size(); s++)
		slice[s] = jm_encp_scan_slice(&mb[s * mbw], mbw, ordinal[s / mbh] % gop != 0, r_size, &g_tables, &g_ptables, &kinds[s * 4]);
	for (uint32_t k = 0; k < count; k++) {
		pic_bytes[k] = jm_encp_scan_picture(&slice[(size_t)k * mbh], mbh, ordinal[k] % gop ? JM_ENC_P_HEAD_BYTES : JM_ENC_PIC_HEAD_BYTES);
		for (uint32_t i = 0; i < 4; i++) {
			stats[k * 4 + i] = 0;
			for (uint32_t r = 0; r < mbh; r++) stats[k * 4 + i] += kinds[((size_t)k * mbh + r) * 4 + i];
		}
	}
	for (uint32_t s = 0; s < max_streams; s++) stream_begin[s] = stream_end[s] = 0;
	JmEncPlace place = jm_enc_place_begin();
	for (uint32_t k = 0; k < count; k++) pic_off[k] = jm_enc_place_picture(place, stream ? stream[k] : 0, pic_bytes[k], end != 0, stream_begin, stream_end);
	jm_enc_place_close(place, end != 0, stream_end);
	const uint64_t total = place.at;
	if (total > cap) return -1;
	/* k_enc_clear */
	memset(out, 0, total);
	memset(out + total, 0xff, JM_ENC_TAIL);
	/* k_enc_write_p */
	uint32_t *words = reinterpret_cast<uint32_t *>(out);
	for (size_t g = 0; g < mb.size(); g++) {
		const uint32_t k = (uint32_t)(g / mbs), m = (uint32_t)(g % mbs), row = m / mbw, col = m % mbw;
		const bool p_picture = ordinal[k] % gop != 0;
		const uint64_t slice_at = pic_off[k] + slice[(size_t)k * mbh + row];
		const uint32_t s = stream ? stream[k] : 0;
		if (col == 0) {
			jm_enc_put_slice_header(words, slice_at, row, q[k]);
			if (row == 0) {
				if (p_picture) jm_encp_put_picture_header(words, pic_off[k], ordinal[k] % gop, r_size);
				else jm_enc_put_picture_headers(words, pic_off[k], w, h, frame_rate_code, ordinal[k]);
				if (k + 1 == count || (stream && stream[k + 1] != s)) jm_enc_put_stream_tail(words, pic_off[k] + pic_bytes[k], end != 0);
				if (k == 0) memset(out, 0xff, JM_ENC_LEAD_GAP);
			}
		}
		JmEncBits bw = jm_enc_bits_at(words, slice_at * 8u + mb[g].bits);
		jm_encp_write(mb[g], frames + k * fb, recon + (p_picture ? k - 1 : k) * fb, cw, ch, col, row, p_picture, r_size, q[k], &g_tables, &g_ptables,
		              zz, 1, pp, 1, bw);
		jm_enc_flush(bw);
	}
	return (int64_t)total;
}
