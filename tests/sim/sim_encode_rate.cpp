/* TEST-ONLY simulator of the encoder's pass with rate control (jsmpeg_amd/csrc/encode.hip with jsmpeg_hip_encoder_set_rate):
 * enc_rate.h's device functions compiled by g++ and driven in the kernels' order -- level by level the search, then per picture
 * k_enc_rate_measure (every macroblock at every scale), k_enc_rate_scan (every slice at every scale), k_enc_rate_pick (the
 * budget from the final bytes of the GOP's earlier levels, the smallest scale that fits) and the measure with its reconstruction
 * at the chosen scale.  The rest of the pass reads nothing but the chosen scales: it is sim_encode_p, called with them. */
#include "sim_encode_p.cpp"      /* sim_motion, the tables, sim_encode_p */
#include "enc_rate.h"

/* sim_encode_p's arguments with the rule's four values (T > 0) in place of the scales; chosen, budget, bytes: count each, out */
extern "C" int64_t sim_encode_rate(const uint8_t *frames, uint32_t w, uint32_t h, uint32_t count, const uint32_t *stream,
                                   uint32_t frame_rate_code, uint32_t end, uint32_t max_streams, uint32_t gop, uint32_t R,
                                   uint32_t T, uint32_t q_min, uint32_t q_max, uint32_t W, uint8_t *out, uint64_t cap,
                                   uint64_t *pic_off, uint32_t *pic_bytes, uint64_t *stream_begin, uint64_t *stream_end,
                                   uint8_t *recon, uint32_t *info, uint32_t *stats, uint8_t *chosen, uint64_t *budget, uint32_t *bytes) {
	const uint32_t mbw = (w + 15u) >> 4, mbh = (h + 15u) >> 4, cw = mbw * 16, ch = mbh * 16, mbs = mbw * mbh, nq = q_max - q_min + 1u;
	const size_t fb = (size_t)cw * ch * 3 / 2;
	const uint32_t r_size = jm_encp_r_size(R);
	std::vector<JmEncPMb> mb(mbs);
	std::vector<uint16_t> rec((size_t)mbs * JM_ENCR_MAX_Q);
	std::vector<uint32_t> ordinal(count), m(count);
	int16_t zz[64];
	uint32_t pp[16], acc[JM_ENCR_MAX_Q];
	uint32_t levels = 0;
	for (uint32_t k = 0; k < count; k++) {
		ordinal[k] = (k && (stream ? stream[k] == stream[k - 1] : true)) ? ordinal[k - 1] + 1 : 0;
		levels = std::max(levels, ordinal[k] % gop + 1);
	}
	for (uint32_t k = count, len = 0; k-- > 0;) {
		if (k + 1 == count || (stream && stream[k + 1] != stream[k])) len = ordinal[k] + 1;
		m[k] = std::min(gop, len - (ordinal[k] - ordinal[k] % gop));
	}
	for (uint32_t l = 0; l < levels; l++)
		for (uint32_t k = 0; k < count; k++) {
			if (ordinal[k] % gop != l) continue;
			const uint8_t *f = frames + k * fb;
			uint8_t *rc = recon + k * fb;
			/* k_enc_motion, k_enc_rate_measure */
			for (uint32_t i = 0; i < mbs; i++) {
				const uint32_t row = i / mbw, col = i % mbw;
				mb[i] = JmEncPMb();
				mb[i].info = l ? sim_motion(f, rc - fb, cw, ch, col, row, R) : 0u;
				for (uint32_t j = 0; j < JM_ENCR_MAX_Q; j++) rec[(size_t)i * JM_ENCR_MAX_Q + j] = 0xffffu;      /* what the range does not cover is never read */
				uint64_t dcs;
				if (jm_encr_measure(f, rc - fb, cw, ch, mbw, col, row, mb[i].info, q_min, nq, &g_tables, &g_ptables, zz, 1, pp, 1, acc, 1,
				                    &rec[(size_t)i * JM_ENCR_MAX_Q], &dcs)) {
					mb[i].dc[0] = (uint32_t)dcs; mb[i].dc[1] = (uint32_t)(dcs >> 32);
				}
			}
			/* k_enc_rate_scan, k_enc_rate_pick */
			uint64_t spent = 0;
			for (uint32_t j = 1; j <= l; j++) spent += bytes[k - j];
			budget[k] = jm_encr_budget(T, m[k], l, W, spent);
			uint32_t size[JM_ENCR_MAX_Q], fit = nq - 1u;
			for (uint32_t qi = 0; qi < nq; qi++) {
				size[qi] = l ? JM_ENC_P_HEAD_BYTES : JM_ENC_PIC_HEAD_BYTES;
				for (uint32_t row = 0; row < mbh; row++)
					size[qi] += jm_encr_scan(&rec[(size_t)row * mbw * JM_ENCR_MAX_Q], &mb[(size_t)row * mbw], qi, mbw, l != 0, r_size, &g_tables, &g_ptables);
			}
			for (uint32_t qi = nq; qi-- > 0;) if (size[qi] <= budget[k]) fit = qi;
			chosen[k] = (uint8_t)(q_min + fit); bytes[k] = size[fit];
			/* k_enc_measure_p at the chosen scale: the reconstruction the next level searches */
			for (uint32_t i = 0; i < mbs; i++) {
				const uint32_t row = i / mbw, col = i % mbw, found = mb[i].info;
				uint32_t unused;
				uint64_t dcs;
				if (found & 1u)
					jm_encp_measure_inter(f, rc - fb, rc, cw, ch, mbw, col, row, jm_encp_mvh(found), jm_encp_mvv(found), chosen[k], &g_tables, &g_ptables, zz, 1, pp, 1, &unused);
				else jm_encp_measure_intra(f, rc, cw, ch, col, row, chosen[k], &g_tables, zz, 1, &dcs);
			}
		}
	return sim_encode_p(frames, w, h, count, stream, chosen, frame_rate_code, end, max_streams, gop, R, out, cap, pic_off, pic_bytes, stream_begin, stream_end,
	                    recon, info, stats);
}
