/* TEST-ONLY simulator of the encoder's calls with JSMPEG_HIP_ENC_CHAIN (jsmpeg_amd/csrc/encode.hip; the rule: enc_chain.h): a
 * handle with the host's chain records, the carry frames and the GOPs' spent bytes, and calls one after another, chained or not.
 * A call drives enc_chain.h's plan and the device functions of enc_motion.h / enc_rate.h in the kernels' order with every
 * picture's reference and reconstruction where the plan puts them -- level by level the search, with rate control the measure
 * at every scale, the scan and the pick (the bytes earlier calls left included), the measure with its reconstruction; then the
 * scans, place, clear and the write.  tests/test_enc_chain_sim.py holds its calls against ONE call of sim_encode_p /
 * sim_encode_rate over the same pictures.  gop 1 without rate control is not the level loop and is refused here (-2). */
#include "sim_encode_rate.cpp"   /* sim_motion, the tables */
#include "enc_chain.h"

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
 * device's pass is settled), -2 for what this simulator does not cover. */
extern "C" int64_t sim_chain_encode(SimChain *c, const uint8_t *frames, uint32_t count, const uint32_t *stream, uint8_t *q, uint32_t flags,
                                    uint8_t *out, uint64_t cap, uint64_t *pic_off, uint32_t *pic_bytes, uint64_t *stream_begin, uint64_t *stream_end,
                                    uint8_t *recon_out, uint32_t *info, uint32_t *stats, uint32_t *ordinal, uint64_t *budget, uint32_t *bytes) {
	const uint32_t w = c->w, h = c->h, gop = c->gop, R = c->R;
	const uint32_t mbw = (w + 15u) >> 4, mbh = (h + 15u) >> 4, cw = mbw * 16, ch = mbh * 16, mbs = mbw * mbh, nq = c->q_max - c->q_min + 1u;
	const size_t fb = c->fb;
	const uint32_t r_size = jm_encp_r_size(R);
	const bool chained = (flags & 2u) != 0, end = (flags & 1u) != 0, rate = c->T != 0;
	if (gop == 1 && !rate) return -2;
	if (flags & ~3u) return -2;
	std::vector<JmEncPlan> plan(count);
	std::vector<uint8_t> store((size_t)count * fb + 16, 0x5a);
	std::vector<uint8_t *> ref(count), rec(count);
	for (uint32_t k0 = 0; k0 < count;) {
		const uint32_t s = stream ? stream[k0] : 0;
		uint32_t n = 1;
		while (k0 + n < count && (!stream || stream[k0 + n] == s)) n++;
		jm_encc_plan(chained ? &c->chain[s] : nullptr, s, rate, gop, k0, n, &plan[k0]);
		if (chained) jm_encc_advance(c->chain[s], plan[k0 + n - 1], rate, end, gop);
		k0 += n;
	}
	uint32_t levels = 0;
	for (uint32_t k = 0; k < count; k++) {
		const uint32_t at[2] = { plan[k].ref, plan[k].recon };
		uint8_t *where[2];
		for (int i = 0; i < 2; i++) where[i] = (at[i] & JM_ENCC_SLOT) ? &c->carry[(size_t)(at[i] & ~JM_ENCC_SLOT) * fb] : &store[(size_t)at[i] * fb];
		ref[k] = where[0]; rec[k] = where[1];
		ordinal[k] = plan[k].ordinal;
		levels = std::max(levels, plan[k].ordinal % gop + 1);
	}
	std::vector<JmEncPMb> mb((size_t)count * mbs);
	std::vector<uint16_t> rr((size_t)mbs * JM_ENCR_MAX_Q);
	std::vector<uint32_t> slice((size_t)count * mbh), kinds((size_t)count * mbh * 4, 0);
	int16_t zz[64];
	uint32_t pp[16], acc[JM_ENCR_MAX_Q];
	/* the level loop: k_enc_motion, k_enc_rate_measure, k_enc_rate_scan, k_enc_rate_pick, k_enc_measure_p */
	for (uint32_t l = 0; l < levels; l++)
		for (uint32_t k = 0; k < count; k++) {
			if (plan[k].ordinal % gop != l) continue;
			const uint8_t *f = frames + k * fb;
			const uint32_t s = stream ? stream[k] : 0;
			JmEncPMb *pm = &mb[(size_t)k * mbs];
			for (uint32_t i = 0; i < mbs; i++) {
				pm[i] = JmEncPMb();
				pm[i].info = l ? sim_motion(f, ref[k], cw, ch, i % mbw, i / mbw, R) : 0u;
			}
			if (rate) {
				for (uint32_t i = 0; i < mbs; i++) {
					for (uint32_t j = 0; j < JM_ENCR_MAX_Q; j++) rr[(size_t)i * JM_ENCR_MAX_Q + j] = 0xffffu;
					uint64_t dcs;
					if (jm_encr_measure(f, ref[k], cw, ch, mbw, i % mbw, i / mbw, pm[i].info, c->q_min, nq, &g_tables, &g_ptables, zz, 1, pp, 1, acc, 1,
					                    &rr[(size_t)i * JM_ENCR_MAX_Q], &dcs)) {
						pm[i].dc[0] = (uint32_t)dcs; pm[i].dc[1] = (uint32_t)(dcs >> 32);
					}
				}
				uint64_t spent = 0;
				for (uint32_t j = 1; j <= plan[k].before; j++) spent += bytes[k - j];
				const uint32_t odd = (plan[k].carry & JM_ENCC_ODD) ? 1u : 0u;
				if (plan[k].carry & JM_ENCC_READ) spent += c->spent[(size_t)odd * c->max_streams + s];
				budget[k] = jm_encr_budget(c->T, plan[k].m, l, c->W, spent);
				uint32_t size[JM_ENCR_MAX_Q], fit = nq - 1u;
				for (uint32_t qi = 0; qi < nq; qi++) {
					size[qi] = l ? JM_ENC_P_HEAD_BYTES : JM_ENC_PIC_HEAD_BYTES;
					for (uint32_t row = 0; row < mbh; row++)
						size[qi] += jm_encr_scan(&rr[(size_t)row * mbw * JM_ENCR_MAX_Q], &pm[(size_t)row * mbw], qi, mbw, l != 0, r_size, &g_tables, &g_ptables);
				}
				for (uint32_t qi = nq; qi-- > 0;) if (size[qi] <= budget[k]) fit = qi;
				q[k] = (uint8_t)(c->q_min + fit); bytes[k] = size[fit];
				if (plan[k].carry & JM_ENCC_WRITE) c->spent[(size_t)(odd ^ 1u) * c->max_streams + s] = spent + size[fit];
			}
			for (uint32_t i = 0; i < mbs; i++) {
				const uint32_t row = i / mbw, col = i % mbw, found = pm[i].info;
				JmEncPMb m = JmEncPMb();
				if (found & 1u)
					m.bits = jm_encp_measure_inter(f, ref[k], rec[k], cw, ch, mbw, col, row, jm_encp_mvh(found), jm_encp_mvv(found), q[k], &g_tables, &g_ptables,
					                               zz, 1, pp, 1, &m.info);
				else {
					uint64_t dcs;
					m.bits = jm_encp_measure_intra(f, rec[k], cw, ch, col, row, q[k], &g_tables, zz, 1, &dcs);
					m.dc[0] = (uint32_t)dcs; m.dc[1] = (uint32_t)(dcs >> 32);
					m.info = jm_encp_info(JM_ENCP_INTRA, false, 0, 0, 0);
				}
				pm[i] = m;
				info[(size_t)k * mbs + i] = m.info;
			}
		}
	/* k_enc_scan_slices_p, k_enc_scan_pictures_p, k_enc_place */
	for (size_t s = 0; s < slice.size(); s++)
		slice[s] = jm_encp_scan_slice(&mb[s * mbw], mbw, plan[s / mbh].ordinal % gop != 0, r_size, &g_tables, &g_ptables, &kinds[s * 4]);
	for (uint32_t k = 0; k < count; k++) {
		pic_bytes[k] = jm_encp_scan_picture(&slice[(size_t)k * mbh], mbh, plan[k].ordinal % gop ? JM_ENC_P_HEAD_BYTES : JM_ENC_PIC_HEAD_BYTES);
		for (uint32_t i = 0; i < 4; i++) {
			stats[k * 4 + i] = 0;
			for (uint32_t r = 0; r < mbh; r++) stats[k * 4 + i] += kinds[((size_t)k * mbh + r) * 4 + i];
		}
	}
	for (uint32_t s = 0; s < c->max_streams; s++) stream_begin[s] = stream_end[s] = 0;
	JmEncPlace place = jm_enc_place_begin();
	for (uint32_t k = 0; k < count; k++) pic_off[k] = jm_enc_place_picture(place, stream ? stream[k] : 0, pic_bytes[k], end, stream_begin, stream_end);
	jm_enc_place_close(place, end, stream_end);
	const uint64_t total = place.at;
	if (total > cap) {
		if (chained)
			for (uint32_t k = 0; k < count; k++) jm_encc_reset(c->chain[stream ? stream[k] : 0]);
		return -1;
	}
	/* k_enc_clear, k_enc_write_p */
	memset(out, 0, total);
	memset(out + total, 0xff, JM_ENC_TAIL);
	uint32_t *words = reinterpret_cast<uint32_t *>(out);
	for (size_t g = 0; g < mb.size(); g++) {
		const uint32_t k = (uint32_t)(g / mbs), m = (uint32_t)(g % mbs), row = m / mbw, col = m % mbw;
		const bool p_picture = plan[k].ordinal % gop != 0;
		const uint64_t slice_at = pic_off[k] + slice[(size_t)k * mbh + row];
		if (col == 0) {
			jm_enc_put_slice_header(words, slice_at, row, q[k]);
			if (row == 0) {
				if (p_picture) jm_encp_put_picture_header(words, pic_off[k], plan[k].ordinal % gop, r_size);
				else jm_enc_put_picture_headers(words, pic_off[k], w, h, c->frame_rate_code, plan[k].ordinal);
				if (plan[k].last) jm_enc_put_stream_tail(words, pic_off[k] + pic_bytes[k], end);
				if (k == 0) memset(out, 0xff, JM_ENC_LEAD_GAP);
			}
		}
		JmEncBits bw = jm_enc_bits_at(words, slice_at * 8u + mb[g].bits);
		jm_encp_write(mb[g], frames + k * fb, ref[k], cw, ch, col, row, p_picture, r_size, q[k], &g_tables, &g_ptables, zz, 1, pp, 1, bw);
		jm_enc_flush(bw);
	}
	for (uint32_t k = 0; k < count; k++) memcpy(recon_out + k * fb, rec[k], fb);
	return (int64_t)total;
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
