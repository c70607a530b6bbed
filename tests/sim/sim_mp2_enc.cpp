// TEST INFRASTRUCTURE ONLY -- not part of the product, never shipped or loaded by it.  Compiles the SAME rule and the same
// per-lane bodies k_mp2e_frame wraps (jsmpeg_amd/csrc/mp2_enc.h: mp2e_*) with g++ and runs them in plain loops, one "lane"
// at a time, the host's plan (mp2e_plan) and the chain's carries included -- so the MP2 encoder's bytes can be checked in
// the build container, which has no GPU.  With -DSIM_MP2_ENC_MAIN: a stand-alone program for the sanitizers, which reads
// cases from a file (see main) into buffers of exactly the frames' size.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "mp2_enc.h"

namespace {

// one workgroup: the phases of k_mp2e_frame in its order.  dbg (or null): [64][8] = code, index of part 0 / 1 / 2, loud in any
// part, nsf, scfsi, rounds (low byte) per pair
void run_frame(const Mp2EncRule &R, const Mp2EncFrame &F, const Mp2EncTables *T, int16_t *carry, uint8_t *out, uint32_t *stats, int32_t *S_out, uint8_t *dbg) {
	static Mp2EncLds L;
	for (int t = 0; t < MP2E_WG; t++) mp2e_wg_stage(R, F, T, carry, t, L);
	for (int t = 0; t < MP2E_WG; t++) mp2e_wg_carry_out(R, F, carry, t, L);
	for (int part = 0; part < 3; part++) {
		for (int t = 0; t < MP2E_WG; t++) mp2e_wg_window(R, part, t, L);
		for (int t = 0; t < MP2E_WG; t++) mp2e_wg_matrix(R, part, t, L);
	}
	for (int t = 0; t < MP2E_WG; t++) mp2e_wg_scale(R, t, L);
	Mp2EncPair P[64];
	for (int q = 0; q < 64; q++) { P[q] = mp2e_pair_begin(R, q, L); mp2e_alloc_table(R, P[q], q, L); }
	int left = mp2e_left_begin(R, F), rounds = 0;
	for (; rounds < MP2E_MAX_ROUNDS; rounds++) {
		uint32_t best = 0;
		for (int q = 0; q < 64; q++) {
			const uint32_t key = mp2e_alloc_pick(L, q, P[q].code, left);
			if (key != mp2e_alloc_key(R, P[q], q, left)) abort();      // the table is the rule's key
			best = key > best ? key : best;
		}
		if (!best) break;
		P[MP2E_KEY_PAIR(best)].code++;
		left -= (int)(best & MP2E_KEY_COST);
	}
	for (int q = 0; q < 64; q++) mp2e_pair_end(R, P[q], q, left, L);
	for (int q = 0; q < 64; q++) mp2e_wg_side(R, F, q, L);
	for (int t = 0; t < MP2E_WG; t++) mp2e_wg_quantise(t, L);
	for (int t = 0; t < MP2E_WG; t++) mp2e_wg_store(F, out, t, L);
	mp2e_wg_stats(F, stats, L);
	if (S_out) memcpy(S_out, L.S, sizeof(L.S));
	if (dbg)
		for (int q = 0; q < 64; q++) {
			uint8_t *d = dbg + 8 * q;
			d[0] = L.code[q]; d[1] = L.sfi[q][0]; d[2] = L.sfi[q][1]; d[3] = L.sfi[q][2];
			d[4] = (uint8_t)(L.loud[q][0] | L.loud[q][1] | L.loud[q][2]); d[5] = L.nsf[q]; d[6] = L.sel[q]; d[7] = (uint8_t)(rounds > 255 ? 255 : rounds);
		}
}

}

extern "C" {

// rule[9]: the fields of Mp2EncRule; < 0: the settings are refused
int sim_mp2_enc_rule(int sample_rate_index, int channels, int bitrate_index, int32_t *rule) {
	Mp2EncRule R;
	if (mp2e_rule_make(sample_rate_index, channels, bitrate_index, &R) != 0) return -1;
	if (rule) memcpy(rule, &R, sizeof(R));
	return 0;
}
uint64_t sim_mp2_enc_frame_offset(int sr, int ch, int br, uint64_t n) { Mp2EncRule R; return mp2e_rule_make(sr, ch, br, &R) ? 0 : mp2e_frame_offset(R, n); }
uint32_t sim_mp2_enc_frame_bytes(int sr, int ch, int br, uint64_t n) { Mp2EncRule R; return mp2e_rule_make(sr, ch, br, &R) ? 0 : mp2e_frame_bytes(R, n); }
uint64_t sim_mp2_enc_default_pts(int sr, int ch, int br, uint64_t n) { Mp2EncRule R; return mp2e_rule_make(sr, ch, br, &R) ? 0 : mp2e_default_pts(R, n); }
int sim_mp2_enc_quantise(int S, int steps, int sf) { return mp2e_quantise(S, steps, sf); }
int sim_mp2_enc_requantise(int code, int steps, int sf) { return mp2_requantise(code, steps, sf); }
int sim_mp2_enc_scale_index(int M) { return mp2e_scale_index(M); }
int sim_mp2_enc_gain(int steps) { return mp2e_gain(steps); }
int sim_mp2_enc_pcm_s16(float x) { return mp2e_pcm_s16(x); }
// The analysis of one channel through the kernel's own functions, with what the frame's pass keeps only in passing: x = 480
// samples of history and the frame's 1152; Y [36][64] (mp2e_window_sum), Z [36][32] (mp2e_window_fold), halves [36][32][2]
// (mp2e_y_lo / mp2e_y_hi of Z) and S [36][32] (mp2e_matrix_sum over the halves).
void sim_mp2_enc_analysis(const int16_t *x, int64_t *Y, int64_t *Z, int32_t *halves, int32_t *S) {
	Mp2EncTables T;
	mp2e_tables_make(&T);
	for (int p = 0; p < 36; p++) {
		const int16_t *newest = x + MP2E_HIST + 32 * p + 31;
		int32_t z[32][2];
		for (int i = 0; i < 64; i++) Y[64 * p + i] = mp2e_window_sum(newest, T.win, i);
		for (int t = 0; t < 32; t++) {
			const int64_t v = mp2e_window_fold(newest, T.win, t);
			Z[32 * p + t] = v;
			halves[64 * p + 2 * t] = z[t][0] = mp2e_y_lo(v); halves[64 * p + 2 * t + 1] = z[t][1] = mp2e_y_hi(v);
		}
		for (int k = 0; k < 32; k++) S[32 * p + k] = mp2e_matrix_sum(z, T.cosq, k);
	}
}
void sim_mp2_enc_tables(int32_t *win512, int32_t *cos128) {
	Mp2EncTables T;
	mp2e_tables_make(&T);
	memcpy(win512, T.win, sizeof(T.win)); memcpy(cos128, T.cosq, sizeof(T.cosq));
}

// One call of the encoder the way jsmpeg_hip_mp2_encoder_encode plans and sequences it.  cfg = {sample_rate_index, channels,
// bitrate_index}; flags: 2 = chained, then rec ([max number + 1] records of {have, parity, n (64 bit)}) and carry ([max number
// + 1][2][2][480] int16) are the caller's state between calls, updated here.  out: the call's bytes (cap of them), begin / end
// per listed stream, stats [frame][4], S ([frame][2][36][32], or null), dbg ([frame][64][8], or null).  Returns the total, < 0
// when the settings are refused or cap is too small.
int64_t sim_mp2_enc_chain(const int32_t *cfg, const float *const *pcm, const uint32_t *frames, const uint32_t *numbers, uint32_t n_streams, uint32_t flags,
                          Mp2EncChain *rec, int16_t *carry, uint8_t *out, uint64_t cap, uint64_t *begin, uint64_t *end, uint32_t *stats, int32_t *S, uint8_t *dbg) {
	Mp2EncRule R;
	if (mp2e_rule_make(cfg[0], cfg[1], cfg[2], &R) != 0) return -1;
	Mp2EncTables T;
	mp2e_tables_make(&T);
	uint32_t total_frames = 0;
	for (uint32_t i = 0; i < n_streams; i++) total_frames += frames[i];
	std::vector<Mp2EncFrame> list(total_frames + 1);
	std::vector<Mp2EncChain> none;
	if (!rec) { uint32_t top = 0; for (uint32_t i = 0; i < n_streams; i++) top = (numbers ? numbers[i] : i) > top ? (numbers ? numbers[i] : i) : top; none.assign(top + 1, Mp2EncChain{0, 0, 0}); }
	const uint64_t total = mp2e_plan(R, pcm, frames, numbers, n_streams, flags, rec ? rec : none.data(), list.data(), begin, end);
	if (total > cap) return -2;
	std::vector<int16_t> no_carry;
	if (!carry) no_carry.assign(1, 0);
	for (uint32_t k = 0; k < total_frames; k++)
		run_frame(R, list[k], &T, carry ? carry : no_carry.data(), out, stats + 4 * (size_t)k, S ? S + (size_t)k * 2 * 36 * 32 : nullptr, dbg ? dbg + (size_t)k * 512 : nullptr);
	if (rec) mp2e_plan_commit(frames, numbers, n_streams, flags, rec);
	return (int64_t)total;
}

}

#ifdef SIM_MP2_ENC_MAIN
// The stand-alone program: argv[1] names a file of cases, little endian:
//   u32 n_cases, then per case: i32 cfg[3], u32 n_streams, u32 n_calls, then per call u32 frames[n_streams], then per stream
//   its float32 samples [sum of its frames over the calls][2][1152].
// Every call of a case is chained when n_calls > 1.  Each stream's samples of a call are copied into a buffer of exactly that
// size, so that a read outside the frames is the sanitizer's to find.  Prints "cases <n> bytes <total> hash <fnv1a of all bytes>".
int main(int argc, char **argv) {
	if (argc < 2) return 2;
	FILE *f = fopen(argv[1], "rb");
	if (!f) return 2;
	auto rd = [&](void *p, size_t n) { if (n && fread(p, 1, n, f) != n) { fprintf(stderr, "short file\n"); exit(2); } };
	uint32_t n_cases = 0;
	rd(&n_cases, 4);
	uint64_t bytes = 0, hash = 1469598103934665603ull;
	for (uint32_t c = 0; c < n_cases; c++) {
		int32_t cfg[3];
		uint32_t n_streams, n_calls;
		rd(cfg, 12); rd(&n_streams, 4); rd(&n_calls, 4);
		std::vector<uint32_t> frames((size_t)n_streams * n_calls);
		rd(frames.data(), 4 * frames.size());
		std::vector<std::vector<float>> all(n_streams);
		for (uint32_t s = 0; s < n_streams; s++) {
			size_t n = 0;
			for (uint32_t k = 0; k < n_calls; k++) n += frames[(size_t)k * n_streams + s];
			all[s].resize(n * 2304);
			rd(all[s].data(), 4 * all[s].size());
		}
		std::vector<Mp2EncChain> rec(n_streams, Mp2EncChain{0, 0, 0});
		std::vector<int16_t> carry((size_t)n_streams * MP2E_CARRY_WORDS, 0);
		std::vector<size_t> done(n_streams, 0);
		for (uint32_t k = 0; k < n_calls; k++) {
			const uint32_t *fr = frames.data() + (size_t)k * n_streams;
			std::vector<float *> bufs(n_streams);
			std::vector<const float *> ptrs(n_streams);
			uint32_t total_frames = 0;
			for (uint32_t s = 0; s < n_streams; s++) {
				const size_t n = (size_t)fr[s] * 2304;
				bufs[s] = (float *)malloc(n * 4 + (n ? 0 : 1));
				if (n) memcpy(bufs[s], all[s].data() + done[s] * 2304, n * 4);
				ptrs[s] = bufs[s];
				done[s] += fr[s];
				total_frames += fr[s];
			}
			const size_t cap = (size_t)total_frames * (MP2E_MAX_FRAME_BYTES + 1) + 16 * n_streams;
			uint8_t *out = (uint8_t *)malloc(cap + 1);
			std::vector<uint64_t> begin(n_streams), end(n_streams);
			std::vector<uint32_t> stats((size_t)total_frames * 4 + 4);
			const int64_t total = sim_mp2_enc_chain(cfg, ptrs.data(), fr, nullptr, n_streams, n_calls > 1 ? MP2E_CHAIN : 0u, rec.data(), carry.data(), out, cap,
			                                        begin.data(), end.data(), stats.data(), nullptr, nullptr);
			if (total < 0) { fprintf(stderr, "case %u refused\n", c); return 1; }
			for (uint32_t s = 0; s < n_streams; s++)
				for (uint64_t b = begin[s]; b < end[s]; b++) { hash = (hash ^ out[b]) * 1099511628211ull; bytes++; }
			free(out);
			for (uint32_t s = 0; s < n_streams; s++) free(bufs[s]);
		}
	}
	fclose(f);
	printf("cases %u bytes %llu hash %016llx\n", n_cases, (unsigned long long)bytes, (unsigned long long)hash);
	return 0;
}
#endif
