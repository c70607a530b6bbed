// TEST INFRASTRUCTURE ONLY -- not part of the product, never shipped or loaded by it.  Compiles the SAME rule, the same host
// plan and the same per-lane bodies k_resample wraps (jsmpeg_amd/csrc/pcm_resample.h: rs_*) with g++ and runs them in plain
// loops, one "lane" at a time, the chain's records and carries included -- so the resampler's samples can be checked in the
// build container, which has no GPU.  With -DSIM_RESAMPLE_MAIN: a stand-alone program for the sanitizers, which reads cases
// from a file (see main) into buffers of exactly the frames' size.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "pcm_resample.h"

extern "C" {

int sim_resample_plan(int in_rate, int out_rate, int32_t *lmh) {
	int L, M, H;
	if (rs_plan(in_rate, out_rate, &L, &M, &H) != 0) return -1;
	lmh[0] = L; lmh[1] = M; lmh[2] = H;
	return 0;
}
int sim_resample_taps(int in_rate, int out_rate, float *out) { return rs_taps_make(in_rate, out_rate, out); }
uint64_t sim_resample_outputs(int in_rate, int out_rate, uint64_t N) {
	RsRule R;
	return rs_rule_make(in_rate, out_rate, 2, 0, 0, 1.0f, 0, &R) ? 0 : rs_outputs(R, N);
}
uint32_t sim_resample_f16(float v) { return rs_f16_bits(v); }
uint32_t sim_resample_bf16(float v) { return rs_bf16_bits(v); }
uint32_t sim_resample_state_floats(int what) { return what ? RS_PART_FLOATS : RS_CARRY_FLOATS; }

// One call of the resampler the way jsmpeg_hip_resampler_resample plans and sequences it.  cfg = {in_rate, out_rate,
// channels_out, form, dtype, row}; flags as the C ABI's; rec ([max number + 1] RsChain), carry ([max number + 1][2][2][191]
// float) and part ([max number + 1][2][2][1152] float) are the caller's state between calls, updated here (all may be null for
// an unchained call).  out: the call's elements or frames (cap_bytes of room), offset / count per listed stream.  Returns the
// total (elements or frames); -1 - i: stream i has more samples than row; -1000001 - i: too many frames; -2000000: the
// settings are refused; -2000001: cap_bytes is too small.
int64_t sim_resample_call(const int32_t *cfg, float gain, const float *const *pcm, const uint32_t *frames, const uint32_t *numbers, uint32_t n_streams,
                          uint32_t flags, RsChain *rec, float *carry, float *part, void *out, uint64_t cap_bytes, uint64_t *offset, uint64_t *count) {
	RsRule R;
	if (rs_rule_make(cfg[0], cfg[1], cfg[2], cfg[3], cfg[4], gain, (uint32_t)cfg[5], &R) != 0) return -2000000;
	std::vector<float> taps((size_t)R.L * R.taps);
	rs_taps_make(cfg[0], cfg[1], taps.data());
	uint32_t top = 0;
	for (uint32_t i = 0; i < n_streams; i++) top = (numbers ? numbers[i] : i) > top ? (numbers ? numbers[i] : i) : top;
	std::vector<RsChain> none;
	std::vector<float> no_carry, no_part;
	if (!rec) { none.assign(top + 1, RsChain{ 0, 0, 0, 0 }); rec = none.data(); }
	if (!carry) { no_carry.assign((size_t)(top + 1) * RS_CARRY_FLOATS, 0.0f); carry = no_carry.data(); }
	if (!part) { no_part.assign((size_t)(top + 1) * RS_PART_FLOATS, 0.0f); part = no_part.data(); }
	std::vector<RsStream> list(n_streams + 1);
	uint64_t total = 0;
	const int rc = rs_plan_call(R, pcm, frames, numbers, n_streams, flags, rec, list.data(), offset, count, &total);
	if (rc < 0) return rc;
	const uint64_t elem = R.form == RS_FORM_FRAMES ? 4ull * 2 * RS_FRAME : (R.dtype == RS_F32 ? 4 : 2);
	if (total * elem > cap_bytes) return -2000001;
	static RsLds L;
	for (uint32_t i = 0; i < n_streams; i++)
		for (int ch = 0; ch < R.channels; ch++)
			for (uint32_t block = 0; block * RS_WG < list[i].slots; block++) {
				for (int t = 0; t < RS_WG; t++) rs_wg_stage(R, list[i], block, ch, t, carry, L);
				for (int t = 0; t < RS_WG; t++) rs_wg_slot(R, list[i], block, ch, t, taps.data(), part, out, L);
			}
	rs_plan_commit(R, frames, numbers, n_streams, flags, rec);
	return (int64_t)total;
}

}

#ifdef SIM_RESAMPLE_MAIN
// The stand-alone program: argv[1] names a file of cases, little endian:
//   u32 n_cases, then per case: i32 cfg[6] (as sim_resample_call's), f32 gain, u32 end, u32 n_streams, u32 n_calls, then per
//   call u32 frames[n_streams], then per stream its float32 samples [sum of its frames over the calls][2][1152].
// Every call of a case is chained when n_calls > 1; `end` puts END on the last call.  Each stream's samples of a call are
// copied into a buffer of exactly that size, and the output has exactly the call's size, so that a read or a write outside
// them is the sanitizer's to find.  Prints "cases <n> bytes <total> hash <fnv1a of all output bytes>".
int main(int argc, char **argv) {
	if (argc < 2) return 2;
	FILE *f = fopen(argv[1], "rb");
	if (!f) return 2;
	auto rd = [&](void *p, size_t n) { if (n && fread(p, 1, n, f) != n) { fprintf(stderr, "short file\n"); exit(2); } };
	uint32_t n_cases = 0;
	rd(&n_cases, 4);
	uint64_t bytes = 0, hash = 1469598103934665603ull;
	for (uint32_t c = 0; c < n_cases; c++) {
		int32_t cfg[6];
		float gain;
		uint32_t end, n_streams, n_calls;
		rd(cfg, 24); rd(&gain, 4); rd(&end, 4); rd(&n_streams, 4); rd(&n_calls, 4);
		std::vector<uint32_t> frames((size_t)n_streams * n_calls);
		rd(frames.data(), 4 * frames.size());
		std::vector<std::vector<float>> all(n_streams);
		for (uint32_t s = 0; s < n_streams; s++) {
			size_t n = 0;
			for (uint32_t k = 0; k < n_calls; k++) n += frames[(size_t)k * n_streams + s];
			all[s].resize(n * 2304);
			rd(all[s].data(), 4 * all[s].size());
		}
		RsRule R;
		if (rs_rule_make(cfg[0], cfg[1], cfg[2], cfg[3], cfg[4], gain, (uint32_t)cfg[5], &R) != 0) { fprintf(stderr, "case %u refused\n", c); return 1; }
		std::vector<RsChain> rec(n_streams, RsChain{ 0, 0, 0, 0 });
		std::vector<float> carry((size_t)n_streams * RS_CARRY_FLOATS, 0.0f), part((size_t)n_streams * RS_PART_FLOATS, 0.0f);
		std::vector<size_t> done(n_streams, 0);
		for (uint32_t k = 0; k < n_calls; k++) {
			const uint32_t *fr = frames.data() + (size_t)k * n_streams;
			const uint32_t flags = (n_calls > 1 ? RS_CHAIN : 0u) | ((end && k + 1 == n_calls) ? RS_END : 0u);
			std::vector<float *> bufs(n_streams);
			std::vector<const float *> ptrs(n_streams);
			for (uint32_t s = 0; s < n_streams; s++) {
				const size_t n = (size_t)fr[s] * 2304;
				bufs[s] = (float *)malloc(n * 4 + (n ? 0 : 1));
				if (n) memcpy(bufs[s], all[s].data() + done[s] * 2304, n * 4);
				ptrs[s] = bufs[s];
				done[s] += fr[s];
			}
			// the size of the call's output, from the plan alone
			std::vector<RsStream> list(n_streams + 1);
			std::vector<uint64_t> offset(n_streams + 1), count(n_streams + 1);
			uint64_t total = 0;
			if (rs_plan_call(R, ptrs.data(), fr, nullptr, n_streams, flags, rec.data(), list.data(), offset.data(), count.data(), &total) < 0) { fprintf(stderr, "case %u: plan refused\n", c); return 1; }
			const size_t elem = R.form == RS_FORM_FRAMES ? 4u * 2 * RS_FRAME : (R.dtype == RS_F32 ? 4 : 2);
			uint8_t *out = (uint8_t *)malloc(total * elem + (total ? 0 : 1));
			const int64_t got = sim_resample_call(cfg, gain, ptrs.data(), fr, nullptr, n_streams, flags, rec.data(), carry.data(), part.data(), out, total * elem,
			                                      offset.data(), count.data());
			if (got != (int64_t)total) { fprintf(stderr, "case %u call %u: %lld\n", c, k, (long long)got); return 1; }
			for (uint64_t b = 0; b < total * elem; b++) { hash = (hash ^ out[b]) * 1099511628211ull; bytes++; }
			free(out);
			for (uint32_t s = 0; s < n_streams; s++) free(bufs[s]);
		}
	}
	fclose(f);
	printf("cases %u bytes %llu hash %016llx\n", n_cases, (unsigned long long)bytes, (unsigned long long)hash);
	return 0;
}
#endif
