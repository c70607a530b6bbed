// TEST INFRASTRUCTURE ONLY -- not part of the product, never shipped or loaded by it.  Compiles the SAME rule, the same host
// plan, the same tables and the same per-lane bodies k_logmel wraps (jsmpeg_amd/csrc/logmel.h: lm_*) with g++ and runs them in
// plain loops, one "lane" at a time, the chain's records and carries included; the DFT's chains, which the kernel hands to the
// matrix unit, run here as the rule writes them, with fmaf (lm_dft_bin).  With -DSIM_LOGMEL_MAIN: a stand-alone program for the
// sanitizers, which reads cases from a file (see main) into buffers of exactly the samples' size.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "logmel.h"

// icfg = {sample_rate, n_fft, hop, n_mels, mel_scale, mel_norm, scale, layout, dtype, row}; fcfg = {f_min, f_max, floor}
static int make_rule(const int32_t *icfg, const float *fcfg, LmRule *R) {
	return lm_rule_make(icfg[0], icfg[1], icfg[2], icfg[3], icfg[6], icfg[7], icfg[8], fcfg[2], (uint32_t)icfg[9], R);
}

extern "C" {

// out = {bins, cols_pad, frames per workgroup, LDS floats, carry floats, sh, fstride}
int sim_logmel_rule(const int32_t *icfg, const float *fcfg, int32_t *out) {
	LmRule R;
	const int rc = make_rule(icfg, fcfg, &R);
	if (rc) return rc;
	out[0] = R.bins; out[1] = R.cols_pad; out[2] = LM_F; out[3] = (int32_t)lm_lds_floats(R); out[4] = R.carry_cap; out[5] = R.sh; out[6] = R.fstride;
	return 0;
}
uint64_t sim_logmel_frames(const int32_t *icfg, const float *fcfg, uint64_t n, int end) {
	LmRule R;
	return make_rule(icfg, fcfg, &R) ? 0 : lm_frames(R, n, end != 0);
}
int sim_logmel_basis(const int32_t *icfg, const float *fcfg, const float *window, float *out) {
	LmRule R;
	if (make_rule(icfg, fcfg, &R)) return -1;
	std::vector<double> w(R.n_fft);
	lm_window_make(R.n_fft, window, w.data());
	lm_basis_make(R.n_fft, w.data(), R.cols_pad, out);
	return 0;
}
int sim_logmel_filters(const int32_t *icfg, const float *fcfg, float *fb, int32_t *range) {
	LmRule R;
	if (make_rule(icfg, fcfg, &R)) return -1;
	std::vector<double> pts(R.n_mels + 2);
	return lm_filters_make(R.sample_rate, R.n_fft, R.n_mels, (double)fcfg[0], (double)fcfg[1], icfg[4], icfg[5], fb, range, pts.data());
}
void sim_logmel_log2(const float *in, float *out, uint64_t n) { for (uint64_t i = 0; i < n; i++) out[i] = lm_log2(in[i]); }
void sim_logmel_scale(int scale, float floor_, const float *in, float *out, uint64_t n) {
	for (uint64_t i = 0; i < n; i++) out[i] = scale == LM_POWER ? in[i] : lm_log_of(scale, floor_, in[i]);
}

// One call of the features the way jsmpeg_hip_logmel_features plans and sequences it.  rec ([max number + 1] LmChain) and carry
// ([max number + 1][2][carry floats]) are the caller's state between calls (both may be null for an unchained call).  out: the
// call's n_streams * n_mels * row elements (cap_bytes of room), count per listed stream.  dft (may be null): float32
// [stream][row][2 bins], re and im of every frame as the chains leave them.  Returns the elements; -1 - i: stream i has more
// frames than row; -2000000: the settings are refused; -2000001: cap_bytes is too small; -2000002: whisper with CHAIN.
int64_t sim_logmel_call(const int32_t *icfg, const float *fcfg, const float *window, const float *const *pcm, const uint32_t *samples, const uint32_t *numbers,
                        uint32_t n_streams, uint32_t flags, LmChain *rec, float *carry, void *out, uint64_t cap_bytes, uint64_t *count, float *dft) {
	LmRule R;
	if (make_rule(icfg, fcfg, &R) != 0) return -2000000;
	if ((flags & LM_CHAIN) && R.scale == LM_WHISPER) return -2000002;
	std::vector<double> w(R.n_fft), pts(R.n_mels + 2);
	std::vector<float> basis((size_t)R.n_fft * R.cols_pad), fb((size_t)R.n_mels * R.bins);
	std::vector<int32_t> range(2 * (size_t)R.n_mels);
	lm_window_make(R.n_fft, window, w.data());
	lm_basis_make(R.n_fft, w.data(), R.cols_pad, basis.data());
	if (lm_filters_make(R.sample_rate, R.n_fft, R.n_mels, (double)fcfg[0], (double)fcfg[1], icfg[4], icfg[5], fb.data(), range.data(), pts.data()) != 0) return -2000000;
	uint32_t top = 0;
	for (uint32_t i = 0; i < n_streams; i++) top = (numbers ? numbers[i] : i) > top ? (numbers ? numbers[i] : i) : top;
	std::vector<LmChain> none;
	std::vector<float> no_carry;
	if (!rec) { none.assign(top + 1, LmChain{ 0, 0, 0 }); rec = none.data(); }
	if (!carry) { no_carry.assign((size_t)(top + 1) * 2 * R.carry_cap, 0.0f); carry = no_carry.data(); }
	std::vector<LmStream> list(n_streams + 1);
	const int rc = lm_plan_call(R, pcm, samples, numbers, n_streams, flags, rec, list.data(), count);
	if (rc < 0) return rc;
	const uint64_t total = (uint64_t)n_streams * (uint64_t)R.n_mels * R.row;
	if (total * (R.dtype == RS_F32 ? 4 : 2) > cap_bytes) return -2000001;
	std::vector<float> lds(lm_lds_floats(R), 0.0f), tmp(R.scale == LM_WHISPER ? total : 0);
	float *xl = lds.data(), *p = lds.data() + R.span_lds;
	for (uint32_t i = 0; i < n_streams; i++)
		for (uint32_t block = 0; block * LM_F < R.row; block++) {
			for (int t = 0; t < LM_WG; t++) lm_wg_stage(R, list[i], block, t, carry, xl);
			for (int f = 0; f < LM_F && block * LM_F + f < list[i].frames; f++)
				for (int b = 0; b < R.bins; b++) {
					float re, im;
					lm_dft_bin(R, xl, basis.data(), f, b, &re, &im);
					p[(size_t)f * R.pstride + b] = lm_power(re, im);
					if (dft) { float *d = dft + (((size_t)i * R.row + block * LM_F + f) * R.bins + b) * 2; d[0] = re; d[1] = im; }
				}
			for (int t = 0; t < LM_WG; t++) {
				const uint32_t key = lm_wg_mel(R, list[i], block, t, fb.data(), range.data(), p, out, tmp.data());
				if (R.scale == LM_WHISPER && key > list[i].maxkey) list[i].maxkey = key;
			}
		}
	if (R.scale == LM_WHISPER)
		for (uint64_t e = 0; e < total; e++) lm_clamp_elem(R, list.data(), (size_t)e, tmp.data(), out);
	lm_plan_commit(samples, numbers, n_streams, flags, rec);
	return (int64_t)total;
}

}

#ifdef SIM_LOGMEL_MAIN
// The stand-alone program: argv[1] names a file of cases, little endian:
//   u32 n_cases, then per case: i32 icfg[10], f32 fcfg[3], u32 end, u32 n_streams, u32 n_calls, then per call
//   u32 samples[n_streams], then per stream its float32 samples (the sum of its counts over the calls).
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
		int32_t icfg[10];
		float fcfg[3];
		uint32_t end, n_streams, n_calls;
		rd(icfg, 40); rd(fcfg, 12); rd(&end, 4); rd(&n_streams, 4); rd(&n_calls, 4);
		std::vector<uint32_t> samples((size_t)n_streams * n_calls);
		rd(samples.data(), 4 * samples.size());
		std::vector<std::vector<float>> all(n_streams);
		for (uint32_t s = 0; s < n_streams; s++) {
			size_t n = 0;
			for (uint32_t k = 0; k < n_calls; k++) n += samples[(size_t)k * n_streams + s];
			all[s].resize(n);
			rd(all[s].data(), 4 * n);
		}
		LmRule R;
		if (make_rule(icfg, fcfg, &R) != 0) { fprintf(stderr, "case %u refused\n", c); return 1; }
		std::vector<LmChain> rec(n_streams, LmChain{ 0, 0, 0 });
		std::vector<float> carry((size_t)n_streams * 2 * R.carry_cap, 0.0f);
		std::vector<size_t> done(n_streams, 0);
		for (uint32_t k = 0; k < n_calls; k++) {
			const uint32_t *cnt = samples.data() + (size_t)k * n_streams;
			const uint32_t flags = (n_calls > 1 ? LM_CHAIN : 0u) | ((end && k + 1 == n_calls) ? LM_END : 0u);
			std::vector<float *> bufs(n_streams);
			std::vector<const float *> ptrs(n_streams);
			for (uint32_t s = 0; s < n_streams; s++) {
				bufs[s] = (float *)malloc((size_t)cnt[s] * 4 + (cnt[s] ? 0 : 1));
				if (cnt[s]) memcpy(bufs[s], all[s].data() + done[s], (size_t)cnt[s] * 4);
				ptrs[s] = bufs[s];
				done[s] += cnt[s];
			}
			const size_t size = (size_t)n_streams * R.n_mels * R.row * (R.dtype == RS_F32 ? 4 : 2);
			uint8_t *out = (uint8_t *)malloc(size + (size ? 0 : 1));
			std::vector<uint64_t> count(n_streams + 1);
			const int64_t got = sim_logmel_call(icfg, fcfg, nullptr, ptrs.data(), cnt, nullptr, n_streams, flags, rec.data(), carry.data(), out, size, count.data(), nullptr);
			if (got < 0) { fprintf(stderr, "case %u call %u: %lld\n", c, k, (long long)got); return 1; }
			for (size_t b = 0; b < size; b++) { hash = (hash ^ out[b]) * 1099511628211ull; bytes++; }
			free(out);
			for (uint32_t s = 0; s < n_streams; s++) free(bufs[s]);
		}
	}
	fclose(f);
	printf("cases %u bytes %llu hash %016llx\n", n_cases, (unsigned long long)bytes, (unsigned long long)hash);
	return 0;
}
#endif
