/*
 * LOG-MEL FEATURES on the device: the gfx950 kernels and the host runtime behind part 12 of include/jsmpeg_hip.h.  Float32 mono
 * PCM in HBM (the resampler's waveform, a tensor) -> [stream][n_mels][row] or [stream][row][n_mels] in f32 / f16 / bf16, what a
 * speech model reads.
 *
 * The rule, the per-lane bodies and the host's plan: logmel.h, shared with the test-only simulator.  Counts are closed form, so
 * a call is ONE kernel (two for the whisper scale: its maximum belongs to a whole stream) and a pure enqueue.  No audio
 * arithmetic happens on the host; the tables are built there once, at create.
 */
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "host_common.h"
#include "pass_state.h"
#include "jsmpeg_hip.h"
#include "logmel.h"

static_assert(JSMPEG_HIP_LOGMEL_END == LM_END && JSMPEG_HIP_LOGMEL_CHAIN == LM_CHAIN, "flags");
static_assert(JSMPEG_HIP_LOGMEL_POWER == LM_POWER && JSMPEG_HIP_LOGMEL_LOG == LM_LOG && JSMPEG_HIP_LOGMEL_LOG10 == LM_LOG10 && JSMPEG_HIP_LOGMEL_DB == LM_DB &&
              JSMPEG_HIP_LOGMEL_WHISPER == LM_WHISPER, "scales");
static_assert(JSMPEG_HIP_LOGMEL_MEL_MAJOR == LM_MEL_MAJOR && JSMPEG_HIP_LOGMEL_TIME_MAJOR == LM_TIME_MAJOR, "layouts");
static_assert(JSMPEG_HIP_LOGMEL_HTK == LM_HTK && JSMPEG_HIP_LOGMEL_SLANEY == LM_SLANEY, "mel scales");
static_assert(LM_F == 32 && LM_TILE == 32 && LM_WG == 64 * LM_WAVES, "the tile is one 32x32 MFMA");

/* ================================================================================================ kernels */

typedef float lm_acc_t __attribute__((ext_vector_type(16)));

/* NV tiles of 32 columns of B (g, g + 4, ..) against the block's 32 frames.  v_mfma_f32_32x32x2_f32: lane l gives A[row l & 31]
 * [k = l >> 5] = x of frame l & 31 and B[k = l >> 5][column l & 31]; D = fma(a_k1, b_k1, fma(a_k0, b_k0, C)), so the steps in
 * ascending k are logmel.h's chain.  The accumulators have the column on the lane (l & 31) and the frame in the register:
 * (reg & 3) + 8 (reg >> 2) + 4 (l >> 5).  re sits on an even lane and im on the next one: one lane exchange, then the even
 * lane writes the power. */
template <int NV>
static __device__ __forceinline__ void lm_tiles(const LmRule &R, const float *xa, const float *basis, int g, int r, int hf, float *p) {
	lm_acc_t acc[NV];
#pragma unroll
	for (int j = 0; j < NV; j++)
		for (int i = 0; i < 16; i++) acc[j][i] = 0.0f;
	const float *bp = basis + (size_t)hf * R.cols_pad + g * LM_TILE + r;
	const size_t step = 2 * (size_t)R.cols_pad;
	const int steps = R.half, sh = R.sh;
	const int whole = steps & ~3;
	int kk = 0;
	if (whole) {
		/* four steps at a time; the NEXT four steps' operands are asked for before this four's MFMAs are issued, so that a
		 * wavefront's loads from L2 run under its own matrix work (the last round asks for its own operands again) */
		float a[4], b[4][NV];
#pragma unroll
		for (int u = 0; u < 4; u++) {
			const int k = 2 * u + hf;
			a[u] = xa[k + (k >> sh)];
#pragma unroll
			for (int j = 0; j < NV; j++) b[u][j] = bp[u * step + j * LM_WAVES * LM_TILE];
		}
		for (; kk < whole; kk += 4) {
			const int kn = kk + 4 < whole ? kk + 4 : kk;
			const float *bn = bp + (size_t)kn * step;
			float an[4], bb[4][NV];
#pragma unroll
			for (int u = 0; u < 4; u++) {
				const int k = 2 * (kn + u) + hf;
				an[u] = xa[k + (k >> sh)];
#pragma unroll
				for (int j = 0; j < NV; j++) bb[u][j] = bn[u * step + j * LM_WAVES * LM_TILE];
			}
			__builtin_amdgcn_sched_barrier(0);                     /* (left alone, the scheduler sinks each load to just in front of its MFMA) */
#pragma unroll
			for (int u = 0; u < 4; u++)
#pragma unroll
				for (int j = 0; j < NV; j++) acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[u], b[u][j], acc[j], 0, 0, 0);
			__builtin_amdgcn_sched_barrier(0);
#pragma unroll
			for (int u = 0; u < 4; u++) {
				a[u] = an[u];
#pragma unroll
				for (int j = 0; j < NV; j++) b[u][j] = bb[u][j];
			}
		}
		bp += (size_t)whole * step;
	}
	for (; kk < steps; kk++) {
		const int k = 2 * kk + hf;
		const float a = xa[k + (k >> sh)];
#pragma unroll
		for (int j = 0; j < NV; j++) acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, bp[j * LM_WAVES * LM_TILE], acc[j], 0, 0, 0);
		bp += step;
	}
#pragma unroll
	for (int j = 0; j < NV; j++) {
		const int c = (g + j * LM_WAVES) * LM_TILE + r, b = c >> 1;
#pragma unroll
		for (int i = 0; i < 16; i++) {
			const float re = acc[j][i], im = __shfl_xor(re, 1);
			const int f = (i & 3) + 8 * (i >> 2) + 4 * hf;
			if (!(r & 1) && b < R.bins) p[f * R.pstride + b] = lm_power(re, im);
		}
	}
}

static __device__ __forceinline__ void lm_wg_dft(const LmRule &R, const float *xl, const float *basis, int tid, float *p) {
	const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), r = lane & 31, hf = lane >> 5;
	const float *xa = xl + r * R.fstride;
	for (int g = wave; g < R.tiles; g += LM_WAVES * LM_NT) {
		const int nv = (R.tiles - g + LM_WAVES - 1) / LM_WAVES;        /* (the same in the whole wave) */
		if (nv >= 4) lm_tiles<4>(R, xa, basis, g, r, hf, p);
		else if (nv == 3) lm_tiles<3>(R, xa, basis, g, r, hf, p);
		else if (nv == 2) lm_tiles<2>(R, xa, basis, g, r, hf, p);
		else lm_tiles<1>(R, xa, basis, g, r, hf, p);
	}
}

/* workgroup = LM_F consecutive columns of one stream of the call: grid (blocks of the row, streams).  Dynamic LDS: the span,
 * then p (lm_lds_floats).  A block behind the stream's frames only writes the pad value. */
__global__ void __launch_bounds__(LM_WG) k_logmel(LmRule R, LmStream *streams, const float *basis, const float *fb, const int32_t *range, float *carry, void *out,
                                                  float *tmp) {
	extern __shared__ float lm_lds[];
	float *xl = lm_lds, *p = lm_lds + R.span_lds;
	const LmStream S = streams[blockIdx.y];
	const int tid = (int)threadIdx.x;
	lm_wg_stage(R, S, blockIdx.x, tid, carry, xl);
	if (blockIdx.x * LM_F < S.frames) {                            /* (uniform in the workgroup) */
		__syncthreads();
		lm_wg_dft(R, xl, basis, tid, p);
		__syncthreads();
	}
	const uint32_t key = lm_wg_mel(R, S, blockIdx.x, tid, fb, range, p, out, tmp);
	if (R.scale == LM_WHISPER && key) atomicMax(&streams[blockIdx.y].maxkey, key);
}

__global__ void __launch_bounds__(256) k_logmel_clamp(LmRule R, const LmStream *streams, const float *tmp, void *out, uint64_t total) {
	const uint64_t e = (uint64_t)blockIdx.x * 256u + threadIdx.x;
	if (e < total) lm_clamp_elem(R, streams, (size_t)e, tmp, out);
}

/* ================================================================================================ host */

struct jsmpeg_hip_logmel_t {
	jsmpeg_hip_logmel_config_t cfg;
	JmPass pass{ "logmel: a pass is in flight: jsmpeg_hip_logmel_sync (or a reader) settles it first", "logmel: no features were computed yet" };
	LmRule R;
	float *d_basis = nullptr, *d_fb = nullptr, *d_carry = nullptr, *d_tmp = nullptr;
	int32_t *d_range = nullptr;
	LmStream *d_streams = nullptr, *h_streams = nullptr;       /* h_: pinned */
	void *d_out = nullptr;
	std::vector<LmChain> chain;                                /* per stream number */
	std::vector<uint64_t> offset, count, c_list;               /* per stream number; per listed stream */
	uint64_t total = 0;                                        /* elements of the last call */
};                                                             /* pass.ev[1]: behind the upload */

static size_t lm_elem_bytes(const LmRule &R) { return R.dtype == RS_F32 ? 4 : 2; }

/* the settings as the rule sees them; nullptr and a message when they are refused */
static const char *lm_check(const jsmpeg_hip_logmel_config_t *c, LmRule *R) {
	if (!c) return "logmel: NULL config";
	if (c->n_fft > 1024 || c->hop > 1024 || c->n_mels > 256 || c->sample_rate > 48000) return "logmel: sample_rate is 8000 .. 48000, n_fft even in 32 .. 1024, hop 1 .. n_fft / 2, n_mels 1 .. 256";
	if (!(c->floor == c->floor)) return "logmel: floor is not a number";
	switch (lm_rule_make((int)c->sample_rate, (int)c->n_fft, (int)c->hop, (int)c->n_mels, (int)c->scale, (int)c->layout, (int)c->dtype, c->floor, 0, R)) {
	case 0: break;
	case -5: return "logmel: scale is POWER, LOG, LOG10, DB or WHISPER, layout MEL_MAJOR or TIME_MAJOR, dtype F32, F16 or BF16";
	case -6: return "logmel: floor must be a normal positive float (0: 1e-10)";
	default: return "logmel: sample_rate is 8000 .. 48000, n_fft even in 32 .. 1024, hop 1 .. n_fft / 2, n_mels 1 .. 256";
	}
	if (c->scale > 4 || c->layout > 1 || c->dtype > 2) return "logmel: scale, layout or dtype out of range";
	if (lm_lds_floats(*R) * sizeof(float) > LM_LDS_MAX) return "logmel: the tile does not fit the LDS";
	return nullptr;
}

static int lm_tables(const jsmpeg_hip_logmel_config_t *c, const LmRule &R, std::vector<float> *basis, std::vector<float> *fb, std::vector<int32_t> *range) {
	if (basis) {
		if (c->window)
			for (uint32_t k = 0; k < c->n_fft; k++)
				if (!(c->window[k] - c->window[k] == 0.0f)) return fail("logmel: window[%u] is not finite", k);
		std::vector<double> w(R.n_fft);
		lm_window_make(R.n_fft, c->window, w.data());
		basis->resize((size_t)R.n_fft * R.cols_pad);
		lm_basis_make(R.n_fft, w.data(), R.cols_pad, basis->data());
	}
	if (fb) {
		std::vector<double> pts(R.n_mels + 2);
		fb->resize((size_t)R.n_mels * R.bins); range->resize(2 * (size_t)R.n_mels);
		if (lm_filters_make(R.sample_rate, R.n_fft, R.n_mels, (double)c->f_min, (double)c->f_max, (int)c->mel_scale, (int)c->mel_norm, fb->data(), range->data(), pts.data()) != 0)
			return fail("logmel: 0 <= f_min < f_max <= sample_rate / 2 (f_max 0: sample_rate / 2), mel_scale HTK or SLANEY, mel_norm 0 or 1");
	}
	return 0;
}

static uint32_t lm_default_row(const LmRule &R, uint32_t max_samples) { return (uint32_t)(((uint64_t)max_samples + (uint64_t)R.half) / (uint64_t)R.hop + 2); }

extern "C" int jsmpeg_hip_logmel_plan(const jsmpeg_hip_logmel_config_t *config, uint64_t n, uint64_t out[8]) {
	g_err[0] = 0;
	LmRule R;
	if (const char *why = lm_check(config, &R)) return fail("%s", why);
	if (!out) return fail("logmel: NULL out");
	out[0] = (uint64_t)R.bins; out[1] = (uint64_t)R.cols_pad; out[2] = lm_frames(R, n, false); out[3] = lm_frames(R, n, true);
	out[4] = LM_F; out[5] = lm_lds_floats(R) * sizeof(float); out[6] = (uint64_t)R.carry_cap; out[7] = config->row ? config->row : lm_default_row(R, config->max_samples);
	return 0;
}

extern "C" int jsmpeg_hip_logmel_basis(const jsmpeg_hip_logmel_config_t *config, float *out) {
	g_err[0] = 0;
	LmRule R;
	if (const char *why = lm_check(config, &R)) return fail("%s", why);
	if (!out) return fail("logmel: NULL out");
	std::vector<float> basis;
	if (lm_tables(config, R, &basis, nullptr, nullptr) < 0) return -1;
	memcpy(out, basis.data(), sizeof(float) * basis.size());
	return 0;
}

extern "C" int jsmpeg_hip_logmel_filters(const jsmpeg_hip_logmel_config_t *config, float *fb, int32_t *ranges) {
	g_err[0] = 0;
	LmRule R;
	if (const char *why = lm_check(config, &R)) return fail("%s", why);
	std::vector<float> f;
	std::vector<int32_t> r;
	if (lm_tables(config, R, nullptr, &f, &r) < 0) return -1;
	if (fb) memcpy(fb, f.data(), sizeof(float) * f.size());
	if (ranges) memcpy(ranges, r.data(), sizeof(int32_t) * r.size());
	return 0;
}

static void lm_free(jsmpeg_hip_logmel_t *h) {
	if (!h) return;
	jm_pass_close(h->pass);
	hipFree(h->d_basis); hipFree(h->d_fb); hipFree(h->d_range); hipFree(h->d_carry); hipFree(h->d_tmp); hipFree(h->d_streams); hipFree(h->d_out);
	if (h->h_streams) hipHostFree(h->h_streams);
	delete h;
}

static int lm_alloc(jsmpeg_hip_logmel_t *h, const std::vector<float> &basis, const std::vector<float> &fb, const std::vector<int32_t> &range) {
	const size_t ns = h->cfg.max_streams, cap = ns * (size_t)h->R.n_mels * h->R.row;
	HIP_TRY(jm_malloc(&h->d_basis, sizeof(float) * basis.size()));
	HIP_TRY(hipMemcpy(h->d_basis, basis.data(), sizeof(float) * basis.size(), hipMemcpyHostToDevice));
	HIP_TRY(jm_malloc(&h->d_fb, sizeof(float) * fb.size()));
	HIP_TRY(hipMemcpy(h->d_fb, fb.data(), sizeof(float) * fb.size(), hipMemcpyHostToDevice));
	HIP_TRY(jm_malloc(&h->d_range, sizeof(int32_t) * range.size()));
	HIP_TRY(hipMemcpy(h->d_range, range.data(), sizeof(int32_t) * range.size(), hipMemcpyHostToDevice));
	HIP_TRY(jm_malloc(&h->d_carry, sizeof(float) * 2 * (size_t)h->R.carry_cap * ns));
	HIP_TRY(hipMemset(h->d_carry, 0, sizeof(float) * 2 * (size_t)h->R.carry_cap * ns));
	HIP_TRY(jm_malloc(&h->d_streams, sizeof(LmStream) * ns));
	HIP_TRY(hipHostMalloc(reinterpret_cast<void **>(&h->h_streams), sizeof(LmStream) * ns, hipHostMallocDefault));
	HIP_TRY(jm_malloc(reinterpret_cast<uint8_t **>(&h->d_out), cap * lm_elem_bytes(h->R)));
	if (h->R.scale == LM_WHISPER) HIP_TRY(jm_malloc(&h->d_tmp, cap * sizeof(float)));
	/* the attribute belongs to the kernel, not to the handle: every handle asks for the whole LDS, so that none lowers another's */
	HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(k_logmel), hipFuncAttributeMaxDynamicSharedMemorySize, LM_LDS_MAX));
	if (jm_pass_events(h->pass) < 0) return -1;
	HIP_TRY(hipDeviceSynchronize());
	return 0;
}

extern "C" jsmpeg_hip_logmel_t *jsmpeg_hip_logmel_create(const jsmpeg_hip_logmel_config_t *config) {
	g_err[0] = 0;
	LmRule R;
	if (const char *why = lm_check(config, &R)) { fail("%s", why); return nullptr; }
	if (config->max_streams < 1 || config->max_streams > 65535 || config->max_samples < 1 || config->max_samples > (1u << 30)) {
		fail("logmel: max_streams is 1 .. 65535 and max_samples 1 .. 2^30");
		return nullptr;
	}
	const uint32_t row = config->row ? config->row : lm_default_row(R, config->max_samples);
	if (row > 0x7fffffffu - LM_F) { fail("logmel: row %u is too large", row); return nullptr; }
	R.row = row;
	if (getenv("JSMPEG_HIP_LOGMEL_NO_SKEW")) { R.sh = 31; R.fstride = R.hop; R.span_lds = R.span; }      /* measurements only: the naive LDS map, same results */
	std::vector<float> basis, fb;
	std::vector<int32_t> range;
	if (lm_tables(config, R, &basis, &fb, &range) < 0) return nullptr;
	if (jsmpeg_hip_device_count() <= 0) { fail("no HIP device available: the log-mel features have no CPU fallback"); return nullptr; }
	jsmpeg_hip_logmel_t *h = new jsmpeg_hip_logmel_t();
	h->cfg = *config;
	h->cfg.window = nullptr;
	h->R = R;
	if (jm_pass_open(h->pass, config->device) < 0) { delete h; return nullptr; }
	h->chain.assign(config->max_streams, LmChain{ 0, 0, 0 });
	h->offset.assign(config->max_streams, 0); h->count.assign(config->max_streams, 0);
	h->c_list.resize(config->max_streams);
	if (lm_alloc(h, basis, fb, range) != 0) { lm_free(h); return nullptr; }
	return h;
}

extern "C" void jsmpeg_hip_logmel_destroy(jsmpeg_hip_logmel_t *h) { lm_free(h); }

extern "C" int jsmpeg_hip_logmel_features(jsmpeg_hip_logmel_t *h, const void *const *pcm, const uint32_t *samples, const uint32_t *stream_numbers, uint32_t n_streams,
                                          uint32_t flags, void *hip_stream) {
	g_err[0] = 0;
	if (!h) return fail("logmel: NULL handle");
	if (jm_pass_idle(h->pass) < 0) return -1;
	if (flags & ~(JSMPEG_HIP_LOGMEL_END | JSMPEG_HIP_LOGMEL_CHAIN)) return fail("logmel: unknown flags 0x%x", flags);
	if ((flags & JSMPEG_HIP_LOGMEL_CHAIN) && h->R.scale == LM_WHISPER) return fail("logmel: the whisper scale takes its maximum over a whole call, so it is refused with CHAIN");
	if (n_streams > h->cfg.max_streams) return fail("logmel: %u streams > max_streams %u", n_streams, h->cfg.max_streams);
	if (n_streams && (!pcm || !samples)) return fail("logmel: NULL pcm or samples");
	for (uint32_t i = 0; i < n_streams; i++) {
		if (jm_pass_check_number("logmel", stream_numbers, i, h->cfg.max_streams) < 0) return -1;
		if (samples[i] > h->cfg.max_samples) return fail("logmel: stream %u of the call has %u samples > max_samples %u: nothing was enqueued", i, samples[i], h->cfg.max_samples);
		if (jm_pass_check_pcm("logmel", pcm, samples, i) < 0) return -1;
	}
	const int rc = lm_plan_call(h->R, reinterpret_cast<const float *const *>(pcm), samples, stream_numbers, n_streams, flags, h->chain.data(), h->h_streams, h->c_list.data());
	if (rc < 0) return fail("logmel: stream %d of the call yields %llu frames, row is %u: nothing was enqueued", -1 - rc, (unsigned long long)h->c_list[-1 - rc], h->R.row);
	const uint64_t total = (uint64_t)n_streams * (uint64_t)h->R.n_mels * h->R.row;
	hipStream_t st = (hipStream_t)hip_stream;
	if (jm_pass_begin(h->pass, st) < 0) return -1;
	if (n_streams) HIP_TRY(hipMemcpyAsync(h->d_streams, h->h_streams, sizeof(LmStream) * n_streams, hipMemcpyHostToDevice, st));
	if (jm_pass_mark(h->pass, st) < 0) return -1;
	if (n_streams) {
		hipLaunchKernelGGL(k_logmel, dim3((h->R.row + LM_F - 1) / LM_F, n_streams), dim3(LM_WG), lm_lds_floats(h->R) * sizeof(float), st, h->R, h->d_streams, h->d_basis,
		                   h->d_fb, h->d_range, h->d_carry, h->d_out, h->d_tmp);
		HIP_TRY(hipGetLastError());
		if (h->R.scale == LM_WHISPER) {
			hipLaunchKernelGGL(k_logmel_clamp, dim3((uint32_t)((total + 255) / 256)), dim3(256), 0, st, h->R, h->d_streams, h->d_tmp, h->d_out, total);
			HIP_TRY(hipGetLastError());
		}
	}
	if (jm_pass_end(h->pass, st) < 0) return -1;
	std::fill(h->offset.begin(), h->offset.end(), 0); std::fill(h->count.begin(), h->count.end(), 0);
	for (uint32_t i = 0; i < n_streams; i++) {
		const uint32_t s = stream_numbers ? stream_numbers[i] : i;
		h->offset[s] = (uint64_t)i * (uint64_t)h->R.n_mels * h->R.row; h->count[s] = h->c_list[i];
	}
	lm_plan_commit(samples, stream_numbers, n_streams, flags, h->chain.data());
	h->total = total;
	h->pass.pending = true; h->pass.have_pass = true;
	return 0;
}

extern "C" int jsmpeg_hip_logmel_sync(jsmpeg_hip_logmel_t *h) {
	g_err[0] = 0;
	if (!h) return fail("logmel: NULL handle");
	return jm_pass_settle(h->pass);
}

extern "C" int jsmpeg_hip_logmel_query(jsmpeg_hip_logmel_t *h) {
	g_err[0] = 0;
	if (!h) return fail("logmel: NULL handle");
	return jm_pass_query(h->pass);
}

/* the address and the bytes are the plan's: answered without waiting */
extern "C" void *jsmpeg_hip_logmel_out(jsmpeg_hip_logmel_t *h, uint64_t *bytes) {
	g_err[0] = 0;
	if (!h) { fail("logmel: NULL handle"); return nullptr; }
	if (jm_pass_have(h->pass) < 0) return nullptr;
	if (bytes) *bytes = h->total * lm_elem_bytes(h->R);
	return h->d_out;
}

/* closed form: answered from the plan, without waiting */
extern "C" int jsmpeg_hip_logmel_stream_out(jsmpeg_hip_logmel_t *h, uint32_t stream, uint64_t *offset, uint64_t *count) {
	g_err[0] = 0;
	if (!h) return fail("logmel: NULL handle");
	if (jm_pass_have(h->pass) < 0 || jm_pass_stream_bound("logmel", stream, h->cfg.max_streams) < 0) return -1;
	if (offset) *offset = h->offset[stream];
	if (count) *count = h->count[stream];
	return 0;
}

extern "C" int jsmpeg_hip_logmel_chain_reset(jsmpeg_hip_logmel_t *h, uint32_t stream) {
	g_err[0] = 0;
	if (!h) return fail("logmel: NULL handle");
	return jm_pass_chain_reset(h->pass, "logmel", h->chain, stream);
}

extern "C" int jsmpeg_hip_logmel_chain_info(jsmpeg_hip_logmel_t *h, uint32_t stream, uint64_t out[3]) {
	g_err[0] = 0;
	if (!h) return fail("logmel: NULL handle");
	if (!out) return fail("logmel: NULL out");
	if (jm_pass_stream_bound("logmel", stream, h->cfg.max_streams) < 0) return -1;
	const LmChain &c = h->chain[stream];
	out[0] = c.have; out[1] = c.have ? c.n : 0; out[2] = c.have ? lm_frames(h->R, c.n, false) : 0;
	return 0;
}

extern "C" int jsmpeg_hip_logmel_timings(jsmpeg_hip_logmel_t *h, float out_ms[2]) {
	g_err[0] = 0;
	if (!h) return fail("logmel: NULL handle");
	if (jm_pass_ready(h->pass) < 0) return -1;
	if (!out_ms) return fail("logmel: NULL out_ms");
	if (jm_pass_elapsed(h->pass, 1, 2, &out_ms[0]) < 0) return -1;
	return jm_pass_elapsed(h->pass, 0, 2, &out_ms[1]);
}
