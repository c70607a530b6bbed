/*
 * The PCM RESAMPLER on the device: the gfx950 kernel and the host runtime behind part 11 of include/jsmpeg_hip.h.  PCM in HBM
 * (the decoders' [frame][2][1152] float32) -> a padded batch of waveforms for models (f32 / f16 / bf16), or frames at another
 * rate for the MP2 encoder of part 9.
 *
 * The rule, the per-lane bodies and the host's plan: pcm_resample.h, shared with the test-only simulator.  Counts are closed
 * form, so nothing is scanned: the host knows every count and offset at enqueue time and a call is ONE kernel.  No audio
 * arithmetic happens on the host.
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
#include "pcm_resample.h"

static_assert(JSMPEG_HIP_RESAMPLE_END == RS_END && JSMPEG_HIP_RESAMPLE_CHAIN == RS_CHAIN, "flags");
static_assert(JSMPEG_HIP_RESAMPLE_WAVEFORM == RS_FORM_WAVEFORM && JSMPEG_HIP_RESAMPLE_FRAMES == RS_FORM_FRAMES, "forms");
static_assert(JSMPEG_HIP_RESAMPLE_F32 == RS_F32 && JSMPEG_HIP_RESAMPLE_F16 == RS_F16 && JSMPEG_HIP_RESAMPLE_BF16 == RS_BF16, "dtypes");

/* ================================================================================================ kernel */

/* workgroup = RS_WG consecutive slots of one (stream of the call, filter channel): grid (blocks, channels, streams).  LDS: the
 * input span the block's outputs read, 7 KB; the taps come from the table in device memory (at most 83 KB, shared by every
 * workgroup, so it stays in L2).  Streams without slots and blocks past a stream's slots leave at once. */
__global__ void __launch_bounds__(RS_WG) k_resample(RsRule R, const RsStream *streams, const float *taps, float *carry, float *part, void *out) {
	__shared__ RsLds L;
	const RsStream S = streams[blockIdx.z];
	if (blockIdx.x * RS_WG >= S.slots) return;             /* (uniform in the workgroup) */
	const int tid = (int)threadIdx.x, ch = (int)blockIdx.y;
	rs_wg_stage(R, S, blockIdx.x, ch, tid, carry, L);
	__syncthreads();
	rs_wg_slot(R, S, blockIdx.x, ch, tid, taps, part, out, L);
}

/* ================================================================================================ host */

struct jsmpeg_hip_resampler_t {
	jsmpeg_hip_resampler_config_t cfg;
	JmPass pass{ "resampler: a pass is in flight: jsmpeg_hip_resampler_sync (or a reader) settles it first", "resampler: nothing was resampled yet" };
	RsRule R;
	uint64_t cap = 0;                                          /* of d_out: elements (WAVEFORM) or frames (FRAMES) */
	float *d_taps = nullptr, *d_carry = nullptr, *d_part = nullptr;
	RsStream *d_streams = nullptr, *h_streams = nullptr;       /* h_: pinned */
	void *d_out = nullptr;
	std::vector<RsChain> chain;                                /* per stream number */
	std::vector<uint64_t> offset, count, o_list, c_list;       /* per stream number; per listed stream */
	uint64_t total = 0;
};                                                             /* pass.ev[1]: behind the upload */

static size_t rs_elem_bytes(const RsRule &R) { return R.form == RS_FORM_FRAMES ? sizeof(float) * 2 * RS_FRAME : (R.dtype == RS_F32 ? 4 : 2); }

static void rs_free(jsmpeg_hip_resampler_t *r) {
	if (!r) return;
	jm_pass_close(r->pass);
	hipFree(r->d_taps); hipFree(r->d_carry); hipFree(r->d_part); hipFree(r->d_streams); hipFree(r->d_out);
	if (r->h_streams) hipHostFree(r->h_streams);
	delete r;
}

static int rs_alloc(jsmpeg_hip_resampler_t *r) {
	const size_t ns = r->cfg.max_streams, nt = (size_t)r->R.L * (size_t)r->R.taps;
	std::vector<float> taps(nt);
	rs_taps_make(r->R.in_rate, r->R.out_rate, taps.data());
	HIP_TRY(jm_malloc(&r->d_taps, sizeof(float) * nt));
	HIP_TRY(hipMemcpy(r->d_taps, taps.data(), sizeof(float) * nt, hipMemcpyHostToDevice));
	HIP_TRY(jm_malloc(&r->d_carry, sizeof(float) * RS_CARRY_FLOATS * ns));
	HIP_TRY(hipMemset(r->d_carry, 0, sizeof(float) * RS_CARRY_FLOATS * ns));
	HIP_TRY(jm_malloc(&r->d_part, sizeof(float) * RS_PART_FLOATS * ns));
	HIP_TRY(hipMemset(r->d_part, 0, sizeof(float) * RS_PART_FLOATS * ns));
	HIP_TRY(jm_malloc(&r->d_streams, sizeof(RsStream) * ns));
	HIP_TRY(hipHostMalloc(reinterpret_cast<void **>(&r->h_streams), sizeof(RsStream) * ns, hipHostMallocDefault));
	HIP_TRY(jm_malloc(reinterpret_cast<uint8_t **>(&r->d_out), (size_t)r->cap * rs_elem_bytes(r->R)));
	if (jm_pass_events(r->pass) < 0) return -1;
	HIP_TRY(hipDeviceSynchronize());
	return 0;
}

extern "C" int jsmpeg_hip_resample_plan(uint32_t in_rate, uint32_t out_rate, uint32_t *L, uint32_t *M, uint32_t *H) {
	g_err[0] = 0;
	int l, m, h;
	if (in_rate > 0x7fffffffu || out_rate > 0x7fffffffu || rs_plan((int)in_rate, (int)out_rate, &l, &m, &h) != 0)
		return fail("resampler: %u -> %u Hz is not a supported pair (in 32000 / 44100 / 48000, out 8000 / 16000 / 22050 / 24000 / 32000 / 44100 / 48000, out != in)", in_rate, out_rate);
	if (L) *L = (uint32_t)l;
	if (M) *M = (uint32_t)m;
	if (H) *H = (uint32_t)h;
	return 0;
}

extern "C" int jsmpeg_hip_resample_taps(uint32_t in_rate, uint32_t out_rate, float *out) {
	if (jsmpeg_hip_resample_plan(in_rate, out_rate, nullptr, nullptr, nullptr) < 0) return -1;
	if (!out) return fail("resampler: NULL out");
	return rs_taps_make((int)in_rate, (int)out_rate, out);
}

extern "C" jsmpeg_hip_resampler_t *jsmpeg_hip_resampler_create(const jsmpeg_hip_resampler_config_t *config) {
	g_err[0] = 0;
	if (!config) { fail("jsmpeg_hip_resampler_create: NULL config"); return nullptr; }
	if (jsmpeg_hip_resample_plan(config->in_rate, config->out_rate, nullptr, nullptr, nullptr) < 0) return nullptr;
	if (config->max_streams < 1 || config->max_frames < 1) { fail("resampler: max_streams and max_frames must be >= 1"); return nullptr; }
	if (!(config->gain == config->gain) || config->gain - config->gain != 0.0f) { fail("resampler: gain is not finite"); return nullptr; }
	RsRule R;
	if (rs_rule_make((int)config->in_rate, (int)config->out_rate, (int)config->channels_out, (int)config->form, (int)config->dtype, config->gain, 0, &R) != 0) {
		fail("resampler: channels_out %u, form %u, dtype %u: channels_out is 1 or 2, form WAVEFORM or FRAMES, dtype F32, F16 or BF16 (FRAMES: F32)",
		     config->channels_out, config->form, config->dtype);
		return nullptr;
	}
	if ((RS_WG - 1) * R.M / R.L + 1 + R.taps > RS_SPAN || R.carry > RS_MAX_CARRY || R.L * R.taps > RS_MAX_TAPS) { fail("resampler: the plan does not fit the kernel's LDS"); return nullptr; }
	/* what one stream yields from max_frames frames and END's tail: the default row, and the bound of a call's outputs */
	const uint64_t most = rs_outputs(R, (uint64_t)config->max_frames * RS_FRAME + (uint64_t)R.H);
	uint64_t cap;
	if (R.form == RS_FORM_WAVEFORM) {
		const uint64_t row = config->row ? config->row : most;
		if (row > 0x7fffffffull) { fail("resampler: row %llu is above 2^31 - 1", (unsigned long long)row); return nullptr; }
		R.row = (uint32_t)row;
		cap = (uint64_t)config->max_streams * (uint64_t)R.channels * row;
	} else {
		/* every stream completes at most (lead + count) / 1152 + 1 frames, lead < 1152, and the counts of a call add up to at
		 * most what max_frames frames and a tail per stream yield, rounded up per stream */
		cap = (rs_outputs(R, (uint64_t)config->max_frames * RS_FRAME + (uint64_t)R.H * config->max_streams) + config->max_streams) / RS_FRAME + 2ull * config->max_streams;
	}
	if (jsmpeg_hip_device_count() <= 0) { fail("no HIP device available: the resampler has no CPU fallback"); return nullptr; }
	jsmpeg_hip_resampler_t *r = new jsmpeg_hip_resampler_t();
	r->cfg = *config;
	r->R = R;
	r->cap = cap;
	if (jm_pass_open(r->pass, config->device) < 0) { delete r; return nullptr; }
	r->chain.assign(config->max_streams, RsChain{ 0, 0, 0, 0 });
	r->offset.assign(config->max_streams, 0); r->count.assign(config->max_streams, 0);
	r->o_list.resize(config->max_streams); r->c_list.resize(config->max_streams);
	if (rs_alloc(r) != 0) { rs_free(r); return nullptr; }
	return r;
}

extern "C" void jsmpeg_hip_resampler_destroy(jsmpeg_hip_resampler_t *r) { rs_free(r); }

extern "C" int jsmpeg_hip_resampler_resample(jsmpeg_hip_resampler_t *r, const void *const *pcm, const uint32_t *frames, const uint32_t *stream_numbers,
                                             uint32_t n_streams, uint32_t flags, void *hip_stream) {
	g_err[0] = 0;
	if (!r) return fail("resampler: NULL handle");
	if (jm_pass_idle(r->pass) < 0) return -1;
	if (flags & ~(JSMPEG_HIP_RESAMPLE_END | JSMPEG_HIP_RESAMPLE_CHAIN)) return fail("resampler: unknown flags 0x%x", flags);
	if (n_streams > r->cfg.max_streams) return fail("resampler: %u streams > max_streams %u", n_streams, r->cfg.max_streams);
	if (n_streams && (!pcm || !frames)) return fail("resampler: NULL pcm or frames");
	if (jm_pass_check_streams("resampler", pcm, frames, stream_numbers, n_streams, r->cfg.max_streams) < 0) return -1;
	uint64_t in_frames = 0;
	for (uint32_t i = 0; i < n_streams; i++) in_frames += frames[i];
	if (in_frames > r->cfg.max_frames) return fail("resampler: %llu frames > max_frames %u", (unsigned long long)in_frames, r->cfg.max_frames);
	uint64_t total = 0;
	const int rc = rs_plan_call(r->R, reinterpret_cast<const float *const *>(pcm), frames, stream_numbers, n_streams, flags, r->chain.data(), r->h_streams,
	                            r->o_list.data(), r->c_list.data(), &total);
	if (rc <= -1000001) return fail("resampler: stream %d of the call has %u frames: more than the 32-bit arithmetic of a call takes", -1000001 - rc, frames[-1000001 - rc]);
	if (rc < 0) return fail("resampler: stream %d of the call yields %u samples, row is %u: nothing was enqueued", -1 - rc, r->h_streams[-1 - rc].count, r->R.row);
	if (total > r->cap) return fail("resampler: the call yields %llu frames, the buffer holds %llu: nothing was enqueued", (unsigned long long)total, (unsigned long long)r->cap);
	uint32_t slots = 0;
	for (uint32_t i = 0; i < n_streams; i++) slots = std::max(slots, r->h_streams[i].slots);
	hipStream_t st = (hipStream_t)hip_stream;
	if (jm_pass_begin(r->pass, st) < 0) return -1;
	if (slots) HIP_TRY(hipMemcpyAsync(r->d_streams, r->h_streams, sizeof(RsStream) * n_streams, hipMemcpyHostToDevice, st));
	if (jm_pass_mark(r->pass, st) < 0) return -1;
	if (slots) {
		hipLaunchKernelGGL(k_resample, dim3((slots + RS_WG - 1) / RS_WG, (uint32_t)r->R.channels, n_streams), dim3(RS_WG), 0, st, r->R, r->d_streams, r->d_taps,
		                   r->d_carry, r->d_part, r->d_out);
		HIP_TRY(hipGetLastError());
	}
	if (jm_pass_end(r->pass, st) < 0) return -1;
	std::fill(r->offset.begin(), r->offset.end(), 0); std::fill(r->count.begin(), r->count.end(), 0);
	for (uint32_t i = 0; i < n_streams; i++) {
		const uint32_t s = stream_numbers ? stream_numbers[i] : i;
		r->offset[s] = r->o_list[i]; r->count[s] = r->c_list[i];
	}
	rs_plan_commit(r->R, frames, stream_numbers, n_streams, flags, r->chain.data());
	r->total = total;
	r->pass.pending = true; r->pass.have_pass = true;
	return 0;
}

extern "C" int jsmpeg_hip_resampler_sync(jsmpeg_hip_resampler_t *r) {
	g_err[0] = 0;
	if (!r) return fail("resampler: NULL handle");
	return jm_pass_settle(r->pass);
}

extern "C" int jsmpeg_hip_resampler_query(jsmpeg_hip_resampler_t *r) {
	g_err[0] = 0;
	if (!r) return fail("resampler: NULL handle");
	return jm_pass_query(r->pass);
}

/* the address and the bytes are the plan's: answered without waiting, so that a consumer on the same HIP stream is enqueued
 * right behind the pass */
extern "C" void *jsmpeg_hip_resampler_out(jsmpeg_hip_resampler_t *r, uint64_t *bytes) {
	g_err[0] = 0;
	if (!r) { fail("resampler: NULL handle"); return nullptr; }
	if (jm_pass_have(r->pass) < 0) return nullptr;
	if (bytes) *bytes = r->total * rs_elem_bytes(r->R);
	return r->d_out;
}

/* closed form: answered from the plan, without waiting */
extern "C" int jsmpeg_hip_resampler_stream_out(jsmpeg_hip_resampler_t *r, uint32_t stream, uint64_t *offset, uint64_t *count) {
	g_err[0] = 0;
	if (!r) return fail("resampler: NULL handle");
	if (jm_pass_have(r->pass) < 0 || jm_pass_stream_bound("resampler", stream, r->cfg.max_streams) < 0) return -1;
	if (offset) *offset = r->offset[stream];
	if (count) *count = r->count[stream];
	return 0;
}

extern "C" int jsmpeg_hip_resampler_chain_reset(jsmpeg_hip_resampler_t *r, uint32_t stream) {
	g_err[0] = 0;
	if (!r) return fail("resampler: NULL handle");
	return jm_pass_chain_reset(r->pass, "resampler", r->chain, stream);
}

extern "C" int jsmpeg_hip_resampler_chain_info(jsmpeg_hip_resampler_t *r, uint32_t stream, uint64_t out[3]) {
	g_err[0] = 0;
	if (!r) return fail("resampler: NULL handle");
	if (!out) return fail("resampler: NULL out");
	if (jm_pass_stream_bound("resampler", stream, r->cfg.max_streams) < 0) return -1;
	const RsChain &c = r->chain[stream];
	out[0] = c.have; out[1] = c.have ? c.n_in : 0; out[2] = c.have ? c.n_out : 0;
	return 0;
}

extern "C" int jsmpeg_hip_resampler_timings(jsmpeg_hip_resampler_t *r, float out_ms[2]) {
	g_err[0] = 0;
	if (!r) return fail("resampler: NULL handle");
	if (jm_pass_ready(r->pass) < 0) return -1;
	if (!out_ms) return fail("resampler: NULL out_ms");
	if (jm_pass_elapsed(r->pass, 1, 2, &out_ms[0]) < 0) return -1;
	return jm_pass_elapsed(r->pass, 0, 2, &out_ms[1]);
}
