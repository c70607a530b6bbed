/*
 * The MP2 (MPEG-1 Audio Layer II) ENCODER on the device: the gfx950 kernel and the host runtime behind part 9 of
 * include/jsmpeg_hip.h.  PCM in HBM (the decoder's own [frame][2][1152] float32) -> Layer II frames in a device buffer.
 *
 * The rule, the per-lane bodies and the host's plan: mp2_enc.h, shared with the test-only simulator.  Frame lengths are closed
 * form at constant bit rate, so nothing is scanned: the host knows every offset at enqueue time, every frame is one workgroup
 * of ONE kernel, and everything between the PCM and the frame's bytes stays in LDS.  No audio arithmetic happens on the host.
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
#include "mp2_enc.h"
#include "ts_prog_sources.h"

/* ================================================================================================ kernel */

/* the largest value of the wavefront, in every lane: quad swaps, then the mirrors inside a row of 16 (DPP), then the four rows
 * through scalar registers.  All 64 lanes are active where it is called. */
__device__ __forceinline__ uint32_t mp2e_wave_max(uint32_t key) {
	int v = (int)key;                                      /* keys are below 2^31 */
	v = max(v, __builtin_amdgcn_update_dpp(v, v, 0xb1, 0xf, 0xf, false));     /* quad_perm [1, 0, 3, 2] */
	v = max(v, __builtin_amdgcn_update_dpp(v, v, 0x4e, 0xf, 0xf, false));     /* quad_perm [2, 3, 0, 1] */
	v = max(v, __builtin_amdgcn_update_dpp(v, v, 0x141, 0xf, 0xf, false));    /* row_half_mirror */
	v = max(v, __builtin_amdgcn_update_dpp(v, v, 0x140, 0xf, 0xf, false));    /* row_mirror */
	const int a = __builtin_amdgcn_readlane(v, 0), b = __builtin_amdgcn_readlane(v, 16);
	const int c = __builtin_amdgcn_readlane(v, 32), d = __builtin_amdgcn_readlane(v, 48);
	return (uint32_t)max(max(a, b), max(c, d));
}

/* workgroup = frame of the call.  LDS: sizeof(Mp2EncLds), about 33 KB -- the samples as int16, one part's Y, all of S, the
 * side information and the frame's image. */
__global__ void __launch_bounds__(MP2E_WG) k_mp2e_frame(Mp2EncRule R, const Mp2EncFrame *frames, const Mp2EncTables *tables, int16_t *carry,
                                                       uint8_t *out, uint32_t *stats) {
	__shared__ Mp2EncLds L;
	const int tid = (int)threadIdx.x;
	const Mp2EncFrame F = frames[blockIdx.x];
	mp2e_wg_stage(R, F, tables, carry, tid, L);
	__syncthreads();
	mp2e_wg_carry_out(R, F, carry, tid, L);
	for (int part = 0; part < 3; part++) {
		mp2e_wg_window(R, part, tid, L);
		__syncthreads();
		mp2e_wg_matrix(R, part, tid, L);
		__syncthreads();
	}
	mp2e_wg_scale(R, tid, L);
	__syncthreads();
	if (tid < 64) {                                        /* ONE wavefront: lane = pair, a round = one wave-wide maximum */
		Mp2EncPair P = mp2e_pair_begin(R, tid, L);
		int left = mp2e_left_begin(R, F);
		mp2e_alloc_table(R, P, tid, L);                    /* (the lane's own column: no barrier) */
		for (int round = 0; round < MP2E_MAX_ROUNDS; round++) {
			const uint32_t key = mp2e_alloc_pick(L, tid, P.code, left);
			const uint32_t best = mp2e_wave_max(key);
			if (!best) break;
			if (key == best) P.code++;
			left -= (int)(best & MP2E_KEY_COST);
		}
		mp2e_pair_end(R, P, tid, left, L);
	}
	__syncthreads();
	if (tid < 64) mp2e_wg_side(R, F, tid, L);
	__syncthreads();
	mp2e_wg_quantise(tid, L);
	__syncthreads();
	mp2e_wg_store(F, out, tid, L);
	if (tid == 0) mp2e_wg_stats(F, stats + 4 * (size_t)blockIdx.x, L);
}

/* ================================================================================================ host */

struct jsmpeg_hip_mp2_encoder_t {
	jsmpeg_hip_mp2_encoder_config_t cfg;
	JmPass pass{ "MP2 encoder: an encode is in flight: jsmpeg_hip_mp2_encoder_sync (or a reader) settles it first", "MP2 encoder: nothing was encoded yet" };
	Mp2EncRule R;
	Mp2EncTables *d_tables = nullptr;
	Mp2EncFrame *d_frames = nullptr, *h_frames = nullptr;      /* h_: pinned */
	int16_t *d_carry = nullptr;
	uint8_t *d_es = nullptr;
	uint32_t *d_stats = nullptr, *h_stats = nullptr;
	std::vector<Mp2EncChain> chain;                            /* per stream number */
	std::vector<uint64_t> begin, end, b_list, e_list;          /* per stream number; per listed stream */
	std::vector<uint64_t> ordinal;                             /* per frame of the last call: its ordinal in its stream (ts_prog_sources.h) */
	uint32_t count = 0;                                        /* frames of the last call */
	uint64_t total = 0;
};                                                             /* pass.ev[1]: behind the kernel */

static void mp2e_free(jsmpeg_hip_mp2_encoder_t *e) {
	if (!e) return;
	jm_pass_close(e->pass);
	hipFree(e->d_tables); hipFree(e->d_frames); hipFree(e->d_carry); hipFree(e->d_es); hipFree(e->d_stats);
	if (e->h_frames) hipHostFree(e->h_frames);
	if (e->h_stats) hipHostFree(e->h_stats);
	delete e;
}

static int mp2e_alloc(jsmpeg_hip_mp2_encoder_t *e) {
	Mp2EncTables T;
	mp2e_tables_make(&T);
	const size_t nf = e->cfg.max_frames, ns = e->cfg.max_streams;
	HIP_TRY(jm_malloc(&e->d_tables, sizeof(T)));
	HIP_TRY(hipMemcpy(e->d_tables, &T, sizeof(T), hipMemcpyHostToDevice));
	HIP_TRY(jm_malloc(&e->d_frames, sizeof(Mp2EncFrame) * nf));
	HIP_TRY(hipHostMalloc(reinterpret_cast<void **>(&e->h_frames), sizeof(Mp2EncFrame) * nf, hipHostMallocDefault));
	HIP_TRY(jm_malloc(&e->d_carry, sizeof(int16_t) * MP2E_CARRY_WORDS * ns));
	HIP_TRY(hipMemset(e->d_carry, 0, sizeof(int16_t) * MP2E_CARRY_WORDS * ns));
	HIP_TRY(jm_malloc(&e->d_es, ((size_t)e->cfg.max_es_bytes + 15) & ~(size_t)15));
	HIP_TRY(jm_malloc(&e->d_stats, sizeof(uint32_t) * 4 * nf));
	HIP_TRY(hipHostMalloc(reinterpret_cast<void **>(&e->h_stats), sizeof(uint32_t) * 4 * nf, hipHostMallocDefault));
	if (jm_pass_events(e->pass) < 0) return -1;
	HIP_TRY(hipDeviceSynchronize());
	return 0;
}

extern "C" jsmpeg_hip_mp2_encoder_t *jsmpeg_hip_mp2_encoder_create(const jsmpeg_hip_mp2_encoder_config_t *config) {
	g_err[0] = 0;
	if (!config) { fail("jsmpeg_hip_mp2_encoder_create: NULL config"); return nullptr; }
	Mp2EncRule R;
	if (mp2e_rule_make((int)config->sample_rate_index, (int)config->channels, (int)config->bitrate_index, &R) != 0) {
		fail("MP2 encoder: sample_rate_index %u, channels %u, bitrate_index %u: not a Layer II combination (indices 0..2 / 1..14; no 32, 48, 56, 80 kbit/s "
		     "with two channels, no 224 .. 384 with one)", config->sample_rate_index, config->channels, config->bitrate_index);
		return nullptr;
	}
	if (config->max_streams < 1 || config->max_frames < 1 || config->max_es_bytes < 16) { fail("MP2 encoder: max_streams, max_frames must be >= 1 and max_es_bytes >= 16"); return nullptr; }
	if (config->max_es_bytes > 0xffffffffull) { fail("MP2 encoder: max_es_bytes above 4 GiB (jsmpeg_hip_mp2_batch_upload_device takes 32-bit ranges)"); return nullptr; }
	if (jsmpeg_hip_device_count() <= 0) { fail("no HIP device available: the MP2 encode path has no CPU fallback"); return nullptr; }
	jsmpeg_hip_mp2_encoder_t *e = new jsmpeg_hip_mp2_encoder_t();
	e->cfg = *config;
	e->R = R;
	if (jm_pass_open(e->pass, config->device) < 0) { delete e; return nullptr; }
	e->chain.assign(config->max_streams, Mp2EncChain{ 0, 0, 0 });
	e->begin.assign(config->max_streams, 0); e->end.assign(config->max_streams, 0);
	e->b_list.resize(config->max_streams); e->e_list.resize(config->max_streams);
	if (mp2e_alloc(e) != 0) { mp2e_free(e); return nullptr; }
	return e;
}

extern "C" void jsmpeg_hip_mp2_encoder_destroy(jsmpeg_hip_mp2_encoder_t *e) { mp2e_free(e); }

extern "C" int jsmpeg_hip_mp2_encoder_encode(jsmpeg_hip_mp2_encoder_t *e, const void *const *pcm, const uint32_t *frames, const uint32_t *stream_numbers,
                                             uint32_t n_streams, uint32_t flags, void *hip_stream) {
	g_err[0] = 0;
	if (!e) return fail("MP2 encoder: NULL handle");
	if (jm_pass_idle(e->pass) < 0) return -1;
	if (flags & ~(JSMPEG_HIP_MP2_ENC_END | JSMPEG_HIP_MP2_ENC_CHAIN)) return fail("MP2 encoder: unknown flags 0x%x", flags);
	if (n_streams > e->cfg.max_streams) return fail("MP2 encoder: %u streams > max_streams %u", n_streams, e->cfg.max_streams);
	if (n_streams && (!pcm || !frames)) return fail("MP2 encoder: NULL pcm or frames");
	if (jm_pass_check_streams("MP2 encoder", pcm, frames, stream_numbers, n_streams, e->cfg.max_streams) < 0) return -1;
	uint64_t count = 0;
	for (uint32_t i = 0; i < n_streams; i++) count += frames[i];
	if (count > e->cfg.max_frames) return fail("MP2 encoder: %llu frames > max_frames %u", (unsigned long long)count, e->cfg.max_frames);
	const uint64_t total = mp2e_plan(e->R, reinterpret_cast<const float *const *>(pcm), frames, stream_numbers, n_streams, flags, e->chain.data(), e->h_frames,
	                                 e->b_list.data(), e->e_list.data());
	if (total > e->cfg.max_es_bytes)
		return fail("MP2 encoder: the call's streams need %llu bytes, max_es_bytes is %llu: nothing was enqueued", (unsigned long long)total, (unsigned long long)e->cfg.max_es_bytes);
	hipStream_t st = (hipStream_t)hip_stream;
	if (jm_pass_begin(e->pass, st) < 0) return -1;
	if (count) {
		HIP_TRY(hipMemcpyAsync(e->d_frames, e->h_frames, sizeof(Mp2EncFrame) * count, hipMemcpyHostToDevice, st));
		hipLaunchKernelGGL(k_mp2e_frame, dim3((uint32_t)count), dim3(MP2E_WG), 0, st, e->R, e->d_frames, e->d_tables, e->d_carry, e->d_es, e->d_stats);
		HIP_TRY(hipGetLastError());
	}
	if (jm_pass_mark(e->pass, st) < 0) return -1;
	if (count) HIP_TRY(hipMemcpyAsync(e->h_stats, e->d_stats, sizeof(uint32_t) * 4 * count, hipMemcpyDeviceToHost, st));
	if (jm_pass_end(e->pass, st) < 0) return -1;
	std::fill(e->begin.begin(), e->begin.end(), 0); std::fill(e->end.begin(), e->end.end(), 0);
	for (uint32_t i = 0; i < n_streams; i++) {
		const uint32_t s = stream_numbers ? stream_numbers[i] : i;
		e->begin[s] = e->b_list[i]; e->end[s] = e->e_list[i];
	}
	e->ordinal.clear();
	for (uint32_t i = 0; i < n_streams; i++) {
		const Mp2EncChain &c = e->chain[stream_numbers ? stream_numbers[i] : i];
		const uint64_t n0 = ((flags & JSMPEG_HIP_MP2_ENC_CHAIN) && c.have) ? c.n : 0;          /* as mp2e_plan continues the stream */
		for (uint32_t k = 0; k < frames[i]; k++) e->ordinal.push_back(n0 + k);
	}
	mp2e_plan_commit(frames, stream_numbers, n_streams, flags, e->chain.data());
	if ((flags & JSMPEG_HIP_MP2_ENC_CHAIN) && (flags & JSMPEG_HIP_MP2_ENC_END))
		for (uint32_t i = 0; i < n_streams; i++) e->chain[stream_numbers ? stream_numbers[i] : i] = Mp2EncChain{ 0, 0, 0 };
	e->count = (uint32_t)count; e->total = total;
	e->pass.pending = true; e->pass.have_pass = true;
	return 0;
}

extern "C" int jsmpeg_hip_mp2_encoder_sync(jsmpeg_hip_mp2_encoder_t *e) {
	g_err[0] = 0;
	if (!e) return fail("MP2 encoder: NULL handle");
	return jm_pass_settle(e->pass);
}

extern "C" int jsmpeg_hip_mp2_encoder_query(jsmpeg_hip_mp2_encoder_t *e) {
	g_err[0] = 0;
	if (!e) return fail("MP2 encoder: NULL handle");
	return jm_pass_query(e->pass);
}

/* the readers of the device's results: settle, then refuse a handle without a pass */
static int mp2e_ready(jsmpeg_hip_mp2_encoder_t *e) {
	g_err[0] = 0;
	if (!e) return fail("MP2 encoder: NULL handle");
	return jm_pass_ready(e->pass);
}

extern "C" void *jsmpeg_hip_mp2_encoder_es(jsmpeg_hip_mp2_encoder_t *e, uint64_t *total_bytes) {
	if (mp2e_ready(e) < 0) return nullptr;
	if (total_bytes) *total_bytes = e->total;
	return e->d_es;
}

/* closed form: answered from the plan, without waiting */
extern "C" int jsmpeg_hip_mp2_encoder_stream_range(jsmpeg_hip_mp2_encoder_t *e, uint32_t stream, uint64_t *begin, uint64_t *end) {
	g_err[0] = 0;
	if (!e) return fail("MP2 encoder: NULL handle");
	if (jm_pass_have(e->pass) < 0 || jm_pass_stream_bound("MP2 encoder", stream, e->cfg.max_streams) < 0) return -1;
	if (begin) *begin = e->begin[stream];
	if (end) *end = e->end[stream];
	return 0;
}

extern "C" int jsmpeg_hip_mp2_encoder_frame_range(jsmpeg_hip_mp2_encoder_t *e, uint32_t k, uint64_t *offset, uint32_t *bytes) {
	g_err[0] = 0;
	if (!e) return fail("MP2 encoder: NULL handle");
	if (jm_pass_have(e->pass) < 0) return -1;
	if (k >= e->count) return fail("MP2 encoder: frame %u of %u", k, e->count);
	if (offset) *offset = e->h_frames[k].out;
	if (bytes) *bytes = e->h_frames[k].bytes;
	return 0;
}

extern "C" int64_t jsmpeg_hip_mp2_encoder_read_es(jsmpeg_hip_mp2_encoder_t *e, uint32_t stream, void *host, uint64_t cap) {
	if (mp2e_ready(e) < 0) return -1;
	if (jm_pass_stream_bound("MP2 encoder", stream, e->cfg.max_streams) < 0) return -1;
	const uint64_t b = e->begin[stream], n = e->end[stream] - b, k = std::min(n, cap);
	if (k && host) {
		HIP_TRY(hipSetDevice(e->pass.device));
		HIP_TRY(hipMemcpy(host, e->d_es + b, k, hipMemcpyDeviceToHost));
	}
	return (int64_t)n;
}

extern "C" int jsmpeg_hip_mp2_encoder_frame_stats(jsmpeg_hip_mp2_encoder_t *e, uint32_t k, uint32_t out[4]) {
	if (mp2e_ready(e) < 0) return -1;
	if (k >= e->count) return fail("MP2 encoder: frame %u of %u", k, e->count);
	if (!out) return fail("MP2 encoder: NULL out");
	for (int i = 0; i < 4; i++) out[i] = e->h_stats[(size_t)k * 4 + i];
	return 0;
}

extern "C" int jsmpeg_hip_mp2_encoder_chain_reset(jsmpeg_hip_mp2_encoder_t *e, uint32_t stream) {
	g_err[0] = 0;
	if (!e) return fail("MP2 encoder: NULL handle");
	return jm_pass_chain_reset(e->pass, "MP2 encoder", e->chain, stream);
}

extern "C" int jsmpeg_hip_mp2_encoder_chain_info(jsmpeg_hip_mp2_encoder_t *e, uint32_t stream, uint64_t out[2]) {
	g_err[0] = 0;
	if (!e) return fail("MP2 encoder: NULL handle");
	if (!out) return fail("MP2 encoder: NULL out");
	if (jm_pass_stream_bound("MP2 encoder", stream, e->cfg.max_streams) < 0) return -1;
	out[0] = e->chain[stream].have; out[1] = e->chain[stream].have ? e->chain[stream].n : 0;
	return 0;
}

extern "C" int jsmpeg_hip_mp2_encoder_timings(jsmpeg_hip_mp2_encoder_t *e, float out_ms[2]) {
	if (mp2e_ready(e) < 0) return -1;
	if (!out_ms) return fail("MP2 encoder: NULL out_ms");
	if (jm_pass_elapsed(e->pass, 0, 1, &out_ms[0]) < 0) return -1;
	return jm_pass_elapsed(e->pass, 0, 2, &out_ms[1]);
}

/* ------------------------------------------------------------------ the last call as the program mux's audio source
 * (ts_prog_sources.h): closed form, so everything is the host's at enqueue time */
int jm_mp2e_tsp_source(jsmpeg_hip_mp2_encoder_t *e, JmTspAudioSource *out, uint64_t *offset, uint32_t *bytes, uint32_t *stream, uint64_t *ordinal, uint32_t cap) {
	if (!e) return fail("ts_program: NULL MP2 encoder");
	if (!e->pass.have_pass) return fail("ts_program: the MP2 encoder has not encoded anything yet");
	if (e->count > cap) return fail("ts_program: the MP2 encoder's last call has %u frames, max_audio_units is %u", e->count, cap);
	out->count = e->count; out->max_streams = e->cfg.max_streams; out->sample_rate = (uint32_t)e->R.fs; out->device = e->pass.device;
	out->d_es = e->d_es;
	for (uint32_t k = 0; k < e->count; k++) {
		offset[k] = e->h_frames[k].out; bytes[k] = e->h_frames[k].bytes; stream[k] = e->h_frames[k].stream; ordinal[k] = e->ordinal[k];
	}
	return 0;
}
