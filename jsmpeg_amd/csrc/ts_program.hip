/*
 * The TS PROGRAM MUX on the device (include/jsmpeg_hip.h part 10): video and audio units of many streams -> one transport stream
 * per stream number, PAT / PMT / PCR on request.  The rule and every per-lane step: ts_prog.h, shared with the test-only
 * simulator (tests/sim/sim_ts_prog.cpp).  Here: the two kernels, the handle, the pass as a pure enqueue, and the serial host mux.
 *
 *   k_tsp_plan    ONE workgroup, no lane walks the units (a batch call has some 17 k of them): a lane per unit finds its rank
 *                 in the merged order by binary search in the other table and reads the payload's first dword for the key
 *                 test; a workgroup scan over the merged units in chunks of 256 with a carry sums (PAT/PMT, video, audio, all)
 *                 packets; a second one over the stream numbers sums the streams' padded sizes; a last sweep leaves per
 *                 merged unit `first`, `at` and the counters of its first packet and of its PSI pair.  The streams' words
 *                 are staged and committed when the total fits.
 *   k_tsp_write   a fixed grid over (all packets) x 47 dwords: the merged unit by binary search on `first`, a PSI dword from
 *                 the template, a unit dword by jm_tsp_dword over the source buffer of the unit's kind; every output dword
 *                 has one owner and one plain store, consecutive lanes store consecutive dwords.
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
#include "ts_prog.h"
#include "ts_prog_sources.h"

/* ================================================================================================ kernels */

struct JmTspArgs {
	JmTspRule rule;
	const uint8_t *src_v, *src_a;    /* the bytes the units' offsets count from, per kind */
	const JmTsUnit *v, *a;           /* [n_v], [n_a] */
	uint32_t n_v, n_a, n_streams;
	JmTspPlaced *placed;             /* [n_v + n_a], merged order */
	uint32_t *rank;                  /* [n_v + n_a]: video units, then audio */
	uint32_t *work;                  /* [5][n_v + n_a]: scan 1's prefix, the flags */
	JmTspEdges *edges;               /* [n_streams] */
	uint32_t *state;                 /* [n_streams][5], from call to call */
	uint64_t *result;                /* total | status (1: above cap, 2: no ES) | packets | merged units | stream_begin[n_streams] | stream_end[n_streams] | staged, after (u32 [n_streams][5] each) */
	uint64_t cap;
	const uint32_t *tpl;             /* PAT, PMT: 47 dwords each */
	uint32_t *out;
	const uint64_t *es_result;       /* the video encoder's total | status, NULL without one */
};
JM_HD uint64_t *tsp_stream_begin(const JmTspArgs &t) { return t.result + 4; }
JM_HD uint64_t *tsp_stream_end(const JmTspArgs &t) { return t.result + 4 + t.n_streams; }
JM_HD uint32_t *tsp_staged(const JmTspArgs &t) { return (uint32_t *)(t.result + 4 + 2 * (size_t)t.n_streams); }
JM_HD uint32_t *tsp_after(const JmTspArgs &t) { return tsp_staged(t) + JM_TSP_STATE * (size_t)t.n_streams; }
JM_HD size_t tsp_result_bytes(uint32_t n_streams) { return 8 * (4 + 2 * (size_t)n_streams) + 4 * ((2 * JM_TSP_STATE * (size_t)n_streams + 1) & ~(size_t)1); }

__device__ __forceinline__ uint32_t tsp_shfl_up(uint32_t v, uint32_t d) { return (uint32_t)__shfl_up((int)v, d); }
__device__ __forceinline__ uint64_t tsp_shfl_up(uint64_t v, uint32_t d) {
	return ((uint64_t)tsp_shfl_up((uint32_t)(v >> 32), d) << 32) | tsp_shfl_up((uint32_t)v, d);
}
/* inclusive sum over the 256 lanes of the workgroup, every lane calls it; *sum: the workgroup's */
template <class T>
__device__ __forceinline__ T tsp_scan(T v, T *s_wave, T *sum) {
	const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
	for (uint32_t d = 1; d < 64u; d <<= 1) {
		const T up = tsp_shfl_up(v, d);
		if (lane >= d) v += up;
	}
	if (lane == 63u) s_wave[wave] = v;
	__syncthreads();
	T add = 0, all = 0;
	for (uint32_t w = 0; w < 4u; w++) { if (w < wave) add += s_wave[w]; all += s_wave[w]; }
	__syncthreads();
	*sum = all;
	return v + add;
}

__global__ void __launch_bounds__(256) k_tsp_plan(JmTspArgs t) {
	__shared__ uint32_t s_wave[4];
	__shared__ uint64_t s_wave64[4];
	__shared__ unsigned long long s_total;
	const uint32_t n = t.n_v + t.n_a, tid = threadIdx.x;
	uint64_t *sb = tsp_stream_begin(t), *se = tsp_stream_end(t);
	uint32_t *staged = tsp_staged(t), *after = tsp_after(t);
	if (t.es_result && t.es_result[1]) {                           /* after an ES overflow of the video encoder there is no program */
		for (uint32_t s = tid; s < t.n_streams; s += 256u) {
			sb[s] = 0; se[s] = 0;
			for (uint32_t i = 0; i < JM_TSP_STATE; i++) after[JM_TSP_STATE * s + i] = t.state[JM_TSP_STATE * s + i];
		}
		if (tid == 0) { t.result[0] = 0; t.result[1] = 2u; t.result[2] = 0; t.result[3] = 0; }
		return;
	}
	for (uint32_t s = tid; s < t.n_streams; s += 256u) {
		JmTspEdges z;
		for (int i = 0; i < 4; i++) { z.begin[i] = 0; z.end[i] = 0; }
		t.edges[s] = z;
	}
	if (tid == 0) s_total = 0;
	for (uint32_t i = tid; i < n; i += 256u) {
		const uint32_t kind = i >= t.n_v ? 1u : 0u;
		jm_tsp_step_place<JmTsFetchAligned>(t.rule, t.v, t.n_v, t.a, t.n_a, kind, kind ? i - t.n_v : i, t.src_v, t.placed, t.rank);
	}
	__syncthreads();
	/* scan 1: the merged units */
	uint32_t carry[4] = { 0, 0, 0, 0 };
	for (uint32_t base = 0; base < n; base += 256u) {
		const uint32_t m = base + tid;
		uint32_t c[4] = { 0, 0, 0, 0 }, e[4], flags = 0;
		if (m < n) flags = jm_tsp_step_count(t.rule, t.placed, m, t.state, c);
		for (int i = 0; i < 4; i++) {
			uint32_t sum;
			const uint32_t incl = tsp_scan(c[i], s_wave, &sum);
			e[i] = carry[i] + incl - c[i];
			carry[i] += sum;
		}
		if (m < n) {
			for (int i = 0; i < 4; i++) t.work[(size_t)i * n + m] = e[i];
			t.work[(size_t)4 * n + m] = flags;
			jm_tsp_step_edges(t.placed, m, n, e, c, t.edges);
		}
	}
	__syncthreads();
	/* scan 2: the stream numbers */
	uint64_t at = 0;
	for (uint32_t base = 0; base < t.n_streams; base += 256u) {
		const uint32_t s = base + tid;
		const uint64_t size = s < t.n_streams ? jm_tsp_stream_size(t.edges, s) : 0;
		uint64_t sum;
		const uint64_t incl = tsp_scan(size, s_wave64, &sum);
		if (s < t.n_streams) {
			const uint64_t end = jm_tsp_step_stream(s, at + incl - size, t.edges, t.state, sb, se, staged);
			if (end) atomicMax(&s_total, (unsigned long long)end);
		}
		at += sum;
	}
	__syncthreads();
	for (uint32_t m = tid; m < n; m += 256u) {
		uint32_t e[4];
		for (int i = 0; i < 4; i++) e[i] = t.work[(size_t)i * n + m];
		jm_tsp_step_final(t.placed, m, t.work[(size_t)4 * n + m], e, t.edges, t.state, sb);
	}
	const uint64_t total = s_total;
	const bool fits = total <= t.cap;
	__syncthreads();                                               /* the sweep above read the words the commit below replaces */
	if (tid == 0) { t.result[0] = total; t.result[1] = fits ? 0u : 1u; t.result[2] = carry[3]; t.result[3] = n; }
	for (uint32_t s = tid; s < t.n_streams; s += 256u) {
		if (fits) jm_tsp_commit(s, staged, t.state);
		for (uint32_t i = 0; i < JM_TSP_STATE; i++) after[JM_TSP_STATE * s + i] = t.state[JM_TSP_STATE * s + i];
	}
}

__global__ void __launch_bounds__(256) k_tsp_write(JmTspArgs t) {
	if (t.result[1]) return;
	const uint64_t dwords = t.result[2] * JM_TS_DWORDS;
	const uint32_t n = t.n_v + t.n_a;
	for (uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; g < dwords; g += (uint64_t)gridDim.x * blockDim.x) {
		uint64_t where;
		const uint32_t v = jm_tsp_output_dword<JmTsFetchAligned>(t.rule, t.v, t.a, t.placed, n, g, t.tpl, t.src_v, t.src_a, &where);
		t.out[where] = v;
	}
}
#define JM_TSP_WRITE_GRID 1024u

/* ================================================================================================ host: the tables */

static JmTspRule tsp_rule(const jsmpeg_hip_ts_program_config_t &c) {
	JmTspRule r;
	r.pid[0] = c.video_pid; r.pid[1] = c.audio_pid;
	r.sid[0] = c.video_stream_id ? c.video_stream_id : 0xE0u; r.sid[1] = c.audio_stream_id ? c.audio_stream_id : 0xC0u;
	r.pmt_pid = c.pmt_pid; r.flags = c.flags; r.pcr_lead = c.pcr_lead_90k;
	return r;
}

/* what create and the host mux refuse in a config */
static int tsp_check_config(const jsmpeg_hip_ts_program_config_t *c) {
	if (!c) return fail("ts_program: NULL config");
	if (c->max_streams < 1) return fail("ts_program: max_streams 0");
	if (c->video_pid > 0x1fff || c->audio_pid > 0x1fff || c->pmt_pid > 0x1fff) return fail("ts_program: a PID above 0x1fff");
	if (c->video_pid == JM_TSP_NO_PID && c->audio_pid == JM_TSP_NO_PID) return fail("ts_program: both kinds are absent (video_pid and audio_pid are 0x1fff)");
	if (c->video_pid == 0 || c->audio_pid == 0 || c->pmt_pid == 0) return fail("ts_program: PID 0 is the PAT's");
	if (c->pmt_pid == JM_TSP_NO_PID) return fail("ts_program: pmt_pid 0x1fff is the null PID");
	if (c->video_pid == c->audio_pid || c->video_pid == c->pmt_pid || c->audio_pid == c->pmt_pid) return fail("ts_program: video_pid, audio_pid and pmt_pid must differ");
	if (c->video_stream_id > 0xff || c->audio_stream_id > 0xff) return fail("ts_program: a stream id above 0xff");
	if (c->program_number > 0xffff || c->transport_stream_id > 0xffff) return fail("ts_program: program_number / transport_stream_id above 0xffff");
	if (c->flags & ~(JSMPEG_HIP_TSP_PSI | JSMPEG_HIP_TSP_PCR)) return fail("ts_program: unknown flags 0x%x", c->flags);
	return 0;
}

/* one table as the rule wants it: streams ascending and below max_streams, PTS non-decreasing within a stream, none of an
 * absent kind; `bytes` may be NULL (the device knows them) */
static int tsp_check_table(const char *what, uint32_t pid, const uint32_t *stream, const uint64_t *pts, uint32_t n, uint32_t max_streams) {
	if (n && pid == JM_TSP_NO_PID) return fail("ts_program: %u %s units, but the %s PID is 0x1fff (absent)", n, what, what);
	for (uint32_t i = 0; i < n; i++) {
		const uint32_t s = stream ? stream[i] : 0u;
		if (s >= max_streams) return fail("ts_program: %s stream[%u] = %u >= max_streams %u", what, i, s, max_streams);
		if (!i) continue;
		const uint32_t before = stream ? stream[i - 1] : 0u;
		if (s < before) return fail("ts_program: %s stream[] must ascend (stream[%u] = %u after %u)", what, i, s, before);
		if (s == before && pts[i] < pts[i - 1]) return fail("ts_program: %s pts[%u] is below pts[%u] of the same stream", what, i, i - 1);
	}
	return 0;
}

/* ================================================================================================ host: the handle */

struct jsmpeg_hip_ts_program_t {
	jsmpeg_hip_ts_program_config_t cfg;
	JmTspRule rule;
	JmPass pass{ "ts_program: a pass is in flight: jsmpeg_hip_ts_program_sync (or a reader) settles it first", "ts_program: nothing was muxed yet" };
	uint32_t max_units = 0;
	uint8_t *d_ts = nullptr;                                   /* the handle's own output */
	uint8_t *out = nullptr;                                    /* where the calls write: d_ts or the caller's */
	uint64_t out_cap = 0;
	JmTsUnit *d_units = nullptr, *h_units = nullptr;           /* video at 0, audio at max_video_units; h_: pinned */
	uint64_t *d_pts = nullptr, *h_pts = nullptr;               /* [max_video_units]: for the encoder's unit table; h_: pinned */
	uint8_t *d_back = nullptr, *h_back = nullptr;              /* result | rank | placed: what one copy brings back; h_: pinned */
	uint32_t *d_work = nullptr;
	JmTspEdges *d_edges = nullptr;
	uint32_t *d_state = nullptr, *d_tpl = nullptr;
	uint32_t n_v = 0, n_a = 0;                                 /* of the last call; pass.ev[1]: behind the kernels */
	std::vector<uint32_t> scratch_stream;
	std::vector<uint64_t> scratch_ord, scratch_off;
	std::vector<uint32_t> scratch_bytes, scratch_ord32;
};

static size_t tsp_rank_bytes(const jsmpeg_hip_ts_program_t *p) { return 4 * (((size_t)p->max_units + 1) & ~(size_t)1); }
static const uint64_t *tsp_h_result(const jsmpeg_hip_ts_program_t *p) { return reinterpret_cast<const uint64_t *>(p->h_back); }
static const uint32_t *tsp_h_rank(const jsmpeg_hip_ts_program_t *p) { return reinterpret_cast<const uint32_t *>(p->h_back + tsp_result_bytes(p->cfg.max_streams)); }
static const JmTspPlaced *tsp_h_placed(const jsmpeg_hip_ts_program_t *p) {
	return reinterpret_cast<const JmTspPlaced *>(p->h_back + tsp_result_bytes(p->cfg.max_streams) + tsp_rank_bytes(p));
}

static void tsp_free(jsmpeg_hip_ts_program_t *p) {
	if (!p) return;
	jm_pass_close(p->pass);
	hipFree(p->d_ts); hipFree(p->d_units); hipFree(p->d_pts); hipFree(p->d_back); hipFree(p->d_work); hipFree(p->d_edges); hipFree(p->d_state); hipFree(p->d_tpl);
	if (p->h_units) hipHostFree(p->h_units);
	if (p->h_pts) hipHostFree(p->h_pts);
	if (p->h_back) hipHostFree(p->h_back);
	delete p;
}

static int tsp_alloc(jsmpeg_hip_ts_program_t *p) {
	const size_t nu = std::max<size_t>(1, p->max_units), ns = p->cfg.max_streams, nv = std::max<size_t>(1, p->cfg.max_video_units);
	const size_t back = tsp_result_bytes(p->cfg.max_streams) + tsp_rank_bytes(p) + sizeof(JmTspPlaced) * nu;
	uint8_t psi[2 * JM_TS_PACKET];
	jm_tsp_psi_packets(p->rule, p->cfg.program_number, p->cfg.transport_stream_id, psi);
	HIP_TRY(jm_malloc(&p->d_ts, jm_ts_align16(p->cfg.max_ts_bytes) + 16));
	HIP_TRY(jm_malloc(&p->d_units, sizeof(JmTsUnit) * nu));
	HIP_TRY(hipHostMalloc(reinterpret_cast<void **>(&p->h_units), sizeof(JmTsUnit) * nu, hipHostMallocDefault));
	HIP_TRY(jm_malloc(&p->d_pts, sizeof(uint64_t) * nv));
	HIP_TRY(hipHostMalloc(reinterpret_cast<void **>(&p->h_pts), sizeof(uint64_t) * nv, hipHostMallocDefault));
	HIP_TRY(jm_malloc(&p->d_back, back));
	HIP_TRY(hipHostMalloc(reinterpret_cast<void **>(&p->h_back), back, hipHostMallocDefault));
	memset(p->h_back, 0, back);
	HIP_TRY(jm_malloc(&p->d_work, sizeof(uint32_t) * 5 * nu));
	HIP_TRY(jm_malloc(&p->d_edges, sizeof(JmTspEdges) * ns));
	HIP_TRY(jm_malloc(&p->d_state, sizeof(uint32_t) * JM_TSP_STATE * ns));
	HIP_TRY(hipMemset(p->d_state, 0, sizeof(uint32_t) * JM_TSP_STATE * ns));
	HIP_TRY(jm_malloc(&p->d_tpl, sizeof(psi)));
	HIP_TRY(hipMemcpy(p->d_tpl, psi, sizeof(psi), hipMemcpyHostToDevice));
	if (jm_pass_events(p->pass) < 0) return -1;
	HIP_TRY(hipDeviceSynchronize());
	p->out = p->d_ts; p->out_cap = p->cfg.max_ts_bytes;
	return 0;
}

extern "C" jsmpeg_hip_ts_program_t *jsmpeg_hip_ts_program_create(const jsmpeg_hip_ts_program_config_t *config) {
	g_err[0] = 0;
	if (tsp_check_config(config) < 0) return nullptr;
	if (config->max_video_units + (uint64_t)config->max_audio_units < 1 || config->max_video_units + (uint64_t)config->max_audio_units > 0x7fffffffu) {
		fail("ts_program: max_video_units + max_audio_units must be 1 .. 2^31 - 1"); return nullptr;
	}
	if (config->max_ts_bytes < JM_TS_PACKET || config->max_ts_bytes > 0xffffffffull * 4) { fail("ts_program: max_ts_bytes must be 188 .. 16 GiB"); return nullptr; }
	if (jsmpeg_hip_device_count() <= 0) { fail("no HIP device available: the TS program mux on the device has no CPU fallback (jsmpeg_hip_ts_program_mux_host)"); return nullptr; }
	jsmpeg_hip_ts_program_t *p = new jsmpeg_hip_ts_program_t();
	p->cfg = *config;
	p->rule = tsp_rule(*config);
	p->max_units = config->max_video_units + config->max_audio_units;
	if (jm_pass_open(p->pass, config->device) < 0) { delete p; return nullptr; }
	if (tsp_alloc(p) != 0) { tsp_free(p); return nullptr; }
	return p;
}

extern "C" void jsmpeg_hip_ts_program_destroy(jsmpeg_hip_ts_program_t *p) { tsp_free(p); }

extern "C" int jsmpeg_hip_ts_program_set_output(jsmpeg_hip_ts_program_t *p, void *dev_ts, uint64_t cap) {
	g_err[0] = 0;
	if (!p) return fail("ts_program: NULL handle");
	if (jm_pass_idle(p->pass) < 0) return -1;
	if ((uintptr_t)dev_ts & 3u) return fail("ts_program: dev_ts is not 4-byte aligned");
	if (dev_ts && cap > 0xffffffffull * 4) return fail("ts_program: cap above 16 GiB");
	p->out = dev_ts ? (uint8_t *)dev_ts : p->d_ts;
	p->out_cap = dev_ts ? cap : p->cfg.max_ts_bytes;
	return 0;
}

/* the pass behind the tables: d_units holds the video units at 0 (n_v) and the audio units at max_video_units (n_a) */
static int tsp_enqueue(jsmpeg_hip_ts_program_t *p, const uint8_t *src_v, const uint8_t *src_a, uint32_t n_v, uint32_t n_a, const uint64_t *es_result, hipStream_t st) {
	const uint32_t n = n_v + n_a;
	JmTspArgs t;
	t.rule = p->rule; t.src_v = src_v; t.src_a = src_a;
	t.v = p->d_units; t.a = p->d_units + p->cfg.max_video_units; t.n_v = n_v; t.n_a = n_a; t.n_streams = p->cfg.max_streams;
	t.result = reinterpret_cast<uint64_t *>(p->d_back);
	t.rank = reinterpret_cast<uint32_t *>(p->d_back + tsp_result_bytes(p->cfg.max_streams));
	t.placed = reinterpret_cast<JmTspPlaced *>(p->d_back + tsp_result_bytes(p->cfg.max_streams) + tsp_rank_bytes(p));
	t.work = p->d_work; t.edges = p->d_edges; t.state = p->d_state; t.cap = p->out_cap; t.tpl = p->d_tpl;
	t.out = reinterpret_cast<uint32_t *>(p->out); t.es_result = es_result;
	k_tsp_plan<<<dim3(1), dim3(256), 0, st>>>(t);
	k_tsp_write<<<dim3(JM_TSP_WRITE_GRID), dim3(256), 0, st>>>(t);
	HIP_TRY(hipGetLastError());
	if (jm_pass_mark(p->pass, st) < 0) return -1;
	HIP_TRY(hipMemcpyAsync(p->h_back, p->d_back, tsp_result_bytes(p->cfg.max_streams) + tsp_rank_bytes(p) + sizeof(JmTspPlaced) * n, hipMemcpyDeviceToHost, st));
	if (jm_pass_end(p->pass, st) < 0) return -1;
	p->n_v = n_v; p->n_a = n_a;
	p->pass.pending = true; p->pass.have_pass = true;
	return 0;
}

extern "C" int jsmpeg_hip_ts_program_mux(jsmpeg_hip_ts_program_t *p,
                                         const void *dev_video, const uint64_t *v_offset, const uint32_t *v_bytes, const uint32_t *v_stream, const uint64_t *v_pts, uint32_t n_v,
                                         const void *dev_audio, const uint64_t *a_offset, const uint32_t *a_bytes, const uint32_t *a_stream, const uint64_t *a_pts, uint32_t n_a,
                                         void *hip_stream) {
	g_err[0] = 0;
	if (!p) return fail("ts_program: NULL handle");
	if (jm_pass_idle(p->pass) < 0) return -1;
	if (n_v > p->cfg.max_video_units) return fail("ts_program: %u video units > max_video_units %u", n_v, p->cfg.max_video_units);
	if (n_a > p->cfg.max_audio_units) return fail("ts_program: %u audio units > max_audio_units %u", n_a, p->cfg.max_audio_units);
	if (n_v && (!dev_video || !v_offset || !v_bytes || !v_pts)) return fail("ts_program: NULL video argument");
	if (n_a && (!dev_audio || !a_offset || !a_bytes || !a_pts)) return fail("ts_program: NULL audio argument");
	if (tsp_check_table("video", p->rule.pid[0], v_stream, v_pts, n_v, p->cfg.max_streams) < 0) return -1;
	if (tsp_check_table("audio", p->rule.pid[1], a_stream, a_pts, n_a, p->cfg.max_streams) < 0) return -1;
	uint64_t payload = 0;
	for (uint32_t i = 0; i < n_v; i++) payload += v_bytes[i];
	for (uint32_t i = 0; i < n_a; i++) payload += a_bytes[i];
	if (payload > 0xffffffffull * 4) return fail("ts_program: the call's units hold more than 16 GiB");
	hipStream_t st = (hipStream_t)hip_stream;
	JmTsUnit *hv = p->h_units, *ha = p->h_units + p->cfg.max_video_units;
	for (uint32_t i = 0; i < n_v; i++) { hv[i].off = v_offset[i]; hv[i].bytes = v_bytes[i]; hv[i].stream = v_stream ? v_stream[i] : 0u; hv[i].pts = v_pts[i]; }
	for (uint32_t i = 0; i < n_a; i++) { ha[i].off = a_offset[i]; ha[i].bytes = a_bytes[i]; ha[i].stream = a_stream ? a_stream[i] : 0u; ha[i].pts = a_pts[i]; }
	if (jm_pass_begin(p->pass, st) < 0) return -1;
	if (n_v) HIP_TRY(hipMemcpyAsync(p->d_units, hv, sizeof(JmTsUnit) * n_v, hipMemcpyHostToDevice, st));
	if (n_a) HIP_TRY(hipMemcpyAsync(p->d_units + p->cfg.max_video_units, ha, sizeof(JmTsUnit) * n_a, hipMemcpyHostToDevice, st));
	return tsp_enqueue(p, (const uint8_t *)dev_video, (const uint8_t *)dev_audio, n_v, n_a, nullptr, st);
}

extern "C" int jsmpeg_hip_ts_program_mux_encoders(jsmpeg_hip_ts_program_t *p, jsmpeg_hip_encoder_t *enc, const uint64_t *v_pts,
                                                  jsmpeg_hip_mp2_encoder_t *mp2enc, const uint64_t *a_pts, void *hip_stream) {
	g_err[0] = 0;
	if (!p) return fail("ts_program: NULL handle");
	if (jm_pass_idle(p->pass) < 0) return -1;
	JmTspVideoSource vs;
	JmTspAudioSource as;
	memset(&vs, 0, sizeof(vs)); memset(&as, 0, sizeof(as));
	const uint32_t mv = p->cfg.max_video_units, ma = p->cfg.max_audio_units;
	p->scratch_stream.resize(std::max(mv, ma) + 1); p->scratch_ord32.resize(mv + 1);
	p->scratch_ord.resize(ma + 1); p->scratch_off.resize(ma + 1); p->scratch_bytes.resize(ma + 1);
	JmTsUnit *ha = p->h_units + mv;
	if (enc) {
		if (jm_enc_tsp_source(enc, &vs, p->scratch_stream.data(), p->scratch_ord32.data(), mv) < 0) return -1;
		if (vs.device != p->pass.device) return fail("ts_program: the encoder lives on device %d, the program handle on %d", vs.device, p->pass.device);
		uint32_t num, den;
		jm_ts_frame_rate(vs.frame_rate_code, &num, &den);
		for (uint32_t k = 0; k < vs.count; k++) p->h_pts[k] = v_pts ? v_pts[k] : (uint64_t)p->scratch_ord32[k] * 90000u * den / num;
		if (tsp_check_table("video", p->rule.pid[0], p->scratch_stream.data(), p->h_pts, vs.count, p->cfg.max_streams) < 0) return -1;
	}
	if (mp2enc) {
		if (jm_mp2e_tsp_source(mp2enc, &as, p->scratch_off.data(), p->scratch_bytes.data(), p->scratch_stream.data(), p->scratch_ord.data(), ma) < 0) return -1;
		if (as.device != p->pass.device) return fail("ts_program: the MP2 encoder lives on device %d, the program handle on %d", as.device, p->pass.device);
		for (uint32_t k = 0; k < as.count; k++) {
			ha[k].off = p->scratch_off[k]; ha[k].bytes = p->scratch_bytes[k]; ha[k].stream = p->scratch_stream[k];
			ha[k].pts = a_pts ? a_pts[k] : p->scratch_ord[k] * 1152u * 90000u / as.sample_rate;
		}
		for (uint32_t k = 0; k < as.count; k++) { p->scratch_stream[k] = ha[k].stream; p->scratch_ord[k] = ha[k].pts; }
		if (tsp_check_table("audio", p->rule.pid[1], p->scratch_stream.data(), p->scratch_ord.data(), as.count, p->cfg.max_streams) < 0) return -1;
	}
	hipStream_t st = (hipStream_t)hip_stream;
	if (jm_pass_begin(p->pass, st) < 0) return -1;
	if (vs.count) {
		HIP_TRY(hipMemcpyAsync(p->d_pts, p->h_pts, sizeof(uint64_t) * vs.count, hipMemcpyHostToDevice, st));
		if (jm_enc_tsp_units(enc, p->d_units, p->d_pts, hip_stream) < 0) return -1;
	}
	if (as.count) HIP_TRY(hipMemcpyAsync(p->d_units + mv, ha, sizeof(JmTsUnit) * as.count, hipMemcpyHostToDevice, st));
	return tsp_enqueue(p, vs.d_es, as.d_es, vs.count, as.count, vs.count ? vs.d_result : nullptr, st);
}

/* settles, then the verdict of the last call */
static int tsp_ready(jsmpeg_hip_ts_program_t *p) {
	g_err[0] = 0;
	if (!p) return fail("ts_program: NULL handle");
	if (jm_pass_ready(p->pass) < 0) return -1;
	const uint64_t *r = tsp_h_result(p);
	if (r[1] == 1) return fail("ts_program: the call needs %llu bytes, the output holds %llu: nothing was written, the state stays", (unsigned long long)r[0], (unsigned long long)p->out_cap);
	if (r[1] == 2) return fail("ts_program: the video encoder's call overflowed its max_es_bytes: there is no program, the state stays");
	return 0;
}

extern "C" int jsmpeg_hip_ts_program_sync(jsmpeg_hip_ts_program_t *p) {
	if (!p) { g_err[0] = 0; return fail("ts_program: NULL handle"); }
	if (!p->pass.have_pass) { g_err[0] = 0; return 0; }
	return tsp_ready(p);
}

extern "C" int jsmpeg_hip_ts_program_query(jsmpeg_hip_ts_program_t *p) {
	g_err[0] = 0;
	if (!p) return fail("ts_program: NULL handle");
	return jm_pass_query(p->pass);
}

extern "C" void *jsmpeg_hip_ts_program_ts(jsmpeg_hip_ts_program_t *p, uint64_t *total_bytes) {
	if (tsp_ready(p) < 0) return nullptr;
	if (total_bytes) *total_bytes = tsp_h_result(p)[0];
	return p->out;
}

extern "C" int jsmpeg_hip_ts_program_stream_range(jsmpeg_hip_ts_program_t *p, uint32_t stream, uint64_t *begin, uint64_t *end) {
	if (tsp_ready(p) < 0) return -1;
	if (jm_pass_stream_bound("ts_program", stream, p->cfg.max_streams) < 0) return -1;
	if (begin) *begin = tsp_h_result(p)[4 + stream];
	if (end) *end = tsp_h_result(p)[4 + p->cfg.max_streams + stream];
	return 0;
}

extern "C" int jsmpeg_hip_ts_program_unit_range(jsmpeg_hip_ts_program_t *p, uint32_t kind, uint32_t k, uint64_t *offset, uint32_t *bytes, uint32_t *psi_bytes) {
	if (tsp_ready(p) < 0) return -1;
	if (kind > 1u) return fail("ts_program: kind %u, must be 0 (video) or 1 (audio)", kind);
	if (k >= (kind ? p->n_a : p->n_v)) return fail("ts_program: %s unit %u of %u", kind ? "audio" : "video", k, kind ? p->n_a : p->n_v);
	const JmTspPlaced &u = tsp_h_placed(p)[tsp_h_rank(p)[kind ? p->n_v + k : k]];
	const uint32_t psi = (u.cc & JM_TSP_P_PSI) ? 2u : 0u;
	if (offset) *offset = u.at;
	if (bytes) *bytes = (u.packets + psi) * JM_TS_PACKET;
	if (psi_bytes) *psi_bytes = psi * JM_TS_PACKET;
	return 0;
}

extern "C" int64_t jsmpeg_hip_ts_program_read(jsmpeg_hip_ts_program_t *p, uint32_t stream, void *host, uint64_t cap) {
	uint64_t b = 0, n = 0;
	if (stream == UINT32_MAX) {
		if (tsp_ready(p) < 0) return -1;
		n = tsp_h_result(p)[0];
	} else {
		if (jsmpeg_hip_ts_program_stream_range(p, stream, &b, &n) < 0) return -1;
		n -= b;
	}
	const uint64_t k = std::min(n, cap);
	if (k && host) {
		HIP_TRY(hipSetDevice(p->pass.device));
		HIP_TRY(hipMemcpy(host, p->out + b, k, hipMemcpyDeviceToHost));
	}
	return (int64_t)n;
}

/* the words behind the last call, whatever its verdict: a failed call left them where they were */
extern "C" int jsmpeg_hip_ts_program_state(jsmpeg_hip_ts_program_t *p, uint32_t stream, uint32_t out[5]) {
	g_err[0] = 0;
	if (!p) return fail("ts_program: NULL handle");
	if (!out) return fail("ts_program: NULL out");
	if (jm_pass_stream_bound("ts_program", stream, p->cfg.max_streams) < 0) return -1;
	if (jm_pass_settle(p->pass) < 0) return -1;
	const uint32_t *after = reinterpret_cast<const uint32_t *>(tsp_h_result(p) + 4 + 2 * (size_t)p->cfg.max_streams) + JM_TSP_STATE * (size_t)p->cfg.max_streams;
	for (uint32_t i = 0; i < JM_TSP_STATE; i++) out[i] = after[JM_TSP_STATE * stream + i];   /* (zeros before the first call; reset and set_state keep the copy current) */
	return 0;
}

extern "C" int jsmpeg_hip_ts_program_reset(jsmpeg_hip_ts_program_t *p, uint32_t stream) {
	g_err[0] = 0;
	if (!p) return fail("ts_program: NULL handle");
	if (jm_pass_idle(p->pass) < 0) return -1;
	if (stream != UINT32_MAX && jm_pass_stream_bound("ts_program", stream, p->cfg.max_streams) < 0) return -1;
	HIP_TRY(hipSetDevice(p->pass.device));
	const size_t ns = p->cfg.max_streams, first = stream == UINT32_MAX ? 0 : stream, count = stream == UINT32_MAX ? ns : 1;
	HIP_TRY(hipMemset(p->d_state + JM_TSP_STATE * first, 0, sizeof(uint32_t) * JM_TSP_STATE * count));
	HIP_TRY(hipDeviceSynchronize());
	uint32_t *after = reinterpret_cast<uint32_t *>(reinterpret_cast<uint64_t *>(p->h_back) + 4 + 2 * ns) + JM_TSP_STATE * ns;
	memset(after + JM_TSP_STATE * first, 0, sizeof(uint32_t) * JM_TSP_STATE * count);
	return 0;
}

extern "C" int jsmpeg_hip_ts_program_set_state(jsmpeg_hip_ts_program_t *p, uint32_t stream, const uint32_t in[5]) {
	g_err[0] = 0;
	if (!p) return fail("ts_program: NULL handle");
	if (!in) return fail("ts_program: NULL in");
	if (jm_pass_idle(p->pass) < 0) return -1;
	if (jm_pass_stream_bound("ts_program", stream, p->cfg.max_streams) < 0) return -1;
	for (uint32_t i = 0; i < JM_TSP_STATE; i++)
		if (in[i] > (i == 4u ? 1u : 15u)) return fail("ts_program: state word %u = %u (counters are 0 .. 15, started 0 or 1)", i, in[i]);
	HIP_TRY(hipSetDevice(p->pass.device));
	HIP_TRY(hipMemcpy(p->d_state + JM_TSP_STATE * (size_t)stream, in, sizeof(uint32_t) * JM_TSP_STATE, hipMemcpyHostToDevice));
	const size_t ns = p->cfg.max_streams;
	uint32_t *after = reinterpret_cast<uint32_t *>(reinterpret_cast<uint64_t *>(p->h_back) + 4 + 2 * ns) + JM_TSP_STATE * ns;
	memcpy(after + JM_TSP_STATE * (size_t)stream, in, sizeof(uint32_t) * JM_TSP_STATE);
	return 0;
}

extern "C" int jsmpeg_hip_ts_program_timings(jsmpeg_hip_ts_program_t *p, float out_ms[2]) {
	g_err[0] = 0;
	if (!p) return fail("ts_program: NULL handle");
	if (jm_pass_ready(p->pass) < 0) return -1;
	if (!out_ms) return fail("ts_program: NULL out_ms");
	if (jm_pass_elapsed(p->pass, 0, 1, &out_ms[0]) < 0) return -1;
	return jm_pass_elapsed(p->pass, 0, 2, &out_ms[1]);
}

extern "C" uint64_t jsmpeg_hip_ts_program_bound(uint64_t v_bytes, uint32_t n_v, uint64_t a_bytes, uint32_t n_a, uint32_t streams) {
	return jm_tsp_bound(v_bytes, n_v, a_bytes, n_a, streams);
}

extern "C" int jsmpeg_hip_ts_program_psi(const jsmpeg_hip_ts_program_config_t *config, uint8_t out[376]) {
	g_err[0] = 0;
	if (tsp_check_config(config) < 0) return -1;
	if (!out) return fail("ts_program: NULL out");
	jm_tsp_psi_packets(tsp_rule(*config), config->program_number, config->transport_stream_id, out);
	return 0;
}

/* ================================================================================================ host: the serial mux
 * No device and none of ts_prog.h's plan: a walk over the streams, a two-pointer merge of each stream's two lists, packets
 * written byte by byte in order.  What the kernels and the simulator are held to. */

struct TspHostTable { const uint8_t *src; const uint64_t *off; const uint32_t *bytes, *stream; const uint64_t *pts; uint32_t n; };

/* one unit's packets at `ts` (NULL: counted only); *cc: the PID's counter, in / out; returns the packets */
static uint32_t tsp_host_unit(const JmTspRule &r, uint32_t kind, const uint8_t *payload, uint32_t bytes, uint64_t pts, uint32_t *cc, uint8_t *ts) {
	const uint64_t total = 14 + (uint64_t)bytes;
	const bool sized = (uint64_t)bytes + 8 <= 0xffff, pcr = (r.flags & JM_TSP_PCR) && kind == (r.pid[0] != JM_TSP_NO_PID ? 0u : 1u);
	const uint64_t lead0 = pcr ? 8 : 0, lead = lead0 + ((!sized && (total + lead0) % 184 == 0) ? 1 : 0);
	const uint32_t packets = (uint32_t)((total + lead + 183) / 184);
	if (!ts) { *cc = (*cc + packets) & 15u; return packets; }
	const uint32_t plen = sized ? bytes + 8 : 0, pid = r.pid[kind];
	const uint64_t p = pts & 0x1ffffffffull, base = (pts - r.pcr_lead) & 0x1ffffffffull;
	const uint8_t head[14] = { 0, 0, 1, (uint8_t)r.sid[kind], (uint8_t)(plen >> 8), (uint8_t)plen, 0x80, 0x80, 5,
	                           (uint8_t)(0x21 | ((p >> 29) & 0x0e)), (uint8_t)(p >> 22), (uint8_t)(0x01 | ((p >> 14) & 0xfe)), (uint8_t)(p >> 7), (uint8_t)(0x01 | ((p << 1) & 0xfe)) };
	uint64_t done = 0;
	for (uint32_t k = 0; k < packets; k++, ts += 188) {
		const uint64_t left = total - done;
		uint64_t stuff = k == 0 ? lead : 0;
		if (left + stuff < 184) stuff = 184 - left;
		ts[0] = 0x47; ts[1] = (uint8_t)((k == 0 ? 0x40 : 0) | (pid >> 8)); ts[2] = (uint8_t)pid; ts[3] = (uint8_t)((stuff ? 0x30 : 0x10) | *cc);
		*cc = (*cc + 1) & 15u;
		uint8_t *w = ts + 4;
		if (stuff) {
			w[0] = (uint8_t)(stuff - 1);
			if (stuff > 1) { w[1] = (pcr && k == 0) ? 0x10 : 0x00; memset(w + 2, 0xff, stuff - 2); }
			if (pcr && k == 0) {
				w[2] = (uint8_t)(base >> 25); w[3] = (uint8_t)(base >> 17); w[4] = (uint8_t)(base >> 9); w[5] = (uint8_t)(base >> 1);
				w[6] = (uint8_t)(((base & 1) << 7) | 0x7e); w[7] = 0;
			}
			w += stuff;
		}
		for (uint64_t i = 0, m = 184 - stuff; i < m; i++, done++) w[i] = done < 14 ? head[done] : payload[done - 14];
	}
	return packets;
}

/* the whole call: ts NULL counts; state is advanced in place (the caller hands in a copy); returns the total */
static uint64_t tsp_host_walk(const JmTspRule &r, const uint8_t psi[2 * JM_TS_PACKET], const TspHostTable T[2], uint32_t max_streams, uint32_t *state,
                              uint8_t *ts, uint64_t *stream_begin, uint64_t *stream_end) {
	uint32_t at_unit[2] = { 0, 0 };
	uint64_t at = 0;
	for (uint32_t s = 0; s < max_streams; s++) {
		uint32_t end[2];
		for (int kind = 0; kind < 2; kind++) {
			end[kind] = at_unit[kind];
			while (end[kind] < T[kind].n && (T[kind].stream ? T[kind].stream[end[kind]] : 0u) == s) end[kind]++;
		}
		if (stream_begin) stream_begin[s] = 0;
		if (stream_end) stream_end[s] = 0;
		if (end[0] == at_unit[0] && end[1] == at_unit[1]) continue;
		at = (at + 15) & ~(uint64_t)15;
		if (stream_begin) stream_begin[s] = at;
		uint32_t *w = state + JM_TSP_STATE * s;
		bool opens = true;
		while (at_unit[0] < end[0] || at_unit[1] < end[1]) {
			const uint32_t kind = (at_unit[0] < end[0] && (at_unit[1] >= end[1] || T[0].pts[at_unit[0]] <= T[1].pts[at_unit[1]])) ? 0u : 1u;
			const uint32_t i = at_unit[kind]++, bytes = T[kind].bytes[i];
			const uint8_t *payload = T[kind].src ? T[kind].src + T[kind].off[i] : nullptr;
			const bool key = kind == 0 && bytes >= 4 && payload && payload[0] == 0 && payload[1] == 0 && payload[2] == 1 && payload[3] == 0xb3;
			if ((r.flags & JM_TSP_PSI) && ((opens && !w[4]) || key)) {
				for (uint32_t k = 0; k < 2; k++, at += 188) {
					if (ts) { memcpy(ts + at, psi + 188 * k, 188); ts[at + 3] |= (uint8_t)w[k]; }
					w[k] = (w[k] + 1) & 15u;
				}
			}
			opens = false;
			at += 188ull * tsp_host_unit(r, kind, payload, bytes, T[kind].pts[i], &w[2 + kind], ts ? ts + at : nullptr);
		}
		w[4] = 1;
		if (stream_end) stream_end[s] = at;
	}
	return at;
}

extern "C" int64_t jsmpeg_hip_ts_program_mux_host(const jsmpeg_hip_ts_program_config_t *config,
                                                  const uint8_t *video, const uint64_t *v_offset, const uint32_t *v_bytes, const uint32_t *v_stream, const uint64_t *v_pts, uint32_t n_v,
                                                  const uint8_t *audio, const uint64_t *a_offset, const uint32_t *a_bytes, const uint32_t *a_stream, const uint64_t *a_pts, uint32_t n_a,
                                                  uint32_t *state, uint8_t *ts, uint64_t ts_cap, uint64_t *stream_begin, uint64_t *stream_end) {
	g_err[0] = 0;
	if (tsp_check_config(config) < 0) return -1;
	if (n_v && (!video || !v_offset || !v_bytes || !v_pts)) return fail("ts_program: NULL video argument");
	if (n_a && (!audio || !a_offset || !a_bytes || !a_pts)) return fail("ts_program: NULL audio argument");
	const JmTspRule r = tsp_rule(*config);
	if (tsp_check_table("video", r.pid[0], v_stream, v_pts, n_v, config->max_streams) < 0) return -1;
	if (tsp_check_table("audio", r.pid[1], a_stream, a_pts, n_a, config->max_streams) < 0) return -1;
	uint8_t psi[2 * JM_TS_PACKET];
	jm_tsp_psi_packets(r, config->program_number, config->transport_stream_id, psi);
	const TspHostTable T[2] = { { video, v_offset, v_bytes, v_stream, v_pts, n_v }, { audio, a_offset, a_bytes, a_stream, a_pts, n_a } };
	std::vector<uint32_t> work(JM_TSP_STATE * (size_t)config->max_streams, 0u);
	if (state) work.assign(state, state + work.size());
	for (size_t i = 0; i < work.size(); i++) work[i] = (i % JM_TSP_STATE == 4) ? (work[i] ? 1u : 0u) : (work[i] & 15u);
	const std::vector<uint32_t> entry = work;
	const uint64_t need = tsp_host_walk(r, psi, T, config->max_streams, work.data(), nullptr, stream_begin, stream_end);
	if (!ts) return (int64_t)need;
	if (need > ts_cap) return fail("ts_program: %llu bytes do not fit ts_cap %llu", (unsigned long long)need, (unsigned long long)ts_cap);
	work = entry;
	tsp_host_walk(r, psi, T, config->max_streams, work.data(), ts, stream_begin, stream_end);
	if (state) memcpy(state, work.data(), sizeof(uint32_t) * work.size());
	return (int64_t)need;
}
