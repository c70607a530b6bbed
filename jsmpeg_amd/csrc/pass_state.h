/*
 * The lifecycle of a PASS HANDLE, once: a handle whose calls are pure enqueues on the caller's HIP stream, one pass in flight at
 * a time, settled by sync or by a reader of the device's results.  The resampler, the log-mel features, the MP2 encoder and
 * the TS program mux (pcm_resample.hip, logmel.hip, mp2_encode.hip, ts_program.hip) each embed a JmPass and keep their
 * extern "C" entry points; a new pass gets its lifecycle here.  Host only; include it after host_common.h.
 *
 * What differs between handles is data: the two fixed refusals are whole strings in the JmPass, the prefix of the others
 * (`who`) is an argument.  Nothing here asks which handle is calling.  g_err is the entry points' to clear.
 */
#pragma once
#include <cstdint>
#include <vector>

#include "host_common.h"

struct JmPass {
	const char *in_flight, *nothing_yet;                       /* what a second enqueue or a mutator / a reader without a pass is told */
	int device = 0;
	hipEvent_t ev[3] = { nullptr, nullptr, nullptr };          /* begin, the handle's mark between, done */
	bool pending = false, have_pass = false;                   /* set by the handle behind jm_pass_end and its own bookkeeping */
};

/* create: config_device < 0 keeps the calling thread's device */
static int jm_pass_open(JmPass &p, int config_device) {
	if (config_device >= 0 && hipSetDevice(config_device) != hipSuccess) return fail("hipSetDevice(%d) failed", config_device);
	if (hipGetDevice(&p.device) != hipSuccess) return fail("hipGetDevice failed");
	return 0;
}

static int jm_pass_events(JmPass &p) {
	for (hipEvent_t &v : p.ev) HIP_TRY(hipEventCreate(&v));
	return 0;
}

/* destroy: waits for the pass in flight, so that the handle's buffers can be freed behind it */
static void jm_pass_close(JmPass &p) {
	hipSetDevice(p.device);
	if (p.pending) hipEventSynchronize(p.ev[2]);
	for (hipEvent_t v : p.ev) if (v) hipEventDestroy(v);
}

/* waits for the pass in flight */
static int jm_pass_settle(JmPass &p) {
	if (!p.pending) return 0;
	HIP_TRY(hipSetDevice(p.device));
	p.pending = false;
	HIP_TRY(hipEventSynchronize(p.ev[2]));
	return 0;
}

/* 1 once the pass in flight has finished, 0 while it runs; never waits */
static int jm_pass_query(JmPass &p) {
	if (!p.pending) return 1;
	HIP_TRY(hipSetDevice(p.device));
	const hipError_t e = hipEventQuery(p.ev[2]);
	if (e == hipSuccess) return 1;
	if (e == hipErrorNotReady) return 0;
	return fail("hipEventQuery: %s", hipGetErrorString(e));
}

static int jm_pass_idle(const JmPass &p) { return p.pending ? fail("%s", p.in_flight) : 0; }
static int jm_pass_have(const JmPass &p) { return p.have_pass ? 0 : fail("%s", p.nothing_yet); }

/* the readers of the device's results: settle, then refuse a handle without a pass */
static int jm_pass_ready(JmPass &p) { return jm_pass_settle(p) < 0 ? -1 : jm_pass_have(p); }

static int jm_pass_begin(JmPass &p, hipStream_t st) {
	HIP_TRY(hipSetDevice(p.device));
	HIP_TRY(hipEventRecord(p.ev[0], st));
	return 0;
}
static int jm_pass_mark(JmPass &p, hipStream_t st) { HIP_TRY(hipEventRecord(p.ev[1], st)); return 0; }
static int jm_pass_end(JmPass &p, hipStream_t st) { HIP_TRY(hipEventRecord(p.ev[2], st)); return 0; }

static int jm_pass_elapsed(JmPass &p, int from, int to, float *ms) {
	HIP_TRY(hipSetDevice(p.device));
	HIP_TRY(hipEventElapsedTime(ms, p.ev[from], p.ev[to]));
	return 0;
}

/* ------------------------------------------------------------------ the chained handles: a call lists streams by NUMBER */

static int jm_pass_stream_bound(const char *who, uint32_t stream, uint32_t max_streams) {
	return stream < max_streams ? 0 : fail("%s: stream %u >= max_streams %u", who, stream, max_streams);
}

/* stream i of a call: its number (NULL: i) is below max_streams and above the one before it */
static int jm_pass_check_number(const char *who, const uint32_t *numbers, uint32_t i, uint32_t max_streams) {
	const uint32_t s = numbers ? numbers[i] : i;
	if (s >= max_streams) return fail("%s: stream_numbers[%u] = %u >= max_streams %u", who, i, s, max_streams);
	if (numbers && i && s <= numbers[i - 1]) return fail("%s: stream_numbers[] must ascend (stream_numbers[%u] = %u after %u)", who, i, s, numbers[i - 1]);
	return 0;
}

/* ... and its input, when it has any: there and whole floats.  Checked on the host, so nothing dereferences it */
static int jm_pass_check_pcm(const char *who, const void *const *pcm, const uint32_t *count, uint32_t i) {
	if (count[i] && !pcm[i]) return fail("%s: pcm[%u] is NULL", who, i);
	if (count[i] && ((uintptr_t)pcm[i] & 3u)) return fail("%s: pcm[%u] is not 4-byte aligned", who, i);
	return 0;
}

/* both, stream by stream: the first fault of the first faulty stream is the one reported */
static int jm_pass_check_streams(const char *who, const void *const *pcm, const uint32_t *count, const uint32_t *numbers, uint32_t n, uint32_t max_streams) {
	for (uint32_t i = 0; i < n; i++)
		if (jm_pass_check_number(who, numbers, i, max_streams) < 0 || jm_pass_check_pcm(who, pcm, count, i) < 0) return -1;
	return 0;
}

/* ends the chain of `stream` (0xffffffff: of every stream); C: the handle's record per stream number, all zeros when it has none */
template <class C>
static int jm_pass_chain_reset(const JmPass &p, const char *who, std::vector<C> &chain, uint32_t stream) {
	if (jm_pass_idle(p) < 0) return -1;
	if (stream != 0xffffffffu && jm_pass_stream_bound(who, stream, (uint32_t)chain.size()) < 0) return -1;
	for (size_t s = 0; s < chain.size(); s++)
		if (stream == 0xffffffffu || stream == s) chain[s] = C();
	return 0;
}
