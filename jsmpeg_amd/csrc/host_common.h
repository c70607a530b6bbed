/*
 * The one error and allocation dialect of the host runtime: every translation unit of the library (engine.hip, live.hip,
 * decoder.hip, encode.hip through engine_internal.h; ts_ingest.hip, mp2_stage.hip, mp2_live.hip, shard.hip directly;
 * pcm_resample.hip, logmel.hip, mp2_encode.hip, ts_program.hip with pass_state.h, the lifecycle of their handles, on top)
 * reports through fail() into the calling thread's message and allocates device memory through jm_malloc.  Knows nothing of
 * the batch object.  Not installed; nothing outside jsmpeg_amd/csrc includes it.
 */
#pragma once
#include <hip/hip_runtime.h>

#include <cstdlib>

/* the calling thread's last message (jsmpeg_hip_last_error); defined in engine.hip.  An entry point clears it with
 * g_err[0] = 0 and returns fail(printf format, ...), which is -1 */
extern thread_local char g_err[512];
int fail(const char *fmt, ...) __attribute__((format(printf, 1, 2)));
#define HIP_TRY(expr)                                                                        \
	do {                                                                                     \
		hipError_t e_ = (expr);                                                              \
		if (e_ != hipSuccess) return fail("%s: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
	} while (0)

/* Every device allocation of the engine goes through here.  JSMPEG_HIP_POISON=<byte> fills fresh allocations with
 * that byte (diagnostics: a kernel that reads memory nobody wrote then misbehaves the same way every time instead
 * of depending on what the allocator hands back). */
template <class T>
static hipError_t jm_malloc(T **p, size_t bytes) {
	hipError_t e = hipMalloc(reinterpret_cast<void **>(p), bytes);
	static const int poison = [] { const char *v = getenv("JSMPEG_HIP_POISON"); return v ? (int)strtol(v, nullptr, 0) & 255 : -1; }();
	if (e == hipSuccess && poison >= 0 && bytes) { e = hipMemset(*p, poison, bytes); if (e == hipSuccess) e = hipDeviceSynchronize(); }
	return e;
}
