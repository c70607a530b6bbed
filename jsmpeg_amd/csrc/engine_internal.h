/*
 * What the translation units of the host runtime share (engine.hip: the batch engine; live.hip: live streams, C ABI part 5;
 * decoder.hip: the reference's one-picture-per-call decoder ABI): the batch object itself -- the live front end and the
 * decoder's decode-ahead both drive a batch from the inside.  The error message and the allocation helper come from
 * host_common.h, the batch's TS ingest from ts_ingest.h.  Not installed; nothing outside jsmpeg_amd/csrc includes it.
 */
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <vector>

#include "host_common.h"
#include "index_tables.h"
#include "jsmpeg_hip.h"
#include "kernels.h"
#include "recon_plan.h"
#include "ts_ingest.h"
#include "ts_sync.h"

/* ------------------------------------------------------------ shared state */

int luts_for_device(int dev, JmVlcLuts **out);      /* the VLC tables on a device, built and uploaded once (engine.hip) */
static inline void geom_init(JmGeom &g, int width, int height) { jm_geom_init(g, width, height); }

/* What a batch's decode reads from the environment -- once, when the batch is created (batch_create); tests and tools set
 * these before they create one:
 *   JSMPEG_HIP_RECON_ORDER=0 / n     the reconstruct level by level / n streams in lockstep per class of the ordered launch
 *                                    whatever the picture size (default: the engine's choice, recon_plan.h jm_choose_recon)
 *   JSMPEG_HIP_RECON_DENSE=0 / 1     never / always the intra form with a transform slot per lane (default: by the intra
 *                                    pictures' bytes per macroblock, JM_DENSE_INTRA_X16)
 *   JSMPEG_HIP_RECON_CHAINS=1        tests: the ordered launch over GOP chains whatever the batch's shape
 *   JSMPEG_HIP_RECON_BREAK=n         tests: picture n of the ordered plan never reports (its successor's wait runs out)
 *   JSMPEG_HIP_RECON_PATIENCE=n      tests: polls before an ordered launch's wait gives up (0: the kernel's)
 *   JSMPEG_HIP_DEBUG=flags           diagnostics of the slice parse (kernels.h JmParseBufs::debug_flags)
 *   JSMPEG_HIP_TRACE=1               where the host's time goes in each decode call (stderr)
 * Read elsewhere: JSMPEG_HIP_POISON (jm_malloc), the tuning knobs JSMPEG_HIP_PARSE_*, _T_COLD, _RECON_LDSPAD (kernels.hip),
 * and in a -DJSMPEG_HIP_MEASUREMENT_HOOKS build JSMPEG_HIP_T_FIXEDFWD / _T_FIXEDDST (engine.hip fill_desc). */
/* pictures the one-picture interface decodes per pass of the batch engine when that many are buffered (mpeg1_decoder_t::ahead) */
#ifndef JM_DECODE_AHEAD
#define JM_DECODE_AHEAD 48u        /* ... at most, and no more than fit 160 MB of frames (1080p: 48, 2160p: 12): dec_sequence_header */
#endif
#define JM_TENSOR_STAGES 4u     /* slot tables of part-7 renders in flight at a time (jsmpeg_hip_batch_t::tstage) */
#define POOL_GUARD 256 /* bytes before/after a frame pool: aligned 12-byte prediction loads may straddle */

/* =========================================================================
 * The batch object
 * ========================================================================= */

struct jsmpeg_hip_batch_t {
	jsmpeg_hip_batch_config_t cfg;
	int device;
	JmGeom g;
	JmVlcLuts *d_luts;
	hipStream_t stream;          /* stream of the last decode */
	hipStream_t own_stream;      /* made by jsmpeg_hip_batch_own_stream for hosts without a HIP runtime of their own; null until asked for */

	uint8_t *d_es; uint64_t es_cap; uint32_t es_bytes;
	const uint8_t *es_view;      /* what the decode reads: d_es, or the caller's buffer after jsmpeg_hip_batch_attach_device */
	uint32_t n_streams;
	std::vector<JmStream> h_streams;
	JmStream *d_streams;

	uint32_t sc_cap;
	uint64_t *d_scan_state;
	uint32_t *d_sc_pos; uint8_t *d_sc_code; uint32_t *d_sc_owner; uint32_t *d_pic_sc; uint32_t *d_slice_sc; uint32_t *d_slice_order; uint32_t *d_order_hist; uint32_t *d_counters;
	JmPic *d_pics; JmPic *h_pics;                 /* h_pics, h_desc: pinned host memory (copies of pageable memory stall on the runtime's staging path) */
	JmReconDesc *d_desc; JmReconDesc *h_desc;
	uint32_t *d_covered, *h_covered;   /* macroblock records written per picture (k_parse); h_covered pinned */
	uint32_t desc_cap, n_uncovered;
	hipEvent_t ev_cov;
	hipEvent_t ev_idx;           /* the index's counters and picture table have arrived on the host (the slice order runs on beside the host's turn-around).
	                                SAME-STREAM RULE: the order's kernels are enqueued before the host has looked at the counters, and they share
	                                d_order_hist with the parse that follows (its ticket and per-CU counters sit behind the histogram) -- with no host
	                                barrier between one decode's parse and the next decode's order.  That is safe because everything of a batch is
	                                enqueued on ONE stream at a time (jsmpeg_hip_batch_decode's hip_stream; a caller that changes streams between decodes
	                                synchronises the old one first -- jsmpeg_hip_batch_sync) and because the kernels clamp what they read from the counters
	                                to the tables' capacity (order_dims): a pass the host then refuses (overflow) has touched nothing outside them */
	/* ordered reconstruct (one launch per batch, recon_plan.h jm_plan_ordered): per-picture tile counts, the launch's
	 * status words (kernels.h JM_RECON_STATUS_WORDS; h_: pinned), and how the last decode went */
	uint32_t *d_done, *d_rstatus, *h_rstatus;
	/* streams that continue other streams (jsmpeg_hip_batch_link_streams / _seed_stream; recon_plan.h): cleared by every upload / attach */
	std::vector<int32_t> link_prev;
	std::vector<uint8_t> seeded;
	std::vector<const uint8_t *> seed_frames;   /* [2 * stream + which] */
	uint32_t last_group;         /* lockstep width of the last decode's launch, 0: it went level by level */
	JmReconPolicy recon;         /* what decides the reconstruct's plan besides the pictures (recon_plan.h) */
	int debug_flags;             /* JSMPEG_HIP_DEBUG */
	bool trace;                  /* JSMPEG_HIP_TRACE */
	uint32_t roots_x16;          /* compressed bytes per macroblock (x 16) of the last decode's pictures without a forward reference */
	bool ordered;                /* the last decode used the ordered launch (its status is checked at the next sync) */
	std::vector<uint32_t> chain_heads;   /* ordered by GOP chains (narrow batches): the pictures whose `stale` frame lies in ANOTHER chain -- they must
	                                        turn out to have written every macroblock (checked at the next sync, else the frames are done over) */
	bool stats_pending;          /* n_levels / n_uncovered of the last decode not worked out yet (needs the parse's counts) */
	uint32_t ordered_status;     /* status of the last checked ordered launch (non-zero: it was done over) */
	uint32_t ordered_waits;      /* polls of the last checked ordered launch that found their picture unfinished */
	JmMbRec *d_mb; uint16_t *d_tokens; uint8_t *d_pool_alloc, *d_pool;
	uint64_t *d_hashes;
	uint8_t *d_rgba;             /* one RGBA frame: scratch of jsmpeg_hip_batch_read_rgba */
	JmTsIngest ts;                /* ingest side (jsmpeg_hip_batch_upload_ts, _ts_writes): the device TS demux and its last write list */
	uint32_t *d_dbg;
	uint8_t epoch;

	uint32_t n_sc, n_pics, n_levels, n_decoded, n_slices, n_slice_codes;
	hipEvent_t ev[5];
	hipEvent_t ev_level[65];     /* before every reconstruct launch (the first 64) and after the last */
	uint32_t n_level_ev;
	bool timed;
	uint32_t *h_counters; /* pinned */
	void *h_counters_dev, *h_pics_dev;   /* the device's addresses of h_counters and h_pics (written by k_to_host) */
	/* LIVE (jsmpeg_hip_live_t below: a batch pass over what has arrived of streams that go on): the pool holds
	 * `pool_frames` frames (the streams' rings), and picture p of a pass is written to pool slot slot[p] -- a live stream
	 * owns a ring of slots, so that the frames of its last two decoded pictures are still there, untouched, when the next
	 * pass predicts from them.  slot empty: picture p = slot p (every other batch). */
	uint32_t pool_frames;
	uint32_t mb_pictures;        /* pictures the macroblock records are allocated for (max_pictures; live: what a pass can DECODE, JmPic::mb_index) */
	uint32_t pics_first_copy;    /* picture-table entries that come to the host with the index's counters (all of them; live: a pass's usual
	                                number -- the table is sized for the start codes a pass can SEE --, the rest in a second copy when there are more) */
	std::vector<uint32_t> slot;
	struct jsmpeg_hip_live_t *live;
	/* ENQUEUED passes (jsmpeg_hip_batch_enqueue): planned on the device (enqueue_plan.h), settled by the next call that reads
	 * results (batch_settle_enqueued).  rows_cap: rows of the ordered launch's grid (max_pictures with jm_plan_ordered's 8 %
	 * of slack); d_plan: the plan block; d_plan_u32: the planner's scratch (JmPlanArgs) */
	uint32_t rows_cap;
	JmDevPlan *d_plan, h_plan;
	uint32_t *d_plan_u32;
	bool enq_pending;            /* a pass is enqueued and not settled yet */
	bool enqueued;               /* the last pass was enqueued (timings: no host turn-around) */
	bool enq_failed;             /* ... and settling it failed: sync reports enq_err once */
	char enq_err[512];
	/* TENSOR renders (part 7, batch_render_tensor): ev_pool is recorded on the decode's stream before a render and waited for on
	 * the render's; ev_tensor is recorded on the render's stream after it, and the next decode, enqueue or tick waits for it
	 * (tensor_pending) before it writes the pool.  A render's slot table goes to the device from pinned memory through one of
	 * JM_TENSOR_STAGES stages taken in turn; a stage is used again once the render that used it last has finished (its event):
	 * the host waits only when it is that many renders ahead of the device.  A stage that is too small for a call gets larger
	 * buffers (a power of two, at least max_pictures); the outgrown ones are freed with the batch -- a free in between would
	 * synchronise the device. */
	/* SELECTED frames (jsmpeg_hip_batch_select; select_plan.h): the requests as given, their layout on the host and -- bits | off |
	 * nbits | frame_pic in ONE allocation -- on the device, where k_select reads it behind the index of every pass until the next
	 * upload / attach clears it.  sel_pending: a selected pass's check of its unwritten macroblocks is outstanding (batch_settle_selected:
	 * every reader and sync; a stream that fails it is widened -- sel_widened, sel_bits -- and the pass run once more, sel_redone) */
	std::vector<uint32_t> sel_stream, sel_frame, sel_off, sel_nbits, sel_bits, sel_frame_pic;
	std::vector<uint8_t> sel_widened;
	uint32_t *d_sel; size_t sel_cap_words;
	int32_t *d_before_last;      /* [max_pictures] the whole decode's decoded picture before last of every picture (k_select) */
	bool sel_set, sel_pending, sel_redone, sel_in_redo, sel_have_map;
	hipEvent_t ev_pool, ev_tensor;
	bool tensor_pending;
	struct TensorStage { uint32_t *h, *d; uint32_t cap; hipEvent_t done; };
	TensorStage tstage[JM_TENSOR_STAGES];
	uint32_t tstage_next;
	std::vector<uint32_t *> tretired_h, tretired_d;
};
/* part 7: rows of pool slots (JM_NONE: a row of zeros) -> a tensor on `st`; the descriptor has passed jm_tensor_check */
int batch_render_tensor(jsmpeg_hip_batch_t *b, const uint32_t *slots, uint32_t count, const jsmpeg_hip_tensor_desc_t *desc,
                        void *dev_out, hipStream_t st);
/* ... with dev_rois (device memory, ready on `st`): a row per region of interest of those slots, n_rois rows, their status to
 * dev_status (or null); the descriptor has passed jm_tensor_roi_check.  dev_rois null: batch_render_tensor. */
int batch_render_tensor_rois(jsmpeg_hip_batch_t *b, const uint32_t *slots, uint32_t count, const jsmpeg_hip_tensor_desc_t *desc,
                             const jsmpeg_hip_roi_t *dev_rois, uint32_t n_rois, void *dev_out, uint8_t *dev_status, hipStream_t st);
/* ... and the wait of a stream that is about to write the pool for the renders since the last one */
static inline int batch_wait_tensor(jsmpeg_hip_batch_t *b, hipStream_t st) {
	if (!b->tensor_pending) return 0;
	b->tensor_pending = false;
	HIP_TRY(hipStreamWaitEvent(st, b->ev_tensor, 0));
	return 0;
}
int live_assign_slots(struct jsmpeg_hip_live_t *l);    /* the live front end's turn inside a decode: once the picture table is on the host */
static inline uint8_t *frame_of(const jsmpeg_hip_batch_t *b, uint32_t p) {
	return b->d_pool + (uint64_t)(b->slot.empty() ? p : b->slot[p]) * b->g.frame_bytes;
}

/* the live front end's form of jsmpeg_hip_batch_create: pool_frames frames in the pool (rings of slots), macroblock records for
 * mb_pictures pictures (0 / 0: max_pictures of each) */
jsmpeg_hip_batch_t *batch_create(const jsmpeg_hip_batch_config_t *config, uint32_t pool_frames, uint32_t mb_pictures);
void batch_free(jsmpeg_hip_batch_t *b);

