/*
 * The DEVICE PLAN of an enqueued pass (jsmpeg_hip_batch_enqueue, engine.hip): what the decode path's host works out from
 * the picture table between the index and the parse -- the parse launch's sizing, `stale` per picture, the ordered
 * reconstruct's sequence and waits -- as plain C++ that one workgroup runs on the device (kernels.hip k_plan) and
 * tests/sim/plan_main.cpp runs on the CPU, stage by stage.  One source for the rules: the walk and jm_plan_parse_rules
 * below are what the decode path's collect_index and jm_plan_parse call, and the sequence is jm_plan_ordered's
 * (recon_plan.h), by streams or by GOP chains.
 *
 * What it relies on: a batch's decoded pictures are grouped by stream in the table (the index numbers them in ES order,
 * and the streams lie one behind the other in the ES), so a stream -- and a GOP chain -- is a RUN of the compacted list of
 * decoded pictures, and the picture before last of a picture's stream is two places back in that list.  Linked or seeded
 * streams (recon_plan.h) are not planned here: such a batch takes the blocking decode.
 */
#ifndef JSMPEG_AMD_ENQUEUE_PLAN_H
#define JSMPEG_AMD_ENQUEUE_PLAN_H

#include <stdint.h>

#include "mpeg1_dev.h"
#include "recon_plan.h"
#include "slice_parse.h"

#ifndef JM_PARSE_WG
#define JM_PARSE_WG 512   /* 8 wavefronts share one copy of the tables: 2 workgroups = 16 wavefronts per CU */
#endif
#define JM_PARSE_WAVES (JM_PARSE_WG / 64)
#define JM_PARSE_FILL_WAVES 4096u   /* wavefronts that fill the GPU for this kernel: 256 CUs x 16 */
#define JM_PARSE_RESIDENT_WGS (JM_PARSE_FILL_WAVES / JM_PARSE_WAVES)

#ifndef JM_DONE_STRIDE
#define JM_DONE_STRIDE 32     /* (kernels.h) words between two pictures' tile counts of an ordered launch */
#endif

JM_HD uint32_t jm_umin(uint32_t a, uint32_t b) { return a < b ? a : b; }
JM_HD uint64_t jm_umin64(uint64_t a, uint64_t b) { return a < b ? a : b; }

/* ------------------------------------------------------------------ parse sizing */

/* The tuning / test overrides of the parse launch (JSMPEG_HIP_PARSE_LANES, _T_COLD, _PARSE_SPLIT, _PARSE_HEAD, _PARSE_PRIO,
 * _PARSE_RESIDENT, _PARSE_EVEN): read on the host (kernels.hip jm_parse_overrides) and handed to the rules, so that a pass
 * planned on the device follows them as the host's does. */
struct JmParseOverrides {
	int32_t lanes;          /* 1 .. 64: slices per wavefront, else not set */
	int32_t t_cold;         /* 1 .. 64: the header step's threshold, else not set */
	int32_t split;          /* < 0 not set, else the ring service in two halves (1) or not (0) */
	int32_t prio;           /* < 0 the rule, else that many batches at raised priority */
	uint32_t head_set, head_a, head_l0, head_h, head_l1;   /* "a,l0,h,l1" parsed and valid */
	uint32_t resident;      /* workgroups the GPU holds at a time (tickets beyond) */
	int32_t even;           /* the grid of passes without tickets (kernels.hip jm_plan_parse) */
};

/* what the rules read (n_lanes .. debug_flags) and decide (the rest): the fields of JmParseBufs of the same names */
struct JmParseSizing {
	uint32_t n_lanes, long_slices, bytes_per_mb_x16;
	int32_t debug_flags;
	uint32_t lanes_per_wave, t_cold, split_service, prio_batches, n_batches;
	int32_t cold_threshold;
	uint32_t head_batches[2], head_lanes[2], head_first[3];
};

/* kernels.hip jm_plan_parse's arithmetic (the measurements behind the rules: kernels.hip jm_parse_overrides and the profiles
 * it names).  n_lanes != 0.  Returns the
 * workgroups; *use_ticket: the wavefronts draw further batches by ticket. */
JM_HD uint32_t jm_plan_parse_rules(JmParseSizing &b, const JmParseOverrides &o, bool have_ticket, bool *use_ticket) {
	uint32_t lanes = 64;
	if (b.n_lanes <= 512u * 64u) {
		lanes = 1;
		while (lanes < 64 && (uint64_t)lanes * (JM_PARSE_FILL_WAVES / 2) < b.n_lanes) lanes <<= 1;
	}
	if (b.debug_flags & 8) lanes = 64;
	bool lanes_forced = false;
	if (o.lanes >= 1 && o.lanes <= 64) { lanes = (uint32_t)o.lanes; lanes_forced = true; }
	b.lanes_per_wave = lanes;
	b.t_cold = JM_T_COLD;
	if (b.bytes_per_mb_x16 >= JM_T_COLD_DENSE_X16) b.t_cold = JM_T_COLD_DENSE;
	if (o.t_cold >= 1 && o.t_cold <= 64) b.t_cold = (uint32_t)o.t_cold;
	b.cold_threshold = (int32_t)((b.t_cold * lanes + 63) / 64);
	b.split_service = b.bytes_per_mb_x16 >= JM_T_COLD_DENSE_X16 ? 1u : 0u;
	if (o.split >= 0) b.split_service = o.split ? 1u : 0u;
	b.head_batches[0] = b.head_batches[1] = 0; b.head_lanes[0] = b.head_lanes[1] = 1;
	b.head_first[0] = b.head_first[1] = b.head_first[2] = 0;
	uint32_t H = b.long_slices, seg_a = 0;
	bool forced = false;
	if (o.head_set) {
		H = jm_umin(o.head_h, b.n_lanes); seg_a = jm_umin(o.head_a, H); seg_a -= seg_a % o.head_l0;
		b.head_lanes[0] = o.head_l0; b.head_lanes[1] = o.head_l1; forced = true;
	}
	if (!forced) {
		uint32_t lh = 0, lt = 0;
		if (H > 0 && (uint64_t)H * 3 <= b.n_lanes && !(b.debug_flags & 8) && !lanes_forced) {
			for (uint32_t w = JM_PARSE_FILL_WAVES / 2; w <= JM_PARSE_FILL_WAVES * 3 / 4 && !lh; w += JM_PARSE_FILL_WAVES / 4)
				for (uint32_t l = 1; l <= 16 && !lh; l <<= 1) {
					const uint32_t head_w = (H + l - 1) / l;
					if (head_w > w * 3 / 4) continue;
					for (uint32_t t = 16; t <= 64; t <<= 1)
						if (t > l && (b.n_lanes - H + t - 1) / t <= w - head_w) { lh = l; lt = t; break; }
				}
		}
		if (lh) {
			seg_a = H - H % lh;
			b.head_lanes[0] = b.head_lanes[1] = lh;
			lanes = lt;
			b.lanes_per_wave = lanes;
			b.cold_threshold = (int32_t)((b.t_cold * lanes + 63) / 64);
		} else H = 0;
	}
	if (H) {
		b.head_batches[0] = seg_a / b.head_lanes[0];
		b.head_first[1] = seg_a;
		b.head_batches[1] = (H - seg_a + b.head_lanes[1] - 1) / b.head_lanes[1];
		b.head_first[2] = jm_umin(seg_a + b.head_batches[1] * b.head_lanes[1], b.n_lanes);
	}
	b.n_batches = b.head_batches[0] + b.head_batches[1] + (b.n_lanes - b.head_first[2] + lanes - 1) / lanes;
	b.prio_batches = 0;
	if (o.prio >= 0) b.prio_batches = (uint32_t)o.prio;
	else if (b.long_slices) b.prio_batches = b.head_batches[0] + b.head_batches[1] ? b.head_batches[0] + b.head_batches[1] : (b.long_slices + lanes - 1) / lanes;
	uint32_t groups = (b.n_batches + JM_PARSE_WAVES - 1) / JM_PARSE_WAVES;
	const uint32_t resident = o.resident;
	*use_ticket = groups > resident && resident >= 1 && have_ticket;
	if (*use_ticket) groups = resident;
	else {
		if (o.even && groups > resident / 2 && groups < resident) groups = resident;
		else if (o.even && b.n_batches <= resident / 2) groups = b.n_batches;
		else if (o.even >= 2 && groups < resident / 2) groups = resident / 2;
	}
	return groups;
}

/* The walk over the picture table (engine.hip collect_index): decoded pictures and their slices, how many slices are much
 * longer than the mean, the bytes of the pictures whose slices are several times it (coded video's intra pictures) and of
 * the pictures without a forward reference.  `lanes`: the pass's slice codes. */
struct JmWalkSums { uint64_t n_decoded, n_slices, long_slices, crit_bytes, crit_pics, root_bytes, roots,
                    bytes; };       /* bytes: of the decoded pictures -- what a pass over SELECTED frames (select_plan.h) parses, where es_bytes is all there is */
JM_HD void jm_walk_picture(const JmPic *pics, uint32_t n_pics, uint32_t p, const JmStream *streams, uint32_t n_streams,
                           uint64_t lanes, uint32_t es_bytes, JmWalkSums &s) {
	const JmPic &pic = pics[p];
	if (!pic.decoded) return;
	s.n_decoded++; s.n_slices += pic.n_slices;
	if (pic.stream >= n_streams) return;
	const uint32_t end = p + 1 < n_pics && pics[p + 1].stream == pic.stream ? pics[p + 1].pos : streams[pic.stream].es_end;
	const uint64_t bytes = end > pic.pos ? end - pic.pos : 0;
	s.bytes += bytes;
	if (pic.fwd < 0) { s.root_bytes += bytes; s.roots++; }
	if (!pic.n_slices) return;
	if (bytes * 2 * lanes >= (uint64_t)3 * es_bytes * pic.n_slices) s.long_slices += pic.n_slices;   /* >= 1.5 x the mean slice */
	if (bytes * lanes >= (uint64_t)4 * es_bytes * pic.n_slices) { s.crit_bytes += bytes; s.crit_pics++; }   /* >= 4 x: coded video's intra pictures */
}

/* A pass over selected frames: the slice order puts the slice codes nobody owns last, so the parse takes the owned ones only,
 * and the bytes per macroblock are those of the pictures it parses (jm_parse_sizing_from_walk's n_lanes and es_bytes) */
JM_HD uint32_t jm_selected_lanes(const JmWalkSums &w, uint32_t lanes) { return (uint32_t)jm_umin64(w.n_slices, lanes); }
JM_HD uint32_t jm_selected_bytes(const JmWalkSums &w, uint32_t es_bytes) { return (uint32_t)jm_umin64(w.bytes, es_bytes); }

/* ... and what the parse's launch takes from it (engine.hip enqueue_parse): the estimate of long slices (+ 1/8: the estimate
 * is by picture, the order by slice), the compressed bytes per macroblock x 16 -- the critical pictures' when there are any --
 * and *roots_x16, the pictures without a forward reference's (the reconstruct's dense intra rule) */
JM_HD void jm_parse_sizing_from_walk(const JmWalkSums &w, uint32_t n_lanes, uint32_t es_bytes, int32_t mb_size, JmParseSizing &ps, uint32_t *roots_x16) {
	const uint64_t mbs = (uint64_t)(mb_size > 1 ? mb_size : 1);
	ps.n_lanes = n_lanes;
	ps.long_slices = n_lanes ? (uint32_t)jm_umin64(w.long_slices + w.long_slices / 8, n_lanes) : 0;
	ps.bytes_per_mb_x16 = 0;
	if (w.n_decoded) ps.bytes_per_mb_x16 = (uint32_t)jm_umin64(1u << 20, (uint64_t)es_bytes * 16 / (w.n_decoded * mbs));
	if (w.crit_pics) {
		const uint32_t crit = (uint32_t)jm_umin64(1u << 20, w.crit_bytes * 16 / (w.crit_pics * mbs));
		if (crit > ps.bytes_per_mb_x16) ps.bytes_per_mb_x16 = crit;
	}
	if (roots_x16) *roots_x16 = w.roots ? (uint32_t)jm_umin64(w.root_bytes * 16 / (w.roots * mbs), 0xffffffffu) : 0u;
}

/* ------------------------------------------------------------------ the plan */

#define JM_PLAN_THREADS 512u       /* k_plan's workgroup */
#define JM_PLAN_SORT_CAP 2048u     /* streams / GOP chains the device deals to the classes; more: the pass is planned on the host at sync */
#define JM_PLAN_MAXW 64u           /* streams (chains) a class walks in lockstep at most; more: planned on the host at sync */

enum JmPlanKind { JM_PLAN_HOST = 0, JM_PLAN_STREAMS = 1, JM_PLAN_CHAINS = 2 };

/* The plan block (device memory): the parse's launch reads its sizing from here (JmParseBufs::plan), sync reads the rest. */
struct JmDevPlan {
	JmParseSizing parse;
	uint32_t n_sc;               /* the index's start codes */
	uint32_t n_pics, n_units_dec; /* pictures of the pass; decoded pictures of the streams */
	uint32_t overflow;           /* the index's tables overflowed: nothing is parsed or reconstructed, sync reports it */
	uint32_t kind;               /* JmPlanKind: how the ordered launch walks, or JM_PLAN_HOST: it has nothing to do, sync reconstructs */
	uint32_t rows, lockstep, n_chains;
	uint32_t load[8];            /* pictures per class */
};

/* what the host hands the planner (kernel arguments: nothing of it is copied) */
struct JmPlanArgs {
	const uint32_t *counters;    /* the index's counters (kernels.h JmScanBufs::counters) */
	const JmPic *pics;
	const JmStream *streams;
	uint32_t n_streams, es_bytes, sc_cap, pic_cap;
	int32_t mb_size, debug_flags;
	JmParseOverrides ov;
	/* the reconstruct: recon_plan.h jm_choose_recon's inputs that do not come from the pictures */
	uint32_t rows_cap;           /* rows of descriptors the launch has (its grid) */
	uint32_t tiles_per_picture, group;
	uint32_t try_streams, try_chains, streams_forced, chains_forced;   /* jm_choose_recon: the kinds it tries; forced = no distance rule */
	int32_t brk;                 /* JSMPEG_HIP_RECON_BREAK */
	uint32_t selected;           /* the pass has a selection (k_select ran): the parse is sized by the needed pictures */
	/* scratch, device memory: dec, chain_id, cstart, cend [pic_cap]; ustart, uend [n_streams]; seq [8 rows_cap] */
	uint32_t *dec, *chain_id, *ustart, *uend, *cstart, *cend, *seq;
	int32_t *stale;              /* out [pic_cap]: recon_plan.h jm_plan_stale */
	JmDevPlan *plan;             /* out */
	/* zeroed here: the parse's covered counts, the launch's done words (JM_DONE_STRIDE apart) and status words */
	uint32_t *covered, *done, *status;
};

/* the planner's shared memory (LDS on the device) */
struct JmPlanShared {
	JmWalkSums sums;
	uint32_t scan[2][JM_PLAN_THREADS];
	uint64_t key[JM_PLAN_SORT_CAP];
	uint32_t deal[JM_PLAN_SORT_CAP];           /* sorted unit k: class | place in the class << 3, JM_NONE: empty */
	uint32_t list[JM_PLAN_SORT_CAP];           /* units by class, cls_off[c] .. */
	uint32_t act_start[8][JM_PLAN_MAXW], act_len[8][JM_PLAN_MAXW], act_at[8][JM_PLAN_MAXW];
	uint32_t cls_n[8], cls_off[8], width[8];
	uint64_t load[8];
	uint32_t n_pics, n_dec, n_chains, n_lanes, overflow, n_units, n_pow2, kind, ok, rows, lockstep, scan_total;
};

/* a decoded picture of the streams (what jm_plan_stale / jm_plan_ordered / jm_plan_chains look at) */
JM_HD bool jm_plan_in_unit(const JmPic &pic, uint32_t n_streams) { return pic.decoded && pic.stream < n_streams; }
/* decoded picture r (of the compacted list) begins a GOP chain (recon_plan.h jm_plan_chains) / a stream's run */
JM_HD bool jm_plan_stream_head(const JmPic *pics, const uint32_t *dec, uint32_t r) { return r == 0 || pics[dec[r - 1]].stream != pics[dec[r]].stream; }
JM_HD bool jm_plan_chain_head(const JmPic *pics, const uint32_t *dec, uint32_t r) { return jm_plan_stream_head(pics, dec, r) || pics[dec[r]].fwd < 0; }

/* The waits of the picture in slot k of the ordered sequence, decoded picture r (engine.hip enqueue_ordered): its own count,
 * its forward reference, its `stale` frame -- which a GOP chain's first pictures do not wait for (another chain's: sync
 * checks that they wrote every macroblock) -- and JSMPEG_HIP_RECON_BREAK's picture that never reports. */
JM_HD void jm_plan_slot_waits(const JmPic *pics, const uint32_t *dec, const int32_t *stale, const uint32_t *chain_id, uint32_t kind,
                              uint32_t r, bool brk, uint32_t &done_pic, uint32_t &wait_fwd, uint32_t &wait_stale) {
	const uint32_t p = dec[r];
	done_pic = brk ? JM_NONE : p;
	wait_fwd = pics[p].fwd >= 0 ? (uint32_t)pics[p].fwd : JM_NONE;
	wait_stale = stale[p] >= 0 ? (uint32_t)stale[p] : JM_NONE;
	if (kind == JM_PLAN_CHAINS && stale[p] >= 0 && chain_id[r - 2] != chain_id[r]) wait_stale = JM_NONE;   /* (stale[p] >= 0: r >= 2, same stream) */
}

/* An exclusive scan of per-thread counts over the workgroup (Hillis-Steele, two buffers): s.scan[..][t] after it holds the
 * INCLUSIVE sum of threads 0 .. t; returns the buffer that does. */
template <class X>
JM_HD uint32_t jm_plan_scan(X &x, JmPlanShared &s) {
	uint32_t k = 0;
	for (uint32_t d = 1; d < x.nt; d <<= 1) {
		x.par([&](uint32_t t, uint32_t) { s.scan[k ^ 1][t] = s.scan[k][t] + (t >= d ? s.scan[k][t - d] : 0u); });
		k ^= 1;
	}
	return k;
}

/* Sort the units by length, longest first, equal lengths in their order (std::stable_sort in jm_plan_ordered): a bitonic sort
 * of (~length, unit) keys in shared memory; then deal them with one lane, longest first onto the class with the least so far,
 * and check the plan as jm_plan_ordered and jm_choose_recon's `fits` do.  Leaves s.ok and the classes' lists. */
template <class X>
JM_HD void jm_plan_deal(X &x, const JmPlanArgs &a, JmPlanShared &s, const uint32_t *ustart, const uint32_t *uend, bool forced) {
	x.par([&](uint32_t t, uint32_t nt) {
		if (t == 0) { uint32_t n2 = 1; while (n2 < s.n_units) n2 <<= 1; s.n_pow2 = n2; }
		for (uint32_t i = t; i < JM_PLAN_SORT_CAP; i += nt)
			s.key[i] = i < s.n_units ? ((uint64_t)(0xffffffffu - (uend[i] - ustart[i])) << 32) | i : ~0ull;
	});
	for (uint32_t k = 2; k <= s.n_pow2; k <<= 1)
		for (uint32_t j = k >> 1; j > 0; j >>= 1)
			x.par([&](uint32_t t, uint32_t nt) {
				for (uint32_t i = t; i < s.n_pow2; i += nt) {
					const uint32_t l = i ^ j;
					if (l <= i) continue;
					const uint64_t ki = s.key[i], kl = s.key[l];
					if ((ki > kl) == ((i & k) == 0)) { s.key[i] = kl; s.key[l] = ki; }
				}
			});
	x.par([&](uint32_t t, uint32_t) {
		if (t != 0) return;
		for (uint32_t c = 0; c < 8; c++) { s.load[c] = 0; s.cls_n[c] = 0; }
		uint64_t total = 0;
		for (uint32_t k = 0; k < s.n_units; k++) {
			const uint32_t len = 0xffffffffu - (uint32_t)(s.key[k] >> 32);
			if (len == 0) { s.deal[k] = JM_NONE; continue; }
			uint32_t best = 0;
			for (uint32_t c = 1; c < 8; c++) if (s.load[c] < s.load[best]) best = c;
			s.deal[k] = best | (s.cls_n[best] << 3);
			s.cls_n[best]++; s.load[best] += len; total += len;
		}
		uint64_t most = 0;
		uint32_t off = 0, lockstep = a.group;
		bool ok = total != 0;
		for (uint32_t c = 0; c < 8; c++) {
			if (s.load[c] > most) most = s.load[c];
			s.cls_off[c] = off; off += s.cls_n[c];
			lockstep = jm_umin(lockstep, s.cls_n[c]);
			/* the lockstep width of the class (jm_plan_ordered) */
			const uint32_t n = s.cls_n[c];
			uint32_t width = jm_umin(a.group, n);
			while (width < n && n % width != 0 && n % width < a.group) width++;
			s.width[c] = width;
			ok = ok && width <= JM_PLAN_MAXW;
		}
		ok = ok && most * 8 * 100 <= total * (100 + 8);
		ok = ok && most <= a.rows_cap && (forced || (lockstep - 1) * a.tiles_per_picture >= JM_ORDER_MIN_DISTANCE);
		s.ok = ok ? 1u : 0u; s.rows = (uint32_t)most; s.lockstep = lockstep;
	});
}

/* every class (one lane each) walks its units in lockstep (jm_plan_ordered): seq[8 i + c] = the decoded picture (its place in
 * the compacted list) that class c takes i-th */
template <class X>
JM_HD void jm_plan_walk(X &x, const JmPlanArgs &a, JmPlanShared &s, const uint32_t *ustart, const uint32_t *uend) {
	x.par([&](uint32_t t, uint32_t nt) {
		for (uint32_t k = t; k < s.n_units; k += nt)
			if (s.deal[k] != JM_NONE) s.list[s.cls_off[s.deal[k] & 7] + (s.deal[k] >> 3)] = (uint32_t)s.key[k];
	});
	x.par([&](uint32_t t, uint32_t) {
		if (t >= 8) return;
		const uint32_t c = t, n = s.cls_n[c], *list = s.list + s.cls_off[c];
		uint32_t *st = s.act_start[c], *ln = s.act_len[c], *at = s.act_at[c];
		uint32_t next = 0, na = 0, i = 0;
		while (na < s.width[c] && next < n) { const uint32_t u = list[next++]; st[na] = ustart[u]; ln[na] = uend[u] - ustart[u]; at[na] = 0; na++; }
		while (na > 0) {
			for (uint32_t q = 0; q < na;) {
				const uint32_t k = at[q] + 1;
				a.seq[8 * i++ + c] = st[q] + k - 1;
				at[q] = k;
				if (k < ln[q]) { q++; continue; }
				if (next < n) { const uint32_t u = list[next++]; st[q] = ustart[u]; ln[q] = uend[u] - ustart[u]; at[q] = 0; q++; }   /* the next unit takes the place */
				else {
					for (uint32_t m = q + 1; m < na; m++) { st[m - 1] = st[m]; ln[m - 1] = ln[m]; at[m - 1] = at[m]; }
					na--;
				}
			}
		}
	});
}

/* The planner: everything but the descriptors' addresses (k_plan adds those, slot by slot, behind it).  X: the executor --
 * x.nt threads, x.par(f) runs f(thread, x.nt) on every thread and then waits for all of them, x.add64 an atomic add into
 * shared memory. */
template <class X>
JM_HD void jm_plan_run(X &x, const JmPlanArgs &a, JmPlanShared &s) {
	/* the index's counts; an overflowed pass is planned as empty (sync reports it) */
	x.par([&](uint32_t t, uint32_t) {
		if (t != 0) return;
		s.overflow = a.counters[2] != 0;
		s.n_pics = s.overflow ? 0u : jm_umin(a.counters[1], a.pic_cap);
		s.n_lanes = s.overflow ? 0u : jm_umin(a.counters[4], a.sc_cap);
		s.sums = JmWalkSums{ 0, 0, 0, 0, 0, 0, 0, 0 };
		s.kind = JM_PLAN_HOST; s.rows = 0; s.lockstep = 0; s.n_chains = 0; s.n_dec = 0;
		for (uint32_t c = 0; c < 8; c++) s.load[c] = 0;
	});
	/* the walk; what the pass's launches start from: covered counts, done words, status words, `stale` */
	x.par([&](uint32_t t, uint32_t nt) {
		JmWalkSums w = { 0, 0, 0, 0, 0, 0, 0, 0 };
		for (uint32_t p = t; p < s.n_pics; p += nt) {
			jm_walk_picture(a.pics, s.n_pics, p, a.streams, a.n_streams, s.n_lanes, a.es_bytes, w);
			a.covered[p] = 0; a.done[(size_t)JM_DONE_STRIDE * p] = 0; a.stale[p] = JM_STALE_NONE;
		}
		for (uint32_t u = t; u < a.n_streams; u += nt) { a.ustart[u] = 0; a.uend[u] = 0; }
		if (t < 16) a.status[t] = t < 8 ? 0u : 0xffffffffu;
		if (w.n_decoded) {
			x.add64(&s.sums.n_decoded, w.n_decoded); x.add64(&s.sums.n_slices, w.n_slices); x.add64(&s.sums.long_slices, w.long_slices);
			x.add64(&s.sums.crit_bytes, w.crit_bytes); x.add64(&s.sums.crit_pics, w.crit_pics); x.add64(&s.sums.root_bytes, w.root_bytes);
			x.add64(&s.sums.roots, w.roots); x.add64(&s.sums.bytes, w.bytes);
		}
	});
	/* the parse's sizing (one lane); the decoded pictures of the streams, compacted in table order (each thread a run of the table) */
	x.par([&](uint32_t t, uint32_t nt) {
		if (t == 0) {
			JmDevPlan &P = *a.plan;
			P.n_sc = s.overflow ? 0u : a.counters[0];
			P.overflow = s.overflow; P.n_pics = s.n_pics;
			if (a.selected) jm_parse_sizing_from_walk(s.sums, jm_selected_lanes(s.sums, s.n_lanes), jm_selected_bytes(s.sums, a.es_bytes), a.mb_size, P.parse, nullptr);
			else jm_parse_sizing_from_walk(s.sums, s.n_lanes, a.es_bytes, a.mb_size, P.parse, nullptr);
			P.parse.debug_flags = a.debug_flags;
			if (P.parse.n_lanes) { bool tk = false; jm_plan_parse_rules(P.parse, a.ov, true, &tk); }
			else { P.parse.n_batches = 0; P.parse.lanes_per_wave = 64; P.parse.split_service = 0; P.parse.prio_batches = 0; }
		}
		const uint32_t chunk = (s.n_pics + nt - 1) / nt;
		uint32_t n = 0;
		for (uint32_t p = t * chunk; p < s.n_pics && p < (t + 1) * chunk; p++) n += jm_plan_in_unit(a.pics[p], a.n_streams);
		s.scan[0][t] = n;
	});
	uint32_t k = jm_plan_scan(x, s);
	x.par([&](uint32_t t, uint32_t nt) {
		const uint32_t chunk = (s.n_pics + nt - 1) / nt;
		uint32_t r = t ? s.scan[k][t - 1] : 0u;
		for (uint32_t p = t * chunk; p < s.n_pics && p < (t + 1) * chunk; p++) if (jm_plan_in_unit(a.pics[p], a.n_streams)) a.dec[r++] = p;
		if (t == nt - 1) s.n_dec = s.scan[k][t];
	});
	/* `stale` (the decoded picture before last of the stream: two places back in the list), the streams' runs; GOP chains counted */
	x.par([&](uint32_t t, uint32_t nt) {
		for (uint32_t r = t; r < s.n_dec; r += nt) {
			const uint32_t p = a.dec[r], st = a.pics[p].stream;
			if (r >= 2 && a.pics[a.dec[r - 2]].stream == st) a.stale[p] = (int32_t)a.dec[r - 2];
			if (jm_plan_stream_head(a.pics, a.dec, r)) a.ustart[st] = r;
			if (r + 1 == s.n_dec || a.pics[a.dec[r + 1]].stream != st) a.uend[st] = r + 1;
		}
		const uint32_t chunk = (s.n_dec + nt - 1) / nt;
		uint32_t n = 0;
		for (uint32_t r = t * chunk; r < s.n_dec && r < (t + 1) * chunk; r++) n += jm_plan_chain_head(a.pics, a.dec, r);
		s.scan[0][t] = n;
	});
	const bool tried_chains = a.try_chains != 0;
	k = jm_plan_scan(x, s);
	/* GOP chains: numbered in table order, each a run of the list */
	uint32_t *cstart = a.cstart, *cend = a.cend;
	x.par([&](uint32_t t, uint32_t nt) {
		const uint32_t chunk = (s.n_dec + nt - 1) / nt;
		uint32_t id = t ? s.scan[k][t - 1] : 0u;
		for (uint32_t r = t * chunk; r < s.n_dec && r < (t + 1) * chunk; r++) {
			if (jm_plan_chain_head(a.pics, a.dec, r)) { if (tried_chains) cstart[id] = r; id++; }
			a.chain_id[r] = id - 1;
			if (tried_chains && (r + 1 == s.n_dec || jm_plan_chain_head(a.pics, a.dec, r + 1))) cend[id - 1] = r + 1;
		}
		if (t == nt - 1) s.n_chains = s.scan[k][t];
	});
	if (s.overflow || s.n_dec == 0) return;
	/* by streams, when jm_plan_ordered accepts the batch; else by GOP chains */
	if (a.try_streams && a.n_streams >= 8 && a.n_streams <= JM_PLAN_SORT_CAP && a.group) {
		x.par([&](uint32_t t, uint32_t) { if (t == 0) s.n_units = a.n_streams; });
		jm_plan_deal(x, a, s, a.ustart, a.uend, a.streams_forced != 0);
		if (s.ok) { jm_plan_walk(x, a, s, a.ustart, a.uend); x.par([&](uint32_t t, uint32_t) { if (t == 0) s.kind = JM_PLAN_STREAMS; }); return; }
	}
	if (tried_chains && s.n_chains >= 8 && s.n_chains <= JM_PLAN_SORT_CAP && a.group) {
		x.par([&](uint32_t t, uint32_t) { if (t == 0) s.n_units = s.n_chains; });
		jm_plan_deal(x, a, s, cstart, cend, a.chains_forced != 0);
		if (s.ok) { jm_plan_walk(x, a, s, cstart, cend); x.par([&](uint32_t t, uint32_t) { if (t == 0) s.kind = JM_PLAN_CHAINS; }); return; }
	}
	x.par([&](uint32_t t, uint32_t) { if (t == 0) { s.rows = 0; s.lockstep = 0; for (uint32_t c = 0; c < 8; c++) s.load[c] = 0; } });
}

/* the plan block's reconstruct half (one lane, behind jm_plan_run) */
JM_HD void jm_plan_finish(const JmPlanArgs &a, const JmPlanShared &s) {
	JmDevPlan &P = *a.plan;
	P.kind = s.kind; P.rows = s.kind ? s.rows : 0; P.lockstep = s.kind ? s.lockstep : 0;
	P.n_chains = s.n_chains; P.n_units_dec = s.n_dec;
	for (uint32_t c = 0; c < 8; c++) P.load[c] = s.kind ? (uint32_t)s.load[c] : 0u;
}

/* slot k of the launch's 8 x rows_cap: the compacted list's place of its picture, or JM_NONE (padding) */
JM_HD uint32_t jm_plan_slot(const JmPlanArgs &a, const JmPlanShared &s, uint32_t k) {
	if (s.kind == JM_PLAN_HOST) return JM_NONE;
	return (k >> 3) < s.load[k & 7] ? a.seq[k] : JM_NONE;
}

#endif
