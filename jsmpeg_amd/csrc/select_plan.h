/*
 * A pass over SELECTED frames only (jsmpeg_hip_batch_select, include/jsmpeg_hip.h part 2): the rules of kernels.hip
 * k_select, which runs right behind k_index when a selection is set, and their plain sequential definition -- what
 * tests/sim/sim_select.cpp checks the scan form against, as index_tables.h holds jm_index_chain beside k_index's scans.
 *
 * A request names a FRAME of a stream as a user of the reference counts them: the n-th picture the whole decode would
 * decode (JmPic::decoded), in stream order, from 0.  The host lays the requests out as one bitmap over frame numbers per
 * stream (JmSelectLayout); the device
 *   1. marks the selected pictures by the count of decoded pictures (k_index's scan, taken again) and writes the picture
 *      of every frame number the bitmap covers (frame_pic: the host maps request -> frame -> picture);
 *   2. marks as NEEDED every decoded picture from its chain's anchor (level == 0: an intra picture, or the stream's first
 *      decoded picture) up to the chain's last selected picture -- in an I / P stream a picture's forward reference is the
 *      decoded picture before it, so that is the closure over forward references;
 *   3. DROPS every other decoded picture: decoded = 0, n_slices = 0, its slice codes' owner back to JM_NONE, and
 *      JM_PIC_SEL_DROPPED in JmPic::pad_ -- the picture then goes through every plan the way the B / D pictures do that the
 *      reference consumes without decoding; the flag tells the two apart (frame numbers count the dropped ones);
 *   4. records for every picture of the whole decode the stream's decoded picture BEFORE LAST in the whole decode
 *      (before_last): what a picture's unwritten macroblocks keep showing (recon_plan.h) -- the planners of the thinned
 *      pass take "two places back" in the THINNED list, and the engine checks the two against each other for the pictures
 *      that turn out to leave macroblocks unwritten (jm_select_widen below);
 *   5. sums the needed pictures, their slices and their deepest level.
 *
 * The closure as scans (no lane chases fwd pointers): with nextSel(p) = the first selected picture at or behind p and
 * nextAnchor(p) = the first anchor strictly behind p,
 *      needed(p) = decoded(p) and nextSel(p) exists and nextSel(p) < nextAnchor(p)
 * -- two reverse min-scans over the stream's pictures, a chunk of lanes at a time with a carry, the chunks walked backwards.
 */
#ifndef JSMPEG_AMD_SELECT_PLAN_H
#define JSMPEG_AMD_SELECT_PLAN_H

#include <stdint.h>

#include "mpeg1_dev.h"

/* JmPic::pad_ of a pass with a selection (0 in every other pass) */
#define JM_PIC_SEL_DROPPED 1u      /* the whole decode decodes this picture; this pass did not need it */
#define JM_PIC_SEL_SELECTED 2u     /* a request names this picture */

/* The requests as the device reads them: stream s owns frame numbers [0, nbits[s]) -- bit (off[s] + f) of `bits` says frame
 * f is selected, frame_pic[off[s] + f] receives its picture (JM_NONE: the stream has no such frame); off[s] is a multiple
 * of 32 and off[n_streams] the total. */
struct JmSelectLayout {
	const uint32_t *bits;
	const uint32_t *off;       /* [n_streams + 1] */
	const uint32_t *nbits;     /* [n_streams] */
};
struct JmSelectTotals { uint32_t needed, slices, levels; };   /* levels: the needed pictures' deepest level + 1 */

/* ------------------------------------------------------------------ per-lane rules */

JM_HD bool jm_select_bit(const JmSelectLayout &l, uint32_t stream, uint32_t frame) {
	if (frame >= l.nbits[stream]) return false;
	const uint32_t i = l.off[stream] + frame;
	return (l.bits[i >> 5] >> (i & 31)) & 1u;
}
/* the whole decode's decoded picture before last of a decoded picture: `rank` = its place among the chunk's decoded pictures
 * (byrank: those, compacted), last1 / last2 = the stream's last two decoded pictures in front of the chunk (-1: none) */
JM_HD int32_t jm_select_before_last(const int32_t *byrank, uint32_t rank, int32_t last1, int32_t last2) {
	return rank >= 2 ? byrank[rank - 2] : rank == 1 ? last1 : last2;
}
/* the carries behind a chunk of n decoded pictures */
JM_HD void jm_select_carry_last(const int32_t *byrank, uint32_t n, int32_t &last1, int32_t &last2) {
	const int32_t l1 = n >= 1 ? byrank[n - 1] : last1;
	const int32_t l2 = n >= 2 ? byrank[n - 2] : n == 1 ? last1 : last2;
	last1 = l1; last2 = l2;
}
/* a chain begins here: the reverse walk's closure stops behind it (k_index: level 0 = not a P picture, or the stream's first) */
JM_HD bool jm_select_anchor(const JmPic &pic) { return pic.decoded && pic.level == 0; }
/* next_sel / next_anchor: picture numbers, JM_NONE = none */
JM_HD bool jm_select_needed(bool decoded, uint32_t next_sel, uint32_t next_anchor) {
	return decoded && next_sel != JM_NONE && next_sel < next_anchor;
}
/* a decoded picture the pass does not need (the lane that owns the picture; its slice codes are its own) */
JM_HD void jm_select_drop(JmPic &pic, uint32_t *sc_owner) {
	for (uint32_t k = 0; k < pic.n_slices; k++) sc_owner[pic.first_slice_sc + k] = JM_NONE;
	pic.decoded = 0; pic.n_slices = 0; pic.pad_ |= JM_PIC_SEL_DROPPED;
}

/* ------------------------------------------------------------------ the sequential definition */

/* One stream, pictures [lo, hi) of the table as k_index left it.  before_last: [n_pics], -1 where there is none or the
 * picture is not one of the whole decode's. */
static inline void jm_select_stream(JmPic *pics, uint32_t lo, uint32_t hi, uint32_t stream, const JmSelectLayout &l, uint32_t *frame_pic,
                                    int32_t *before_last, uint32_t *sc_owner, JmSelectTotals &tot) {
	for (uint32_t f = 0; f < l.nbits[stream]; f++) frame_pic[l.off[stream] + f] = JM_NONE;
	uint32_t frame = 0;
	int32_t last1 = -1, last2 = -1;
	for (uint32_t p = lo; p < hi; p++) {
		JmPic &pic = pics[p];
		before_last[p] = -1;
		if (!pic.decoded) continue;
		before_last[p] = last2; last2 = last1; last1 = (int32_t)p;
		if (frame < l.nbits[stream]) frame_pic[l.off[stream] + frame] = p;
		if (jm_select_bit(l, stream, frame)) pic.pad_ |= JM_PIC_SEL_SELECTED;
		frame++;
	}
	bool want = false;
	for (uint32_t p = hi; p-- > lo;) {
		JmPic &pic = pics[p];
		if (!pic.decoded) continue;
		if (pic.pad_ & JM_PIC_SEL_SELECTED) want = true;
		const bool needed = want;
		if (jm_select_anchor(pic)) want = false;
		if (!needed) { jm_select_drop(pic, sc_owner); continue; }
		tot.needed++; tot.slices += pic.n_slices;
		if ((uint32_t)pic.level + 1 > tot.levels) tot.levels = (uint32_t)pic.level + 1;
	}
}

/* ------------------------------------------------------------------ the scan form, chunk by chunk */

/* What k_select does with W lanes, the lanes as loops: the same rules, the same carries, the same order of the chunks.
 * scratch: 3 * W words. */
static inline void jm_select_stream_chunked(JmPic *pics, uint32_t lo, uint32_t hi, uint32_t stream, const JmSelectLayout &l, uint32_t *frame_pic,
                                            int32_t *before_last, uint32_t *sc_owner, JmSelectTotals &tot, uint32_t W, int32_t *scratch) {
	for (uint32_t f = 0; f < l.nbits[stream]; f++) frame_pic[l.off[stream] + f] = JM_NONE;
	int32_t *byrank = scratch;
	uint32_t *sel_at = (uint32_t *)scratch + W, *anchor_behind = (uint32_t *)scratch + 2 * W;
	/* forward: frame numbers, the selected pictures, before_last */
	uint32_t c0 = 0;
	int32_t last1 = -1, last2 = -1;
	for (uint32_t base = lo; base < hi; base += W) {
		uint32_t n = 0;
		for (uint32_t t = 0; t < W && base + t < hi; t++) if (pics[base + t].decoded) byrank[n++] = (int32_t)(base + t);   /* the compaction: a scan's place */
		uint32_t rank = 0;
		for (uint32_t t = 0; t < W && base + t < hi; t++) {
			const uint32_t p = base + t;
			JmPic &pic = pics[p];
			before_last[p] = -1;
			if (!pic.decoded) continue;
			const uint32_t frame = c0 + rank;
			before_last[p] = jm_select_before_last(byrank, rank, last1, last2);
			if (frame < l.nbits[stream]) frame_pic[l.off[stream] + frame] = p;
			if (jm_select_bit(l, stream, frame)) pic.pad_ |= JM_PIC_SEL_SELECTED;
			rank++;
		}
		jm_select_carry_last(byrank, n, last1, last2);
		c0 += n;
	}
	/* backwards: the closure */
	uint32_t carry_sel = JM_NONE, carry_anchor = JM_NONE;
	const uint32_t n_chunks = (hi - lo + W - 1) / W;
	for (uint32_t c = n_chunks; c-- > 0;) {
		const uint32_t base = lo + c * W;
		/* lane t takes picture base + W - 1 - t: an inclusive min-scan up the lanes for the selected pictures, the same one
		 * lane down (exclusive) for the anchors */
		uint32_t run_sel = carry_sel, run_anchor = carry_anchor;
		for (uint32_t t = 0; t < W; t++) {
			const uint32_t p = base + W - 1 - t;
			anchor_behind[t] = run_anchor;
			if (p < hi && pics[p].decoded) {
				if ((pics[p].pad_ & JM_PIC_SEL_SELECTED) && p < run_sel) run_sel = p;
				if (jm_select_anchor(pics[p]) && p < run_anchor) run_anchor = p;
			}
			sel_at[t] = run_sel;
		}
		for (uint32_t t = 0; t < W; t++) {
			const uint32_t p = base + W - 1 - t;
			if (p >= hi || !pics[p].decoded) continue;
			JmPic &pic = pics[p];
			if (!jm_select_needed(true, sel_at[t], anchor_behind[t])) { jm_select_drop(pic, sc_owner); continue; }
			tot.needed++; tot.slices += pic.n_slices;
			if ((uint32_t)pic.level + 1 > tot.levels) tot.levels = (uint32_t)pic.level + 1;
		}
		carry_sel = run_sel; carry_anchor = run_anchor;
	}
}

/* ------------------------------------------------------------------ unwritten macroblocks: exact, or widened */

/* Once the parse's counts are in.  pics: the THINNED table of the pass; stale[p]: what the pass's plan took for p's unwritten
 * macroblocks (recon_plan.h jm_plan_stale over the thinned table: >= 0 a picture, < 0 zeros); before_last[p]: the whole
 * decode's.  The pass is exact unless a needed picture with unwritten macroblocks (covered[p] < mb_size) showed another
 * frame than the whole decode shows there: its stream is then WIDENED -- widen[stream] = 1 + the frame number of the stream's
 * last needed picture: the selection becomes every frame up to that one, a prefix from the stream's beginning, which IS the
 * whole decode of those pictures (one pass over again always suffices).  widen: [n_streams], 0 where nothing changes.
 * Returns the streams widened. */
static inline uint32_t jm_select_widen(const JmPic *pics, uint32_t n_pics, uint32_t n_streams, const int32_t *stale, const int32_t *before_last,
                                       const uint32_t *covered, uint32_t mb_size, uint32_t *widen) {
	for (uint32_t s = 0; s < n_streams; s++) widen[s] = 0;
	uint32_t n = 0;
	for (uint32_t p = 0; p < n_pics; p++) {
		const JmPic &pic = pics[p];
		if (!pic.decoded || pic.stream >= n_streams || covered[p] >= mb_size) continue;
		const int32_t used = stale[p] >= 0 ? stale[p] : -1;
		if (used != before_last[p] && !widen[pic.stream]) { widen[pic.stream] = 1; n++; }
	}
	if (!n) return 0;
	/* frame numbers count the pictures of the whole decode: the needed ones and the dropped ones */
	uint32_t frame = 0;
	for (uint32_t p = 0; p < n_pics; p++) {
		const JmPic &pic = pics[p];
		if (pic.stream >= n_streams) continue;
		if (p == 0 || pics[p - 1].stream != pic.stream) frame = 0;
		if (!pic.decoded && !(pic.pad_ & JM_PIC_SEL_DROPPED)) continue;
		frame++;
		if (pic.decoded && widen[pic.stream]) widen[pic.stream] = frame;
	}
	return n;
}

#endif
