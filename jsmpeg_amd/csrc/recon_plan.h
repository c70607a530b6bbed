/*
 * The reconstruct plan of a batch (host code, no HIP in here: the engine calls it, and tests/sim compiles it for the CPU
 * tests).  A picture is reconstructed after its forward reference -- and, if it leaves macroblocks UNWRITTEN, after the
 * frame those keep showing: the reference keeps two plane sets and rotates them after every picture
 * (src/wasm/mpeg1.c:986-994), so a macroblock a picture never writes -- e.g. a last macroblock of 6 bits that hides in
 * the slack of its slice's last byte, mpeg1.c:1018-1020 -- keeps the decoded picture BEFORE LAST of its stream.  Here
 * every picture has its own frame; that picture's frame is the `stale` of the one at hand.
 */
#ifndef JSMPEG_AMD_RECON_PLAN_H
#define JSMPEG_AMD_RECON_PLAN_H

#include <stdint.h>

#include <algorithm>
#include <vector>

#include "mpeg1_dev.h"

/* What a stream's unwritten macroblocks may keep showing that is NOT a picture of this stream in this batch
 * (jsmpeg_hip_batch_link_streams / _seed_stream: a stream that CONTINUES another -- the (stream, GOP) units a sharded
 * job cuts its streams into):
 *   link_prev[s] >= 0: stream s continues stream link_prev[s] of this batch (link_prev[s] < s): its plane rotation goes on
 *                      where that stream's ended;
 *   seeded[s] bit 0 / 1: the caller gave the frame of the decoded picture last / before last in front of stream s
 *                      (decoded elsewhere: another rank, an earlier batch).
 * Both null: every stream starts with zeroed planes (the JS typed arrays start zeroed, mpeg1.js:131-152). */
#define JM_STALE_NONE (-1)
static inline int32_t jm_stale_seed(uint32_t stream, int which) { return -2 - (int32_t)(2 * stream + (uint32_t)which); }   /* which: 0 last, 1 before last */
static inline bool jm_stale_is_seed(int32_t v) { return v <= -2; }
static inline uint32_t jm_stale_seed_slot(int32_t v) { return (uint32_t)(-2 - v); }                                         /* 2 * stream + which */

/* stale[p]: what p's unwritten macroblocks show -- the decoded picture before last of p's stream (>= 0), a seeded frame
 * (jm_stale_is_seed), or JM_STALE_NONE (zeros).  Returns the number of decoded pictures without a forward reference. */
static inline uint32_t jm_plan_stale(const JmPic *pics, uint32_t n_pics, uint32_t n_streams, std::vector<int32_t> &stale,
                                     const int32_t *link_prev = nullptr, const uint8_t *seeded = nullptr) {
	stale.assign(n_pics, JM_STALE_NONE);
	std::vector<int32_t> last1(n_streams, JM_STALE_NONE), last2(n_streams, JM_STALE_NONE);      /* the stream's last two decoded pictures */
	std::vector<uint8_t> begun(n_streams, 0);
	uint32_t n_roots = 0;
	for (uint32_t p = 0; p < n_pics; p++) {
		const JmPic &pic = pics[p];
		if (!pic.decoded) continue;
		if (pic.fwd < 0) n_roots++;
		const uint32_t s = pic.stream;
		if (s >= n_streams) continue;
		if (!begun[s]) {
			begun[s] = 1;
			if (link_prev && link_prev[s] >= 0 && (uint32_t)link_prev[s] < s) { last1[s] = last1[link_prev[s]]; last2[s] = last2[link_prev[s]]; }
			else if (seeded) {
				if (seeded[s] & 1) last1[s] = jm_stale_seed(s, 0);
				if (seeded[s] & 2) last2[s] = jm_stale_seed(s, 1);
			}
		}
		stale[p] = last2[s]; last2[s] = last1[s]; last1[s] = (int32_t)p;
	}
	return n_roots;
}

/* level[p] of every decoded picture once the parse has reported the macroblock records each picture wrote
 * (`covered[p]` of `mb_size`): 0 for a picture without a forward reference and nothing unwritten, else one more than
 * the deepest of what it waits for.  Pictures are in stream order, so fwd < p and stale < p: one pass.  Returns the
 * number of levels; *n_uncovered: pictures with unwritten macroblocks. */
static inline uint32_t jm_plan_levels(const JmPic *pics, uint32_t n_pics, const std::vector<int32_t> &stale, const uint32_t *covered,
                                      uint32_t mb_size, std::vector<int32_t> &level, uint32_t *n_uncovered) {
	level.assign(n_pics, 0);
	uint32_t n_levels = 0, unc = 0;
	for (uint32_t p = 0; p < n_pics; p++) {
		const JmPic &pic = pics[p];
		if (!pic.decoded) continue;
		const bool uncovered = covered[p] < mb_size;
		unc += uncovered;
		int32_t l = pic.fwd >= 0 ? level[pic.fwd] + 1 : 0;
		if (uncovered && stale[p] >= 0) l = std::max(l, level[stale[p]] + 1);
		level[p] = l;
		n_levels = std::max(n_levels, (uint32_t)l + 1);
	}
	if (n_uncovered) *n_uncovered = unc;
	return n_levels;
}

/* THE ORDERED PLAN: one reconstruct launch for the whole batch (kernels.h, JmReconBufs::need).  Streams are dealt to
 * eight CLASSES (a class = the workgroups b with b % 8 == c = one XCD: one dispatcher that starts its blocks in order,
 * one L2); a class takes its streams `group` at a time and walks them in lockstep -- picture i of stream A, picture i of
 * stream B, picture i + 1 of A ... -- so that a picture's forward reference (the picture before it in its stream) lies
 * `group` pictures back in the class's dispatch order: far enough, in workgroups, to be finished or about to be when the
 * picture's first tile looks (the caller picks `group` by the tiles a picture has).
 *   seq[8 i + c] = the i-th picture of class c, -1 = padding;   lockstep = the narrowest class's streams in lockstep.
 * A picture's dependencies -- its forward reference, and for a tile with a macroblock the picture never wrote the
 * frame that keeps showing there (jm_plan_stale) -- are earlier pictures of its own stream: earlier in its class.
 * Returns false when the batch does not fill eight classes evenly (fewer than eight streams, or a class more than
 * `slack_pct` percent above the mean): the caller then launches level by level. */
struct JmOrderedPlan { std::vector<int32_t> seq; uint32_t rows, lockstep; };
static inline bool jm_plan_ordered(const JmPic *pics, uint32_t n_pics, uint32_t n_streams, uint32_t group, uint32_t slack_pct, JmOrderedPlan &out,
                                   const int32_t *link_prev = nullptr) {
	out.seq.clear(); out.rows = 0; out.lockstep = 0;
	if (n_streams < 8 || group == 0) return false;
	/* streams that continue one another (link_prev) are ONE stream here: the chain's first stream carries them all, in
	 * order -- a chain stays in its class, and a continuing stream's `stale` frames lie earlier in it */
	std::vector<uint32_t> root(n_streams);
	uint32_t n_chains = 0;
	for (uint32_t s = 0; s < n_streams; s++) {
		root[s] = link_prev && link_prev[s] >= 0 && (uint32_t)link_prev[s] < s ? root[link_prev[s]] : s;
		n_chains += root[s] == s;
	}
	if (n_chains < 8) return false;
	std::vector<std::vector<int32_t>> of(n_streams);
	uint64_t total = 0;
	for (uint32_t p = 0; p < n_pics; p++) {
		const JmPic &pic = pics[p];
		if (!pic.decoded || pic.stream >= n_streams) continue;
		of[root[pic.stream]].push_back((int32_t)p);
		total++;
	}
	if (total == 0) return false;
	/* longest stream first onto the class with the least so far (equal streams: round robin) */
	std::vector<uint32_t> by(n_streams);
	for (uint32_t s = 0; s < n_streams; s++) by[s] = s;
	std::stable_sort(by.begin(), by.end(), [&](uint32_t a, uint32_t b) { return of[a].size() > of[b].size(); });
	std::vector<uint32_t> cls[8];
	uint64_t load[8] = { 0 };
	for (uint32_t s : by) {
		if (of[s].empty()) continue;
		uint32_t best = 0;
		for (uint32_t c = 1; c < 8; c++) if (load[c] < load[best]) best = c;
		cls[best].push_back(s); load[best] += of[s].size();
	}
	const uint64_t most = *std::max_element(load, load + 8);
	if (most * 8 * 100 > total * (100 + slack_pct)) return false;
	out.rows = (uint32_t)most;
	out.seq.assign((size_t)8 * out.rows, -1);
	out.lockstep = group;
	for (uint32_t c = 0; c < 8; c++) out.lockstep = std::min<uint32_t>(out.lockstep, (uint32_t)cls[c].size());
	for (uint32_t c = 0; c < 8; c++) {
		std::vector<uint32_t> active, at;            /* the streams walked in lockstep, and where each one is */
		size_t next = 0, i = 0;
		/* how many at a time: `group` -- or a few more, so that the class's LAST set is not a remainder of fewer than
		 * `group` (five chains two at a time would end with one chain walking alone: every picture right behind its
		 * reference; three, then two, do not) */
		size_t width = std::min<size_t>(group, cls[c].size());
		while (width < cls[c].size() && cls[c].size() % width != 0 && cls[c].size() % width < group) width++;
		while (active.size() < width && next < cls[c].size()) { active.push_back(cls[c][next++]); at.push_back(0); }
		while (!active.empty()) {
			for (size_t a = 0; a < active.size();) {
				const std::vector<int32_t> &l = of[active[a]];
				out.seq[8 * i++ + c] = l[at[a]++];
				if (at[a] < l.size()) { a++; continue; }
				if (next < cls[c].size()) { active[a] = cls[c][next++]; at[a] = 0; a++; }   /* the next stream takes the place */
				else { active.erase(active.begin() + (long)a); at.erase(at.begin() + (long)a); }
			}
		}
	}
	return true;
}

/* GOP CHAINS of a batch (the ordered plan of NARROW batches: classes walk chains instead of streams): chain[p] = the
 * number of the chain decoded picture p belongs to -- a new chain begins at every decoded picture without a forward
 * reference and at a stream's first decoded picture -- JM_NONE for pictures that are not decoded.  Returns the number of
 * chains.  by_chain (optional): a copy of the picture table with the chain number in place of the stream number, which
 * is what jm_plan_ordered then deals to the classes. */
static inline uint32_t jm_plan_chains(const JmPic *pics, uint32_t n_pics, uint32_t n_streams, std::vector<uint32_t> &chain, std::vector<JmPic> *by_chain) {
	chain.assign(n_pics, JM_NONE);
	if (by_chain) by_chain->assign(pics, pics + n_pics);
	std::vector<int32_t> cur(n_streams, -1);
	uint32_t n_chains = 0;
	for (uint32_t p = 0; p < n_pics; p++) {
		const JmPic &pic = pics[p];
		if (!pic.decoded || pic.stream >= n_streams) continue;
		if (pic.fwd < 0 || cur[pic.stream] < 0) cur[pic.stream] = (int32_t)n_chains++;
		chain[p] = (uint32_t)cur[pic.stream];
		if (by_chain) (*by_chain)[p].stream = chain[p];
	}
	return n_chains;
}

/* WHICH PLAN a pass takes (jm_choose_recon below).  The ordered launch: how far back, in workgroups of its class's dispatch order, the LAST tile of a picture's forward
 * reference should lie behind the picture's FIRST tile: (streams in lockstep - 1) x tiles per picture.
 * A class (32 CUs) holds 160 workgroups at a time; 200 back is finished but for stragglers (cfg2, 200 tiles per picture,
 * two streams in lockstep: 0-1000 unfinished first looks in 1.5 M; one stream in lockstep, distance 1: 1.16 M, three times
 * the time; 4K, 816 tiles, one stream: 0.87 M).  Below the residency the per-level launches are the better form (small
 * pictures with few streams per class).
 * Late in round 6 the distance aimed at went from 200 to 400: on CODED video (encoder-made 1080p, profiles/r06k_enc_content.md)
 * a predicted picture's tiles are mostly copies and run up against a forward reference only 204 tiles ahead -- two 1080p streams
 * in lockstep: 339 k waits, the launch 18.9 ms against 10.2 with three (0 waits; four, six, eight the same) -- and the generator's
 * cfg2 is the same with three within a box's noise (alternating on two boxes, three rounds each: 11.03-11.05 against 11.11-11.16 ms
 * on one, 11.17-11.22 against 11.14-11.15 on the other: profiles/r06n_order_ab.txt, r06o_order_ab.txt; 720p goes from four streams
 * in lockstep to six: 5.01 against 5.06). */
#define JM_ORDER_DISTANCE 400u
#define JM_ORDER_MIN_DISTANCE 160u
/* WIDE batches go level by level (late round 6, profiles/r06n_levels_vs_ordered.txt): from ~2.5 M macroblocks per level up
 * -- 32 streams x 120 pictures of 1080p, the headline's 64 x 120 -- a level's launch is long against the gap behind it and the
 * two plans take the same time (11.151 against 11.152 ms, 5.745 / 5.734); below that the one launch is 1-12 % faster and stays.
 * What the levels have for them where they cost nothing: they share the GPU better with another batch in flight (582.6 k
 * against 554.1 k frames/s), and they stand on kernel boundaries, not on the ordered launch's argument about one XCD's L2
 * (kernels.hip jm_recon_wait). */
#define JM_WIDE_LEVEL_MBS 2500000u
/* A launch without a forward frame in any picture takes the tile's form without prediction (k_recon_intra) -- and, when those
 * pictures are DENSE (bytes of compressed data per macroblock: practically every block has AC coefficients, a tile needs a
 * transform slot per lane), the variant with 256 slots (cfg0, 21 bytes per macroblock, -6 %; cfg2's intra pictures, 12.7, +11 %:
 * profiles/r04_recon_notes.md 8).  Only a launch without predicted pictures can take it, so a batch left to itself with dense
 * intra pictures (cfg4's: 27) and a shallow dependency structure goes level by level: 2160p 64 x 24: reconstruct 10.73-10.81 ms
 * against 11.05-11.18 in one ordered launch.  In sixteenths: 19.4 bytes per macroblock (all-intra 1080p at 18.0 is 5 % faster
 * with 220 slots, at 20.7 5 % faster with 256). */
#define JM_DENSE_INTRA_X16 310

/* What decides a batch's plan besides its pictures (engine_internal.h: set when the batch is created, the environment
 * variables read then). */
struct JmReconPolicy {
	bool levels;        /* the host's setting (jsmpeg_hip_batch_set_reconstruct 0): always level by level */
	int32_t order;      /* JSMPEG_HIP_RECON_ORDER: < 0 not set (the engine's choice), 0 level by level, n streams in lockstep */
	int dense;          /* JSMPEG_HIP_RECON_DENSE: -1 by the intra pictures' bytes per macroblock, 0 / 1 never / always the dense form */
	bool chains;        /* JSMPEG_HIP_RECON_CHAINS: GOP chains whatever the batch's shape */
	int32_t brk;        /* JSMPEG_HIP_RECON_BREAK: picture n of the ordered plan never reports (< 0: none) */
	uint32_t patience;  /* JSMPEG_HIP_RECON_PATIENCE: polls before an ordered wait gives up (0: the kernel's) */
	bool demoted;       /* an ordered launch flagged itself: level by level from then on, whatever is set */
};

enum JmReconKind { JM_RECON_LEVELS, JM_RECON_BY_STREAMS, JM_RECON_BY_CHAINS };

/* The plan of a pass whose picture table has arrived (before the parse has reported anything).  n_roots: decoded pictures
 * without a forward reference (jm_plan_stale), roots_x16 their compressed bytes per macroblock in sixteenths; link_prev: as
 * for jm_plan_stale; linked_or_seeded: a stream continues another or was seeded (the GOP chains' assumption fails then).
 * Fills `plan` for the ordered kinds, `chain_of` (jm_plan_chains) for JM_RECON_BY_CHAINS. */
static inline JmReconKind jm_choose_recon(const JmPic *pics, uint32_t n_pics, uint32_t n_streams, uint32_t n_decoded, uint32_t n_roots,
                                          uint32_t mb_size, uint32_t tiles_per_picture, uint32_t desc_cap, uint32_t roots_x16,
                                          const int32_t *link_prev, bool linked_or_seeded, const JmReconPolicy &pol,
                                          JmOrderedPlan &plan, std::vector<uint32_t> &chain_of) {
	chain_of.clear();
	const bool own = !pol.levels && !pol.demoted && pol.order < 0;          /* the engine's own choice */
	const uint32_t group = pol.levels || pol.demoted ? 0u
	                     : own ? 1 + (JM_ORDER_DISTANCE + tiles_per_picture - 1) / tiles_per_picture : (uint32_t)pol.order;
	/* (a batch without a single predicted picture has nothing to order: one plain launch) */
	if (n_roots >= n_decoded || group == 0) return JM_RECON_LEVELS;
	if (own && !pol.chains) {
		int32_t deepest = 0;
		for (uint32_t p = 0; p < n_pics; p++) if (pics[p].decoded) deepest = std::max(deepest, pics[p].level);
		if (deepest < 16 && pol.dense != 0 && roots_x16 >= JM_DENSE_INTRA_X16) return JM_RECON_LEVELS;
		if (deepest < 16 && (uint64_t)n_decoded * std::max(1u, mb_size) >= (uint64_t)JM_WIDE_LEVEL_MBS * (uint64_t)(deepest + 1)) return JM_RECON_LEVELS;
	}
	const auto fits = [&](bool far_enough_or_forced) {
		return (size_t)8 * plan.rows <= desc_cap && (far_enough_or_forced || (plan.lockstep - 1) * tiles_per_picture >= JM_ORDER_MIN_DISTANCE);
	};
	if (!pol.chains && jm_plan_ordered(pics, n_pics, n_streams, group, 8, plan, link_prev) && fits(!own)) return JM_RECON_BY_STREAMS;
	/* NARROW batches (fewer than eight streams, or streams of very different lengths: one file of many GOPs): the classes walk
	 * GOP CHAINS instead of streams -- a chain = an intra picture and the P pictures behind it.  The one thing that crosses
	 * chains is the `stale` frame of a chain's first two pictures (it belongs to the GOP before, maybe another class's): the
	 * plan assumes those pictures write every macroblock -- intra pictures and a GOP's first P picture practically always
	 * do -- and the engine CHECKS the assumption once the parse's counts are in: a picture that did not is done over, with
	 * everything else, level by level. */
	if ((own || pol.chains) && !linked_or_seeded) {
		std::vector<JmPic> by_chain;
		const uint32_t n_chains = jm_plan_chains(pics, n_pics, n_streams, chain_of, &by_chain);
		if (n_chains >= 8 && jm_plan_ordered(by_chain.data(), n_pics, n_chains, group, 8, plan) && fits(pol.chains)) return JM_RECON_BY_CHAINS;
		chain_of.clear();
	}
	return JM_RECON_LEVELS;
}

#endif
