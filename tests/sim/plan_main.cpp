// TEST INFRASTRUCTURE ONLY -- not part of the product, never shipped or loaded by it.  Runs the device planner of an
// enqueued pass (jsmpeg_amd/csrc/enqueue_plan.h jm_plan_run: what k_plan runs on one workgroup) on the CPU, stage by stage
// with every "thread" of a stage one after the other, and checks what it writes against the host path's own functions
// (recon_plan.h jm_plan_stale / jm_plan_ordered / jm_plan_chains, the walk and the parse rules).  tests/test_enqueue_plan.py
// builds it with g++ and feeds it random picture tables.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "enqueue_plan.h"

struct CpuExec {
	uint32_t nt;
	template <class F> void par(F f) { for (uint32_t t = 0; t < nt; t++) f(t, nt); }
	void add64(uint64_t *p, uint64_t v) { *p += v; }
};

static char g_msg[512];
#define CHECK(cond, ...) do { if (!(cond)) { snprintf(g_msg, sizeof g_msg, __VA_ARGS__); return 1; } } while (0)

extern "C" const char *sim_plan_message(void) { return g_msg; }

/* the table: per picture stream, decoded, fwd, n_slices, pos; per stream es_end.  knobs[]: 0 group, 1 tiles per picture,
 * 2 try_streams, 3 try_chains, 4 streams_forced, 5 chains_forced, 6 brk, 7 rows_cap, 8 overflow, 9 n_sc, 10 slice codes,
 * 11 sc_cap, 12 es_bytes, 13 mb_size, 14 split override (-1), 15 head override set, 16..19 head a, l0, h, l1.
 * out[]: 0 kind, 1 rows, 2 lockstep, 3 n_lanes, 4 long_slices, 5 bytes_per_mb_x16, 6 split, 7 lanes_per_wave, 8 n_batches,
 * 9 t_cold, 10 head_lanes[0], 11 head batches, 12 head_first[2], 13 prio_batches, 14 n_chains, 15 host kind */
extern "C" int sim_plan_check(uint32_t n_pics, const uint32_t *stream, const uint8_t *decoded, const int32_t *fwd, const uint32_t *n_slices,
                              const uint32_t *pos, uint32_t n_streams, const uint32_t *es_end, const int32_t *knobs, uint32_t *out) {
	g_msg[0] = 0;
	const uint32_t pic_cap = n_pics + 8;
	std::vector<JmPic> pics(pic_cap);
	memset(pics.data(), 0, sizeof(JmPic) * pic_cap);
	for (uint32_t p = 0; p < n_pics; p++) {
		JmPic &q = pics[p];
		q.stream = stream[p]; q.decoded = decoded[p]; q.fwd = fwd[p]; q.n_slices = n_slices[p]; q.pos = pos[p];
		q.type = fwd[p] >= 0 ? 2 : 1; q.mb_index = p;
	}
	std::vector<JmStream> streams(n_streams + 1);
	memset(streams.data(), 0, sizeof(JmStream) * streams.size());
	for (uint32_t s = 0; s < n_streams; s++) streams[s].es_end = es_end[s];
	uint32_t counters[8] = { (uint32_t)knobs[9], n_pics, (uint32_t)knobs[8], 0, (uint32_t)knobs[10], 0, 0, 0 };
	const uint32_t rows_cap = (uint32_t)knobs[7];
	std::vector<uint32_t> dec(pic_cap), chain_id(pic_cap), cstart(pic_cap), cend(pic_cap), ustart(n_streams + 1), uend(n_streams + 1),
		seq(8 * (size_t)rows_cap + 8), covered(pic_cap, 7), done((size_t)JM_DONE_STRIDE * pic_cap, 7), status(16, 7);
	std::vector<int32_t> stale(pic_cap, 7);
	JmDevPlan plan;
	memset(&plan, 0xab, sizeof plan);
	JmPlanArgs a;
	memset(&a, 0, sizeof a);
	a.counters = counters; a.pics = pics.data(); a.streams = streams.data();
	a.n_streams = n_streams; a.es_bytes = (uint32_t)knobs[12]; a.sc_cap = (uint32_t)knobs[11]; a.pic_cap = pic_cap;
	a.mb_size = knobs[13]; a.debug_flags = 0;
	a.ov.lanes = 0; a.ov.t_cold = 0; a.ov.split = knobs[14]; a.ov.prio = -1; a.ov.resident = JM_PARSE_RESIDENT_WGS; a.ov.even = 1;
	a.ov.head_set = (uint32_t)knobs[15]; a.ov.head_a = (uint32_t)knobs[16]; a.ov.head_l0 = (uint32_t)knobs[17];
	a.ov.head_h = (uint32_t)knobs[18]; a.ov.head_l1 = (uint32_t)knobs[19];
	a.rows_cap = rows_cap; a.tiles_per_picture = (uint32_t)knobs[1]; a.group = (uint32_t)knobs[0];
	a.try_streams = (uint32_t)knobs[2]; a.try_chains = (uint32_t)knobs[3]; a.streams_forced = (uint32_t)knobs[4]; a.chains_forced = (uint32_t)knobs[5];
	a.brk = knobs[6];
	a.dec = dec.data(); a.chain_id = chain_id.data(); a.ustart = ustart.data(); a.uend = uend.data(); a.cstart = cstart.data(); a.cend = cend.data();
	a.seq = seq.data(); a.stale = stale.data(); a.plan = &plan; a.covered = covered.data(); a.done = done.data(); a.status = status.data();
	std::unique_ptr<JmPlanShared> sh(new JmPlanShared());
	CpuExec x{ JM_PLAN_THREADS };
	jm_plan_run(x, a, *sh);
	jm_plan_finish(a, *sh);
	const bool overflow = knobs[8] != 0;
	const uint32_t np = overflow ? 0 : n_pics;

	/* the launches start from zeroed counts */
	for (uint32_t p = 0; p < np; p++) CHECK(covered[p] == 0 && done[(size_t)JM_DONE_STRIDE * p] == 0, "picture %u: covered / done not zeroed", p);
	for (uint32_t i = 0; i < 16; i++) CHECK(status[i] == (i < 8 ? 0u : 0xffffffffu), "status word %u", i);

	/* stale = jm_plan_stale */
	std::vector<int32_t> want_stale;
	const uint32_t n_roots = jm_plan_stale(pics.data(), np, n_streams, want_stale);
	(void)n_roots;
	for (uint32_t p = 0; p < np; p++) CHECK(stale[p] == want_stale[p], "stale[%u] = %d, jm_plan_stale %d", p, stale[p], want_stale[p]);

	/* the parse's sizing = the host's walk + rules (collect_index / enqueue_parse / jm_plan_parse) */
	JmWalkSums w = { 0, 0, 0, 0, 0, 0, 0 };
	const uint32_t lanes = overflow ? 0 : jm_umin(counters[4], a.sc_cap);
	for (uint32_t p = 0; p < np; p++) jm_walk_picture(pics.data(), np, p, streams.data(), n_streams, lanes, a.es_bytes, w);
	JmParseSizing ps;
	memset(&ps, 0, sizeof ps);
	jm_parse_sizing_from_walk(w, lanes, a.es_bytes, a.mb_size, ps, nullptr);
	ps.debug_flags = 0;
	CHECK(plan.overflow == (overflow ? 1u : 0u) && plan.n_pics == np, "overflow / pictures");
	CHECK(plan.parse.n_lanes == lanes && plan.parse.long_slices == ps.long_slices && plan.parse.bytes_per_mb_x16 == ps.bytes_per_mb_x16,
	      "walk: lanes %u/%u long %u/%u bpm %u/%u", plan.parse.n_lanes, lanes, plan.parse.long_slices, ps.long_slices, plan.parse.bytes_per_mb_x16, ps.bytes_per_mb_x16);
	if (lanes) {
		bool tk = false;
		jm_plan_parse_rules(ps, a.ov, true, &tk);
		CHECK(plan.parse.lanes_per_wave == ps.lanes_per_wave && plan.parse.t_cold == ps.t_cold && plan.parse.split_service == ps.split_service &&
		      plan.parse.prio_batches == ps.prio_batches && plan.parse.n_batches == ps.n_batches && plan.parse.cold_threshold == ps.cold_threshold &&
		      plan.parse.head_batches[0] == ps.head_batches[0] && plan.parse.head_batches[1] == ps.head_batches[1] &&
		      plan.parse.head_lanes[0] == ps.head_lanes[0] && plan.parse.head_lanes[1] == ps.head_lanes[1] &&
		      plan.parse.head_first[1] == ps.head_first[1] && plan.parse.head_first[2] == ps.head_first[2], "parse rules differ");
	} else CHECK(plan.parse.n_batches == 0, "an empty / overflowed pass parses nothing");

	/* which plan the host path's functions give (jm_choose_recon's ordered kinds), and its sequence */
	uint32_t host_kind = JM_PLAN_HOST;
	JmOrderedPlan hp;
	hp.rows = 0; hp.lockstep = 0;
	std::vector<uint32_t> chain_of;
	const uint32_t tiles = a.tiles_per_picture;
	const auto fits = [&](bool forced) { return hp.rows <= rows_cap && (forced || (hp.lockstep - 1) * tiles >= JM_ORDER_MIN_DISTANCE); };
	bool capped = false;    /* the device's own limits (enqueue_plan.h): more units or a wider lockstep than it deals */
	if (!overflow && a.try_streams && jm_plan_ordered(pics.data(), np, n_streams, a.group, 8, hp) && fits(a.streams_forced)) {
		host_kind = JM_PLAN_STREAMS;
		capped = n_streams > JM_PLAN_SORT_CAP;
	}
	std::vector<JmPic> by_chain;
	const uint32_t n_chains = jm_plan_chains(pics.data(), np, n_streams, chain_of, &by_chain);
	if (!overflow && host_kind == JM_PLAN_HOST && a.try_chains && n_chains >= 8 &&
	    jm_plan_ordered(by_chain.data(), np, n_chains, a.group, 8, hp) && fits(a.chains_forced)) {
		host_kind = JM_PLAN_CHAINS;
		capped = n_chains > JM_PLAN_SORT_CAP;
	}
	for (uint32_t c = 0; c < 8; c++) capped = capped || sh->width[c] > JM_PLAN_MAXW;
	out[0] = plan.kind; out[1] = plan.rows; out[2] = plan.lockstep; out[3] = plan.parse.n_lanes; out[4] = plan.parse.long_slices;
	out[5] = plan.parse.bytes_per_mb_x16; out[6] = plan.parse.split_service; out[7] = plan.parse.lanes_per_wave; out[8] = plan.parse.n_batches;
	out[9] = plan.parse.t_cold; out[10] = plan.parse.head_lanes[0]; out[11] = plan.parse.head_batches[0] + plan.parse.head_batches[1];
	out[12] = plan.parse.head_first[2]; out[13] = plan.parse.prio_batches; out[14] = plan.n_chains; out[15] = host_kind;
	if (plan.kind != host_kind) {
		CHECK(plan.kind == JM_PLAN_HOST && capped, "plan kind %u, the host's functions %u", plan.kind, host_kind);
		return 0;
	}
	if (plan.kind == JM_PLAN_HOST) {
		for (uint32_t k = 0; k < 8 * rows_cap; k++) CHECK(jm_plan_slot(a, *sh, k) == JM_NONE, "a deferred plan has a picture in slot %u", k);
		return 0;
	}
	CHECK(plan.rows == hp.rows && plan.lockstep == hp.lockstep, "rows %u/%u lockstep %u/%u", plan.rows, hp.rows, plan.lockstep, hp.lockstep);
	/* seq = jm_plan_ordered's; every decoded picture once; padding behind */
	std::vector<uint32_t> seen(np, 0);
	for (uint32_t k = 0; k < 8 * rows_cap; k++) {
		const uint32_t r = jm_plan_slot(a, *sh, k);
		const int32_t want = k < hp.seq.size() ? hp.seq[k] : -1;
		const int32_t got = r == JM_NONE ? -1 : (int32_t)dec[r];
		CHECK(got == want, "slot %u: picture %d, jm_plan_ordered %d", k, got, want);
		if (got < 0) continue;
		seen[got]++;
		uint32_t done_pic, wf, ws;
		jm_plan_slot_waits(pics.data(), dec.data(), stale.data(), chain_id.data(), plan.kind, r, (int32_t)k == a.brk, done_pic, wf, ws);
		CHECK(done_pic == ((int32_t)k == a.brk ? JM_NONE : (uint32_t)got), "slot %u: done_pic", k);
		CHECK(wf == (pics[got].fwd >= 0 ? (uint32_t)pics[got].fwd : JM_NONE), "slot %u: wait_fwd", k);
		uint32_t ws_want = stale[got] >= 0 ? (uint32_t)stale[got] : JM_NONE;
		if (plan.kind == JM_PLAN_CHAINS && stale[got] >= 0 && chain_of[stale[got]] != chain_of[got]) ws_want = JM_NONE;
		CHECK(ws == ws_want, "slot %u: wait_stale %u, want %u", k, ws, ws_want);
		/* what a slot waits for lies earlier in its class */
		for (uint32_t wait : { wf, ws }) {
			if (wait == JM_NONE) continue;
			bool earlier = false;
			for (uint32_t j = k % 8; j < k && !earlier; j += 8) { const uint32_t rj = jm_plan_slot(a, *sh, j); earlier = rj != JM_NONE && dec[rj] == wait; }
			CHECK(earlier, "slot %u (picture %d) waits for picture %u, which is not earlier in its class", k, got, wait);
		}
	}
	for (uint32_t p = 0; p < np; p++) CHECK(seen[p] == (jm_plan_in_unit(pics[p], n_streams) ? 1u : 0u), "picture %u appears %u times", p, seen[p]);
	return 0;
}
