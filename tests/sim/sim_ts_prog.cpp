/*
 * TEST INFRASTRUCTURE ONLY -- the CPU simulator of the TS program mux on the device (jsmpeg_amd/csrc/ts_prog.h): k_tsp_plan as
 * the kernel states it -- the rank of every unit by binary search, the per-lane steps around plain prefix sums where the kernel
 * scans across a workgroup -- and k_tsp_write's dwords, each on its own and in REVERSE order, from the same functions the
 * kernels compile, under g++.  The units are placed in reverse order too: no step may depend on the lanes before it.
 * With -DSIM_TSP_MAIN: a stand-alone driver (for -fsanitize=address,undefined).  It holds the generalised geometry to enc_ts.h's
 * at lead0 == 0, and takes the simulator's programs apart again with a demuxer of its own (sync, PIDs, counters per PID, PES
 * lengths, PCR, payload bytes, PSI position) over every payload size 1 .. 400 as PCR units, the one-packet and unsized edges
 * and random two-table cases, the source buffers exactly the units' size.
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "ts_prog.h"

struct SimTables {
	const uint8_t *src[2];
	std::vector<JmTsUnit> t[2];
};

/* k_tsp_plan + k_tsp_write.  state: [n_streams][5] in / out (replaced unless the call overflowed); ts: cap bytes are writable.
 * Returns the total, or -1 on overflow. */
static int64_t sim_program(const JmTspRule &r, const SimTables &T, uint32_t *state, uint32_t n_streams, uint8_t *ts, uint64_t cap,
                           uint64_t *sb, uint64_t *se, std::vector<JmTspPlaced> &placed, std::vector<uint32_t> &rank, int aligned) {
	const uint32_t n_v = (uint32_t)T.t[0].size(), n_a = (uint32_t)T.t[1].size(), n = n_v + n_a;
	const JmTsUnit *v = T.t[0].data(), *a = T.t[1].data();
	placed.assign(n ? n : 1, JmTspPlaced());
	rank.assign(n ? n : 1, 0u);
	std::vector<JmTspEdges> edges(n_streams);
	memset(edges.data(), 0, sizeof(JmTspEdges) * n_streams);
	std::vector<uint32_t> staged(JM_TSP_STATE * (size_t)n_streams), work(5 * (size_t)(n ? n : 1));
	for (uint32_t i = n; i-- > 0;) {
		const uint32_t kind = i >= n_v ? 1u : 0u;
		if (aligned) jm_tsp_step_place<JmTsFetchAligned>(r, v, n_v, a, n_a, kind, kind ? i - n_v : i, T.src[0], placed.data(), rank.data());
		else jm_tsp_step_place<JmTsFetchBytes>(r, v, n_v, a, n_a, kind, kind ? i - n_v : i, T.src[0], placed.data(), rank.data());
	}
	uint32_t carry[4] = { 0, 0, 0, 0 };
	for (uint32_t m = 0; m < n; m++) {                             /* scan 1 */
		uint32_t c[4];
		work[4 * (size_t)n + m] = jm_tsp_step_count(r, placed.data(), m, state, c);
		for (int i = 0; i < 4; i++) { work[(size_t)i * n + m] = carry[i]; carry[i] += c[i]; }
	}
	for (uint32_t m = n; m-- > 0;) {
		uint32_t c[4], e[4];
		jm_tsp_step_count(r, placed.data(), m, state, c);
		for (int i = 0; i < 4; i++) e[i] = work[(size_t)i * n + m];
		jm_tsp_step_edges(placed.data(), m, n, e, c, edges.data());
	}
	std::vector<uint64_t> begin(n_streams);
	uint64_t at = 0, total = 0;
	for (uint32_t s = 0; s < n_streams; s++) { begin[s] = at; at += jm_tsp_stream_size(edges.data(), s); }     /* scan 2 */
	for (uint32_t s = n_streams; s-- > 0;) {
		const uint64_t end = jm_tsp_step_stream(s, begin[s], edges.data(), state, sb, se, staged.data());
		if (end > total) total = end;
	}
	for (uint32_t m = n; m-- > 0;) {
		uint32_t e[4];
		for (int i = 0; i < 4; i++) e[i] = work[(size_t)i * n + m];
		jm_tsp_step_final(placed.data(), m, work[4 * (size_t)n + m], e, edges.data(), state, sb);
	}
	if (total > cap) return -1;
	for (uint32_t s = 0; s < n_streams; s++) jm_tsp_commit(s, staged.data(), state);
	uint8_t psi[2 * JM_TS_PACKET];
	uint32_t tpl[2 * JM_TS_DWORDS];
	jm_tsp_psi_packets(r, 1, 1, psi);
	memcpy(tpl, psi, sizeof(tpl));
	for (uint64_t g = (uint64_t)carry[3] * JM_TS_DWORDS; g-- > 0;) {
		uint64_t where;
		const uint32_t d = aligned ? jm_tsp_output_dword<JmTsFetchAligned>(r, v, a, placed.data(), n, g, tpl, T.src[0], T.src[1], &where)
		                           : jm_tsp_output_dword<JmTsFetchBytes>(r, v, a, placed.data(), n, g, tpl, T.src[0], T.src[1], &where);
		memcpy(ts + 4 * where, &d, 4);
	}
	return (int64_t)total;
}

extern "C" {

/* cfg: video_pid, audio_pid, pmt_pid, video_stream_id, audio_stream_id, flags, program_number, transport_stream_id; the PSI
 * packets of the simulator carry program_number / transport_stream_id 1 unless cfg says otherwise (sim_tsp_mux patches them) */
int64_t sim_tsp_mux(const uint32_t *cfg, uint64_t pcr_lead,
                    const uint8_t *video, const uint64_t *v_off, const uint32_t *v_bytes, const uint32_t *v_stream, const uint64_t *v_pts, uint32_t n_v,
                    const uint8_t *audio, const uint64_t *a_off, const uint32_t *a_bytes, const uint32_t *a_stream, const uint64_t *a_pts, uint32_t n_a,
                    uint32_t *state, uint32_t n_streams, uint8_t *ts, uint64_t cap, uint64_t *sb, uint64_t *se,
                    uint64_t *unit_at, uint32_t *unit_bytes, uint32_t *unit_psi, uint32_t *unit_cc, int aligned) {
	JmTspRule r;
	r.pid[0] = cfg[0]; r.pid[1] = cfg[1]; r.pmt_pid = cfg[2]; r.sid[0] = cfg[3]; r.sid[1] = cfg[4]; r.flags = cfg[5]; r.pcr_lead = pcr_lead;
	SimTables T;
	T.src[0] = video; T.src[1] = audio;
	T.t[0].resize(n_v); T.t[1].resize(n_a);
	for (uint32_t i = 0; i < n_v; i++) { T.t[0][i].off = v_off[i]; T.t[0][i].bytes = v_bytes[i]; T.t[0][i].stream = v_stream ? v_stream[i] : 0; T.t[0][i].pts = v_pts[i]; }
	for (uint32_t i = 0; i < n_a; i++) { T.t[1][i].off = a_off[i]; T.t[1][i].bytes = a_bytes[i]; T.t[1][i].stream = a_stream ? a_stream[i] : 0; T.t[1][i].pts = a_pts[i]; }
	std::vector<JmTspPlaced> placed;
	std::vector<uint32_t> rank;
	const int64_t total = sim_program(r, T, state, n_streams, ts, cap, sb, se, placed, rank, aligned);
	if (total < 0) return total;
	if (cfg[6] != 1 || cfg[7] != 1) {                              /* the PSI packets of another program: the templates differ, not the plan */
		uint8_t psi[2 * JM_TS_PACKET];
		jm_tsp_psi_packets(r, cfg[6], cfg[7], psi);
		for (const JmTspPlaced &p : placed)
			if ((p.cc & JM_TSP_P_PSI) && n_v + n_a)
				for (uint32_t k = 0; k < 2; k++) {
					uint8_t *q = ts + p.at + 188 * k;
					const uint8_t cc = q[3] & 15u;
					memcpy(q, psi + 188 * k, 188);
					q[3] |= cc;
				}
	}
	for (uint32_t i = 0; i < n_v + n_a; i++) {
		const JmTspPlaced &p = placed[rank[i]];
		const uint32_t psi = (p.cc & JM_TSP_P_PSI) ? 2u : 0u;
		if (unit_at) unit_at[i] = p.at;
		if (unit_bytes) unit_bytes[i] = (p.packets + psi) * JM_TS_PACKET;
		if (unit_psi) unit_psi[i] = psi * JM_TS_PACKET;
		if (unit_cc) unit_cc[i] = p.cc & 0xfffu;
	}
	return total;
}

uint32_t sim_tsp_packets(uint32_t bytes, uint32_t lead0) { return jm_tsp_packets(bytes, lead0); }
uint64_t sim_tsp_bound(uint64_t v_bytes, uint32_t n_v, uint64_t a_bytes, uint32_t n_a, uint32_t streams) { return jm_tsp_bound(v_bytes, n_v, a_bytes, n_a, streams); }
uint32_t sim_tsp_rank(const uint32_t *v_stream, const uint64_t *v_pts, uint32_t n_v, const uint32_t *a_stream, const uint64_t *a_pts, uint32_t n_a, uint32_t kind, uint32_t i) {
	std::vector<JmTsUnit> v(n_v ? n_v : 1), a(n_a ? n_a : 1);
	for (uint32_t k = 0; k < n_v; k++) { v[k].stream = v_stream[k]; v[k].pts = v_pts[k]; }
	for (uint32_t k = 0; k < n_a; k++) { a[k].stream = a_stream[k]; a[k].pts = a_pts[k]; }
	return jm_tsp_rank(v.data(), n_v, a.data(), n_a, kind, i);
}

}

#ifdef SIM_TSP_MAIN
static uint32_t rnd_state = 4711u;
static uint32_t rnd() { rnd_state = rnd_state * 1664525u + 1013904223u; return rnd_state >> 8; }

/* with lead0 == 0 the generalised functions ARE enc_ts.h's */
static int check_reduction(uint32_t bytes) {
	std::vector<uint8_t> es(bytes);
	for (uint8_t &b : es) b = (uint8_t)rnd();
	JmTsUnit u;
	u.off = 0; u.bytes = bytes; u.stream = 0; u.pts = ((uint64_t)rnd() << 16) ^ rnd();
	if (jm_tsp_lead(bytes, 0) != jm_ts_lead(bytes) || jm_tsp_packets(bytes, 0) != jm_ts_packets(bytes)) return 1;
	JmTsFetchBytes f;
	f.base = es.data();
	for (uint32_t k = 0, n = jm_ts_packets(bytes); k < n; k++) {
		uint64_t d0, d1;
		uint32_t s0, s1;
		jm_ts_packet(bytes, k, &d0, &s0);
		jm_tsp_packet(bytes, 0, k, &d1, &s1);
		if (d0 != d1 || s0 != s1) return 1;
		for (uint32_t w = 0; w < JM_TS_DWORDS; w++)
			if (jm_ts_dword(u, 7, 0xE0, 0x100, k, w, f) != jm_tsp_dword(u, 7, 0xE0, 0x100, 0, 12345, k, w, f)) return 1;
	}
	return 0;
}

/* THE DRIVER'S OWN DEMUXER over stream s's range: every packet in order -- sync byte, a known PID, the PID's counter going on
 * from `state`, PAT + PMT only as a pair equal to the templates and only in front of a unit; a unit's packets back to back, an
 * adaptation field in its first and last packet only, the PCR where the rule puts it, the PES header and the payload bytes.
 * `order`: the stream's units as (kind, index) in the order they must appear. */
static int demux(const JmTspRule &r, const SimTables &T, const std::vector<std::pair<uint32_t, uint32_t>> &order, const uint8_t *ts, uint64_t b, uint64_t e,
                 const uint32_t *state_in, const uint32_t *state_out, std::vector<int> *psi_at) {
	uint8_t psi[2 * JM_TS_PACKET];
	jm_tsp_psi_packets(r, 1, 1, psi);
	uint32_t cc[4] = { state_in[0], state_in[1], state_in[2], state_in[3] };
	uint64_t at = b;
	if ((b & 15u) || (e - b) % 188u) return 1;
	for (size_t o = 0; o < order.size(); o++) {
		const uint32_t kind = order[o].first;
		const JmTsUnit &u = T.t[kind][order[o].second];
		int had_psi = 0;
		if (at + 188 <= e && (((ts[at + 1] & 0x1fu) << 8) | ts[at + 2]) == 0) {            /* a PAT: the pair */
			for (uint32_t k = 0; k < 2; k++, at += 188) {
				if (at + 188 > e || (ts[at + 3] & 15u) != cc[k] || (ts[at + 3] & 0xf0u) != 0x10) return 2;
				uint8_t want[188];
				memcpy(want, psi + 188 * k, 188);
				want[3] |= (uint8_t)cc[k];
				if (memcmp(want, ts + at, 188) != 0) return 3;
				cc[k] = (cc[k] + 1) & 15u;
			}
			had_psi = 1;
		}
		if (psi_at) psi_at->push_back(had_psi);
		const uint32_t lead0 = jm_tsp_lead0(r, kind);
		std::vector<uint8_t> pes;
		const uint64_t want_len = 14 + (uint64_t)u.bytes;
		for (uint32_t k = 0; pes.size() < want_len; k++, at += 188) {
			if (at + 188 > e) return 4;
			const uint8_t *p = ts + at;
			const uint32_t pid = ((p[1] & 0x1fu) << 8) | p[2];
			if (p[0] != 0x47 || pid != r.pid[kind] || ((p[1] & 0x40) != 0) != (k == 0) || (p[3] & 15u) != cc[2 + kind]) return 5;
			cc[2 + kind] = (cc[2 + kind] + 1) & 15u;
			uint32_t skip = 0;
			if (p[3] & 0x20) {
				skip = 1u + p[4];
				if (skip > 184) return 6;
				if (k == 0 && lead0) {
					const uint64_t base = (u.pts - r.pcr_lead) & 0x1ffffffffull;
					const uint64_t got = ((uint64_t)p[6] << 25) | ((uint64_t)p[7] << 17) | ((uint64_t)p[8] << 9) | ((uint64_t)p[9] << 1) | (p[10] >> 7);
					if (p[4] < 7 || p[5] != 0x10 || got != base || (p[10] & 0x7f) != 0x7e || p[11] != 0) return 7;
					for (uint32_t i = 8; i < skip; i++) if (p[4 + i] != 0xff) return 7;
				} else if (skip > 1) {
					if (p[5] != 0) return 8;
					for (uint32_t i = 2; i < skip; i++) if (p[4 + i] != 0xff) return 8;
				}
				if (k != 0 && pes.size() + (184 - skip) != want_len) return 9;                 /* a later field: the last packet only */
			} else if (k == 0 && lead0) return 7;
			if (!(p[3] & 0x10)) return 10;
			pes.insert(pes.end(), p + 4 + skip, p + 188);
		}
		if (pes.size() != want_len) return 11;
		const uint32_t plen = (uint64_t)u.bytes + 8 <= 0xffff ? u.bytes + 8 : 0;
		const uint64_t pts = (((uint64_t)pes[9] >> 1) & 7) << 30 | (uint64_t)pes[10] << 22 | ((uint64_t)pes[11] >> 1) << 15 | (uint64_t)pes[12] << 7 | pes[13] >> 1;
		if (pes[0] || pes[1] || pes[2] != 1 || pes[3] != r.sid[kind] || (uint32_t)(pes[4] << 8 | pes[5]) != plen || pts != (u.pts & 0x1ffffffffull)) return 12;
		if (u.bytes && memcmp(pes.data() + 14, T.src[kind] + u.off, u.bytes) != 0) return 13;
	}
	if (at != e) return 14;
	for (int i = 0; i < 4; i++) if (cc[i] != state_out[i]) return 15;
	return 0;
}

struct DriverCase { std::vector<uint32_t> bytes[2], stream[2]; std::vector<uint64_t> pts[2]; };

/* the tables over source buffers of exactly the units' size; the byte fetch, and -- when both sizes are multiples of 4 -- the
 * aligned fetch; every stream demuxed in the merged order a stable sort by (pts, kind) gives */
static int check(const DriverCase &c, uint32_t n_streams, uint32_t flags, bool audio_only, const char *what) {
	JmTspRule r;
	r.pid[0] = audio_only ? JM_TSP_NO_PID : 0x100; r.pid[1] = 0x101; r.sid[0] = 0xE0; r.sid[1] = 0xC0; r.pmt_pid = 0x1000; r.flags = flags; r.pcr_lead = 9000;
	SimTables T;
	uint8_t *src[2];
	uint64_t sum[2] = { 0, 0 };
	for (int kind = 0; kind < 2; kind++) {
		for (uint32_t b : c.bytes[kind]) sum[kind] += b;
		src[kind] = (uint8_t *)malloc(sum[kind] ? sum[kind] : 1);
		for (uint64_t i = 0; i < sum[kind]; i++) src[kind][i] = (uint8_t)rnd();
		T.src[kind] = src[kind];
		uint64_t at = 0;
		for (size_t i = 0; i < c.bytes[kind].size(); i++) {
			JmTsUnit u;
			u.off = at; u.bytes = c.bytes[kind][i]; u.stream = c.stream[kind][i]; u.pts = c.pts[kind][i];
			if (kind == 0 && u.bytes >= 4 && rnd() % 3u == 0) { src[0][at] = 0; src[0][at + 1] = 0; src[0][at + 2] = 1; src[0][at + 3] = 0xb3; }
			T.t[kind].push_back(u);
			at += u.bytes;
		}
	}
	const uint32_t n_v = (uint32_t)T.t[0].size(), n_a = (uint32_t)T.t[1].size();
	std::vector<uint32_t> st0(JM_TSP_STATE * (size_t)n_streams), st;
	for (size_t i = 0; i < st0.size(); i++) st0[i] = i % JM_TSP_STATE == 4 ? rnd() & 1u : rnd() & 15u;
	const uint64_t cap = jm_tsp_bound(sum[0], n_v, sum[1], n_a, n_streams);
	std::vector<uint64_t> sb(n_streams), se(n_streams);
	std::vector<JmTspPlaced> placed;
	std::vector<uint32_t> rank;
	int bad = 0;
	for (int aligned = 0; aligned < (((sum[0] | sum[1]) & 3u) ? 1 : 2) && !bad; aligned++) {
		uint8_t *ts = (uint8_t *)malloc(cap ? cap : 1);
		st = st0;
		const int64_t total = sim_program(r, T, st.data(), n_streams, ts, cap, sb.data(), se.data(), placed, rank, aligned);
		if (total < 0) { printf("%s: the bound %llu does not hold\n", what, (unsigned long long)cap); bad = 1; }
		for (uint32_t s = 0; s < n_streams && !bad; s++) {
			std::vector<std::pair<uint32_t, uint32_t>> order;
			uint32_t iv = 0, ia = 0;
			while (true) {                                              /* the merge as a walk: what the ranks must equal */
				while (iv < n_v && T.t[0][iv].stream != s) iv++;
				while (ia < n_a && T.t[1][ia].stream != s) ia++;
				if (iv >= n_v && ia >= n_a) break;
				if (iv < n_v && (ia >= n_a || T.t[0][iv].pts <= T.t[1][ia].pts)) order.push_back({ 0u, iv++ }); else order.push_back({ 1u, ia++ });
			}
			if (order.empty()) {
				if (sb[s] || se[s] || memcmp(&st[JM_TSP_STATE * s], &st0[JM_TSP_STATE * s], 4 * JM_TSP_STATE) != 0) { printf("%s: absent stream %u changed\n", what, s); bad = 1; }
				continue;
			}
			std::vector<int> psi_at;
			const int why = demux(r, T, order, ts, sb[s], se[s], &st0[JM_TSP_STATE * s], &st[JM_TSP_STATE * s], &psi_at);
			if (why) { printf("%s: stream %u does not demux (%d, aligned %d)\n", what, s, why, aligned); bad = 1; break; }
			for (size_t o = 0; o < order.size(); o++) {
				const JmTsUnit &u = T.t[order[o].first][order[o].second];
				const uint8_t *q = T.src[0] + u.off;
				const bool key = order[o].first == 0 && u.bytes >= 4 && q[0] == 0 && q[1] == 0 && q[2] == 1 && q[3] == 0xb3;
				const int want = (flags & JM_TSP_PSI) && ((o == 0 && !st0[JM_TSP_STATE * s + 4]) || key) ? 1 : 0;
				if (psi_at[o] != want) { printf("%s: stream %u unit %u: PSI %d, expected %d\n", what, s, (unsigned)o, psi_at[o], want); bad = 1; }
			}
			if (st[JM_TSP_STATE * s + 4] != 1) { printf("%s: stream %u not started\n", what, s); bad = 1; }
		}
		if (!bad && total > 0) {                                        /* one byte short: refused, the state stays */
			st = st0;
			if (sim_program(r, T, st.data(), n_streams, ts, (uint64_t)total - 1, sb.data(), se.data(), placed, rank, aligned) >= 0 || st != st0) {
				printf("%s: a capacity one byte short was not refused\n", what); bad = 1;
			}
		}
		free(ts);
	}
	free(src[0]); free(src[1]);
	return bad;
}

int main() {
	int bad = 0, cases = 0;
	const uint32_t edge[] = { 1, 161, 162, 163, 170, 174, 184 * 3 - 14, 184 * 3 - 22, 65527, 65528, 184 * 400 - 14, 184 * 400 - 22, 184 * 400 - 13, 100000 };
	for (uint32_t b = 1; b <= 400 && !bad; b++) { bad |= check_reduction(b); cases++; }
	for (uint32_t b : edge) { bad |= check_reduction(b); cases++; }
	if (bad) { printf("the reduction to enc_ts.h fails\n"); return 1; }
	DriverCase sweep;
	for (uint32_t b = 1; b <= 400; b++) { sweep.bytes[0].push_back(b); sweep.stream[0].push_back(0); sweep.pts[0].push_back(3000ull * b); }
	bad |= check(sweep, 1, JM_TSP_PCR | JM_TSP_PSI, false, "1 .. 400 with PCR"); cases++;
	for (uint32_t one = 1; one <= 400 && !bad; one++) {
		DriverCase c;
		c.bytes[0] = { one }; c.stream[0] = { 0 }; c.pts[0] = { 100 };          /* pts < pcr_lead: the PCR wraps */
		bad |= check(c, 1, JM_TSP_PCR, false, "one PCR unit"); cases++;
	}
	for (uint32_t b : edge) {
		if (bad) break;
		DriverCase c;
		c.bytes[0] = { b, b }; c.stream[0] = { 0, 0 }; c.pts[0] = { 5, 5 };
		c.bytes[1] = { b }; c.stream[1] = { 0 }; c.pts[1] = { 5 };
		bad |= check(c, 2, JM_TSP_PCR | JM_TSP_PSI, false, "edge sizes"); cases++;
		bad |= check(c, 2, 0, false, "edge sizes, plain"); cases++;
	}
	for (int k = 0; k < 150 && !bad; k++) {
		const uint32_t n_streams = 8, flags = rnd() & 3u;
		const bool audio_only = rnd() % 5u == 0;
		DriverCase c;
		for (uint32_t s = rnd() % 3u; s < n_streams; s += 1 + rnd() % 3u)
			for (int kind = audio_only ? 1 : 0; kind < 2; kind++) {
				uint64_t pts = rnd() % 100u;
				for (uint32_t i = 0, m = rnd() % 5u; i < m; i++) {
					c.bytes[kind].push_back(rnd() % 16u == 0 ? 65520u + rnd() % 8000u : 1u + rnd() % 2000u);
					c.stream[kind].push_back(s);
					c.pts[kind].push_back(pts);
					pts += (rnd() % 3u) * 1500u;                        /* ties inside a list and across the two */
				}
			}
		bad |= check(c, n_streams, flags, audio_only, "random"); cases++;
	}
	if (bad) return 1;
	printf("%d cases hold\n", cases);
	return 0;
}
#endif
