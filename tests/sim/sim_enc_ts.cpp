/*
 * TEST INFRASTRUCTURE ONLY -- the CPU simulator of the TS mux on the device (jsmpeg_amd/csrc/enc_ts.h): k_ts_plan's walk and
 * k_ts_write's dwords from the same functions the kernels compile, under g++.  The writer visits the output dwords in
 * REVERSE order: nothing about a dword may depend on the ones before it.  sim_ts_mux_serial is the yardstick, the byte loop
 * jsmpeg_hip_ts_mux_host was before it was rewritten on enc_ts.h, one stream at a time.
 * With -DSIM_TS_MAIN: a stand-alone driver (for -fsanitize=address,undefined) that holds the simulator to the yardstick over
 * edge sizes, every payload size 1 .. 400 and random cases, the units back to back in a buffer of exactly their size.
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "enc_ts.h"

/* the legacy byte loop: one stream, one counter; returns the bytes written */
static uint64_t serial_mux(const uint8_t *es, const uint64_t *offset, const uint32_t *bytes, const uint64_t *pts_90k, uint32_t n_units,
                           uint32_t stream_id, uint32_t pid, uint32_t *continuity, uint8_t *ts) {
	uint8_t cc = (uint8_t)(*continuity & 15u);
	uint64_t at = 0;
	for (uint32_t u = 0; u < n_units; u++) {
		const uint64_t total = 14 + (uint64_t)bytes[u];
		const bool sized = (uint64_t)bytes[u] + 8 <= 0xffff;
		const uint64_t lead = (!sized && total % 184 == 0) ? 1 : 0;
		const uint64_t packets = (total + lead + 183) / 184;
		uint8_t head[14];
		const uint32_t plen = sized ? bytes[u] + 8 : 0;
		const uint64_t p = pts_90k[u] & 0x1ffffffffull;
		head[0] = 0; head[1] = 0; head[2] = 1; head[3] = (uint8_t)stream_id;
		head[4] = (uint8_t)(plen >> 8); head[5] = (uint8_t)plen;
		head[6] = 0x80; head[7] = 0x80; head[8] = 5;
		head[9] = (uint8_t)(0x21 | ((p >> 29) & 0x0e));
		head[10] = (uint8_t)(p >> 22); head[11] = (uint8_t)(0x01 | ((p >> 14) & 0xfe));
		head[12] = (uint8_t)(p >> 7); head[13] = (uint8_t)(0x01 | ((p << 1) & 0xfe));
		uint64_t done = 0;
		for (uint64_t k = 0; k < packets; k++) {
			uint8_t *pk = ts + at;
			const uint64_t left = total - done;
			uint64_t stuff = k == 0 ? lead : 0;
			if (left + stuff < 184) stuff = 184 - left;
			const uint64_t n = 184 - stuff;
			pk[0] = 0x47;
			pk[1] = (uint8_t)((k == 0 ? 0x40 : 0) | (pid >> 8));
			pk[2] = (uint8_t)pid;
			pk[3] = (uint8_t)((stuff ? 0x30 : 0x10) | cc);
			cc = (cc + 1) & 15u;
			uint8_t *w = pk + 4;
			if (stuff) {
				*w++ = (uint8_t)(stuff - 1);
				if (stuff > 1) { *w++ = 0; memset(w, 0xff, stuff - 2); w += stuff - 2; }
			}
			for (uint64_t i = 0; i < n; i++, done++) w[i] = done < 14 ? head[done] : es[offset[u] + done - 14];
			at += 188;
		}
	}
	*continuity = cc;
	return at;
}

/* k_ts_plan + k_ts_write.  cc: [n_streams] in / out (written back unless the call overflowed); ts: cap bytes are
 * writable; aligned: fetch the source as the kernel does, from aligned dwords (the dwords around every unit's ends
 * are then read: the caller pads), else byte by byte.  Returns the total, or -1 on overflow. */
static int64_t sim_mux(const uint8_t *es, const JmTsUnit *units, uint32_t n, uint32_t stream_id, uint32_t pid, uint32_t *cc, uint32_t n_streams,
                       uint8_t *ts, uint64_t cap, uint64_t *sb, uint64_t *se, JmTsPlaced *placed, int aligned) {
	std::vector<uint32_t> cn(n_streams, 0u);
	std::vector<JmTsPlaced> own(n ? n : 1);
	if (!placed) placed = own.data();
	uint64_t result[3];
	for (uint32_t i = 0; i < n_streams; i++) { sb[i] = 0; se[i] = 0; }
	JmTsPlan p = jm_ts_plan_begin();
	for (uint32_t i = 0; i < n; i++) placed[i] = jm_ts_plan_unit(p, units[i].stream, units[i].bytes, cc, sb, se, cn.data());
	jm_ts_plan_close(p, cap, se, cn.data(), result);
	if (result[1]) return -1;
	for (uint32_t i = 0; i < n_streams; i++) jm_ts_plan_commit(i, sb, se, cn.data(), cc);
	for (uint64_t g = result[2] * JM_TS_DWORDS; g-- > 0;) {
		uint64_t where;
		const uint32_t v = aligned ? jm_ts_output_dword<JmTsFetchAligned>(units, placed, n, g, stream_id, pid, es, &where)
		                           : jm_ts_output_dword<JmTsFetchBytes>(units, placed, n, g, stream_id, pid, es, &where);
		memcpy(ts + 4 * where, &v, 4);
	}
	return (int64_t)result[0];
}

extern "C" {

int64_t sim_ts_mux(const uint8_t *es, const uint64_t *offset, const uint32_t *bytes, const uint32_t *stream, const uint64_t *pts_90k, uint32_t n,
                   uint32_t stream_id, uint32_t pid, uint32_t *cc, uint32_t n_streams, uint8_t *ts, uint64_t cap, uint64_t *sb, uint64_t *se,
                   uint64_t *unit_at, uint32_t *unit_packets, uint32_t *unit_cc, int aligned) {
	std::vector<JmTsUnit> units(n);
	std::vector<JmTsPlaced> placed(n ? n : 1);
	for (uint32_t i = 0; i < n; i++) { units[i].off = offset[i]; units[i].bytes = bytes[i]; units[i].stream = stream ? stream[i] : 0; units[i].pts = pts_90k[i]; }
	const int64_t total = sim_mux(es, units.data(), n, stream_id, pid, cc, n_streams, ts, cap, sb, se, placed.data(), aligned);
	for (uint32_t i = 0; i < n && total >= 0; i++) {
		if (unit_at) unit_at[i] = placed[i].at;
		if (unit_packets) unit_packets[i] = placed[i].packets;
		if (unit_cc) unit_cc[i] = placed[i].cc;
	}
	return total;
}

int64_t sim_ts_mux_serial(const uint8_t *es, const uint64_t *offset, const uint32_t *bytes, const uint64_t *pts_90k, uint32_t n,
                          uint32_t stream_id, uint32_t pid, uint32_t *continuity, uint8_t *ts) {
	return (int64_t)serial_mux(es, offset, bytes, pts_90k, n, stream_id, pid, continuity, ts);
}

uint32_t sim_ts_packets(uint32_t bytes) { return jm_ts_packets(bytes); }
uint64_t sim_ts_bound(uint64_t es_bytes, uint32_t units, uint32_t streams) { return jm_ts_bound(es_bytes, units, streams); }
uint64_t sim_ts_default_pts(uint32_t ordinal, uint32_t frame_rate_code) { return jm_ts_default_pts(ordinal, frame_rate_code); }

}

#ifdef SIM_TS_MAIN
static uint32_t rnd_state = 12345u;
static uint32_t rnd() { rnd_state = rnd_state * 1664525u + 1013904223u; return rnd_state >> 8; }

/* units of `sizes` over `streams` (ascending, contiguous), back to back in a buffer of exactly their size: the simulator with
 * the byte fetch and -- when that size is a multiple of 4, so that every dword that holds a unit's byte lies inside -- with the
 * aligned fetch, against the yardstick per stream */
static int check(const std::vector<uint32_t> &sizes, const std::vector<uint32_t> &streams, uint32_t n_streams, const char *what) {
	const uint32_t n = (uint32_t)sizes.size();
	uint64_t sum = 0;
	for (uint32_t b : sizes) sum += b;
	uint8_t *es = (uint8_t *)malloc(sum ? sum : 1);
	for (uint64_t i = 0; i < sum; i++) es[i] = (uint8_t)rnd();
	std::vector<JmTsUnit> units(n);
	std::vector<uint64_t> off(n), pts(n);
	uint64_t at = 0;
	for (uint32_t i = 0; i < n; i++) {
		off[i] = at; pts[i] = ((uint64_t)rnd() << 16) ^ rnd();
		units[i].off = at; units[i].bytes = sizes[i]; units[i].stream = streams[i]; units[i].pts = pts[i];
		at += sizes[i];
	}
	std::vector<uint32_t> cc0(n_streams), cc(n_streams);
	for (uint32_t &c : cc0) c = rnd() & 15u;
	const uint64_t cap = jm_ts_bound(sum, n, n_streams);
	std::vector<uint64_t> sb(n_streams), se(n_streams);
	int bad = 0;
	for (int aligned = 0; aligned < ((sum & 3u) ? 1 : 2); aligned++) {
		uint8_t *ts = (uint8_t *)malloc(cap ? cap : 1);
		cc = cc0;
		const int64_t total = sim_mux(es, units.data(), n, 0xE0, 0x100, cc.data(), n_streams, ts, cap, sb.data(), se.data(), nullptr, aligned);
		if (total < 0 || (uint64_t)total > cap) { printf("%s: total %lld above the bound %llu\n", what, (long long)total, (unsigned long long)cap); bad = 1; }
		for (uint32_t i = 0; i < n && !bad;) {
			uint32_t j = i;
			while (j < n && streams[j] == streams[i]) j++;
			const uint32_t s = streams[i];
			uint64_t need = 0;
			for (uint32_t k = i; k < j; k++) need += (uint64_t)jm_ts_packets(sizes[k]) * 188;
			uint8_t *want = (uint8_t *)malloc(need);
			uint32_t c = cc0[s];
			const uint64_t got = serial_mux(es, &off[i], &sizes[i], &pts[i], j - i, 0xE0, 0x100, &c, want);
			if (got != need || se[s] - sb[s] != need || (sb[s] & 15u) || c != cc[s] || memcmp(want, ts + sb[s], need) != 0) {
				printf("%s: stream %u differs (aligned %d)\n", what, s, aligned); bad = 1;
			}
			free(want);
			i = j;
		}
		/* one byte short: refused, the counters stay */
		if (!bad && total > 0) {
			cc = cc0;
			if (sim_mux(es, units.data(), n, 0xE0, 0x100, cc.data(), n_streams, ts, (uint64_t)total - 1, sb.data(), se.data(), nullptr, aligned) >= 0 || cc != cc0) {
				printf("%s: a capacity one byte short was not refused\n", what); bad = 1;
			}
		}
		free(ts);
	}
	free(es);
	return bad;
}

int main() {
	int bad = 0, cases = 0;
	const std::vector<uint32_t> edge = { 170, 174, 1, 184 * 3 - 14, 1000, 65527, 65528, 184 * 400 - 14, 184 * 400 - 13, 100000 };
	bad |= check(edge, std::vector<uint32_t>(edge.size(), 0u), 1, "edge sizes"); cases++;
	std::vector<uint32_t> sweep;
	for (uint32_t b = 1; b <= 400; b++) sweep.push_back(b);
	bad |= check(sweep, std::vector<uint32_t>(sweep.size(), 0u), 1, "1 .. 400"); cases++;
	for (uint32_t one = 1; one <= 400 && !bad; one++) { bad |= check({ one }, { 0u }, 1, "one unit"); cases++; }
	for (int r = 0; r < 100 && !bad; r++) {
		const uint32_t ns = 1 + rnd() % 5u, n_streams = 12;
		std::vector<uint32_t> sizes, streams;
		uint32_t s = rnd() % 3u;
		for (uint32_t i = 0; i < ns; i++, s += 1 + rnd() % 2u)
			for (uint32_t k = 0, m = 1 + rnd() % 4u; k < m; k++) {
				sizes.push_back(rnd() % 16u == 0 ? 65520u + rnd() % 8000u : 1u + rnd() % 3000u);
				streams.push_back(s);
			}
		bad |= check(sizes, streams, n_streams, "random"); cases++;
	}
	if (bad) return 1;
	printf("%d cases equal the serial mux\n", cases);
	return 0;
}
#endif
