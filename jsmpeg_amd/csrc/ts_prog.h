/*
 * TS PROGRAM MUX (include/jsmpeg_hip.h part 10): ONE transport stream per stream number with video and audio interleaved in it
 * and, on request, PAT / PMT in front of entry points and a PCR on the carrier's PES -- which unit goes where, what its packets
 * hold and which counters they carry, stated once, host + device: what the kernels of ts_program.hip (k_tsp_plan, k_tsp_write)
 * and the CPU simulator (tests/sim/sim_ts_prog.cpp) share.  Built ON enc_ts.h (the PES header, JmTsUnit, the fetchers,
 * jm_ts_align16), which it leaves as it is; jsmpeg_hip_ts_program_mux_host (ts_program.hip) is a serial walk of its own that
 * must write the same bytes.
 *
 * INPUTS OF A CALL.  Two unit tables: video units over one source buffer (PID rule.pid[0], stream id rule.sid[0], 0xE0 by
 *    default), audio units over another (pid[1], sid[1], 0xC0).  In each a stream's units are contiguous and the streams ascend;
 *    the PTS are 64-bit 90 kHz values, unwrapped (their low 33 bits go out), non-decreasing within a stream and a table -- the
 *    host, which always supplies them, refuses anything else.  A kind whose PID is 0x1fff is ABSENT: it has no units and the
 *    PMT does not list it.
 * ORDER.  Per stream number the two lists are merged by PTS, video first at equal PTS; a unit is atomic (its packets lie back
 *    to back).  NO WALK: both tables are sorted by (stream, pts), so over the whole call
 *      rank(video i) = i + #(audio units with (stream, pts) <  its own)
 *      rank(audio j) = j + #(video units with (stream, pts) <= its own)
 *    one binary search each (jm_tsp_rank), and the ranks are a permutation of 0 .. n_v + n_a - 1: the MERGED order.  A stream's
 *    merged units tile one range of the output; the first stream begins at 0, each next one at the end before it rounded up
 *    to 16 as in enc_ts.h.  A range that begins at a multiple of 16 and holds p packets ends 188 p behind it, so the padding
 *    behind a stream depends on its own packets alone and the begins are a plain prefix sum of jm_ts_align16(188 p).
 * PCR.  With JM_TSP_PCR the FIRST packet of every unit of the carrier kind (video if present, else audio) carries an adaptation
 *    field of 8 bytes: length 7, flags 0x10, six PCR bytes with base = (pts - pcr_lead) mod 2^33 and extension 0:
 *    base >> 25, base >> 17, base >> 9, base >> 1, ((base & 1) << 7) | 0x7e, 0x00.  The first packet is the only place:
 *    ts.js:143 ends a video PES at any LATER packet with an adaptation field; one on the payload-start packet ends nothing.
 * GEOMETRY, enc_ts.h's `lead` generalised:
 *      lead0   = 8 for a PCR unit, else 0
 *      lead    = lead0 + ((!sized && (total + lead0) % 184 == 0) ? 1 : 0)
 *      packets = (total + lead + 183) / 184
 *      done(k) = k ? 184 k - lead : 0
 *    packet 0's field is `lead` bytes (the PCR, then at most one 0xff), the last packet's is raised to fill the packet -- for
 *    a unit that fits one packet: the PCR followed by 0xff.  With lead0 == 0 jm_tsp_packets / jm_tsp_packet / jm_tsp_dword
 *    return what jm_ts_packets / jm_ts_packet / jm_ts_dword return.
 * PSI.  With JM_TSP_PSI one PAT packet (PID 0) and one PMT packet (rule.pmt_pid) go in front of a unit when it is its stream's
 *    first unit of the call and the stream has emitted none since create / reset (the `started` word), or when it is a video
 *    unit whose payload begins 00 00 01 B3 (every I picture the encoder writes: a viewer joining at a key picture gets the
 *    tables first); once if both hold.  The two packets are constant for a handle: jm_tsp_psi_packets builds them on the
 *    host, the device patches the continuity nibble only.
 * STATE.  JM_TSP_STATE = 5 words per stream number: the counters of PAT, PMT, video, audio, and `started`.  A unit's counter is
 *    its stream's word for its PID plus the packets of the earlier units of that PID in the stream.  Everything is STAGED and
 *    becomes the stream's words only when the call fits `cap`: an overflowing call writes nothing and leaves all five.
 * THE PLAN in steps a lane does alone, around three scans (ts_program.hip does them across a workgroup, the simulator in a loop):
 *      jm_tsp_step_place   a lane per UNIT: its rank, its packets, whether it is key           -> placed[rank]
 *      jm_tsp_step_count   a lane per MERGED unit: PSI in front or not, the four counts it adds (PAT = PMT, video, audio, all)
 *      (scan 1: exclusive prefix of the four counts over the merged units)
 *      jm_tsp_step_edges   a stream's first / last merged unit leaves the prefix at the stream's begin / end
 *      (scan 2: exclusive prefix of jm_tsp_stream_size over the stream numbers)
 *      jm_tsp_step_stream  a lane per STREAM: its range, its staged words
 *      jm_tsp_step_final   a lane per merged unit: `first`, `at`, the counters of its first packet and of its PSI pair
 * OUT OF SCOPE: packet-level interleave inside a unit; T-STD buffer conformance, constant-rate null-packet padding, more
 *    than one audio PID; several frames per PES beyond what the caller's ranges express; B-picture DTS; Node bindings.
 */
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "enc_ts.h"

#define JM_TSP_PSI 1u            /* (= JSMPEG_HIP_TSP_PSI) */
#define JM_TSP_PCR 2u            /* (= JSMPEG_HIP_TSP_PCR) */
#define JM_TSP_NO_PID 0x1fffu    /* a kind that is absent */
#define JM_TSP_STATE 5u          /* words per stream number: PAT, PMT, video, audio counters, started */
#define JM_TSP_P_PSI 0x1000u     /* JmTspPlaced::cc: PAT + PMT lie in front of the unit */
#define JM_TSP_P_KEY 0x2000u     /* ... it is a video unit that begins with a sequence header */
#define JM_TSP_KEY_DWORD 0xb3010000u   /* 00 00 01 B3 as it lies in memory */

struct JmTspRule {
	uint32_t pid[2], sid[2];     /* [0] video, [1] audio */
	uint32_t pmt_pid, flags;
	uint64_t pcr_lead;           /* 90 kHz: how far the PCR runs behind the PTS it is written with */
};

struct JmTspPlaced {             /* what the plan leaves per MERGED unit, 32 bytes */
	uint64_t at;                 /* of its first packet in the output (the PAT, if PSI lies in front), a multiple of 4 */
	uint32_t first;              /* that packet among all packets of the call */
	uint32_t packets;            /* of the unit itself */
	uint32_t unit;               /* kind << 31 | its index in its table */
	uint32_t stream;
	uint32_t cc;                 /* counter of its first packet | PAT's << 4 | PMT's << 8 | JM_TSP_P_* */
	uint32_t pad;
};

JM_HD uint32_t jm_tsp_carrier(const JmTspRule &r) { return r.pid[0] != JM_TSP_NO_PID ? 0u : 1u; }
JM_HD uint32_t jm_tsp_lead0(const JmTspRule &r, uint32_t kind) { return ((r.flags & JM_TSP_PCR) && kind == jm_tsp_carrier(r)) ? 8u : 0u; }

/* ------------------------------------------------------------------ a unit's packets */
JM_HD uint32_t jm_tsp_lead(uint32_t bytes, uint32_t lead0) {
	const uint64_t total = (uint64_t)JM_TS_HEAD + bytes;
	return lead0 + (((uint64_t)bytes + 8u > 0xffffu && (total + lead0) % 184u == 0) ? 1u : 0u);
}
JM_HD uint32_t jm_tsp_packets(uint32_t bytes, uint32_t lead0) { return (uint32_t)(((uint64_t)JM_TS_HEAD + bytes + jm_tsp_lead(bytes, lead0) + 183u) / 184u); }

/* packet k of a unit: the first byte of header + payload it carries, and its bytes of adaptation field (the length byte included) */
JM_HD void jm_tsp_packet(uint32_t bytes, uint32_t lead0, uint32_t k, uint64_t *done, uint32_t *stuff) {
	const uint64_t total = (uint64_t)JM_TS_HEAD + bytes;
	const uint32_t lead = jm_tsp_lead(bytes, lead0);
	const uint64_t d = k ? 184ull * k - lead : 0;
	uint32_t s = k == 0 ? lead : 0u;
	if (total - d + s < 184u) s = 184u - (uint32_t)(total - d);
	*done = d; *stuff = s;
}

/* byte i (0 .. 5) of the PCR field written with `pts` */
JM_HD uint32_t jm_tsp_pcr_byte(uint32_t i, uint64_t pts, uint64_t pcr_lead) {
	const uint64_t base = (pts - pcr_lead) & 0x1ffffffffull;
	switch (i) {
	case 0: return (uint32_t)(base >> 25) & 0xffu;
	case 1: return (uint32_t)(base >> 17) & 0xffu;
	case 2: return (uint32_t)(base >> 9) & 0xffu;
	case 3: return (uint32_t)(base >> 1) & 0xffu;
	case 4: return (uint32_t)((base & 1u) << 7) | 0x7eu;
	default: return 0u;
	}
}

/* DWORD w (0 .. 46) OF PACKET k of unit u, jm_ts_dword with a PCR in the first packet's field when lead0 is 8 */
template <class Fetch>
JM_HD uint32_t jm_tsp_dword(const JmTsUnit &u, uint32_t cc_unit, uint32_t stream_id, uint32_t pid, uint32_t lead0, uint64_t pcr_lead, uint32_t k, uint32_t w, const Fetch &fetch) {
	uint64_t done;
	uint32_t stuff;
	jm_tsp_packet(u.bytes, lead0, k, &done, &stuff);
	if (w == 0) return 0x47u | (((k == 0 ? 0x40u : 0u) | (pid >> 8)) << 8) | ((pid & 0xffu) << 16) | (((stuff ? 0x30u : 0x10u) | ((cc_unit + k) & 15u)) << 24);
	const bool pcr = lead0 != 0 && k == 0;
	const uint32_t q0 = 4u * w - 4u;                                   /* the dword's first byte behind the packet header, 0 .. 180 */
	const int64_t i0 = (int64_t)done + (int64_t)q0 - (int64_t)stuff - (int64_t)JM_TS_HEAD;   /* the payload byte at the dword's byte 0 */
	if (q0 >= stuff && i0 >= 0) return fetch(i0, 0u, 4u);
	uint32_t v = 0, lo = 4u;
	for (uint32_t j = 0; j < 4u; j++) {
		const uint32_t q = q0 + j;
		uint32_t b;
		if (q < stuff) b = q == 0 ? stuff - 1u : (q == 1u ? (pcr ? 0x10u : 0u) : ((pcr && q < 8u) ? jm_tsp_pcr_byte(q - 2u, u.pts, pcr_lead) : 0xffu));
		else if (i0 + (int64_t)j < 0) b = jm_ts_head_byte((uint32_t)(i0 + (int64_t)j + JM_TS_HEAD), u.bytes, u.pts, stream_id);
		else { lo = j; break; }                                        /* payload from here to the dword's end */
		v |= b << (8u * j);
	}
	if (lo < 4u) v |= fetch(i0, lo, 4u) & (0xffffffffu << (8u * lo));
	return v;
}

/* ------------------------------------------------------------------ the order */
/* how many units of t[0 .. n) lie in front of (stream, pts): the smaller ones, with_equal: and the equal ones */
JM_HD uint32_t jm_tsp_count_before(const JmTsUnit *t, uint32_t n, uint32_t stream, uint64_t pts, bool with_equal) {
	uint32_t lo = 0, hi = n;
	while (lo < hi) {
		const uint32_t mid = lo + ((hi - lo) >> 1);
		const uint32_t s = t[mid].stream;
		const uint64_t p = t[mid].pts;
		const bool before = s < stream || (s == stream && (with_equal ? p <= pts : p < pts));
		if (before) lo = mid + 1u; else hi = mid;
	}
	return lo;
}
/* where unit i of `kind` lies among all units of the call */
JM_HD uint32_t jm_tsp_rank(const JmTsUnit *v, uint32_t n_v, const JmTsUnit *a, uint32_t n_a, uint32_t kind, uint32_t i) {
	return kind == 0 ? i + jm_tsp_count_before(a, n_a, v[i].stream, v[i].pts, false)
	                 : i + jm_tsp_count_before(v, n_v, a[i].stream, a[i].pts, true);
}

/* ------------------------------------------------------------------ the plan's steps (a lane each; the scans are the caller's) */
/* per stream number: the exclusive prefix of the four counts at the stream's first merged unit, and behind its last */
struct JmTspEdges { uint32_t begin[4], end[4]; };

/* A LANE PER UNIT.  rank[]: video units first, then audio at n_v.  Units under 4 bytes are not key. */
template <class Fetch>
JM_HD void jm_tsp_step_place(const JmTspRule &r, const JmTsUnit *v, uint32_t n_v, const JmTsUnit *a, uint32_t n_a, uint32_t kind, uint32_t i,
                             const uint8_t *src, JmTspPlaced *placed, uint32_t *rank) {
	const JmTsUnit u = kind ? a[i] : v[i];
	const uint32_t m = jm_tsp_rank(v, n_v, a, n_a, kind, i);
	uint32_t key = 0;
	if (kind == 0 && u.bytes >= 4u) {
		Fetch f;
		f.base = src + u.off;
		key = f(0, 0u, 4u) == JM_TSP_KEY_DWORD ? JM_TSP_P_KEY : 0u;
	}
	JmTspPlaced p;
	p.at = 0; p.first = 0; p.packets = jm_tsp_packets(u.bytes, jm_tsp_lead0(r, kind));
	p.unit = (kind << 31) | i; p.stream = u.stream; p.cc = key; p.pad = 0;
	placed[m] = p;
	rank[kind ? n_v + i : i] = m;
}

/* A LANE PER MERGED UNIT: what it adds to the four sums -- PAT (= PMT) packets, video packets, audio packets, all packets.
 * Reads its left neighbour's stream; returns the unit's flags with JM_TSP_P_PSI decided (the caller keeps them for step_final:
 * nothing is stored here, so no lane reads what another writes) */
JM_HD uint32_t jm_tsp_step_count(const JmTspRule &r, const JmTspPlaced *placed, uint32_t m, const uint32_t *state, uint32_t c[4]) {
	const JmTspPlaced p = placed[m];
	const bool opens = m == 0 || placed[m - 1u].stream != p.stream;
	const bool psi = (r.flags & JM_TSP_PSI) && ((opens && !state[JM_TSP_STATE * p.stream + 4u]) || (p.cc & JM_TSP_P_KEY));
	const uint32_t kind = p.unit >> 31;
	c[0] = psi ? 1u : 0u; c[1] = kind == 0 ? p.packets : 0u; c[2] = kind == 1u ? p.packets : 0u; c[3] = p.packets + (psi ? 2u : 0u);
	return (p.cc & JM_TSP_P_KEY) | (psi ? JM_TSP_P_PSI : 0u);
}

/* behind scan 1 (e: the exclusive prefix at m, c: what m adds): the edges of m's stream, if m is at one; n: all merged units */
JM_HD void jm_tsp_step_edges(const JmTspPlaced *placed, uint32_t m, uint32_t n, const uint32_t e[4], const uint32_t c[4], JmTspEdges *edges) {
	const uint32_t s = placed[m].stream;
	if (m == 0 || placed[m - 1u].stream != s) for (int i = 0; i < 4; i++) edges[s].begin[i] = e[i];
	if (m + 1u == n || placed[m + 1u].stream != s) for (int i = 0; i < 4; i++) edges[s].end[i] = e[i] + c[i];
}

/* the bytes stream s takes, the round-up to the next stream's begin included (0: not in the call) */
JM_HD uint64_t jm_tsp_stream_size(const JmTspEdges *edges, uint32_t s) {
	return jm_ts_align16((uint64_t)(edges[s].end[3] - edges[s].begin[3]) * JM_TS_PACKET);
}

/* A LANE PER STREAM NUMBER behind scan 2 (begin: the exclusive prefix of the sizes at s): its range and its staged words;
 * returns the stream's end (0: not in the call) -- the call's total is the largest */
JM_HD uint64_t jm_tsp_step_stream(uint32_t s, uint64_t begin, const JmTspEdges *edges, const uint32_t *state, uint64_t *stream_begin, uint64_t *stream_end, uint32_t *staged) {
	const JmTspEdges &g = edges[s];
	const uint32_t packets = g.end[3] - g.begin[3];
	const uint32_t *w = state + JM_TSP_STATE * s;
	uint32_t *o = staged + JM_TSP_STATE * s;
	stream_begin[s] = packets ? begin : 0;
	stream_end[s] = packets ? begin + (uint64_t)packets * JM_TS_PACKET : 0;
	o[0] = (w[0] + g.end[0] - g.begin[0]) & 15u;
	o[1] = (w[1] + g.end[0] - g.begin[0]) & 15u;
	o[2] = (w[2] + g.end[1] - g.begin[1]) & 15u;
	o[3] = (w[3] + g.end[2] - g.begin[2]) & 15u;
	o[4] = packets ? 1u : w[4];
	return stream_end[s];
}

/* A LANE PER MERGED UNIT, last: flags from step_count, e its exclusive prefix of scan 1 */
JM_HD void jm_tsp_step_final(JmTspPlaced *placed, uint32_t m, uint32_t flags, const uint32_t e[4], const JmTspEdges *edges, const uint32_t *state, const uint64_t *stream_begin) {
	const uint32_t s = placed[m].stream, kind = placed[m].unit >> 31;
	const JmTspEdges &g = edges[s];
	const uint32_t *w = state + JM_TSP_STATE * s;
	placed[m].first = e[3];
	placed[m].at = stream_begin[s] + (uint64_t)(e[3] - g.begin[3]) * JM_TS_PACKET;
	placed[m].cc = ((w[2u + kind] + e[1u + kind] - g.begin[1u + kind]) & 15u) | (((w[0] + e[0] - g.begin[0]) & 15u) << 4) | (((w[1] + e[0] - g.begin[0]) & 15u) << 8) | flags;
}

/* the staged words of stream s become its words: only behind a call that did not overflow */
JM_HD void jm_tsp_commit(uint32_t s, const uint32_t *staged, uint32_t *state) {
	for (uint32_t i = 0; i < JM_TSP_STATE; i++) state[JM_TSP_STATE * s + i] = staged[JM_TSP_STATE * s + i];
}

/* ------------------------------------------------------------------ the write */
/* the merged unit packet p (of all the call's packets) belongs to: the last one whose `first` is at most p; n >= 1 */
JM_HD uint32_t jm_tsp_find_unit(const JmTspPlaced *placed, uint32_t n, uint32_t p) {
	uint32_t lo = 0, hi = n;
	while (hi - lo > 1u) {
		const uint32_t mid = lo + ((hi - lo) >> 1);
		if (placed[mid].first <= p) lo = mid; else hi = mid;
	}
	return lo;
}

/* THE OUTPUT DWORD g of a call with `packets` packets, g < packets * 47: where it lies (in dwords) and what it is.
 * tpl: the PAT and the PMT packet, 47 dwords each, their continuity nibbles 0 */
template <class Fetch>
JM_HD uint32_t jm_tsp_output_dword(const JmTspRule &r, const JmTsUnit *v, const JmTsUnit *a, const JmTspPlaced *placed, uint32_t n, uint64_t g,
                                   const uint32_t *tpl, const uint8_t *src_v, const uint8_t *src_a, uint64_t *where) {
	const uint32_t p = (uint32_t)(g / JM_TS_DWORDS), w = (uint32_t)(g % JM_TS_DWORDS);
	const uint32_t m = jm_tsp_find_unit(placed, n, p);
	const JmTspPlaced pl = placed[m];
	uint32_t k = p - pl.first;
	*where = (pl.at + (uint64_t)k * JM_TS_PACKET) / 4u + w;
	if (pl.cc & JM_TSP_P_PSI) {
		if (k < 2u) return tpl[JM_TS_DWORDS * k + w] | (w == 0 ? ((pl.cc >> (4u + 4u * k)) & 15u) << 24 : 0u);
		k -= 2u;
	}
	const uint32_t kind = pl.unit >> 31;
	const JmTsUnit u = (kind ? a : v)[pl.unit & 0x7fffffffu];
	Fetch f;
	f.base = (kind ? src_a : src_v) + u.off;
	return jm_tsp_dword(u, pl.cc & 15u, r.sid[kind], r.pid[kind], jm_tsp_lead0(r, kind), r.pcr_lead, k, w, f);
}

/* ------------------------------------------------------------------ capacity
 * A unit of b bytes has at most b / 184 + 2 packets: (b + 14 + 9 + 183) / 184 with the longest lead, PCR and one stuffing byte,
 * and b % 184 + 206 <= 389 < 3 * 184.  The floors of the units sum to at most the floor of their sum.  PSI goes in front
 * of key video units -- at most every video unit -- and of a stream's first unit: 2 more packets per video unit and per
 * stream.  A stream's begin is rounded up by at most 15. */
JM_HD uint64_t jm_tsp_bound(uint64_t v_bytes, uint32_t n_v, uint64_t a_bytes, uint32_t n_a, uint32_t streams) {
	return (uint64_t)JM_TS_PACKET * (v_bytes / 184u + a_bytes / 184u + 2ull * n_v + 2ull * n_a + 2ull * n_v + 2ull * streams) + 15ull * streams;
}

/* ------------------------------------------------------------------ PSI, on the host */
/* CRC-32/MPEG-2: poly 0x04C11DB7, init 0xffffffff, not reflected, no final xor */
static inline uint32_t jm_tsp_crc32(const uint8_t *p, size_t n) {
	uint32_t c = 0xffffffffu;
	for (size_t i = 0; i < n; i++) {
		c ^= (uint32_t)p[i] << 24;
		for (int b = 0; b < 8; b++) c = (c & 0x80000000u) ? (c << 1) ^ 0x04c11db7u : c << 1;
	}
	return c;
}
/* closes a section that begins at pk[5] and has `len` bytes in front of its CRC: the CRC, then 0xff to the packet's end */
static inline void jm_tsp_psi_close(uint8_t *pk, uint32_t len) {
	const uint32_t crc = jm_tsp_crc32(pk + 5, len);
	uint8_t *q = pk + 5 + len;
	q[0] = (uint8_t)(crc >> 24); q[1] = (uint8_t)(crc >> 16); q[2] = (uint8_t)(crc >> 8); q[3] = (uint8_t)crc;
	memset(q + 4, 0xff, JM_TS_PACKET - 5u - len - 4u);
}
/* the PAT packet, then the PMT packet, continuity nibbles 0 */
static inline void jm_tsp_psi_packets(const JmTspRule &r, uint32_t program_number, uint32_t transport_stream_id, uint8_t out[2 * JM_TS_PACKET]) {
	uint8_t *p = out;
	p[0] = 0x47; p[1] = 0x40; p[2] = 0x00; p[3] = 0x10; p[4] = 0x00;            /* payload start, PID 0; pointer_field 0 */
	p[5] = 0x00; p[6] = 0xb0; p[7] = 13;                                        /* table 0, section syntax, 5 + 4 + 4 bytes follow */
	p[8] = (uint8_t)(transport_stream_id >> 8); p[9] = (uint8_t)transport_stream_id;
	p[10] = 0xc1; p[11] = 0; p[12] = 0;                                         /* version 0, current; section 0 of 0 */
	p[13] = (uint8_t)(program_number >> 8); p[14] = (uint8_t)program_number;
	p[15] = (uint8_t)(0xe0u | (r.pmt_pid >> 8)); p[16] = (uint8_t)r.pmt_pid;
	jm_tsp_psi_close(p, 12);
	p = out + JM_TS_PACKET;
	const uint32_t kinds = (r.pid[0] != JM_TSP_NO_PID ? 1u : 0u) + (r.pid[1] != JM_TSP_NO_PID ? 1u : 0u);
	const uint32_t pcr_pid = r.pid[jm_tsp_carrier(r)], slen = 9u + 5u * kinds + 4u;
	p[0] = 0x47; p[1] = (uint8_t)(0x40u | (r.pmt_pid >> 8)); p[2] = (uint8_t)r.pmt_pid; p[3] = 0x10; p[4] = 0x00;
	p[5] = 0x02; p[6] = (uint8_t)(0xb0u | (slen >> 8)); p[7] = (uint8_t)slen;
	p[8] = (uint8_t)(program_number >> 8); p[9] = (uint8_t)program_number;
	p[10] = 0xc1; p[11] = 0; p[12] = 0;
	p[13] = (uint8_t)(0xe0u | (pcr_pid >> 8)); p[14] = (uint8_t)pcr_pid;
	p[15] = 0xf0; p[16] = 0x00;                                                 /* program_info_length 0 */
	uint32_t at = 17;
	for (uint32_t kind = 0; kind < 2u; kind++) {
		if (r.pid[kind] == JM_TSP_NO_PID) continue;
		p[at] = kind ? 0x03 : 0x01;                                             /* MPEG-1 audio / MPEG-1 video */
		p[at + 1] = (uint8_t)(0xe0u | (r.pid[kind] >> 8)); p[at + 2] = (uint8_t)r.pid[kind];
		p[at + 3] = 0xf0; p[at + 4] = 0x00;                                     /* ES_info_length 0 */
		at += 5;
	}
	jm_tsp_psi_close(p, at - 5u);
}
