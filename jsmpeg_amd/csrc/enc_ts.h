/*
 * MPEG-TS MUX, ONE PES PER UNIT (include/jsmpeg_hip.h part 8): which bytes packet k of a unit holds, where a unit's packets lie
 * in the output and which continuity counter they carry, stated once, host + device -- what the kernels of encode.hip
 * (k_ts_plan, k_ts_write), the host mux (jsmpeg_hip_ts_mux_host) and the CPU simulator (tests/sim/sim_enc_ts.cpp) share.
 *
 * THE UNIT.  `bytes` payload bytes behind a PES header of 14: 00 00 01 stream_id, PES_packet_length (bytes + 8, or 0 when that
 *    does not fit 16 bits), 80 80 05, the PTS in five bytes.  total = 14 + bytes go out in 184-byte pieces, one per packet.
 *    The reference's demuxer (ts.js:127-147) ends a PES by its length or -- length 0 -- by a LATER packet of it that carries an
 *    adaptation field, so: the unit's last packet is stuffed to its size by an adaptation field, no packet between the first and
 *    the last has one, and a unit of unknown length whose last packet would come out full gets one stuffing byte in its FIRST
 *    packet (`lead`; an adaptation field there ends nothing: ts.js:143).
 * NO WALK.  Nothing about packet k depends on the packets before it:
 *      sized   = bytes + 8 <= 0xffff
 *      lead    = (!sized && total % 184 == 0) ? 1 : 0
 *      packets = (total + lead + 183) / 184
 *      done    = k ? 184 k - lead : 0                   the first byte of header + payload the packet carries
 *      stuff   = (k == 0 ? lead : 0), raised to 184 - (total - done) when total - done + stuff < 184
 *    and the packet carries bytes [done, done + 184 - stuff) behind 47 sync, PUSI (k == 0) | pid, (stuff ? 30 : 10) | counter,
 *    and `stuff` bytes of adaptation field: its length stuff - 1, a flags byte 0, 0xff.  The counter is (cc_unit + k) & 15.
 *    A packet is 47 dwords; jm_ts_dword gives any one of them, so every output dword has one owner and is stored once.
 * THE PLAN (jm_ts_plan_*, one walk over the units, which are contiguous per stream, streams ascending): a unit's packets lie
 *    back to back from JmTsPlaced::at; the first stream begins at 0, each next one at the end before it rounded up to 16 (the
 *    bytes between are unspecified); a stream's first unit takes its counter from the stream's word cc[stream], and the counter
 *    behind the stream's last unit is STAGED (cc_next[stream]): it becomes the stream's word (jm_ts_plan_commit) only when the
 *    call did not overflow, so that a failed call leaves the counters where it found them.
 * DEFAULT PTS (jm_ts_default_pts): floor(ordinal * 90000 * den / num) in 64 bits, masked to 33 bits, num / den the pictures per
 *    second of the sequence header's frame_rate_code.
 * OUT OF SCOPE: PAT / PMT / PCR (jsmpeg's demuxer needs none; other players do), audio or a second PID in the same buffer
 *    (packets are self-contained, so a host may interleave) -- both are part 10's: ts_prog.h builds a program on this rule.
 */
#pragma once
#include <stdint.h>

#include "recon_block.h"

#define JM_TS_PACKET 188u
#define JM_TS_DWORDS 47u         /* of a packet */
#define JM_TS_HEAD 14u           /* the PES header */
#define JM_TS_NO_STREAM 0xffffffffu

struct JmTsUnit {                /* the device table, 24 bytes */
	uint64_t off;                /* of the payload in the source bytes */
	uint32_t bytes, stream;
	uint64_t pts;                /* 90 kHz; its low 33 bits go out */
};

struct JmTsPlaced {              /* what the plan leaves per unit, 24 bytes */
	uint64_t at;                 /* of its first packet in the output, a multiple of 4 */
	uint32_t first;              /* its first packet among all packets of the call */
	uint32_t packets;
	uint32_t cc;                 /* the counter of its first packet */
	uint32_t pad;
};

JM_HD uint32_t jm_ts_lead(uint32_t bytes) {
	const uint64_t total = (uint64_t)JM_TS_HEAD + bytes;
	return ((uint64_t)bytes + 8u > 0xffffu && total % 184u == 0) ? 1u : 0u;
}
JM_HD uint32_t jm_ts_packets(uint32_t bytes) { return (uint32_t)(((uint64_t)JM_TS_HEAD + bytes + jm_ts_lead(bytes) + 183u) / 184u); }

/* packet k of a unit: the first byte of header + payload it carries, and its bytes of adaptation field (the length byte included) */
JM_HD void jm_ts_packet(uint32_t bytes, uint32_t k, uint64_t *done, uint32_t *stuff) {
	const uint64_t total = (uint64_t)JM_TS_HEAD + bytes;
	const uint32_t lead = jm_ts_lead(bytes);
	const uint64_t d = k ? 184ull * k - lead : 0;
	uint32_t s = k == 0 ? lead : 0u;
	if (total - d + s < 184u) s = 184u - (uint32_t)(total - d);
	*done = d; *stuff = s;
}

/* byte i (0 .. 13) of the PES header */
JM_HD uint32_t jm_ts_head_byte(uint32_t i, uint32_t bytes, uint64_t pts, uint32_t stream_id) {
	const uint32_t plen = (uint64_t)bytes + 8u <= 0xffffu ? bytes + 8u : 0u;
	const uint64_t p = pts & 0x1ffffffffull;
	switch (i) {
	case 0: case 1: return 0u;
	case 2: return 1u;
	case 3: return stream_id & 0xffu;
	case 4: return plen >> 8;
	case 5: return plen & 0xffu;
	case 6: case 7: return 0x80u;
	case 8: return 5u;
	case 9: return (uint32_t)(0x21u | ((p >> 29) & 0x0eu));
	case 10: return (uint32_t)(p >> 22) & 0xffu;
	case 11: return (uint32_t)(0x01u | ((p >> 14) & 0xfeu));
	case 12: return (uint32_t)(p >> 7) & 0xffu;
	default: return (uint32_t)(0x01u | ((p << 1) & 0xfeu));
	}
}

/* DWORD w (0 .. 46) OF PACKET k of unit u, little endian as it lies in memory; cc_unit: the counter of the unit's first packet.
 * fetch(i, lo, hi) returns a dword whose bytes j = lo .. hi - 1 are payload bytes i + j (all inside 0 .. bytes - 1; i itself
 * may be negative) -- its other bytes are not used. */
template <class Fetch>
JM_HD uint32_t jm_ts_dword(const JmTsUnit &u, uint32_t cc_unit, uint32_t stream_id, uint32_t pid, uint32_t k, uint32_t w, const Fetch &fetch) {
	uint64_t done;
	uint32_t stuff;
	jm_ts_packet(u.bytes, k, &done, &stuff);
	if (w == 0) return 0x47u | (((k == 0 ? 0x40u : 0u) | (pid >> 8)) << 8) | ((pid & 0xffu) << 16) | (((stuff ? 0x30u : 0x10u) | ((cc_unit + k) & 15u)) << 24);
	const uint32_t q0 = 4u * w - 4u;                                   /* the dword's first byte behind the packet header, 0 .. 180 */
	const int64_t i0 = (int64_t)done + (int64_t)q0 - (int64_t)stuff - (int64_t)JM_TS_HEAD;   /* the payload byte at the dword's byte 0 */
	if (q0 >= stuff && i0 >= 0) return fetch(i0, 0u, 4u);
	uint32_t v = 0, lo = 4u;
	for (uint32_t j = 0; j < 4u; j++) {
		const uint32_t q = q0 + j;
		uint32_t b;
		if (q < stuff) b = q == 0 ? stuff - 1u : (q == 1u ? 0u : 0xffu);
		else if (i0 + (int64_t)j < 0) b = jm_ts_head_byte((uint32_t)(i0 + (int64_t)j + JM_TS_HEAD), u.bytes, u.pts, stream_id);
		else { lo = j; break; }                                        /* payload from here to the dword's end */
		v |= b << (8u * j);
	}
	if (lo < 4u) v |= fetch(i0, lo, 4u) & (0xffffffffu << (8u * lo));
	return v;
}

/* the fetch of jm_ts_dword from ALIGNED dwords, combined by v_alignbyte; only dwords that hold at least one of the bytes asked
 * for are loaded.  base: where the unit's payload begins, any alignment. */
struct JmTsFetchAligned {
	const uint8_t *base;
	JM_HD uint32_t operator()(int64_t i, uint32_t lo, uint32_t hi) const {
		const uintptr_t a = (uintptr_t)base + (uintptr_t)i;
		const uint32_t s = (uint32_t)(a & 3u);
		JM_GLOBAL const uint32_t *q = (JM_GLOBAL const uint32_t *)(a - s);
		const uint32_t d0 = lo + s < 4u ? q[0] : 0u, d1 = s + hi > 4u ? q[1] : 0u;
		return jm_alignbyte(d1, d0, s);
	}
};
/* the same byte by byte (the host, whose source has no readable dword around a unit's ends) */
struct JmTsFetchBytes {
	const uint8_t *base;
	JM_HD uint32_t operator()(int64_t i, uint32_t lo, uint32_t hi) const {
		uint32_t v = 0;
		for (uint32_t j = lo; j < hi; j++) v |= (uint32_t)base[i + (int64_t)j] << (8u * j);
		return v;
	}
};

/* ------------------------------------------------------------------ the plan */
struct JmTsPlan {
	uint64_t at;                 /* next free byte */
	uint32_t stream;             /* of the unit before, JM_TS_NO_STREAM before the first */
	uint32_t cc;                 /* the counter of the next packet of that stream */
	uint32_t first;              /* packets so far */
};
JM_HD uint64_t jm_ts_align16(uint64_t v) { return (v + 15u) & ~(uint64_t)15u; }
JM_HD JmTsPlan jm_ts_plan_begin() { JmTsPlan p; p.at = 0; p.stream = JM_TS_NO_STREAM; p.cc = 0; p.first = 0; return p; }
JM_HD void jm_ts_plan_end_stream(JmTsPlan &p, uint64_t *stream_end, uint32_t *cc_next) {
	if (p.stream == JM_TS_NO_STREAM) return;
	stream_end[p.stream] = p.at;
	cc_next[p.stream] = p.cc;
}
/* THE PLAN STEP PER UNIT.  cc: the streams' counter words (read only); stream_begin, stream_end, cc_next: per stream number */
JM_HD JmTsPlaced jm_ts_plan_unit(JmTsPlan &p, uint32_t stream, uint32_t bytes, const uint32_t *cc, uint64_t *stream_begin, uint64_t *stream_end, uint32_t *cc_next) {
	if (stream != p.stream) {
		jm_ts_plan_end_stream(p, stream_end, cc_next);
		p.at = jm_ts_align16(p.at);
		stream_begin[stream] = p.at;
		p.stream = stream;
		p.cc = cc[stream] & 15u;
	}
	JmTsPlaced u;
	u.at = p.at; u.first = p.first; u.packets = jm_ts_packets(bytes); u.cc = p.cc; u.pad = 0;
	p.at += (uint64_t)u.packets * JM_TS_PACKET;
	p.first += u.packets;
	p.cc = (p.cc + u.packets) & 15u;
	return u;
}
/* behind the last unit: the total; result: total bytes | status (1: the total is above cap) | packets */
JM_HD void jm_ts_plan_close(JmTsPlan &p, uint64_t cap, uint64_t *stream_end, uint32_t *cc_next, uint64_t *result) {
	jm_ts_plan_end_stream(p, stream_end, cc_next);
	result[0] = p.at;
	result[1] = p.at > cap ? 1u : 0u;
	result[2] = p.first;
}
/* the staged counter of stream s becomes its word: only behind a call that did not overflow, only for a stream the call had */
JM_HD void jm_ts_plan_commit(uint32_t s, const uint64_t *stream_begin, const uint64_t *stream_end, const uint32_t *cc_next, uint32_t *cc) {
	if (stream_end[s] > stream_begin[s]) cc[s] = cc_next[s];
}

/* the unit packet p (of all the call's packets) belongs to: the last one whose `first` is at most p; n >= 1 */
JM_HD uint32_t jm_ts_find_unit(const JmTsPlaced *placed, uint32_t n, uint32_t p) {
	uint32_t lo = 0, hi = n;
	while (hi - lo > 1u) {
		const uint32_t mid = lo + ((hi - lo) >> 1);
		if (placed[mid].first <= p) lo = mid; else hi = mid;
	}
	return lo;
}

/* THE OUTPUT DWORD g of a call with `packets` packets, g < packets * 47: where it lies (in dwords) and what it is */
template <class Fetch>
JM_HD uint32_t jm_ts_output_dword(const JmTsUnit *units, const JmTsPlaced *placed, uint32_t n, uint64_t g, uint32_t stream_id, uint32_t pid, const uint8_t *src, uint64_t *where) {
	const uint32_t p = (uint32_t)(g / JM_TS_DWORDS), w = (uint32_t)(g % JM_TS_DWORDS);
	const uint32_t i = jm_ts_find_unit(placed, n, p), k = p - placed[i].first;
	const JmTsUnit u = units[i];
	Fetch f;
	f.base = src + u.off;
	*where = (placed[i].at + (uint64_t)k * JM_TS_PACKET) / 4u + w;
	return jm_ts_dword(u, placed[i].cc, stream_id, pid, k, w, f);
}

/* a safe capacity for es_bytes of payload in `units` units over `streams` streams: a unit of b bytes has at most b / 184 + 2
 * packets ((b + 14 + 1 + 183) / 184), and a stream's begin is rounded up by at most 15 */
JM_HD uint64_t jm_ts_bound(uint64_t es_bytes, uint32_t units, uint32_t streams) {
	return (uint64_t)JM_TS_PACKET * (es_bytes / 184u + 2ull * units) + 15ull * streams;
}

/* pictures per second of a frame_rate_code 1 .. 8 as num / den */
JM_HD void jm_ts_frame_rate(uint32_t code, uint32_t *num, uint32_t *den) {
	*den = (code == 1u || code == 4u || code == 7u) ? 1001u : 1u;
	*num = code == 1u ? 24000u : code == 2u ? 24u : code == 3u ? 25u : code == 4u ? 30000u : code == 5u ? 30u : code == 6u ? 50u : code == 7u ? 60000u : 60u;
}
JM_HD uint64_t jm_ts_default_pts(uint32_t ordinal, uint32_t frame_rate_code) {
	uint32_t num, den;
	jm_ts_frame_rate(frame_rate_code, &num, &den);
	return ((uint64_t)ordinal * 90000u * den / num) & 0x1ffffffffull;
}
