/*
 * Packet framing of the reference's TS demuxer (reference src/ts.js:25-41 write, :43-50 the sync check of
 * parsePacket, :150-187 resync): where the 188-byte packets that ts.js parses lie in a byte stream handed over in
 * one or several write() calls.  A host pre-pass of the ingest stage: one byte looked at per packet while the
 * stream is in sync, the resync search only where it is not.  What the packets SAY is parsed on the device
 * (ts_kernels.hip); the runs found here are copied to the device back to back, so the kernels see nothing but
 * aligned packets.
 *
 *   write(buffer):   bits = leftover + buffer; while (bits.has(188 bytes) && parsePacket()) {}; leftover = the rest
 *   parsePacket():   a byte that is not 0x47 is CONSUMED, then resync(): with fewer than 6 * 188 bytes ahead it gives
 *                    up (false: the write() loop ends, the rest waits for the next write); else the first 0x47 within
 *                    187 bytes that has four more at 188-byte distances becomes the packet's sync byte; none found:
 *                    187 bytes are skipped and the write() loop ends.
 */
#ifndef JSMPEG_AMD_TS_SYNC_H
#define JSMPEG_AMD_TS_SYNC_H

#include <stdint.h>

#include <algorithm>
#include <vector>

struct JmTsRun { uint64_t src; uint32_t packets; };   /* `packets` consecutive 188-byte packets from byte `src` */
struct JmTsWriteEnd { uint64_t packets, end; };       /* after a write(): packets parsed so far, and where its buffer ended */

/* write_bytes[0 .. n_writes): the sizes of the write() calls (their sum may be less than n: the rest is never
 * written); n_writes == 0: one write of everything.  Returns the number of packets; *rest = first byte ts.js still
 * holds as leftover after the last write. */
static inline uint64_t jm_ts_sync_runs(const uint8_t *ts, uint64_t n, const uint64_t *write_bytes, uint32_t n_writes,
                                       std::vector<JmTsRun> &runs, uint64_t *rest, std::vector<JmTsWriteEnd> *ends = nullptr) {
	runs.clear();
	if (ends) ends->clear();
	uint64_t idx = 0, end = 0, total = 0;
	const uint64_t one = n;
	if (n_writes == 0) { write_bytes = &one; n_writes = 1; }
	auto packet_at = [&](uint64_t p) {
		if (!runs.empty() && runs.back().src + 188ull * runs.back().packets == p && runs.back().packets < 0xffffffffu) runs.back().packets++;
		else runs.push_back({ p, 1 });
		total++;
	};
	for (uint32_t w = 0; w < n_writes; w++) {
		end += write_bytes[w];
		if (end > n) end = n;
		while (end - idx >= 188) {
			if (ts[idx] == 0x47) { packet_at(idx); idx += 188; continue; }
			idx += 1;                                          /* the byte has been read */
			if (end - idx < 188 * 6) break;                    /* resync: not enough data, maybe next time */
			int found = -1;
			for (int i = 0; i < 187 && found < 0; i++)
				if (ts[idx + i] == 0x47 && ts[idx + i + 188] == 0x47 && ts[idx + i + 376] == 0x47 && ts[idx + i + 564] == 0x47 &&
				    ts[idx + i + 752] == 0x47) found = i;
			if (found < 0) { idx += 187; break; }              /* garbage: skipped, this write() is over */
			packet_at(idx + (uint64_t)found);
			idx += (uint64_t)found + 188;
		}
		if (ends) ends->push_back({ total, end });
	}
	if (rest) *rest = idx;
	return total;
}

/* The kernels see the framed packets back to back, ts.js sees the written bytes.  The two differ for ONE kind of
 * packet: a payload start whose PES header begins so late that ts.js reads it -- the start code (buffer.js:140-150, which
 * also says yes at the end of the buffer), stream id, PES_packet_length, flags, header_length, PTS (ts.js:79-105) -- from
 * the bytes behind the packet.  There ts.js finds what was written after the packet in THIS write() (junk, a partial
 * packet, nothing: the end of the data), the device the next framed packet (nothing only behind the last).  Returns the
 * first packet for which the two read something different, or -1: then the kernels' view is ts.js's.
 * `ends` as filled by jm_ts_sync_runs for the same input. */
static inline int64_t jm_ts_header_spill_differs(const uint8_t *ts, const std::vector<JmTsRun> &runs, const std::vector<JmTsWriteEnd> &ends) {
	uint64_t k = 0;
	size_t w = 0;
	for (size_t r = 0; r < runs.size(); r++)
		for (uint32_t j = 0; j < runs[r].packets; j++, k++) {
			const uint64_t o = runs[r].src + 188ull * j;
			const uint8_t *p = ts + o;
			if (!(p[1] & 0x40) || !(p[3] & 0x10)) continue;
			const uint32_t idx = (p[3] & 0x20) ? 5u + p[4] : 4u;
			if (idx + 14 <= 188) continue;                             /* start code, fixed header and PTS lie inside the packet */
			while (w + 1 < ends.size() && ends[w].packets <= k) w++;
			const uint64_t vis = ends.empty() ? o + 188 : ends[w].end;   /* the end of the buffer ts.js parses this packet in */
			const bool has_next = j + 1 < runs[r].packets || r + 1 < runs.size();
			const uint64_t next = j + 1 < runs[r].packets ? o + 188 : has_next ? runs[r + 1].src : 0;
			auto ref = [&](uint32_t i) -> int { const uint64_t q = o + idx + i; return q < vis ? ts[q] : -1; };
			auto dev = [&](uint32_t i) -> int { const uint32_t q = idx + i; return q < 188 ? p[q] : has_next ? ts[next + q - 188] : -1; };
			auto start_code = [](int b0, int b1, int b2) { return b0 < 0 || (b0 == 0 && b2 >= 0 && b1 == 0 && b2 == 1); };
			const bool sc = start_code(ref(0), ref(1), ref(2));
			if (sc != start_code(dev(0), dev(1), dev(2))) return (int64_t)k;
			if (!sc) continue;
			const uint32_t n_read = (std::max(ref(7), 0) | std::max(dev(7), 0)) & 0x80 ? 14 : 9;      /* bytes past the end read as 0 */
			for (uint32_t i = 3; i < n_read; i++)
				if (i != 6 && std::max(ref(i), 0) != std::max(dev(i), 0)) return (int64_t)k;
		}
	return -1;
}

#endif
