/*
 * The reference's MPEG-TS demuxer (src/ts.js:25-210) as HOST code in front of a live stream's write(): its state between
 * write() calls, the feed that turns TS bytes into destination.write(pts, payload) calls (live_ts_feed), and the body of a live
 * stream's write_ts around it (live_ts_write).  Shared by the live video streams (live.hip: jsmpeg_hip_live_write_ts,
 * jsmpeg_hip_ts_demux_host) and the live audio streams (mp2_live.hip: jsmpeg_hip_mp2_live_write_ts).  Not installed; nothing
 * outside jsmpeg_amd/csrc includes it.
 */
#pragma once
#include <cstdint>
#include <cstring>
#include <utility>
#include <vector>

#include "host_common.h"
#include "ts_sync.h"

/* a live stream fed as MPEG-TS (jsmpeg_hip_live_write_ts): the reference demuxer's state between write() calls (ts.js:3-41) */
struct LiveTs {
	std::vector<uint8_t> left;                         /* leftoverBytes */
	std::vector<std::pair<uint16_t, uint8_t>> pids;    /* pidsToStreamIds */
	int64_t cur_len = 0, total_len = 0;                /* pesPacketInfo[stream id]: currentLength, totalLength, pts, buffers */
	double pts = 0;
	std::vector<uint8_t> pes;
	std::vector<uint8_t> joined;                       /* scratch: leftover + the new bytes */
	uint64_t writes = 0;                               /* destination.write calls made so far */
};

/* The stream as MPEG-TS: the reference's demuxer in front of write() (src/ts.js:25-147), with its state between calls --
 * leftover bytes of a cut packet (ts.js:25-41), the PID -> stream id table, the PES being collected (currentLength, totalLength,
 * pts) -- kept per live stream.  Host code like the ingest stage's framing pre-pass (ts_sync.h, shared): it looks at packet
 * HEADERS and moves payload bytes; every completed PES goes to `on_pes(pts, bytes, n)` (ts.js:189-194 packetComplete ->
 * destination.write(pts, buffers)).  Where the packets lie -- sync bytes, resync after garbage, what a write leaves over --
 * is jm_ts_sync_runs' restatement of ts.js:43-50, 150-187. */
template <class F>
static void live_ts_feed(LiveTs &T, const uint8_t *buf, uint64_t len, uint32_t stream_id, F &&on_pes) {
	if (!T.left.empty()) {
		T.joined.assign(T.left.begin(), T.left.end());
		T.joined.insert(T.joined.end(), buf, buf + len);
		buf = T.joined.data(); len = T.joined.size();
	}
	std::vector<JmTsRun> runs;
	uint64_t rest = 0;
	jm_ts_sync_runs(buf, len, nullptr, 0, runs, &rest);
	auto complete = [&]() {                                       /* ts.js:189-194 */
		on_pes(T.pts, T.pes.data(), (uint32_t)T.pes.size());
		T.writes++;
		T.total_len = 0; T.cur_len = 0; T.pes.clear();
	};
	for (const JmTsRun &r : runs) {
		for (uint32_t k = 0; k < r.packets; k++) {
			const uint8_t *p = buf + r.src + 188ull * k;
			const bool start = (p[1] & 0x40) != 0;
			const uint16_t pid = (uint16_t)(((p[1] & 0x1f) << 8) | p[2]);
			const uint32_t af = (p[3] >> 4) & 3u;
			uint32_t sid = 0;
			for (const auto &e : T.pids) if (e.first == pid) sid = e.second;
			if (start && sid == stream_id && T.cur_len) complete();        /* a new payload of the stream: the frame before it is over (ts.js:65-73) */
			if (!(af & 1)) continue;
			/* the header fields are read like ts.js reads them: on in the buffer of this write() where they run past the packet,
			 * as zeros behind its end -- and a start code is also "seen" at the end of the buffer (buffer.js:140-150) */
			const uint64_t o = r.src + 188ull * k;
			auto byte = [&](uint64_t i) -> uint32_t { return i < len ? buf[i] : 0u; };
			uint64_t at = o + 4;
			if (af & 2) at = o + 5 + p[4];
			if (start && (at >= len || (buf[at] == 0 && at + 2 < len && buf[at + 1] == 0 && buf[at + 2] == 1))) {
				sid = byte(at + 3);
				bool known = false;
				for (auto &e : T.pids) if (e.first == pid) { e.second = (uint8_t)sid; known = true; }
				if (!known) T.pids.push_back({ pid, (uint8_t)sid });
				const uint32_t packet_length = (byte(at + 4) << 8) | byte(at + 5), flags = byte(at + 7) >> 6, header_length = byte(at + 8);
				if (sid == stream_id) {
					double pts = 0;
					if (flags & 2) {                                        /* the 33-bit PTS in its five bytes (ts.js:96-113) */
						const double p32_30 = (byte(at + 9) >> 1) & 7, p29_15 = ((byte(at + 10) << 8) | byte(at + 11)) >> 1,
						             p14_0 = ((byte(at + 12) << 8) | byte(at + 13)) >> 1;
						pts = (p32_30 * 1073741824.0 + p29_15 * 32768.0 + p14_0) / 90000.0;
					}
					T.total_len = packet_length ? (int64_t)packet_length - (int64_t)header_length - 3 : 0;      /* packetStart (ts.js:189-193); may be negative */
					T.cur_len = 0; T.pts = pts;
				}
				at += 9 + header_length;
			}
			if (sid != stream_id) continue;
			if (at < o + 188) T.pes.insert(T.pes.end(), buf + at, buf + o + 188);
			T.cur_len += (int64_t)(o + 188) - (int64_t)at;                 /* a header past its packet adds no bytes, but the length still moves (ts.js:195-199) */
			const bool full = T.total_len != 0 && T.cur_len >= T.total_len;
			const bool padded = !start && (af & 2);                                     /* the video frame end guess (ts.js:127-147) */
			if (full || padded) complete();
		}
	}
	T.left.assign(buf + rest, buf + len);
}

/* A live stream's write_ts behind its argument checks: the stream's demuxer state (made here on first use) is fed the bytes, and
 * every PES goes to `write(pts, bytes, n)`, the stream's own write (< 0: failed, its message in g_err).  All of them are written;
 * returns 0, or -1 with the FIRST failure's message. */
template <class W>
static int live_ts_write(LiveTs *&ts, const uint8_t *bytes, uint32_t n, uint32_t stream_id, W &&write) {
	if (!ts) ts = new LiveTs();
	int rc = 0;
	char first_err[sizeof(g_err)] = "";
	live_ts_feed(*ts, bytes, n, stream_id, [&](double pts, const uint8_t *pes, uint32_t m) {
		if (write(pts, pes, m) < 0 && rc == 0) { rc = -1; memcpy(first_err, g_err, sizeof(g_err)); }
	});
	if (rc < 0) memcpy(g_err, first_err, sizeof(g_err));
	return rc;
}
