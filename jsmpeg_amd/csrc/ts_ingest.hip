/*
 * The device TS ingest of the two batch handles (ts_ingest.h): host code around the kernels of ts_kernels.hip.  Where the
 * packets lie -- sync bytes, resync after garbage, what a write() leaves over for the next (ts.js:25-50, 150-187) -- is found
 * by a host pre-pass (ts_sync.h); the packets' content is parsed on the device.
 */
#include "ts_ingest.h"

#include <algorithm>

#include "host_common.h"
#include "ts_sync.h"

int jm_ts_ingest_parse(JmTsIngest &t, uint32_t max_streams, uint32_t n_streams, const uint8_t *const *ts, const uint64_t *ts_bytes,
                       const uint32_t *n_writes, const uint64_t *write_bytes, uint32_t stream_id, std::vector<uint64_t> &es_len) {
	t.n_writes.clear(); t.parsed_n_writes.clear();
	es_len.clear();
	if (stream_id == 0 || stream_id > 255) return fail("stream id %u out of range", stream_id);
	if (n_streams == 0) return 0;     /* nothing to launch; the caller decides what an empty upload is */
	/* the packets of every stream (host pre-pass), then the layout of the TS scratch: the packets of a stream back to
	 * back from a 16-byte aligned start, 16 readable bytes behind each stream */
	std::vector<std::vector<JmTsRun>> runs(n_streams);
	std::vector<uint64_t> begin(n_streams), len(n_streams);
	std::vector<JmTsWriteEnd> ends;
	t.pkt_first.assign(n_streams + 1, 0);
	uint64_t off = 0;
	t.max_packets = 0;
	const uint64_t *wb = write_bytes;
	for (uint32_t i = 0; i < n_streams; i++) {
		const uint32_t nw = n_writes ? n_writes[i] : 0;
		/* with a write table, zero writes deliver nothing (bytes beyond the writes are never written); without one the
		 * whole buffer is one write */
		const uint64_t pk = n_writes && nw == 0 ? 0 : jm_ts_sync_runs(ts[i], ts_bytes[i], nw ? wb : nullptr, nw, runs[i], nullptr, &ends);
		if (n_writes) wb += nw;
		/* the kernels parse framed packets: refuse the input for which that is not what ts.js parses (ts_sync.h) */
		const int64_t bad = pk ? jm_ts_header_spill_differs(ts[i], runs[i], ends) : -1;
		if (bad >= 0) return fail("stream %u: TS packet %lld: a payload start reads past the packet's end, and what follows it in the written bytes is not the next packet", i, (long long)bad);
		begin[i] = off; len[i] = pk * 188;
		off += (len[i] + 16 + 15) & ~15ull;
		if (t.pkt_first[i] + pk > 0x3fffffffull) return fail("too many TS packets in one batch");
		t.pkt_first[i + 1] = t.pkt_first[i] + (uint32_t)pk;
		t.max_packets = std::max(t.max_packets, (uint32_t)pk);
	}
	const uint32_t n_packets = t.pkt_first[n_streams];
	if (off > t.ts_cap) {
		hipFree(t.d_ts); t.d_ts = nullptr; t.ts_cap = 0;
		HIP_TRY(jm_malloc(&t.d_ts, off));
		t.ts_cap = off;
	}
	if (n_packets > t.ts_pkt_cap) {
		hipFree(t.d_ts_rec); hipFree(t.d_ts_es_off); hipFree(t.d_ts_cand); hipFree(t.d_ts_writes);
		t.d_ts_rec = nullptr; t.d_ts_es_off = nullptr; t.d_ts_cand = nullptr; t.d_ts_writes = nullptr; t.ts_pkt_cap = 0;
		HIP_TRY(jm_malloc(&t.d_ts_rec, sizeof(JmTsRec) * (size_t)n_packets));
		HIP_TRY(jm_malloc(&t.d_ts_es_off, sizeof(uint32_t) * (size_t)n_packets));
		HIP_TRY(jm_malloc(&t.d_ts_cand, sizeof(JmTsCand) * (size_t)n_packets));
		HIP_TRY(jm_malloc(&t.d_ts_writes, sizeof(JmTsWrite) * 2 * (size_t)n_packets));
		t.ts_pkt_cap = n_packets;
	}
	const uint32_t ms = max_streams;
	if (!t.d_ts_begin) {
		HIP_TRY(jm_malloc(&t.d_ts_begin, sizeof(uint64_t) * ms));
		HIP_TRY(jm_malloc(&t.d_ts_len, sizeof(uint64_t) * ms));
		HIP_TRY(jm_malloc(&t.d_ts_small, sizeof(uint32_t) * (6 * (size_t)ms + 1)));
	}
	uint32_t *d_pkt_first = t.d_ts_small, *d_n_writes = d_pkt_first + ms + 1, *d_es_total = d_n_writes + ms,
	         *d_es_given = d_es_total + ms, *d_status = d_es_given + ms, *d_es_begin = d_status + ms;
	for (uint32_t i = 0; i < n_streams; i++) {
		uint64_t at = begin[i];
		for (const JmTsRun &r : runs[i]) {                      /* in sync from the first byte: one run, one copy */
			HIP_TRY(hipMemcpy(t.d_ts + at, ts[i] + r.src, 188ull * r.packets, hipMemcpyHostToDevice));
			at += 188ull * r.packets;
		}
	}
	HIP_TRY(hipMemcpy(t.d_ts_begin, begin.data(), sizeof(uint64_t) * n_streams, hipMemcpyHostToDevice));
	HIP_TRY(hipMemcpy(t.d_ts_len, len.data(), sizeof(uint64_t) * n_streams, hipMemcpyHostToDevice));
	HIP_TRY(hipMemcpy(d_pkt_first, t.pkt_first.data(), sizeof(uint32_t) * (n_streams + 1), hipMemcpyHostToDevice));
	HIP_TRY(hipDeviceSynchronize());
	JmTsBufs &tb = t.tb;
	tb.ts = t.d_ts; tb.ts_begin = t.d_ts_begin; tb.ts_len = t.d_ts_len; tb.pkt_first = d_pkt_first;
	tb.n_streams = n_streams; tb.stream_id = stream_id;
	tb.rec = t.d_ts_rec; tb.es_off = t.d_ts_es_off; tb.cand = t.d_ts_cand; tb.writes = t.d_ts_writes;
	tb.n_writes = d_n_writes; tb.es_total = d_es_total; tb.es_given = d_es_given; tb.status = d_status;
	tb.es = nullptr; tb.es_begin = d_es_begin;               /* the target: jm_ts_ingest_gather */
	HIP_TRY(jm_launch_ts_parse_walk(tb, t.max_packets, nullptr));
	std::vector<uint32_t> small(4 * (size_t)ms);
	HIP_TRY(hipMemcpy(small.data(), d_n_writes, sizeof(uint32_t) * 4 * (size_t)ms, hipMemcpyDeviceToHost));
	const uint32_t *h_n_writes = small.data(), *h_es_given = small.data() + 2 * ms, *h_status = small.data() + 3 * ms;
	es_len.resize(n_streams);
	for (uint32_t i = 0; i < n_streams; i++) {
		if (h_status[i] == 1) return fail("internal: stream %u: a framed TS packet does not start with the sync byte", i);
		if (h_status[i] == 3) return fail("stream %u: a PES / adaptation-field header runs past the end of its TS packet", i);
		if (h_status[i]) return fail("stream %u: more than 16 PIDs carry PES headers", i);
		es_len[i] = h_es_given[i];     /* what the destination received; a PES still open at the end of the input stays pending, like in ts.js */
	}
	t.parsed_n_writes.assign(h_n_writes, h_n_writes + n_streams);
	return 0;
}

int jm_ts_ingest_gather(JmTsIngest &t, uint8_t *es, const uint32_t *es_begin, uint32_t n_streams) {
	if (n_streams != t.tb.n_streams || n_streams != t.parsed_n_writes.size()) return fail("internal: TS gather without its parse");
	HIP_TRY(hipMemcpy(const_cast<uint32_t *>(t.tb.es_begin), es_begin, sizeof(uint32_t) * n_streams, hipMemcpyHostToDevice));
	HIP_TRY(hipDeviceSynchronize());
	t.tb.es = es;
	HIP_TRY(jm_launch_ts_gather(t.tb, t.max_packets, nullptr));
	t.n_writes.swap(t.parsed_n_writes);
	t.parsed_n_writes.clear();
	return 0;
}

int jm_ts_ingest_writes(const JmTsIngest &t, uint32_t stream, double *pts, uint32_t *offset, uint32_t *length, uint32_t cap) {
	if (stream >= t.n_writes.size()) return fail("no TS upload for stream %u", stream);
	const uint32_t n = t.n_writes[stream], k = std::min(n, cap);
	std::vector<JmTsWrite> w(k);
	if (k) HIP_TRY(hipMemcpy(w.data(), t.d_ts_writes + 2 * (size_t)t.pkt_first[stream], sizeof(JmTsWrite) * k, hipMemcpyDeviceToHost));
	for (uint32_t i = 0; i < k; i++) {
		if (pts) pts[i] = (double)(((uint64_t)w[i].pts_hi << 32) | w[i].pts_lo) / 90000.0;
		if (offset) offset[i] = w[i].begin;
		if (length) length[i] = w[i].length;
	}
	return (int)n;
}

void jm_ts_ingest_free(JmTsIngest &t) {
	hipFree(t.d_ts); hipFree(t.d_ts_rec); hipFree(t.d_ts_es_off); hipFree(t.d_ts_cand); hipFree(t.d_ts_writes);
	hipFree(t.d_ts_begin); hipFree(t.d_ts_len); hipFree(t.d_ts_small);
}
