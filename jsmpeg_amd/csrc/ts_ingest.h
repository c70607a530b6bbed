/*
 * The device TS ingest (reference src/ts.js:25-210) behind jsmpeg_hip_batch_upload_ts and jsmpeg_hip_mp2_batch_upload_ts:
 * n MPEG-TS buffers -> the bytes of one stream id, demultiplexed by k_ts_parse / k_ts_walk / k_ts_gather (ts_kernels.hip)
 * straight into the caller's buffer, and the destination.write list of each.  An upload is two calls around what only the
 * caller knows -- how the delivered bytes are laid out in its buffer:
 *     jm_ts_ingest_parse    framing (ts_sync.h), scratch, copies, k_ts_parse + k_ts_walk -> each stream's delivered length
 *     (the caller lays its buffer out and fills it)
 *     jm_ts_ingest_gather   the streams' starts in that buffer, k_ts_gather; commits the upload's write list
 * Both block on the null stream.  Not installed; nothing outside jsmpeg_amd/csrc includes it.
 */
#pragma once
#include <cstdint>
#include <vector>

#include "kernels.h"

struct JmTsIngest {
	uint8_t *d_ts = nullptr; uint64_t ts_cap = 0;      /* the packets of every stream; grows to the largest upload so far */
	JmTsRec *d_ts_rec = nullptr; uint32_t *d_ts_es_off = nullptr; JmTsCand *d_ts_cand = nullptr; JmTsWrite *d_ts_writes = nullptr;
	uint32_t ts_pkt_cap = 0;                           /* packets the four tables hold */
	uint64_t *d_ts_begin = nullptr, *d_ts_len = nullptr;   /* [max_streams] each */
	uint32_t *d_ts_small = nullptr;                    /* pkt_first[max_streams + 1] | n_writes | es_total | es_given | status | es_begin, [max_streams] each */
	std::vector<uint32_t> pkt_first;                   /* of the last parse */
	std::vector<uint32_t> n_writes;                    /* of the last upload that went through (jm_ts_ingest_writes); empty: none */
	std::vector<uint32_t> parsed_n_writes;             /* between parse and gather */
	JmTsBufs tb = {};
	uint32_t max_packets = 0;
};

/* ts[i], ts_bytes[i]: stream i's buffer, handed to the demuxer in the write() calls of n_writes[i] sizes taken in turn from
 * write_bytes (both null: one write each).  Forgets the last upload's write list, whatever comes of this one.  es_len[i]:
 * the bytes stream i's destination receives (n_streams == 0: nothing is launched).  max_streams: the handle's, at least 1
 * and the same in every call.  0 or < 0 */
int jm_ts_ingest_parse(JmTsIngest &t, uint32_t max_streams, uint32_t n_streams, const uint8_t *const *ts, const uint64_t *ts_bytes,
                       const uint32_t *n_writes, const uint64_t *write_bytes, uint32_t stream_id, std::vector<uint64_t> &es_len);
/* stream i's bytes to es + es_begin[i] (es: device, es_begin: host), for the streams of the parse before it */
int jm_ts_ingest_gather(JmTsIngest &t, uint8_t *es, const uint32_t *es_begin, uint32_t n_streams);
/* the body of the two *_ts_writes entry points (include/jsmpeg_hip.h) */
int jm_ts_ingest_writes(const JmTsIngest &t, uint32_t stream, double *pts, uint32_t *offset, uint32_t *length, uint32_t cap);
void jm_ts_ingest_free(JmTsIngest &t);
