/*
 * jsmpeg_hip -- C ABI of the MI355X (gfx950) MPEG-1 video decode path (parts 1, 2, 5) and of its MP2 audio
 * sibling (part 3); part 4: shards across the GPUs of a node.
 *
 * Drop-in boundary.  Part 1 is, symbol for symbol, the C ABI the reference
 * already defines for this path and that its JS wrapper binds through
 * WebAssembly exports (reference src/wasm/mpeg1.h:10-25, export list
 * build.sh:49-77, binding src/mpeg1-wasm.js:21-119).  A maintainer swaps
 * `module.instance.exports._mpeg1_decoder_*` for these (through the N-API
 * addon jsmpeg_amd/js/jsmpeg_hip.node) and nothing above
 * changes.  Part 2 is the additive batch interface (many streams x many
 * pictures per call, frames left in HBM) that the throughput numbers are
 * measured on; it has no reference counterpart.
 *
 * Plain pointers and sizes only; no torch / HIP types in any signature
 * (streams are passed as void*).  All functions are synchronous unless stated.
 * Nothing here falls back to a CPU decoder: without a usable HIP device
 * mpeg1_decoder_create / jsmpeg_hip_batch_create return NULL and
 * jsmpeg_hip_last_error() says why.
 */
#ifndef JSMPEG_HIP_H
#define JSMPEG_HIP_H

#include <stdbool.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------ part 1
 * The reference's decoder ABI (src/wasm/mpeg1.h:10-25).                    */

typedef struct mpeg1_decoder_t mpeg1_decoder_t;

/* reference src/wasm/buffer.h:8-11 */
typedef enum {
	BIT_BUFFER_MODE_EVICT = 1,
	BIT_BUFFER_MODE_EXPAND = 2
} bit_buffer_mode_t;

/* mpeg1.h:12 -- buffer_size = initial byte capacity of the compressed-data
 * store (JS option videoBufferSize), mode = streaming ? EVICT : EXPAND. */
mpeg1_decoder_t *mpeg1_decoder_create(unsigned int buffer_size, bit_buffer_mode_t buffer_mode);
/* mpeg1.h:13 */
void mpeg1_decoder_destroy(mpeg1_decoder_t *self);
/* mpeg1.h:14 -- host pointer to copy `byte_size` compressed bytes to; may
 * evict or grow the store first (buffer.c:48-65). */
void *mpeg1_decoder_get_write_ptr(mpeg1_decoder_t *self, unsigned int byte_size);
/* mpeg1.h:15-16 -- read cursor, in BITS from the start of the store. */
int mpeg1_decoder_get_index(mpeg1_decoder_t *self);
void mpeg1_decoder_set_index(mpeg1_decoder_t *self, unsigned int index);
/* mpeg1.h:17 -- commit bytes copied to the write pointer; parses the first
 * sequence header when it arrives (mpeg1.c:812-819). */
void mpeg1_decoder_did_write(mpeg1_decoder_t *self, unsigned int byte_size);
/* mpeg1.h:19-23 */
int mpeg1_decoder_has_sequence_header(mpeg1_decoder_t *self);
float mpeg1_decoder_get_frame_rate(mpeg1_decoder_t *self);
int mpeg1_decoder_get_coded_size(mpeg1_decoder_t *self);
int mpeg1_decoder_get_width(mpeg1_decoder_t *self);
int mpeg1_decoder_get_height(mpeg1_decoder_t *self);
/* mpeg1.h:24-26 -- HOST pointers to the most recently decoded picture's
 * coded-size planes (coded_size, coded_size/4, coded_size/4 bytes); valid
 * until the next decode (mpeg1.c:841-851). */
void *mpeg1_decoder_get_y_ptr(mpeg1_decoder_t *self);
void *mpeg1_decoder_get_cr_ptr(mpeg1_decoder_t *self);
void *mpeg1_decoder_get_cb_ptr(mpeg1_decoder_t *self);
/* mpeg1.h:27 -- decode exactly one picture; false = no complete picture
 * start code buffered (mpeg1.c:853-864).  The reference's signature has no
 * error channel; a HIP failure (allocation, device lost) is reported as
 * false + a non-empty jsmpeg_hip_last_error() -- the call clears the message
 * on entry, so "false and a message" always means THIS call failed; the cursor
 * is put back onto the picture's start code.  Callers must tell the two apart
 * (the N-API addon throws, jsmpeg_amd.cabi.Mpeg1Decoder.decode raises): a
 * failure must never read as "no more pictures". */
bool mpeg1_decoder_decode(mpeg1_decoder_t *self);

/* DECODE-AHEAD.  The reference decodes one picture per call; so does this function, as far as a caller can tell.  But
 * when several COMPLETE pictures are buffered behind the cursor (a file written in one piece, EXPAND mode; never the
 * streaming case of one picture written, one pulled) and the caller is pulling them one after the other (the first
 * picture after a write or a seek comes the plain way, at the plain latency), a call decodes up to 48 of them (as many as fit 160 MB of frames) in ONE pass of the batch engine
 * (part 2: all their slices parsed at once, the P chain reconstructed launch by launch, frames left in HBM) and the
 * following calls are served from those frames: planes, cursor (mpeg1_decoder_get_index) and plane rotation exactly as
 * if each call had decoded its picture.  A cursor that is not where the next such picture begins
 * (mpeg1_decoder_set_index: a seek) drops what is left; the last buffered picture (nothing behind it yet) is always
 * decoded the plain way.  Environment JSMPEG_HIP_DECODE_AHEAD = pictures per pass (0 / 1: off).
 * out[0] = passes of the batch engine so far, out[1] = pictures served from them. */
int jsmpeg_hip_decoder_ahead_stats(mpeg1_decoder_t *self, uint64_t out[2]);

/* Additive: DEVICE pointer to the most recently decoded frame (Y | Cr | Cb
 * contiguous, 1.5 * coded_size bytes), for consumers that stay on the GPU. */
void *jsmpeg_hip_decoder_get_device_frame(mpeg1_decoder_t *self);

/* Additive, renderer stage: the most recently decoded picture
 * as RGBA -- exactly the bytes the reference's Canvas2D renderer leaves in
 * imageData.data (src/canvas2d.js:48-122: integer BT.601 per 2x2 pixels,
 * display size width * height * 4, alpha 255; with an odd width the
 * reference's running indices shear the picture by a pixel per row pair and
 * leave unwritten pixels opaque white -- reproduced) -- converted on the
 * device, copied to `host_rgba`.
 * Returns 0 or < 0. */
int jsmpeg_hip_decoder_render_rgba(mpeg1_decoder_t *self, void *host_rgba);

/* ------------------------------------------------------------------ part 2
 * Batch decode: N elementary streams, every picture, planes stay in HBM.   */

typedef struct jsmpeg_hip_batch_t jsmpeg_hip_batch_t;

typedef struct jsmpeg_hip_batch_config_t {
	int32_t width, height;      /* display size every stream's sequence header must carry */
	uint32_t max_streams;
	uint32_t max_pictures;      /* frame pool = max_pictures frames of 1.5 * coded_size   */
	uint64_t max_es_bytes;      /* total compressed bytes per batch                        */
	int32_t device;             /* HIP device ordinal, -1 = current                        */
} jsmpeg_hip_batch_config_t;

typedef struct jsmpeg_hip_picture_info_t {
	uint32_t stream;            /* index of the stream in the batch           */
	uint32_t es_offset;         /* byte offset of the picture start code in that stream */
	int32_t type;               /* picture_coding_type: 1 = I, 2 = P          */
	int32_t decoded;            /* 0: skipped exactly where the reference skips (B/D, f_code 0, before the header) */
	int32_t level;              /* dependency depth inside its chain (the reconstruct order may put a picture
	                               with unwritten macroblocks deeper: counters[3]) */
	int32_t forward;            /* picture index of its forward reference, -1  */
	uint32_t n_slices;
} jsmpeg_hip_picture_info_t;

jsmpeg_hip_batch_t *jsmpeg_hip_batch_create(const jsmpeg_hip_batch_config_t *config);
void jsmpeg_hip_batch_destroy(jsmpeg_hip_batch_t *b);

/* Copies n_streams host elementary streams into the batch's HBM buffer
 * (streams are laid out back to back with a small gap).  Returns 0 or < 0. */
int jsmpeg_hip_batch_upload(jsmpeg_hip_batch_t *b, uint32_t n_streams, const uint8_t *const *es,
                            const uint64_t *es_bytes);
/* Same, from ONE packed DEVICE buffer (`begin[i]`, `end[i]` byte ranges; ranges
 * must not touch: leave >= 8 bytes between streams).  The bytes are copied
 * device-to-device on `hip_stream` (void* hipStream_t, NULL = default). */
int jsmpeg_hip_batch_upload_device(jsmpeg_hip_batch_t *b, const void *dev_es, uint64_t total_bytes,
                                   uint32_t n_streams, const uint32_t *begin, const uint32_t *end,
                                   void *hip_stream);
/* The same WITHOUT the copy: the next decode reads `dev_es` in place (a rank's piece as it arrived by
 * jsmpeg_hip_dist_scatter / _exchange, part 4: no placement pass in front of every step).  What the caller promises:
 * `dev_es` is 16-byte aligned and readable 256 bytes past `total_bytes`; every begin[i] is a multiple of 16, the first
 * one >= 16 (the buffer BEGINS with a gap), ranges ascend with >= 8 bytes between them, and every byte outside the
 * ranges (the leading gap, the gaps, the tail) is 0xff -- unchecked: a stale byte in a gap can complete a start code
 * and change the decode; the buffer stays valid and untouched for as long as it is attached: until the next upload*
 * / attach call (jsmpeg_hip_batch_read_es and the debug read-backs look at it too, not only the decode).
 * Returns at once (the stream table is copied on `hip_stream`); 0 or < 0 (misaligned / touching ranges are refused,
 * nothing is decoded from them).  The next upload* call returns the batch to its own buffer. */
int jsmpeg_hip_batch_attach_device(jsmpeg_hip_batch_t *b, const void *dev_es, uint64_t total_bytes,
                                   uint32_t n_streams, const uint32_t *begin, const uint32_t *end,
                                   void *hip_stream);

/* Ingest side on the device (reference src/ts.js:25-210): n_streams
 * MPEG-TS buffers (host) -> the elementary streams of `stream_id` (0xE0 = the
 * first video stream, ts.js:212-222), demultiplexed by GPU kernels straight into
 * the batch's HBM buffer.  Per stream the result equals feeding the buffer to one
 * JSMpeg.Demuxer.TS with that stream id connected, in one write(): the same
 * bytes, the same destination.write(pts, buffers) boundaries (completion by
 * PES_packet_length and by the stuffing guess, ts.js:127-147).  Input need not
 * be packet aligned: where ts.js resyncs (a byte that is not 0x47 is dropped,
 * the next sync byte with four more at 188-byte distances is taken, ts.js:43-50,
 * 150-187) so does this, and a trailing partial packet stays unread like
 * ts.js's leftover bytes.  Returns 0 or < 0. */
int jsmpeg_hip_batch_upload_ts(jsmpeg_hip_batch_t *b, uint32_t n_streams, const uint8_t *const *ts,
                               const uint64_t *ts_bytes, uint32_t stream_id);
/* The same with every buffer handed over in SEVERAL write() calls (ts.js:25-41: what a write cannot parse waits, as
 * leftover bytes, for the next): stream i is written in n_writes[i] calls whose sizes follow one another in
 * write_bytes (all streams' sizes back to back); bytes of a buffer beyond the sum of its sizes are never written.
 * Differs from one write only where a resync runs out of data at the end of a write. */
int jsmpeg_hip_batch_upload_ts_writes(jsmpeg_hip_batch_t *b, uint32_t n_streams, const uint8_t *const *ts,
                                      const uint64_t *ts_bytes, const uint32_t *n_writes, const uint64_t *write_bytes,
                                      uint32_t stream_id);
/* The packet framing of that alone (host code, no device): where the 188-byte packets lie that ts.js parses when
 * the buffer is handed to it in write() calls of write_bytes[0 .. n_writes) bytes (n_writes == 0: one write).  Fills
 * at most `cap` runs of consecutive packets (run_offset / run_packets, either may be NULL); returns the number of
 * runs or < 0; *n_packets: packets in all; *leftover_at: first byte ts.js still holds as leftover. */
int jsmpeg_hip_ts_packet_runs(const uint8_t *ts, uint64_t ts_bytes, const uint64_t *write_bytes, uint32_t n_writes,
                              uint64_t *run_offset, uint32_t *run_packets, uint32_t cap, uint64_t *n_packets,
                              uint64_t *leftover_at);
/* The destination.write calls of stream `stream` of the last upload_ts: pts in
 * seconds, byte range inside that stream's elementary stream.  Returns their
 * number (fills at most `cap` entries; any array may be NULL) or < 0.  An
 * upload_ts that was refused leaves no list: < 0 until the next one succeeds. */
int jsmpeg_hip_batch_ts_writes(jsmpeg_hip_batch_t *b, uint32_t stream, double *pts, uint32_t *offset,
                               uint32_t *length, uint32_t cap);
/* Device-to-host copy of one stream's resident elementary stream; returns its
 * size in bytes (copies at most `cap`) or < 0. */
int64_t jsmpeg_hip_batch_read_es(jsmpeg_hip_batch_t *b, uint32_t stream, void *out, uint64_t cap);

/* The hot path over the resident batch: start-code index -> tables -> slice
 * parse -> reconstruct, level by level.  Work is enqueued on `hip_stream`; the
 * call returns once everything is enqueued.  It waits for the device twice on
 * the way: after the index, to size the launches, and for the end of the slice
 * parse (the pictures without a forward reference are being reconstructed
 * meanwhile), whose report of unwritten macroblocks decides the order of the
 * remaining reconstruct launches.  Returns the number of pictures found or < 0. */
int jsmpeg_hip_batch_decode(jsmpeg_hip_batch_t *b, void *hip_stream);
/* Waits for the last decode (or enqueued pass, which it settles); returns 0 or < 0. */
int jsmpeg_hip_batch_sync(jsmpeg_hip_batch_t *b);
/* The same pass as a PURE ENQUEUE: start-code index -> a plan built on the device (the parse's sizing, `stale`, the ordered
 * reconstruct's sequence and descriptors) -> slice parse -> ONE ordered reconstruct launch, all on `hip_stream`, with no host
 * wait of any kind -- so one host thread keeps any number of batches in flight.  Returns 0: the
 * pass is enqueued; its results are there once jsmpeg_hip_batch_sync has settled it (every call below that reads results
 * settles it first: picture_count, picture_info, read_frame(s), frame_hashes, render_rgba*, counters, recon_info, timings,
 * level_timings, uncovered, stream_info).  sync reports what decode reports -- a table overflow with decode's message --, redoes
 * a flagged ordered launch level by level, checks GOP chains, and reconstructs a pass the device could not order (one long
 * stream, badly ragged chains: recon_info status 8) level by level there.  Returns 1: the batch cannot be planned on the
 * device -- linked or seeded streams, live handles, a batch set to go level by level (set_reconstruct(0),
 * JSMPEG_HIP_RECON_ORDER=0, or demoted by a flagged ordered launch) -- and jsmpeg_hip_batch_decode ran instead, with the same
 * results.  < 0: an argument error.  While an enqueued pass is not settled, upload*, attach_device, link_streams, seed_stream,
 * decode and enqueue on the batch FAIL ("... in flight: call jsmpeg_hip_batch_sync first"); nothing waits behind the caller's
 * back.  The device plans ONE ordered launch for every batch it can order -- also for the batches decode's engine sends level
 * by level (all-intra and dense-intra batches, wide shallow ones: 1-3 % faster per level one batch at a time); a host that wants
 * those per-level launches calls decode (set_reconstruct(0) makes enqueue do so).  timings[1] of an enqueued pass is 0; of a
 * pass reconstructed at sync (status 8), timings[3] is the level launches' span. */
int jsmpeg_hip_batch_enqueue(jsmpeg_hip_batch_t *b, void *hip_stream);
/* 1 if the last pass's work on the device has finished (or there is none), 0 if not; never blocks, never settles (a host
 * without threads polls this, then calls jsmpeg_hip_batch_sync).  < 0 on error. */
int jsmpeg_hip_batch_query(jsmpeg_hip_batch_t *b);
/* A HIP stream of the batch's own (created on first use, destroyed with the batch) to pass as `hip_stream`, for hosts that link
 * no HIP runtime to make one with (the N-API addon's decodeAsync): two batches in flight need a
 * stream EACH -- on the null stream their passes run one behind the other.  Returns it, or NULL (jsmpeg_hip_last_error). */
void *jsmpeg_hip_batch_own_stream(jsmpeg_hip_batch_t *b);
/* The reconstruct's plan for this batch's passes: 0 = always one launch per dependency level, 1 = the setting the batch was
 * created with (the default: the engine's choice -- level by level for dense intra pictures and for WIDE batches, from 2.5 M
 * macroblocks per level, where both plans take the same time; ONE dependency-ordered launch for everything narrower or shorter,
 * 1-12 % faster there --, or what JSMPEG_HIP_RECON_ORDER said when the batch was created).  A batch whose ordered launch once
 * flagged itself stays level by level under either setting.  One batch at a time the choice is the faster or equal everywhere;
 * a host that keeps two batches in flight sets 0 also on narrower batches: short launches share the GPU better with the other
 * batch's parse (+5 % on the 64 x 1080p workload, +24 % on coded video).  Returns 0 or < 0. */
int jsmpeg_hip_batch_set_reconstruct(jsmpeg_hip_batch_t *b, int plan);

uint32_t jsmpeg_hip_batch_picture_count(jsmpeg_hip_batch_t *b);
int jsmpeg_hip_batch_picture_info(jsmpeg_hip_batch_t *b, uint32_t picture, jsmpeg_hip_picture_info_t *out);
/* What stream `stream`'s FIRST sequence header said, as the last decode read it (mpeg1.c:872-944; any pointer may be NULL):
 * display size and mpeg1_decoder_get_frame_rate's value (the decoder's clock advances by 1 / frame_rate per picture,
 * mpeg1.js:57).  Returns 1, 0 if the stream had no sequence header, or < 0. */
int jsmpeg_hip_batch_stream_info(jsmpeg_hip_batch_t *b, uint32_t stream, int32_t *width, int32_t *height, float *frame_rate);
/* Geometry of a frame in the pool: Y at 0, Cr at luma_bytes, Cb at
 * luma_bytes + chroma_bytes; frame p at pool + p * frame_stride. */
int jsmpeg_hip_batch_geometry(jsmpeg_hip_batch_t *b, int32_t *coded_width, int32_t *coded_height,
                              uint32_t *luma_bytes, uint32_t *chroma_bytes, uint64_t *frame_stride);
/* Device pointer of the pool.  The frames are FINAL only after jsmpeg_hip_batch_sync (or any call of this header that
 * reads pictures back: read_frame, frame_hashes, render_rgba*, read_rgba*, uncovered, counters): the dependency-ordered
 * reconstruct launch is provisional until its status words have been looked at -- a launch that flagged itself is done
 * over level by level inside that call.  A consumer that reads the pool from its own kernels on the decode stream
 * calls jsmpeg_hip_batch_sync first. */
void *jsmpeg_hip_batch_frame_pool(jsmpeg_hip_batch_t *b);
/* Device-to-host copy of one picture's planes (any of y/cr/cb may be NULL). */
int jsmpeg_hip_batch_read_frame(jsmpeg_hip_batch_t *b, uint32_t picture, void *y, void *cr, void *cb);
/* Pictures first .. first + count - 1 in one go: picture first + k's planes (Y | Cr | Cb, luma_bytes + 2 * chroma_bytes contiguous
 * bytes) at host + k * stride -- one strided copy, at the link's rate when `host` is pinned (jsmpeg_hip_host_alloc /
 * jsmpeg_hip_host_register, part 5): 49 GB/s against 27 picture by picture into pageable memory.  Pictures that were not
 * decoded (jsmpeg_hip_batch_picture: decoded 0) are copied like the others; what they hold is undefined. */
int jsmpeg_hip_batch_read_frames(jsmpeg_hip_batch_t *b, uint32_t first, uint32_t count, void *host, uint64_t stride);
/* 64-bit content hash of every picture's planes, computed on the device
 * (jsmpeg_amd/hashing.py gives the same value for host planes). out[picture_count]. */
int jsmpeg_hip_batch_frame_hashes(jsmpeg_hip_batch_t *b, uint64_t *out);
/* Renderer stage (src/canvas2d.js:53-122) for pictures [first_picture,
 * first_picture + count): RGBA frames of width * height * 4 bytes, packed one
 * after the other into the DEVICE buffer `dev_rgba`, enqueued on `hip_stream`. */
int jsmpeg_hip_batch_render_rgba(jsmpeg_hip_batch_t *b, uint32_t first_picture, uint32_t count,
                                 void *dev_rgba, void *hip_stream);
/* Same conversion for ONE picture, copied to host memory (width * height * 4 bytes). */
int jsmpeg_hip_batch_read_rgba(jsmpeg_hip_batch_t *b, uint32_t picture, void *host_rgba);
/* The reference's OTHER renderer form, WebGL (src/webgl.js:259-281): chroma sampled bilinearly from the
 * half-size planes (GL_LINEAR, CLAMP_TO_EDGE, weights 0.75 / 0.25), (y, cr, cb, 1) times the shader's BT.601 matrix in
 * float32, framebuffer conversion round(c * 255), alpha 255; display size, rows packed.  A browser's result depends on its
 * GPU's shader precision and filter hardware, so this form carries a tolerance (1 LSB against the float64 restatement),
 * not the bit-exact contract of the Canvas2D form above. */
int jsmpeg_hip_batch_render_rgba_gl(jsmpeg_hip_batch_t *b, uint32_t first_picture, uint32_t count,
                                    void *dev_rgba, void *hip_stream);
int jsmpeg_hip_batch_read_rgba_gl(jsmpeg_hip_batch_t *b, uint32_t picture, void *host_rgba);
/* hipEvent timings of the last decode, milliseconds: [0] start-code index +
 * tables, [1] host table turn-around, [2] slice parse, [3] reconstruct,
 * [4] total.  Valid after jsmpeg_hip_batch_sync. */
int jsmpeg_hip_batch_timings(jsmpeg_hip_batch_t *b, float out_ms[5]);
/* hipEvent timings of the reconstruct launches of the last decode, one per dependency level in launch order ([0]: the
 * pictures without a forward reference), milliseconds; at most `cap` (and at most 64) are written.  Returns the
 * number written or < 0.  Valid after jsmpeg_hip_batch_sync.  An ordered launch (jsmpeg_hip_batch_recon_info) is ONE entry. */
int jsmpeg_hip_batch_level_timings(jsmpeg_hip_batch_t *b, float *out_ms, uint32_t cap);
/* Counters of the last decode: [0] start codes, [1] pictures, [2] decoded
 * pictures, [3] dependency levels, [4] slices parsed, [5] macroblocks per picture,
 * [6] pictures with macroblocks the stream never writes (they keep the decoded
 * picture before last, see part 4), [7] slice start codes found (01 .. AF; [4] counts the ones a picture owns). */
int jsmpeg_hip_batch_counters(jsmpeg_hip_batch_t *b, uint64_t out[8]);
/* How the last decode reconstructed (waits for the stream): [0] reconstruct launches -- 1: the ORDERED launch (one launch
 * for the whole batch: every eighth of the GPU walks its streams -- or, in a narrow batch, its GOP chains -- in lockstep and
 * a picture's tiles wait for its forward reference; batches that fill eight classes evenly), else one launch per dependency
 * level; [1] streams a class walks in lockstep (0: level by level; environment JSMPEG_HIP_RECON_ORDER = 0 / n);
 * [2] waits of the ordered launch that found their picture unfinished at the first look; [3] its status (0: clean;
 * 1 / 2: the launch flagged itself -- a wait ran out of patience / a class ran on two XCDs --, the frames were
 * reconstructed a second time level by level before jsmpeg_hip_batch_sync returned, and the batch stays with per-level
 * launches; 4: a NARROW batch (fewer than eight streams: the classes walk GOP chains instead of streams, on the
 * assumption that a chain's first two pictures write every macroblock) whose assumption did not hold for this input:
 * done over level by level, this decode only).  Frames of an ordered launch are final
 * once jsmpeg_hip_batch_sync (or any call that reads them back) has returned. */
int jsmpeg_hip_batch_recon_info(jsmpeg_hip_batch_t *b, uint32_t out[4]);
/* Streams that CONTINUE other streams (part 4: the units a sharded job cuts its streams into).  prev[s] >= 0: stream s
 * of the uploaded batch goes on where stream prev[s] (< s) ended -- its unwritten macroblocks show that stream's last
 * pictures (the reference's plane rotation, mpeg1.c:986-994) instead of zeros; -1: a stream of its own.  `n` = the
 * uploaded streams; prev == NULL clears.  Every upload* / attach call clears links and seeds: set them after it. */
int jsmpeg_hip_batch_link_streams(jsmpeg_hip_batch_t *b, const int32_t *prev, uint32_t n);
/* ... and a stream whose predecessor was decoded ELSEWHERE (another rank, an earlier batch): the frames (Y | Cr | Cb,
 * jsmpeg_hip_batch_geometry's layout, device memory, complete before the decode starts and left alone until it has
 * finished) of the decoded picture last / before last in front of the stream; either may be NULL (zeros). */
int jsmpeg_hip_batch_seed_stream(jsmpeg_hip_batch_t *b, uint32_t stream, const void *dev_frame_last, const void *dev_frame_before_last);
/* out[p] = 1 where picture p of the last decode was decoded and left macroblocks unwritten (they show the stream's
 * decoded picture before last); at most `cap` entries; waits for the decode.  Returns the entries written or < 0. */
int jsmpeg_hip_batch_uncovered(jsmpeg_hip_batch_t *b, uint8_t *out, uint32_t cap);
/* SELECTED FRAMES ONLY: a few frames per stream (one per second for an indexing job, one for a thumbnail, the frame at a
 * time for a seek) without decoding the rest.  Request k asks for frame frame[k] of stream stream[k]; frames are counted
 * as a user of the reference counts them: the n-th picture the whole decode would decode (picture_info.decoded == 1), in
 * stream order, from 0.  Repeats and any order are allowed; count == 0 or NULL arrays clear the selection.  Like links
 * and seeds, every upload* / attach_device clears it: set it after the upload; it then holds for every decode / enqueue of
 * that upload.  The passes parse and reconstruct the selection's CLOSURE over forward references only -- the pictures from
 * each selected picture's intra picture (or the stream's first decoded picture) up to it --, worked out on the device
 * behind the index (enqueue stays a pure enqueue).  After such a pass
 *   - a picture that was not needed reads decoded == 0 in picture_info, its frame in the pool is not written, and
 *     render_tensor / render_rgba* refuse it as they refuse every picture that was not decoded;
 *   - picture_count, the picture indices, es_offset, type and the pool slots are exactly the whole decode's;
 *   - counters [2] and [4] count the needed pictures and their slices.
 * Exact, never approximate: a needed picture that leaves macroblocks UNWRITTEN shows its stream's decoded picture before
 * last there, which for a GOP's first two pictures lies in the GOP in front -- maybe outside the closure.  Once the parse's
 * counts are in, a stream with such a picture has its selection WIDENED to every frame from its beginning up to its last
 * needed one, and the pass is run once more before jsmpeg_hip_batch_sync (or any reader) returns -- the contract of
 * recon_info's status 4; the widening stays for the following passes of that upload (select_info says so).
 * Fails for a stream index >= the uploaded streams, for a live handle's batch, and -- with the uploads' message -- while
 * an enqueued pass is unsettled.  A pass (decode / enqueue) of a batch that has both a selection and linked or seeded
 * streams is refused. */
int jsmpeg_hip_batch_select(jsmpeg_hip_batch_t *b, const uint32_t *stream, const uint32_t *frame, uint32_t count);
/* picture[k] = the picture index of request k in the last pass, 0xffffffff where the stream has no such frame; at most
 * `cap` entries; settles the pass first, like every reader.  Returns the entries written (0: no selection) or < 0. */
int jsmpeg_hip_batch_selected(jsmpeg_hip_batch_t *b, uint32_t *picture, uint32_t cap);
/* The last selected pass: [0] selected pictures (distinct), [1] needed pictures (the closure: what was parsed and
 * reconstructed), [2] streams whose selection has been widened, [3] 1 if this pass was done over because of that. */
int jsmpeg_hip_batch_select_info(jsmpeg_hip_batch_t *b, uint64_t out[4]);

/* ------------------------------------------------------------------ part 3
 * MP2 audio (MPEG-1 Audio Layer II) -- the sibling decoder of the reference's
 * wasm module.  First, symbol for symbol, the C ABI the
 * reference defines for it (src/wasm/mp2.h:10-20, export list build.sh:68-77,
 * binding src/mp2-wasm.js:21-104).  PCM is bit-identical to the reference's C /
 * shipped wasm build (binary32, see jsmpeg_amd/csrc/mp2_dev.h for the
 * arithmetic contract; the reference's pure-JS decoder rounds differently and
 * agrees to ~5e-7 of full scale).                                            */

typedef struct mp2_decoder_t mp2_decoder_t;

/* mp2.h:10 -- buffer_size = initial byte capacity (JS option audioBufferSize) */
mp2_decoder_t *mp2_decoder_create(unsigned int buffer_size, bit_buffer_mode_t buffer_mode);
/* mp2.h:11 */
void mp2_decoder_destroy(mp2_decoder_t *self);
/* mp2.h:12-15 -- as for the video decoder */
void *mp2_decoder_get_write_ptr(mp2_decoder_t *self, unsigned int byte_size);
int mp2_decoder_get_index(mp2_decoder_t *self);
void mp2_decoder_set_index(mp2_decoder_t *self, unsigned int index);
void mp2_decoder_did_write(mp2_decoder_t *self, unsigned int byte_size);
/* mp2.h:17-18 -- HOST pointers to the 1152 float samples per channel of the
 * most recently decoded frame; valid until the next decode. */
void *mp2_decoder_get_left_channel_ptr(mp2_decoder_t *self);
void *mp2_decoder_get_right_channel_ptr(mp2_decoder_t *self);
/* mp2.h:19 -- of the most recently decoded frame; 44100 before the first */
int mp2_decoder_get_sample_rate(mp2_decoder_t *self);
/* mp2.h:20 -- decodes the frame at the cursor; returns its length in bytes,
 * 0 if fewer than 16 bits are buffered or the header is not MPEG-1 Layer II
 * with a valid bit rate / sampling frequency (mp2.c:275-302); the cursor then
 * stays where it was.  Frames must be completely buffered (the reference never
 * checks and decodes stale bytes; here the missing bytes read as 0). */
int mp2_decoder_decode(mp2_decoder_t *self);

/* Additive batch interface: N MP2 streams, every frame, PCM left in HBM. */
typedef struct jsmpeg_hip_mp2_batch_t jsmpeg_hip_mp2_batch_t;

/* max_bytes: total compressed bytes per batch (<= 256 MiB). device: HIP ordinal, -1 = current. */
jsmpeg_hip_mp2_batch_t *jsmpeg_hip_mp2_batch_create(uint32_t max_streams, uint64_t max_bytes, int32_t device);
void jsmpeg_hip_mp2_batch_destroy(jsmpeg_hip_mp2_batch_t *b);
/* Copies n_streams host buffers of back-to-back Layer II frames into HBM.  Returns 0 or < 0. */
int jsmpeg_hip_mp2_batch_upload(jsmpeg_hip_mp2_batch_t *b, uint32_t n_streams, const uint8_t *const *data,
                                const uint64_t *bytes);
/* Same, from ONE packed DEVICE buffer (`begin[i]`, `end[i]` byte ranges inside it) -- what a rank holds after the
 * RCCL scatter of its shard.  Copied device-to-device on `hip_stream` (void* hipStream_t, NULL = the batch's own). */
int jsmpeg_hip_mp2_batch_upload_device(jsmpeg_hip_mp2_batch_t *b, const void *dev_bytes, uint64_t total_bytes,
                                       uint32_t n_streams, const uint32_t *begin, const uint32_t *end, void *hip_stream);
/* Ingest side on the device (reference src/ts.js:25-210), the audio twin of
 * jsmpeg_hip_batch_upload_ts: n_streams MPEG-TS buffers (host) -> the payload of `stream_id` (0xC0 = the first
 * audio stream, ts.js:212-222), demultiplexed by the same GPU kernels straight into the batch's HBM buffer; per
 * stream the same bytes and the same destination.write(pts, buffers) boundaries as one JSMpeg.Demuxer.TS fed the
 * buffer in one write() (resync and leftover bytes like ts.js).  The same TS buffers can be handed to both batches
 * (video with 0xE0, audio with 0xC0).  Returns 0 or < 0. */
int jsmpeg_hip_mp2_batch_upload_ts(jsmpeg_hip_mp2_batch_t *b, uint32_t n_streams, const uint8_t *const *ts,
                                   const uint64_t *ts_bytes, uint32_t stream_id);
/* The destination.write calls of stream `stream` of the last upload_ts: pts in seconds, byte range inside that
 * stream's MP2 bytes.  Returns their number (fills at most `cap` entries; any array may be NULL) or < 0.  An upload_ts
 * that was refused leaves no list: < 0 until the next one succeeds. */
int jsmpeg_hip_mp2_batch_ts_writes(jsmpeg_hip_mp2_batch_t *b, uint32_t stream, double *pts, uint32_t *offset,
                                   uint32_t *length, uint32_t cap);
/* Device-to-host copy of one stream's resident MP2 bytes; returns their number (copies at most `cap`) or < 0. */
int64_t jsmpeg_hip_mp2_batch_read_bytes(jsmpeg_hip_mp2_batch_t *b, uint32_t stream, void *out, uint64_t cap);
/* Decodes every frame of every stream -- per stream what `while (mp2_decoder_decode(d));` after one write of the
 * whole buffer gives, except that a last frame that is not completely there is not decoded.  Work is enqueued on
 * `hip_stream` (NULL = the batch's own); the call synchronises once internally (frame counts size the launches).
 * Returns the total number of frames or < 0. */
int jsmpeg_hip_mp2_batch_decode(jsmpeg_hip_mp2_batch_t *b, void *hip_stream);
int jsmpeg_hip_mp2_batch_sync(jsmpeg_hip_mp2_batch_t *b);
/* Frames of one stream, or of the whole batch with stream = -1. */
uint32_t jsmpeg_hip_mp2_batch_frame_count(jsmpeg_hip_mp2_batch_t *b, int32_t stream);
/* Where a frame starts in its stream, its length and sampling frequency (any pointer may be NULL). */
int jsmpeg_hip_mp2_batch_frame_info(jsmpeg_hip_mp2_batch_t *b, uint32_t stream, uint32_t frame,
                                    uint32_t *byte_offset, uint32_t *byte_size, int32_t *sample_rate);
/* DEVICE pointer: float[total frames][2][1152] (left, right), streams one after the other in upload order. */
void *jsmpeg_hip_mp2_batch_pcm(jsmpeg_hip_mp2_batch_t *b);
/* Device-to-host copy of `count` frames of one stream: out[count][2][1152]. */
int jsmpeg_hip_mp2_batch_read_pcm(jsmpeg_hip_mp2_batch_t *b, uint32_t stream, uint32_t first_frame, uint32_t count,
                                  float *out);
/* hipEvent timings of the last decode, milliseconds: [0] frame walk + count read-back, [1] host turn-around +
 * side information, [2] sample read + matrixing, [3] windowing, [4] total. */
int jsmpeg_hip_mp2_batch_timings(jsmpeg_hip_mp2_batch_t *b, float out_ms[5]);

/* ------------------------------------------------------------------ part 4
 * (stream, GOP) shards across the GPUs of one node (additive: the reference is one single-threaded
 * decoder, its nearest relative is the relay that fans a stream out, websocket-relay.js:42-48).  Closed GOPs decode
 * independently -- an I picture is all intra, there are no B pictures, a P picture references the picture before it
 * -- so the one exchange step of the path moves compressed bytes: the rank that holds the streams sends every rank
 * the units it owns (RCCL over xGMI), each rank decodes its piece with its own jsmpeg_hip_batch_t as that many
 * independent streams.
 * ONE THING CROSSES A CUT, and the results are bit-exact to the unsplit stream all the same: the reference rotates two
 * plane sets (mpeg1.c:986-994), so a macroblock a picture never writes keeps showing the decoded picture BEFORE LAST --
 * for the first two pictures of a unit that is a picture of the GOP before.  A unit therefore CONTINUES its
 * predecessor: in the same batch by jsmpeg_hip_batch_link_streams (costs nothing: a pointer per picture, and a
 * dependency only for a picture that really has such a macroblock); across ranks or batches by
 * jsmpeg_hip_batch_seed_stream with the predecessor's last two frames -- needed only when
 * jsmpeg_hip_batch_uncovered() says one of the unit's first two decoded pictures has such macroblocks (none in the
 * benchmark's content, ~1 picture in 8 with coherent motion).  jsmpeg_hip_plan_contiguous keeps a stream's units on one
 * rank wherever the balance allows: at most world - 1 cuts of the whole job cross ranks.  jsmpeg_amd/distributed.py
 * (resolve_history) is the procedure: decode, ask, ship 2 frames per needy cross-rank cut, decode those ranks again. */

typedef struct jsmpeg_hip_gop_unit_t {
	uint64_t offset, bytes;     /* byte range of the unit in the elementary stream */
	uint32_t pictures;          /* picture start codes inside it */
	uint32_t needs_header;      /* 1: the stream's first sequence header must go in front (only the first one counts for
	                               the reference, mpeg1.js:32; a unit's own later header may differ and is ignored) */
} jsmpeg_hip_gop_unit_t;

/* Cuts one elementary stream (HOST memory) at its I pictures -- in front of the sequence / GOP headers glued to each.
 * Returns the number of units (fills at most `cap`), >= 1; *header_offset / *header_bytes: the stream's first sequence
 * header (0 / 0 if it has none: the stream is then one unit). */
int jsmpeg_hip_split_gops(const uint8_t *es, uint64_t es_bytes, jsmpeg_hip_gop_unit_t *units, uint32_t cap,
                          uint64_t *header_offset, uint64_t *header_bytes);
/* Balanced assignment of n units (weights = compressed bytes) to `world` ranks: owner[i] = rank of unit i. */
int jsmpeg_hip_plan_shards(const uint64_t *weights, uint32_t n, uint32_t world, uint32_t *owner);
/* The same as CONTIGUOUS ranges of the unit list (units in job order: stream after stream, GOP after GOP): rank r takes
 * the units whose middle byte falls into the r-th of `world` equal shares of the job's bytes -- balanced to within one
 * unit, and consecutive units of a stream stay together except at the <= world - 1 range boundaries. */
int jsmpeg_hip_plan_contiguous(const uint64_t *weights, uint32_t n, uint32_t world, uint32_t *owner);
/* The same for units that ARRIVED on the ranks (every rank ingests its own streams; home[i] = the rank that holds unit
 * i): a unit stays where it is unless moving it from the most to the least loaded rank narrows the gap between the
 * two -- about half the imbalance travels, a balanced job moves nothing. */
int jsmpeg_hip_plan_rebalance(const uint64_t *weights, const uint32_t *home, uint32_t n, uint32_t world, uint32_t *owner);

/* One RCCL communicator over the ranks of a job (one process per GPU).  The 128-byte id is made on one rank
 * (jsmpeg_hip_dist_unique_id) and handed to the others by whatever launched them (torch.distributed, MPI, a file). */
typedef struct jsmpeg_hip_dist_t jsmpeg_hip_dist_t;
#define JSMPEG_HIP_DIST_ID_BYTES 128
int jsmpeg_hip_dist_unique_id(void *id);
jsmpeg_hip_dist_t *jsmpeg_hip_dist_create(int32_t rank, int32_t world, const void *id, int32_t device);   /* device: HIP ordinal, -1 = current */
void jsmpeg_hip_dist_destroy(jsmpeg_hip_dist_t *d);
int32_t jsmpeg_hip_dist_rank(jsmpeg_hip_dist_t *d);
int32_t jsmpeg_hip_dist_world(jsmpeg_hip_dist_t *d);
/* The exchange step: piece r (offset[r], bytes[r]; the same arrays on every rank) of the packed DEVICE buffer
 * `src_dev` on rank `src_rank` lands in rank r's DEVICE buffer `dst_dev`.  Grouped sends: the source's xGMI links
 * carry their pieces at once.  Enqueued on `hip_stream` (void* hipStream_t).  Returns 0 or < 0. */
int jsmpeg_hip_dist_scatter(jsmpeg_hip_dist_t *d, int32_t src_rank, const void *src_dev, const uint64_t *offset,
                            const uint64_t *bytes, void *dst_dev, void *hip_stream);
/* The exchange step when every rank holds units (jsmpeg_hip_plan_rebalance): rank to rank, only what the plan moved.
 * To rank r go send_bytes[r] bytes from src_dev + send_offset[r]; from rank r come recv_bytes[r] bytes to dst_dev +
 * recv_offset[r] (THIS rank's arrays of `world` entries; its own entry is a device copy).  One group of sends and
 * receives.  Enqueued on `hip_stream`.  Returns 0 or < 0. */
int jsmpeg_hip_dist_exchange(jsmpeg_hip_dist_t *d, const void *src_dev, const uint64_t *send_offset, const uint64_t *send_bytes,
                             void *dst_dev, const uint64_t *recv_offset, const uint64_t *recv_bytes, void *hip_stream);
/* PLAN-TIME check of an exchange (call it once per plan, on every rank, before the first jsmpeg_hip_dist_exchange with
 * these tables): the ranks' send_bytes / recv_bytes tables are all-gathered over the communicator and every pair is
 * compared -- what rank a sends to rank r must be what r expects from a.  A plan that fails is refused ON EVERY RANK
 * (< 0, jsmpeg_hip_last_error names the pairs): enqueued, its receive would never complete and the job would hang.
 * Synchronises `hip_stream`.  Returns 0 or < 0. */
int jsmpeg_hip_dist_check_exchange(jsmpeg_hip_dist_t *d, const uint64_t *send_bytes, const uint64_t *recv_bytes, void *hip_stream);
/* The reverse (set-up: streams that arrived on several ranks are collected where they are distributed from). */
int jsmpeg_hip_dist_gather(jsmpeg_hip_dist_t *d, int32_t dst_rank, const void *src_dev, const uint64_t *offset,
                           const uint64_t *bytes, void *dst_dev, void *hip_stream);
/* `bytes_per_rank` bytes from every rank to every rank (reporting: the 8-byte plane hashes). */
int jsmpeg_hip_dist_allgather(jsmpeg_hip_dist_t *d, const void *src_dev, void *dst_dev, uint64_t bytes_per_rank,
                              void *hip_stream);

/* Device buffers for hosts that bring no tensor library (the Node host, jsmpeg_amd/js/shard-hip.js; a Python host hands the
 * calls above torch tensors' addresses): plain allocations and synchronous copies on the default stream -- the buffers the
 * exchange steps read and write, nothing of the decode path.  fill: a byte value (0xff for buffers that will hold packed
 * units: the gaps between units must not complete a start code), < 0: uninitialised.  device: HIP ordinal, -1 = current. */
void *jsmpeg_hip_device_alloc(uint64_t bytes, int32_t device, int32_t fill);
void jsmpeg_hip_device_free(void *p);
int jsmpeg_hip_device_write(void *dst, const void *host, uint64_t n);
int jsmpeg_hip_device_read(void *host, const void *src, uint64_t n);
int jsmpeg_hip_device_copy(void *dst, const void *src, uint64_t n);
int jsmpeg_hip_device_fill(void *dst, int32_t byte, uint64_t n);
int jsmpeg_hip_device_synchronize(void);

/* ------------------------------------------------------------------ part 5
 * LIVE streams: N streams that GO ON (jsmpeg's main use: MPEG-TS over a WebSocket, reference src/player.js:222-228
 * updateForStreaming -- "decode what has arrived", every tick; src/ts.js:205-210 hands a decoder one PES = one picture
 * per write(pts, buffers); src/buffer.js:64-104 the EVICT store; src/wasm/mpeg1.c:986-994 the two plane sets that carry
 * from picture to picture).  Part 2 decodes whole streams from nothing; here a stream persists across calls: its
 * undecoded bytes, its FIRST sequence header (only the first one counts, mpeg1.c:812-819) and the frames of its last two
 * decoded pictures stay in HBM, and one jsmpeg_hip_live_tick decodes the pending pictures of EVERY stream in ONE pass
 * of the batch engine (all their slices parsed at once, one reconstruct launch) -- per stream exactly the pictures the
 * reference's decoder gives for the same write() calls (held against it with the same writes and ticks, evictions
 * included: tools/fuzz_live.py).  Nothing is copied twice on the way: a write() lands in a pinned staging buffer, which goes
 * to the device a MiB at a time beside the host's next writes (what is left of it with the tick); a picture is reconstructed
 * into its stream's ring of frames, and the next tick predicts from those frames where they lie.  A handle is one
 * thread's at a time (like a decoder of the reference: single-threaded JS); handles are independent of each other.
 * Device memory: per stream (max_pictures_per_tick + 2) frames, 11 x store_bytes, ~0.2 MB of records per picture and tick
 * -- 25 MB per 1080p stream at the defaults, 15 MB with one picture per tick.
 *
 *     id = jsmpeg_hip_live_open(l);                                   a stream joins (any time)
 *     jsmpeg_hip_live_write(l, id, pts, bytes, n);                    == video.write(pts, [bytes])   (ts.js:205-210)
 *     n = jsmpeg_hip_live_tick(l, JSMPEG_HIP_LIVE_FLUSH, NULL);       == for every stream: while (video.decode()) ;
 *     for (i < n) jsmpeg_hip_live_picture(l, i, &pic);                pic.device_frame: Y | Cr | Cb in HBM
 */

typedef struct jsmpeg_hip_live_t jsmpeg_hip_live_t;

typedef struct jsmpeg_hip_live_config_t {
	int32_t width, height;            /* display size every stream's sequence header must carry */
	uint32_t max_streams;             /* streams open at a time */
	uint32_t max_pictures_per_tick;   /* per stream: a tick decodes at most this many picture start codes of a stream, the rest
	                                     wait for the next tick (0: 4).  A stream's ring holds this many frames + 2. */
	uint32_t store_bytes;             /* capacity of a stream's compressed-data store = the reference's videoBufferSize
	                                     (0: 512 KiB, mpeg1-wasm.js:9), with its EVICT rule: see jsmpeg_hip_live_write */
	int32_t device;                   /* HIP device ordinal, -1 = current */
} jsmpeg_hip_live_config_t;

typedef struct jsmpeg_hip_live_picture_t {
	uint32_t stream;                  /* id from jsmpeg_hip_live_open */
	int32_t type;                     /* picture_coding_type: 1 = I, 2 = P */
	double pts;                       /* of the write() in which the picture's start code arrived */
	uint64_t stream_offset;           /* byte offset of that start code in everything ever written to the stream */
	void *device_frame;               /* DEVICE pointer: Y | Cr | Cb (jsmpeg_hip_live_geometry's sizes); valid until the next tick */
} jsmpeg_hip_live_picture_t;

typedef struct jsmpeg_hip_live_stream_info_t {
	int32_t has_sequence_header;      /* mpeg1_decoder_has_sequence_header */
	int32_t width, height;            /* of that header (0 before it) */
	float frame_rate;                 /* mpeg1_decoder_get_frame_rate */
	int32_t status;                   /* 0: fine; 1: the header's size is not the batch's -- nothing of this stream is decoded */
	uint32_t pending_bytes;           /* written and not decoded yet */
	uint64_t bytes_written, pictures; /* totals */
	uint64_t evictions;               /* writes that found the store full of UNDECODED bytes and threw them away (buffer.js:48-56) */
} jsmpeg_hip_live_stream_info_t;

jsmpeg_hip_live_t *jsmpeg_hip_live_create(const jsmpeg_hip_live_config_t *config);
void jsmpeg_hip_live_destroy(jsmpeg_hip_live_t *l);
/* A stream joins: returns its id (0 .. max_streams - 1) or < 0.  It starts like a fresh decoder: no header, zeroed planes. */
int jsmpeg_hip_live_open(jsmpeg_hip_live_t *l);
/* ... and leaves (its id is handed out again by a later open). */
int jsmpeg_hip_live_close(jsmpeg_hip_live_t *l, uint32_t stream);
/* One write(pts, buffers) of the reference's decoder (decoder.js:36-47): `n` bytes of the stream's elementary stream are
 * appended to its store (copied during the call).  The store is the reference's EVICT store (buffer.js:30-62): decoded
 * bytes make room; when the UNDECODED bytes + n exceed store_bytes, the undecoded bytes are thrown away first (the
 * reference's "emergency evac") and the write starts an empty store.  n > store_bytes is refused (the reference's typed
 * array throws a RangeError there).  Returns 0 or < 0. */
int jsmpeg_hip_live_write(jsmpeg_hip_live_t *l, uint32_t stream, double pts, const void *bytes, uint32_t n);
/* The same write with its bytes in several pieces -- the `buffers` array of write(pts, buffers) (ts.js hands a PES over
 * as the payloads of its TS packets): ONE write of the total length (the store's rule looks at the total, buffer.js:66-92). */
int jsmpeg_hip_live_write_v(jsmpeg_hip_live_t *l, uint32_t stream, double pts, const void *const *buffers, const uint32_t *lengths,
                            uint32_t n_buffers);
/* The stream handed over as MPEG-TS bytes, in any pieces: the reference's demuxer (src/ts.js:25-210) runs in front of the
 * write above, with its state kept per stream between calls -- the leftover bytes of a cut packet (ts.js:25-41), resync
 * after garbage, the PES being collected, completion by PES_packet_length or by the padded last packet of a video frame
 * (ts.js:127-147).  Every PES of `stream_id` (0xE0: the first video stream) that the reference's demuxer would hand its
 * destination is one jsmpeg_hip_live_write(pts of the PES, its payload).  Returns 0 or < 0 (a write that was refused: the
 * first one's message; the demuxer's state moves on regardless, like ts.js's). */
int jsmpeg_hip_live_write_ts(jsmpeg_hip_live_t *l, uint32_t stream, const void *bytes, uint32_t n, uint32_t stream_id);
/* That demuxer by itself (host code, no device): `ts` handed over in write() calls of write_bytes[0 .. n_writes) bytes
 * (n_writes == 0: one write) -> the payload bytes of `stream_id` in `es` (at most es_cap) and, per destination.write call
 * the reference's demuxer would make, its pts and byte range (at most `cap` entries; any array may be NULL).  Returns the
 * number of such calls or < 0; *es_bytes: the bytes they carried. */
int jsmpeg_hip_ts_demux_host(const uint8_t *ts, uint64_t ts_bytes, const uint64_t *write_bytes, uint32_t n_writes, uint32_t stream_id,
                             uint8_t *es, uint64_t es_cap, uint64_t *es_bytes, double *pts, uint64_t *offset, uint32_t *length, uint32_t cap);
/* The tick: ONE pass of the batch engine over what has been written.  Per stream, in stream order, it decodes
 *   JSMPEG_HIP_LIVE_FLUSH: every buffered picture, the last one included -- it ends where the data ends, exactly like the
 *       reference's decode() (mpeg1.c:853-864, 947-995), so per stream this is `while (decoder.decode());` after the same
 *       writes.  The form for writes that carry whole pictures (ts.js completes a PES before it writes it);
 *   0: every picture that is COMPLETE -- a start code that is not a slice's follows it in the store; the last picture waits
 *       for the write that brings that code (or for a FLUSH tick).  The form for bytes that arrive in arbitrary pieces:
 *       per stream the pictures are those of the whole stream decoded in one piece, whatever the pieces were.
 * At most max_pictures_per_tick picture start codes per stream and tick; the rest wait.  Work is enqueued on
 * `hip_stream` (void* hipStream_t, NULL = the default stream) and has FINISHED when the call returns.
 * Returns the number of pictures decoded in this tick (all streams) or < 0. */
#define JSMPEG_HIP_LIVE_FLUSH 1u
int jsmpeg_hip_live_tick(jsmpeg_hip_live_t *l, uint32_t flags, void *hip_stream);
/* The same tick in two halves, for a host that has better things to do than wait for the GPU (a Node event loop; the
 * sockets the next pictures arrive on).  _begin lays the pass out, uploads it and enqueues all of it (it returns after the
 * start-code index's turn-around: about a fifth of the tick), _end waits and does the book-keeping and returns what
 * jsmpeg_hip_live_tick returns.  BETWEEN them jsmpeg_hip_live_write / _write_v / _write_ts are allowed and are what they
 * always are to the streams -- writes made right behind the tick: their bytes are copied to the staging buffer at once
 * (that is the work), their place in the stream's store (buffer.js:37-104: room, evacuation, the first header) is
 * decided when the tick has ended, in order.  Any other call on the handle between the halves ends the tick first (and
 * sees its pictures); a second _begin is an error.  _end without a tick in flight returns the last tick's count. */
int jsmpeg_hip_live_tick_begin(jsmpeg_hip_live_t *l, uint32_t flags, void *hip_stream);
int jsmpeg_hip_live_tick_end(jsmpeg_hip_live_t *l);
/* The pictures of the last tick: stream by stream (ascending id), in decode order inside a stream. */
uint32_t jsmpeg_hip_live_picture_count(jsmpeg_hip_live_t *l);
int jsmpeg_hip_live_picture(jsmpeg_hip_live_t *l, uint32_t i, jsmpeg_hip_live_picture_t *out);
/* Plane sizes of a frame: Y at 0, Cr at luma_bytes, Cb at luma_bytes + chroma_bytes. */
int jsmpeg_hip_live_geometry(jsmpeg_hip_live_t *l, int32_t *coded_width, int32_t *coded_height, uint32_t *luma_bytes,
                             uint32_t *chroma_bytes);
/* Device-to-host copy of picture i of the last tick (any of y / cr / cb may be NULL). */
int jsmpeg_hip_live_read_frame(jsmpeg_hip_live_t *l, uint32_t i, void *y, void *cr, void *cb);
/* The same as Canvas2D-identical RGBA (width * height * 4 bytes; jsmpeg_hip_batch_read_rgba). */
int jsmpeg_hip_live_read_rgba(jsmpeg_hip_live_t *l, uint32_t i, void *host_rgba);
/* Pictures first .. first + count - 1 of the last tick to the host in ONE go: picture first + k's planes (Y | Cr | Cb, luma_bytes
 * + 2 * chroma_bytes contiguous bytes) at host + k * stride.  One copy per picture, all enqueued, one wait -- and at the
 * link's rate when `host` is pinned (jsmpeg_hip_host_alloc, or memory of the caller's made so by jsmpeg_hip_host_register):
 * 64 x 1080p pictures in 4.1 ms (49 GB/s) against 7.3-8 ms through 64 jsmpeg_hip_live_read_frame calls into pageable memory.
 * What a host that RENDERS every picture (destination.render(y, cr, cb), mpeg1-wasm.js:109-119) calls once per tick. */
int jsmpeg_hip_live_read_frames(jsmpeg_hip_live_t *l, uint32_t first, uint32_t count, void *host, uint64_t stride);
/* The same read in two halves, for a host whose cycle IS the read-out (64 x 1080p pictures are 199 MB: 4.1 ms on the link against
 * a tick of 0.9): _begin enqueues the copies on a stream of the handle's own and returns; the host writes, and the NEXT tick
 * decodes, while they run; _end waits for them.  One read-out at a time (a second _begin before _end is an error; _end without
 * one returns 0).  The frames being read are safe: the tick right behind them writes other slots of the streams' rings when no
 * stream has more than two pictures among them, and any tick that could write over them (a stream with three or more; the tick
 * after the next) waits for the copies ON THE DEVICE first -- the host never blocks in a tick because of a read-out.  `host`
 * must stay valid (and should be pinned) until _end.  Unlike the other calls _end does not end a tick in flight. */
int jsmpeg_hip_live_read_frames_begin(jsmpeg_hip_live_t *l, uint32_t first, uint32_t count, void *host, uint64_t stride);
int jsmpeg_hip_live_read_frames_end(jsmpeg_hip_live_t *l);
/* Pinned host memory (hipHostMalloc / hipHostRegister): what the copy engines read and write at full rate.  register: the
 * caller's own memory (a JS ArrayBuffer's, a numpy array's) for as long as it stays registered; it must not be freed before
 * jsmpeg_hip_host_unregister. */
void *jsmpeg_hip_host_alloc(uint64_t bytes);
void jsmpeg_hip_host_free(void *p);
int jsmpeg_hip_host_register(void *p, uint64_t bytes);
int jsmpeg_hip_host_unregister(void *p);
/* 64-bit content hashes of the last tick's pictures (jsmpeg_hip_batch_frame_hashes' function). out[picture_count]. */
int jsmpeg_hip_live_frame_hashes(jsmpeg_hip_live_t *l, uint64_t *out);
int jsmpeg_hip_live_stream_info(jsmpeg_hip_live_t *l, uint32_t stream, jsmpeg_hip_live_stream_info_t *out);
/* Host clock of the last tick, milliseconds: [0] staging -> device + placement enqueued, [1] the batch engine's decode call
 * (enqueue + its two turn-arounds), [2] waiting for the device to finish, [3] book-keeping, [4] total; and the device's
 * own hipEvent timings of that pass: [5] index, [6] host turn-around, [7] slice parse, [8] reconstruct. */
int jsmpeg_hip_live_timings(jsmpeg_hip_live_t *l, float out_ms[9]);

/* ------------------------------------------------------------------ part 6
 * LIVE AUDIO streams: the MP2 half of the same loop (reference src/player.js:230-242 updateForStreaming -- "do { decoded =
 * this.audio.decode(); } while (decoded);" every tick; src/ts.js:205-210 hands the audio decoder one PES = a few whole frames
 * per write(pts, buffers); src/mp2-wasm.js:13-16 the 128 KiB EVICT store; src/wasm/mp2.c:213-222 the synthesis ring V and
 * its position v_pos, which carry from frame to frame).  Part 3's batch decodes whole streams from nothing; here a stream
 * persists across calls: its undecoded bytes stay with the handle, its last fifteen matrixing vectors and its position in
 * the synthesis ring stay in HBM, and one jsmpeg_hip_mp2_live_tick decodes the buffered frames of EVERY stream in one pass
 * of the stage's three kernels (frame chain, side information + matrixing, windowing) with ONE wait -- the frame counts
 * never come back to the host in between: a launch has max_frames_per_tick frame places per stream and the empty ones
 * leave at once.  Per stream the samples are bit for bit those of the reference's decoder given the same write() calls.
 * A handle is one thread's at a time; handles are independent of each other and of the video handles of part 5 (the same
 * TS bytes go to both: video with stream id 0xE0, audio with 0xC0).
 *
 *     id = jsmpeg_hip_mp2_live_open(a);
 *     jsmpeg_hip_mp2_live_write(a, id, pts, bytes, n);                == audio.write(pts, [bytes])   (ts.js:205-210)
 *     n = jsmpeg_hip_mp2_live_tick(a, NULL);                          == for every stream: while (audio.decode()) ;
 *     for (i < n) jsmpeg_hip_mp2_live_frame(a, i, &f);                f.device_pcm: float[2][1152] in HBM
 */

typedef struct jsmpeg_hip_mp2_live_t jsmpeg_hip_mp2_live_t;

typedef struct jsmpeg_hip_mp2_live_config_t {
	uint32_t max_streams;             /* streams open at a time */
	uint32_t max_frames_per_tick;     /* per stream: a tick decodes at most this many frames of a stream, the rest wait for the
	                                     next tick (0: 8 -- 0.2 s of sound at 44.1 kHz) */
	uint32_t store_bytes;             /* capacity of a stream's compressed-data store = the reference's audioBufferSize
	                                     (0: 128 KiB, mp2-wasm.js:13), with its EVICT rule: see jsmpeg_hip_mp2_live_write */
	int32_t device;                   /* HIP device ordinal, -1 = current */
} jsmpeg_hip_mp2_live_config_t;

typedef struct jsmpeg_hip_mp2_live_frame_t {
	uint32_t stream;                  /* id from jsmpeg_hip_mp2_live_open */
	int32_t sample_rate;              /* of this frame's header */
	double pts;                       /* of the write() in which the frame's first byte arrived */
	uint64_t stream_offset;           /* byte offset of that byte in everything ever written to the stream */
	uint32_t bytes;                   /* the frame's length (what mp2_decoder_decode returns for it) */
	uint32_t reserved;
	float *device_pcm;                /* DEVICE pointer: left[1152] | right[1152]; valid until the next tick.  The tick's frames lie
	                                     one behind the other: frame i + 1's samples follow frame i's */
} jsmpeg_hip_mp2_live_frame_t;

typedef struct jsmpeg_hip_mp2_live_stream_info_t {
	int32_t sample_rate;              /* mp2_decoder_get_sample_rate: of the frame decoded last, 44100 before the first (mp2.c:234) */
	uint32_t pending_bytes;           /* written and not decoded yet */
	uint64_t bytes_written, frames;   /* totals */
	uint64_t evictions;               /* writes that found the store full of UNDECODED bytes and threw them away (buffer.c:166-180) */
	int32_t stalled;                  /* 1: the bytes at the cursor are not a frame header the reference accepts (mp2.c:283-302): its
	                                     decode() returns 0 there for good, and so does every tick -- until a write that does not
	                                     fit evacuates the store, exactly like the reference's */
	int32_t reserved;
} jsmpeg_hip_mp2_live_stream_info_t;

jsmpeg_hip_mp2_live_t *jsmpeg_hip_mp2_live_create(const jsmpeg_hip_mp2_live_config_t *config);
void jsmpeg_hip_mp2_live_destroy(jsmpeg_hip_mp2_live_t *a);
/* A stream joins: returns its id (0 .. max_streams - 1) or < 0.  It starts like a fresh decoder (mp2.c:229-240): empty store,
 * the synthesis ring all zeros. */
int jsmpeg_hip_mp2_live_open(jsmpeg_hip_mp2_live_t *a);
/* ... and leaves (its id is handed out again by a later open). */
int jsmpeg_hip_mp2_live_close(jsmpeg_hip_mp2_live_t *a, uint32_t stream);
/* One write(pts, buffers) of the reference's decoder (decoder.js:36-47): `n` bytes are appended to the stream's store (copied
 * during the call).  The store is the reference's EVICT store (buffer.c:48-65, 166-189): decoded bytes make room; when the
 * UNDECODED bytes + n exceed store_bytes, the undecoded bytes are thrown away first ("emergency evac") and the write starts an
 * empty store.  n > store_bytes is refused (the reference writes past its allocation there).  Returns 0 or < 0. */
int jsmpeg_hip_mp2_live_write(jsmpeg_hip_mp2_live_t *a, uint32_t stream, double pts, const void *bytes, uint32_t n);
/* The same write with its bytes in several pieces (the `buffers` array): ONE write of the total length. */
int jsmpeg_hip_mp2_live_write_v(jsmpeg_hip_mp2_live_t *a, uint32_t stream, double pts, const void *const *buffers,
                                const uint32_t *lengths, uint32_t n_buffers);
/* The stream handed over as MPEG-TS bytes, in any pieces: the reference's demuxer in front of the write above, its state
 * kept per stream between calls (jsmpeg_hip_live_write_ts' function; stream_id 0xC0: the first audio stream, ts.js:212-222). */
int jsmpeg_hip_mp2_live_write_ts(jsmpeg_hip_mp2_live_t *a, uint32_t stream, const void *bytes, uint32_t n, uint32_t stream_id);
/* The tick: per stream, in stream order, every frame that is COMPLETELY buffered is decoded, from the cursor on, until a
 * header the reference refuses (the stream then stalls, see `stalled`), at most max_frames_per_tick of them.  With writes
 * that carry whole frames (ts.js completes a PES before it writes it) that is `while (mp2_decoder_decode(d));` after the
 * same writes; with bytes in arbitrary pieces a frame waits for its last byte (the reference would decode it from whatever
 * its store holds behind the written bytes) and per stream the frames are those of the whole stream decoded in one piece.
 * Work is enqueued on `hip_stream` (void* hipStream_t, NULL = the handle's own) and has FINISHED when the call returns.
 * Returns the number of frames decoded in this tick (all streams) or < 0. */
int jsmpeg_hip_mp2_live_tick(jsmpeg_hip_mp2_live_t *a, void *hip_stream);
/* The frames of the last tick: stream by stream (ascending id), in decode order inside a stream. */
uint32_t jsmpeg_hip_mp2_live_frame_count(jsmpeg_hip_mp2_live_t *a);
int jsmpeg_hip_mp2_live_frame(jsmpeg_hip_mp2_live_t *a, uint32_t i, jsmpeg_hip_mp2_live_frame_t *out);
/* Frames first .. first + count - 1 of the last tick to the host: out[count][2][1152] floats (left, right) -- what
 * destination.play(sampleRate, left, right) takes (mp2-wasm.js:93-103).  ONE copy (the tick's samples lie packed), one wait;
 * at the link's rate when `out` is pinned (jsmpeg_hip_host_alloc / _register). */
int jsmpeg_hip_mp2_live_read_pcm(jsmpeg_hip_mp2_live_t *a, uint32_t first, uint32_t count, float *out);
int jsmpeg_hip_mp2_live_stream_info(jsmpeg_hip_mp2_live_t *a, uint32_t stream, jsmpeg_hip_mp2_live_stream_info_t *out);
/* Host clock of the last tick, milliseconds: [0] packing the pending bytes + enqueueing, [1] waiting for the device,
 * [2] book-keeping, [3] total; and the device's own hipEvent timings: [4] upload + frame chain, [5] side information +
 * matrixing, [6] windowing + the tables' way back. */
int jsmpeg_hip_mp2_live_timings(jsmpeg_hip_mp2_live_t *a, float out_ms[7]);

/* ------------------------------------------------------------------ part 7
 * Decoded pictures as resized RGB TENSORS on the device, for hosts that feed a model (one kernel, jsmpeg_amd/csrc/tensor_plan.h).
 * Row k of the tensor, from the picture's planes (no full-size intermediate):
 *   RGB       display pixel (x, y): Y[y * coded_width + x], chroma at [(y >> 1) * (coded_width >> 1) + (x >> 1)], the Canvas2D
 *             integer BT.601 of jsmpeg_hip_batch_render_rgba.  Even widths: exactly read_rgba's RGB.  Odd widths: the same
 *             formula WITHOUT the reference's running-index shear and 255 fill -- the tensor is the picture, not the canvas;
 *   crop      (crop_x, crop_y, crop_width, crop_height), display pixels, inside the picture (0, 0, 0, 0: all of it); no filter
 *             tap reaches outside it;
 *   resize    to width x height: torch.nn.functional.interpolate(mode="bilinear", align_corners=False, antialias=antialias)
 *             of the crop's float RGB (0 .. 255) -- torch's tap tables, horizontal pass, then vertical;
 *   value     F16 / BF16 / F32: (v / 255 - mean[c]) / std[c], c in the tensor's channel order (round to nearest even);
 *             U8: rint(v) clamped to 0 .. 255 (mean / std unused);
 *   layout    NCHW: [count][3][height][width]; NHWC: [count][height][width][3]; contiguous; RGB or BGR.
 * Anything else -- a crop outside the picture, a side of 0 or above 4096, an unknown enum value, std 0, a picture or stream
 * index out of range, a batch picture that was not decoded (picture_info.decoded 0) -- is an error and nothing is launched.
 * Stream order: hip_stream first waits (an event, no host wait) for the stream that last wrote the pool; after the kernel an
 * event is recorded on hip_stream, and the next decode, enqueue or tick of the handle waits for it on its own stream before it
 * writes the pool.  The calls return after the launch (the host waits only when it is four renders of the handle ahead of the
 * device: the slot tables in flight).  count 0: returns 0, launches nothing.  f16 / bf16: the f32 value rounded, within one
 * ulp of torch's value cast -- except where normalisation cancels to within 5e-5 of 0, where the narrow type's ulp is finer
 * than the f32 rounding of the resize and the value is within that f32 tolerance instead. */
enum { JSMPEG_HIP_TENSOR_U8 = 0, JSMPEG_HIP_TENSOR_F16 = 1, JSMPEG_HIP_TENSOR_BF16 = 2, JSMPEG_HIP_TENSOR_F32 = 3 };
enum { JSMPEG_HIP_TENSOR_NCHW = 0, JSMPEG_HIP_TENSOR_NHWC = 1 };
enum { JSMPEG_HIP_TENSOR_RGB = 0, JSMPEG_HIP_TENSOR_BGR = 1 };
typedef struct jsmpeg_hip_tensor_desc_t {
	uint32_t width, height;                   /* of each picture in the tensor, 1..4096 */
	uint32_t crop_x, crop_y, crop_width, crop_height;   /* display pixels; crop_width = crop_height = 0: whole picture */
	uint32_t dtype, layout, order, antialias;
	float mean[3], std[3];                    /* float dtypes only, in the tensor's channel order */
} jsmpeg_hip_tensor_desc_t;

/* pictures[k] (host array; NULL = 0 .. count-1) of the last decode -> tensor row k in dev_out, enqueued on hip_stream.  Settles an
 * enqueued pass first, as jsmpeg_hip_batch_render_rgba does. */
int jsmpeg_hip_batch_render_tensor(jsmpeg_hip_batch_t *b, const uint32_t *pictures, uint32_t count,
                                   const jsmpeg_hip_tensor_desc_t *desc, void *dev_out, void *hip_stream);
/* the same over the last tick's pictures (jsmpeg_hip_live_picture's index) */
int jsmpeg_hip_live_render_tensor(jsmpeg_hip_live_t *l, const uint32_t *pictures, uint32_t count,
                                  const jsmpeg_hip_tensor_desc_t *desc, void *dev_out, void *hip_stream);
/* the newest decoded frame of each listed stream, from whichever tick decoded it; a stream with none yet:
 * its row is all-zero bytes and have[k] = 0 (have may be NULL) */
int jsmpeg_hip_live_render_tensor_latest(jsmpeg_hip_live_t *l, const uint32_t *streams, uint32_t count,
                                         const jsmpeg_hip_tensor_desc_t *desc, void *dev_out, void *hip_stream,
                                         uint8_t *have);

/* Per-box crops: tensor rows from REGIONS OF INTEREST that lie in device memory (a detector's boxes in front of a classifier,
 * re-identifier, OCR or face model), with no host wait in between (kernel k_tensor_roi; the rule: jm_roi_clip in tensor_plan.h).
 * Output row r is made from rois[r]: a box of display pixels in picture pictures[row] of the call (streams[row] for the latest
 * call).  The box is clipped to the picture, [0, width) x [0, height), in 64-bit arithmetic -- x = width = INT32_MAX is an
 * ordinary box -- and the row's status says what became of it:
 *   0  empty: row outside 0 .. count-1, width <= 0, height <= 0, no overlap with the picture, or no picture there (a live stream
 *      that has no frame yet).  Every byte of the output row is zero;
 *   1  the box lies inside the picture as given;
 *   2  the box was clipped to the picture.
 * For status 1 and 2 the row is EXACTLY what jsmpeg_hip_*_render_tensor gives for that picture with crop = the clipped box:
 * the same RGB, taps, pass order, value, dtype, layout and order, bit for bit.  A bad box is never an error: it is device data
 * that the host has not seen.  What the host can see keeps part 7's errors, with nothing launched: the descriptor, the picture
 * or stream indices, undecoded pictures -- and a descriptor whose own crop fields are not 0 (crop and rois exclude each other).
 *   dev_rois    DEVICE pointer, n_rois boxes, 4-byte aligned.  They must be READY ON hip_stream: written by earlier work on
 *               that stream, or by work it has been made to wait for; they are read by the kernel, never by the host;
 *   dev_out     n_rois rows of desc->width x desc->height (desc->layout, desc->dtype);
 *   dev_status  DEVICE pointer, n_rois bytes, or NULL: nothing is written.
 * The rest is part 7's contract: an enqueued pass is settled first, hip_stream waits for the pool's last writer, and the next
 * decode, enqueue or tick waits for the render.  n_rois 0: returns 0, launches nothing.  Not covered: aspect-preserving
 * letterbox or fill, rotated boxes, sub-pixel (roi_align) sampling. */
typedef struct jsmpeg_hip_roi_t {
	int32_t row;                              /* index into the call's picture (or stream) list */
	int32_t x, y, width, height;              /* display pixels */
} jsmpeg_hip_roi_t;
enum { JSMPEG_HIP_ROI_EMPTY = 0, JSMPEG_HIP_ROI_INSIDE = 1, JSMPEG_HIP_ROI_CLIPPED = 2 };
int jsmpeg_hip_batch_render_tensor_rois(jsmpeg_hip_batch_t *b, const uint32_t *pictures, uint32_t count,
                                        const jsmpeg_hip_tensor_desc_t *desc, const jsmpeg_hip_roi_t *dev_rois, uint32_t n_rois,
                                        void *dev_out, uint8_t *dev_status, void *hip_stream);
int jsmpeg_hip_live_render_tensor_rois(jsmpeg_hip_live_t *l, const uint32_t *pictures, uint32_t count,
                                       const jsmpeg_hip_tensor_desc_t *desc, const jsmpeg_hip_roi_t *dev_rois, uint32_t n_rois,
                                       void *dev_out, uint8_t *dev_status, void *hip_stream);
/* have[k] (may be NULL): stream streams[k] has a frame; the boxes of one that has none get status 0 */
int jsmpeg_hip_live_render_tensor_rois_latest(jsmpeg_hip_live_t *l, const uint32_t *streams, uint32_t count,
                                              const jsmpeg_hip_tensor_desc_t *desc, const jsmpeg_hip_roi_t *dev_rois, uint32_t n_rois,
                                              void *dev_out, uint8_t *dev_status, void *hip_stream, uint8_t *have);

/* ------------------------------------------------------------------ part 8
 * The way back: an MPEG-1 ENCODER on the device, I pictures and -- with a GOP, jsmpeg_hip_encoder_set_gop -- I + P.  Frames in HBM (a pool slot, a live picture's device_frame, the caller's
 * own planes) or RGB tensors -> elementary streams that a jsmpeg player, the reference decoder and parts 2 and 5 of this header
 * read.  One quantiser scale per picture, the default matrices, one slice per macroblock row; the integer transform, the
 * quantiser and the colour conversion are stated exactly in jsmpeg_amd/csrc/enc_block.h, motion search, mode decision and the
 * closed loop in jsmpeg_amd/csrc/enc_motion.h.  EVERY I picture carries its own sequence and GOP header in front (20 bytes):
 * every I picture -- with gop 1, the default, every picture -- is a joining point for a viewer and a unit for
 * jsmpeg_hip_split_gops.  Streams lie in the output from 16-byte aligned begins with 0xff in front of the first, between them
 * (8 bytes or more) and 256 bytes behind the last: the buffer can be handed to jsmpeg_hip_batch_attach_device as it is.
 * P CHAINS CROSS CALLS ONLY WHEN ASKED: without JSMPEG_HIP_ENC_CHAIN every stream of a call begins with an I picture, whatever
 * the call before ended with; with it a stream goes on where its last chained call left it (below, at the flag) -- a live relay
 * that encodes one picture per stream and tick gets its GOPs and its rate control that way.  Batch STREAMS, not pictures: a P picture waits for the picture before it,
 * so a call with one stream runs one picture at a time on the device.
 * OUT OF SCOPE: B pictures, quantiser changes inside a picture, a VBV model, custom matrices, vectors
 * beyond +-15 pels, a Node binding.
 * A pass is a PURE ENQUEUE on hip_stream, like jsmpeg_hip_batch_enqueue: every size and offset is worked out on the device; the
 * host waits in jsmpeg_hip_encoder_sync and the readers only (they settle the pass first).  One pass at a time per handle: a
 * second encode before the first is settled is refused.  ORDERING AGAINST THE PRODUCER OF THE FRAMES IS THE CALLER'S: pass the
 * stream the decode or render ran on, after jsmpeg_hip_batch_sync, exactly as jsmpeg_hip_batch_frame_pool demands of consumers.
 * A bad argument -- a size of zero or out of range, a quantiser scale of 0 or above 31, streams that do not ascend or reach
 * max_streams, count above max_pictures, a NULL or misaligned (16 bytes) frame -- returns < 0 with jsmpeg_hip_last_error, and
 * nothing is launched.  Without a device jsmpeg_hip_encoder_create returns NULL ("no CPU fallback"). */
typedef struct jsmpeg_hip_encoder_t jsmpeg_hip_encoder_t;
typedef struct jsmpeg_hip_encoder_config_t {
	int32_t width, height;        /* display size, 1..4095; coded size = next multiples of 16; at most 175 macroblock rows */
	uint32_t max_pictures;        /* per call */
	uint32_t max_streams;         /* per call */
	uint64_t max_es_bytes;        /* output capacity per call (the leading gap and the gaps between streams included) */
	uint32_t frame_rate_code;     /* 1..8 as in the sequence header; 0: 5 (30 / s) */
	int32_t device;               /* -1: current */
} jsmpeg_hip_encoder_config_t;
#define JSMPEG_HIP_ENC_END 1u     /* close every stream of the call with a sequence end code */
/* CONTINUE the call's streams (the rule: jsmpeg_amd/csrc/enc_chain.h).  The handle keeps, per stream number below max_streams,
 * whether the stream has chain state and how many pictures it has coded; the stream NUMBER is the stream's identity from call
 * to call (numbers still ascend within a call and may have gaps).  In a call with this flag the first picture of stream s has
 * the ordinal the stream's last chained call left (0 for a stream without state), and the ordinal drives the level in the GOP,
 * the picture type, the temporal reference and the GOP's time code as in one call over all the pictures: the call's first
 * picture of s is a P picture -- predicted from the reconstruction the call before left on the device -- unless that ordinal
 * is a multiple of gop.  The pieces of a stream, concatenated in call order, ARE the stream one call over all its pictures
 * writes (with rate control: when m below is gop for every picture, that is when every GOP is complete).  Still a pure enqueue:
 * the host needs nothing from the device for it.  A call without the flag neither reads nor writes this state and is byte for
 * byte what it was.
 * A PIECE THAT BEGINS WITH A P PICTURE begins at its picture start code (jsmpeg_hip_encoder_stream_range, _picture_range): it is
 * for concatenation, or for a live stream that already holds the sequence header -- not for jsmpeg_hip_batch_attach_device or
 * jsmpeg_hip_split_gops on its own.
 * A stream's chain ENDS, so that its next picture has ordinal 0 and is an I picture with sequence and GOP header: by
 * JSMPEG_HIP_ENC_END together with this flag (the end code is written, then every stream of the call is reset); by
 * jsmpeg_hip_encoder_chain_reset; by jsmpeg_hip_encoder_set_gop (every stream); by a chained call that overflowed (every
 * stream of that call, when the pass is settled).  Before an ordinal would pass 2^32 - 1 a GOP begins at ordinal 0 again: the
 * first multiple of gop above 2^32 - 1025 is replaced by 0.
 * RATE CONTROL in a chained call budgets every GOP for gop pictures (m = gop: later calls are taken to complete it, the call's
 * last GOP is not cut short), and the bytes a GOP's pictures took in earlier calls count as spent whichever call coded them --
 * kept on the device, written by a stream's last picture of a call.  Only calls with rate control keep that sum: bytes coded
 * by a chained call without it, and those of the same GOP before them, are not counted.  jsmpeg_hip_encoder_set_rate does
 * not reset chains; the rule runs with the handle's values at the time of the call.  Budgets still do not carry from GOP to GOP.
 * EXTRA DEVICE MEMORY, allocated by the first chained call with gop > 1 or rate control: two reconstructed frames and 16 bytes
 * per stream number of max_streams.  A stream's last picture of a chained call is reconstructed there (jsmpeg_hip_encoder_recon
 * returns that address); nothing is copied. */
#define JSMPEG_HIP_ENC_CHAIN 2u

jsmpeg_hip_encoder_t *jsmpeg_hip_encoder_create(const jsmpeg_hip_encoder_config_t *config);
void jsmpeg_hip_encoder_destroy(jsmpeg_hip_encoder_t *enc);
/* frames[k]: DEVICE pointer to picture k's planes, Y | Cr | Cb of the coded size (jsmpeg_hip_batch_geometry's layout: a
 * pool slot, a live picture's device_frame, the caller's own); stream[k]: ascending, < max_streams (NULL: all stream 0);
 * qscale[k]: 1..31 (NULL: `quantiser_scale` for all).  Pure enqueue on hip_stream; returns 0 or < 0. */
int jsmpeg_hip_encoder_encode(jsmpeg_hip_encoder_t *enc, const void *const *frames, const uint32_t *stream, const uint8_t *qscale,
                              uint32_t count, uint32_t quantiser_scale, uint32_t flags, void *hip_stream);
/* the same from `count` RGB pictures in ONE device tensor: uint8, layout / order as in part 7's enums, display size; converted
 * into a frame store of the handle's own (max_pictures frames, allocated by the first call) */
int jsmpeg_hip_encoder_encode_rgb(jsmpeg_hip_encoder_t *enc, const void *dev_rgb, uint32_t layout, uint32_t order, const uint32_t *stream,
                                  const uint8_t *qscale, uint32_t count, uint32_t quantiser_scale, uint32_t flags, void *hip_stream);
/* A RENDITION: the same from frames of ANOTHER size, cropped and scaled on the device into the handle's frame store (the one
 * jsmpeg_hip_encoder_encode_rgb fills; the first call of either allocates it) -- planes to planes, no RGB in between.  frames[k]:
 * Y | Cr | Cb of the SOURCE's coded size (a pool slot of a batch or live of `source->width` x `source->height`), one geometry for
 * all the pictures of the call.  The three planes are scaled independently with torch's bilinear / antialiased-bilinear filter
 * shapes (align_corners = False) stated as integer ratios with 14-bit weights, horizontal pass, then vertical, and the coded
 * size is filled by edge replication: the rule, bit for bit, is jsmpeg_amd/csrc/enc_scale.h.  A source of the encoder's size
 * without a crop is a copy.  The pass behind it -- GOP, rate control, JSMPEG_HIP_ENC_CHAIN, flags, readers, overflow -- is the
 * one of the other two entry points; jsmpeg_hip_encoder_timings' "convert" covers the scale.  Still a pure enqueue: the tap
 * table is built on the host in pinned memory and goes up on hip_stream.  A NULL descriptor, a size of 0 or above 4095, a crop
 * outside the picture, an odd crop_x or crop_y, antialias > 1: < 0 with jsmpeg_hip_last_error, nothing is launched. */
typedef struct jsmpeg_hip_enc_source_t {
	uint32_t width, height;                               /* display size of the SOURCE frames, 1..4095; planes of its coded size */
	uint32_t crop_x, crop_y, crop_width, crop_height;     /* display pixels, x / y even; all 0: the whole picture */
	uint32_t antialias;                                   /* 0 / 1 */
} jsmpeg_hip_enc_source_t;
int jsmpeg_hip_encoder_encode_scaled(jsmpeg_hip_encoder_t *enc, const void *const *frames, const jsmpeg_hip_enc_source_t *source,
                                     const uint32_t *stream, const uint8_t *qscale, uint32_t count, uint32_t quantiser_scale,
                                     uint32_t flags, void *hip_stream);
/* device pointer of the planes picture k of the last call was coded FROM (Y | Cr | Cb, the encoder's coded size): the caller's
 * frames[k] after jsmpeg_hip_encoder_encode, the handle's store after _encode_rgb (converted) and _encode_scaled (scaled).
 * Settles the pass first, like the other readers. */
const void *jsmpeg_hip_encoder_source(jsmpeg_hip_encoder_t *enc, uint32_t k);
/* A MOSAIC: one coded picture composed from MANY sources, plane to plane -- a wall of cameras, picture in picture.  A LAYOUT is
 * a fill colour and 1 .. 64 cells; a cell is the geometry of its frames (the descriptor _encode_scaled reads: size, crop,
 * antialias -- the sources may all differ) and a destination rectangle in the encoder's display pixels, x / y even, inside the
 * picture.  Every plane is filled, then each cell's three scaled planes (enc_scale.h, at the cell's size) are pasted in index
 * order: a later cell wins where cells overlap.  The rule, bit for bit, is jsmpeg_amd/csrc/enc_mosaic.h; one cell over the
 * whole picture is jsmpeg_hip_encoder_encode_scaled of that source.
 * OUT OF SCOPE: alpha blending, borders, labels and text, cells that change per picture within a call, rotation, a Node binding. */
typedef struct jsmpeg_hip_enc_cell_t {
	jsmpeg_hip_enc_source_t source;                       /* of this cell's frames */
	uint32_t x, y, width, height;                         /* where it goes: display pixels of the encoder, x / y even */
} jsmpeg_hip_enc_cell_t;   /* 44 bytes */
/* The layout is STATE OF THE HANDLE, like the GOP: checked, planned, its table built and uploaded here (synchronously; this
 * call allocates the table, max_pictures * n_cells frame pointers and, if no call has yet, the frame store).  fill: Y | Cr << 8 |
 * Cb << 16.  n_cells = 0 removes the layout.  Refused while a pass is in flight, and -- with a message that names the cell -- for
 * every breach of the rule: n_cells above 64, NULL cells, a bad source descriptor, a zero size, an odd x or y, a rectangle
 * outside the picture; nothing changes then and the layout before stays. */
int jsmpeg_hip_encoder_set_mosaic(jsmpeg_hip_encoder_t *enc, const jsmpeg_hip_enc_cell_t *cells, uint32_t n_cells, uint32_t fill);
/* frames[k * n_cells + c]: DEVICE pointer to cell c's frame for picture k (Y | Cr | Cb of that cell's source's coded size, 16-byte
 * aligned), or NULL: the cell is ABSENT from that picture and what lies under it shows; all NULL: the picture is all fill.  The
 * host touches no pixel: only the pointer array goes up, from pinned memory on hip_stream.  Everything else is
 * jsmpeg_hip_encoder_encode_scaled's: a pure enqueue; GOP, rate control, JSMPEG_HIP_ENC_CHAIN, TS, overflow and the readers
 * behind the planes unchanged; "convert" of the timings covers the composition; jsmpeg_hip_encoder_source returns the composed
 * planes.  Refused without a layout, for a misaligned frame, and by the argument checks of the other entry points. */
int jsmpeg_hip_encoder_encode_mosaic(jsmpeg_hip_encoder_t *enc, const void *const *frames, const uint32_t *stream, const uint8_t *qscale,
                                     uint32_t count, uint32_t quantiser_scale, uint32_t flags, void *hip_stream);
/* What feeds a mosaic from part 5: device_frames[k] = the frame of the NEWEST decoded picture of live stream streams[k], from
 * whichever tick decoded it (the ring slot jsmpeg_hip_live_render_tensor_latest reads), or NULL for a stream that has decoded
 * nothing yet.  Settles a tick in flight first; a stream that is not open is an error.  HOW LONG THE POINTER HOLDS ITS PICTURE:
 * a stream's ring has max_pictures_per_tick + 2 frames and its pictures are written to the slots after the newest one, in turn;
 * so the frame is written again by the stream's (max_pictures_per_tick + 2)-th picture decoded after this call, and not before.
 * A tick decodes at most max_pictures_per_tick pictures of a stream: the pointer always outlives the NEXT tick whole (that tick
 * writes the other slots), and with one picture per tick the max_pictures_per_tick + 1 next ticks.  A consumer's work on the
 * device must be over before the tick that decodes that picture is begun: ordering is the caller's, as everywhere in part 8.
 * Closing the stream ends the promise. */
int jsmpeg_hip_live_latest_frames(jsmpeg_hip_live_t *live, const uint32_t *streams, uint32_t count, const void **device_frames);
int jsmpeg_hip_encoder_sync(jsmpeg_hip_encoder_t *enc);             /* settles; < 0 with a message on overflow: nothing of the call is valid */
int jsmpeg_hip_encoder_query(jsmpeg_hip_encoder_t *enc);            /* 1 finished, 0 not; never blocks */
void *jsmpeg_hip_encoder_es(jsmpeg_hip_encoder_t *enc, uint64_t *total_bytes);   /* device buffer of the last call; NULL after an overflow */
int jsmpeg_hip_encoder_stream_range(jsmpeg_hip_encoder_t *enc, uint32_t stream, uint64_t *begin, uint64_t *end);
int jsmpeg_hip_encoder_picture_range(jsmpeg_hip_encoder_t *enc, uint32_t k, uint64_t *offset, uint32_t *bytes);   /* from its sequence header on */
/* the stream's bytes to the host (at most cap; host NULL: none); returns the stream's length or < 0 */
int64_t jsmpeg_hip_encoder_read_es(jsmpeg_hip_encoder_t *enc, uint32_t stream, void *host, uint64_t cap);
int jsmpeg_hip_encoder_timings(jsmpeg_hip_encoder_t *enc, float out_ms[4]);      /* convert, measure + scan (a GOP's level loop included), write, total */
/* gop 1 (the default): today's streams, byte for byte.  gop N > 1: in every stream of a call the pictures whose ordinal in the
 * stream is a multiple of N are I pictures with the sequence + GOP header in front, the others are P pictures (picture header
 * only, full_pel_forward_vector 0, temporal reference = the ordinal in the GOP) predicted from the encoder's OWN reconstruction
 * of the picture before -- exactly the frame a decoder holds.  jsmpeg_hip_encoder_picture_range of a P picture begins at its
 * picture start code.  search_range: full-pel radius 0 .. 15; 0 = zero vectors only, no half-pel step (conditional
 * replenishment); forward_f_code is 1 up to 7 and 2 above.  Refused while a pass is in flight, for gop 0, gop > 1024,
 * search_range > 15.  Ends every stream's chain (JSMPEG_HIP_ENC_CHAIN).  The stores only a GOP needs -- a reconstructed frame per picture of a call, the macroblocks' motion
 * records -- are allocated by the first call that asks for gop > 1. */
int jsmpeg_hip_encoder_set_gop(jsmpeg_hip_encoder_t *enc, uint32_t gop, uint32_t search_range);
/* device pointer of picture k's reconstruction in the last call (Y | Cr | Cb, coded size), wherever it lies: the call's store, or
 * -- a chained stream's last picture -- the stream's carry frame, which the stream's next chained call reads and the one after
 * that overwrites; NULL with a message when gop is 1 */
const void *jsmpeg_hip_encoder_recon(jsmpeg_hip_encoder_t *enc, uint32_t k);
/* macroblocks of picture k by kind: intra, predicted + coded, predicted not coded, skipped */
int jsmpeg_hip_encoder_picture_stats(jsmpeg_hip_encoder_t *enc, uint32_t k, uint32_t out[4]);
/* ends the chain of `stream` (UINT32_MAX: of every stream): its next chained picture is an I picture with ordinal 0 -- how a
 * relay gives a joining viewer a picture to start from, or drops a stream.  Refused while a pass is in flight and for a
 * stream >= max_streams. */
int jsmpeg_hip_encoder_chain_reset(jsmpeg_hip_encoder_t *enc, uint32_t stream);
/* out[0]: whether `stream` has chain state; out[1]: the pictures it has coded = the ordinal of its next chained picture.
 * Settles a pass in flight first (an overflow resets the call's streams). */
int jsmpeg_hip_encoder_chain_info(jsmpeg_hip_encoder_t *enc, uint32_t stream, uint32_t out[2]);
/* RATE CONTROL: the quantiser scale of every picture chosen on the device, still a pure enqueue.  bytes_per_picture 0 (the
 * default) switches it off: the scales are the caller's and every stream is what it was.  Otherwise, with m the pictures of a
 * picture's GOP in the call (a stream's last GOP may be short; gop 1: m = 1; in a chained call m = gop), the GOP has m * bytes_per_picture bytes; its I
 * picture gets the share i_weight / (i_weight + m - 1) of them, each P picture an equal share of what the pictures before it
 * left, and a picture is coded at the SMALLEST scale of q_min .. q_max at which it is at most its budget -- measured exactly
 * at every scale of the range, jsmpeg_hip_encoder_picture_range's bytes -- or at q_max if it is at none (the rule, in integers:
 * jsmpeg_amd/csrc/enc_rate.h).  Budgets do not carry from GOP to GOP, and from call to call only with JSMPEG_HIP_ENC_CHAIN; no VBV model, the headers stay as
 * they are.  State of the handle like the GOP; while on, the qscale / quantiser_scale arguments of the encode calls are checked
 * as before and otherwise unused, the pass is the GOP's also at gop 1 (jsmpeg_hip_encoder_recon works), and 62 bytes per
 * macroblock of max_pictures pictures are allocated by the first call that switches it on (with the GOP's stores, if they
 * are not there yet).  Refused while a pass is in flight, for q_min < 1, q_max > 31, q_min > q_max, i_weight outside 1 .. 255. */
int jsmpeg_hip_encoder_set_rate(jsmpeg_hip_encoder_t *enc, uint32_t bytes_per_picture, uint32_t q_min, uint32_t q_max, uint32_t i_weight);
/* what the rule chose for picture k of the last call: the scale, the budget (saturated to 32 bits), the picture's bytes;
 * refused when that call ran with rate control off */
int jsmpeg_hip_encoder_picture_rate(jsmpeg_hip_encoder_t *enc, uint32_t k, uint32_t out[3]);

/* Host-side TS mux (plain C, no device; a jsmpeg player takes TS): one PES per unit (a picture's range in `es`) with its PTS,
 * the payload in 184-byte pieces, the unit's last packet padded by adaptation-field stuffing -- what the reference's demuxer
 * (ts.js:127-147, jsmpeg_hip_ts_demux_host) ends a video PES by.  *continuity (in / out, may be NULL: 0) is the PID's counter,
 * carried across calls.  The rule, stated so that no packet depends on the packets before it: jsmpeg_amd/csrc/enc_ts.h -- the
 * same bytes as the mux on the device below.  Returns the bytes written, a multiple of 188, or < 0; ts == NULL: the bytes needed. */
int64_t jsmpeg_hip_ts_mux_host(const uint8_t *es, const uint64_t *offset, const uint32_t *bytes, const uint64_t *pts_90k,
                               uint32_t n_units, uint32_t stream_id, uint32_t pid, uint8_t *continuity /* in/out */,
                               uint8_t *ts, uint64_t ts_cap);

/* MPEG-TS ON THE DEVICE (a jsmpeg player takes TS): with jsmpeg_hip_encoder_set_ts the encode calls end in ready-to-send packets
 * per stream -- one PES per PICTURE, jsmpeg_hip_ts_mux_host's bytes -- muxed behind the write in the SAME ENQUEUE, and read back
 * in one copy (jsmpeg_hip_encoder_read_ts with UINT32_MAX).  Unit k is picture k's range as jsmpeg_hip_encoder_picture_range
 * reports it (an I picture with its sequence and GOP header, a P picture from its picture start code); a stream's last picture
 * of a call with JSMPEG_HIP_ENC_END runs on over the end code, so a stream's TS carries every byte of the stream.  In the TS
 * buffer the first stream of the call begins at 0, each next one at the end before it rounded up to 16; the bytes between
 * streams are unspecified.  CONTINUITY: a counter per stream number, kept on the device, where the packet counts are known; a
 * property of the PID, not of the chain: jsmpeg_hip_encoder_chain_reset and jsmpeg_hip_encoder_set_gop leave the counters
 * alone, only jsmpeg_hip_encoder_set_ts zeroes them, and a call that overflowed -- in the ES or in the TS -- leaves them where
 * it found them.  A TS OVERFLOW IS AN OVERFLOW OF THE CALL: jsmpeg_hip_encoder_sync fails with a message that names
 * max_ts_bytes, nothing of the call is valid, chained streams are reset as after an ES overflow; after an ES overflow there
 * is no TS.  jsmpeg_hip_encoder_timings' "write" covers the mux.  The ES buffer and all its readers are what they are
 * without TS; a handle that never calls jsmpeg_hip_encoder_set_ts is byte for byte what it was and allocates nothing new.
 * OUT OF SCOPE: PAT / PMT / PCR (jsmpeg's demuxer needs none; other players do); audio or a second PID in the same buffer
 * (packets are self-contained, so a host may interleave) -- both are part 10's, jsmpeg_hip_ts_program_*; Node bindings of the encoder; kernel stores straight into pinned
 * host memory.
 * jsmpeg_hip_encoder_set_ts: max_ts_bytes 0 switches TS off (the default); otherwise the TS buffer, the unit table (56 bytes
 * per picture of max_pictures) and max_streams counter words are allocated and ALL counters set to 0.  Refused while a pass is
 * in flight, for pid > 0x1fff, stream_id > 0xff.  jsmpeg_hip_ts_bound gives a safe max_ts_bytes for es_bytes of payload in
 * `units` units over `streams` streams. */
int jsmpeg_hip_encoder_set_ts(jsmpeg_hip_encoder_t *enc, uint32_t stream_id, uint32_t pid, uint64_t max_ts_bytes);
/* the PTS values (90 kHz, the low 33 bits go out) of the NEXT encode call, one per picture; consumed by that call: a count that
 * differs from the call's is refused BY THAT CALL, nothing is launched, and the call after it is not bound.  Without it picture
 * k's PTS is floor(ordinal * 90000 * den / num) in 64 bits, masked to 33 bits: ordinal the picture's ordinal in its stream (in a
 * chained call the chain's), num / den the pictures per second of frame_rate_code (24000/1001, 24, 25, 30000/1001, 30, 50,
 * 60000/1001, 60).  The host computes the values either way and uploads them on hip_stream: the pass stays a pure enqueue. */
int jsmpeg_hip_encoder_ts_pts(jsmpeg_hip_encoder_t *enc, const uint64_t *pts_90k, uint32_t count);
/* THE READERS settle the pass like every other reader and refuse a handle with TS off or one whose last call overflowed.
 * device buffer of the last call's TS and its total bytes */
void *jsmpeg_hip_encoder_ts(jsmpeg_hip_encoder_t *enc, uint64_t *total_bytes);
/* a stream's range in the TS buffer and the stream's counter behind the call (what its next packet will carry) */
int jsmpeg_hip_encoder_ts_range(jsmpeg_hip_encoder_t *enc, uint32_t stream, uint64_t *begin, uint64_t *end, uint32_t *continuity_next);
/* picture k's packets: offset in the TS buffer and bytes, a multiple of 188; a viewer that joins starts at an I picture's */
int jsmpeg_hip_encoder_ts_picture_range(jsmpeg_hip_encoder_t *enc, uint32_t k, uint64_t *offset, uint32_t *bytes);
/* a stream's TS to the host (at most cap; host NULL: none); stream UINT32_MAX: the whole buffer, every stream, in ONE copy
 * (jsmpeg_hip_encoder_ts_range tells the streams apart); returns the length or < 0 */
int64_t jsmpeg_hip_encoder_read_ts(jsmpeg_hip_encoder_t *enc, uint32_t stream, void *host, uint64_t cap);
uint64_t jsmpeg_hip_ts_bound(uint64_t es_bytes, uint32_t units, uint32_t streams);
/* The same two kernels over ANY device bytes and a host-given unit list, for stored ES on the device: unit i is bytes[i] bytes at
 * dev_es + offset[i] of stream number stream[i] (NULL: all 0) -- a stream's units contiguous, streams ascending and below
 * n_streams.  Synchronous, on the null stream (the producer of dev_es must have finished), with scratch of its own for the
 * call.  continuity: one in / out counter per stream number [n_streams] (NULL: 0, nothing handed back); stream_begin /
 * stream_end: host out arrays [n_streams] (0, 0 for a stream without units), laid out as above; dev_ts: 4-byte aligned,
 * ts_cap bytes writable.  Returns the total bytes, or < 0 (a ts_cap too small: nothing is written, the
 * counters stay).  No CPU fallback: without a device < 0. */
int64_t jsmpeg_hip_ts_mux_device(const void *dev_es, const uint64_t *offset, const uint32_t *bytes, const uint32_t *stream,
                                 const uint64_t *pts_90k, uint32_t n_units, uint32_t stream_id, uint32_t pid,
                                 uint8_t *continuity /* in/out */, uint32_t n_streams,
                                 void *dev_ts, uint64_t ts_cap, uint64_t *stream_begin, uint64_t *stream_end);

/* ------------------------------------------------------------------ part 9
 * The audio half of the way back: an MPEG-1 Audio LAYER II ENCODER on the device.  PCM in HBM -- float32 [frame][2][1152], the
 * layout parts 3 and 6 leave it in; a mono handle reads channel 0 -- -> constant-bit-rate Layer II frames in a device buffer
 * that jsmpeg_hip_mp2_batch_upload_device and jsmpeg_hip_ts_mux_device (stream_id 0xC0) take as it is.  The rule is stated
 * once, in jsmpeg_amd/csrc/mp2_enc.h: exact integer analysis filterbank, scalefactors without lossy merging, a greedy bit
 * allocation on a fixed noise measure, and a quantiser that is closed-loop against the decoder's own requantiser.  The streams
 * carry ISO's level: a full-scale sine has subband samples near 1.  (The decoder of parts 3 and 6 returns, like the reference,
 * HALF of ISO's level -- its window is ISO's D times 2^15 and its output divides by 2^31 -- so PCM decoded here from these
 * streams is the input times one half, 481 samples late.)
 * FRAME LENGTHS ARE CLOSED FORM: N = 144000 kbit/s, b = N / fs, r = N mod fs; frame n of a stream (its ordinal, which goes on
 * across chained calls) has b + floor((n + 1) r / fs) - floor(n r / fs) bytes and begins n b + floor(n r / fs) bytes behind
 * ordinal 0.  Streams of a call begin at multiples of 16 with zeros up to the next multiple behind each; the total is a
 * multiple of 16.  So the host knows every offset at enqueue time: a call is ONE kernel, a workgroup per frame, a PURE ENQUEUE
 * on hip_stream with an event at its end; jsmpeg_hip_mp2_encoder_sync and the readers of device results settle it, the
 * ranges are answered without waiting.  One pass at a time per handle: a second encode before the first is settled is
 * REFUSED, as in part 8.  Ordering against the producer of the PCM is the caller's: pass the stream it ran on.
 * OUT OF SCOPE: a psychoacoustic model, joint stereo, dual channel, CRC, variable bit rate, lossy scfsi merging, a Node binding.
 * A bad argument returns < 0 with jsmpeg_hip_last_error and nothing is launched; so does a call whose total is above
 * max_es_bytes (known on the host), and the handle stays usable.  Without a device create returns NULL (no CPU fallback). */
typedef struct jsmpeg_hip_mp2_encoder_t jsmpeg_hip_mp2_encoder_t;
typedef struct jsmpeg_hip_mp2_encoder_config_t {
	uint32_t sample_rate_index;   /* 0: 44100, 1: 48000, 2: 32000 */
	uint32_t channels;            /* 1: mode mono, 2: mode stereo */
	uint32_t bitrate_index;       /* 1..14; not 32 / 48 / 56 / 80 kbit/s with two channels, not 224 .. 384 with one */
	uint32_t max_streams;         /* per call, and the stream numbers of chained calls lie below it */
	uint32_t max_frames;          /* per call */
	uint64_t max_es_bytes;        /* output capacity per call (the zeros behind every stream included) */
	int32_t device;               /* -1: current */
} jsmpeg_hip_mp2_encoder_config_t;
#define JSMPEG_HIP_MP2_ENC_END 1u     /* with CHAIN: the chains of the call's streams end behind it (as jsmpeg_hip_mp2_encoder_chain_reset) */
/* CONTINUE the call's streams: the handle keeps, per stream number, whether the stream has state, its ordinal and which of
 * two carries on the device holds its last 480 samples per channel.  The first frame of a stream reads that carry, the last
 * one writes the other, so the pieces of a stream, concatenated in call order, ARE byte for byte the stream one call over all
 * its frames writes, padding included.  A stream without frames in a call keeps its state; a call without the flag neither
 * reads nor writes it. */
#define JSMPEG_HIP_MP2_ENC_CHAIN 2u
jsmpeg_hip_mp2_encoder_t *jsmpeg_hip_mp2_encoder_create(const jsmpeg_hip_mp2_encoder_config_t *config);
void jsmpeg_hip_mp2_encoder_destroy(jsmpeg_hip_mp2_encoder_t *enc);
/* stream i: frames[i] (0 allowed) contiguous frames at the device address pcm[i] (4-byte aligned; ignored for 0 frames), stream
 * number stream_numbers[i] (strictly ascending, below max_streams; NULL: i) */
int jsmpeg_hip_mp2_encoder_encode(jsmpeg_hip_mp2_encoder_t *enc, const void *const *pcm, const uint32_t *frames, const uint32_t *stream_numbers,
                                  uint32_t n_streams, uint32_t flags, void *hip_stream);
int jsmpeg_hip_mp2_encoder_sync(jsmpeg_hip_mp2_encoder_t *enc);
/* 1: no pass in flight, 0: still running; never waits */
int jsmpeg_hip_mp2_encoder_query(jsmpeg_hip_mp2_encoder_t *enc);
/* the last call's buffer on the device and its bytes (settles the pass) */
void *jsmpeg_hip_mp2_encoder_es(jsmpeg_hip_mp2_encoder_t *enc, uint64_t *total_bytes);
/* [begin, end) of stream NUMBER `stream` in that buffer (0, 0: not in the call) and of frame k of the call: closed form, no wait */
int jsmpeg_hip_mp2_encoder_stream_range(jsmpeg_hip_mp2_encoder_t *enc, uint32_t stream, uint64_t *begin, uint64_t *end);
int jsmpeg_hip_mp2_encoder_frame_range(jsmpeg_hip_mp2_encoder_t *enc, uint32_t k, uint64_t *offset, uint32_t *bytes);
/* a stream's bytes to the host (at most cap; host NULL: none); returns the length or < 0 */
int64_t jsmpeg_hip_mp2_encoder_read_es(jsmpeg_hip_mp2_encoder_t *enc, uint32_t stream, void *host, uint64_t cap);
/* frame k: pairs that got bits, bits used, bits left over, the largest allocation code */
int jsmpeg_hip_mp2_encoder_frame_stats(jsmpeg_hip_mp2_encoder_t *enc, uint32_t k, uint32_t out[4]);
/* ends the chain of `stream` (UINT32_MAX: of every stream); refused while a pass is in flight */
int jsmpeg_hip_mp2_encoder_chain_reset(jsmpeg_hip_mp2_encoder_t *enc, uint32_t stream);
/* out[0]: the stream has chain state; out[1]: frames it has coded = the ordinal of its next chained frame */
int jsmpeg_hip_mp2_encoder_chain_info(jsmpeg_hip_mp2_encoder_t *enc, uint32_t stream, uint64_t out[2]);
/* the last pass on the device: the kernel (with the upload of its frame list), the whole enqueue */
int jsmpeg_hip_mp2_encoder_timings(jsmpeg_hip_mp2_encoder_t *enc, float out_ms[2]);

/* ------------------------------------------------------------------ part 10
 * TS PROGRAM MUX ON THE DEVICE: the last step of the way back.  A jsmpeg player is fed ONE transport stream per channel with
 * video and audio interleaved in it; parts 8 and 9 end in one buffer per kind.  A program handle turns two unit tables --
 * video units over one device buffer, audio units over another -- into one program per stream number, in ONE enqueue and
 * read back in ONE copy, and on request with PAT / PMT / PCR, so that players other than jsmpeg open the result too.  The
 * rule is stated once, in jsmpeg_amd/csrc/ts_prog.h, on top of part 8's (enc_ts.h: the PES header, one PES per unit, the
 * stuffing); jsmpeg_hip_ts_program_mux_host writes the same bytes without a device.
 * ORDER: per stream number the two lists are merged by PTS (64-bit 90 kHz values, unwrapped; the low 33 bits go out), video
 * first at equal PTS; a unit's packets lie back to back.  In each table a stream's units are contiguous, the streams ascend
 * and stay below max_streams, and the PTS do not decrease within a stream: anything else is REFUSED.  A kind whose PID is
 * configured as 0x1fff is absent: units of it are refused and the PMT does not list it.  In the output the first stream
 * begins at 0, each next one at the end before it rounded up to 16; the bytes between streams are unspecified.
 * JSMPEG_HIP_TSP_PCR: the first packet of every unit of the carrier kind (video if present, else audio) carries a PCR of
 * (pts - pcr_lead_90k) mod 2^33, extension 0, in an adaptation field of 8 bytes -- the only place where the reference's
 * demuxer (ts.js:143) lets a video PES carry one.
 * JSMPEG_HIP_TSP_PSI: one PAT packet (PID 0) and one PMT packet (pmt_pid; stream_type 0x01 video, 0x03 audio, PCR_PID the
 * carrier's) go in front of a stream's first unit since create / reset and in front of every video unit that begins with a
 * sequence header (00 00 01 B3: every I picture part 8 writes), once where both hold.
 * STATE per stream number, on the device: the continuity counters of PAT, PMT, video and audio, and `started`.  A call that
 * does not fit max_ts_bytes (or the caller's buffer) writes NOTHING and leaves all five words; so does a call behind an ES
 * overflow of the video encoder (jsmpeg_hip_ts_program_mux_encoders).  jsmpeg_hip_ts_program_sync then fails with a message.
 * A call is a PURE ENQUEUE on hip_stream with an event at its end; one pass at a time per handle: a second call before the
 * first is settled (sync, or any reader) is REFUSED, as in parts 8 and 9.  Without a device create returns NULL.
 * OUT OF SCOPE: packet-level interleave inside a unit; T-STD buffer conformance, constant-rate null-packet padding, more than
 * one audio PID; several frames per PES beyond what the caller's ranges express; B-picture DTS; Node bindings. */
typedef struct jsmpeg_hip_ts_program_t jsmpeg_hip_ts_program_t;
typedef struct jsmpeg_hip_ts_program_config_t {
	uint32_t max_streams;         /* stream numbers lie below it */
	uint32_t max_video_units;     /* per call */
	uint32_t max_audio_units;     /* per call */
	uint64_t max_ts_bytes;        /* output capacity per call (jsmpeg_hip_ts_program_bound) */
	uint32_t video_pid;           /* 0x1fff: no video */
	uint32_t audio_pid;           /* 0x1fff: no audio */
	uint32_t pmt_pid;
	uint32_t video_stream_id;     /* 0: 0xE0 */
	uint32_t audio_stream_id;     /* 0: 0xC0 */
	uint32_t program_number;
	uint32_t transport_stream_id;
	uint32_t flags;               /* JSMPEG_HIP_TSP_* */
	uint64_t pcr_lead_90k;        /* how far the PCR runs behind the PTS it is written with */
	int32_t device;               /* -1: current */
} jsmpeg_hip_ts_program_config_t;
#define JSMPEG_HIP_TSP_PSI 1u
#define JSMPEG_HIP_TSP_PCR 2u
/* refuses PIDs above 0x1fff, equal PIDs, PID 0 for anything but the PAT, both kinds absent, stream ids above 0xff, sizes of 0 */
jsmpeg_hip_ts_program_t *jsmpeg_hip_ts_program_create(const jsmpeg_hip_ts_program_config_t *config);
void jsmpeg_hip_ts_program_destroy(jsmpeg_hip_ts_program_t *prog);
/* the calls write into dev_ts (4-byte aligned, cap bytes writable) instead of the handle's own buffer; NULL: the handle's
 * again.  Refused while a pass is in flight. */
int jsmpeg_hip_ts_program_set_output(jsmpeg_hip_ts_program_t *prog, void *dev_ts, uint64_t cap);
/* HOST tables over two device buffers: video unit i is v_bytes[i] bytes at dev_video + v_offset[i], stream number v_stream[i]
 * (NULL: all 0), PTS v_pts[i]; the audio units likewise.  Pinned staging, uploads on hip_stream, the two kernels, an event. */
int jsmpeg_hip_ts_program_mux(jsmpeg_hip_ts_program_t *prog,
                              const void *dev_video, const uint64_t *v_offset, const uint32_t *v_bytes, const uint32_t *v_stream, const uint64_t *v_pts, uint32_t n_v,
                              const void *dev_audio, const uint64_t *a_offset, const uint32_t *a_bytes, const uint32_t *a_stream, const uint64_t *a_pts, uint32_t n_a,
                              void *hip_stream);
/* THE RELAY FORM: the video units are the last call of `enc` -- unit k = picture k's range, the end code as
 * jsmpeg_hip_encoder_set_ts does it -- taken from the encoder's picture table ON THE DEVICE: that call may still be in flight
 * on the same hip_stream, nothing is waited for.  The audio units are the frames of the last call of `mp2enc` (closed-form
 * ranges).  v_pts / a_pts: one value per picture / frame, or NULL: floor(ordinal * 90000 * den / num) of the picture's chain
 * ordinal, floor(ordinal * 1152 * 90000 / fs) of the frame's.  Either encoder may be NULL; stream numbers are the encoders' own. */
int jsmpeg_hip_ts_program_mux_encoders(jsmpeg_hip_ts_program_t *prog, jsmpeg_hip_encoder_t *enc, const uint64_t *v_pts,
                                       jsmpeg_hip_mp2_encoder_t *mp2enc, const uint64_t *a_pts, void *hip_stream);
int jsmpeg_hip_ts_program_sync(jsmpeg_hip_ts_program_t *prog);
/* 1: no pass in flight, 0: still running; never waits */
int jsmpeg_hip_ts_program_query(jsmpeg_hip_ts_program_t *prog);
/* THE READERS settle the pass and refuse a handle whose last call failed.  The last call's device buffer and its total bytes */
void *jsmpeg_hip_ts_program_ts(jsmpeg_hip_ts_program_t *prog, uint64_t *total_bytes);
/* [begin, end) of stream NUMBER `stream` in that buffer (0, 0: not in the call) */
int jsmpeg_hip_ts_program_stream_range(jsmpeg_hip_ts_program_t *prog, uint32_t stream, uint64_t *begin, uint64_t *end);
/* unit k of `kind` (0 video, 1 audio) of the call's table: where its packets begin -- at the PAT if PSI lies in front --
 * their bytes (the PSI's included), and the PSI's bytes (0 or 376); a viewer that joins starts at a unit with PSI */
int jsmpeg_hip_ts_program_unit_range(jsmpeg_hip_ts_program_t *prog, uint32_t kind, uint32_t k, uint64_t *offset, uint32_t *bytes, uint32_t *psi_bytes);
/* a stream's program to the host (at most cap; host NULL: none); stream UINT32_MAX: the whole buffer in ONE copy; returns the
 * length or < 0 */
int64_t jsmpeg_hip_ts_program_read(jsmpeg_hip_ts_program_t *prog, uint32_t stream, void *host, uint64_t cap);
/* the stream's words behind the last call: the counters of PAT, PMT, video, audio (what their next packets carry), started */
int jsmpeg_hip_ts_program_state(jsmpeg_hip_ts_program_t *prog, uint32_t stream, uint32_t out[5]);
/* zeroes the five words of `stream` (UINT32_MAX: of every stream); refused while a pass is in flight */
int jsmpeg_hip_ts_program_reset(jsmpeg_hip_ts_program_t *prog, uint32_t stream);
/* sets the five words of `stream` (counters 0 .. 15, started 0 or 1): a relay that restarts goes on where its streams were;
 * refused while a pass is in flight */
int jsmpeg_hip_ts_program_set_state(jsmpeg_hip_ts_program_t *prog, uint32_t stream, const uint32_t in[5]);
/* the last pass on the device: the uploads and the two kernels, the whole enqueue */
int jsmpeg_hip_ts_program_timings(jsmpeg_hip_ts_program_t *prog, float out_ms[2]);
/* THE SAME BYTES ON THE HOST (plain C, no device): the arguments of jsmpeg_hip_ts_program_mux over host bytes.  state: in /
 * out, 5 words per stream number [config->max_streams] (NULL: zeros, nothing handed back); stream_begin / stream_end: out
 * arrays [max_streams], may be NULL.  Returns the total bytes, or < 0 (ts_cap too small: nothing is written, the state
 * stays); ts == NULL: the bytes needed, nothing changes. */
int64_t jsmpeg_hip_ts_program_mux_host(const jsmpeg_hip_ts_program_config_t *config,
                                       const uint8_t *video, const uint64_t *v_offset, const uint32_t *v_bytes, const uint32_t *v_stream, const uint64_t *v_pts, uint32_t n_v,
                                       const uint8_t *audio, const uint64_t *a_offset, const uint32_t *a_bytes, const uint32_t *a_stream, const uint64_t *a_pts, uint32_t n_a,
                                       uint32_t *state /* in/out */, uint8_t *ts, uint64_t ts_cap, uint64_t *stream_begin, uint64_t *stream_end);
/* a safe max_ts_bytes: per unit at most bytes / 184 + 2 packets, 2 PSI packets per video unit and per stream, 15 per stream */
uint64_t jsmpeg_hip_ts_program_bound(uint64_t v_bytes, uint32_t n_v, uint64_t a_bytes, uint32_t n_a, uint32_t streams);
/* the PAT packet and the PMT packet of `config` (2 * 188 bytes, continuity 0), as the handle uploads them; plain C */
int jsmpeg_hip_ts_program_psi(const jsmpeg_hip_ts_program_config_t *config, uint8_t out[376]);

/* ------------------------------------------------------------------ part 11
 * PCM RESAMPLER ON THE DEVICE: the audio side's tensor() and its rendition path, one kernel for both.  PCM in HBM -- float32
 * [frame][2][1152], the layout parts 3 and 6 leave it in -- -> either a padded batch of WAVEFORMS for models (mono or stereo,
 * f32 / f16 / bf16, e.g. 16 kHz mono f16 for a speech model) or FRAMES at another rate in the layout part 9 reads, so that a
 * relay sends 48 kHz audio on at 32 kHz beside a smaller video rendition.  The rule is stated once, in
 * jsmpeg_amd/csrc/pcm_resample.h.  In short: rates 32000 / 44100 / 48000 in, 8000 / 16000 / 22050 / 24000 / 32000 / 44100 /
 * 48000 out, out != in (18 pairs); L = out / gcd, M = in / gcd; a Kaiser-windowed sinc (beta 9, cut-off 0.9 of the lower
 * Nyquist, half width H = 16 input samples, ceil(16 M / L) when the rate goes down) as L phases of 2 H float32 taps computed in
 * double on the host; output m of a stream is gain * sum_j h[(m M) mod L][j] x[floor(m M / L) - 2 H + 1 + j], accumulated in
 * float32 with one fused multiply-add per tap in ascending j, x = 0 before the stream's first sample; a handle with one
 * output channel filters 0.5f * (left + right).  After N input samples a stream has ceil(N L / M) outputs: counts are CLOSED
 * FORM, the host knows every count and offset at enqueue time, a call is ONE kernel and a PURE ENQUEUE on hip_stream with an
 * event at its end.  A stream resampled in pieces, chained call after chained call, is BIT FOR BIT the stream resampled in
 * one call.
 * DELAY: the output is the input delayed by H input samples, H / in_rate seconds (jsmpeg_hip_resample_plan gives H): a relay
 * shifts its PTS by that much, or accepts it.
 * LEVEL: gain multiplies every output once (0 means 1.0).  Parts 3 and 6 return half of ISO's level and part 9 expects ISO's,
 * so a decode-to-encode relay passes gain 2.0 and keeps its level from generation to generation.
 * One pass at a time per handle: a second call before the first is settled (sync, or timings) is REFUSED, as in parts 8 and
 * 9.  Results are valid until the handle's next call.  A bad argument -- an unsupported pair, frames above max_frames, a
 * stream number out of range or not ascending, a stream with more samples than row -- returns < 0 with jsmpeg_hip_last_error,
 * launches nothing and leaves the handle usable.  Without a device create returns NULL (no CPU fallback).
 * OUT OF SCOPE: a Node binding, other rates, dither, any filter choice but this one, sample-rate changes inside a stream. */
typedef struct jsmpeg_hip_resampler_t jsmpeg_hip_resampler_t;
#define JSMPEG_HIP_RESAMPLE_WAVEFORM 0u
#define JSMPEG_HIP_RESAMPLE_FRAMES 1u
#define JSMPEG_HIP_RESAMPLE_F32 0u
#define JSMPEG_HIP_RESAMPLE_F16 1u
#define JSMPEG_HIP_RESAMPLE_BF16 2u
typedef struct jsmpeg_hip_resampler_config_t {
	uint32_t in_rate, out_rate;   /* Hz */
	uint32_t channels_out;        /* 2: left and right; 1: their mix, 0.5f * (left + right), made before the filter */
	uint32_t form;                /* WAVEFORM: [stream of the call][channels_out][row] of dtype, zeros behind a stream's count;
	                                 FRAMES: float32 [frame][2][1152] at out_rate (one channel: the mix in both), stream after stream */
	uint32_t dtype;               /* WAVEFORM only; F16 / BF16: the float32 value rounded to nearest even */
	float gain;                   /* 0: 1.0 */
	uint32_t max_streams;         /* per call, and the stream numbers of chained calls lie below it */
	uint32_t max_frames;          /* input frames per call */
	uint32_t row;                 /* WAVEFORM: samples per stream and channel of the output; 0: what max_frames frames of one stream
	                                 and END's tail yield */
	int32_t device;               /* -1: current */
} jsmpeg_hip_resampler_config_t;
/* continue every listed stream that has any input -- in this call or in its chain -- by H zero samples, so that the filter's
 * tail comes out; FRAMES: the last partial frame is filled with zeros.  With CHAIN the chains of the call's streams end
 * behind it. */
#define JSMPEG_HIP_RESAMPLE_END 1u
/* CONTINUE the call's streams: the handle keeps, per stream number, whether the stream has state, its input and output
 * counts, and which of two carries on the device holds its last 2 H - 1 input samples per channel (FRAMES: and its partial
 * output frame).  A call reads one and writes the other.  A stream without frames in a call keeps its state; a call without
 * the flag starts from nothing and stores nothing (FRAMES: without END its partial last frame is dropped). */
#define JSMPEG_HIP_RESAMPLE_CHAIN 2u
jsmpeg_hip_resampler_t *jsmpeg_hip_resampler_create(const jsmpeg_hip_resampler_config_t *config);
void jsmpeg_hip_resampler_destroy(jsmpeg_hip_resampler_t *rs);
/* the input convention of jsmpeg_hip_mp2_encoder_encode: stream i has frames[i] (0 allowed) contiguous frames at the device
 * address pcm[i] (4-byte aligned; ignored for 0 frames) and the number stream_numbers[i] (strictly ascending, below
 * max_streams; NULL: i) */
int jsmpeg_hip_resampler_resample(jsmpeg_hip_resampler_t *rs, const void *const *pcm, const uint32_t *frames, const uint32_t *stream_numbers,
                                  uint32_t n_streams, uint32_t flags, void *hip_stream);
int jsmpeg_hip_resampler_sync(jsmpeg_hip_resampler_t *rs);
/* 1: no pass in flight, 0: still running; never waits */
int jsmpeg_hip_resampler_query(jsmpeg_hip_resampler_t *rs);
/* the last call's buffer on the device and its bytes: closed form, NO wait -- the contents are there once the pass has
 * finished, that is for work enqueued on the same hip_stream behind it, or after jsmpeg_hip_resampler_sync */
void *jsmpeg_hip_resampler_out(jsmpeg_hip_resampler_t *rs, uint64_t *bytes);
/* stream NUMBER `stream` in that buffer (0, 0: not in the call).  WAVEFORM: offset = the element index of its first channel's
 * row, count = its samples per channel; FRAMES: its first frame and its whole frames.  Closed form, no wait. */
int jsmpeg_hip_resampler_stream_out(jsmpeg_hip_resampler_t *rs, uint32_t stream, uint64_t *offset, uint64_t *count);
/* ends the chain of `stream` (UINT32_MAX: of every stream); refused while a pass is in flight */
int jsmpeg_hip_resampler_chain_reset(jsmpeg_hip_resampler_t *rs, uint32_t stream);
/* out[0]: the stream has chain state; out[1]: input samples per channel it has taken; out[2]: outputs it has made */
int jsmpeg_hip_resampler_chain_info(jsmpeg_hip_resampler_t *rs, uint32_t stream, uint64_t out[3]);
/* the last pass on the device: the kernel, the whole enqueue (with the upload of its stream list) */
int jsmpeg_hip_resampler_timings(jsmpeg_hip_resampler_t *rs, float out_ms[2]);
/* The plan of a pair, no device needed: L, M and the half width H (any may be NULL); < 0: not a supported pair */
int jsmpeg_hip_resample_plan(uint32_t in_rate, uint32_t out_rate, uint32_t *L, uint32_t *M, uint32_t *H);
/* its taps, L * 2 H floats [phase][tap], as the handle uploads them; no device needed */
int jsmpeg_hip_resample_taps(uint32_t in_rate, uint32_t out_rate, float *out);

/* ------------------------------------------------------------------ part 12
 * LOG-MEL FEATURES ON THE DEVICE: the last step between decoded audio and a speech model.  Float32 mono PCM in HBM -- part 11's
 * waveform, or any such buffer -- -> log-mel spectrograms [stream of the call][n_mels][row] (MEL_MAJOR, what Whisper reads) or
 * [stream of the call][row][n_mels] (TIME_MAJOR) in f32 / f16 / bf16.  The rule is stated once, in jsmpeg_amd/csrc/logmel.h.
 * In short: framing as torch.stft(center=True, pad_mode="reflect"), frame t covers [t hop - n_fft / 2, t hop + n_fft / 2); the
 * DFT is a GEMM against a basis with the window folded in (computed in double, rounded once), re and im each ONE k-ascending
 * float32 fmaf chain, done by v_mfma_f32_32x32x2_f32; power fmaf(re, re, im * im); mel sums in ascending bins; the header's own
 * logarithm.  A stream that has taken n samples has n <= n_fft / 2 ? 0 : (n - n_fft / 2) / hop + 1 frames while it is open and
 * n <= n_fft / 2 ? 0 : n / hop + 1 with END (torch refuses n <= n_fft / 2; here such a stream has no frame): CLOSED FORM, so a
 * call is ONE kernel (WHISPER: two) and a PURE ENQUEUE on hip_stream with an event at its end.  Columns at and behind a
 * stream's count hold the PAD VALUE, what a frame of zeros gets: 0 (POWER), the scale of floor (the logs), the stream's own
 * lower clamp (WHISPER).  A stream handed over in pieces, chained call after chained call, yields BIT FOR BIT the frames of one
 * call.  One pass at a time per handle; results are valid until the handle's next call.  A bad argument returns < 0 with
 * jsmpeg_hip_last_error, launches nothing and leaves the handle usable.  Without a device create returns NULL (no CPU
 * fallback).
 * OUT OF SCOPE: a Node binding, the magnitude (square-root) spectrogram, deltas, dithering, pre-emphasis. */
typedef struct jsmpeg_hip_logmel_t jsmpeg_hip_logmel_t;
#define JSMPEG_HIP_LOGMEL_POWER 0u       /* the linear mel power */
#define JSMPEG_HIP_LOGMEL_LOG 1u         /* ln max(mel, floor) */
#define JSMPEG_HIP_LOGMEL_LOG10 2u       /* log10 max(mel, floor) */
#define JSMPEG_HIP_LOGMEL_DB 3u          /* 10 log10 max(mel, floor) */
#define JSMPEG_HIP_LOGMEL_WHISPER 4u     /* (max(log10 max(mel, floor), M - 8) + 4) / 4, M the stream's largest log10 value of the call */
#define JSMPEG_HIP_LOGMEL_MEL_MAJOR 0u
#define JSMPEG_HIP_LOGMEL_TIME_MAJOR 1u
#define JSMPEG_HIP_LOGMEL_HTK 0u
#define JSMPEG_HIP_LOGMEL_SLANEY 1u
typedef struct jsmpeg_hip_logmel_config_t {
	uint32_t sample_rate;         /* 8000 .. 48000 Hz: the filterbank's only */
	uint32_t n_fft;               /* even, 32 .. 1024 */
	uint32_t hop;                 /* 1 .. n_fft / 2 */
	uint32_t n_mels;              /* 1 .. 256 */
	float f_min, f_max;           /* Hz; f_max 0: sample_rate / 2 */
	uint32_t mel_scale;           /* HTK or SLANEY */
	uint32_t mel_norm;            /* 0: none; 1: slaney, every filter divided by half its width in Hz */
	const float *window;          /* n_fft floats read at create; NULL: the periodic Hann window, computed in double */
	float floor;                  /* the logs take max(mel, floor); 0: 1e-10 */
	uint32_t scale, layout;
	uint32_t dtype;               /* JSMPEG_HIP_RESAMPLE_F32 / _F16 / _BF16: the float32 value rounded to nearest even */
	uint32_t max_streams;         /* per call, and the stream numbers of chained calls lie below it */
	uint32_t max_samples;         /* samples of ONE stream per call */
	uint32_t row;                 /* columns per stream of the output; 0: (max_samples + n_fft / 2) / hop + 2, what any call yields */
	int32_t device;               /* -1: current */
} jsmpeg_hip_logmel_config_t;
/* the call's streams end here: indices behind a stream's last sample reflect, and the frames up to n / hop come out.  With
 * CHAIN the chains of the call's streams end behind it; an END call with 0 new samples lets the tail frames come out. */
#define JSMPEG_HIP_LOGMEL_END 1u
/* CONTINUE the call's streams: the handle keeps, per stream number, whether the stream has state, the samples it has taken,
 * and which of two carries on the device holds the samples that later frames and END's reflection can still read (at most
 * n_fft - 1; the exact rule: logmel.h).  A call reads one carry and writes the other.  A stream without samples in a call
 * keeps its state; a call without the flag starts from nothing and stores nothing.  Refused with the WHISPER scale, whose
 * maximum belongs to a whole call. */
#define JSMPEG_HIP_LOGMEL_CHAIN 2u
jsmpeg_hip_logmel_t *jsmpeg_hip_logmel_create(const jsmpeg_hip_logmel_config_t *config);
void jsmpeg_hip_logmel_destroy(jsmpeg_hip_logmel_t *lm);
/* stream i has samples[i] (0 allowed) float32 samples at the device address pcm[i] (4-byte aligned; ignored for 0 samples) and
 * the number stream_numbers[i] (strictly ascending, below max_streams; NULL: i) */
int jsmpeg_hip_logmel_features(jsmpeg_hip_logmel_t *lm, const void *const *pcm, const uint32_t *samples, const uint32_t *stream_numbers, uint32_t n_streams,
                               uint32_t flags, void *hip_stream);
int jsmpeg_hip_logmel_sync(jsmpeg_hip_logmel_t *lm);
/* 1: no pass in flight, 0: still running; never waits */
int jsmpeg_hip_logmel_query(jsmpeg_hip_logmel_t *lm);
/* the last call's buffer on the device and its bytes (streams of the call * n_mels * row elements): closed form, NO wait */
void *jsmpeg_hip_logmel_out(jsmpeg_hip_logmel_t *lm, uint64_t *bytes);
/* stream NUMBER `stream` in that buffer (0, 0: not in the call): the element index of its first row and its frames.  No wait. */
int jsmpeg_hip_logmel_stream_out(jsmpeg_hip_logmel_t *lm, uint32_t stream, uint64_t *offset, uint64_t *count);
/* ends the chain of `stream` (UINT32_MAX: of every stream); refused while a pass is in flight */
int jsmpeg_hip_logmel_chain_reset(jsmpeg_hip_logmel_t *lm, uint32_t stream);
/* out[0]: the stream has chain state; out[1]: samples it has taken; out[2]: frames it has made */
int jsmpeg_hip_logmel_chain_info(jsmpeg_hip_logmel_t *lm, uint32_t stream, uint64_t out[3]);
/* the last pass on the device: the kernels, the whole enqueue (with the upload of its stream list) */
int jsmpeg_hip_logmel_timings(jsmpeg_hip_logmel_t *lm, float out_ms[2]);
/* The tables of a config, no device needed (max_streams, max_samples and device are not looked at).
 * plan: out = { bins, padded columns of the basis, frames of n samples open, frames of n samples with END, frames per
 * workgroup, LDS bytes of a workgroup, floats per carry, row }. */
int jsmpeg_hip_logmel_plan(const jsmpeg_hip_logmel_config_t *config, uint64_t n, uint64_t out[8]);
/* the basis as the handle uploads it: [n_fft][padded columns], column 2 b = w cos, 2 b + 1 = -w sin, zeros behind 2 bins */
int jsmpeg_hip_logmel_basis(const jsmpeg_hip_logmel_config_t *config, float *out);
/* the filterbank [n_mels][bins] and the ranges [n_mels][2] = lo, hi of each row's nonzero span (either may be NULL) */
int jsmpeg_hip_logmel_filters(const jsmpeg_hip_logmel_config_t *config, float *fb, int32_t *ranges);

/* Last error of the calling thread ("" if none). */
const char *jsmpeg_hip_last_error(void);
/* Number of visible HIP devices (0 if none / runtime unusable). */
int jsmpeg_hip_device_count(void);

#ifdef __cplusplus
}
#endif
#endif
