/*
 * INTERNAL: how the TS program mux (ts_program.hip, part 10) reaches the last call of the two encoders without a host
 * turn-around -- their device buffers and, per unit, what the HOST knows at enqueue time (stream numbers, ordinals, closed-form
 * audio ranges).  Nothing here waits for the device.  Not installed; nothing outside jsmpeg_amd/csrc includes it.
 */
#pragma once
#include <stdint.h>

#include "enc_ts.h"
#include "jsmpeg_hip.h"

struct JmTspVideoSource {
	uint32_t count;              /* pictures of the encoder's last call */
	uint32_t max_streams, frame_rate_code;
	int device;
	const uint8_t *d_es;         /* the bytes the units' offsets count from */
	const uint64_t *d_result;    /* total | status of that call's ES, on the device: status != 0 after an ES overflow */
};
/* the last call of `enc` (encode.hip): fills stream[k], ordinal[k] (the chain's) for k < count <= cap; < 0 without a call */
int jm_enc_tsp_source(jsmpeg_hip_encoder_t *enc, JmTspVideoSource *out, uint32_t *stream, uint32_t *ordinal, uint32_t cap);
/* enqueues k_ts_units over that call's picture table: unit k = picture k's range (the end code as set_ts does it) with d_pts[k] */
int jm_enc_tsp_units(jsmpeg_hip_encoder_t *enc, JmTsUnit *d_units, const uint64_t *d_pts, void *hip_stream);

struct JmTspAudioSource {
	uint32_t count;              /* frames of the encoder's last call */
	uint32_t max_streams, sample_rate;
	int device;
	const uint8_t *d_es;
};
/* the last call of `enc` (mp2_encode.hip): fills offset, bytes, stream, ordinal per frame k < count <= cap; < 0 without a call */
int jm_mp2e_tsp_source(jsmpeg_hip_mp2_encoder_t *enc, JmTspAudioSource *out, uint64_t *offset, uint32_t *bytes, uint32_t *stream, uint64_t *ordinal, uint32_t cap);
