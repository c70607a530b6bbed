/*
 * MPEG-1 ENCODER, P CHAINS AND GOP BUDGETS ACROSS CALLS (include/jsmpeg_hip.h part 8, JSMPEG_HIP_ENC_CHAIN): which ordinal,
 * which reference and which reconstruction store a picture of a call has, stated once, host + device -- what the host side of
 * encode.hip and the CPU simulator's chained calls (tests/sim/sim_encode_pass.cpp, sim_chain_encode) share: the plan of a whole
 * call (jm_encc_plan_call), its pictures by level (jm_encc_levels), a frame number's address (jm_encc_frame) and the `spent`
 * row a pick reads (jm_encc_spent_row).  Nothing here reads the device: a pass stays a pure enqueue.
 *
 * CHAIN.  A handle keeps a JmEncChain per stream number s < max_streams: `have` (the stream has chain state), `n` (the pictures
 *    coded so far = the ordinal of the next one), `parity` (which of the stream's two CARRY FRAMES holds its last
 *    reconstruction) and `rated` (the stream's device-side `spent` is that of its last call: that call ran with rate control).
 *    The stream number IS the stream's identity from call to call.
 *    A call WITHOUT the flag uses no record: it reads none and writes none; ordinals begin at 0 in every stream (jm_encc_plan
 *    with c == NULL states what such a call always did).
 *    A call WITH the flag continues its streams: the first picture of stream s has ordinal n[s], or 0 when have[s] is false,
 *    and the ordinal drives the level (ordinal % gop), the type, the temporal reference and the GOP's time code as ever: the
 *    call's first picture is a P picture unless n[s] % gop == 0.  Afterwards have[s] is true and n[s] has grown by the stream's
 *    pictures in the call.  WRAP: the ordinal behind `o` is o + 1, except that a GOP which would begin above JM_ENCC_WRAP
 *    (2^32 - 1 - 1024; gop <= 1024, so there is one before 2^32) begins at ordinal 0 instead (jm_encc_next).
 *    The chain of a stream ENDS -- its next picture has ordinal 0 and is an I picture with sequence and GOP header -- by
 *    JSMPEG_HIP_ENC_END together with the flag (every stream of the call, the end code written), jsmpeg_hip_encoder_chain_reset,
 *    jsmpeg_hip_encoder_set_gop (every stream: levels and forward_f_code change) and a chained call that overflowed (every
 *    stream of that call, when the pass is settled).
 *
 * WHERE.  An unchained call reconstructs picture k into frame k of the call's store and a P picture reads frame k - 1.  A
 *    chained call does the same, except that the LAST picture of stream s in the call is reconstructed straight into carry
 *    frame (s, parity ^ 1) and the FIRST one, if it is a P picture, reads carry frame (s, parity); then parity flips.  No frame
 *    is copied.  Two frames per stream: the write kernel reads the reference again at the end of the pass, and in a call with
 *    one picture per stream that picture reads one carry frame and writes the other.  A JmEncPlan names a frame by a number:
 *    k, or JM_ENCC_SLOT | (2 * s + parity).  An I picture's `ref` is its own `recon` (never read).
 *
 * RATE (enc_rate.h's rule across calls).  In a chained call m = gop for every picture: a GOP is assumed to be completed by
 *    later calls, the call's last GOP is not cut short.  `before` is how many pictures of the picture's GOP lie in front of it IN
 *    THE CALL (their bytes are summed there); the others were coded by earlier calls, and their bytes are the stream's `spent`
 *    on the device, two words per stream taken in turns like the carry frames: JM_ENCC_READ (add spent[parity][s]; only when
 *    the record is `rated` -- bytes coded by a call without rate control, and those before them, are not counted),
 *    JM_ENCC_WRITE (the stream's last picture of the call: spent[parity ^ 1][s] = its spent + its bytes).  In turns, because a
 *    stream's first and last picture of a call can be of the same level, picked by one launch.
 */
#pragma once
#include <stdint.h>

#include "mpeg1_dev.h"

#define JM_ENCC_WRAP (0xffffffffu - 1024u)
#define JM_ENCC_SLOT 0x80000000u
#define JM_ENCC_READ 1u
#define JM_ENCC_WRITE 2u
#define JM_ENCC_ODD 4u           /* parity 1: read spent[1], write spent[0] */

struct JmEncChain { uint32_t have, n, parity, rated; };

struct JmEncPlan {
	uint32_t ordinal;
	uint32_t last;               /* the last picture of its stream in this call */
	uint32_t m;                  /* the pictures its GOP is budgeted for (rate control) */
	uint32_t before;             /* pictures of its GOP in front of it in this call */
	uint32_t carry;              /* JM_ENCC_READ | JM_ENCC_WRITE | JM_ENCC_ODD */
	uint32_t ref, recon;         /* frame numbers: k, or JM_ENCC_SLOT | (2 * stream + parity) */
};

JM_HD uint32_t jm_encc_next(uint32_t ordinal, uint32_t gop) {
	const uint32_t next = ordinal + 1u;
	return (next % gop == 0 && next > JM_ENCC_WRAP) ? 0u : next;
}

JM_HD void jm_encc_reset(JmEncChain &c) { c.have = 0; c.n = 0; c.parity = 0; c.rated = 0; }

/* The n pictures k0 .. k0 + n - 1 of a call that are stream `stream`; c: the stream's record, NULL in an unchained call;
 * rate: the call runs with rate control. */
JM_HD void jm_encc_plan(const JmEncChain *c, uint32_t stream, bool rate, uint32_t gop, uint32_t k0, uint32_t n, JmEncPlan *out) {
	uint32_t o = (c && c->have) ? c->n : 0u;
	const uint32_t parity = c ? c->parity & 1u : 0u;
	for (uint32_t i = 0; i < n; i++) {
		JmEncPlan &p = out[i];
		const uint32_t level = o % gop;
		p.ordinal = o;
		p.last = i + 1 == n ? 1u : 0u;
		p.before = level < i ? level : i;
		p.recon = (c && p.last) ? (JM_ENCC_SLOT | (2u * stream + (parity ^ 1u))) : k0 + i;
		p.ref = level == 0 ? p.recon : (i ? k0 + i - 1u : (JM_ENCC_SLOT | (2u * stream + parity)));
		p.carry = 0;
		if (c) {
			p.m = gop;
			if (rate) p.carry = ((p.before < level && c->rated) ? JM_ENCC_READ : 0u) | (p.last ? JM_ENCC_WRITE : 0u) | (parity ? JM_ENCC_ODD : 0u);
			o = jm_encc_next(o, gop);
		} else {
			const uint32_t rest = n - (i - level);               /* the stream's last GOP in the call is cut short */
			p.m = gop < rest ? gop : rest;
			o++;
		}
	}
}

/* the record behind a call whose last picture of the stream was `last`; end: the call closed its streams */
JM_HD void jm_encc_advance(JmEncChain &c, const JmEncPlan &last, bool rate, bool end, uint32_t gop) {
	if (end) { jm_encc_reset(c); return; }
	c.have = 1; c.n = jm_encc_next(last.ordinal, gop); c.parity = (c.parity & 1u) ^ 1u; c.rated = rate ? 1u : 0u;
}

/* THE CALL'S PLAN, stream by stream: ordinals, GOP sizes and where the reconstructions lie for the `count` pictures of a call
 * whose stream numbers ascend (stream == NULL: all stream 0), and the records advanced behind it.  chain: the handle's records,
 * [max_streams]; an unchained call reads and writes none. */
inline void jm_encc_plan_call(const uint32_t *stream, uint32_t count, JmEncChain *chain, bool rate, uint32_t gop, bool chained, bool end, JmEncPlan *plan) {
	for (uint32_t k0 = 0; k0 < count;) {
		const uint32_t s = stream ? stream[k0] : 0;
		uint32_t n = 1;
		while (k0 + n < count && (!stream || stream[k0 + n] == s)) n++;
		jm_encc_plan(chained ? &chain[s] : nullptr, s, rate, gop, k0, n, &plan[k0]);
		if (chained) jm_encc_advance(chain[s], plan[k0 + n - 1], rate, end, gop);
		k0 += n;
	}
}

/* The call's pictures by level = ordinal mod gop, a counting sort: list[begin[l] .. begin[l + 1]) are the pictures of level l in
 * the call's order.  list: [count], begin: [gop + 1].  Returns the number of levels the call has. */
inline uint32_t jm_encc_levels(const JmEncPlan *plan, uint32_t count, uint32_t gop, uint32_t *list, uint32_t *begin) {
	uint32_t levels = 0;
	for (uint32_t l = 0; l <= gop; l++) begin[l] = 0;
	for (uint32_t k = 0; k < count; k++) {
		const uint32_t l = plan[k].ordinal % gop;
		begin[l + 1]++;
		if (l + 1 > levels) levels = l + 1;
	}
	for (uint32_t l = 0; l < levels; l++) begin[l + 1] += begin[l];
	for (uint32_t k = 0; k < count; k++) list[begin[plan[k].ordinal % gop]++] = k;      /* begin[l] is now where level l ends */
	for (uint32_t l = levels; l > 0; l--) begin[l] = begin[l - 1];
	begin[0] = 0;
	return levels;
}

/* where frame number `frame` of a JmEncPlan lies: store: the call's frames, carry: the streams' carry frames */
JM_HD uint8_t *jm_encc_frame(uint32_t frame, uint8_t *store, uint8_t *carry, size_t frame_bytes) {
	return (frame & JM_ENCC_SLOT) ? carry + (size_t)(frame & ~JM_ENCC_SLOT) * frame_bytes : store + (size_t)frame * frame_bytes;
}

/* spent[2][max_streams]: the row a pick with `carry` reads (JM_ENCC_READ); the one it leaves (JM_ENCC_WRITE) is the other, row ^ 1 */
JM_HD uint32_t jm_encc_spent_row(uint32_t carry) { return (carry & JM_ENCC_ODD) ? 1u : 0u; }
