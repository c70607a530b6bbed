/*
 * MPEG-1 encoder on the device (include/jsmpeg_hip.h part 8): frames in HBM, or RGB tensors, to elementary streams of I and P
 * pictures that a jsmpeg player, the reference decoder and this library's own batch / live front ends read.  The arithmetic is
 * enc_block.h's, enc_motion.h's, enc_rate.h's and enc_chain.h's, what a lane of a kernel does around it is enc_pass.h's -- all
 * shared with the CPU simulator (tests/sim/sim_encode_pass.cpp); here are the kernels (those whose lanes work alone: their LDS,
 * their guards and one call of their body), the pass as a pure enqueue, and the TS mux: on the device behind the pass
 * (jsmpeg_hip_encoder_set_ts), over any device bytes (jsmpeg_hip_ts_mux_device) and on the host -- one rule, enc_ts.h.
 *
 * A pass on the caller's stream, every size and offset worked out on the device:
 *   k_enc_rgb            tensor input only: RGB -> Y | Cr | Cb of the coded size in the encoder's frame store
 *   k_enc_scale          scaled input only: planes of another size, cropped and scaled into the same store (the rule: enc_scale.h)
 *   k_enc_mosaic         mosaic input only: one picture of the store composed from many sources (the rule: enc_mosaic.h)
 *   k_enc_measure        a macroblock per lane: transform, quantise, count bits; 12 bytes per macroblock out
 *   k_enc_scan_slices    a slice per lane: the macroblocks' bit offsets (their DC codes depend on the predecessor), the slice's bytes
 *   k_enc_scan_pictures  a picture per lane: the slices' offsets, the picture's bytes
 *   k_enc_place          one workgroup: the pictures' and streams' offsets in the output, the total, the overflow flag
 *   k_enc_clear          zeroes the total (the write ORs into it), 0xff behind it
 *   k_enc_write          a macroblock per lane again: transform, quantise, write bits; the headers by the lanes that begin them
 * The host waits in jsmpeg_hip_encoder_sync and the readers only.
 *
 * With TS on (jsmpeg_hip_encoder_set_ts; the rule: enc_ts.h) three more kernels follow the write, in the same enqueue:
 *   k_ts_units           a picture per lane: the unit table -- unit k is picture k's range, a stream's last picture of a call with
 *                        JSMPEG_HIP_ENC_END runs on over the end code -- with the PTS values the host uploaded
 *   k_ts_plan            one workgroup, shaped like k_enc_place: per unit its packets, TS offset and first continuity counter, per
 *                        stream its range, the total, the overflow flag; the streams' counter words, read and -- unless the call
 *                        overflowed -- written back
 *   k_ts_write           a fixed grid over (packets) x 47 dwords: the unit by binary search, the dword by jm_ts_dword, the source
 *                        bytes from aligned dwords and v_alignbyte; plain stores, one owner per dword
 * EXTRA DEVICE MEMORY, allocated by jsmpeg_hip_encoder_set_ts: max_ts_bytes, 56 bytes per picture of max_pictures and 28 bytes
 * per stream of max_streams.
 *
 * With a GOP (jsmpeg_hip_encoder_set_gop, gop > 1; the rules: enc_motion.h) the measure step becomes a loop over LEVELS,
 * level = a picture's ordinal in its stream mod gop: all pictures of a level, of every stream, in one launch each of
 *   k_enc_motion         P levels: a wavefront per macroblock searches the reconstruction of the picture before
 *   k_enc_measure_p      a macroblock per lane: mode, residual, quantise, count, reconstruct into the per-picture store
 * then k_enc_scan_slices_p / k_enc_scan_pictures_p (the neighbour-dependent codes, the kinds), place and clear as above, and
 * ONE k_enc_write_p over every macroblock of the call: it recomputes a macroblock's levels from the source and the kept
 * reconstruction of the picture before.  The host builds the level lists from the stream numbers; it never reads the device.
 *
 * With RATE CONTROL (jsmpeg_hip_encoder_set_rate; the rule: enc_rate.h) the pass is always the level loop, also at gop 1, and
 * per level, between k_enc_motion and k_enc_measure_p, the quantiser scale of the level's pictures is chosen on the device:
 *   k_enc_rate_measure   a macroblock per lane: each block transformed once, quantised and counted at every scale of the range;
 *                        16 bits per (macroblock, scale) out
 *   k_enc_rate_scan      a (picture, slice, scale) per lane: the slice's walk over those records, its bytes
 *   k_enc_rate_pick      a wavefront per picture, lanes over the scales: the picture's bytes at each, the budget from the final
 *                        bytes of its GOP's earlier levels, the smallest scale that fits -- into the picture's JmEncPic::q
 * and the kernels behind them read that q as they read the caller's.  EXTRA DEVICE MEMORY, allocated by the first
 * jsmpeg_hip_encoder_set_rate that switches rate control on: per picture of max_pictures 62 bytes per macroblock (31 records of
 * 16 bits; 506 KB at 1080p), 124 bytes per macroblock row and 16 bytes -- and the stores of a GOP, if they are not there yet.
 *
 * ACROSS CALLS (JSMPEG_HIP_ENC_CHAIN; the rule: enc_chain.h) a stream's P chain and its GOP's budget go on where the call before
 * left them.  No kernel of its own and no copy: every picture carries the addresses of its reference and of its reconstruction
 * (JmEncPic::ref, ::recon, filled by the host, which needs nothing from the device for it), a chained stream's last picture
 * of a call is reconstructed into one of the stream's two carry frames and the next call's first picture reads it there;
 * k_enc_rate_pick adds the bytes the GOP's pictures took in earlier calls and leaves the sum for the next one.  EXTRA DEVICE
 * MEMORY, allocated by the first chained call that runs the level loop: two frames and 16 bytes per stream of max_streams.
 */
#include "engine_internal.h"
#include "enc_pass.h"
#include "enc_scale.h"
#include "enc_mosaic.h"
#include "enc_ts.h"
#include "ts_prog_sources.h"

#define JM_ENC_LANES 64
#define JM_ENC_MOTION_WAVES 4    /* macroblocks (one wavefront each) of a k_enc_motion workgroup */

/* ------------------------------------------------------------------ kernels */

__global__ void __launch_bounds__(256) k_enc_rgb(JmEncArgs a, const uint8_t *rgb, uint32_t layout, uint32_t order) {
	const uint32_t qw = a.cw >> 1, qh = a.ch >> 1;
	const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (g >= (uint64_t)a.count * qw * qh) return;
	const uint32_t k = (uint32_t)(g / ((uint64_t)qw * qh)), r = (uint32_t)(g % ((uint64_t)qw * qh));
	jm_enc_rgb_quad(rgb + (size_t)k * a.width * a.height * 3, layout, order, a.width, a.height, r % qw, r / qw,
	                const_cast<uint8_t *>(a.pics[k].frame), a.cw, a.ch);
}

/* Scaled input (the rule, the table and the tile plan: enc_scale.h; the CPU simulator tests/sim/sim_encode_scale.cpp runs the
 * same taps pixel by pixel).  A workgroup owns a tile of JM_ES_TW x JM_ES_TH samples of one plane of the CODED size of one
 * picture -- a sample beyond the scaled picture takes the taps of the last column / row, which is the edge replication -- and
 * walks the source rows its vertical taps need in chunks of at most JM_ES_CR rows, as k_tensor does:
 *   1. stage: the chunk's rows of the tile's source span into LDS, 16-byte loads from the coded luma row, 8-byte loads from
 *      the chroma row (its stride is a multiple of 8 only);
 *   2. horizontal pass: thread = output column (two row groups), each weight read once for the thread's 16 rows of the chunk,
 *      into LDS as 16-bit t;
 *   3. vertical pass: a thread owns four adjacent columns of four rows of the tile; the chunk's rows inside their taps are added
 *      in registers, across chunks.
 * Then a whole word per thread and row is stored.  The weights come from the host's table (built by enc_scale.h's functions
 * in pinned memory, uploaded on the call's stream).  Any number of taps works: a source row is at most 4096 bytes, so a chunk
 * has at least four rows.  24.25 KiB of LDS. */
struct JmEncScaleArgs {
	JmEsPlan plan;
	const uint8_t *const *src;   /* [count]: the source frames */
	const uint32_t *tab;
};

__global__ void __launch_bounds__(256) k_enc_scale(JmEncArgs a, JmEncScaleArgs s) {
	__shared__ __attribute__((aligned(16))) uint8_t src[JM_ES_SRC];
	__shared__ __attribute__((aligned(16))) uint16_t ts[JM_ES_CR][JM_ES_TW];
	__shared__ uint32_t vt[JM_ES_TH][2];
	const uint32_t nl = s.plan.pl[0].tiles_x * s.plan.pl[0].tiles_y, nc = s.plan.pl[1].tiles_x * s.plan.pl[1].tiles_y;
	uint32_t tile = blockIdx.x, comp = 0;
	if (tile >= nl) { tile -= nl; comp = 1; if (tile >= nc) { tile -= nc; comp = 2; } }
	const JmEsPlane q = comp ? s.plan.pl[1] : s.plan.pl[0];
	const uint32_t ox0 = (tile % q.tiles_x) * JM_ES_TW, oy0 = (tile / q.tiles_x) * JM_ES_TH;
	const uint32_t nw = min(JM_ES_TW, q.out_w - ox0), nh = min(JM_ES_TH, q.out_h - oy0);
	const uint32_t *ex = s.tab + q.ent_x, *ey = s.tab + q.ent_y;
	const uint16_t *wt = reinterpret_cast<const uint16_t *>(s.tab + s.plan.wts);
	const uint32_t tid = threadIdx.x;
	if (tid < nh) {
		const uint32_t i = min(oy0 + tid, q.ay.n_out - 1u);
		vt[tid][0] = ey[2u * i]; vt[tid][1] = ey[2u * i + 1u];
	}
	const uint32_t col = tid & (JM_ES_TW - 1u), rg = tid / JM_ES_TW;
	const bool hcol = col < nw;
	const uint32_t ci = min(ox0 + min(col, nw - 1u), q.ax.n_out - 1u);
	const uint32_t he = ex[2u * ci], hoff = ex[2u * ci + 1u], hsize = he >> 16;
	/* the tile's source rectangle (xmin and xmin + xsize do not decrease with the output index) */
	const uint32_t ef = ex[2u * ox0], el = ex[2u * min(ox0 + nw - 1u, q.ax.n_out - 1u)];
	const uint32_t vf = ey[2u * oy0], vl = ey[2u * min(oy0 + nh - 1u, q.ay.n_out - 1u)];
	const uint32_t gran = comp ? 8u : 16u;
	const uint32_t ax0 = (q.x0 + (ef & 0xffffu)) & ~(gran - 1u), ax1 = (q.x0 + (el & 0xffffu) + (el >> 16) + gran - 1u) & ~(gran - 1u);
	const uint32_t stride = ax1 - ax0, cr_max = min(JM_ES_CR, JM_ES_SRC / stride);
	const uint32_t sy0 = vf & 0xffffu, sy1 = (vl & 0xffffu) + (vl >> 16);
	const uint32_t hbase = q.x0 - ax0 + (he & 0xffffu);
	const uint32_t src_off = comp == 0 ? 0u : comp == 1 ? s.plan.src_luma : s.plan.src_luma + s.plan.src_chroma;
	const uint32_t out_off = comp == 0 ? 0u : comp == 1 ? s.plan.out_luma : s.plan.out_luma + s.plan.out_chroma;
	for (uint32_t k = blockIdx.y; k < a.count; k += gridDim.y) {
		const uint8_t *P = s.src[k] + src_off + (size_t)q.y0 * q.src_w + ax0;
		uint8_t *O = const_cast<uint8_t *>(a.pics[k].frame) + out_off;
		uint32_t acc[4][4] = {};
		for (uint32_t r0 = sy0; r0 < sy1; r0 += cr_max) {
			const uint32_t cn = min(cr_max, sy1 - r0);
			__syncthreads();                                       /* the last chunk's (or picture's) readers are done */
			if (comp == 0) {
				const uint32_t gpr = stride / 16u;
				for (uint32_t g = tid; g < cn * gpr; g += 256u) {
					const uint32_t r = g / gpr, x = (g - r * gpr) * 16u;
					*reinterpret_cast<uint4 *>(src + r * stride + x) = *reinterpret_cast<const uint4 *>(P + (size_t)(r0 + r) * q.src_w + x);
				}
			} else {
				const uint32_t gpr = stride / 8u;
				for (uint32_t g = tid; g < cn * gpr; g += 256u) {
					const uint32_t r = g / gpr, x = (g - r * gpr) * 8u;
					*reinterpret_cast<uint2 *>(src + r * stride + x) = *reinterpret_cast<const uint2 *>(P + (size_t)(r0 + r) * q.src_w + x);
				}
			}
			__syncthreads();
			if (hcol) {
				uint32_t h[JM_ES_CR / 2u] = {};
				for (uint32_t j = 0; j < hsize; j++) {
					const uint32_t w = wt[hoff + j];
#pragma unroll
					for (uint32_t i = 0; i < JM_ES_CR / 2u; i++) h[i] += w * src[min(rg + 2u * i, cn - 1u) * stride + hbase + j];
				}
#pragma unroll
				for (uint32_t i = 0; i < JM_ES_CR / 2u; i++)
					if (rg + 2u * i < cn) ts[rg + 2u * i][col] = (uint16_t)jm_es_round_h(h[i]);
			}
			__syncthreads();
#pragma unroll
			for (uint32_t i = 0; i < 4u; i++) {
				const uint32_t idx = tid + 256u * i, ol = idx / (JM_ES_TW / 4u), cg = idx % (JM_ES_TW / 4u);
				if (ol >= nh || cg * 4u >= nw) continue;
				const uint32_t xmin = vt[ol][0] & 0xffffu, xsize = vt[ol][0] >> 16, woff = vt[ol][1];
				const uint32_t lo = max(xmin, r0), hi = min(xmin + xsize, r0 + cn);
				for (uint32_t sr = lo; sr < hi; sr++) {
					const uint32_t w = wt[woff + sr - xmin];
					const uint2 v = *reinterpret_cast<const uint2 *>(&ts[sr - r0][cg * 4u]);
					acc[i][0] += w * (v.x & 0xffffu); acc[i][1] += w * (v.x >> 16);
					acc[i][2] += w * (v.y & 0xffffu); acc[i][3] += w * (v.y >> 16);
				}
			}
		}
#pragma unroll
		for (uint32_t i = 0; i < 4u; i++) {
			const uint32_t idx = tid + 256u * i, ol = idx / (JM_ES_TW / 4u), cg = idx % (JM_ES_TW / 4u);
			if (ol >= nh || cg * 4u >= nw) continue;
			*reinterpret_cast<uint32_t *>(O + (size_t)(oy0 + ol) * q.out_w + ox0 + cg * 4u) =
				jm_es_round_v(acc[i][0]) | (jm_es_round_v(acc[i][1]) << 8) | (jm_es_round_v(acc[i][2]) << 16) | (jm_es_round_v(acc[i][3]) << 24);
		}
	}
}

/* Mosaic input (the rule, the table and the tile plan: enc_mosaic.h; the CPU simulator tests/sim/sim_encode_mosaic.cpp pastes
 * the same samples pixel by pixel).  A workgroup owns a tile of JM_ES_TW x JM_ES_TH samples of one plane of the coded size of
 * one picture and composes it in LDS: the fill, then -- for each cell in index order whose rectangle in this plane meets the
 * tile and whose frame is there (found by the first wavefront, a cell per lane) -- k_enc_scale's three steps over the
 * intersection (stage the source rows in chunks, horizontal pass, vertical pass across chunks in registers; the cell's entries
 * at cell-local indices), the result written over the composed bytes.  Every byte of the tile is this workgroup's, so overlapping cells are ordered by its barriers alone.  Then
 * the last display column and row are replicated into the coded margin (every tile holds one of each: enc_mosaic.h TILES) and
 * whole words are stored, once per word.  28.25 KiB of LDS: k_enc_scale's 24.25 and the composed tile. */
/* src_frames: [count][p.n], the cells' frames, NULL = absent; tab: the layout's table.  Both are parameters of their own and restrict:
 * nothing the kernel stores goes through them, so what is read from them stays in scalar registers across the barriers. */
static_assert(JM_EM_MAX_CELLS == 64u, "k_enc_mosaic finds a tile's cells with one wavefront, a cell per lane");
__global__ void __launch_bounds__(256) k_enc_mosaic(JmEncArgs a, JmEmPlan p, const uint8_t *const *__restrict__ src_frames,
                                                    const uint32_t *__restrict__ tab) {
	__shared__ __attribute__((aligned(16))) uint8_t src[JM_ES_SRC];
	__shared__ __attribute__((aligned(16))) uint16_t ts[JM_ES_CR][JM_ES_TW];
	__shared__ uint32_t vt[JM_ES_TH][2];
	__shared__ __attribute__((aligned(16))) uint8_t comp[JM_ES_TH][JM_ES_TW];
	__shared__ uint32_t hit[2];      /* the cells of this picture that meet the tile, a bit each */
	const uint32_t nl = p.tiles_x[0] * p.tiles_y[0], nc = p.tiles_x[1] * p.tiles_y[1];
	uint32_t tile = blockIdx.x, plane = 0;
	if (tile >= nl) { tile -= nl; plane = 1; if (tile >= nc) { tile -= nc; plane = 2; } }
	const uint32_t ck = plane ? 1u : 0u;
	const uint32_t out_w = p.out_w[ck], out_h = p.out_h[ck];
	const uint32_t ox0 = (tile % p.tiles_x[ck]) * JM_ES_TW, oy0 = (tile / p.tiles_x[ck]) * JM_ES_TH;
	const uint32_t nw = min(JM_ES_TW, out_w - ox0), nh = min(JM_ES_TH, out_h - oy0);
	/* the display samples of the tile: vw x vh, at least 1 x 1 */
	const uint32_t vw = min(nw, p.disp_w[ck] - ox0), vh = min(nh, p.disp_h[ck] - oy0);
	const uint32_t tid = threadIdx.x;
	/* rg is the same in all 64 lanes of a wavefront.  Read as a scalar, the 16 row offsets of the horizontal pass live in scalar
	 * registers; as a per-lane value they took 16 vector registers which, beside acc[][] and a cell's values, left the compiler
	 * none under the 128 of four wavefronts per SIMD to keep the tap's 16 LDS reads in flight together: it issued them one at a
	 * time, each waited for (profiles/enc_mosaic_notes.md). */
	const uint32_t col = tid & (JM_ES_TW - 1u), rg = (uint32_t)__builtin_amdgcn_readfirstlane((int)(tid / JM_ES_TW));
	const uint32_t gran = plane ? 8u : 16u;
	const uint32_t out_off = plane == 0 ? 0u : plane == 1 ? p.out_luma : p.out_luma + p.out_chroma;
	const uint32_t fill4 = ((p.fill >> (8u * plane)) & 0xffu) * 0x01010101u;
	const JmEmCellRec *recs = reinterpret_cast<const JmEmCellRec *>(tab);
	for (uint32_t k = blockIdx.y; k < a.count; k += gridDim.y) {
		uint8_t *O = const_cast<uint8_t *>(a.pics[k].frame) + out_off;
		__syncthreads();                                           /* the last picture's readers of comp are done */
#pragma unroll
		for (uint32_t i = 0; i < 4u; i++) reinterpret_cast<uint32_t *>(&comp[0][0])[tid + 256u * i] = fill4;
		/* which cells meet the tile: the first wavefront, a cell per lane (JM_EM_MAX_CELLS is its 64 lanes) */
		if (tid < 64u) {
			bool meets = false;
			if (tid < p.n && src_frames[(size_t)k * p.n + tid]) {
				const JmEmCellRec &r = recs[tid];
				const uint32_t dx = plane ? r.dx >> 1 : r.dx, dy = plane ? r.dy >> 1 : r.dy;
				meets = max(dx, ox0) < min(dx + r.pl[ck].ax.n_out, ox0 + vw) && max(dy, oy0) < min(dy + r.pl[ck].ay.n_out, oy0 + vh);
			}
			const unsigned long long m = __ballot(meets);
			if (tid == 0) { hit[0] = (uint32_t)m; hit[1] = (uint32_t)(m >> 32); }
		}
		__syncthreads();
		uint32_t todo[2] = { (uint32_t)__builtin_amdgcn_readfirstlane((int)hit[0]), (uint32_t)__builtin_amdgcn_readfirstlane((int)hit[1]) };
		for (uint32_t half = 0; half < 2u; half++) while (todo[half]) {
			const uint32_t c = 32u * half + (uint32_t)__builtin_ctz(todo[half]);
			todo[half] &= todo[half] - 1u;
			const uint8_t *F = src_frames[(size_t)k * p.n + c];
			const JmEmCellRec &rec = recs[c];
			const JmEsPlane q = rec.pl[ck];
			const uint32_t dx = plane ? rec.dx >> 1 : rec.dx, dy = plane ? rec.dy >> 1 : rec.dy;
			/* the intersection of the cell and the tile's display samples, in plane coordinates: not empty */
			const uint32_t ix0 = max(dx, ox0), ix1 = min(dx + q.ax.n_out, ox0 + vw);
			const uint32_t iy0 = max(dy, oy0), iy1 = min(dy + q.ay.n_out, oy0 + vh);
			const uint32_t cw = ix1 - ix0, chh = iy1 - iy0;        /* <= JM_ES_TW, JM_ES_TH */
			const uint32_t lx0 = ix0 - dx, ly0 = iy0 - dy;         /* cell-local output indices of the intersection's corner */
			const uint32_t tx0 = ix0 - ox0, ty0 = iy0 - oy0;       /* ... and where it lies in the tile */
			const uint32_t *ex = tab + q.ent_x, *ey = tab + q.ent_y;
			const uint16_t *wt = reinterpret_cast<const uint16_t *>(tab + rec.wts);
			__syncthreads();                                       /* the last cell's readers of vt are done */
			if (tid < chh) { vt[tid][0] = ey[2u * (ly0 + tid)]; vt[tid][1] = ey[2u * (ly0 + tid) + 1u]; }
			const bool hcol = col < cw;
			const uint32_t ci = lx0 + min(col, cw - 1u);
			const uint32_t he = ex[2u * ci], hoff = ex[2u * ci + 1u], hsize = he >> 16;
			const uint32_t ef = ex[2u * lx0], el = ex[2u * (lx0 + cw - 1u)];
			const uint32_t vf = ey[2u * ly0], vl = ey[2u * (ly0 + chh - 1u)];
			const uint32_t ax0 = (q.x0 + (ef & 0xffffu)) & ~(gran - 1u), ax1 = (q.x0 + (el & 0xffffu) + (el >> 16) + gran - 1u) & ~(gran - 1u);
			const uint32_t stride = ax1 - ax0, cr_max = min(JM_ES_CR, JM_ES_SRC / stride);
			const uint32_t sy0 = vf & 0xffffu, sy1 = (vl & 0xffffu) + (vl >> 16);
			const uint32_t hbase = q.x0 - ax0 + (he & 0xffffu);
			const uint32_t src_luma = rec.src_luma;
			const uint32_t src_off = plane == 0 ? 0u : plane == 1 ? src_luma : src_luma + (src_luma >> 2);
			const uint8_t *P = F + src_off + (size_t)q.y0 * q.src_w + ax0;
			uint32_t acc[4][4] = {};
			for (uint32_t r0 = sy0; r0 < sy1; r0 += cr_max) {
				const uint32_t cn = min(cr_max, sy1 - r0);
				__syncthreads();                                   /* the last chunk's readers are done */
				if (plane == 0) {
					const uint32_t gpr = stride / 16u;
					for (uint32_t g = tid; g < cn * gpr; g += 256u) {
						const uint32_t r = g / gpr, x = (g - r * gpr) * 16u;
						*reinterpret_cast<uint4 *>(src + r * stride + x) = *reinterpret_cast<const uint4 *>(P + (size_t)(r0 + r) * q.src_w + x);
					}
				} else {
					const uint32_t gpr = stride / 8u;
					for (uint32_t g = tid; g < cn * gpr; g += 256u) {
						const uint32_t r = g / gpr, x = (g - r * gpr) * 8u;
						*reinterpret_cast<uint2 *>(src + r * stride + x) = *reinterpret_cast<const uint2 *>(P + (size_t)(r0 + r) * q.src_w + x);
					}
				}
				__syncthreads();
				if (hcol) {
					uint32_t h[JM_ES_CR / 2u] = {};
					for (uint32_t j = 0; j < hsize; j++) {
						const uint32_t w = wt[hoff + j];
#pragma unroll
						for (uint32_t i = 0; i < JM_ES_CR / 2u; i++) h[i] += w * src[min(rg + 2u * i, cn - 1u) * stride + hbase + j];
					}
#pragma unroll
					for (uint32_t i = 0; i < JM_ES_CR / 2u; i++)
						if (rg + 2u * i < cn) ts[rg + 2u * i][col] = (uint16_t)jm_es_round_h(h[i]);
				}
				__syncthreads();
				/* (columns of ts from cw up to the end of a thread's four were not written for this cell: what is summed from them
				 * is dropped where the composed bytes are written) */
#pragma unroll
				for (uint32_t i = 0; i < 4u; i++) {
					const uint32_t idx = tid + 256u * i, ol = idx / (JM_ES_TW / 4u), cg = idx % (JM_ES_TW / 4u);
					if (ol >= chh || cg * 4u >= cw) continue;
					const uint32_t xmin = vt[ol][0] & 0xffffu, xsize = vt[ol][0] >> 16, woff = vt[ol][1];
					const uint32_t lo = max(xmin, r0), hi = min(xmin + xsize, r0 + cn);
					for (uint32_t sr = lo; sr < hi; sr++) {
						const uint32_t w = wt[woff + sr - xmin];
						const uint2 v = *reinterpret_cast<const uint2 *>(&ts[sr - r0][cg * 4u]);
						acc[i][0] += w * (v.x & 0xffffu); acc[i][1] += w * (v.x >> 16);
						acc[i][2] += w * (v.y & 0xffffu); acc[i][3] += w * (v.y >> 16);
					}
				}
			}
			/* over the composed bytes (the cell before wrote them ahead of this cell's barriers) */
#pragma unroll
			for (uint32_t i = 0; i < 4u; i++) {
				const uint32_t idx = tid + 256u * i, ol = idx / (JM_ES_TW / 4u), cg = idx % (JM_ES_TW / 4u);
				if (ol >= chh || cg * 4u >= cw) continue;
#pragma unroll
				for (uint32_t j = 0; j < 4u; j++)
					if (cg * 4u + j < cw) comp[ty0 + ol][tx0 + cg * 4u + j] = (uint8_t)jm_es_round_v(acc[i][j]);
			}
		}
		__syncthreads();
#pragma unroll
		for (uint32_t i = 0; i < 4u; i++) {
			const uint32_t idx = tid + 256u * i, ol = idx / (JM_ES_TW / 4u), x = (idx % (JM_ES_TW / 4u)) * 4u;
			if (ol >= nh || x >= nw) continue;
			const uint8_t *row = comp[min(ol, vh - 1u)];
			const uint32_t v = x + 3u < vw ? *reinterpret_cast<const uint32_t *>(row + x)
			                               : (uint32_t)row[min(x, vw - 1u)] | ((uint32_t)row[min(x + 1u, vw - 1u)] << 8) |
			                                 ((uint32_t)row[min(x + 2u, vw - 1u)] << 16) | ((uint32_t)row[vw - 1u] << 24);
			*reinterpret_cast<uint32_t *>(O + (size_t)(oy0 + ol) * out_w + ox0 + x) = v;
		}
	}
}

__global__ void __launch_bounds__(JM_ENC_LANES) k_enc_measure(JmEncArgs a) {
	__shared__ int16_t zz[64 * JM_ENC_LANES];
	const uint64_t g = (uint64_t)blockIdx.x * JM_ENC_LANES + threadIdx.x;
	if (g >= (uint64_t)a.count * a.mbw * a.mbh) return;
	jm_pass_measure(a, g, zz + threadIdx.x, JM_ENC_LANES);
}

__global__ void __launch_bounds__(64) k_enc_scan_slices(JmEncArgs a) {
	const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
	if (s >= a.count * a.mbh) return;
	jm_pass_scan_slice(a, s);
}

__global__ void __launch_bounds__(64) k_enc_scan_pictures(JmEncArgs a) {
	const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
	if (k >= a.count) return;
	jm_pass_scan_picture(a, k);
}

/* one workgroup: 256 pictures at a time through LDS, lane 0 walks them */
__global__ void __launch_bounds__(256) k_enc_place(JmEncArgs a) {
	__shared__ uint32_t s_bytes[256], s_stream[256];
	__shared__ uint64_t s_off[256];
	__shared__ JmEncPlace place;
	uint64_t *sb = enc_stream_begin(a), *se = enc_stream_end(a);
	for (uint32_t i = threadIdx.x; i < a.max_streams; i += 256) { sb[i] = 0; se[i] = 0; }
	if (threadIdx.x == 0) place = jm_enc_place_begin();
	__syncthreads();
	for (uint32_t base = 0; base < a.count; base += 256) {
		const uint32_t k = base + threadIdx.x, n = min(256u, a.count - base);
		if (k < a.count) { s_bytes[threadIdx.x] = enc_pic_bytes(a)[k]; s_stream[threadIdx.x] = a.pics[k].stream; }
		__syncthreads();
		if (threadIdx.x == 0) {
			JmEncPlace p = place;
			for (uint32_t i = 0; i < n; i++) s_off[i] = jm_enc_place_picture(p, s_stream[i], s_bytes[i], a.end != 0, sb, se);
			place = p;
		}
		__syncthreads();
		if (k < a.count) enc_pic_off(a)[k] = s_off[threadIdx.x];
		__syncthreads();
	}
	if (threadIdx.x == 0) {
		JmEncPlace p = place;
		jm_enc_place_close(p, a.end != 0, se);
		a.result[0] = p.at;
		a.result[1] = p.at > a.cap ? 1u : 0u;
	}
}

__global__ void __launch_bounds__(256) k_enc_clear(JmEncArgs a) {
	if (a.result[1]) return;
	const uint64_t total16 = a.result[0] >> 4, n = total16 + (JM_ENC_TAIL >> 4);
	uint4 *out = reinterpret_cast<uint4 *>(a.words);
	for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
		const uint32_t v = i < total16 ? 0u : 0xffffffffu;
		out[i] = make_uint4(v, v, v, v);
	}
}

__global__ void __launch_bounds__(JM_ENC_LANES) k_enc_write(JmEncArgs a) {
	__shared__ int16_t zz[64 * JM_ENC_LANES];
	if (a.result[1]) return;
	const uint64_t g = (uint64_t)blockIdx.x * JM_ENC_LANES + threadIdx.x;
	if (g >= (uint64_t)a.count * a.mbw * a.mbh) return;
	jm_pass_write(a, g, zz + threadIdx.x, JM_ENC_LANES);
}

/* ------------------------------------------------------------------ kernels of the level loop (gop > 1, or rate control) */

static __device__ __forceinline__ uint64_t enc_wave_min(uint64_t v) {
#pragma unroll
	for (int o = 32; o; o >>= 1) { const uint64_t t = __shfl_xor((unsigned long long)v, o); v = t < v ? t : v; }
	return v;
}
static __device__ __forceinline__ uint32_t enc_wave_sum(uint32_t v) {
#pragma unroll
	for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o);
	return v;
}

/* A WAVEFRONT PER MACROBLOCK of the n pictures list[first ..]: the window and the macroblock staged in LDS, a lane per item
 * (dy, four dx sharing their dwords: 64 packed SADs per candidate, the unaligned dwords by v_alignbyte with constant shifts),
 * a wavefront min-reduction of the packed key; then the eight half-pel neighbours on eight lanes each, and the activity. */
__global__ void __launch_bounds__(64 * JM_ENC_MOTION_WAVES) k_enc_motion(JmEncArgs a, JmEncPArgs p, uint32_t first, uint32_t n) {
	__shared__ uint32_t s_win[JM_ENC_MOTION_WAVES][JM_ENCP_WIN_WORDS];
	__shared__ uint32_t s_cur[JM_ENC_MOTION_WAVES][64];
	const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u, mbs = a.mbw * a.mbh;
	const uint64_t total = (uint64_t)n * mbs;
	uint64_t g = (uint64_t)blockIdx.x * JM_ENC_MOTION_WAVES + wave;
	const bool live = g < total;
	if (!live) g = total - 1;                  /* a wavefront without a macroblock repeats the last one and stores nothing */
	const uint32_t k = p.list[first + (uint32_t)(g / mbs)], m = (uint32_t)(g % mbs), row = m / a.mbw, col = m % a.mbw;
	JM_GLOBAL const uint8_t *cur = (JM_GLOBAL const uint8_t *)a.pics[k].frame + ((size_t)row * 16u * a.cw + (size_t)col * 16u);
	JM_GLOBAL const uint8_t *ref = (JM_GLOBAL const uint8_t *)a.pics[k].ref;
	uint32_t *win = s_win[wave], *mb = s_cur[wave];
	const uint32_t R = p.search;
	/* the rows a search of radius R and its half-pel step read: 15 - R .. 32 + R */
	for (uint32_t i = (15u - R) * JM_ENCP_WIN_DW + lane; i < (33u + R) * JM_ENCP_WIN_DW; i += 64u) win[i] = jm_encp_window_dword(ref, a.cw, a.ch, col, row, i);
	mb[lane] = *reinterpret_cast<JM_GLOBAL const uint32_t *>(cur + (size_t)(lane >> 2) * a.cw + (size_t)(lane & 3u) * 4u);
	__syncthreads();

	const JmEncSearch shape = jm_encp_search_shape(R);
	uint64_t best = JM_ENCP_NO_KEY;
	for (uint32_t it = lane; it < shape.items; it += 64u) {
		const uint64_t key = jm_encp_search_item(win, mb, R, shape, it, a.cw, a.ch, col, row);
		best = key < best ? key : best;
	}
	best = enc_wave_min(best);
	uint32_t sad = jm_encp_key_sad(best);
	int mvh = 2 * jm_encp_key_dx(best), mvv = 2 * jm_encp_key_dy(best);
	if (R) {
		int hh, hv;
		jm_encp_half_step(lane >> 3, &hh, &hv);
		const int mh = mvh + hh, mv = mvv + hv;
		const bool ok = jm_encp_half_ok(a.cw, a.ch, col, row, mh, mv, p.r_size);
		uint32_t part = ok ? jm_encp_halfpel_part(win, mb, mh, mv, lane & 7u) : 0u;
		part += __shfl_xor(part, 1); part += __shfl_xor(part, 2); part += __shfl_xor(part, 4);
		const uint64_t hk = enc_wave_min(ok ? ((uint64_t)part << 3) | (lane >> 3) : JM_ENCP_NO_KEY);
		if (hk != JM_ENCP_NO_KEY && (uint32_t)(hk >> 3) < sad) {
			jm_encp_half_step((uint32_t)(hk & 7u), &hh, &hv);
			sad = (uint32_t)(hk >> 3); mvh += hh; mvv += hv;
		}
	}
	const uint32_t mean = (enc_wave_sum(jm_encp_sad4(mb[lane], 0u, 0u)) + 128u) >> 8;
	const uint32_t activity = enc_wave_sum(jm_encp_sad4(mb[lane], mean * 0x01010101u, 0u));
	if (live && lane == 0) p.pmb[(size_t)k * mbs + m].info = jm_encp_decide(sad, activity, mvh, mvv);
}

__global__ void __launch_bounds__(JM_ENC_LANES) k_enc_measure_p(JmEncArgs a, JmEncPArgs p, uint32_t first, uint32_t n) {
	__shared__ int16_t zz[64 * JM_ENC_LANES];
	__shared__ uint32_t pp[16 * JM_ENC_LANES];
	const uint64_t g = (uint64_t)blockIdx.x * JM_ENC_LANES + threadIdx.x;
	if (g >= (uint64_t)n * a.mbw * a.mbh) return;
	jm_pass_measure_p(a, p, first, g, zz + threadIdx.x, JM_ENC_LANES, pp + threadIdx.x, JM_ENC_LANES);
}

/* ------------------------------------------------------------------ kernels of rate control (enc_rate.h) */

__global__ void __launch_bounds__(JM_ENC_LANES) k_enc_rate_measure(JmEncArgs a, JmEncPArgs p, JmEncRArgs r, uint32_t first, uint32_t n) {
	__shared__ int16_t zz[64 * JM_ENC_LANES];
	__shared__ uint32_t pp[16 * JM_ENC_LANES];
	__shared__ uint32_t acc[JM_ENCR_MAX_Q * JM_ENC_LANES];
	const uint64_t g = (uint64_t)blockIdx.x * JM_ENC_LANES + threadIdx.x;
	if (g >= (uint64_t)n * a.mbw * a.mbh) return;
	const JmEncLane l = jm_pass_lane<true>(a, p.list, first, g);
	const JmEncPic pic = a.pics[l.k];
	const size_t at = (size_t)l.k * a.mbw * a.mbh + l.m;
	JmEncPMb *rec = p.pmb + at;
	JM_GLOBAL const uint8_t *ref = (JM_GLOBAL const uint8_t *)pic.ref;    /* only read in a P picture */
	const uint32_t found = (pic.ordinal % p.gop) ? rec->info : 0u;
	uint64_t dcs;
	if (jm_encr_measure((JM_GLOBAL const uint8_t *)pic.frame, ref, a.cw, a.ch, a.mbw, l.col, l.row, found, r.q_min, r.nq, a.tables, p.ptables,
	                    zz + threadIdx.x, JM_ENC_LANES, pp + threadIdx.x, JM_ENC_LANES, acc + threadIdx.x, JM_ENC_LANES, r.rec + at * JM_ENCR_MAX_Q, &dcs)) {
		rec->dc[0] = (uint32_t)dcs; rec->dc[1] = (uint32_t)(dcs >> 32);
	}
}

__global__ void __launch_bounds__(64) k_enc_rate_scan(JmEncArgs a, JmEncPArgs p, JmEncRArgs r, uint32_t first, uint32_t n) {
	const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (g >= (uint64_t)n * a.mbh * r.nq) return;
	const uint32_t qi = (uint32_t)(g % r.nq), row = (uint32_t)((g / r.nq) % a.mbh), k = p.list[first + (uint32_t)(g / ((uint64_t)r.nq * a.mbh))];
	const size_t s = (size_t)k * a.mbh + row;
	r.slice[s * JM_ENCR_MAX_Q + qi] = jm_encr_scan(r.rec + s * a.mbw * JM_ENCR_MAX_Q, p.pmb + s * a.mbw, qi, a.mbw, (a.pics[k].ordinal % p.gop) != 0, p.r_size, a.tables, p.ptables);
}

/* a wavefront per picture of the n pictures list[first ..]; lane qi: the picture at scale q_min + qi */
__global__ void __launch_bounds__(64) k_enc_rate_pick(JmEncArgs a, JmEncPArgs p, JmEncRArgs r, uint32_t first, uint32_t n) {
	if (blockIdx.x >= n) return;
	const uint32_t lane = threadIdx.x, k = p.list[first + blockIdx.x];
	const JmEncPic pic = a.pics[k];
	const uint32_t level = pic.ordinal % p.gop;
	uint32_t bytes = jm_encr_head_bytes(level);
	if (lane < r.nq)
		for (uint32_t row = 0; row < a.mbh; row++) bytes += r.slice[((size_t)k * a.mbh + row) * JM_ENCR_MAX_Q + lane];
	/* the GOP's pictures at the levels before: the `before` pictures in front of this one (all `level` of them unless the GOP
	 * began in an earlier call) -- their final bytes -- and what the earlier calls left */
	uint64_t spent = 0;
	for (uint32_t j = 1 + lane; j <= pic.before; j += 64u) spent += r.out[(size_t)(k - j) * 4 + 2];
#pragma unroll
	for (int o = 32; o; o >>= 1) spent += __shfl_xor((unsigned long long)spent, o);
	const uint32_t odd = jm_encc_spent_row(pic.carry);
	if (pic.carry & JM_ENCC_READ) spent += r.spent[(size_t)odd * a.max_streams + pic.stream];
	const uint64_t budget = jm_encr_budget(r.T, pic.m, level, r.W, spent);
	const uint32_t fit = (uint32_t)enc_wave_min(lane < r.nq && bytes <= budget ? lane : r.nq - 1u);
	const uint32_t taken = __shfl(bytes, (int)fit);
	if (lane == 0) {
		const_cast<JmEncPic *>(a.pics)[k].q = r.q_min + fit;
		r.out[(size_t)k * 4] = r.q_min + fit; r.out[(size_t)k * 4 + 1] = jm_encr_saturate(budget); r.out[(size_t)k * 4 + 2] = taken; r.out[(size_t)k * 4 + 3] = 0;
		if (pic.carry & JM_ENCC_WRITE) r.spent[(size_t)(odd ^ 1u) * a.max_streams + pic.stream] = spent + taken;
	}
}

__global__ void __launch_bounds__(64) k_enc_scan_slices_p(JmEncArgs a, JmEncPArgs p) {
	const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
	if (s >= a.count * a.mbh) return;
	jm_pass_scan_slice_p(a, p, s);
}

__global__ void __launch_bounds__(64) k_enc_scan_pictures_p(JmEncArgs a, JmEncPArgs p) {
	const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
	if (k >= a.count) return;
	jm_pass_scan_picture_p(a, p, k);
}

__global__ void __launch_bounds__(JM_ENC_LANES) k_enc_write_p(JmEncArgs a, JmEncPArgs p) {
	__shared__ int16_t zz[64 * JM_ENC_LANES];
	__shared__ uint32_t pp[16 * JM_ENC_LANES];
	if (a.result[1]) return;
	const uint64_t g = (uint64_t)blockIdx.x * JM_ENC_LANES + threadIdx.x;
	if (g >= (uint64_t)a.count * a.mbw * a.mbh) return;
	jm_pass_write_p(a, p, g, zz + threadIdx.x, JM_ENC_LANES, pp + threadIdx.x, JM_ENC_LANES);
}

/* ------------------------------------------------------------------ kernels of the TS mux (enc_ts.h) */

struct JmTsArgs {
	const uint8_t *src;          /* the bytes the units' offsets count from */
	const JmTsUnit *units;       /* [n] */
	JmTsPlaced *placed;          /* [n] */
	uint32_t n, n_streams, stream_id, pid;
	uint32_t *cc;                /* [n_streams]: the streams' continuity counters, from call to call */
	uint64_t *result;            /* total | status (1: above cap, 2: no ES) | packets | 0 | stream_begin[n_streams] | stream_end[n_streams] | cc_next, cc_after (u32 [n_streams] each) */
	uint64_t cap;
	uint32_t *out;
	const uint64_t *es_result;   /* the encoder's total | status, NULL without an encoder */
};
JM_HD uint64_t *ts_stream_begin(const JmTsArgs &t) { return t.result + 4; }
JM_HD uint64_t *ts_stream_end(const JmTsArgs &t) { return t.result + 4 + t.n_streams; }
JM_HD uint32_t *ts_cc_next(const JmTsArgs &t) { return (uint32_t *)(t.result + 4 + 2 * (size_t)t.n_streams); }
JM_HD uint32_t *ts_cc_after(const JmTsArgs &t) { return ts_cc_next(t) + t.n_streams; }
JM_HD size_t ts_result_bytes(uint32_t n_streams) { return 8 * (4 + 3 * (size_t)n_streams); }

__global__ void __launch_bounds__(256) k_ts_units(JmEncArgs a, JmTsUnit *units, const uint64_t *pts) {
	const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
	if (k >= a.count) return;
	JmTsUnit u;
	u.off = enc_pic_off(a)[k];
	u.bytes = enc_pic_bytes(a)[k] + ((a.end && a.pics[k].last) ? 4u : 0u);
	u.stream = a.pics[k].stream;
	u.pts = pts[k];
	units[k] = u;
}

/* one workgroup: 256 units at a time through LDS, lane 0 walks them */
__global__ void __launch_bounds__(256) k_ts_plan(JmTsArgs t) {
	__shared__ uint32_t s_bytes[256], s_stream[256];
	__shared__ JmTsPlaced s_out[256];
	__shared__ JmTsPlan plan;
	__shared__ uint32_t s_status;
	uint64_t *sb = ts_stream_begin(t), *se = ts_stream_end(t);
	uint32_t *cn = ts_cc_next(t), *ca = ts_cc_after(t);
	const bool no_es = t.es_result && t.es_result[1];              /* after an ES overflow there is no TS */
	for (uint32_t i = threadIdx.x; i < t.n_streams; i += 256) { sb[i] = 0; se[i] = 0; cn[i] = 0; }
	if (threadIdx.x == 0) plan = jm_ts_plan_begin();
	__syncthreads();
	for (uint32_t base = 0; base < t.n && !no_es; base += 256) {
		const uint32_t k = base + threadIdx.x, n = min(256u, t.n - base);
		if (k < t.n) { s_bytes[threadIdx.x] = t.units[k].bytes; s_stream[threadIdx.x] = t.units[k].stream; }
		__syncthreads();
		if (threadIdx.x == 0) {
			JmTsPlan p = plan;
			for (uint32_t i = 0; i < n; i++) s_out[i] = jm_ts_plan_unit(p, s_stream[i], s_bytes[i], t.cc, sb, se, cn);
			plan = p;
		}
		__syncthreads();
		if (k < t.n) t.placed[k] = s_out[threadIdx.x];
		__syncthreads();
	}
	if (threadIdx.x == 0) {
		JmTsPlan p = plan;
		jm_ts_plan_close(p, t.cap, se, cn, t.result);
		if (no_es) t.result[1] = 2u;
		t.result[3] = 0;
		s_status = (uint32_t)t.result[1];
	}
	__syncthreads();
	for (uint32_t i = threadIdx.x; i < t.n_streams; i += 256) {
		if (s_status == 0) jm_ts_plan_commit(i, sb, se, cn, t.cc);
		ca[i] = t.cc[i];
	}
}

__global__ void __launch_bounds__(256) k_ts_write(JmTsArgs t) {
	if (t.result[1]) return;
	const uint64_t dwords = t.result[2] * JM_TS_DWORDS;
	for (uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; g < dwords; g += (uint64_t)gridDim.x * blockDim.x) {
		uint64_t where;
		const uint32_t v = jm_ts_output_dword<JmTsFetchAligned>(t.units, t.placed, t.n, g, t.stream_id, t.pid, t.src, &where);
		t.out[where] = v;
	}
}
#define JM_TS_WRITE_GRID 1024u

/* ------------------------------------------------------------------ the handle */

struct jsmpeg_hip_encoder_t {
	jsmpeg_hip_encoder_config_t cfg;
	int device;
	uint32_t cw, ch, mbw, mbh;
	uint64_t frame_bytes;
	JmEncTables *d_tables;
	JmEncPic *d_pics, *h_pics;       /* h_pics: pinned */
	JmEncMb *d_mb;
	uint32_t *d_slice;
	uint64_t *d_result, *h_result;   /* h_result: pinned */
	uint8_t *d_es;
	uint8_t *d_store;                /* frames of the tensor and the scaled input, allocated by the first jsmpeg_hip_encoder_encode_rgb / _encode_scaled */
	/* scaled input (jsmpeg_hip_encoder_encode_scaled; enc_scale.h), allocated by its first call */
	uint32_t *d_scale_tab, *h_scale_tab;          /* the tap table; h_: pinned */
	const uint8_t **d_scale_src, **h_scale_src;   /* [max_pictures] source frames; h_: pinned */
	jsmpeg_hip_enc_source_t scale_key;            /* the geometry scale_plan and d_scale_tab were made for */
	JmEsPlan scale_plan;
	bool scale_have;
	/* mosaic input (jsmpeg_hip_encoder_set_mosaic / _encode_mosaic; enc_mosaic.h), everything allocated by set_mosaic */
	uint32_t *d_mosaic_tab;                       /* the layout's table */
	uint32_t mosaic_tab_words;                    /* ... and what it holds at most */
	const uint8_t **d_mosaic_src, **h_mosaic_src; /* [max_pictures][cells] frames; h_: pinned */
	uint32_t mosaic_src_cells;                    /* the cells per picture they hold at most */
	JmEmPlan mosaic_plan;                         /* mosaic_plan.n 0: no layout */
	hipStream_t stream;
	hipEvent_t ev[4], ev_done;
	bool pending, valid, have_pass;
	uint32_t count;
	/* a GOP (jsmpeg_hip_encoder_set_gop); the stores are allocated by the first call that asks for gop > 1 */
	uint32_t gop, search;
	uint8_t *d_recon;                /* a reconstructed frame per picture of a call */
	JmEncPMb *d_pmb;
	JmEncPTables *d_ptables;
	uint32_t *d_list, *h_list;       /* the pictures by level; h_list: pinned */
	uint32_t *d_slice_kinds, *d_stats, *h_stats;   /* h_stats: pinned */
	bool gop_ready;                  /* all of the stores above are there */
	bool pass_gop;                   /* the last call ran the level loop: gop > 1, or rate control */
	/* rate control (jsmpeg_hip_encoder_set_rate); the stores are allocated by the first call that switches it on */
	uint32_t rate_bytes, q_min, q_max, i_weight;   /* rate_bytes 0: off */
	uint16_t *d_rate_rec;
	uint32_t *d_rate_slice, *d_rate_out, *h_rate;  /* h_rate: pinned */
	bool rate_ready;
	bool pass_rate;                  /* the last call ran with rate control */
	/* chains across calls (JSMPEG_HIP_ENC_CHAIN; the rule: enc_chain.h) */
	std::vector<JmEncChain> chain;   /* [max_streams], host only */
	std::vector<JmEncPlan> plan;     /* scratch of a call */
	uint8_t *d_carry;                /* two frames per stream number, allocated by the first chained call that runs the level loop */
	uint64_t *d_spent;               /* [2][max_streams], with d_carry */
	bool pass_chain;                 /* the last call was chained: an overflow resets its streams */
	/* TS on the device (jsmpeg_hip_encoder_set_ts; the rule: enc_ts.h); everything allocated by set_ts */
	uint64_t max_ts_bytes;           /* 0: off */
	uint32_t ts_stream_id, ts_pid;
	uint8_t *d_ts;
	JmTsUnit *d_ts_units;
	JmTsPlaced *d_ts_placed;         /* behind d_ts_result, in one allocation: one copy brings both back */
	uint32_t *d_ts_cc;               /* [max_streams]: a property of the PID, not of the chain */
	uint64_t *d_ts_result, *h_ts_result;   /* h_: pinned */
	uint64_t *d_ts_pts, *h_ts_pts;   /* [max_pictures]; h_: pinned */
	std::vector<uint64_t> ts_pts;    /* jsmpeg_hip_encoder_ts_pts: for the next call */
	bool ts_pts_set;
	bool pass_ts;                    /* the last call ran with TS on */
	bool ts_overflowed;              /* ... and its TS did not fit */
	JmEncArgs last_args;             /* of the last call that launched (count != 0): for the program mux (ts_prog_sources.h) */
};

static void enc_free_gop(jsmpeg_hip_encoder_t *e);
static void enc_free_rate(jsmpeg_hip_encoder_t *e);
static void enc_free_ts(jsmpeg_hip_encoder_t *e);
static void enc_free(jsmpeg_hip_encoder_t *e) {
	if (!e) return;
	hipSetDevice(e->device);
	if (e->pending) hipEventSynchronize(e->ev_done);
	hipFree(e->d_tables); hipFree(e->d_pics); hipFree(e->d_mb); hipFree(e->d_slice); hipFree(e->d_result); hipFree(e->d_es); hipFree(e->d_store);
	enc_free_gop(e);
	enc_free_rate(e);
	enc_free_ts(e);
	hipFree(e->d_carry); hipFree(e->d_spent);
	if (e->h_pics) hipHostFree(e->h_pics);
	if (e->h_result) hipHostFree(e->h_result);
	hipFree(e->d_scale_tab); hipFree(e->d_scale_src);
	if (e->h_scale_tab) hipHostFree(e->h_scale_tab);
	if (e->h_scale_src) hipHostFree(e->h_scale_src);
	hipFree(e->d_mosaic_tab); hipFree(e->d_mosaic_src);
	if (e->h_mosaic_src) hipHostFree(e->h_mosaic_src);
	for (hipEvent_t &v : e->ev) if (v) hipEventDestroy(v);
	if (e->ev_done) hipEventDestroy(e->ev_done);
	delete e;
}

static int enc_alloc(jsmpeg_hip_encoder_t *e) {
	static const JmEncTables tables = jm_enc_make_tables();
	const size_t mbs = (size_t)e->mbw * e->mbh, np = e->cfg.max_pictures;
	const size_t rb = enc_result_bytes(e->cfg.max_streams, e->cfg.max_pictures);
	HIP_TRY(jm_malloc(&e->d_tables, sizeof(JmEncTables)));
	HIP_TRY(hipMemcpy(e->d_tables, &tables, sizeof(JmEncTables), hipMemcpyHostToDevice));
	HIP_TRY(jm_malloc(&e->d_pics, sizeof(JmEncPic) * np));
	HIP_TRY(hipHostMalloc(reinterpret_cast<void **>(&e->h_pics), sizeof(JmEncPic) * np, hipHostMallocDefault));
	HIP_TRY(jm_malloc(&e->d_mb, sizeof(JmEncMb) * mbs * np));
	HIP_TRY(jm_malloc(&e->d_slice, sizeof(uint32_t) * e->mbh * np));
	HIP_TRY(jm_malloc(&e->d_result, rb));
	HIP_TRY(hipHostMalloc(reinterpret_cast<void **>(&e->h_result), rb, hipHostMallocDefault));
	memset(e->h_result, 0, rb);
	HIP_TRY(jm_malloc(&e->d_es, jm_enc_align16(e->cfg.max_es_bytes) + JM_ENC_TAIL + 16));
	for (hipEvent_t &v : e->ev) HIP_TRY(hipEventCreate(&v));
	HIP_TRY(hipEventCreateWithFlags(&e->ev_done, hipEventDisableTiming));
	return 0;
}

extern "C" jsmpeg_hip_encoder_t *jsmpeg_hip_encoder_create(const jsmpeg_hip_encoder_config_t *config) {
	g_err[0] = 0;
	if (!config) { fail("jsmpeg_hip_encoder_create: NULL config"); return nullptr; }
	if (jsmpeg_hip_device_count() <= 0) {
		fail("no HIP device available: the MPEG-1 encode path has no CPU fallback");
		return nullptr;
	}
	if (config->width < 1 || config->width > 4095 || config->height < 1 || config->height > 4095) {
		fail("encoder: size %d x %d, each side must be 1 .. 4095", config->width, config->height); return nullptr;
	}
	if ((config->height + 15) / 16 > 175) { fail("encoder: height %d has more than 175 macroblock rows (slice start codes 01 .. AF)", config->height); return nullptr; }
	if (config->max_pictures < 1 || config->max_streams < 1 || config->max_es_bytes < 64) {
		fail("encoder: max_pictures, max_streams must be >= 1 and max_es_bytes >= 64"); return nullptr;
	}
	if (config->max_es_bytes > 0xffffffffull * 4) { fail("encoder: max_es_bytes above 16 GiB"); return nullptr; }
	if (config->frame_rate_code > 8) { fail("encoder: frame_rate_code %u, must be 1 .. 8 (0: 30 / s)", config->frame_rate_code); return nullptr; }
	jsmpeg_hip_encoder_t *e = new jsmpeg_hip_encoder_t();
	e->cfg = *config;
	if (e->cfg.frame_rate_code == 0) e->cfg.frame_rate_code = 5;
	if (config->device >= 0 && hipSetDevice(config->device) != hipSuccess) { fail("hipSetDevice(%d) failed", config->device); delete e; return nullptr; }
	if (hipGetDevice(&e->device) != hipSuccess) { fail("hipGetDevice failed"); delete e; return nullptr; }
	e->mbw = (uint32_t)(config->width + 15) >> 4; e->mbh = (uint32_t)(config->height + 15) >> 4;
	e->cw = e->mbw * 16; e->ch = e->mbh * 16;
	e->frame_bytes = (uint64_t)e->cw * e->ch * 3 / 2;
	e->gop = 1; e->search = 0;
	e->q_min = 1; e->q_max = JM_ENCR_MAX_Q; e->i_weight = 1;
	e->chain.assign(config->max_streams, JmEncChain{ 0, 0, 0, 0 });
	e->plan.resize(config->max_pictures);
	if (enc_alloc(e) != 0) { enc_free(e); return nullptr; }
	return e;
}

extern "C" void jsmpeg_hip_encoder_destroy(jsmpeg_hip_encoder_t *e) { enc_free(e); }

/* waits for the pass in flight, reads its verdict */
static int enc_settle(jsmpeg_hip_encoder_t *e) {
	if (!e->pending) return 0;
	HIP_TRY(hipSetDevice(e->device));
	e->pending = false;
	HIP_TRY(hipEventSynchronize(e->ev_done));
	if (e->h_result[1]) {
		e->valid = false;
		if (e->pass_chain)                                       /* what the call's streams were continued with is not there */
			for (uint32_t k = 0; k < e->count; k++) jm_encc_reset(e->chain[e->h_pics[k].stream]);
		return fail("encoder: the call's streams need %llu bytes, max_es_bytes is %llu: nothing of the call is valid",
		            (unsigned long long)e->h_result[0], (unsigned long long)e->cfg.max_es_bytes);
	}
	if (e->pass_ts && e->count && e->h_ts_result[1] == 1) {        /* a TS overflow is an overflow of the call; the counters stayed */
		e->valid = false;
		e->ts_overflowed = true;
		if (e->pass_chain)
			for (uint32_t k = 0; k < e->count; k++) jm_encc_reset(e->chain[e->h_pics[k].stream]);
		return fail("encoder: the call's TS needs %llu bytes, max_ts_bytes is %llu: nothing of the call is valid",
		            (unsigned long long)e->h_ts_result[0], (unsigned long long)e->max_ts_bytes);
	}
	e->valid = true;
	return 0;
}

static void enc_free_gop(jsmpeg_hip_encoder_t *e) {
	hipFree(e->d_recon); hipFree(e->d_pmb); hipFree(e->d_ptables); hipFree(e->d_list); hipFree(e->d_slice_kinds); hipFree(e->d_stats);
	if (e->h_list) hipHostFree(e->h_list);
	if (e->h_stats) hipHostFree(e->h_stats);
	e->d_recon = nullptr; e->d_pmb = nullptr; e->d_ptables = nullptr; e->d_list = nullptr; e->d_slice_kinds = nullptr; e->d_stats = nullptr;
	e->h_list = nullptr; e->h_stats = nullptr;
	e->gop_ready = false;
}

/* the stores only a GOP needs; the caller frees what a failure leaves behind (enc_free_gop) */
static int enc_alloc_gop(jsmpeg_hip_encoder_t *e) {
	static const JmEncPTables ptables = jm_encp_make_tables();
	const size_t mbs = (size_t)e->mbw * e->mbh, np = e->cfg.max_pictures;
	HIP_TRY(hipSetDevice(e->device));
	HIP_TRY(jm_malloc(&e->d_ptables, sizeof(JmEncPTables)));
	HIP_TRY(hipMemcpy(e->d_ptables, &ptables, sizeof(JmEncPTables), hipMemcpyHostToDevice));
	HIP_TRY(jm_malloc(&e->d_recon, (size_t)e->frame_bytes * np + 16));      /* + 16: jm_encp_predict8 reads whole dwords */
	HIP_TRY(jm_malloc(&e->d_pmb, sizeof(JmEncPMb) * mbs * np));
	HIP_TRY(jm_malloc(&e->d_list, sizeof(uint32_t) * np));
	HIP_TRY(hipHostMalloc(reinterpret_cast<void **>(&e->h_list), sizeof(uint32_t) * np, hipHostMallocDefault));
	HIP_TRY(jm_malloc(&e->d_slice_kinds, sizeof(uint32_t) * 4 * e->mbh * np));
	HIP_TRY(jm_malloc(&e->d_stats, sizeof(uint32_t) * 4 * np));
	HIP_TRY(hipHostMalloc(reinterpret_cast<void **>(&e->h_stats), sizeof(uint32_t) * 4 * np, hipHostMallocDefault));
	e->gop_ready = true;
	return 0;
}

extern "C" int jsmpeg_hip_encoder_set_gop(jsmpeg_hip_encoder_t *e, uint32_t gop, uint32_t search_range) {
	g_err[0] = 0;
	if (!e) return fail("encoder: NULL handle");
	if (e->pending) return fail("encoder: an encode is in flight: jsmpeg_hip_encoder_sync (or a reader) settles it first");
	if (gop < 1 || gop > 1024) return fail("encoder: gop %u, must be 1 .. 1024", gop);
	if (search_range > JM_ENC_MAX_SEARCH) return fail("encoder: search_range %u, must be 0 .. %u", search_range, JM_ENC_MAX_SEARCH);
	if (gop > 1 && !e->gop_ready && enc_alloc_gop(e) != 0) { enc_free_gop(e); return -1; }     /* gop and search_range stay as they were */
	e->gop = gop; e->search = search_range;
	for (JmEncChain &c : e->chain) jm_encc_reset(c);           /* levels and forward_f_code change */
	return 0;
}

/* the carry frames and the GOPs' spent bytes; a failure leaves neither */
static int enc_alloc_carry(jsmpeg_hip_encoder_t *e) {
	const size_t ns = e->cfg.max_streams;
	HIP_TRY(hipSetDevice(e->device));
	if (jm_malloc(&e->d_carry, 2 * ns * (size_t)e->frame_bytes + 16) != hipSuccess || jm_malloc(&e->d_spent, sizeof(uint64_t) * 2 * ns) != hipSuccess ||
	    hipMemset(e->d_spent, 0, sizeof(uint64_t) * 2 * ns) != hipSuccess || hipStreamSynchronize(nullptr) != hipSuccess) {   /* the caller's stream may not wait for the null stream */
		hipFree(e->d_carry); hipFree(e->d_spent);
		e->d_carry = nullptr; e->d_spent = nullptr;
		return fail("encoder: no memory for the carry frames of %u streams", e->cfg.max_streams);
	}
	return 0;
}

extern "C" int jsmpeg_hip_encoder_chain_reset(jsmpeg_hip_encoder_t *e, uint32_t stream) {
	g_err[0] = 0;
	if (!e) return fail("encoder: NULL handle");
	if (e->pending) return fail("encoder: an encode is in flight: jsmpeg_hip_encoder_sync (or a reader) settles it first");
	if (stream != UINT32_MAX && stream >= e->cfg.max_streams) return fail("encoder: stream %u >= max_streams %u", stream, e->cfg.max_streams);
	for (uint32_t s = 0; s < e->cfg.max_streams; s++)
		if (stream == UINT32_MAX || s == stream) jm_encc_reset(e->chain[s]);
	return 0;
}

static void enc_free_rate(jsmpeg_hip_encoder_t *e) {
	hipFree(e->d_rate_rec); hipFree(e->d_rate_slice); hipFree(e->d_rate_out);
	if (e->h_rate) hipHostFree(e->h_rate);
	e->d_rate_rec = nullptr; e->d_rate_slice = nullptr; e->d_rate_out = nullptr; e->h_rate = nullptr;
	e->rate_ready = false;
}

/* the stores only rate control needs; the caller frees what a failure leaves behind (enc_free_rate) */
static int enc_alloc_rate(jsmpeg_hip_encoder_t *e) {
	const size_t mbs = (size_t)e->mbw * e->mbh, np = e->cfg.max_pictures;
	HIP_TRY(hipSetDevice(e->device));
	HIP_TRY(jm_malloc(&e->d_rate_rec, sizeof(uint16_t) * JM_ENCR_MAX_Q * mbs * np));
	HIP_TRY(jm_malloc(&e->d_rate_slice, sizeof(uint32_t) * JM_ENCR_MAX_Q * e->mbh * np));
	HIP_TRY(jm_malloc(&e->d_rate_out, sizeof(uint32_t) * 4 * np));
	HIP_TRY(hipHostMalloc(reinterpret_cast<void **>(&e->h_rate), sizeof(uint32_t) * 4 * np, hipHostMallocDefault));
	e->rate_ready = true;
	return 0;
}

extern "C" int jsmpeg_hip_encoder_set_rate(jsmpeg_hip_encoder_t *e, uint32_t bytes_per_picture, uint32_t q_min, uint32_t q_max, uint32_t i_weight) {
	g_err[0] = 0;
	if (!e) return fail("encoder: NULL handle");
	if (e->pending) return fail("encoder: an encode is in flight: jsmpeg_hip_encoder_sync (or a reader) settles it first");
	if (q_min < 1 || q_max > JM_ENCR_MAX_Q || q_min > q_max) return fail("encoder: q_min %u, q_max %u: 1 <= q_min <= q_max <= 31 is needed", q_min, q_max);
	if (i_weight < 1 || i_weight > 255) return fail("encoder: i_weight %u, must be 1 .. 255", i_weight);
	if (bytes_per_picture) {                                                               /* on a failure the handle's rate stays as it was */
		if (!e->gop_ready && enc_alloc_gop(e) != 0) { enc_free_gop(e); return -1; }
		if (!e->rate_ready && enc_alloc_rate(e) != 0) { enc_free_rate(e); return -1; }
	}
	e->rate_bytes = bytes_per_picture; e->q_min = q_min; e->q_max = q_max; e->i_weight = i_weight;
	return 0;
}

static void enc_free_ts(jsmpeg_hip_encoder_t *e) {
	hipFree(e->d_ts); hipFree(e->d_ts_units); hipFree(e->d_ts_cc); hipFree(e->d_ts_result); hipFree(e->d_ts_pts);
	if (e->h_ts_result) hipHostFree(e->h_ts_result);
	if (e->h_ts_pts) hipHostFree(e->h_ts_pts);
	e->d_ts = nullptr; e->d_ts_units = nullptr; e->d_ts_placed = nullptr; e->d_ts_cc = nullptr; e->d_ts_result = nullptr; e->d_ts_pts = nullptr;
	e->h_ts_result = nullptr; e->h_ts_pts = nullptr;
	e->max_ts_bytes = 0;
}

static size_t enc_ts_result_bytes(const jsmpeg_hip_encoder_t *e) { return ts_result_bytes(e->cfg.max_streams) + sizeof(JmTsPlaced) * e->cfg.max_pictures; }

/* the TS buffer, the unit table, the counters (all 0); the caller frees what a failure leaves behind (enc_free_ts) */
static int enc_alloc_ts(jsmpeg_hip_encoder_t *e, uint64_t max_ts_bytes) {
	const size_t np = e->cfg.max_pictures, ns = e->cfg.max_streams, rb = enc_ts_result_bytes(e);
	HIP_TRY(hipSetDevice(e->device));
	HIP_TRY(jm_malloc(&e->d_ts, jm_ts_align16(max_ts_bytes) + 16));
	HIP_TRY(jm_malloc(&e->d_ts_units, sizeof(JmTsUnit) * np));
	HIP_TRY(jm_malloc(&e->d_ts_cc, sizeof(uint32_t) * ns));
	HIP_TRY(jm_malloc(&e->d_ts_result, rb));
	HIP_TRY(jm_malloc(&e->d_ts_pts, sizeof(uint64_t) * np));
	HIP_TRY(hipHostMalloc(reinterpret_cast<void **>(&e->h_ts_result), rb, hipHostMallocDefault));
	HIP_TRY(hipHostMalloc(reinterpret_cast<void **>(&e->h_ts_pts), sizeof(uint64_t) * np, hipHostMallocDefault));
	memset(e->h_ts_result, 0, rb);
	e->d_ts_placed = reinterpret_cast<JmTsPlaced *>(reinterpret_cast<uint8_t *>(e->d_ts_result) + ts_result_bytes(e->cfg.max_streams));
	HIP_TRY(hipMemset(e->d_ts_cc, 0, sizeof(uint32_t) * ns));
	HIP_TRY(hipStreamSynchronize(nullptr));                    /* the caller's stream may not wait for the null stream */
	e->max_ts_bytes = max_ts_bytes;
	return 0;
}

extern "C" int jsmpeg_hip_encoder_set_ts(jsmpeg_hip_encoder_t *e, uint32_t stream_id, uint32_t pid, uint64_t max_ts_bytes) {
	g_err[0] = 0;
	if (!e) return fail("encoder: NULL handle");
	if (e->pending) return fail("encoder: an encode is in flight: jsmpeg_hip_encoder_sync (or a reader) settles it first");
	if (pid > 0x1fff || stream_id > 0xff) return fail("encoder: pid %u / stream id %u out of range (0x1fff, 0xff)", pid, stream_id);
	if (max_ts_bytes > 0xffffffffull * 4) return fail("encoder: max_ts_bytes above 16 GiB");
	enc_free_ts(e);                                            /* off; the last call's TS is gone either way */
	e->pass_ts = false; e->ts_overflowed = false; e->ts_pts_set = false;
	if (max_ts_bytes && enc_alloc_ts(e, max_ts_bytes) != 0) { enc_free_ts(e); return -1; }
	e->ts_stream_id = stream_id; e->ts_pid = pid;
	return 0;
}

extern "C" int jsmpeg_hip_encoder_ts_pts(jsmpeg_hip_encoder_t *e, const uint64_t *pts_90k, uint32_t count) {
	g_err[0] = 0;
	if (!e) return fail("encoder: NULL handle");
	if (e->pending) return fail("encoder: an encode is in flight: jsmpeg_hip_encoder_sync (or a reader) settles it first");
	if (!e->max_ts_bytes) return fail("encoder: TS is off (jsmpeg_hip_encoder_set_ts)");
	if (count && !pts_90k) return fail("encoder: NULL pts_90k");
	e->ts_pts.assign(pts_90k, pts_90k + count);
	e->ts_pts_set = true;
	return 0;
}

/* the mux behind the write, in the same enqueue; `a` is the pass's */
static int enc_run_ts(jsmpeg_hip_encoder_t *e, const JmEncArgs &a, uint32_t count, bool have_pts, hipStream_t st) {
	for (uint32_t k = 0; k < count; k++) e->h_ts_pts[k] = have_pts ? e->ts_pts[k] : jm_ts_default_pts(e->plan[k].ordinal, e->cfg.frame_rate_code);
	HIP_TRY(hipMemcpyAsync(e->d_ts_pts, e->h_ts_pts, sizeof(uint64_t) * count, hipMemcpyHostToDevice, st));
	JmTsArgs t;
	t.src = e->d_es; t.units = e->d_ts_units; t.placed = e->d_ts_placed; t.n = count; t.n_streams = e->cfg.max_streams;
	t.stream_id = e->ts_stream_id; t.pid = e->ts_pid; t.cc = e->d_ts_cc; t.result = e->d_ts_result; t.cap = e->max_ts_bytes;
	t.out = reinterpret_cast<uint32_t *>(e->d_ts); t.es_result = e->d_result;
	k_ts_units<<<dim3((count + 255) / 256), dim3(256), 0, st>>>(a, e->d_ts_units, e->d_ts_pts);
	k_ts_plan<<<dim3(1), dim3(256), 0, st>>>(t);
	k_ts_write<<<dim3(JM_TS_WRITE_GRID), dim3(256), 0, st>>>(t);
	HIP_TRY(hipGetLastError());
	return 0;
}

/* the stores of the scaled input, and the plan and table of `source` (kept while the geometry stays) */
static int enc_alloc_scale(jsmpeg_hip_encoder_t *e) {
	const size_t words = jm_es_table_bound((uint32_t)e->cfg.width, (uint32_t)e->cfg.height), np = e->cfg.max_pictures;
	if (!e->d_scale_tab) HIP_TRY(jm_malloc(&e->d_scale_tab, 4 * words));
	if (!e->h_scale_tab) HIP_TRY(hipHostMalloc(reinterpret_cast<void **>(&e->h_scale_tab), 4 * words, hipHostMallocDefault));
	if (!e->d_scale_src) HIP_TRY(jm_malloc(&e->d_scale_src, sizeof(uint8_t *) * np));
	if (!e->h_scale_src) HIP_TRY(hipHostMalloc(reinterpret_cast<void **>(&e->h_scale_src), sizeof(uint8_t *) * np, hipHostMallocDefault));
	return 0;
}

/* the level loop (gop > 1, or rate control) between ev[1] and ev[3]; `a` is complete */
static int enc_run_gop(jsmpeg_hip_encoder_t *e, const JmEncArgs &a, uint32_t count, hipStream_t st) {
	JmEncPArgs p;
	p.pmb = e->d_pmb; p.ptables = e->d_ptables; p.list = e->d_list;
	p.slice_kinds = e->d_slice_kinds; p.stats = e->d_stats;
	p.gop = e->gop; p.search = e->search; p.r_size = jm_encp_r_size(e->search);
	std::vector<uint32_t> begin(e->gop + 1);
	const uint32_t levels = jm_encc_levels(e->plan.data(), count, e->gop, e->h_list, begin.data());
	HIP_TRY(hipMemcpyAsync(e->d_list, e->h_list, sizeof(uint32_t) * count, hipMemcpyHostToDevice, st));
	const uint64_t mbs = (uint64_t)e->mbw * e->mbh;
	JmEncRArgs r;
	r.rec = e->d_rate_rec; r.slice = e->d_rate_slice; r.out = e->d_rate_out; r.spent = e->d_spent;
	r.T = e->rate_bytes; r.q_min = e->q_min; r.nq = e->q_max - e->q_min + 1u; r.W = e->i_weight;
	for (uint32_t l = 0; l < levels; l++) {
		const uint32_t first = begin[l], n = begin[l + 1] - begin[l];
		if (!n) continue;
		if (l) k_enc_motion<<<dim3((uint32_t)((n * mbs + JM_ENC_MOTION_WAVES - 1) / JM_ENC_MOTION_WAVES)), dim3(64 * JM_ENC_MOTION_WAVES), 0, st>>>(a, p, first, n);
		if (e->pass_rate) {
			k_enc_rate_measure<<<dim3((uint32_t)((n * mbs + JM_ENC_LANES - 1) / JM_ENC_LANES)), dim3(JM_ENC_LANES), 0, st>>>(a, p, r, first, n);
			k_enc_rate_scan<<<dim3((uint32_t)(((uint64_t)n * e->mbh * r.nq + 63) / 64)), dim3(64), 0, st>>>(a, p, r, first, n);
			k_enc_rate_pick<<<dim3(n), dim3(64), 0, st>>>(a, p, r, first, n);
		}
		k_enc_measure_p<<<dim3((uint32_t)((n * mbs + JM_ENC_LANES - 1) / JM_ENC_LANES)), dim3(JM_ENC_LANES), 0, st>>>(a, p, first, n);
	}
	k_enc_scan_slices_p<<<dim3((count * e->mbh + 63) / 64), dim3(64), 0, st>>>(a, p);
	k_enc_scan_pictures_p<<<dim3((count + 63) / 64), dim3(64), 0, st>>>(a, p);
	k_enc_place<<<dim3(1), dim3(256), 0, st>>>(a);
	HIP_TRY(hipEventRecord(e->ev[2], st));
	k_enc_clear<<<dim3(1024), dim3(256), 0, st>>>(a);
	k_enc_write_p<<<dim3((uint32_t)((count * mbs + JM_ENC_LANES - 1) / JM_ENC_LANES)), dim3(JM_ENC_LANES), 0, st>>>(a, p);
	HIP_TRY(hipGetLastError());
	HIP_TRY(hipMemcpyAsync(e->h_stats, e->d_stats, sizeof(uint32_t) * 4 * count, hipMemcpyDeviceToHost, st));
	if (e->pass_rate) HIP_TRY(hipMemcpyAsync(e->h_rate, e->d_rate_out, sizeof(uint32_t) * 4 * count, hipMemcpyDeviceToHost, st));
	return 0;
}

static int enc_run(jsmpeg_hip_encoder_t *e, const void *const *frames, const void *dev_rgb, uint32_t layout, uint32_t order,
                   const jsmpeg_hip_enc_source_t *source, const void *const *cell_frames, const uint32_t *stream, const uint8_t *qscale, uint32_t count, uint32_t quantiser_scale, uint32_t flags, void *hip_stream) {
	g_err[0] = 0;
	if (!e) return fail("encoder: NULL handle");
	if (e->pending) return fail("encoder: an encode is in flight: jsmpeg_hip_encoder_sync (or a reader) settles it first");
	const bool have_pts = e->ts_pts_set;                       /* jsmpeg_hip_encoder_ts_pts binds this call only, refused or not */
	e->ts_pts_set = false;
	if (have_pts && e->ts_pts.size() != count) return fail("encoder: %u pts values for a call of %u pictures", (unsigned)e->ts_pts.size(), count);
	if (count > e->cfg.max_pictures) return fail("encoder: %u pictures > max_pictures %u", count, e->cfg.max_pictures);
	if (flags & ~(JSMPEG_HIP_ENC_END | JSMPEG_HIP_ENC_CHAIN)) return fail("encoder: unknown flags 0x%x", flags);
	if (count && !frames && !dev_rgb && !cell_frames) return fail("encoder: NULL frames");
	if (dev_rgb && (layout > JSMPEG_HIP_TENSOR_NHWC || order > JSMPEG_HIP_TENSOR_BGR)) return fail("encoder: layout %u / order %u unknown", layout, order);
	if (!qscale && (quantiser_scale < 1 || quantiser_scale > 31)) return fail("encoder: quantiser_scale %u, must be 1 .. 31", quantiser_scale);
	if (source) {
		const char *why = jm_es_check(source);
		if (why) return fail("encoder: %s", why);
	}
	for (uint32_t k = 0; k < count; k++) {
		if (frames && !frames[k]) return fail("encoder: frames[%u] is NULL", k);
		if (frames && ((uintptr_t)frames[k] & 15u)) return fail("encoder: frames[%u] is not 16-byte aligned", k);
		if (qscale && (qscale[k] < 1 || qscale[k] > 31)) return fail("encoder: qscale[%u] = %u, must be 1 .. 31", k, qscale[k]);
		if (stream && stream[k] >= e->cfg.max_streams) return fail("encoder: stream[%u] = %u >= max_streams %u", k, stream[k], e->cfg.max_streams);
		if (stream && k && stream[k] < stream[k - 1]) return fail("encoder: stream[] must ascend (stream[%u] = %u after %u)", k, stream[k], stream[k - 1]);
	}
	if (cell_frames) {
		if (!e->mosaic_plan.n) return fail("encoder: no mosaic layout is set (jsmpeg_hip_encoder_set_mosaic)");
		for (uint64_t i = 0; i < (uint64_t)count * e->mosaic_plan.n; i++)
			if ((uintptr_t)cell_frames[i] & 15u)
				return fail("encoder: the frame of cell %u of picture %u is not 16-byte aligned", (unsigned)(i % e->mosaic_plan.n), (unsigned)(i / e->mosaic_plan.n));
	}
	HIP_TRY(hipSetDevice(e->device));
	hipStream_t st = (hipStream_t)hip_stream;
	const bool chained = (flags & JSMPEG_HIP_ENC_CHAIN) != 0, end = (flags & JSMPEG_HIP_ENC_END) != 0;
	const bool rate = e->rate_bytes != 0, level_loop = e->gop > 1 || rate;
	if (chained && count && level_loop) {
		if (!e->gop_ready && enc_alloc_gop(e) != 0) { enc_free_gop(e); return -1; }
		if (!e->d_carry && enc_alloc_carry(e) != 0) return -1;
	}
	if (source && count) {
		if (enc_alloc_scale(e) != 0) return -1;
		if (!e->d_store) HIP_TRY(jm_malloc(&e->d_store, (size_t)e->frame_bytes * e->cfg.max_pictures));
		if (!e->scale_have || memcmp(&e->scale_key, source, sizeof(*source)) != 0) {
			e->scale_have = false;
			e->scale_plan = jm_es_plan(source, (uint32_t)e->cfg.width, (uint32_t)e->cfg.height);
			if (e->scale_plan.words > jm_es_table_bound((uint32_t)e->cfg.width, (uint32_t)e->cfg.height)) return fail("encoder: the tap table is larger than its bound");
		}
	}
	e->count = count;
	e->have_pass = true;
	e->pass_chain = chained;
	e->pass_ts = e->max_ts_bytes != 0;
	e->ts_overflowed = false;
	if (count == 0) {
		e->valid = true; e->h_result[0] = 0; e->h_result[1] = 0;
		if (e->pass_ts) e->h_ts_result[0] = e->h_ts_result[1] = e->h_ts_result[2] = 0;
		return 0;
	}
	if (dev_rgb && !e->d_store) HIP_TRY(jm_malloc(&e->d_store, (size_t)e->frame_bytes * e->cfg.max_pictures));
	jm_encc_plan_call(stream, count, e->chain.data(), rate, e->gop, chained, end, e->plan.data());
	for (uint32_t k = 0; k < count; k++) {
		const JmEncPlan &pl = e->plan[k];
		JmEncPic &p = e->h_pics[k];
		p.frame = frames && !source ? (const uint8_t *)frames[k] : e->d_store + (size_t)k * e->frame_bytes;
		p.stream = stream ? stream[k] : 0; p.ordinal = pl.ordinal; p.q = qscale ? qscale[k] : quantiser_scale;
		p.last = pl.last; p.m = pl.m; p.before = pl.before; p.carry = pl.carry;
		p.ref = level_loop ? jm_encc_frame(pl.ref, e->d_recon, e->d_carry, e->frame_bytes) : nullptr;
		p.recon = level_loop ? jm_encc_frame(pl.recon, e->d_recon, e->d_carry, e->frame_bytes) : nullptr;
	}
	JmEncArgs a;
	a.width = (uint32_t)e->cfg.width; a.height = (uint32_t)e->cfg.height; a.cw = e->cw; a.ch = e->ch; a.mbw = e->mbw; a.mbh = e->mbh;
	a.count = count; a.frame_rate_code = e->cfg.frame_rate_code; a.end = end ? 1u : 0u;
	a.cap = e->cfg.max_es_bytes;
	a.pics = e->d_pics; a.tables = e->d_tables; a.mb = e->d_mb; a.slice = e->d_slice; a.result = e->d_result;
	a.max_streams = e->cfg.max_streams; a.max_pictures = e->cfg.max_pictures;
	a.words = reinterpret_cast<uint32_t *>(e->d_es);
	e->last_args = a;
	const uint64_t lanes = (uint64_t)count * e->mbw * e->mbh;
	const uint32_t mb_grid = (uint32_t)((lanes + JM_ENC_LANES - 1) / JM_ENC_LANES);
	e->stream = st;
	e->valid = false;
	HIP_TRY(hipMemcpyAsync(e->d_pics, e->h_pics, sizeof(JmEncPic) * count, hipMemcpyHostToDevice, st));
	HIP_TRY(hipEventRecord(e->ev[0], st));
	if (dev_rgb) {
		const uint64_t quads = (uint64_t)count * (e->cw >> 1) * (e->ch >> 1);
		k_enc_rgb<<<dim3((uint32_t)((quads + 255) / 256)), dim3(256), 0, st>>>(a, (const uint8_t *)dev_rgb, layout, order);
	}
	if (source) {
		JmEncScaleArgs s;
		if (!e->scale_have) {                                   /* (no pass is in flight: the pinned table is free) */
			jm_es_table(e->scale_plan, e->h_scale_tab);
			HIP_TRY(hipMemcpyAsync(e->d_scale_tab, e->h_scale_tab, 4 * (size_t)e->scale_plan.words, hipMemcpyHostToDevice, st));
			e->scale_key = *source;
			e->scale_have = true;
		}
		for (uint32_t k = 0; k < count; k++) e->h_scale_src[k] = (const uint8_t *)frames[k];
		HIP_TRY(hipMemcpyAsync(e->d_scale_src, e->h_scale_src, sizeof(uint8_t *) * count, hipMemcpyHostToDevice, st));
		s.plan = e->scale_plan; s.src = e->d_scale_src; s.tab = e->d_scale_tab;
		k_enc_scale<<<dim3(s.plan.tiles, std::min(count, 65535u)), dim3(256), 0, st>>>(a, s);
	}
	if (cell_frames) {
		const size_t np = (size_t)count * e->mosaic_plan.n;        /* (no pass is in flight: the pinned pointers are free) */
		for (size_t i = 0; i < np; i++) e->h_mosaic_src[i] = (const uint8_t *)cell_frames[i];
		HIP_TRY(hipMemcpyAsync(e->d_mosaic_src, e->h_mosaic_src, sizeof(uint8_t *) * np, hipMemcpyHostToDevice, st));
		k_enc_mosaic<<<dim3(e->mosaic_plan.tiles, std::min(count, 65535u)), dim3(256), 0, st>>>(a, e->mosaic_plan, e->d_mosaic_src, e->d_mosaic_tab);
	}
	HIP_TRY(hipEventRecord(e->ev[1], st));
	e->pass_rate = rate;
	e->pass_gop = level_loop;
	if (e->pass_gop) {
		if (enc_run_gop(e, a, count, st) != 0) return -1;
	} else {
		k_enc_measure<<<dim3(mb_grid), dim3(JM_ENC_LANES), 0, st>>>(a);
		k_enc_scan_slices<<<dim3((count * e->mbh + 63) / 64), dim3(64), 0, st>>>(a);
		k_enc_scan_pictures<<<dim3((count + 63) / 64), dim3(64), 0, st>>>(a);
		k_enc_place<<<dim3(1), dim3(256), 0, st>>>(a);
		HIP_TRY(hipEventRecord(e->ev[2], st));
		k_enc_clear<<<dim3(1024), dim3(256), 0, st>>>(a);
		k_enc_write<<<dim3(mb_grid), dim3(JM_ENC_LANES), 0, st>>>(a);
		HIP_TRY(hipGetLastError());
	}
	if (e->pass_ts && enc_run_ts(e, a, count, have_pts, st) != 0) return -1;
	HIP_TRY(hipEventRecord(e->ev[3], st));
	HIP_TRY(hipMemcpyAsync(e->h_result, e->d_result, enc_result_bytes(e->cfg.max_streams, e->cfg.max_pictures), hipMemcpyDeviceToHost, st));
	if (e->pass_ts) HIP_TRY(hipMemcpyAsync(e->h_ts_result, e->d_ts_result, ts_result_bytes(e->cfg.max_streams) + sizeof(JmTsPlaced) * count, hipMemcpyDeviceToHost, st));
	HIP_TRY(hipEventRecord(e->ev_done, st));
	e->pending = true;
	return 0;
}

extern "C" int jsmpeg_hip_encoder_encode(jsmpeg_hip_encoder_t *e, const void *const *frames, const uint32_t *stream, const uint8_t *qscale,
                                         uint32_t count, uint32_t quantiser_scale, uint32_t flags, void *hip_stream) {
	if (count && !frames) { g_err[0] = 0; return fail("encoder: NULL frames"); }
	return enc_run(e, frames, nullptr, 0, 0, nullptr, nullptr, stream, qscale, count, quantiser_scale, flags, hip_stream);
}

extern "C" int jsmpeg_hip_encoder_encode_scaled(jsmpeg_hip_encoder_t *e, const void *const *frames, const jsmpeg_hip_enc_source_t *source,
                                                const uint32_t *stream, const uint8_t *qscale, uint32_t count, uint32_t quantiser_scale,
                                                uint32_t flags, void *hip_stream) {
	if (!source) { g_err[0] = 0; return fail("encoder: null source descriptor"); }
	if (count && !frames) { g_err[0] = 0; return fail("encoder: NULL frames"); }
	return enc_run(e, frames, nullptr, 0, 0, source, nullptr, stream, qscale, count, quantiser_scale, flags, hip_stream);
}

extern "C" int jsmpeg_hip_encoder_encode_rgb(jsmpeg_hip_encoder_t *e, const void *dev_rgb, uint32_t layout, uint32_t order, const uint32_t *stream,
                                             const uint8_t *qscale, uint32_t count, uint32_t quantiser_scale, uint32_t flags, void *hip_stream) {
	if (count && !dev_rgb) { g_err[0] = 0; return fail("encoder: NULL tensor"); }
	return enc_run(e, nullptr, dev_rgb, layout, order, nullptr, nullptr, stream, qscale, count, quantiser_scale, flags, hip_stream);
}

/* The layout of the mosaic input: checked, planned and uploaded here; a refusal leaves the layout before as it was */
extern "C" int jsmpeg_hip_encoder_set_mosaic(jsmpeg_hip_encoder_t *e, const jsmpeg_hip_enc_cell_t *cells, uint32_t n_cells, uint32_t fill) {
	g_err[0] = 0;
	if (!e) return fail("encoder: NULL handle");
	if (e->pending) return fail("encoder: an encode is in flight: jsmpeg_hip_encoder_sync (or a reader) settles it first");
	if (n_cells == 0) { e->mosaic_plan.n = 0; return 0; }
	const uint32_t W = (uint32_t)e->cfg.width, H = (uint32_t)e->cfg.height;
	uint32_t cell;
	if (const char *why = jm_em_check(cells, n_cells, fill, W, H, &cell))
		return cell == 0xffffffffu ? fail("encoder: mosaic: %s", why) : fail("encoder: mosaic cell %u: %s", cell, why);
	const JmEmPlan plan = jm_em_plan(cells, n_cells, fill, W, H);
	if (plan.words > jm_em_table_bound(n_cells, W, H)) return fail("encoder: the mosaic table is larger than its bound");
	if (!jm_em_tiles_ok(plan)) return fail("encoder: a mosaic tile without a display sample");
	HIP_TRY(hipSetDevice(e->device));
	/* what is missing is allocated beside what is there, and swapped in once nothing can fail any more */
	uint32_t *d_tab = nullptr;
	const uint8_t **d_src = nullptr, **h_src = nullptr;
	const size_t np = (size_t)e->cfg.max_pictures * n_cells;
	hipError_t r = hipSuccess;
	if (plan.words > e->mosaic_tab_words) r = jm_malloc(&d_tab, 4 * (size_t)plan.words);
	if (r == hipSuccess && n_cells > e->mosaic_src_cells) {
		r = jm_malloc(&d_src, sizeof(uint8_t *) * np);
		if (r == hipSuccess) r = hipHostMalloc(reinterpret_cast<void **>(&h_src), sizeof(uint8_t *) * np, hipHostMallocDefault);
	}
	if (r == hipSuccess && !e->d_store) r = jm_malloc(&e->d_store, (size_t)e->frame_bytes * e->cfg.max_pictures);
	if (r == hipSuccess) {
		std::vector<uint32_t> tab(plan.words);
		jm_em_table(plan, cells, tab.data());
		/* (the one exception to "a refusal leaves the layout before as it was": a table that fits the allocation in use is
		 * copied over it, so if this copy itself fails -- the device is lost then -- the old layout's table is not whole either) */
		r = hipMemcpy(d_tab ? d_tab : e->d_mosaic_tab, tab.data(), 4 * (size_t)plan.words, hipMemcpyHostToDevice);
	}
	if (r != hipSuccess) {
		hipFree(d_tab); hipFree(d_src);
		if (h_src) hipHostFree(h_src);
		return fail("encoder: set_mosaic: %s", hipGetErrorString(r));
	}
	if (d_tab) { hipFree(e->d_mosaic_tab); e->d_mosaic_tab = d_tab; e->mosaic_tab_words = plan.words; }
	if (d_src) {
		hipFree(e->d_mosaic_src);
		if (e->h_mosaic_src) hipHostFree(e->h_mosaic_src);
		e->d_mosaic_src = d_src; e->h_mosaic_src = h_src; e->mosaic_src_cells = n_cells;
	}
	e->mosaic_plan = plan;
	return 0;
}

extern "C" int jsmpeg_hip_encoder_encode_mosaic(jsmpeg_hip_encoder_t *e, const void *const *frames, const uint32_t *stream, const uint8_t *qscale,
                                                uint32_t count, uint32_t quantiser_scale, uint32_t flags, void *hip_stream) {
	static const void *const none[1] = { nullptr };
	if (count && !frames) { g_err[0] = 0; return fail("encoder: NULL frames"); }
	return enc_run(e, nullptr, nullptr, 0, 0, nullptr, frames ? frames : none, stream, qscale, count, quantiser_scale, flags, hip_stream);
}

extern "C" int jsmpeg_hip_encoder_sync(jsmpeg_hip_encoder_t *e) {
	g_err[0] = 0;
	if (!e) return fail("encoder: NULL handle");
	return enc_settle(e);
}

extern "C" int jsmpeg_hip_encoder_query(jsmpeg_hip_encoder_t *e) {
	g_err[0] = 0;
	if (!e) return fail("encoder: NULL handle");
	if (!e->pending) return 1;
	HIP_TRY(hipSetDevice(e->device));
	const hipError_t r = hipEventQuery(e->ev_done);
	if (r == hipSuccess) return 1;
	if (r == hipErrorNotReady) return 0;
	return fail("hipEventQuery: %s", hipGetErrorString(r));
}

/* the readers: settle, then refuse a handle without a valid pass */
static int enc_ready(jsmpeg_hip_encoder_t *e) {
	g_err[0] = 0;
	if (!e) return fail("encoder: NULL handle");
	if (enc_settle(e) < 0) return -1;
	if (!e->have_pass) return fail("encoder: nothing was encoded yet");
	if (!e->valid && e->ts_overflowed) return fail("encoder: the last call overflowed max_ts_bytes (%llu): nothing of it is valid", (unsigned long long)e->max_ts_bytes);
	if (!e->valid) return fail("encoder: the last call overflowed max_es_bytes (%llu): nothing of it is valid", (unsigned long long)e->cfg.max_es_bytes);
	return 0;
}

extern "C" void *jsmpeg_hip_encoder_es(jsmpeg_hip_encoder_t *e, uint64_t *total_bytes) {
	if (enc_ready(e) < 0) return nullptr;
	if (total_bytes) *total_bytes = e->h_result[0];
	return e->d_es;
}

extern "C" int jsmpeg_hip_encoder_stream_range(jsmpeg_hip_encoder_t *e, uint32_t stream, uint64_t *begin, uint64_t *end) {
	if (enc_ready(e) < 0) return -1;
	if (stream >= e->cfg.max_streams) return fail("encoder: stream %u >= max_streams %u", stream, e->cfg.max_streams);
	const bool any = e->count != 0;
	if (begin) *begin = any ? e->h_result[2 + stream] : 0;
	if (end) *end = any ? e->h_result[2 + e->cfg.max_streams + stream] : 0;
	return 0;
}

extern "C" int jsmpeg_hip_encoder_picture_range(jsmpeg_hip_encoder_t *e, uint32_t k, uint64_t *offset, uint32_t *bytes) {
	if (enc_ready(e) < 0) return -1;
	if (k >= e->count) return fail("encoder: picture %u of %u", k, e->count);
	const uint64_t *off = e->h_result + 2 + 2 * (size_t)e->cfg.max_streams;
	if (offset) *offset = off[k];
	if (bytes) *bytes = reinterpret_cast<const uint32_t *>(off + e->cfg.max_pictures)[k];
	return 0;
}

extern "C" const void *jsmpeg_hip_encoder_recon(jsmpeg_hip_encoder_t *e, uint32_t k) {
	if (enc_ready(e) < 0) return nullptr;
	if (!e->pass_gop) { fail("encoder: the last call ran with gop 1: it keeps no reconstruction (jsmpeg_hip_encoder_set_gop)"); return nullptr; }
	if (k >= e->count) { fail("encoder: picture %u of %u", k, e->count); return nullptr; }
	return e->h_pics[k].recon;                                 /* the call's store, or a chained stream's carry frame */
}

extern "C" const void *jsmpeg_hip_encoder_source(jsmpeg_hip_encoder_t *e, uint32_t k) {
	if (enc_ready(e) < 0) return nullptr;
	if (k >= e->count) { fail("encoder: picture %u of %u", k, e->count); return nullptr; }
	return e->h_pics[k].frame;                                 /* the caller's frame, or the handle's store (converted / scaled) */
}

extern "C" int jsmpeg_hip_encoder_chain_info(jsmpeg_hip_encoder_t *e, uint32_t stream, uint32_t out[2]) {
	g_err[0] = 0;
	if (!e) return fail("encoder: NULL handle");
	if (!out) return fail("encoder: NULL out");
	if (stream >= e->cfg.max_streams) return fail("encoder: stream %u >= max_streams %u", stream, e->cfg.max_streams);
	if (e->pending) { enc_settle(e); g_err[0] = 0; }           /* an overflow resets the call's streams; sync and the readers report it */
	out[0] = e->chain[stream].have; out[1] = e->chain[stream].n;
	return 0;
}

extern "C" int jsmpeg_hip_encoder_picture_stats(jsmpeg_hip_encoder_t *e, uint32_t k, uint32_t out[4]) {
	if (enc_ready(e) < 0) return -1;
	if (k >= e->count) return fail("encoder: picture %u of %u", k, e->count);
	if (!out) return fail("encoder: NULL out");
	const uint32_t mbs = e->mbw * e->mbh;
	for (int i = 0; i < 4; i++) out[i] = e->pass_gop ? e->h_stats[(size_t)k * 4 + i] : (i == 0 ? mbs : 0u);
	return 0;
}

extern "C" int jsmpeg_hip_encoder_picture_rate(jsmpeg_hip_encoder_t *e, uint32_t k, uint32_t out[3]) {
	if (enc_ready(e) < 0) return -1;
	if (!e->pass_rate) return fail("encoder: the last call ran with rate control off (jsmpeg_hip_encoder_set_rate)");
	if (k >= e->count) return fail("encoder: picture %u of %u", k, e->count);
	if (!out) return fail("encoder: NULL out");
	for (int i = 0; i < 3; i++) out[i] = e->h_rate[(size_t)k * 4 + i];
	return 0;
}

extern "C" int64_t jsmpeg_hip_encoder_read_es(jsmpeg_hip_encoder_t *e, uint32_t stream, void *host, uint64_t cap) {
	uint64_t b = 0, n = 0;
	if (jsmpeg_hip_encoder_stream_range(e, stream, &b, &n) < 0) return -1;
	n -= b;
	const uint64_t k = std::min(n, cap);
	if (k && host) {
		HIP_TRY(hipSetDevice(e->device));
		HIP_TRY(hipMemcpy(host, e->d_es + b, k, hipMemcpyDeviceToHost));
	}
	return (int64_t)n;
}

extern "C" int jsmpeg_hip_encoder_timings(jsmpeg_hip_encoder_t *e, float out_ms[4]) {
	if (enc_ready(e) < 0) return -1;
	if (!out_ms) return fail("encoder: NULL out_ms");
	for (int i = 0; i < 4; i++) out_ms[i] = 0.0f;
	if (!e->count) return 0;
	HIP_TRY(hipSetDevice(e->device));
	for (int i = 0; i < 3; i++) HIP_TRY(hipEventElapsedTime(&out_ms[i], e->ev[i], e->ev[i + 1]));
	HIP_TRY(hipEventElapsedTime(&out_ms[3], e->ev[0], e->ev[3]));
	return 0;
}

/* ------------------------------------------------------------------ the TS readers */

static int enc_ts_ready(jsmpeg_hip_encoder_t *e) {
	if (enc_ready(e) < 0) return -1;
	if (!e->pass_ts) return fail(e->max_ts_bytes ? "encoder: TS was switched on after the last call: nothing of it is muxed" : "encoder: TS is off (jsmpeg_hip_encoder_set_ts)");
	return 0;
}

extern "C" void *jsmpeg_hip_encoder_ts(jsmpeg_hip_encoder_t *e, uint64_t *total_bytes) {
	if (enc_ts_ready(e) < 0) return nullptr;
	if (total_bytes) *total_bytes = e->h_ts_result[0];
	return e->d_ts;
}

extern "C" int jsmpeg_hip_encoder_ts_range(jsmpeg_hip_encoder_t *e, uint32_t stream, uint64_t *begin, uint64_t *end, uint32_t *continuity_next) {
	if (enc_ts_ready(e) < 0) return -1;
	if (stream >= e->cfg.max_streams) return fail("encoder: stream %u >= max_streams %u", stream, e->cfg.max_streams);
	const uint32_t ns = e->cfg.max_streams;
	const bool any = e->count != 0;
	if (begin) *begin = any ? e->h_ts_result[4 + stream] : 0;
	if (end) *end = any ? e->h_ts_result[4 + ns + stream] : 0;
	if (continuity_next) *continuity_next = reinterpret_cast<const uint32_t *>(e->h_ts_result + 4 + 2 * (size_t)ns)[ns + stream];   /* cc_after: kept over a call of no pictures */
	return 0;
}

extern "C" int jsmpeg_hip_encoder_ts_picture_range(jsmpeg_hip_encoder_t *e, uint32_t k, uint64_t *offset, uint32_t *bytes) {
	if (enc_ts_ready(e) < 0) return -1;
	if (k >= e->count) return fail("encoder: picture %u of %u", k, e->count);
	const JmTsPlaced &u = reinterpret_cast<const JmTsPlaced *>(reinterpret_cast<const uint8_t *>(e->h_ts_result) + ts_result_bytes(e->cfg.max_streams))[k];
	if (offset) *offset = u.at;
	if (bytes) *bytes = u.packets * JM_TS_PACKET;
	return 0;
}

extern "C" int64_t jsmpeg_hip_encoder_read_ts(jsmpeg_hip_encoder_t *e, uint32_t stream, void *host, uint64_t cap) {
	uint64_t b = 0, n = 0;
	if (stream == UINT32_MAX) {
		if (enc_ts_ready(e) < 0) return -1;
		n = e->h_ts_result[0];
	} else {
		if (jsmpeg_hip_encoder_ts_range(e, stream, &b, &n, nullptr) < 0) return -1;
		n -= b;
	}
	const uint64_t k = std::min(n, cap);
	if (k && host) {
		HIP_TRY(hipSetDevice(e->device));
		HIP_TRY(hipMemcpy(host, e->d_ts + b, k, hipMemcpyDeviceToHost));
	}
	return (int64_t)n;
}

/* ------------------------------------------------------------------ the last call as the program mux's video source
 * (ts_prog_sources.h): the device-side picture table becomes a unit table on the caller's stream; the host is not waited for */
int jm_enc_tsp_source(jsmpeg_hip_encoder_t *e, JmTspVideoSource *out, uint32_t *stream, uint32_t *ordinal, uint32_t cap) {
	if (!e) return fail("ts_program: NULL encoder");
	if (!e->have_pass) return fail("ts_program: the encoder has not encoded anything yet");
	if (e->count > cap) return fail("ts_program: the encoder's last call has %u pictures, max_video_units is %u", e->count, cap);
	out->count = e->count; out->max_streams = e->cfg.max_streams; out->frame_rate_code = e->cfg.frame_rate_code; out->device = e->device;
	out->d_es = e->d_es; out->d_result = e->d_result;
	for (uint32_t k = 0; k < e->count; k++) { stream[k] = e->h_pics[k].stream; ordinal[k] = e->h_pics[k].ordinal; }
	return 0;
}

int jm_enc_tsp_units(jsmpeg_hip_encoder_t *e, JmTsUnit *d_units, const uint64_t *d_pts, void *hip_stream) {
	if (!e || !e->have_pass) return fail("ts_program: the encoder has not encoded anything yet");
	if (!e->count) return 0;
	k_ts_units<<<dim3((e->count + 255) / 256), dim3(256), 0, (hipStream_t)hip_stream>>>(e->last_args, d_units, d_pts);
	HIP_TRY(hipGetLastError());
	return 0;
}

extern "C" uint64_t jsmpeg_hip_ts_bound(uint64_t es_bytes, uint32_t units, uint32_t streams) { return jm_ts_bound(es_bytes, units, streams); }

/* ------------------------------------------------------------------ TS mux on the host (no device) and over any device bytes
 * The rule, the PES and the stuffing: enc_ts.h.  The host walks units, packets and dwords in order; nothing depends on it. */
extern "C" int64_t jsmpeg_hip_ts_mux_host(const uint8_t *es, const uint64_t *offset, const uint32_t *bytes, const uint64_t *pts_90k,
                                          uint32_t n_units, uint32_t stream_id, uint32_t pid, uint8_t *continuity, uint8_t *ts, uint64_t ts_cap) {
	g_err[0] = 0;
	if (n_units && (!offset || !bytes || !pts_90k || (ts && !es))) return fail("ts_mux: NULL argument");
	if (pid > 0x1fff || stream_id > 0xff) return fail("ts_mux: pid %u / stream id %u out of range", pid, stream_id);
	uint32_t cc = continuity ? (uint32_t)(*continuity & 15u) : 0u;
	uint64_t at = 0;
	for (uint32_t i = 0; i < n_units; i++) {
		const uint32_t packets = jm_ts_packets(bytes[i]);
		if (!ts) { at += (uint64_t)packets * JM_TS_PACKET; continue; }
		if (at + (uint64_t)packets * JM_TS_PACKET > ts_cap) return fail("ts_mux: %llu bytes do not fit ts_cap %llu", (unsigned long long)(at + (uint64_t)packets * JM_TS_PACKET), (unsigned long long)ts_cap);
		JmTsUnit u;
		u.off = offset[i]; u.bytes = bytes[i]; u.stream = 0; u.pts = pts_90k[i];
		JmTsFetchBytes f;
		f.base = es + u.off;
		for (uint32_t k = 0; k < packets; k++, at += JM_TS_PACKET)
			for (uint32_t w = 0; w < JM_TS_DWORDS; w++) {
				const uint32_t v = jm_ts_dword(u, cc, stream_id, pid, k, w, f);
				memcpy(ts + at + 4u * w, &v, 4);
			}
		cc = (cc + packets) & 15u;
	}
	if (ts && continuity) *continuity = (uint8_t)cc;
	return (int64_t)at;
}

/* The two kernels over any device bytes and a host-given unit list; synchronous, on the null stream, with scratch of its own
 * for the call: for stored ES on the device.  The units of a stream are contiguous, the streams ascend and stay below
 * n_streams; continuity: one in / out counter per stream number. */
extern "C" int64_t jsmpeg_hip_ts_mux_device(const void *dev_es, const uint64_t *offset, const uint32_t *bytes, const uint32_t *stream,
                                            const uint64_t *pts_90k, uint32_t n_units, uint32_t stream_id, uint32_t pid,
                                            uint8_t *continuity, uint32_t n_streams,
                                            void *dev_ts, uint64_t ts_cap, uint64_t *stream_begin, uint64_t *stream_end) {
	g_err[0] = 0;
	if (jsmpeg_hip_device_count() <= 0) return fail("no HIP device available: jsmpeg_hip_ts_mux_device has no CPU fallback (jsmpeg_hip_ts_mux_host)");
	if (n_units && (!dev_es || !offset || !bytes || !pts_90k || !dev_ts)) return fail("ts_mux: NULL argument");
	if (n_streams < 1) return fail("ts_mux: n_streams 0");
	if (pid > 0x1fff || stream_id > 0xff) return fail("ts_mux: pid %u / stream id %u out of range", pid, stream_id);
	if ((uintptr_t)dev_ts & 3u) return fail("ts_mux: dev_ts is not 4-byte aligned");
	if (ts_cap > 0xffffffffull * 4) return fail("ts_mux: ts_cap above 16 GiB");
	std::vector<JmTsUnit> units(n_units);
	for (uint32_t i = 0; i < n_units; i++) {
		JmTsUnit &u = units[i];
		u.off = offset[i]; u.bytes = bytes[i]; u.stream = stream ? stream[i] : 0u; u.pts = pts_90k[i];
		if (u.stream >= n_streams) return fail("ts_mux: stream[%u] = %u >= n_streams %u", i, u.stream, n_streams);
		if (i && u.stream < units[i - 1].stream) return fail("ts_mux: stream[] must ascend (stream[%u] = %u after %u)", i, u.stream, units[i - 1].stream);
	}
	std::vector<uint32_t> cc(n_streams, 0u);
	for (uint32_t s = 0; continuity && s < n_streams; s++) cc[s] = continuity[s] & 15u;
	const size_t rb = ts_result_bytes(n_streams);
	std::vector<uint64_t> result(rb / 8, 0);
	uint8_t *scratch = nullptr;                                /* units | placed | result | cc */
	const size_t o_placed = sizeof(JmTsUnit) * n_units, o_result = o_placed + sizeof(JmTsPlaced) * n_units, o_cc = o_result + rb;
	HIP_TRY(jm_malloc(&scratch, o_cc + sizeof(uint32_t) * n_streams));
	JmTsArgs t;
	t.src = (const uint8_t *)dev_es; t.units = reinterpret_cast<JmTsUnit *>(scratch); t.placed = reinterpret_cast<JmTsPlaced *>(scratch + o_placed);
	t.n = n_units; t.n_streams = n_streams; t.stream_id = stream_id; t.pid = pid;
	t.cc = reinterpret_cast<uint32_t *>(scratch + o_cc); t.result = reinterpret_cast<uint64_t *>(scratch + o_result);
	t.cap = ts_cap; t.out = reinterpret_cast<uint32_t *>(dev_ts); t.es_result = nullptr;
	hipError_t r = n_units ? hipMemcpy(scratch, units.data(), o_placed, hipMemcpyHostToDevice) : hipSuccess;
	if (r == hipSuccess) r = hipMemcpy(t.cc, cc.data(), sizeof(uint32_t) * n_streams, hipMemcpyHostToDevice);
	if (r == hipSuccess) {
		k_ts_plan<<<dim3(1), dim3(256), 0, nullptr>>>(t);
		k_ts_write<<<dim3(JM_TS_WRITE_GRID), dim3(256), 0, nullptr>>>(t);
		r = hipGetLastError();
	}
	if (r == hipSuccess) r = hipMemcpy(result.data(), t.result, rb, hipMemcpyDeviceToHost);      /* waits for both kernels */
	hipFree(scratch);
	if (r != hipSuccess) return fail("ts_mux: %s", hipGetErrorString(r));
	if (result[1]) return fail("ts_mux: %llu bytes do not fit ts_cap %llu", (unsigned long long)result[0], (unsigned long long)ts_cap);
	const uint32_t *after = reinterpret_cast<const uint32_t *>(result.data() + 4 + 2 * (size_t)n_streams) + n_streams;
	for (uint32_t s = 0; s < n_streams; s++) {
		if (continuity) continuity[s] = (uint8_t)after[s];
		if (stream_begin) stream_begin[s] = result[4 + s];
		if (stream_end) stream_end[s] = result[4 + n_streams + s];
	}
	return (int64_t)result[0];
}
