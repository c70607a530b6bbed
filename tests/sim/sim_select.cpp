/* TEST-ONLY: select_plan.h (the rules of kernels.hip k_select) compiled for the CPU -- the sequential definition and the scan
 * form chunk by chunk, over picture tables the test makes up; the chain (fwd, level) is index_tables.h jm_index_chain's. */
#include <cstdint>
#include <cstring>
#include <vector>

#include "index_tables.h"
#include "recon_plan.h"
#include "select_plan.h"

extern "C" {

/* pictures [lo[s], hi[s]) belong to stream s; decoded_in / type_in / nslices_in: the whole decode's table.  width == 0: the
 * sequential definition, else the scan form with chunks of `width` lanes.  out_*: [n_pics]; sc_owner: [sum of nslices_in],
 * picture p's slice codes from the prefix sum, preset to p; totals: needed | slices | levels. */
int sim_select(uint32_t n_pics, uint32_t n_streams, const uint32_t *lo, const uint32_t *hi, const uint8_t *decoded_in, const uint8_t *type_in,
               const uint32_t *nslices_in, const uint32_t *bits, const uint32_t *off, const uint32_t *nbits, uint32_t width,
               uint8_t *out_decoded, uint32_t *out_pad, int32_t *out_fwd, int32_t *out_level, uint32_t *out_nslices,
               uint32_t *frame_pic, int32_t *before_last, uint32_t *sc_owner, uint32_t *totals) {
	std::vector<JmPic> pics(n_pics);
	uint32_t sc = 0;
	for (uint32_t s = 0; s < n_streams; s++)
		for (uint32_t p = lo[s]; p < hi[s]; p++) {
			JmPic &pic = pics[p];
			memset(&pic, 0, sizeof pic);
			pic.stream = s; pic.decoded = decoded_in[p]; pic.type = type_in[p]; pic.fwd = -1; pic.level = 0;
			pic.n_slices = pic.decoded ? nslices_in[p] : 0;
			pic.first_slice_sc = pic.n_slices ? sc : JM_NONE;
			for (uint32_t k = 0; k < pic.n_slices; k++) sc_owner[sc++] = p;
		}
	for (uint32_t s = 0; s < n_streams; s++) {
		JmStream st;
		memset(&st, 0, sizeof st);
		st.pic_lo = lo[s]; st.pic_hi = hi[s];
		jm_index_chain(st, pics.data());
	}
	for (uint32_t p = 0; p < n_pics; p++) { out_fwd[p] = pics[p].fwd; out_level[p] = pics[p].level; }
	JmSelectLayout l = { bits, off, nbits };
	JmSelectTotals tot = { 0, 0, 0 };
	std::vector<int32_t> scratch(3 * (size_t)(width ? width : 1));
	for (uint32_t s = 0; s < n_streams; s++) {
		if (width) jm_select_stream_chunked(pics.data(), lo[s], hi[s], s, l, frame_pic, before_last, sc_owner, tot, width, scratch.data());
		else jm_select_stream(pics.data(), lo[s], hi[s], s, l, frame_pic, before_last, sc_owner, tot);
	}
	for (uint32_t p = 0; p < n_pics; p++) { out_decoded[p] = pics[p].decoded; out_pad[p] = pics[p].pad_; out_nslices[p] = pics[p].n_slices; }
	totals[0] = tot.needed; totals[1] = tot.slices; totals[2] = tot.levels;
	return 0;
}

/* the thinned table's `stale` (recon_plan.h jm_plan_stale: what the pass's plan takes) and the widening rule */
int sim_select_widen(uint32_t n_pics, uint32_t n_streams, const uint32_t *stream, const uint8_t *decoded, const uint32_t *pad, const int32_t *fwd,
                     const int32_t *before_last, const uint32_t *covered, uint32_t mb_size, int32_t *stale_out, uint32_t *widen) {
	std::vector<JmPic> pics(n_pics);
	for (uint32_t p = 0; p < n_pics; p++) {
		memset(&pics[p], 0, sizeof(JmPic));
		pics[p].stream = stream[p]; pics[p].decoded = decoded[p]; pics[p].pad_ = pad[p]; pics[p].fwd = fwd[p];
	}
	std::vector<int32_t> stale;
	jm_plan_stale(pics.data(), n_pics, n_streams, stale);
	for (uint32_t p = 0; p < n_pics; p++) stale_out[p] = stale[p];
	return (int)jm_select_widen(pics.data(), n_pics, n_streams, stale.data(), before_last, covered, mb_size, widen);
}

}
