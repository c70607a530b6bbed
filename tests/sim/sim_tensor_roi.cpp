/* TEST-ONLY simulator of k_tensor_roi (kernels.hip): tensor_plan.h's jm_roi_clip and jm_tensor_roi_plan, then the per-pixel
 * loop of sim_tensor.cpp over a list of regions of interest, so that tests/test_tensor_roi_plan.py holds the rows against
 * torch's F.interpolate of the clipped box without a GPU. */
#include <math.h>
#include <stdint.h>

#include "tensor_plan.h"

/* the clip rule: the status, and the clipped rectangle (x, y, width, height) in out[4] */
extern "C" int sim_roi_clip(const jsmpeg_hip_roi_t *r, uint32_t count, uint32_t w, uint32_t h, int32_t *out) {
	const JmRoiClip c = jm_roi_clip(*r, count, w, h);
	out[0] = c.x; out[1] = c.y; out[2] = c.width; out[3] = c.height;
	return (int)c.status;
}

/* "" or the message of the descriptor check of a call with boxes */
extern "C" const char *sim_tensor_roi_check(const jsmpeg_hip_tensor_desc_t *d, uint32_t w, uint32_t h) {
	const char *m = jm_tensor_roi_check(d, w, h);
	return m ? m : "";
}

/* `count` pictures (frames + k * frame_bytes: Y | Cr | Cb of coded_width x coded_height, display w x h; present[k] 0: no picture
 * there) and n_rois boxes -> out[n_rois][3][height][width] floats in the tensor's channel order (a float dtype's value, U8's
 * rounded one; zeros for status 0) and status[n_rois].  0, or -1 for a descriptor the check refuses. */
extern "C" int sim_tensor_rois(const uint8_t *frames, const uint8_t *present, uint32_t count, uint32_t cw, uint32_t ch, uint32_t w,
                               uint32_t h, const jsmpeg_hip_tensor_desc_t *d, const jsmpeg_hip_roi_t *rois, uint32_t n_rois,
                               float *out, uint8_t *status) {
	if (jm_tensor_roi_check(d, w, h)) return -1;
	const JmTensorPlan p0 = jm_tensor_plan(d, w, h);
	const size_t frame_bytes = (size_t)cw * ch * 3 / 2, row = (size_t)3 * p0.out_h * p0.out_w;
	for (uint32_t r = 0; r < n_rois; r++) {
		float *o = out + r * row;
		for (size_t i = 0; i < row; i++) o[i] = 0.0f;
		const JmRoiClip c = jm_roi_clip(rois[r], count, w, h);
		status[r] = c.status != JSMPEG_HIP_ROI_EMPTY && present[rois[r].row] ? (uint8_t)c.status : (uint8_t)JSMPEG_HIP_ROI_EMPTY;
		if (status[r] == JSMPEG_HIP_ROI_EMPTY) continue;
		const JmTensorPlan p = jm_tensor_roi_plan(p0, c);
		const uint8_t *Y = frames + (size_t)rois[r].row * frame_bytes, *Cr = Y + (size_t)cw * ch, *Cb = Cr + (size_t)(cw >> 1) * (ch >> 1);
		for (uint32_t oy = 0; oy < p.out_h; oy++) {
			const JmTaps vt = jm_tp_taps(p.ay, (int32_t)oy);
			for (uint32_t ox = 0; ox < p.out_w; ox++) {
				const JmTaps ht = jm_tp_taps(p.ax, (int32_t)ox);
				float acc[3] = { 0.0f, 0.0f, 0.0f };
				for (int32_t jy = 0; jy < vt.xsize; jy++) {
					const uint32_t sy = p.crop_y + (uint32_t)(vt.xmin + jy);
					float hh[3] = { 0.0f, 0.0f, 0.0f };
					for (int32_t jx = 0; jx < ht.xsize; jx++) {
						const uint32_t sx = p.crop_x + (uint32_t)(ht.xmin + jx);
						const size_t ci = (size_t)(sy >> 1) * (cw >> 1) + (sx >> 1);
						const uint32_t v = jm_tp_rgb(Y[(size_t)sy * cw + sx], Cr[ci], Cb[ci]);
						const float wx = jm_tp_weight(p.ax, ht, jx);
						for (int ch3 = 0; ch3 < 3; ch3++) hh[ch3] += wx * (float)((v >> (8 * ch3)) & 255u);
					}
					const float wy = jm_tp_weight(p.ay, vt, jy);
					for (int ch3 = 0; ch3 < 3; ch3++) acc[ch3] += wy * hh[ch3];
				}
				for (int ch3 = 0; ch3 < 3; ch3++) {
					const int oc = p.order == JSMPEG_HIP_TENSOR_BGR ? 2 - ch3 : ch3;
					o[((size_t)oc * p.out_h + oy) * p.out_w + ox] = jm_tp_value(p, oc, acc[ch3]);
				}
			}
		}
	}
	return 0;
}
