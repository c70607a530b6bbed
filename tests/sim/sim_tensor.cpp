/* TEST-ONLY simulator of k_tensor (kernels.hip): tensor_plan.h's taps, colour and value functions run per output pixel in
 * scalar loops on the CPU, so that tests/test_tensor_plan.py holds them against torch's F.interpolate without a GPU. */
#include <math.h>
#include <stdint.h>

#include "tensor_plan.h"

/* "" or the descriptor check's message */
extern "C" const char *sim_tensor_check(const jsmpeg_hip_tensor_desc_t *d, uint32_t w, uint32_t h) {
	const char *m = jm_tensor_check(d, w, h);
	return m ? m : "";
}

/* One picture (Y | Cr | Cb of coded_width x coded_height, display w x h) -> out[3][height][width] floats in the tensor's
 * channel order: the float value of a float dtype, the rounded value of U8.  0, or -1 for a descriptor the check refuses. */
extern "C" int sim_tensor(const uint8_t *frame, uint32_t cw, uint32_t ch, uint32_t w, uint32_t h, const jsmpeg_hip_tensor_desc_t *d,
                          float *out) {
	if (jm_tensor_check(d, w, h)) return -1;
	const JmTensorPlan p = jm_tensor_plan(d, w, h);
	const uint8_t *Y = frame, *Cr = frame + (size_t)cw * ch, *Cb = Cr + (size_t)(cw >> 1) * (ch >> 1);
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
					for (int c = 0; c < 3; c++) hh[c] += wx * (float)((v >> (8 * c)) & 255u);
				}
				const float wy = jm_tp_weight(p.ay, vt, jy);
				for (int c = 0; c < 3; c++) acc[c] += wy * hh[c];
			}
			for (int c = 0; c < 3; c++) {
				const int oc = p.order == JSMPEG_HIP_TENSOR_BGR ? 2 - c : c;
				out[((size_t)oc * p.out_h + oy) * p.out_w + ox] = jm_tp_value(p, oc, acc[c]);
			}
		}
	}
	return 0;
}

/* the kernel's bfloat16 rounding */
extern "C" uint16_t sim_bf16(float f) { return jm_tp_bf16(f); }
