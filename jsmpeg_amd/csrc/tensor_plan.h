/*
 * Decoded pictures as resized RGB tensors (include/jsmpeg_hip.h part 7): what k_tensor (kernels.hip) and the CPU simulator
 * (tests/sim/sim_tensor.cpp) share -- the descriptor check, the per-axis taps and the per-pixel colour.  Host + device.
 *
 * The value of output pixel (ox, oy), channel c:
 *   source RGB    display pixel (x, y) of the picture: luma Y[y * coded_width + x], chroma at [(y >> 1) * (coded_width >> 1)
 *                 + (x >> 1)], the reference's Canvas2D integer BT.601 (k_rgba's formula).  For an odd width this is NOT
 *                 read_rgba's picture: no running-index shear, no 255 fill -- the tensor is the picture, not the canvas;
 *   crop          (crop_x, crop_y, crop_width, crop_height) of it; every tap lies inside the crop;
 *   resize        torch.nn.functional.interpolate(mode="bilinear", align_corners=False, antialias=aa) over the crop's
 *                 float RGB: per axis a list of taps (xmin, xsize, weights), horizontal pass first, then vertical, each
 *                 a sum in tap order starting with tap 0 -- torch's separable order;
 *   output        float: (v / 255 - mean[c]) / std[c] as v * a[c] + b[c]; uint8: rint(v) clamped to 0 .. 255.
 * An axis whose size does not change is a copy (one tap of weight 1), as torch skips it.
 *
 * Rows from regions of interest (jsmpeg_hip_*_render_tensor_rois, k_tensor_roi, tests/sim/sim_tensor_roi.cpp): the crop of
 * every row is a box from device memory, clipped to the picture by jm_roi_clip; jm_tensor_roi_plan gives the row the plan
 * that jm_tensor_plan gives a descriptor with that crop, so the value above holds per row.
 */
#pragma once
#include <stdint.h>
#include <string.h>

#include "jsmpeg_hip.h"

#if defined(__HIPCC__)
#define JM_TP_FN __host__ __device__ inline
#else
#include <math.h>
#define JM_TP_FN static inline
#endif

#define JM_TENSOR_MAX_SIDE 4096u

/* One axis of the resize: in (crop) size -> out size; torch's _compute_indices_weights_aa / compute_indices_weights_linear */
struct JmTapAxis {
	float scale, support, invscale;
	int32_t in, out;
	uint32_t aa;
};
/* Output index i's taps: source indices xmin .. xmin + xsize - 1; p: the centre (AA) or lambda (plain); q: 1 / total weight (AA) */
struct JmTaps {
	int32_t xmin, xsize;
	float p, q;
};

JM_TP_FN JmTapAxis jm_tp_axis(int32_t in, int32_t out, uint32_t aa) {
	JmTapAxis a;
	a.in = in; a.out = out; a.aa = aa;
	a.scale = (float)in / (float)out;                                  /* area_pixel_compute_scale, align_corners = False */
	a.support = (aa && a.scale >= 1.0f) ? a.scale : 1.0f;              /* interp_size (2) * 0.5, widened by the scale */
	a.invscale = (aa && a.scale >= 1.0f) ? (float)(1.0 / (double)a.scale) : 1.0f;
	return a;
}

/* the triangle filter of the AA form, at tap j of output i whose centre is `center` */
JM_TP_FN float jm_tp_filter(const JmTapAxis &a, int32_t xmin, int32_t j, float center) {
	float x = ((float)(j + xmin) - center + 0.5f) * a.invscale;
	x = x < 0.0f ? -x : x;
	return x < 1.0f ? 1.0f - x : 0.0f;
}

JM_TP_FN JmTaps jm_tp_taps(const JmTapAxis &a, int32_t i) {
	JmTaps t;
	if (a.in == a.out) { t.xmin = i; t.xsize = 1; t.p = 0.0f; t.q = 1.0f; return t; }
	if (a.aa) {
		const float center = (float)((double)a.scale * ((double)i + 0.5));
		const int32_t lo = (int32_t)((double)(center - a.support) + 0.5);             /* truncation, as torch's int64 cast */
		const int32_t hi = (int32_t)((double)(center + a.support) + 0.5);
		t.xmin = lo > 0 ? lo : 0;
		t.xsize = (hi < a.in ? hi : a.in) - t.xmin;
		float total = 0.0f;
		for (int32_t j = 0; j < t.xsize; j++) total += jm_tp_filter(a, t.xmin, j, center);
		t.p = center;
		t.q = total != 0.0f ? 1.0f / total : 0.0f;
	} else {
		float real = fmaf(a.scale, (float)i + 0.5f, -0.5f);                           /* area_pixel_compute_source_index (torch's
		                                                                                 build contracts it into one fma) */
		real = real < 0.0f ? 0.0f : real;
		int32_t i0 = (int32_t)floorf(real);
		i0 = i0 < a.in - 1 ? i0 : a.in - 1;                                            /* guard_index_and_lambda */
		float lambda = real - (float)i0;
		lambda = lambda < 0.0f ? 0.0f : lambda > 1.0f ? 1.0f : lambda;
		t.xmin = i0;
		t.xsize = i0 < a.in - 1 ? 2 : 1;                                               /* the index guard: both taps on the last pixel */
		t.p = lambda; t.q = 1.0f;
	}
	return t;
}

/* weight of tap j (0 <= j < t.xsize) */
JM_TP_FN float jm_tp_weight(const JmTapAxis &a, const JmTaps &t, int32_t j) {
	if (a.in == a.out) return 1.0f;
	if (a.aa) return jm_tp_filter(a, t.xmin, j, t.p) * t.q;
	if (t.xsize == 1) return 1.0f;
	return j == 0 ? 1.0f - t.p : t.p;
}

/* the reference's Canvas2D integer BT.601 (k_rgba): R | G << 8 | B << 16 */
JM_TP_FN uint32_t jm_tp_rgb(int y, int cr, int cb) {
	const int r = (cr + ((cr * 103) >> 8)) - 179;
	const int g = ((cb * 88) >> 8) - 44 + ((cr * 183) >> 8) - 91;
	const int b = (cb + ((cb * 198) >> 8)) - 227;
	const int R = y + r, G = y - g, B = y + b;
	return (uint32_t)(R < 0 ? 0 : R > 255 ? 255 : R) | ((uint32_t)(G < 0 ? 0 : G > 255 ? 255 : G) << 8) |
	       ((uint32_t)(B < 0 ? 0 : B > 255 ? 255 : B) << 16);
}

/* What a launch needs besides the frames, worked out once on the host from a checked descriptor */
struct JmTensorPlan {
	JmTapAxis ax, ay;                /* horizontal, vertical */
	uint32_t crop_x, crop_y;
	uint32_t out_w, out_h;
	uint32_t dtype, layout, order;
	float a[3], b[3];                /* per OUTPUT channel: value = v * a + b (float dtypes) */
};

/* The descriptor check: 0, or a message (static text) of what the contract does not cover.  `w` x `h`: the display size. */
JM_TP_FN const char *jm_tensor_check(const jsmpeg_hip_tensor_desc_t *d, uint32_t w, uint32_t h) {
	if (!d) return "null tensor descriptor";
	if (d->width < 1 || d->width > JM_TENSOR_MAX_SIDE || d->height < 1 || d->height > JM_TENSOR_MAX_SIDE)
		return "tensor width and height must be 1 .. 4096";
	if (d->dtype > JSMPEG_HIP_TENSOR_F32) return "unknown tensor dtype";
	if (d->layout > JSMPEG_HIP_TENSOR_NHWC) return "unknown tensor layout";
	if (d->order > JSMPEG_HIP_TENSOR_BGR) return "unknown tensor channel order";
	if (d->antialias > 1) return "antialias must be 0 or 1";
	const bool whole = d->crop_width == 0 && d->crop_height == 0;
	if (whole ? (d->crop_x || d->crop_y)
	          : (d->crop_width == 0 || d->crop_height == 0 || (uint64_t)d->crop_x + d->crop_width > w ||
	             (uint64_t)d->crop_y + d->crop_height > h))
		return "crop rectangle outside the picture";
	if (d->dtype != JSMPEG_HIP_TENSOR_U8)
		for (int c = 0; c < 3; c++) {
			if (!(d->std[c] - d->std[c] == 0.0f) || !(d->mean[c] - d->mean[c] == 0.0f))      /* (false for inf and NaN) */
				return "tensor mean / std must be finite";
			if (d->std[c] == 0.0f) return "tensor std must not be 0";
		}
	return 0;
}

/* ... and the plan of a descriptor that passed it */
JM_TP_FN JmTensorPlan jm_tensor_plan(const jsmpeg_hip_tensor_desc_t *d, uint32_t w, uint32_t h) {
	JmTensorPlan p;
	const bool whole = d->crop_width == 0 && d->crop_height == 0;
	const uint32_t cw = whole ? w : d->crop_width, ch = whole ? h : d->crop_height;
	p.crop_x = whole ? 0 : d->crop_x; p.crop_y = whole ? 0 : d->crop_y;
	p.out_w = d->width; p.out_h = d->height;
	p.ax = jm_tp_axis((int32_t)cw, (int32_t)d->width, d->antialias);
	p.ay = jm_tp_axis((int32_t)ch, (int32_t)d->height, d->antialias);
	p.dtype = d->dtype; p.layout = d->layout; p.order = d->order;
	for (int c = 0; c < 3; c++) {
		p.a[c] = d->dtype == JSMPEG_HIP_TENSOR_U8 ? 1.0f : 1.0f / (255.0f * d->std[c]);
		p.b[c] = d->dtype == JSMPEG_HIP_TENSOR_U8 ? 0.0f : -d->mean[c] / d->std[c];
	}
	return p;
}

/* ---- rows from regions of interest (jsmpeg_hip_*_render_tensor_rois; k_tensor_roi, tests/sim/sim_tensor_roi.cpp) ---- */

/* A box clipped to the w x h picture of a call with `count` pictures: the rectangle, and the status the header defines (the
 * fourth reason for EMPTY, a picture list entry with no picture, is the caller's to add: it knows the slots).  64-bit sums:
 * x + width does not wrap for any int32 pair. */
struct JmRoiClip {
	int32_t x, y, width, height;
	uint32_t status;
};
JM_TP_FN JmRoiClip jm_roi_clip(const jsmpeg_hip_roi_t &r, uint32_t count, uint32_t w, uint32_t h) {
	JmRoiClip c;
	c.x = 0; c.y = 0; c.width = 0; c.height = 0; c.status = JSMPEG_HIP_ROI_EMPTY;
	if (r.row < 0 || (uint32_t)r.row >= count || r.width <= 0 || r.height <= 0) return c;
	const int64_t x0 = r.x > 0 ? (int64_t)r.x : 0, y0 = r.y > 0 ? (int64_t)r.y : 0;
	const int64_t xe = (int64_t)r.x + r.width, ye = (int64_t)r.y + r.height;
	const int64_t x1 = xe < (int64_t)w ? xe : (int64_t)w, y1 = ye < (int64_t)h ? ye : (int64_t)h;
	if (x1 <= x0 || y1 <= y0) return c;
	c.x = (int32_t)x0; c.y = (int32_t)y0; c.width = (int32_t)(x1 - x0); c.height = (int32_t)(y1 - y0);
	c.status = (c.x == r.x && c.y == r.y && c.width == r.width && c.height == r.height) ? JSMPEG_HIP_ROI_INSIDE : JSMPEG_HIP_ROI_CLIPPED;
	return c;
}

/* The descriptor check of a call with boxes: the descriptor's own crop must be unset */
JM_TP_FN const char *jm_tensor_roi_check(const jsmpeg_hip_tensor_desc_t *d, uint32_t w, uint32_t h) {
	if (d && (d->crop_x || d->crop_y || d->crop_width || d->crop_height)) return "crop and rois exclude each other";
	return jm_tensor_check(d, w, h);
}

/* ... and the plan of one row: the call's plan (the descriptor's, whole picture) with the crop and both axes of a clipped box
 * (status 1 or 2) -- what jm_tensor_plan makes of the same descriptor with crop = that box */
JM_TP_FN JmTensorPlan jm_tensor_roi_plan(JmTensorPlan p, const JmRoiClip &c) {
	p.crop_x = (uint32_t)c.x; p.crop_y = (uint32_t)c.y;
	p.ax = jm_tp_axis(c.width, (int32_t)p.out_w, p.ax.aa);
	p.ay = jm_tp_axis(c.height, (int32_t)p.out_h, p.ay.aa);
	return p;
}

/* the output element of value v (0 .. 255 scale) in output channel c: float for F32; the bits of an F16 / BF16 (round to nearest
 * even) or the U8 in the low bits */
JM_TP_FN float jm_tp_value(const JmTensorPlan &p, int c, float v) {
	if (p.dtype == JSMPEG_HIP_TENSOR_U8) {
		const float r = rintf(v);
		return r < 0.0f ? 0.0f : r > 255.0f ? 255.0f : r;
	}
	const float a = c == 0 ? p.a[0] : c == 1 ? p.a[1] : p.a[2], b = c == 0 ? p.b[0] : c == 1 ? p.b[1] : p.b[2];
	return v * a + b;
}
JM_TP_FN uint16_t jm_tp_bf16(float f) {
	uint32_t u;
	memcpy(&u, &f, 4);
	u += 0x7fffu + ((u >> 16) & 1u);
	return (uint16_t)(u >> 16);
}
