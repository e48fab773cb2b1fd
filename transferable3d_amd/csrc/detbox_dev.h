// A decoded box as the stages behind t3d_detect_decode pass it on: its label-format row (h, w, l, tx, ty, tz, ry), its corners and the IoU
// of two corner sets under a call's metric.  detect.hip writes the corners, fuse.hip and ensemble.hip write them again from a fused label,
// and the fp64 specifications (tests/fake_fuse.py, tests/fake_ensemble.py) rely on all three rounding alike: this is the one formula.
//
// Contraction: what is specified here is NumPy, elementwise -- no fused multiply-adds.  A file-scope pragma in a header would run on to the
// end of whoever includes it, so every function below that does arithmetic turns contraction off at the start of its own body, and the
// header may be included anywhere, before or after a unit's own pragma.  boxgeom_dev.h is included from here as the units included it
// before: ahead of their pragma, contracted, in every unit alike.
#pragma once
#include "common.h"
#include "boxgeom_dev.h"

namespace {

__device__ __forceinline__ bool detbox_finite(double x) { return fabs(x) <= 1.7976931348623157e308; }      // false for a NaN

// A vote's weight: what the caller gave, or 0 for a negative one, an infinity or a NaN.
__device__ __forceinline__ double detbox_weight(float w) {
  const double x = (double)w;
  return (detbox_finite(x) && x >= 0.0) ? x : 0.0;
}

// x brought into (-pi, pi]
__device__ __forceinline__ double detbox_wrap(double x) {
#pragma clang fp contract(off)
  const double PI = 3.14159265358979323846, TWO_PI = 2.0 * PI;
  return x - TWO_PI * ceil((x - PI) / TWO_PI);
}

__device__ __forceinline__ bool detbox_label_ok(const float* l) {      // a label-format row without a NaN or an infinity
  bool ok = true;
#pragma unroll
  for (int c = 0; c < 7; ++c) ok = ok && detbox_finite((double)l[c]);
  return ok;
}

// Corner c of get_3d_box((l, w, h), ry, (tx, yc, tz)) (roi_seg_box3d_dataset.py:86-101), cr and sn the cosine and sine of ry:
// x (l, l, -l, -l, ..) / 2, y (h x4, -h x4) / 2, z (w, -w, -w, w, ..) / 2.  yc is the centre's height, ty - h / 2 of a label.
__device__ __forceinline__ void detbox_corner(float h, float w, float l, float cr, float sn, float tx, float yc, float tz, int c, float* o) {
#pragma clang fp contract(off)
  const float x = ((c & 2) ? -l : l) / 2.0f, y = (c < 4 ? h : -h) / 2.0f, z = (((c + 1) & 2) ? -w : w) / 2.0f;
  o[0] = (cr * x + sn * z) + tx;
  o[1] = y + yc;
  o[2] = (-sn * x + cr * z) + tz;
}

__device__ __forceinline__ void detbox_corners(float h, float w, float l, float ry, float tx, float yc, float tz, float* k) {
  const float cr = cosf(ry), sn = sinf(ry);
#pragma unroll
  for (int c = 0; c < 8; ++c) detbox_corner(h, w, l, cr, sn, tx, yc, tz, c, k + c * 3);
}

// The IoU a call asked for (t3d.h T3D_NMS_IOU3D / T3D_NMS_IOU2D) of two corner sets.  The callers shift their boxes towards the origin
// first, each in its own way, and the argument order is theirs too: both are pinned by their specifications.
__device__ __forceinline__ float iou_by_metric(const float* k1, const float* k2, int metric) {
  float iou2d;
  const float iou3d = boxgeom::box3d_iou_corners(k1, k2, &iou2d);
  return metric == T3D_NMS_IOU2D ? iou2d : iou3d;
}

}  // namespace
