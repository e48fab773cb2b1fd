// Official SUN-RGBD detection evaluation of one class (t3d.h t3d_sunrgbd_eval), in place of the MATLAB chain
// evaluation/sunrgbd/detection/computePRCurve3D.m -> SUNRGBDtoolbox/mBB/bb3dOverlapCloseForm.m (get_corners_of_bb3d.m, cuboidVolume.m,
// cuboidIntersectionVolume.c) -> get_average_precision.m.  Five launches on the caller's stream, no host synchronisation between them:
//   k_eval_footprints  one thread per box (detections, then ground truth): get_corners_of_bb3d.m:14-44 -> the 10-vector
//                      x1 y1 .. x4 y4 zMin zMax of bb3dOverlapCloseForm.m:17-30 and cuboidVolume.m:3-5;
//   k_eval_rank        one thread per detection: its position in the stable descending order of the confidences, by counting
//                      (computePRCurve3D.m:20);
//   k_eval_match       one thread per detection: the overlaps with the ground truth of its own image (every other entry of allOverlaps
//                      is zeroed, :30-31), the running maximum with the first index on ties, `< eps`, `>= threshold` (:32-36), and the
//                      claim atomicMin(first sorted position per ground-truth box) that stands for unique(gtIdx,'first') (:39);
//   k_eval_flags       tp / fp / difficult / gtAssignment per detection, isMissed per ground-truth box (:40-75);
//   k_eval_curve       one workgroup: integer scans of tp and fp over the sorted order, recall and precision from the integer counts
//                      (:78-81), the right-to-left running maximum and the area of get_average_precision.m:15-23, summed in a fixed order.
// Everything is fp64.  The only atomics are integer minima, so every output is a function of the inputs alone.
// The workspace layout, the footprint, the overlap, the scan and the curve are in sunrgbd_eval_dev.h, which the diagnosis shares.
#include "sunrgbd_eval_dev.h"

namespace {

__global__ __launch_bounds__(EV_THREADS) void k_eval_footprints(const t3d_sunrgbd_eval_args p) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const EvWork w = ev_work(p.workspace, p.P, p.G);
  double fp[EV_FP];
  if (i < p.P) {
    ev_footprint(p.det_centroid + (size_t)i * 3, p.det_basis + (size_t)i * 9, p.det_coeffs + (size_t)i * 3, fp);
#pragma unroll
    for (int k = 0; k < EV_FP; ++k) w.fp_det[(size_t)i * EV_FP + k] = fp[k];
  } else if (i < p.P + p.G) {
    const int g = i - p.P;
    ev_footprint(p.gt_centroid + (size_t)g * 3, p.gt_basis + (size_t)g * 9, p.gt_coeffs + (size_t)g * 3, fp);
#pragma unroll
    for (int k = 0; k < EV_FP; ++k) w.fp_gt[(size_t)g * EV_FP + k] = fp[k];
    w.gt_first[g] = EV_UNCLAIMED;
  }
}

// MATLAB's sort(.,'descend'): NaN first, then decreasing, ties in file order
__device__ __forceinline__ bool ev_before(double a, double b) { return (a != a) ? (b == b) : (a > b); }
__device__ __forceinline__ bool ev_same(double a, double b) { return a == b || (a != a && b != b); }

__global__ __launch_bounds__(EV_THREADS) void k_eval_rank(const t3d_sunrgbd_eval_args p) {
  __shared__ double tile[EV_THREADS];
  const int i = blockIdx.x * EV_THREADS + threadIdx.x;
  const double si = i < p.P ? p.det_confidence[i] : 0.0;
  int r = 0;
  for (int j0 = 0; j0 < p.P; j0 += EV_THREADS) {
    __syncthreads();
    if (j0 + (int)threadIdx.x < p.P) tile[threadIdx.x] = p.det_confidence[j0 + threadIdx.x];
    __syncthreads();
    const int nt = min(EV_THREADS, p.P - j0);
    for (int k = 0; k < nt; ++k) {
      const double sj = tile[k];
      r += (ev_before(sj, si) || (j0 + k < i && ev_same(sj, si))) ? 1 : 0;
    }
  }
  if (i < p.P) {
    ev_work(p.workspace, p.P, p.G).rank[i] = r;
    p.order[r] = i;                          // r is a permutation of [0, P): a strict total order
  }
}

__global__ __launch_bounds__(EV_THREADS) void k_eval_match(const t3d_sunrgbd_eval_args p) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= p.P) return;
  const EvWork w = ev_work(p.workspace, p.P, p.G);
  const int img = p.det_image[i];
  int lo = 0, hi = p.n_images;                // the first image id >= img
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (p.image_ids[mid] < img) lo = mid + 1; else hi = mid;
  }
  int g0 = 0, g1 = 0;
  if (lo < p.n_images && p.image_ids[lo] == img) { g0 = p.image_gt_offsets[lo]; g1 = p.image_gt_offsets[lo + 1]; }
  g0 = max(g0, 0);
  g1 = min(g1, p.G);
  double a[EV_FP];
#pragma unroll
  for (int k = 0; k < EV_FP; ++k) a[k] = w.fp_det[(size_t)i * EV_FP + k];
  int64_t o0 = 0, o1 = 0;
  if (p.overlaps) { o0 = p.overlap_offsets[i]; o1 = p.overlap_offsets[i + 1]; }
  // [m, idx] = max(row): the first index of the largest entry; a row of zeros gives index 1 and is cleared by `< eps`
  double best = 0.0;
  int best_g = -1;
  for (int k = g0; k < g1; ++k) {
    const int g = p.image_gt[k];
    double ov = 0.0;
    if (g >= 0 && g < p.G && p.gt_image[g] == img) {
      double b[EV_FP];
#pragma unroll
      for (int t = 0; t < EV_FP; ++t) b[t] = w.fp_gt[(size_t)g * EV_FP + t];
      ov = ev_overlap(a, b);
      if (ov > best) { best = ov; best_g = g; }
    }
    if (p.overlaps && o0 + (k - g0) < o1) {
      p.overlaps[o0 + (k - g0)] = ov;
      p.overlap_gt[o0 + (k - g0)] = g;
    }
  }
  if (best < EV_EPS) best_g = -1;
  p.max_overlap[i] = best;
  p.gt_idx[i] = best_g + 1;
  if (best_g >= 0 && best >= p.threshold) atomicMin(&w.gt_first[best_g], w.rank[i]);      // integer minimum: order-independent
}

__global__ __launch_bounds__(EV_THREADS) void k_eval_flags(const t3d_sunrgbd_eval_args p) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const EvWork w = ev_work(p.workspace, p.P, p.G);
  if (i < p.P) {
    const int g = p.gt_idx[i] - 1;
    const bool claims = g >= 0 && p.max_overlap[i] >= p.threshold;            // gtIdx after gtIdx(~isOverlapping) = 0
    const bool first = claims && w.gt_first[g] == w.rank[i];
    const bool dc = claims && p.gt_difficult != nullptr && p.gt_difficult[g] != 0;
    p.is_tp[i] = (first && !dc) ? 1 : 0;
    p.is_fp[i] = (!first && !dc) ? 1 : 0;
    p.gt_assignment[i] = first ? g + 1 : 0;
  }
  if (i < p.G) p.is_missed[i] = w.gt_first[i] == EV_UNCLAIMED ? 1 : 0;
}

__global__ __launch_bounds__(EV_CURVE_THREADS) void k_eval_curve(const t3d_sunrgbd_eval_args p) {
  __shared__ int wsum[EV_CURVE_THREADS / 64];
  __shared__ double part[EV_CURVE_THREADS / 64];
  // sum(~isDifficult)
  int c = 0;
  for (int g = threadIdx.x; g < p.G; g += EV_CURVE_THREADS) c += (p.gt_difficult == nullptr || p.gt_difficult[g] == 0) ? 1 : 0;
  int n_pos;
  ev_block_scan(c, wsum, n_pos);
  ev_curve(p.P, p.G > 0, n_pos, p.order, [&](int i) { return (int)p.is_tp[i]; }, [&](int i) { return (int)p.is_fp[i]; }, p.recall,
           p.precision, p.ap, wsum, part);
}

}  // namespace

extern "C" int t3d_sunrgbd_eval(const t3d_sunrgbd_eval_args* a, t3d_stream_t stream) {
  T3D_ABI_TAKE(sunrgbd_eval_args, a);
  if (!a || !a->ap) return T3D_ERR_ARG;
  if (a->P < 0 || a->G < 0 || a->n_images < 0 || a->P > T3D_SUNRGBD_EVAL_MAX_BOXES || a->G > T3D_SUNRGBD_EVAL_MAX_BOXES) return T3D_ERR_SHAPE;
  if (a->P > 0 && (!a->det_centroid || !a->det_basis || !a->det_coeffs || !a->det_confidence || !a->det_image || !a->order ||
                   !a->max_overlap || !a->gt_idx || !a->is_tp || !a->is_fp || !a->gt_assignment || !a->precision || !a->recall))
    return T3D_ERR_ARG;
  if (a->G > 0 && (!a->gt_centroid || !a->gt_basis || !a->gt_coeffs || !a->gt_image || !a->is_missed || !a->image_gt)) return T3D_ERR_ARG;
  if (a->n_images > 0 && (!a->image_ids || !a->image_gt_offsets)) return T3D_ERR_ARG;
  if (a->overlaps && (!a->overlap_offsets || !a->overlap_gt)) return T3D_ERR_ARG;
  if (a->P + a->G > 0 && (!a->workspace || a->workspace_bytes < T3D_SUNRGBD_EVAL_WORKSPACE_BYTES(a->P, a->G))) return T3D_ERR_ARG;
  const hipStream_t st = static_cast<hipStream_t>(stream);
  const auto blocks = [](int n) { return dim3((n + EV_THREADS - 1) / EV_THREADS); };
  if (a->P + a->G > 0) {
    T3D_LAUNCH(k_eval_footprints, blocks(a->P + a->G), dim3(EV_THREADS), 0, st, *a);
    T3D_CHECK_LAUNCH();
  }
  if (a->P > 0) {
    T3D_LAUNCH(k_eval_rank, blocks(a->P), dim3(EV_THREADS), 0, st, *a);
    T3D_CHECK_LAUNCH();
    T3D_LAUNCH(k_eval_match, blocks(a->P), dim3(EV_THREADS), 0, st, *a);
    T3D_CHECK_LAUNCH();
  }
  if (a->P + a->G > 0) {
    T3D_LAUNCH(k_eval_flags, blocks(a->P > a->G ? a->P : a->G), dim3(EV_THREADS), 0, st, *a);
    T3D_CHECK_LAUNCH();
  }
  T3D_LAUNCH(k_eval_curve, dim3(1), dim3(EV_CURVE_THREADS), 0, st, *a);
  T3D_CHECK_LAUNCH();
  return T3D_OK;
}
