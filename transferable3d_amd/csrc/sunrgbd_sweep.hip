// The official evaluation of one class for many subsets of its detections (t3d.h t3d_sunrgbd_eval_sweep): the evaluation of
// sunrgbd_eval.hip, then three launches on the same stream that read what it left on the device -- the ranks in its workspace, max_overlap,
// gt_idx and order among its outputs.  The overlaps and the best box of a detection do not depend on the other detections, and the
// stable order of a subset is the induced order, so a configuration needs only its own claims and its own curve:
//   k_sweep_unclaim  first[m, g] = unclaimed, for every configuration m and box g;
//   k_sweep_claim    one thread per (configuration, detection): a selected detection that claims its box enters its rank there by
//                    atomicMin, as k_eval_match finds gt_first;
//   k_sweep_curves   one workgroup per configuration: ev_curve, the evaluation's curve, over the full order, where an unselected
//                    detection counts in neither sum (as a removed detection does in k_diag_curves), and the three counts.
// Everything is fp64.  The only atomics are integer minima, so every output is a function of the inputs alone.
#include "sunrgbd_eval_dev.h"

namespace {

constexpr int SW_Y = 32768;      // configurations along gridDim.y; gridDim.z carries the rest (a grid's y and z end at 65535)

__device__ __forceinline__ bool sw_selected(const t3d_sunrgbd_sweep_args& s, int m, int i) {
  const int col = s.det_index ? s.det_index[i] : i;
  return col >= 0 && col < s.mask_stride && s.mask[(size_t)m * s.mask_stride + col] != 0;
}

// the box (0-based) detection i claims, or -1: gtIdx after gtIdx(~isOverlapping) = 0, as k_eval_flags reads it
__device__ __forceinline__ int sw_claim(const t3d_sunrgbd_eval_args& p, int i) {
  const int g = p.gt_idx[i] - 1;
  return (g >= 0 && g < p.G && p.max_overlap[i] >= p.threshold) ? g : -1;
}

__global__ __launch_bounds__(EV_THREADS) void k_sweep_unclaim(const t3d_sunrgbd_eval_args p, const t3d_sunrgbd_sweep_args s) {
  const int g = blockIdx.x * EV_THREADS + threadIdx.x, m = blockIdx.z * SW_Y + blockIdx.y;
  if (g < p.G && m < s.M) static_cast<int32_t*>(s.workspace)[(size_t)m * p.G + g] = EV_UNCLAIMED;
}

__global__ __launch_bounds__(EV_THREADS) void k_sweep_claim(const t3d_sunrgbd_eval_args p, const t3d_sunrgbd_sweep_args s) {
  const int i = blockIdx.x * EV_THREADS + threadIdx.x, m = blockIdx.z * SW_Y + blockIdx.y;
  if (i >= p.P || m >= s.M) return;
  const int g = sw_claim(p, i);
  if (g < 0 || !sw_selected(s, m, i)) return;
  atomicMin(static_cast<int32_t*>(s.workspace) + (size_t)m * p.G + g, ev_work(p.workspace, p.P, p.G).rank[i]);      // integer minimum: order-independent
}

__global__ __launch_bounds__(EV_CURVE_THREADS) void k_sweep_curves(const t3d_sunrgbd_eval_args p, const t3d_sunrgbd_sweep_args s) {
  __shared__ int wsum[EV_CURVE_THREADS / 64];
  __shared__ double part[EV_CURVE_THREADS / 64];
  const int t = threadIdx.x, m = blockIdx.x;
  const int32_t* rank = ev_work(p.workspace, p.P, p.G).rank;
  const int32_t* first = static_cast<const int32_t*>(s.workspace) + (size_t)m * p.G;
  const auto tp_of = [&](int i) {
    if (!sw_selected(s, m, i)) return 0;
    const int g = sw_claim(p, i);
    return (g >= 0 && first[g] == rank[i]) ? 1 : 0;
  };
  const auto fp_of = [&](int i) { return sw_selected(s, m, i) ? 1 - tp_of(i) : 0; };
  int ctp = 0, cfp = 0, n_tp, n_fp;
  for (int i = t; i < p.P; i += EV_CURVE_THREADS) {
    ctp += tp_of(i);
    cfp += fp_of(i);
  }
  ev_block_scan(ctp, wsum, n_tp);
  ev_block_scan(cfp, wsum, n_fp);
  if (t == 0) {
    s.n_tp[m] = n_tp;
    s.n_fp[m] = n_fp;
    s.n_det[m] = n_tp + n_fp;
  }
  ev_curve(p.P, p.G > 0, p.G, p.order, tp_of, fp_of, (double*)nullptr, (double*)nullptr, s.ap + m, wsum, part);
}

}  // namespace

extern "C" int t3d_sunrgbd_eval_sweep(const t3d_sunrgbd_eval_args* a, const t3d_sunrgbd_sweep_args* s, t3d_stream_t stream) {
  T3D_ABI_TAKE(sunrgbd_eval_args, a);
  T3D_ABI_TAKE(sunrgbd_sweep_args, s);
  if (!a || !s || !s->ap || !s->n_det || !s->n_tp || !s->n_fp) return T3D_ERR_ARG;
  if (a->gt_difficult) return T3D_ERR_ARG;
  if (a->P < 0 || a->G < 0 || a->P > T3D_SUNRGBD_EVAL_MAX_BOXES || a->G > T3D_SUNRGBD_EVAL_MAX_BOXES) return T3D_ERR_SHAPE;
  if (s->M < 1 || s->M > T3D_SWEEP_MAX_CONFIGS) return T3D_ERR_SHAPE;
  if (a->P > 0 && (!s->mask || s->mask_stride < (s->det_index ? 1 : a->P))) return T3D_ERR_ARG;
  if (a->G > 0 && (!s->workspace || s->workspace_bytes < T3D_SUNRGBD_SWEEP_WORKSPACE_BYTES(s->M, a->G) ||
                   (reinterpret_cast<uintptr_t>(s->workspace) & 7u)))
    return T3D_ERR_ARG;
  const int e = t3d_sunrgbd_eval(a, stream);   // every output of the evaluation, by the evaluation itself; it launches nothing when it refuses
  if (e != T3D_OK) return e;
  const hipStream_t st = static_cast<hipStream_t>(stream);
  const int my = s->M < SW_Y ? s->M : SW_Y, mz = (s->M + SW_Y - 1) / SW_Y;
  const auto blocks = [&](int n) { return dim3((n + EV_THREADS - 1) / EV_THREADS, my, mz); };
  if (a->P > 0 && a->G > 0) {                  // (without detections or without boxes nobody claims, and the curves read no claim)
    T3D_LAUNCH(k_sweep_unclaim, blocks(a->G), dim3(EV_THREADS), 0, st, *a, *s);
    T3D_CHECK_LAUNCH();
    T3D_LAUNCH(k_sweep_claim, blocks(a->P), dim3(EV_THREADS), 0, st, *a, *s);
    T3D_CHECK_LAUNCH();
  }
  T3D_LAUNCH(k_sweep_curves, dim3(s->M), dim3(EV_CURVE_THREADS), 0, st, *a, *s);
  T3D_CHECK_LAUNCH();
  return T3D_OK;
}
