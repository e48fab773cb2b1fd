// Diagnosis of one class's detection errors (t3d.h t3d_sunrgbd_diagnose): the evaluation of sunrgbd_eval.hip, then four launches on the
// same stream that read what it left on the device -- the footprints and ranks in its workspace, max_overlap, gt_idx, is_tp, is_fp,
// is_missed and order among its outputs -- with no host synchronisation between any of them:
//   k_diag_prepare  one thread per other-class box: its footprint (ev_footprint); one per own-class box: no LOC detection yet;
//   k_diag_match    one thread per detection: the overlaps (ev_overlap) with the other-class boxes of its image, the maximum with the
//                   first index on ties and `< eps`, as k_eval_match; its kind; a LOC detection enters its rank at its box by atomicMin;
//   k_diag_states   one thread per own-class box: claimed / missed but localised / missed;
//   k_diag_curves   nine workgroups: eight run ev_curve, the evaluation's curve, on the eight fixed variants; the ninth counts the
//                   kinds and the states by workgroup scans.
// Everything is fp64.  The only atomics are integer minima, so every output is a function of the inputs alone.
#include "sunrgbd_eval_dev.h"

namespace {

constexpr int DG_KINDS = 6, DG_STATES = 3, DG_FIXES = 8;

struct DgWork {
  double* fp_other;     // [Go, 11]
  int32_t* loc_first;   // [G] smallest sorted position among the LOC detections whose best box this is
};

__host__ __device__ inline DgWork dg_work(void* ws, int G, int Go) {
  DgWork w;
  w.fp_other = static_cast<double*>(ws);
  w.loc_first = reinterpret_cast<int32_t*>(w.fp_other + (size_t)Go * EV_FP);
  return w;
}

__global__ __launch_bounds__(EV_THREADS) void k_diag_prepare(const t3d_sunrgbd_eval_args p, const t3d_sunrgbd_diagnose_args d) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const DgWork w = dg_work(d.workspace, p.G, d.Go);
  if (i < d.Go) {
    double fp[EV_FP];
    ev_footprint(d.other_centroid + (size_t)i * 3, d.other_basis + (size_t)i * 9, d.other_coeffs + (size_t)i * 3, fp);
#pragma unroll
    for (int k = 0; k < EV_FP; ++k) w.fp_other[(size_t)i * EV_FP + k] = fp[k];
  }
  if (i < p.G) w.loc_first[i] = EV_UNCLAIMED;
}

__global__ __launch_bounds__(EV_THREADS) void k_diag_match(const t3d_sunrgbd_eval_args p, const t3d_sunrgbd_diagnose_args d) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= p.P) return;
  const EvWork ew = ev_work(p.workspace, p.P, p.G);
  const DgWork w = dg_work(d.workspace, p.G, d.Go);
  const int img = p.det_image[i];
  int lo = 0, hi = d.n_other_images;          // the first image id >= img
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (d.other_image_ids[mid] < img) lo = mid + 1; else hi = mid;
  }
  int g0 = 0, g1 = 0;
  if (lo < d.n_other_images && d.other_image_ids[lo] == img) { g0 = d.other_image_offsets[lo]; g1 = d.other_image_offsets[lo + 1]; }
  g0 = max(g0, 0);
  g1 = min(g1, d.Go);
  double a[EV_FP];
#pragma unroll
  for (int k = 0; k < EV_FP; ++k) a[k] = ew.fp_det[(size_t)i * EV_FP + k];
  double best = 0.0;
  int best_g = -1;
  for (int k = g0; k < g1; ++k) {
    const int g = d.other_image_list[k];
    if (g >= 0 && g < d.Go && d.other_image[g] == img) {
      double b[EV_FP];
#pragma unroll
      for (int t = 0; t < EV_FP; ++t) b[t] = w.fp_other[(size_t)g * EV_FP + t];
      const double ov = ev_overlap(a, b);
      if (ov > best) { best = ov; best_g = g; }
    }
  }
  if (best < EV_EPS) best_g = -1;
  d.other_overlap[i] = best;
  d.other_gt[i] = best_g + 1;
  // own-class evidence first
  const double o_s = p.max_overlap[i], t_f = p.threshold, t_b = d.bg_threshold;
  int kind;
  if (p.is_tp[i]) kind = T3D_DIAG_TP;
  else if (o_s >= t_f) kind = T3D_DIAG_DUP;
  else if (o_s >= t_b) kind = T3D_DIAG_LOC;
  else if (best >= t_f) kind = T3D_DIAG_CLS;
  else if (best >= t_b) kind = T3D_DIAG_BOTH;
  else kind = T3D_DIAG_BKG;
  d.kind[i] = (uint8_t)kind;
  const int g = p.gt_idx[i] - 1;
  if (kind == T3D_DIAG_LOC && g >= 0 && g < p.G) atomicMin(&w.loc_first[g], ew.rank[i]);      // integer minimum: order-independent
}

__global__ __launch_bounds__(EV_THREADS) void k_diag_states(const t3d_sunrgbd_eval_args p, const t3d_sunrgbd_diagnose_args d) {
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= p.G) return;
  const DgWork w = dg_work(d.workspace, p.G, d.Go);
  d.gt_state[g] = p.is_missed[g] == 0 ? 1 : (w.loc_first[g] != EV_UNCLAIMED ? 2 : 3);
}

__global__ __launch_bounds__(EV_CURVE_THREADS) void k_diag_curves(const t3d_sunrgbd_eval_args p, const t3d_sunrgbd_diagnose_args d) {
  __shared__ int wsum[EV_CURVE_THREADS / 64];
  __shared__ double part[EV_CURVE_THREADS / 64];
  const int t = threadIdx.x, fix = blockIdx.x;
  if (fix == DG_FIXES) {                      // the counts
    for (int k = 0; k < DG_KINDS; ++k) {
      int c = 0, n;
      for (int i = t; i < p.P; i += EV_CURVE_THREADS) c += d.kind[i] == k ? 1 : 0;
      ev_block_scan(c, wsum, n);
      if (t == 0) d.counts[k] = n;
    }
    for (int s = 1; s <= DG_STATES; ++s) {
      int c = 0, n;
      for (int g = t; g < p.G; g += EV_CURVE_THREADS) c += d.gt_state[g] == s ? 1 : 0;
      ev_block_scan(c, wsum, n);
      if (t == 0) d.gt_counts[s - 1] = n;
    }
    return;
  }
  // the boxes that leave the ground truth
  int c = 0, gone;
  if (fix == T3D_DIAG_FIX_MISSED || fix == T3D_DIAG_FIX_FN) {
    const int from = fix == T3D_DIAG_FIX_MISSED ? 3 : 2;
    for (int g = t; g < p.G; g += EV_CURVE_THREADS) c += d.gt_state[g] >= from ? 1 : 0;
  }
  ev_block_scan(c, wsum, gone);
  const int n_pos = p.G - gone;
  const int removed = fix == T3D_DIAG_FIX_CLS ? T3D_DIAG_CLS : fix == T3D_DIAG_FIX_BOTH ? T3D_DIAG_BOTH :
                      fix == T3D_DIAG_FIX_DUP ? T3D_DIAG_DUP : fix == T3D_DIAG_FIX_BKG ? T3D_DIAG_BKG : -1;
  const EvWork ew = ev_work(p.workspace, p.P, p.G);
  const DgWork w = dg_work(d.workspace, p.G, d.Go);
  // a LOC detection that becomes a true positive: the best-ranked one of a box in state 2
  const auto promoted = [&](int i) {
    const int g = p.gt_idx[i] - 1;
    return g >= 0 && g < p.G && d.gt_state[g] == 2 && w.loc_first[g] == ew.rank[i];
  };
  const auto tp_of = [&](int i) {
    const int k = d.kind[i];
    if (fix == T3D_DIAG_FIX_LOC && k == T3D_DIAG_LOC) return promoted(i) ? 1 : 0;
    return k == T3D_DIAG_TP ? 1 : 0;
  };
  const auto fp_of = [&](int i) {
    const int k = d.kind[i];
    if (k == T3D_DIAG_TP || fix == T3D_DIAG_FIX_FP || k == removed) return 0;
    if (fix == T3D_DIAG_FIX_LOC && k == T3D_DIAG_LOC) return 0;
    return 1;
  };
  ev_curve(p.P, n_pos > 0, n_pos, p.order, tp_of, fp_of, (double*)nullptr, (double*)nullptr, d.ap_fixed + fix, wsum, part);
}

}  // namespace

extern "C" int t3d_sunrgbd_diagnose(const t3d_sunrgbd_eval_args* a, const t3d_sunrgbd_diagnose_args* d, t3d_stream_t stream) {
  T3D_ABI_TAKE(sunrgbd_eval_args, a);
  T3D_ABI_TAKE(sunrgbd_diagnose_args, d);
  if (!a || !d || !d->counts || !d->gt_counts || !d->ap_fixed) return T3D_ERR_ARG;
  if (a->gt_difficult) return T3D_ERR_ARG;
  if (!(d->bg_threshold >= 0.0 && d->bg_threshold < a->threshold)) return T3D_ERR_ARG;
  if (a->P < 0 || a->G < 0 || a->P > T3D_SUNRGBD_EVAL_MAX_BOXES || a->G > T3D_SUNRGBD_EVAL_MAX_BOXES) return T3D_ERR_SHAPE;
  if (d->Go < 0 || d->n_other_images < 0 || d->Go > T3D_SUNRGBD_EVAL_MAX_BOXES) return T3D_ERR_SHAPE;
  if (a->P > 0 && (!d->other_overlap || !d->other_gt || !d->kind)) return T3D_ERR_ARG;
  if (a->G > 0 && !d->gt_state) return T3D_ERR_ARG;
  if (d->Go > 0 && (!d->other_centroid || !d->other_basis || !d->other_coeffs || !d->other_image || !d->other_image_list)) return T3D_ERR_ARG;
  if (d->n_other_images > 0 && (!d->other_image_ids || !d->other_image_offsets)) return T3D_ERR_ARG;
  if (a->G + d->Go > 0 && (!d->workspace || d->workspace_bytes < T3D_SUNRGBD_DIAGNOSE_WORKSPACE_BYTES(a->P, a->G, d->Go))) return T3D_ERR_ARG;
  const int e = t3d_sunrgbd_eval(a, stream);   // every output of the evaluation, by the evaluation itself; it launches nothing when it refuses
  if (e != T3D_OK) return e;
  const hipStream_t st = static_cast<hipStream_t>(stream);
  const auto blocks = [](int n) { return dim3((n + EV_THREADS - 1) / EV_THREADS); };
  if (a->G + d->Go > 0) {
    T3D_LAUNCH(k_diag_prepare, blocks(a->G > d->Go ? a->G : d->Go), dim3(EV_THREADS), 0, st, *a, *d);
    T3D_CHECK_LAUNCH();
  }
  if (a->P > 0) {
    T3D_LAUNCH(k_diag_match, blocks(a->P), dim3(EV_THREADS), 0, st, *a, *d);
    T3D_CHECK_LAUNCH();
  }
  if (a->G > 0) {
    T3D_LAUNCH(k_diag_states, blocks(a->G), dim3(EV_THREADS), 0, st, *a, *d);
    T3D_CHECK_LAUNCH();
  }
  T3D_LAUNCH(k_diag_curves, dim3(DG_FIXES + 1), dim3(EV_CURVE_THREADS), 0, st, *a, *d);
  T3D_CHECK_LAUNCH();
  return T3D_OK;
}
