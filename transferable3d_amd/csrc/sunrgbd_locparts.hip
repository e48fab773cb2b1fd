// Localisation errors split into centre, size and heading (t3d.h t3d_sunrgbd_locparts): the diagnosis of sunrgbd_diagnose.hip, then
// three launches on the same stream that read what the evaluation and the diagnosis left on the device -- the ground-truth footprints
// and the ranks in the evaluation's workspace, gt_idx and order among its outputs, kind and gt_state among the diagnosis' -- with no
// host synchronisation between any of them:
//   k_parts_init    one thread per (part, own-class box): no repaired detection yet;
//   k_parts_match   one thread per (detection, part): the counterfactual box of that part (one parameter group of the detection
//                   replaced by its arg-max box's), its footprint (ev_footprint) and its overlap (ev_overlap) with the box's footprint;
//                   a LOC detection the part repairs enters its rank at its box by atomicMin; the part-0 lane writes the six errors;
//   k_parts_curves  six workgroups: five run ev_curve, the evaluation's curve, on the five repaired variants; the sixth counts the
//                   repaired detections and the boxes that gain a true positive by workgroup scans.
// Everything is fp64.  The only atomics are integer minima, so every output is a function of the inputs alone.
#include "sunrgbd_eval_dev.h"

namespace {

constexpr int LP_PARTS = 5, LP_ERRORS = 6;

// [5, G] smallest sorted position among the LOC detections that part f repairs and whose best box this is
__host__ __device__ inline int32_t* lp_first(void* ws) { return static_cast<int32_t*>(ws); }

__global__ __launch_bounds__(EV_THREADS) void k_parts_init(const t3d_sunrgbd_eval_args p, const t3d_sunrgbd_locparts_args q) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < LP_PARTS * p.G) lp_first(q.workspace)[i] = EV_UNCLAIMED;
}

// one of three values by an index in 0..2 (selects: no dynamically indexed private array)
__device__ __forceinline__ double lp_pick(int k, double v0, double v1, double v2) { return k == 0 ? v0 : (k == 1 ? v1 : v2); }

// the vertical row of a basis: the largest |z component|, the first on ties
__device__ __forceinline__ int lp_vertical(const double* basis) {
  const double z0 = fabs(basis[2]), z1 = fabs(basis[5]), z2 = fabs(basis[8]);
  int v = 0;
  double best = z0;
  if (z1 > best) { best = z1; v = 1; }
  if (z2 > best) v = 2;
  return v;
}

__global__ __launch_bounds__(EV_THREADS) void k_parts_match(const t3d_sunrgbd_eval_args p, const t3d_sunrgbd_diagnose_args d,
                                                             const t3d_sunrgbd_locparts_args q) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  const int i = idx / LP_PARTS, f = idx - i * LP_PARTS;
  if (i >= p.P) return;
  const int g = p.gt_idx[i] - 1;
  if (g < 0 || g >= p.G) {                    // on no box: nothing to compare with
    q.part_overlap[(size_t)i * LP_PARTS + f] = 0.0;
    if (f == 0) {
      const double nan = __longlong_as_double(0x7ff8000000000000LL);
#pragma unroll
      for (int k = 0; k < LP_ERRORS; ++k) q.loc_error[(size_t)i * LP_ERRORS + k] = nan;
    }
    return;
  }
  double Ac[3], Ab[9], Ak[3], Bc[3], Bb[9], Bk[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    Ac[k] = p.det_centroid[(size_t)i * 3 + k]; Ak[k] = p.det_coeffs[(size_t)i * 3 + k];
    Bc[k] = p.gt_centroid[(size_t)g * 3 + k]; Bk[k] = p.gt_coeffs[(size_t)g * 3 + k];
  }
#pragma unroll
  for (int k = 0; k < 9; ++k) { Ab[k] = p.det_basis[(size_t)i * 9 + k]; Bb[k] = p.gt_basis[(size_t)g * 9 + k]; }
  // the rows: vertical, and the two horizontal ones in row order
  const int va = lp_vertical(Ab), vb = lp_vertical(Bb);
  const int a0 = va == 0 ? 1 : 0, a1 = va == 2 ? 1 : 2, b0 = vb == 0 ? 1 : 0, b1 = vb == 2 ? 1 : 2;
  const double a0x = lp_pick(a0, Ab[0], Ab[3], Ab[6]), a0y = lp_pick(a0, Ab[1], Ab[4], Ab[7]);
  const double b0x = lp_pick(b0, Bb[0], Bb[3], Bb[6]), b0y = lp_pick(b0, Bb[1], Bb[4], Bb[7]);
  const double b1x = lp_pick(b1, Bb[0], Bb[3], Bb[6]), b1y = lp_pick(b1, Bb[1], Bb[4], Bb[7]);
  const double pp = fabs(a0x * b0x + a0y * b0y), qq = fabs(a0x * b1x + a0y * b1y);
  const bool straight = pp >= qq;             // a0 <-> b0, a1 <-> b1; otherwise a0 <-> b1, a1 <-> b0
  const double sA0 = fabs(lp_pick(a0, Ak[0], Ak[1], Ak[2])), sA1 = fabs(lp_pick(a1, Ak[0], Ak[1], Ak[2])), sAv = fabs(lp_pick(va, Ak[0], Ak[1], Ak[2]));
  const double sB0 = fabs(lp_pick(b0, Bk[0], Bk[1], Bk[2])), sB1 = fabs(lp_pick(b1, Bk[0], Bk[1], Bk[2])), sBv = fabs(lp_pick(vb, Bk[0], Bk[1], Bk[2]));
  const double sAofB0 = straight ? sA0 : sA1, sAofB1 = straight ? sA1 : sA0;      // the partner rows' sizes
  const double sBofA0 = straight ? sB0 : sB1, sBofA1 = straight ? sB1 : sB0;
  if (f == 0) {
    double* e = q.loc_error + (size_t)i * LP_ERRORS;
    e[0] = hypot(Ac[0] - Bc[0], Ac[1] - Bc[1]);
    e[1] = Ac[2] - Bc[2];
    e[2] = log(sAofB0 / sB0);
    e[3] = log(sAofB1 / sB1);
    e[4] = log(sAv / sBv);
    e[5] = atan2(fmin(pp, qq), fmax(pp, qq));
  }
  // the counterfactual box, its rows in the order of the box they come from
  const bool xy = f == T3D_LOCPART_XY || f == T3D_LOCPART_CENTRE, z = f == T3D_LOCPART_Z || f == T3D_LOCPART_CENTRE;
  const bool size = f == T3D_LOCPART_SIZE, heading = f == T3D_LOCPART_HEADING;
  double Cc[3], Cb[9], Ck[3];
  Cc[0] = xy ? Bc[0] : Ac[0];
  Cc[1] = xy ? Bc[1] : Ac[1];
  Cc[2] = z ? Bc[2] : Ac[2];
#pragma unroll
  for (int k = 0; k < 9; ++k) Cb[k] = heading ? Bb[k] : Ab[k];
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    const double of_b = r == va ? sBv : (r == a0 ? sBofA0 : sBofA1);      // row r of A with its partner's size
    const double of_a = r == vb ? sAv : (r == b0 ? sAofB0 : sAofB1);      // row r of B with its partner's size
    Ck[r] = size ? of_b : (heading ? of_a : Ak[r]);
  }
  double fa[EV_FP], fb[EV_FP];
  ev_footprint(Cc, Cb, Ck, fa);
  const EvWork ew = ev_work(p.workspace, p.P, p.G);
#pragma unroll
  for (int k = 0; k < EV_FP; ++k) fb[k] = ew.fp_gt[(size_t)g * EV_FP + k];
  const double ov = ev_overlap(fa, fb);
  q.part_overlap[(size_t)i * LP_PARTS + f] = ov;
  if (d.kind[i] == T3D_DIAG_LOC && ov >= p.threshold) atomicMin(&lp_first(q.workspace)[(size_t)f * p.G + g], ew.rank[i]);   // integer minimum: order-independent
}

__global__ __launch_bounds__(EV_CURVE_THREADS) void k_parts_curves(const t3d_sunrgbd_eval_args p, const t3d_sunrgbd_diagnose_args d,
                                                                    const t3d_sunrgbd_locparts_args q) {
  __shared__ int wsum[EV_CURVE_THREADS / 64];
  __shared__ double part[EV_CURVE_THREADS / 64];
  const int t = threadIdx.x, f = blockIdx.x;
  const int32_t* first = lp_first(q.workspace);
  const double t_f = p.threshold;
  if (f == LP_PARTS) {                        // the counts
    for (int k = 0; k < LP_PARTS; ++k) {
      int c = 0, n;
      for (int i = t; i < p.P; i += EV_CURVE_THREADS) c += (d.kind[i] == T3D_DIAG_LOC && q.part_overlap[(size_t)i * LP_PARTS + k] >= t_f) ? 1 : 0;
      ev_block_scan(c, wsum, n);
      if (t == 0) q.part_counts[k] = n;
      c = 0;
      for (int g = t; g < p.G; g += EV_CURVE_THREADS) c += (d.gt_state[g] == 2 && first[(size_t)k * p.G + g] != EV_UNCLAIMED) ? 1 : 0;
      ev_block_scan(c, wsum, n);
      if (t == 0) q.part_boxes[k] = n;
    }
    return;
  }
  const EvWork ew = ev_work(p.workspace, p.P, p.G);
  const auto repaired = [&](int i) { return d.kind[i] == T3D_DIAG_LOC && q.part_overlap[(size_t)i * LP_PARTS + f] >= t_f; };
  // a repaired detection that becomes a true positive: the best-ranked one of a box in state 2
  const auto promoted = [&](int i) {
    const int g = p.gt_idx[i] - 1;
    return g >= 0 && g < p.G && d.gt_state[g] == 2 && first[(size_t)f * p.G + g] == ew.rank[i];
  };
  const auto tp_of = [&](int i) {
    if (d.kind[i] == T3D_DIAG_TP) return 1;
    return repaired(i) && promoted(i) ? 1 : 0;
  };
  const auto fp_of = [&](int i) { return (d.kind[i] == T3D_DIAG_TP || repaired(i)) ? 0 : 1; };
  ev_curve(p.P, p.G > 0, p.G, p.order, tp_of, fp_of, (double*)nullptr, (double*)nullptr, q.ap_part + f, wsum, part);
}

}  // namespace

extern "C" int t3d_sunrgbd_locparts(const t3d_sunrgbd_eval_args* a, const t3d_sunrgbd_diagnose_args* d, const t3d_sunrgbd_locparts_args* q,
                                    t3d_stream_t stream) {
  T3D_ABI_TAKE(sunrgbd_eval_args, a);
  T3D_ABI_TAKE(sunrgbd_diagnose_args, d);
  T3D_ABI_TAKE(sunrgbd_locparts_args, q);
  if (!a || !d || !q || q->reserved != 0 || !q->part_counts || !q->part_boxes || !q->ap_part) return T3D_ERR_ARG;
  if (a->P > 0 && (!q->part_overlap || !q->loc_error)) return T3D_ERR_ARG;
  if (a->G > 0 && (!q->workspace || q->workspace_bytes < T3D_SUNRGBD_LOCPARTS_WORKSPACE_BYTES(a->P, a->G))) return T3D_ERR_ARG;
  const int e = t3d_sunrgbd_diagnose(a, d, stream);      // every output of both structs, by the diagnosis itself; it launches nothing when it refuses
  if (e != T3D_OK) return e;
  const hipStream_t st = static_cast<hipStream_t>(stream);
  const auto blocks = [](int n) { return dim3((n + EV_THREADS - 1) / EV_THREADS); };
  if (a->G > 0) {
    T3D_LAUNCH(k_parts_init, blocks(LP_PARTS * a->G), dim3(EV_THREADS), 0, st, *a, *q);
    T3D_CHECK_LAUNCH();
  }
  if (a->P > 0) {
    T3D_LAUNCH(k_parts_match, blocks(LP_PARTS * a->P), dim3(EV_THREADS), 0, st, *a, *d, *q);
    T3D_CHECK_LAUNCH();
  }
  T3D_LAUNCH(k_parts_curves, dim3(LP_PARTS + 1), dim3(EV_CURVE_THREADS), 0, st, *a, *d, *q);
  T3D_CHECK_LAUNCH();
  return T3D_OK;
}
