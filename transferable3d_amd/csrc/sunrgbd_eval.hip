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
#include "common.h"

// MATLAB evaluates the corner and volume expressions operation by operation: no fused multiply-adds
#pragma clang fp contract(off)

namespace {

constexpr int EV_THREADS = 256;
constexpr int EV_CURVE_THREADS = 1024;
constexpr int EV_FP = 11;                     // x1 y1 x2 y2 x3 y3 x4 y4 zMin zMax volume
constexpr int EV_UNCLAIMED = 0x7fffffff;
constexpr double EV_EPS = 2.220446049250313e-16;      // MATLAB's eps

struct EvWork {
  double* fp_det;       // [P, 11]
  double* fp_gt;        // [G, 11]
  int32_t* rank;        // [P] sorted position of detection i
  int32_t* gt_first;    // [G] smallest sorted position among the detections that claim the box
};

__host__ __device__ inline EvWork ev_work(void* ws, int P, int G) {
  EvWork w;
  w.fp_det = static_cast<double*>(ws);
  w.fp_gt = w.fp_det + (size_t)P * EV_FP;
  w.rank = reinterpret_cast<int32_t*>(w.fp_gt + (size_t)G * EV_FP);
  w.gt_first = w.rank + P;
  return w;
}

// get_corners_of_bb3d.m for one box {centroid, basis (rows), coeffs}
__device__ void ev_footprint(const double* ce, const double* basis, const double* coeffs, double* out) {
  // :17-19  rows by |basis(:,1)|, descending, ties in their order
  double B[3][3], c[3];
  {
    const double k0 = fabs(basis[0]), k1 = fabs(basis[3]), k2 = fabs(basis[6]);
    const double k[3] = {k0, k1, k2};
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      int r = 0;
#pragma unroll
      for (int j = 0; j < 3; ++j) r += (k[j] > k[i]) || (j < i && k[j] == k[i]);
#pragma unroll
      for (int t = 0; t < 3; ++t) {           // (a select per slot: no dynamically indexed private array)
        if (r == t) {
          B[t][0] = basis[i * 3]; B[t][1] = basis[i * 3 + 1]; B[t][2] = basis[i * 3 + 2];
          c[t] = coeffs[i];
        }
      }
    }
  }
  // :21-25  rows 2, 3 by |basis(2:3,2)|
  if (fabs(B[2][1]) > fabs(B[1][1])) {
#pragma unroll
    for (int t = 0; t < 3; ++t) { const double s = B[1][t]; B[1][t] = B[2][t]; B[2][t] = s; }
    const double s = c[1]; c[1] = c[2]; c[2] = s;
  }
  // :29, 46-53  flip_towards_viewer: a row whose projection on the unit centroid is positive is negated
  const double n = sqrt(ce[0] * ce[0] + ce[1] * ce[1] + ce[2] * ce[2]);
  const double p0 = ce[0] / n, p1 = ce[1] / n, p2 = ce[2] / n;
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    const double proj = p0 * B[r][0] + p1 * B[r][1] + p2 * B[r][2];
    if (proj > 0) { B[r][0] = -B[r][0]; B[r][1] = -B[r][1]; B[r][2] = -B[r][2]; }
  }
  // :31
  c[0] = fabs(c[0]); c[1] = fabs(c[1]); c[2] = fabs(c[2]);
  // :33-36, 41, 43  corners 1-4 (x, y) and the z of corners 1 and 8
  const double s1[4] = {-1.0, 1.0, 1.0, -1.0}, s2[4] = {1.0, 1.0, -1.0, -1.0};
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    out[2 * k] = (s1[k] * B[0][0]) * c[0] + (s2[k] * B[1][0]) * c[1] + B[2][0] * c[2] + ce[0];
    out[2 * k + 1] = (s1[k] * B[0][1]) * c[0] + (s2[k] * B[1][1]) * c[1] + B[2][1] * c[2] + ce[1];
  }
  const double z1 = (-B[0][2]) * c[0] + B[1][2] * c[1] + B[2][2] * c[2] + ce[2];
  const double z8 = (-B[0][2]) * c[0] + (-B[1][2]) * c[1] + (-B[2][2]) * c[2] + ce[2];
  out[8] = fmin(z1, z8);
  out[9] = fmax(z1, z8);
  // cuboidVolume.m:3-5
  const double d1 = (out[0] - out[2]) * (out[0] - out[2]), d2 = (out[1] - out[3]) * (out[1] - out[3]);
  const double d3 = (out[4] - out[2]) * (out[4] - out[2]), d4 = (out[5] - out[3]) * (out[5] - out[3]);
  out[10] = (out[9] - out[8]) * sqrt((d1 + d2) * (d3 + d4));
}

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

struct EvQuad { double x[4], y[4]; };

__device__ __forceinline__ double ev_area2(const EvQuad& q) {
  double a = 0.0;
#pragma unroll
  for (int i = 0; i < 4; ++i) { const int j = (i + 1) & 3; a += q.x[i] * q.y[j] - q.y[i] * q.x[j]; }
  return a;
}

__device__ __forceinline__ void ev_make_ccw(EvQuad& q) {
  if (ev_area2(q) < 0.0) {
    double t = q.x[1]; q.x[1] = q.x[3]; q.x[3] = t;
    t = q.y[1]; q.y[1] = q.y[3]; q.y[3] = t;
  }
}

// The boundary integral of boxgeom_dev.h in fp64: 1/2 sum of cross(a', b') over the parts [a', b'] of P's edges inside Q (Cyrus-Beck
// against Q's four half-planes).  CLOSED: points on Q's boundary count as inside; edges of P are kept where they run along Q's boundary
// in the same direction, edges of Q are not, so that coincident edges are counted once.  A point within 1e-12 edge lengths of an edge
// line is on it.
template <bool CLOSED>
__device__ __forceinline__ double ev_boundary_inside(const EvQuad& P, const EvQuad& Q) {
  double acc = 0.0;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int j = (i + 1) & 3;
    const double ax = P.x[i], ay = P.y[i], bx = P.x[j], by = P.y[j];
    double t0 = 0.0, t1 = 1.0;
    bool alive = true;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int f = (e + 1) & 3;
      const double ex = Q.x[f] - Q.x[e], ey = Q.y[f] - Q.y[e];
      const double da = ex * (ay - Q.y[e]) - ey * (ax - Q.x[e]);
      const double db = ex * (by - Q.y[e]) - ey * (bx - Q.x[e]);
      const double tol = 1e-12 * (ex * ex + ey * ey) + 1e-300;
      const bool ina = CLOSED ? da >= -tol : da > tol, inb = CLOSED ? db >= -tol : db > tol;
      const double t = fmin(fmax(da / (da - db), 0.0), 1.0);   // used only when the two ends lie on different sides
      if (CLOSED) {
        const bool on_line = fabs(da) <= tol && fabs(db) <= tol;
        alive = alive && !(on_line && (bx - ax) * ex + (by - ay) * ey <= 0.0);
      }
      alive = alive && (ina || inb);
      t0 = (!ina && inb) ? fmax(t0, t) : t0;
      t1 = (ina && !inb) ? fmin(t1, t) : t1;
    }
    alive = alive && t1 > t0;
    const double px = ax + t0 * (bx - ax), py = ay + t0 * (by - ay);
    const double qx = ax + t1 * (bx - ax), qy = ay + t1 * (by - ay);
    acc += alive ? 0.5 * (px * qy - py * qx) : 0.0;
  }
  return acc;
}

// bb3dOverlapCloseForm.m:41-58 for one pair of 10-vectors (+ volume): cuboidIntersectionVolume.c:62-88, then inter / union.
// A box of volume 0 overlaps nothing (MATLAB: 0 / union; 0 / 0 only for two such boxes, which is defined as 0 here).
__device__ double ev_overlap(const double* a, const double* b) {
  const double z = fmin(a[9], b[9]) - fmax(a[8], b[8]);
  if (!(z > 0.0) || !(a[10] > 0.0) || !(b[10] > 0.0)) return 0.0;
  EvQuad P, Q;
#pragma unroll
  for (int k = 0; k < 4; ++k) { P.x[k] = a[2 * k]; P.y[k] = a[2 * k + 1]; Q.x[k] = b[2 * k]; Q.y[k] = b[2 * k + 1]; }
  ev_make_ccw(P);
  ev_make_ccw(Q);
  const double ox = P.x[0], oy = P.y[0];      // cross products of small numbers: the boxes sit metres from the origin
#pragma unroll
  for (int k = 0; k < 4; ++k) { P.x[k] -= ox; P.y[k] -= oy; Q.x[k] -= ox; Q.y[k] -= oy; }
  const double area = ev_boundary_inside<true>(P, Q) + ev_boundary_inside<false>(Q, P);
  const double inter = z * area;
  if (!(inter > 0.0)) return 0.0;
  return inter / (a[10] + b[10] - inter);
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

// Exclusive prefix sum of one int per thread over the workgroup's 16 waves; `total`: the sum.  wsum: 16 ints of LDS.
__device__ __forceinline__ int ev_block_scan(int v, int* wsum, int& total) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  int x = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int y = __shfl_up(x, o, 64);
    if (lane >= o) x += y;
  }
  __syncthreads();
  if (lane == 63) wsum[wv] = x;
  __syncthreads();
  int off = 0, tot = 0;
  for (int k = 0; k < EV_CURVE_THREADS / 64; ++k) {
    off += k < wv ? wsum[k] : 0;
    tot += wsum[k];
  }
  total = tot;
  return off + x - v;
}

__global__ __launch_bounds__(EV_CURVE_THREADS) void k_eval_curve(const t3d_sunrgbd_eval_args p) {
  __shared__ int wsum[EV_CURVE_THREADS / 64];
  __shared__ double part[EV_CURVE_THREADS / 64];
  const int t = threadIdx.x, P = p.P;
  // sum(~isDifficult)
  int c = 0;
  for (int g = t; g < p.G; g += EV_CURVE_THREADS) c += (p.gt_difficult == nullptr || p.gt_difficult[g] == 0) ? 1 : 0;
  int n_pos;
  ev_block_scan(c, wsum, n_pos);
  const int chunk = (P + EV_CURVE_THREADS - 1) / EV_CURVE_THREADS;
  const int k0 = min(t * chunk, P), k1 = min(k0 + chunk, P);
  // cumsum(tp), cumsum(fp) in integers
  int ntp = 0, nfp = 0;
  for (int k = k0; k < k1; ++k) {
    const int i = p.order[k];
    ntp += p.is_tp[i];
    nfp += p.is_fp[i];
  }
  int tot;
  int ctp = ev_block_scan(ntp, wsum, tot);
  int cfp = ev_block_scan(nfp, wsum, tot);
  double pmax = 0.0;
  for (int k = k0; k < k1; ++k) {
    const int i = p.order[k];
    ctp += p.is_tp[i];
    cfp += p.is_fp[i];
    const double rec = p.G > 0 ? (double)ctp / (double)n_pos : 0.0;
    const double pre = (double)ctp / ((double)cfp + (double)ctp);           // 0 / 0 = NaN, as in MATLAB (a leading "difficult" match)
    p.recall[k] = rec;
    p.precision[k] = pre;
    pmax = fmax(pmax, pre);                                                 // max(a, b) of MATLAB ignores a NaN, as fmax does
  }
  // mpre(ii) = max(mpre(ii), mpre(ii+1)) from the right, the sentinel 0 behind the last entry
  // (a suffix scan in the pattern of ev_block_scan: within the wave by shuffles, across the 16 waves through LDS; a maximum is exact,
  // so the order of the scan does not matter)
  const int lane = t & 63, wv = t >> 6;
  double sfx = pmax;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const double y = __shfl_down(sfx, o, 64);
    if (lane + o < 64) sfx = fmax(sfx, y);
  }
  const double right = __shfl_down(sfx, 1, 64);                             // the threads to the right of this one in its wave
  if (lane == 0) part[wv] = sfx;
  __syncthreads();
  double run = lane < 63 ? right : 0.0;
  for (int k = wv + 1; k < EV_CURVE_THREADS / 64; ++k) run = fmax(run, part[k]);
  __syncthreads();
  // sum((mrec(ii) - mrec(ii-1)) .* mpre(ii)) over the ii where the recall changes; mrec = [0; recall; 1]
  double acc = 0.0;
  for (int k = k1 - 1; k >= k0; --k) {
    run = fmax(run, p.precision[k]);
    const double r1 = p.recall[k], r0 = k > 0 ? p.recall[k - 1] : 0.0;
    if (r1 != r0) acc += (r1 - r0) * run;
  }
  // a fixed tree: the lanes of a wave pairwise at distances 32 .. 1, then the 16 waves in index order -- the same bits every run
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_down(acc, o, 64);
  if (lane == 0) part[wv] = acc;
  __syncthreads();
  if (t == 0) {
    double ap = 0.0;
    for (int k = 0; k < EV_CURVE_THREADS / 64; ++k) ap += part[k];
    const double last = P > 0 ? p.recall[P - 1] : 0.0;
    if (1.0 != last) ap += (1.0 - last) * 0.0;                              // the closing sentinel pair (1, 0)
    p.ap[0] = ap;
  }
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
