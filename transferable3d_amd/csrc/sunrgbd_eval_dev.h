// Device code of the official SUN-RGBD evaluation that t3d_sunrgbd_eval (sunrgbd_eval.hip) and t3d_sunrgbd_diagnose
// (sunrgbd_diagnose.hip) share: the workspace layout, the footprint of a box, the overlap of two footprints, the workgroup scan and the
// precision / recall / AP curve.  The diagnosis measures its detections with the very code the evaluation scores them with.
#pragma once
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

// computePRCurve3D.m:78-81 and get_average_precision.m:15-23 by one workgroup of EV_CURVE_THREADS threads: integer scans of tp and fp
// over the sorted order, recall and precision from the integer counts, the right-to-left running maximum and the area, summed in a
// fixed order.  tp_of(i) / fp_of(i): 0 or 1 for the detection of file index i (one that counts in neither sum gives 0 and 0);
// n_pos: the number of boxes to find; have_gt false: recall 0 throughout.  recall / precision: [P] in sorted order, or NULL (not
// stored).  The area pass takes every value from the integer counts again, by the expressions that stored it: the same bits.
// Thread 0 writes ap[0].  wsum: 16 ints, part: 16 doubles of LDS.
template <class Tp, class Fp>
__device__ __forceinline__ void ev_curve(int P, bool have_gt, int n_pos, const int32_t* order, Tp tp_of, Fp fp_of, double* recall,
                                         double* precision, double* ap, int* wsum, double* part) {
  const int t = threadIdx.x;
  const auto rec_of = [&](int ctp) { return have_gt ? (double)ctp / (double)n_pos : 0.0; };
  // 0 / 0 = NaN, as in MATLAB (a leading "difficult" match)
  const auto pre_of = [](int ctp, int cfp) { return (double)ctp / ((double)cfp + (double)ctp); };
  const int chunk = (P + EV_CURVE_THREADS - 1) / EV_CURVE_THREADS;
  const int k0 = min(t * chunk, P), k1 = min(k0 + chunk, P);
  // cumsum(tp), cumsum(fp) in integers
  int ntp = 0, nfp = 0;
  for (int k = k0; k < k1; ++k) {
    const int i = order[k];
    ntp += tp_of(i);
    nfp += fp_of(i);
  }
  int n_tp, n_fp;
  int ctp = ev_block_scan(ntp, wsum, n_tp);
  int cfp = ev_block_scan(nfp, wsum, n_fp);
  double pmax = 0.0;
  for (int k = k0; k < k1; ++k) {
    const int i = order[k];
    ctp += tp_of(i);
    cfp += fp_of(i);
    const double pre = pre_of(ctp, cfp);
    if (recall) recall[k] = rec_of(ctp);
    if (precision) precision[k] = pre;
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
    const int i = order[k];
    run = fmax(run, pre_of(ctp, cfp));
    const double r1 = rec_of(ctp);
    ctp -= tp_of(i);
    cfp -= fp_of(i);
    const double r0 = k > 0 ? rec_of(ctp) : 0.0;
    if (r1 != r0) acc += (r1 - r0) * run;
  }
  // a fixed tree: the lanes of a wave pairwise at distances 32 .. 1, then the 16 waves in index order -- the same bits every run
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_down(acc, o, 64);
  if (lane == 0) part[wv] = acc;
  __syncthreads();
  if (t == 0) {
    double sum = 0.0;
    for (int k = 0; k < EV_CURVE_THREADS / 64; ++k) sum += part[k];
    const double last = P > 0 ? rec_of(n_tp) : 0.0;
    if (1.0 != last) sum += (1.0 - last) * 0.0;                             // the closing sentinel pair (1, 0)
    ap[0] = sum;
  }
}

}  // namespace
