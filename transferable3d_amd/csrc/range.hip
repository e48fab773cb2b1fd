// The free space of a scene (t3d.h t3d_scene_range) and how a detection stands in it (t3d_detect_visibility).
//   k_range_fill     every cell of the range map to T3D_RANGE_EMPTY, the counts to 0;
//   k_range_points   T3D_RANGE_BLOCKS workgroups per scene, one thread per point: the projection, an integer atomicMin of the bits of
//                    (float)depth into the point's cell; the three counts through LDS, then integer global atomics;
//   k_detect_visibility   one workgroup per detection: K * 8 lanes project the candidates' corners, K lanes fold the rectangles
//                    into cell ranges, then all lanes walk each candidate's cells -- a ray per cell, three slabs, one category --
//                    and count into LDS by integer atomics; lane 0 takes the measures, the choice and the flags, 31 lanes write the row.
// Integer sums and minima only: no output depends on the order of anything.
#include <float.h>
#include <math.h>

#include "common.h"

// The specification (t3d.h, tests/fake_visibility.py) is elementwise fp64 in a stated order: no fused multiply-adds.
#pragma clang fp contract(off)

namespace {

constexpr int RG_THREADS = 256;
constexpr int RG_BLOCKS = T3D_RANGE_BLOCKS;
constexpr int RG_CALIB = 20;               // Rtilt (9), K (9), image W, image H
constexpr int VS_K = T3D_VIS_MAX_OFFSETS;
enum { VS_UNKNOWN = 1, VS_FRONT = 2, VS_INSIDE = 3, VS_THROUGH = 4, VS_GRAZE = 5 };      // columns of a profile row; 0 = rays

__device__ __forceinline__ bool rg_finite(double v) { return fabs(v) <= DBL_MAX; }

// The grid of a scene: true where it is one that fits `range` (t3d.h T3D_RANGE_BAD_GRID otherwise).
__device__ __forceinline__ bool rg_grid(const int32_t* grid_dims, const int64_t* grid_offsets, int64_t n_cells, int s, int& gw, int& gh,
                                        int64_t& off) {
  gw = grid_dims[(size_t)s * 2];
  gh = grid_dims[(size_t)s * 2 + 1];
  off = grid_offsets[s];
  if (gw < 1 || gh < 1) return false;
  const int64_t cells = (int64_t)gw * (int64_t)gh;
  return cells <= (int64_t)T3D_RANGE_MAX_CELLS && off >= 0 && off <= n_cells - cells;
}

// "Projection" of t3d_detect_consistency: d in upright depth coordinates -> u, v, depth.
__device__ __forceinline__ void rg_project(const double* cal, double d0, double d1, double d2, double& u, double& v, double& depth) {
  double tt[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) tt[i] = (cal[i] * d0 + cal[3 + i] * d1) + cal[6 + i] * d2;      // Rtilt^T d
  const double cam0 = tt[0], cam1 = -tt[2], cam2 = tt[1];
  double w[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) w[i] = (cal[9 + 3 * i] * cam0 + cal[10 + 3 * i] * cam1) + cal[11 + 3 * i] * cam2;
  u = w[0] / w[2];
  v = w[1] / w[2];
  depth = cam2;
}

// (int)floor(x / cell) of 0 <= x < g * cell, taken as g - 1 where the quotient rounds up to g.
__device__ __forceinline__ int rg_cell(double x, double cell, int g) {
  const int c = (int)floor(x / cell);
  return c > g - 1 ? g - 1 : c;
}

__global__ __launch_bounds__(RG_THREADS) void k_range_fill(const t3d_scene_range_args p) {
  const int64_t i = (int64_t)blockIdx.x * RG_THREADS + threadIdx.x;
  if (i < p.n_cells) p.range[i] = T3D_RANGE_EMPTY;
  if (i < (int64_t)p.n_scenes * 4) p.counts[i] = 0;
}

__global__ __launch_bounds__(RG_THREADS) void k_range_points(const t3d_scene_range_args p) {
  __shared__ int tally[3];                   // finite, binned, cells filled
  const int s = blockIdx.y, j = blockIdx.x;
  const int64_t lo = p.scene_offsets[s], end = p.scene_offsets[s + 1];
  const int64_t first = lo > 0 ? lo : 0;     // (as t3d_scene_floor: a negative offset is taken as 0, an end before the start as the start)
  const int64_t n = end > first ? end - first : 0;
  if (threadIdx.x < 3) tally[threadIdx.x] = 0;
  __syncthreads();
  const int ci = p.calib_index[s];
  int gw, gh;
  int64_t off;
  int flags = (ci >= 0 && ci < p.n_calib) ? 0 : T3D_RANGE_NO_CALIB;
  if (!rg_grid(p.grid_dims, p.grid_offsets, p.n_cells, s, gw, gh, off)) flags |= T3D_RANGE_BAD_GRID;
  const double* cal = p.calib + (size_t)(flags & T3D_RANGE_NO_CALIB ? 0 : ci) * RG_CALIB;      // read only where flags == 0
  const double cell = (double)p.cell;
  const double GW = (double)gw * cell, GH = (double)gh * cell;
  int n_fin = 0, n_bin = 0, n_fill = 0;
  for (int64_t i = (int64_t)j * RG_THREADS + threadIdx.x; i < n; i += (int64_t)RG_BLOCKS * RG_THREADS) {
    const double* q = p.points + (size_t)(first + i) * p.ld;
    const double x = q[0], y = q[1], z = q[2];
    if (!(rg_finite(x) && rg_finite(y) && rg_finite(z))) continue;
    ++n_fin;
    if (flags) continue;
    double u, v, depth;
    rg_project(cal, x, y, z, u, v, depth);
    if (!(depth > 0.0)) continue;
    const uint32_t bits = __float_as_uint((float)depth);
    if (!(bits < T3D_RANGE_EMPTY)) continue;
    if (!(rg_finite(u) && rg_finite(v) && u >= 0.0 && u < GW && v >= 0.0 && v < GH)) continue;
    const int cx = rg_cell(u, cell, gw), cy = rg_cell(v, cell, gh);
    ++n_bin;
    // the one thread that finds the cell empty counts it: every later minimum finds a depth there
    if (atomicMin(&p.range[off + (int64_t)cy * gw + cx], bits) == T3D_RANGE_EMPTY) ++n_fill;
  }
  if (n_fin) atomicAdd(&tally[0], n_fin);
  if (n_bin) atomicAdd(&tally[1], n_bin);
  if (n_fill) atomicAdd(&tally[2], n_fill);
  __syncthreads();
  int32_t* c = p.counts + (size_t)s * 4;
  if (threadIdx.x < 3 && tally[threadIdx.x]) atomicAdd(&c[threadIdx.x], tally[threadIdx.x]);
  if (threadIdx.x == 3 && j == 0) c[3] = flags;
}

__global__ __launch_bounds__(RG_THREADS) void k_detect_visibility(const t3d_detect_visibility_args p) {
  __shared__ double proj[VS_K][8][3];        // u, v, depth of the candidates' corners
  __shared__ int rect[VS_K][5];              // cx0, cx1, cy0, cy1 (cx1 < cx0: no cell), measured
  __shared__ int prof[VS_K][6];
  __shared__ int decided[2];                 // choice, moved
  const int i = blockIdx.x, t = threadIdx.x;
  const int K = p.K, mid = (K - 1) / 2;
  const float* lf = p.label + (size_t)i * 7;
  const float* kf = p.corners + (size_t)i * 24;
  bool finite = true;
  for (int k = 0; k < 7; ++k) finite = finite && fabsf(lf[k]) <= FLT_MAX;
  for (int k = 0; k < 24; ++k) finite = finite && fabsf(kf[k]) <= FLT_MAX;
  const int s = p.scene_index[i];
  int gw = 0, gh = 0;
  int64_t off = 0;
  int flags = 0;
  if (s < 0 || s >= p.n_scenes || !rg_grid(p.grid_dims, p.grid_offsets, p.n_cells, s, gw, gh, off)) flags = T3D_VIS_NO_SCENE;
  if (!finite) flags |= T3D_VIS_NOT_FINITE;
  if (t < K * 6) prof[t / 6][t % 6] = 0;
  __syncthreads();
  if (flags == 0) {                          // (the same for every lane of the workgroup)
    const double* cal = p.calib + (size_t)s * RG_CALIB;
    const double tx = (double)lf[3], tz = (double)lf[5];
    const double cell = (double)p.cell;
    if (t < K * 8) {
      const int k = t >> 3, c = t & 7;
      const double X = (double)kf[3 * c] + p.offsets[k] * tx, Y = (double)kf[3 * c + 1], Z = (double)kf[3 * c + 2] + p.offsets[k] * tz;
      rg_project(cal, X, Z, -Y, proj[k][c][0], proj[k][c][1], proj[k][c][2]);      // upright camera -> upright depth
    }
    __syncthreads();
    if (t < K) {
      const double GW = (double)gw * cell, GH = (double)gh * cell;
      bool ok = true;
      double xmin = proj[t][0][0], ymin = proj[t][0][1], xmax = xmin, ymax = ymin;
      for (int c = 0; c < 8; ++c) {
        const double u = proj[t][c][0], v = proj[t][c][1];
        ok = ok && proj[t][c][2] > 0.0 && rg_finite(u) && rg_finite(v);
        xmin = u < xmin ? u : xmin;
        xmax = u > xmax ? u : xmax;
        ymin = v < ymin ? v : ymin;
        ymax = v > ymax ? v : ymax;
      }
      int cx0 = 0, cx1 = -1, cy0 = 0, cy1 = -1;
      if (ok && !(xmax < 0.0 || xmin >= GW || ymax < 0.0 || ymin >= GH)) {
        cx0 = xmin < 0.0 ? 0 : rg_cell(xmin, cell, gw);
        cx1 = xmax >= GW ? gw - 1 : rg_cell(xmax, cell, gw);
        cy0 = ymin < 0.0 ? 0 : rg_cell(ymin, cell, gh);
        cy1 = ymax >= GH ? gh - 1 : rg_cell(ymax, cell, gh);
      }
      rect[t][0] = cx0; rect[t][1] = cx1; rect[t][2] = cy0; rect[t][3] = cy1; rect[t][4] = ok ? 1 : 0;
    }
    __syncthreads();
    const double k02 = cal[11], k00 = cal[9], k12 = cal[14], k11 = cal[13];
    const uint32_t* map = p.range + off;
#pragma unroll 1
    for (int k = 0; k < K; ++k) {
      const int cx0 = rect[k][0], cy0 = rect[k][2];
      const int ncx = rect[k][1] - cx0 + 1, ncy = rect[k][3] - cy0 + 1;
      if (ncx <= 0 || ncy <= 0) continue;
      const int total = ncx * ncy;           // <= gw * gh <= T3D_RANGE_MAX_CELLS
      const double o = p.offsets[k];
      const double k0x = (double)kf[0] + o * tx, k0y = (double)kf[1], k0z = (double)kf[2] + o * tz;
      double e[3][3], b[3], dd[3];
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        const float* kj = kf + 3 * (j == 0 ? 1 : j == 1 ? 3 : 4);      // the edges to corners 1, 3, 4
        e[j][0] = ((double)kj[0] + o * tx) - k0x;
        e[j][1] = (double)kj[1] - k0y;
        e[j][2] = ((double)kj[2] + o * tz) - k0z;
        b[j] = (k0x * e[j][0] + k0y * e[j][1]) + k0z * e[j][2];
        dd[j] = (e[j][0] * e[j][0] + e[j][1] * e[j][1]) + e[j][2] * e[j][2];
      }
      int n_unknown = 0, n_front = 0, n_inside = 0, n_through = 0, n_graze = 0;      // (named: an indexed array would live in scratch)
#pragma unroll 1
      for (int idx = t; idx < total; idx += RG_THREADS) {
        const int cy = cy0 + idx / ncx, cx = cx0 + idx % ncx;
        const double pu = ((double)cx + 0.5) * cell, pv = ((double)cy + 0.5) * cell;
        const double q0 = (pu - k02) / k00, q1 = 1.0, q2 = -((pv - k12) / k11);
        double d[3];
#pragma unroll
        for (int r = 0; r < 3; ++r) d[r] = (cal[3 * r] * q0 + cal[3 * r + 1] * q1) + cal[3 * r + 2] * q2;
        const double g0 = d[0], g1 = -d[2], g2 = d[1];
        double t_in = 0.0, t_out = INFINITY;
        bool hit = true;
#pragma unroll
        for (int j = 0; j < 3; ++j) {
          const double a = (g0 * e[j][0] + g1 * e[j][1]) + g2 * e[j][2];
          if (a == 0.0) {
            const double nb = -b[j];
            hit = hit && 0.0 <= nb && nb <= dd[j];
          } else {
            const double r0 = b[j] / a, r1 = (dd[j] + b[j]) / a;
            const double lo = r0 < r1 ? r0 : r1, hi = r0 < r1 ? r1 : r0;
            t_in = lo > t_in ? lo : t_in;
            t_out = hi < t_out ? hi : t_out;
          }
        }
        if (!(hit && t_in < t_out)) continue;
        int cat;
        if (t_out - t_in < p.min_chord) {
          cat = VS_GRAZE;
        } else {
          const uint32_t bits = map[(int64_t)cy * gw + cx];
          const double z = (double)__uint_as_float(bits);
          cat = bits == T3D_RANGE_EMPTY ? VS_UNKNOWN : z < t_in - p.margin ? VS_FRONT : z > t_out + p.margin ? VS_THROUGH : VS_INSIDE;
        }
        n_unknown += cat == VS_UNKNOWN;
        n_front += cat == VS_FRONT;
        n_inside += cat == VS_INSIDE;
        n_through += cat == VS_THROUGH;
        n_graze += cat == VS_GRAZE;
      }
      if (n_unknown) atomicAdd(&prof[k][VS_UNKNOWN], n_unknown);
      if (n_front) atomicAdd(&prof[k][VS_FRONT], n_front);
      if (n_inside) atomicAdd(&prof[k][VS_INSIDE], n_inside);
      if (n_through) atomicAdd(&prof[k][VS_THROUGH], n_through);
      if (n_graze) atomicAdd(&prof[k][VS_GRAZE], n_graze);
    }
    __syncthreads();
  }
  if (t == 0) {
    int choice = mid, moved = 0;
    double m[3] = {0.0, 0.0, 0.0};
    if (flags == 0) {
      for (int k = 0; k < K; ++k) prof[k][0] = (prof[k][VS_UNKNOWN] + prof[k][VS_FRONT]) + (prof[k][VS_INSIDE] + prof[k][VS_THROUGH]);
      if (!rect[mid][4]) {
        flags = T3D_VIS_BEHIND;
      } else {
        const int rays = prof[mid][0], seen = prof[mid][VS_THROUGH] + prof[mid][VS_INSIDE];
        if (rays == 0) flags |= T3D_VIS_NO_RAYS;
        if (seen == 0) flags |= T3D_VIS_NO_EVIDENCE;
        if (seen > 0) m[0] = (double)prof[mid][VS_THROUGH] / (double)seen;
        if (rays > 0) {
          m[1] = (double)prof[mid][VS_FRONT] / (double)rays;
          m[2] = (double)prof[mid][VS_INSIDE] / (double)rays;
        }
        int best = prof[mid][VS_INSIDE] - prof[mid][VS_THROUGH];
        const int score_mid = best;
        for (int k = 0; k < K; ++k) {          // ascending k: a later candidate wins only where it is strictly better
          if (!rect[k][4]) continue;
          const int sc = prof[k][VS_INSIDE] - prof[k][VS_THROUGH];
          const int dk = k > mid ? k - mid : mid - k, dc = choice > mid ? choice - mid : mid - choice;
          if (sc > best || (sc == best && dk < dc)) {
            best = sc;
            choice = k;
          }
        }
        if (p.mode == 1 && choice != mid && best - score_mid >= p.min_gain) {
          moved = 1;
          flags |= T3D_VIS_SNAPPED;
        }
      }
    }
    decided[0] = choice;
    decided[1] = moved;
    p.choice[i] = choice;
    p.flags[i] = flags;
    for (int c = 0; c < 3; ++c) p.measures[(size_t)i * 3 + c] = m[c];
  }
  __syncthreads();
  if (t < K * 6) p.profile[(size_t)i * K * 6 + t] = prof[t / 6][t % 6];
  const bool moved = decided[1] != 0;
  const double o = p.offsets[decided[0]];
  if (p.label_out && t < 7) {
    float v = lf[t];
    if (moved && (t == 3 || t == 5)) v = (float)((double)v + o * (double)v);
    p.label_out[(size_t)i * 7 + t] = v;
  }
  if (p.corners_out && t >= 32 && t < 56) {
    const int c = t - 32;
    float v = kf[c];
    if (moved && c % 3 == 0) v = (float)((double)v + o * (double)lf[3]);
    if (moved && c % 3 == 2) v = (float)((double)v + o * (double)lf[5]);
    p.corners_out[(size_t)i * 24 + c] = v;
  }
}

inline bool rg_nonneg_finite(double v) { return v >= 0.0 && v <= DBL_MAX; }      // false for a NaN

}  // namespace

extern "C" int t3d_scene_range(const t3d_scene_range_args* a, t3d_stream_t stream) {
  T3D_ABI_TAKE(scene_range_args, a);
  if (!a || !a->points || !a->scene_offsets || !a->calib || !a->calib_index || !a->grid_dims || !a->grid_offsets || !a->counts) return T3D_ERR_ARG;
  if (a->reserved != 0 || a->n_scenes < 0 || a->cell < 1 || a->n_calib < 0 || a->n_cells < 0 || (a->n_cells > 0 && !a->range)) return T3D_ERR_ARG;
  if (a->ld < 3 || a->n_scenes > 65535 || a->n_cells > (int64_t)INT32_MAX) return T3D_ERR_SHAPE;
  if (a->n_scenes == 0) return T3D_OK;
  const hipStream_t st = static_cast<hipStream_t>(stream);
  const int S = a->n_scenes;
  const int64_t items = a->n_cells > (int64_t)S * 4 ? a->n_cells : (int64_t)S * 4;
  T3D_LAUNCH(k_range_fill, dim3((unsigned)((items + RG_THREADS - 1) / RG_THREADS)), dim3(RG_THREADS), 0, st, *a);
  T3D_CHECK_LAUNCH();
  T3D_LAUNCH(k_range_points, dim3(RG_BLOCKS, S), dim3(RG_THREADS), 0, st, *a);
  T3D_CHECK_LAUNCH();
  return T3D_OK;
}

extern "C" int t3d_detect_visibility(const t3d_detect_visibility_args* a, t3d_stream_t stream) {
  T3D_ABI_TAKE(detect_visibility_args, a);
  if (!a || !a->label || !a->corners || !a->scene_index || !a->profile || !a->measures || !a->choice || !a->flags) return T3D_ERR_ARG;
  if (a->reserved != 0 || a->n < 0 || a->n_scenes < 0 || a->n_cells < 0) return T3D_ERR_ARG;
  if (a->n_scenes > 0 && (!a->calib || !a->grid_dims || !a->grid_offsets)) return T3D_ERR_ARG;
  if (a->n_cells > 0 && !a->range) return T3D_ERR_ARG;
  if (a->mode < 0 || a->mode > 1 || (a->mode == 1 && (!a->label_out || !a->corners_out))) return T3D_ERR_ARG;
  if (a->cell < 1 || a->min_gain < 0 || !rg_nonneg_finite(a->margin) || !rg_nonneg_finite(a->min_chord)) return T3D_ERR_ARG;
  if (a->K < 1 || a->K > T3D_VIS_MAX_OFFSETS || a->K % 2 == 0) return T3D_ERR_SHAPE;
  for (int k = 0; k < a->K; ++k) {
    if (!(a->offsets[k] > -1.0 && a->offsets[k] <= DBL_MAX)) return T3D_ERR_ARG;
    if (k > 0 && !(a->offsets[k] > a->offsets[k - 1])) return T3D_ERR_ARG;
  }
  if (a->offsets[(a->K - 1) / 2] != 0.0) return T3D_ERR_ARG;
  if (a->n == 0) return T3D_OK;
  T3D_LAUNCH(k_detect_visibility, dim3(a->n), dim3(RG_THREADS), 0, static_cast<hipStream_t>(stream), *a);
  T3D_CHECK_LAUNCH();
  return T3D_OK;
}
