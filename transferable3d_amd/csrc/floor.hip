// The floor of a scene (t3d.h t3d_scene_floor) and how a detection stands on it (t3d_detect_floor).
// t3d_scene_floor streams the scenes' points three times, T3D_SCENE_FLOOR_BLOCKS workgroups per scene, each walking the chunks
// j, j + BLOCKS, ... of its scene:
//   k_floor_hist     the height histogram in LDS (integer atomics), added to hist by integer global atomics; n_finite alike;
//   k_floor_peak     one workgroup per scene: the floor bin, the cleared plane row, counts;
//   k_floor_sums<false>   the level pass: n1, Sx, Sy, Sz of the inliers -> the workgroup's row of the workspace;
//   k_floor_sums<true>    the moment pass: the means from those rows, then Sxx .. Szz -> the same row;
//   k_floor_fit      one thread per scene: the rows summed in ascending order, the plane.
// The order of every fp64 sum is the header's: lane, halving tree, chunk, workgroup.  No floating-point atomic.
#include <float.h>

#include "common.h"

// The specification (t3d.h, tests/fake_floor.py) is elementwise fp64 in a stated order: no fused multiply-adds.
#pragma clang fp contract(off)

namespace {

constexpr int FL_THREADS = 256;
constexpr int FL_BLOCKS = T3D_SCENE_FLOOR_BLOCKS;
constexpr int FL_CHUNK = T3D_SCENE_FLOOR_CHUNK;
constexpr int FL_PASSES = FL_CHUNK / FL_THREADS;
constexpr int FL_ROW = 10;                 // doubles per workgroup in the workspace: n1 (as int64), Sx, Sy, Sz, Sxx, Sxy, Syy, Sxz, Syz, Szz
static_assert(FL_CHUNK % FL_THREADS == 0, "a workgroup covers whole passes");
static_assert(T3D_SCENE_FLOOR_WORKSPACE_BYTES(1) == FL_BLOCKS * FL_ROW * 8, "the workspace holds one row per workgroup");

__device__ __forceinline__ bool fl_finite(double v) { return fabs(v) <= DBL_MAX; }

__device__ __forceinline__ void fl_scene(const t3d_scene_floor_args& p, int s, int64_t& first, int64_t& n) {
  const int64_t lo = p.scene_offsets[s], end = p.scene_offsets[s + 1];
  first = lo > 0 ? lo : 0;                       // (as the specification: a negative offset is taken as 0, an end before the start as the start)
  n = end > first ? end - first : 0;
}

__device__ __forceinline__ double* fl_row(const t3d_scene_floor_args& p, int s, int j) {
  return static_cast<double*>(p.workspace) + ((size_t)s * FL_BLOCKS + j) * FL_ROW;
}

__device__ __forceinline__ double fl_z0(const t3d_scene_floor_args& p, int b) { return p.z_lo + ((double)b + 0.5) * p.bin; }

// The halving tree over the 256 lanes: v[t] = v[t] + v[t+s], s = 128 ... 1; every lane returns with v[0].
template <int K>
__device__ __forceinline__ void fl_tree(double (&v)[K], double (*red)[FL_THREADS]) {
  const int t = threadIdx.x;
#pragma unroll
  for (int k = 0; k < K; ++k) red[k][t] = v[k];
  __syncthreads();
  for (int s = FL_THREADS / 2; s >= 1; s >>= 1) {
    if (t < s) {
#pragma unroll
      for (int k = 0; k < K; ++k) red[k][t] = red[k][t] + red[k][t + s];
    }
    __syncthreads();
  }
#pragma unroll
  for (int k = 0; k < K; ++k) v[k] = red[k][0];
  __syncthreads();
}

__global__ __launch_bounds__(FL_THREADS) void k_floor_hist(const t3d_scene_floor_args p) {
  __shared__ int hist[T3D_SCENE_FLOOR_MAX_BINS];
  __shared__ int n_fin;
  const int s = blockIdx.y, j = blockIdx.x;
  int64_t first, n;
  fl_scene(p, s, first, n);
  for (int b = threadIdx.x; b < p.n_bins; b += FL_THREADS) hist[b] = 0;
  if (threadIdx.x == 0) n_fin = 0;
  __syncthreads();
  const double nb = (double)p.n_bins;
  int mine = 0;
  for (int64_t c0 = (int64_t)j * FL_CHUNK; c0 < n; c0 += (int64_t)FL_BLOCKS * FL_CHUNK) {
#pragma unroll 4
    for (int r = 0; r < FL_PASSES; ++r) {
      const int64_t i = c0 + r * FL_THREADS + threadIdx.x;
      if (i >= n) continue;
      const double* q = p.points + (size_t)(first + i) * p.ld;
      const double x = q[0], y = q[1], z = q[2];
      if (!(fl_finite(x) && fl_finite(y) && fl_finite(z))) continue;
      ++mine;
      const double t = (z - p.z_lo) * p.inv_bin;
      if (t >= 0.0 && t < nb) atomicAdd(&hist[(int)floor(t)], 1);
    }
  }
  if (mine) atomicAdd(&n_fin, mine);
  __syncthreads();
  for (int b = threadIdx.x; b < p.n_bins; b += FL_THREADS)
    if (hist[b]) atomicAdd(&p.hist[(size_t)s * p.n_bins + b], hist[b]);
  if (threadIdx.x == 0 && n_fin) atomicAdd(&p.counts[(size_t)s * 4], n_fin);
}

__global__ __launch_bounds__(FL_THREADS) void k_floor_peak(const t3d_scene_floor_args p) {
  __shared__ int hist[T3D_SCENE_FLOOR_MAX_BINS + 2];      // hist[b + 1]; a zero at either end
  __shared__ int best;
  const int s = blockIdx.x, nb = p.n_bins;
  for (int b = threadIdx.x; b < nb + 2; b += FL_THREADS) hist[b] = (b >= 1 && b <= nb) ? p.hist[(size_t)s * nb + b - 1] : 0;
  if (threadIdx.x == 0) best = nb;
  __syncthreads();
  const int n_finite = p.counts[(size_t)s * 4];
  const double need = p.min_share * (double)n_finite;
  auto c3 = [&](int b) { return (b < 0 || b >= nb) ? 0 : hist[b] + hist[b + 1] + hist[b + 2]; };
  for (int b = threadIdx.x; b < nb; b += FL_THREADS) {
    const int c = c3(b);
    if ((double)c >= need && c >= p.min_inliers && c > c3(b - 2) && c > c3(b - 1) && c >= c3(b + 1) && c >= c3(b + 2)) atomicMin(&best, b);
  }
  __syncthreads();
  if (threadIdx.x < 8) p.plane[(size_t)s * 8 + threadIdx.x] = (threadIdx.x == 7 && best < nb) ? fl_z0(p, best) : 0.0;
  if (threadIdx.x == 0) {
    int32_t* c = p.counts + (size_t)s * 4;
    c[1] = 0;
    c[2] = best < nb ? best : -1;
    c[3] = best < nb ? 0 : T3D_FLOOR_NONE;
  }
}

// MOMENT false: the level pass (n1, Sx, Sy, Sz); true: the moment pass about the means of the level pass.
template <bool MOMENT>
__global__ __launch_bounds__(FL_THREADS) void k_floor_sums(const t3d_scene_floor_args p) {
  constexpr int K = MOMENT ? 6 : 3;
  __shared__ double red[K][FL_THREADS];
  __shared__ double mean[3];
  __shared__ int n_in;
  const int s = blockIdx.y, j = blockIdx.x;
  const int b = p.counts[(size_t)s * 4 + 2];
  if (b < 0) return;
  int64_t first, n;
  fl_scene(p, s, first, n);
  if (threadIdx.x == 0) n_in = 0;
  if (MOMENT && threadIdx.x < 3) {          // the means: the level rows in ascending order
    int64_t n1 = 0;
    double sum = 0.0;
    for (int k = 0; k < FL_BLOCKS; ++k) {
      const double* row = fl_row(p, s, k);
      n1 += reinterpret_cast<const int64_t*>(row)[0];
      sum = sum + row[1 + threadIdx.x];
    }
    mean[threadIdx.x] = sum / (double)n1;
  }
  __syncthreads();
  const double z0 = fl_z0(p, b);
  const double mx = MOMENT ? mean[0] : 0.0, my = MOMENT ? mean[1] : 0.0, mz = MOMENT ? mean[2] : 0.0;
  double total[K];
#pragma unroll
  for (int k = 0; k < K; ++k) total[k] = 0.0;
  int mine = 0;
  for (int64_t c0 = (int64_t)j * FL_CHUNK; c0 < n; c0 += (int64_t)FL_BLOCKS * FL_CHUNK) {
    double v[K];
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = 0.0;
#pragma unroll 4
    for (int r = 0; r < FL_PASSES; ++r) {
      const int64_t i = c0 + r * FL_THREADS + threadIdx.x;
      if (i >= n) continue;
      const double* q = p.points + (size_t)(first + i) * p.ld;
      const double x = q[0], y = q[1], z = q[2];
      if (!(fl_finite(x) && fl_finite(y) && fl_finite(z)) || !(fabs(z - z0) <= p.band)) continue;
      ++mine;
      if constexpr (MOMENT) {
        const double dx = x - mx, dy = y - my, dz = z - mz;
        v[0] = v[0] + dx * dx; v[1] = v[1] + dx * dy; v[2] = v[2] + dy * dy;
        v[3] = v[3] + dx * dz; v[4] = v[4] + dy * dz; v[5] = v[5] + dz * dz;
      } else {
        v[0] = v[0] + x; v[1] = v[1] + y; v[2] = v[2] + z;
      }
    }
    fl_tree<K>(v, red);
#pragma unroll
    for (int k = 0; k < K; ++k) total[k] = total[k] + v[k];
  }
  if (!MOMENT && mine) atomicAdd(&n_in, mine);
  __syncthreads();
  if (threadIdx.x == 0) {
    double* row = fl_row(p, s, j);
    if (!MOMENT) reinterpret_cast<int64_t*>(row)[0] = n_in;
#pragma unroll
    for (int k = 0; k < K; ++k) row[(MOMENT ? 4 : 1) + k] = total[k];
  }
}

__global__ __launch_bounds__(64) void k_floor_fit(const t3d_scene_floor_args p) {
  const int s = blockIdx.x * 64 + threadIdx.x;
  if (s >= p.n_scenes) return;
  int32_t* counts = p.counts + (size_t)s * 4;
  double* plane = p.plane + (size_t)s * 8;
  if (counts[2] < 0) return;
  int64_t n1 = 0;
  double S[9];
  for (int k = 0; k < 9; ++k) S[k] = 0.0;
  for (int j = 0; j < FL_BLOCKS; ++j) {
    const double* row = fl_row(p, s, j);
    n1 += reinterpret_cast<const int64_t*>(row)[0];
    for (int k = 0; k < 9; ++k) S[k] = S[k] + row[1 + k];
  }
  if (n1 == 0) {
    plane[7] = 0.0;
    counts[3] = T3D_FLOOR_NONE;
    return;
  }
  const double dn = (double)n1;
  const double mx = S[0] / dn, my = S[1] / dn, mz = S[2] / dn;
  const double Sxx = S[3], Sxy = S[4], Syy = S[5], Sxz = S[6], Syz = S[7], Szz = S[8];
  const double det = Sxx * Syy - Sxy * Sxy;
  double a = (Sxz * Syy - Syz * Sxy) / det, b = (Syz * Sxx - Sxz * Sxy) / det;
  const double spread = (dn * p.min_spread) * p.min_spread;
  const bool ok = fl_finite(a) && fl_finite(b) && a * a + b * b <= p.max_slope2 && Sxx >= spread && Syy >= spread &&
                  det >= p.min_det_ratio * (Sxx * Syy);
  int flags = 0;
  if (!ok) { a = 0.0; b = 0.0; flags = T3D_FLOOR_LEVEL; }
  const double r = Szz - (a * Sxz + b * Syz);
  plane[0] = a; plane[1] = b; plane[2] = mz - (a * mx + b * my);
  plane[3] = mx; plane[4] = my; plane[5] = mz;
  plane[6] = (r > 0.0 ? r : 0.0) / dn;
  counts[1] = (int32_t)n1;
  counts[3] = flags;
}

__global__ __launch_bounds__(FL_THREADS) void k_detect_floor(const t3d_detect_floor_args p) {
  const int i = blockIdx.x * FL_THREADS + threadIdx.x;
  if (i >= p.n) return;
  float lab[7];
  bool finite = true;
  for (int k = 0; k < 7; ++k) {
    lab[k] = p.label[(size_t)i * 7 + k];
    finite = finite && fabsf(lab[k]) <= FLT_MAX;
  }
  const int s = p.scene_index[i];
  int flags = 0;
  if (s < 0 || s >= p.n_scenes || (p.counts[(size_t)s * 4 + 3] & T3D_FLOOR_NONE)) flags = T3D_DETECT_FLOOR_NO_FLOOR;
  if (!finite) flags |= T3D_DETECT_FLOOR_NOT_FINITE;
  double gap = 0.0;
  float h1 = lab[0], ty1 = lab[4];
  if (flags == 0) {
    const double* pl = p.plane + (size_t)s * 8;
    const double yf = -((pl[0] * (double)lab[3] + pl[1] * (double)lab[5]) + pl[2]);
    gap = yf - (double)lab[4];
    if (fabs(gap) > p.max_snap) flags |= T3D_DETECT_FLOOR_TOO_FAR;
    ty1 = (float)yf;
    if (p.mode == 2) {
      h1 = (float)(yf - ((double)lab[4] - (double)lab[0]));
      if (!(h1 > 0.0f)) flags |= T3D_DETECT_FLOOR_INVERTED;
    }
    if (p.mode != 0 && flags == 0) flags = T3D_DETECT_FLOOR_SNAPPED;
    p.gap[i] = gap;
  } else {
    reinterpret_cast<unsigned long long*>(p.gap)[i] = 0x7FF8000000000000ULL;
  }
  p.flags[i] = flags;
  const bool snapped = (flags & T3D_DETECT_FLOOR_SNAPPED) != 0;
  if (p.label_out) {
    float* o = p.label_out + (size_t)i * 7;
    for (int k = 0; k < 7; ++k) o[k] = lab[k];
    if (snapped) { o[0] = h1; o[4] = ty1; }
  }
  if (p.corners_out) {
    const float* c = p.corners + (size_t)i * 24;
    float* o = p.corners_out + (size_t)i * 24;
    for (int k = 0; k < 24; ++k) o[k] = c[k];
    if (snapped)
      for (int k = 0; k < 8; ++k) o[k * 3 + 1] = (k < 4 ? h1 : -h1) / 2.0f + (ty1 - h1 / 2.0f);
  }
}

inline bool fl_nonneg(double v) { return v >= 0.0; }      // false for a NaN

}  // namespace

extern "C" int t3d_scene_floor(const t3d_scene_floor_args* a, t3d_stream_t stream) {
  T3D_ABI_TAKE(scene_floor_args, a);
  if (!a || !a->points || !a->scene_offsets || !a->plane || !a->counts || !a->hist || !a->workspace || a->reserved != 0) return T3D_ERR_ARG;
  if (a->n_scenes < 0 || a->n_bins < 1) return T3D_ERR_ARG;
  if (!(a->bin > 0.0 && a->bin <= DBL_MAX) || !(a->inv_bin > 0.0 && a->inv_bin <= DBL_MAX) || !(a->z_hi > a->z_lo)) return T3D_ERR_ARG;
  if (!(a->min_share >= 0.0 && a->min_share <= 1.0) || a->min_inliers < 0) return T3D_ERR_ARG;
  if (!fl_nonneg(a->band) || !fl_nonneg(a->max_slope2) || !fl_nonneg(a->min_spread) || !fl_nonneg(a->min_det_ratio)) return T3D_ERR_ARG;
  if (a->n_bins > T3D_SCENE_FLOOR_MAX_BINS || a->ld < 3) return T3D_ERR_SHAPE;
  if (a->n_scenes > 65535) return T3D_ERR_SHAPE;
  if ((reinterpret_cast<uintptr_t>(a->workspace) & 7u) != 0 || a->workspace_bytes < T3D_SCENE_FLOOR_WORKSPACE_BYTES(a->n_scenes)) return T3D_ERR_ARG;
  if (a->n_scenes == 0) return T3D_OK;
  const hipStream_t st = static_cast<hipStream_t>(stream);
  const int S = a->n_scenes;
  if (hipMemsetAsync(a->hist, 0, (size_t)S * a->n_bins * sizeof(int32_t), st) != hipSuccess) return T3D_ERR_LAUNCH;
  if (hipMemsetAsync(a->counts, 0, (size_t)S * 4 * sizeof(int32_t), st) != hipSuccess) return T3D_ERR_LAUNCH;
  T3D_LAUNCH(k_floor_hist, dim3(FL_BLOCKS, S), dim3(FL_THREADS), 0, st, *a);
  T3D_CHECK_LAUNCH();
  T3D_LAUNCH(k_floor_peak, dim3(S), dim3(FL_THREADS), 0, st, *a);
  T3D_CHECK_LAUNCH();
  T3D_LAUNCH(k_floor_sums<false>, dim3(FL_BLOCKS, S), dim3(FL_THREADS), 0, st, *a);
  T3D_CHECK_LAUNCH();
  T3D_LAUNCH(k_floor_sums<true>, dim3(FL_BLOCKS, S), dim3(FL_THREADS), 0, st, *a);
  T3D_CHECK_LAUNCH();
  T3D_LAUNCH(k_floor_fit, dim3((S + 63) / 64), dim3(64), 0, st, *a);
  T3D_CHECK_LAUNCH();
  return T3D_OK;
}

extern "C" int t3d_detect_floor(const t3d_detect_floor_args* a, t3d_stream_t stream) {
  T3D_ABI_TAKE(detect_floor_args, a);
  if (!a || !a->label || !a->corners || !a->scene_index || !a->gap || !a->flags || a->reserved != 0) return T3D_ERR_ARG;
  if (a->n < 0 || a->n_scenes < 0 || (a->n_scenes > 0 && (!a->plane || !a->counts))) return T3D_ERR_ARG;
  if (a->mode < 0 || a->mode > 2 || (a->mode != 0 && (!a->label_out || !a->corners_out)) || !fl_nonneg(a->max_snap)) return T3D_ERR_ARG;
  if (a->n == 0) return T3D_OK;
  T3D_LAUNCH(k_detect_floor, dim3((a->n + FL_THREADS - 1) / FL_THREADS), dim3(FL_THREADS), 0, static_cast<hipStream_t>(stream), *a);
  T3D_CHECK_LAUNCH();
  return T3D_OK;
}
