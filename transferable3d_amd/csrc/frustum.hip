// Frustum extraction from SUN-RGBD scenes (t3d.h t3d_frustum_extract), in place of the reference's per-box host loop
// extract_roi_seg / extract_roi_seg_from_rgb_detection (sunrgbd/sunrgbd_data/sunrgbd_data.py:64-195, 221-326; helpers utils.py:78-130,
// 198-291).  Three launches over a batch of scenes, no host synchronisation between them:
//   k_frustum_boxes   one thread per job: the (perturbed) 2-D box and the frustum angle;
//   k_frustum_mask    one thread per point: fp64 projection to the image, then, for every job of the point's scene, a wave64 ballot of
//                     "uv inside the box" -> one 64-bit membership mask per (job, 64-point segment);
//   k_frustum_select  one workgroup per job: exclusive scan of the masks' popcounts (rank of every frustum point, in the cloud's order),
//                     the subsample (given ranks, or the num_points smallest hash keys by radix select), then the gather of the kept
//                     points in upright camera coordinates and their 3-D box labels.
// Nothing depends on atomics' order: the result is a function of the inputs and of (seed, job key) only, not of the batch.
#include "common.h"

// The reference's projection and box arithmetic is NumPy fp64, elementwise: no fused multiply-adds, so that the perturbed boxes and the
// angles round as the reference's do.
#pragma clang fp contract(off)

namespace {

constexpr int FX_THREADS = 256;
constexpr int FX_MAX_POINTS = 4096;
constexpr int FX_JOB_TILE = 128;

__device__ __forceinline__ uint32_t fx_mix(uint64_t x) {      // the finaliser of data.hip's counter-based hash
  x ^= x >> 33; x *= 0xff51afd7ed558ccdULL;
  x ^= x >> 33; x *= 0xc4ceb9fe1a85ec53ULL;
  x ^= x >> 33;
  return (uint32_t)(x >> 16);
}
__device__ __forceinline__ uint64_t fx_job_base(uint32_t seed, const int32_t* key) {
  return ((uint64_t)seed << 32) ^ ((uint64_t)(uint32_t)key[0] * 0x9E3779B97F4A7C15ULL) ^
         ((uint64_t)(uint32_t)(key[1] + 1) * 0xA24BAED4963EE407ULL) ^ ((uint64_t)(uint32_t)(key[2] + 1) * 0xC2B2AE3D27D4EB4FULL);
}
__device__ __forceinline__ uint32_t fx_rank_key(uint64_t base, uint32_t r) {
  return fx_mix(base + ((uint64_t)r + 1ull) * 0xD6E8FEB86659FD93ULL);
}
__device__ __forceinline__ double fx_uniform(uint64_t base, int i) {
  return ((double)fx_mix((base ^ 0x632BE59BD9B4E019ULL) + (uint64_t)(i + 1) * 0x165667B19E3779F9ULL) + 0.5) * (1.0 / 4294967296.0);
}

__device__ __forceinline__ int fx_scene_of(const int32_t* scene_jobs, int n_scenes, int j) {
  int lo = 0, hi = n_scenes - 1;          // the last scene whose first job is <= j (empty scenes share their first job)
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (scene_jobs[mid] <= j) lo = mid; else hi = mid - 1;
  }
  return lo;
}

__global__ __launch_bounds__(FX_THREADS) void k_frustum_boxes(const t3d_frustum_extract_args p) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= p.n_jobs) return;
  double xmin = p.box2d[j * 4], ymin = p.box2d[j * 4 + 1], xmax = p.box2d[j * 4 + 2], ymax = p.box2d[j * 4 + 3];
  if (p.perturb_box2d) {                  // utils.random_shift_box2d, operation for operation
    const uint64_t base = fx_job_base(p.seed, p.job_key + (size_t)j * 3);
    double u[4];
    for (int i = 0; i < 4; ++i) u[i] = p.perturb_draws ? p.perturb_draws[(size_t)j * 4 + i] : fx_uniform(base, i);
    const double r = 0.1;
    const double h = ymax - ymin, w = xmax - xmin;
    const double cx = (xmin + xmax) / 2.0, cy = (ymin + ymax) / 2.0;
    const double cx2 = cx + w * r * (u[0] * 2 - 1);
    const double cy2 = cy + h * r * (u[1] * 2 - 1);
    const double h2 = h * (1 + u[2] * 2 * r - r);
    const double w2 = w * (1 + u[3] * 2 * r - r);
    xmin = cx2 - w2 / 2.0; ymin = cy2 - h2 / 2.0; xmax = cx2 + w2 / 2.0; ymax = cy2 + h2 / 2.0;
  }
  p.box2d_out[(size_t)j * 4] = xmin; p.box2d_out[(size_t)j * 4 + 1] = ymin;
  p.box2d_out[(size_t)j * 4 + 2] = xmax; p.box2d_out[(size_t)j * 4 + 3] = ymax;
  // project_image_to_upright_camerea of the box centre at depth 20 (utils.py:115-129), then -arctan2(z, x)
  const int s = fx_scene_of(p.scene_jobs, p.n_scenes, j);
  const double* K = p.K + (size_t)s * 9;
  const double* R = p.rtilt + (size_t)s * 9;
  const double uc = (xmin + xmax) / 2.0, vc = (ymin + ymax) / 2.0, d = 20.0;
  const double x = ((uc - K[2]) * d) / K[0], y = ((vc - K[5]) * d) / K[4];
  const double q0 = x, q1 = d, q2 = -y;                                     // flip_axis_to_depth
  const double X = R[0] * q0 + R[1] * q1 + R[2] * q2;
  const double Y = R[3] * q0 + R[4] * q1 + R[5] * q2;                       // upright camera z = upright depth y
  p.frustum_angle[j] = -atan2(Y, X);
}

__global__ __launch_bounds__(FX_THREADS) void k_frustum_mask(const t3d_frustum_extract_args p) {
  __shared__ double box[FX_JOB_TILE][4];
  const int s = blockIdx.y;
  const int64_t lo = p.scene_offsets[s];
  const int n = (int)(p.scene_offsets[s + 1] - lo);
  const int j0 = p.scene_jobs[s], j1 = p.scene_jobs[s + 1];
  if ((int)blockIdx.x * FX_THREADS >= n || j0 >= j1) return;              // uniform over the workgroup
  const int i = blockIdx.x * FX_THREADS + threadIdx.x, lane = threadIdx.x & 63, g = i >> 6;
  const bool valid = i < n;
  double u = 0.0, v = 0.0;
  if (valid) {
    // project_upright_depth_to_image (utils.py:93-107): Rtilt^T p, flip_axis_to_camera, K, divide
    const double* pt = p.points + (size_t)(lo + i) * p.C_src;
    const double px = pt[0], py = pt[1], pz = pt[2];
    const double* R = p.rtilt + (size_t)s * 9;
    const double* K = p.K + (size_t)s * 9;
    const double d0 = R[0] * px + R[3] * py + R[6] * pz;
    const double d1 = R[1] * px + R[4] * py + R[7] * pz;
    const double d2 = R[2] * px + R[5] * py + R[8] * pz;
    const double c0 = d0, c1 = -d2, c2 = d1;
    const double w0 = c0 * K[0] + c1 * K[1] + c2 * K[2];
    const double w1 = c0 * K[3] + c1 * K[4] + c2 * K[5];
    const double w2 = c0 * K[6] + c1 * K[7] + c2 * K[8];
    u = w0 / w2;
    v = w1 / w2;
  }
  for (int t0 = j0; t0 < j1; t0 += FX_JOB_TILE) {
    const int nt = min(FX_JOB_TILE, j1 - t0);
    __syncthreads();
    for (int k = threadIdx.x; k < nt * 4; k += FX_THREADS) box[k >> 2][k & 3] = p.box2d_out[(size_t)t0 * 4 + k];
    __syncthreads();
    for (int k = 0; k < nt; ++k) {
      // sunrgbd_data.py:85 / 293: u < xmax & u >= xmin & v < ymax & v >= ymin (NaN: outside)
      const bool in = valid && u < box[k][2] && u >= box[k][0] && v < box[k][3] && v >= box[k][1];
      const unsigned long long m = __ballot(in);
      const int64_t off = p.mask_offsets[t0 + k];
      if (lane == 0 && g < p.mask_offsets[t0 + k + 1] - off) p.masks[off + g] = m;
    }
  }
}

// Exclusive prefix sum over the 256 threads of the workgroup (4 waves); `total` receives the sum.  `wsum`: 4 ints of LDS.
__device__ __forceinline__ int fx_block_scan(int v, int* wsum, int& total) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  int x = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int y = __shfl_up(x, o, 64);
    if (lane >= o) x += y;
  }
  if (lane == 63) wsum[w] = x;
  __syncthreads();
  int off = 0;
  for (int k = 0; k < w; ++k) off += wsum[k];
  total = wsum[0] + wsum[1] + wsum[2] + wsum[3];
  __syncthreads();
  return off + x - v;
}

// The k-th smallest (1-based) key(r) over the r in [0, n) with pred(r), 8 bits a pass; *k_rem: how many of the k smallest equal it.
template <class KeyF, class PredF>
__device__ uint32_t fx_radix_select(int n, int k, KeyF key, PredF pred, int* hist, int* bcast, int* k_rem) {
  uint32_t prefix = 0u, mask = 0u;
  int krem = k;
  for (int shift = 24; shift >= 0; shift -= 8) {
    hist[threadIdx.x] = 0;
    __syncthreads();
    for (int r = threadIdx.x; r < n; r += FX_THREADS) {
      if (!pred(r)) continue;
      const uint32_t kv = key(r);
      if ((kv & mask) == prefix) atomicAdd(&hist[(kv >> shift) & 255u], 1);   // counts only: the order of the adds is immaterial
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      int cum = 0, d = 0;
      for (; d < 255; ++d) {
        if (cum + hist[d] >= krem) break;
        cum += hist[d];
      }
      bcast[0] = d;
      bcast[1] = krem - cum;
    }
    __syncthreads();
    prefix |= (uint32_t)bcast[0] << shift;
    mask |= 255u << shift;
    krem = bcast[1];
    __syncthreads();
  }
  *k_rem = krem;
  return prefix;
}

__global__ __launch_bounds__(FX_THREADS) void k_frustum_select(const t3d_frustum_extract_args p) {
  __shared__ int ranks[FX_MAX_POINTS];
  __shared__ int hist[256];
  __shared__ int wsum[4];
  __shared__ int bcast[2];
  const int j = blockIdx.x, NP = p.num_points;
  const int s = fx_scene_of(p.scene_jobs, p.n_scenes, j);
  const int64_t lo = p.scene_offsets[s];
  const int n_scene = (int)(p.scene_offsets[s + 1] - lo);
  const int64_t moff = p.mask_offsets[j];
  const int G = (int)(p.mask_offsets[j + 1] - moff);
  const uint64_t* masks = p.masks + moff;
  int32_t* seg_prefix = p.seg_prefix + moff;
  // rank of the first frustum point of every segment
  int n = 0;
  for (int g0 = 0; g0 < G; g0 += FX_THREADS) {
    const int g = g0 + threadIdx.x;
    const int c = g < G ? __popcll(masks[g]) : 0;
    int tot;
    const int e = fx_block_scan(c, wsum, tot);
    if (g < G) seg_prefix[g] = n + e;
    n += tot;
  }
  const int count = min(n, NP);
  // the ranks to keep, in output order
  const bool given = n > NP && p.choice != nullptr && p.choice[(size_t)j * NP] >= 0;
  if (n <= NP) {
    for (int k = threadIdx.x; k < n; k += FX_THREADS) ranks[k] = k;
  } else if (given) {
    for (int k = threadIdx.x; k < NP; k += FX_THREADS) ranks[k] = p.choice[(size_t)j * NP + k];
  } else {
    // the NP smallest (key, rank) pairs: the NP-th smallest key T, then among the ranks of key T the k_rem smallest
    const uint64_t base = fx_job_base(p.seed, p.job_key + (size_t)j * 3);
    int krem, krem2;
    const uint32_t T = fx_radix_select(n, NP, [&](int r) { return fx_rank_key(base, (uint32_t)r); }, [](int) { return true; },
                                       hist, bcast, &krem);
    const uint32_t Rsel = fx_radix_select(n, krem, [](int r) { return (uint32_t)r; },
                                          [&](int r) { return fx_rank_key(base, (uint32_t)r) == T; }, hist, bcast, &krem2);
    int carry = 0;
    for (int r0 = 0; r0 < n; r0 += FX_THREADS) {
      const int r = r0 + threadIdx.x;
      bool sel = false;
      if (r < n) {
        const uint32_t kv = fx_rank_key(base, (uint32_t)r);
        sel = kv < T || (kv == T && (uint32_t)r <= Rsel);
      }
      int tot;
      const int e = fx_block_scan(sel ? 1 : 0, wsum, tot);
      if (sel && carry + e < NP) ranks[carry + e] = r;
      carry += tot;
    }
  }
  __syncthreads();
  const double* box = p.box3d ? p.box3d + (size_t)j * 24 : nullptr;
  for (int k = threadIdx.x; k < NP; k += FX_THREADS) {
    const size_t o = (size_t)j * NP + k;
    double* dst = p.out_points + o * p.C;
    int idx = -1;
    if (k < count) {
      const int r = ranks[k];
      if (r >= 0 && r < n) {
        int a = 0, b = G - 1;               // the last segment whose first rank is <= r (empty segments share their first rank)
        while (a < b) {
          const int mid = (a + b + 1) >> 1;
          if (seg_prefix[mid] <= r) a = mid; else b = mid - 1;
        }
        unsigned long long m = masks[a];
        for (int t = r - seg_prefix[a]; t > 0; --t) m &= m - 1ull;
        const int i = a * 64 + __ffsll((long long)m) - 1;
        if (m != 0ull && i < n_scene) idx = i;
      }
    }
    p.index[o] = idx;
    int lab = 0;
    if (idx >= 0) {
      const double* src = p.points + (size_t)(lo + idx) * p.C_src;
      const double x = src[0], y = -src[2], z = src[1];                    // flip_axis_to_camera
      dst[0] = x; dst[1] = y; dst[2] = z;
      for (int c = 3; c < p.C; ++c) dst[c] = src[c];
      if (box) {
        // inside or on the parallelepiped spanned at corner 1 by the edges to corners 2, 5 and 0 (compute_box_3d's order)
        const double q[3] = {x - box[3], y - box[4], z - box[5]};
        bool in = true;
        const int far[3] = {2, 5, 0};
        for (int e = 0; e < 3; ++e) {
          const double ex = box[far[e] * 3] - box[3], ey = box[far[e] * 3 + 1] - box[4], ez = box[far[e] * 3 + 2] - box[5];
          const double dv = q[0] * ex + q[1] * ey + q[2] * ez, dd = ex * ex + ey * ey + ez * ez;
          in = in && dv >= 0.0 && dv <= dd;
        }
        lab = in ? 1 : 0;
      }
    } else {
      for (int c = 0; c < p.C; ++c) dst[c] = 0.0;
    }
    if (p.label) p.label[o] = lab;
  }
  if (threadIdx.x == 0) {
    p.n_in_box[j] = n;
    p.count[j] = count;
  }
}

}  // namespace

extern "C" int t3d_frustum_extract(const t3d_frustum_extract_args* a, t3d_stream_t stream) {
  T3D_ABI_TAKE(frustum_extract_args, a);
  if (!a || !a->points || !a->scene_offsets || !a->rtilt || !a->K || !a->scene_jobs || !a->box2d || !a->job_key || !a->mask_offsets ||
      !a->masks || !a->seg_prefix || !a->box2d_out || !a->frustum_angle || !a->n_in_box || !a->count || !a->index || !a->out_points)
    return T3D_ERR_ARG;
  if (a->box3d && !a->label) return T3D_ERR_ARG;
  if (a->n_scenes <= 0 || a->n_scenes > 65535 || a->n_jobs < 0 || a->max_scene_points < 0 || a->num_points <= 0 ||
      a->num_points > FX_MAX_POINTS || a->C < 3 || a->C_src < a->C)
    return T3D_ERR_SHAPE;
  if (a->n_jobs == 0) return T3D_OK;
  const hipStream_t st = static_cast<hipStream_t>(stream);
  T3D_LAUNCH(k_frustum_boxes, dim3((a->n_jobs + FX_THREADS - 1) / FX_THREADS), dim3(FX_THREADS), 0, st, *a);
  T3D_CHECK_LAUNCH();
  if (a->max_scene_points > 0) {
    T3D_LAUNCH(k_frustum_mask, dim3((a->max_scene_points + FX_THREADS - 1) / FX_THREADS, a->n_scenes), dim3(FX_THREADS), 0, st, *a);
    T3D_CHECK_LAUNCH();
  }
  T3D_LAUNCH(k_frustum_select, dim3(a->n_jobs), dim3(FX_THREADS), 0, st, *a);
  T3D_CHECK_LAUNCH();
  return T3D_OK;
}
