// The percentile bootstrap over images for the official AP (t3d.h t3d_bootstrap_weights, t3d_sunrgbd_eval_bootstrap).
//   k_boot_clear / k_boot_draw   the weights: the matrix is cleared, then one thread per (replicate, draw) hashes its counter into a
//                                column and counts there by an integer atomic add;
//   k_boot_stream                after the evaluation of sunrgbd_eval.hip: per rank k the packed word det_col << 1 | is_tp of detection
//                                order[k], BS_NEITHER for one that counts in neither sum, so that a replicate reads one int32 stream and
//                                needs neither order, is_tp, is_fp nor det_col;
//   k_boot_curves<LDS>           one workgroup per replicate: its weight row staged in LDS (LDS) or gathered from global memory, n_pos,
//                                then the curve of ev_curve (sunrgbd_eval_dev.h) with 64-bit weighted counts: the same chunking, the
//                                same envelope scan, the same summation tree, so a row of ones gives the bytes of eval->ap.
// Everything is fp64 and int64; the only atomics are the integer adds of k_boot_draw.
#include <algorithm>

#include "sunrgbd_eval_dev.h"

namespace {

constexpr int BS_NEITHER = -1;
constexpr int BS_WAVES = EV_CURVE_THREADS / 64;
constexpr size_t BS_MAX_BLOCKS = 1 << 16;      // of the two weight kernels: beyond it a thread takes several elements
// dynamic LDS of k_boot_curves: the scan scratch (BS_WAVES int64, BS_WAVES doubles), then the weight row; everything 16-byte aligned
constexpr size_t BS_SCRATCH_BYTES = BS_WAVES * (sizeof(long long) + sizeof(double));
constexpr size_t BS_LDS_PER_CU = 160 * 1024;
constexpr size_t BS_MAX_ROW_BYTES = BS_LDS_PER_CU - BS_SCRATCH_BYTES;
static_assert(BS_SCRATCH_BYTES % 16 == 0, "the weight row starts 16-byte aligned");

__device__ __forceinline__ uint32_t bs_mix_u32(uint64_t x) {      // mix_u32 of data.hip / frustum.hip
  x ^= x >> 33; x *= 0xff51afd7ed558ccdULL;
  x ^= x >> 33; x *= 0xc4ceb9fe1a85ec53ULL;
  x ^= x >> 33;
  return (uint32_t)(x >> 16);
}

// (both over a flat index with a grid-stride loop: R * stride may exceed what a grid's x, let alone its y, can carry)
__global__ __launch_bounds__(EV_THREADS) void k_boot_clear(const t3d_bootstrap_weights_args p) {
  const size_t total = (size_t)p.R * p.stride, step = (size_t)gridDim.x * EV_THREADS;
  for (size_t e = (size_t)blockIdx.x * EV_THREADS + threadIdx.x; e < total; e += step) p.weights[e] = 0;
}

__global__ __launch_bounds__(EV_THREADS) void k_boot_draw(const t3d_bootstrap_weights_args p) {
  const size_t total = (size_t)p.R * p.n_images, step = (size_t)gridDim.x * EV_THREADS;
  for (size_t e = (size_t)blockIdx.x * EV_THREADS + threadIdx.x; e < total; e += step) {
    const uint64_t r = e / (size_t)p.n_images, d = e % (size_t)p.n_images;
    const uint64_t key = (((uint64_t)p.seed << 32) | r) * 0x9E3779B97F4A7C15ULL + (d + 1) * 0xD6E8FEB86659FD93ULL;
    const int col = (int)(((uint64_t)bs_mix_u32(key) * (uint64_t)p.n_images) >> 32);      // < n_images
    atomicAdd(p.weights + r * (size_t)p.stride + col, 1);                                 // integer: order-independent
  }
}

__global__ __launch_bounds__(EV_THREADS) void k_boot_stream(const t3d_sunrgbd_eval_args p, const t3d_sunrgbd_bootstrap_args b) {
  const int k = blockIdx.x * EV_THREADS + threadIdx.x;
  if (k >= p.P) return;
  const int i = p.order[k];
  const int col = b.det_col[i];
  const int tp = p.is_tp[i] != 0, fp = p.is_fp[i] != 0;
  static_cast<int32_t*>(b.workspace)[k] = (col >= 0 && col < b.weight_stride && (tp || fp)) ? (col << 1 | tp) : BS_NEITHER;
}

// ev_block_scan for one int64 per thread.  wsum: BS_WAVES int64 of LDS.
__device__ __forceinline__ long long bs_block_scan(long long v, long long* wsum, long long& total) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  long long x = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const long long y = __shfl_up(x, o, 64);
    if (lane >= o) x += y;
  }
  __syncthreads();
  if (lane == 63) wsum[wv] = x;
  __syncthreads();
  long long off = 0, tot = 0;
#pragma unroll 1
  for (int k = 0; k < BS_WAVES; ++k) {
    off += k < wv ? wsum[k] : 0;
    tot += wsum[k];
  }
  total = tot;
  return off + x - v;
}

template <bool LDS>
__global__ __launch_bounds__(EV_CURVE_THREADS) void k_boot_curves(const t3d_sunrgbd_eval_args p, const t3d_sunrgbd_bootstrap_args b) {
  extern __shared__ __attribute__((aligned(16))) unsigned char bs_lds[];
  long long* wsum = reinterpret_cast<long long*>(bs_lds);
  double* part = reinterpret_cast<double*>(bs_lds + BS_WAVES * sizeof(long long));
  int32_t* row_lds = reinterpret_cast<int32_t*>(bs_lds + BS_SCRATCH_BYTES);
  const int t = threadIdx.x, r = blockIdx.x, P = p.P;
  const int32_t* row = b.weights + (size_t)r * b.weight_stride;
  if (LDS) {
    for (int c = t; c < b.weight_stride; c += EV_CURVE_THREADS) row_lds[c] = row[c];
    __syncthreads();
  }
  const auto w_of = [&](int col) { return (long long)(LDS ? row_lds[col] : row[col]); };      // col in [0, weight_stride)
  // n_pos: the boxes of the resampled list
  long long mine = 0, n_pos;
  for (int g = t; g < p.G; g += EV_CURVE_THREADS) {
    const int col = b.gt_col[g];
    mine += (col >= 0 && col < b.weight_stride) ? w_of(col) : 0;
  }
  bs_block_scan(mine, wsum, n_pos);
  // ev_curve from here on, a packed word of the stream in place of tp_of / fp_of
  const int32_t* stream = static_cast<const int32_t*>(b.workspace);
  const bool have_gt = n_pos > 0;
  const auto rec_of = [&](long long ctp) { return have_gt ? (double)ctp / (double)n_pos : 0.0; };
  const auto pre_of = [](long long ctp, long long cfp) { return (double)ctp / ((double)cfp + (double)ctp); };      // 0 / 0 = NaN
  const int chunk = (P + EV_CURVE_THREADS - 1) / EV_CURVE_THREADS;
  const int k0 = min(t * chunk, P), k1 = min(k0 + chunk, P);
  long long ntp = 0, nfp = 0;
#pragma unroll 1
  for (int k = k0; k < k1; ++k) {
    const int s = stream[k];
    const long long w = s >= 0 ? w_of(s >> 1) : 0;
    ntp += (s & 1) ? w : 0;
    nfp += (s & 1) ? 0 : w;
  }
  long long n_tp, n_fp;
  long long ctp = bs_block_scan(ntp, wsum, n_tp);
  long long cfp = bs_block_scan(nfp, wsum, n_fp);
  double pmax = 0.0;
#pragma unroll 1
  for (int k = k0; k < k1; ++k) {
    const int s = stream[k];
    const long long w = s >= 0 ? w_of(s >> 1) : 0;
    ctp += (s & 1) ? w : 0;
    cfp += (s & 1) ? 0 : w;
    pmax = fmax(pmax, pre_of(ctp, cfp));
  }
  const int lane = t & 63, wv = t >> 6;
  double sfx = pmax;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const double y = __shfl_down(sfx, o, 64);
    if (lane + o < 64) sfx = fmax(sfx, y);
  }
  const double right = __shfl_down(sfx, 1, 64);
  if (lane == 0) part[wv] = sfx;
  __syncthreads();
  double run = lane < 63 ? right : 0.0;
  for (int k = wv + 1; k < BS_WAVES; ++k) run = fmax(run, part[k]);
  __syncthreads();
  double acc = 0.0;
#pragma unroll 1
  for (int k = k1 - 1; k >= k0; --k) {
    const int s = stream[k];
    const long long w = s >= 0 ? w_of(s >> 1) : 0;
    run = fmax(run, pre_of(ctp, cfp));
    const double r1 = rec_of(ctp);
    ctp -= (s & 1) ? w : 0;
    cfp -= (s & 1) ? 0 : w;
    const double r0 = k > 0 ? rec_of(ctp) : 0.0;
    if (r1 != r0) acc += (r1 - r0) * run;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_down(acc, o, 64);
  if (lane == 0) part[wv] = acc;
  __syncthreads();
  if (t == 0) {
    double sum = 0.0;
    for (int k = 0; k < BS_WAVES; ++k) sum += part[k];
    const double last = P > 0 ? rec_of(n_tp) : 0.0;
    if (1.0 != last) sum += (1.0 - last) * 0.0;
    b.ap[r] = (n_pos > 0 && P > 0) ? sum : 0.0;
    b.n_pos[r] = n_pos;
    b.n_tp[r] = n_tp;
    b.n_fp[r] = n_fp;
  }
}

}  // namespace

extern "C" int t3d_bootstrap_weights(const t3d_bootstrap_weights_args* a, t3d_stream_t stream) {
  T3D_ABI_TAKE(bootstrap_weights_args, a);
  if (!a || !a->weights) return T3D_ERR_ARG;
  if (a->R < 1 || a->R > T3D_BOOTSTRAP_MAX_REPLICATES || a->n_images < 1) return T3D_ERR_SHAPE;
  if (a->stride < a->n_images) return T3D_ERR_ARG;
  const hipStream_t st = static_cast<hipStream_t>(stream);
  const auto blocks = [](size_t n) { return dim3((unsigned)std::min<size_t>((n + EV_THREADS - 1) / EV_THREADS, BS_MAX_BLOCKS)); };
  T3D_LAUNCH(k_boot_clear, blocks((size_t)a->R * a->stride), dim3(EV_THREADS), 0, st, *a);
  T3D_CHECK_LAUNCH();
  T3D_LAUNCH(k_boot_draw, blocks((size_t)a->R * a->n_images), dim3(EV_THREADS), 0, st, *a);
  T3D_CHECK_LAUNCH();
  return T3D_OK;
}

extern "C" int t3d_sunrgbd_eval_bootstrap(const t3d_sunrgbd_eval_args* a, const t3d_sunrgbd_bootstrap_args* b, t3d_stream_t stream) {
  T3D_ABI_TAKE(sunrgbd_eval_args, a);
  T3D_ABI_TAKE(sunrgbd_bootstrap_args, b);
  if (!a || !b || !b->weights || !b->ap || !b->n_pos || !b->n_tp || !b->n_fp) return T3D_ERR_ARG;
  if (a->gt_difficult) return T3D_ERR_ARG;
  if (a->P < 0 || a->G < 0 || a->P > T3D_SUNRGBD_EVAL_MAX_BOXES || a->G > T3D_SUNRGBD_EVAL_MAX_BOXES) return T3D_ERR_SHAPE;
  if (b->R < 1 || b->R > T3D_BOOTSTRAP_MAX_REPLICATES || b->weight_stride < 1 || b->weight_stride > (1 << 30)) return T3D_ERR_SHAPE;
  if ((a->P > 0 && !b->det_col) || (a->G > 0 && !b->gt_col)) return T3D_ERR_ARG;
  if (a->P > 0 && (!b->workspace || b->workspace_bytes < T3D_SUNRGBD_BOOTSTRAP_WORKSPACE_BYTES(a->P) ||
                   (reinterpret_cast<uintptr_t>(b->workspace) & 7u)))
    return T3D_ERR_ARG;
  const int e = t3d_sunrgbd_eval(a, stream);   // every output of the evaluation, by the evaluation itself; it launches nothing when it refuses
  if (e != T3D_OK) return e;
  const hipStream_t st = static_cast<hipStream_t>(stream);
  if (a->P > 0) {
    T3D_LAUNCH(k_boot_stream, dim3((a->P + EV_THREADS - 1) / EV_THREADS), dim3(EV_THREADS), 0, st, *a, *b);
    T3D_CHECK_LAUNCH();
  }
  const size_t row_bytes = ((size_t)b->weight_stride * 4 + 15) / 16 * 16;
  if (row_bytes <= BS_MAX_ROW_BYTES) {
    const size_t lds = BS_SCRATCH_BYTES + row_bytes;
    static size_t allowed = 0;          // set the > 64 KB attribute once per size, not per launch
    if (lds > 64 * 1024 && lds > allowed) {
      (void)hipFuncSetAttribute(reinterpret_cast<const void*>(k_boot_curves<true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
      allowed = lds;
    }
    T3D_LAUNCH(k_boot_curves<true>, dim3(b->R), dim3(EV_CURVE_THREADS), lds, st, *a, *b);
  } else {
    T3D_LAUNCH(k_boot_curves<false>, dim3(b->R), dim3(EV_CURVE_THREADS), BS_SCRATCH_BYTES, st, *a, *b);
  }
  T3D_CHECK_LAUNCH();
  return T3D_OK;
}
