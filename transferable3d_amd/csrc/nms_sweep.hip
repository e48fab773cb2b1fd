// The greedy suppression of nms.hip for many configurations at once (t3d.h t3d_detect_nms_sweep): a configuration is one of K thresholds
// (or none) and a subset of the boxes ("listed"), and its answer is what t3d_detect_nms answers on the groups restricted to that subset.
// Neither the order of a group nor the IoU of a pair depends on the configuration -- the order of a subset is the induced order -- so
// both are computed once, by the kernels nms.hip launches (nms_pairs_dev.h):
//   k_nms_order     the rank of every box in its group, once;
//   k_nms_pairs     <4> or <16>, with K thresholds: (sorted position s of g, word w) computes each IoU(box at s, box at 64 w + c) once and
//                   sets bit c of K words, mask[(first(g) + s) W + w][k] = IoU > thresholds[k];
//   k_sweep_clear   keep[m, 0 .. n) = 0 and n_kept[m] = 0 for every configuration m (8 bytes per thread where the row allows it);
//   k_sweep_walk    k_nms_sweep per (configuration, group): blockIdx.y / .z carry the configuration, the lanes of a group start with
//                   the unlisted boxes of their words already "removed" (so those are never kept and suppress nothing), walk the ranks
//                   with the bit rows of the configuration's threshold, and write a 1 for every box left.  A configuration without a
//                   threshold skips the walk.  The ones are counted per wave and added to n_kept[m] by one integer atomic.
// The work per configuration is spread over ceil(n_groups / groups per workgroup) workgroups, as the single suppression's is.
#include "nms_pairs_dev.h"

namespace {

constexpr int SW_Y = 32768;      // configurations along gridDim.y; gridDim.z carries the rest (a grid's y and z end at 65535)

__device__ __forceinline__ int sw_config() { return blockIdx.z * SW_Y + blockIdx.y; }

__global__ __launch_bounds__(NMS_THREADS) void k_sweep_clear(const t3d_detect_nms_sweep_args s, int n_clear) {
  const int m = sw_config();
  if (m >= s.M) return;
  const int i = blockIdx.x * NMS_THREADS + threadIdx.x;
  if (i == 0) s.n_kept[m] = 0;
  const int b0 = 8 * i, b1 = min(b0 + 8, n_clear);
  if (b0 >= b1) return;
  uint8_t* row = s.keep + (size_t)m * s.keep_stride;
  if (b1 - b0 == 8 && (reinterpret_cast<uintptr_t>(row + b0) & 7u) == 0) {
    *reinterpret_cast<unsigned long long*>(row + b0) = 0ull;
  } else {
    for (int b = b0; b < b1; ++b) row[b] = 0;
  }
}

template <int LPG>      // lanes per group: a power of two, >= W
__global__ __launch_bounds__(NMS_THREADS) void k_sweep_walk(const t3d_detect_nms_args a, const t3d_detect_nms_sweep_args s,
                                                             const int32_t* order, const unsigned long long* mask, int W) {
  constexpr int GPB = NMS_THREADS / LPG;        // groups per workgroup
  const int m = sw_config();
  if (m >= s.M) return;                          // (the workgroup as a whole)
  const int ct = s.config_threshold[m], K = s.n_thresholds;
  if (ct < -1 || ct >= K) return;                // not a configuration: its row stays 0
  const int gi = blockIdx.x * GPB + threadIdx.x / LPG, w = threadIdx.x % LPG;
  const NmsGroup g = nms_group_at(a, gi);       // (a group that breaks the contract is not visited)
  const int first = g.first, size = max(g.size, 0);
  const bool has_word = 64 * w < size;           // (implies w < W)
  const int nc = has_word ? min(64, size - 64 * w) : 0;
  const unsigned long long cols = nms_cols(nc);
  // the boxes of this lane's word that take part in configuration m
  unsigned long long in = 0;
  const uint8_t* listed = s.listed ? s.listed + (size_t)m * s.listed_stride : nullptr;
  for (int c = 0; c < nc; ++c) {
    const int box = order[first + 64 * w + c];
    if (nms_box_ok(a, box) && (!listed || listed[box] != 0)) in |= 1ull << c;
  }
  unsigned long long removed = cols & ~in;       // a box that is not listed is never kept, and its row is never taken
  if (ct >= 0) {                                  // (the same for every lane of the workgroup)
    const int steps = nms_wave_steps(size);
    for (int st = 0; st < steps; ++st) {
      const int sw = st >> 6;
      const unsigned long long owner = LPG == 1 ? removed : __shfl(removed, sw, LPG);
      const bool kept = st < size && !((owner >> (st & 63)) & 1ull);
      if (kept && has_word && w >= sw) removed |= mask[((size_t)(first + st) * W + w) * K + ct] & cols;
    }
  }
  unsigned long long left = cols & ~removed;
  int count = 0;
  uint8_t* row = s.keep + (size_t)m * s.keep_stride;
  while (left) {
    const int c = __ffsll((long long)left) - 1;
    left &= left - 1;
    row[order[first + 64 * w + c]] = 1;          // (a bit of `in`: the box index was checked above)
    ++count;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) count += __shfl_xor(count, o, 64);
  if ((threadIdx.x & 63) == 0 && count > 0) atomicAdd(&s.n_kept[m], count);      // an integer sum: order-independent
}

}  // namespace

extern "C" int t3d_detect_nms_sweep(const t3d_detect_nms_sweep_args* s, t3d_stream_t stream) {
  T3D_ABI_TAKE(detect_nms_sweep_args, s);
  bool empty;
  if (const int refused = nms_lists_gate(s, true, &empty)) return refused;
  if (s->M < 1 || s->M > T3D_SWEEP_MAX_CONFIGS) return T3D_ERR_SHAPE;
  if (s->n_thresholds < 1 || s->n_thresholds > T3D_NMS_SWEEP_MAX_THRESHOLDS) return T3D_ERR_SHAPE;
  NmsThresholds th;
  for (int k = 0; k < T3D_NMS_SWEEP_MAX_THRESHOLDS; ++k) {
    th.t[k] = k < s->n_thresholds ? s->thresholds[k] : 0.f;
    if (th.t[k] != th.t[k]) return T3D_ERR_ARG;
  }
  if (!s->n_kept) return T3D_ERR_ARG;
  if (s->keep && s->keep_stride < s->n) return T3D_ERR_ARG;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int my = s->M < SW_Y ? s->M : SW_Y, mz = (s->M + SW_Y - 1) / SW_Y;
  if (!empty) {
    if (!s->corners || !s->score || !s->group_offsets || !s->members || !s->config_threshold || !s->keep || !s->workspace) return T3D_ERR_ARG;
    if (s->listed && s->listed_stride < s->n) return T3D_ERR_ARG;
    if (s->workspace_bytes < T3D_DETECT_NMS_SWEEP_WORKSPACE_BYTES(s->n, s->max_group, s->n_thresholds) ||
        (reinterpret_cast<uintptr_t>(s->workspace) & 7u))
      return T3D_ERR_ARG;
  }
  // n_kept reads 0 whatever follows, and so does every keep row: the one launch of an empty call (which writes no row without `keep`)
  const int n_clear = s->keep ? s->n : 0;
  const int clear_blocks = ((n_clear + 7) / 8 + NMS_THREADS - 1) / NMS_THREADS;
  T3D_LAUNCH(k_sweep_clear, dim3(clear_blocks > 0 ? clear_blocks : 1, my, mz), dim3(NMS_THREADS), 0, st, *s, n_clear);
  T3D_CHECK_LAUNCH();
  if (empty) return T3D_OK;
  const int W = (s->max_group + 63) / 64, K = s->n_thresholds;
  unsigned long long* mask;
  int32_t* order = nms_carve(s->workspace, s->n, &mask);
  t3d_detect_nms_args a;      // what nms.hip's kernels read of a call: the boxes, the scores and the lists
  memset(&a, 0, sizeof(a));
  a.struct_size = (uint32_t)sizeof(a);
  a.n = s->n; a.n_groups = s->n_groups; a.metric = s->metric;
  a.corners = s->corners; a.score = s->score; a.group_offsets = s->group_offsets; a.members = s->members;
  a.max_group = s->max_group;
  const int blocks = (s->n + NMS_THREADS - 1) / NMS_THREADS;
  T3D_LAUNCH(k_nms_order, dim3(blocks), dim3(NMS_THREADS), 0, st, a, order);
  T3D_CHECK_LAUNCH();
  if (K <= 4) T3D_LAUNCH(k_nms_pairs<4>, dim3(blocks, W), dim3(NMS_THREADS), 0, st, a, order, mask, W, K, th);
  else T3D_LAUNCH(k_nms_pairs<T3D_NMS_SWEEP_MAX_THRESHOLDS>, dim3(blocks, W), dim3(NMS_THREADS), 0, st, a, order, mask, W, K, th);
  T3D_CHECK_LAUNCH();
  nms_for_lanes<16>(W, s->n_groups, [&](auto lpg, int group_blocks) {
    T3D_LAUNCH(k_sweep_walk<decltype(lpg)::value>, dim3(group_blocks, my, mz), dim3(NMS_THREADS), 0, st, a, *s, order, mask, W);
  });
  T3D_CHECK_LAUNCH();
  return T3D_OK;
}
