// The two kernels that t3d_detect_nms (nms.hip) and t3d_detect_nms_sweep (nms_sweep.hip) share: the order of every group by counting
// and the pair bits above the diagonal.  The sweep ranks its boxes and takes its IoUs with the very kernels the single suppression does
// -- it is that suppression for K thresholds, and its promise to answer what t3d_detect_nms answers rests on there being one body.
// Both run one thread per POSITION of the concatenated member lists (nms_dev.h nms_group_of).
#pragma once
#include "detbox_dev.h"
#include "nms_dev.h"

namespace {

__device__ __forceinline__ float nms_key(const t3d_detect_nms_args& a, int box) {
  const float s = nms_box_ok(a, box) ? a.score[box] : 0.f;
  return s != s ? -__builtin_inff() : s;
}

// position p of group g: the rank of its box by counting the boxes of g that come before it (size^2 comparisons per group, as k_order
// of sunrgbd_eval.hip); order[first(g) + rank] = box
__global__ __launch_bounds__(NMS_THREADS) void k_nms_order(const t3d_detect_nms_args a, int32_t* order) {
  const int p = blockIdx.x * NMS_THREADS + threadIdx.x;
  if (p >= a.n) return;
  const NmsGroup g = nms_group_of(a, p);
  if (g.size < 0) return;
  const int box = a.members[p];
  const float key = nms_key(a, box);
  int r = 0;
  for (int q = g.first; q < g.first + g.size; ++q) {
    const int other = a.members[q];
    const float k = nms_key(a, other);
    r += (k > key || (k == key && other < box)) ? 1 : 0;
  }
  if (r >= g.size) return;      // (a box listed twice: the contract is broken, nothing is written out of the group's rows)
  order[g.first + r] = box;
  if (a.rank && nms_box_ok(a, box)) a.rank[box] = r;
}

struct NmsThresholds { float t[T3D_NMS_SWEEP_MAX_THRESHOLDS]; };      // the first K are a call's (a.threshold is not read)

// (sorted position s of g, word w): bit c of mask[((first(g) + s) W + w) K + k] = IoU(box at s, box at 64 w + c) > th.t[k], for the columns
// 64 w + c > s only; words wholly below the diagonal are neither computed nor written (nor read by the walks).  Every IoU is computed
// once, whatever K is.  blockIdx.y is w: the lanes of a wave walk the same columns of the same few groups, the column loads are
// broadcasts.  Rows are W = ceil(max_group / 64) words apart, whatever the group's own size: a row's address needs no per-group prefix sum.
template <int KMAX>      // the thresholds a thread keeps bit words for: >= K (KMAX == 1: K is 1, and known to the compiler)
__global__ __launch_bounds__(NMS_THREADS) void k_nms_pairs(const t3d_detect_nms_args a, const int32_t* order, unsigned long long* mask,
                                                            int W, int K_given, const NmsThresholds th) {
  const int K = KMAX == 1 ? 1 : K_given;
  const int p = blockIdx.x * NMS_THREADS + threadIdx.x, w = blockIdx.y;
  if (p >= a.n) return;
  const NmsGroup g = nms_group_of(a, p);
  if (g.size < 0) return;
  const int s = p - g.first;                    // this row's sorted position
  const int c0 = max(s + 1, 64 * w), c1 = min(g.size, 64 * w + 64);
  if (64 * w + 63 < s || 64 * w >= g.size) return;       // wholly below the diagonal, or past the group: never read
  unsigned long long bits[KMAX];
#pragma unroll
  for (int k = 0; k < KMAX; ++k) bits[k] = 0;
  const int row = order[p];
  if (nms_box_ok(a, row)) {
    float k1[24];
#pragma unroll
    for (int i = 0; i < 24; ++i) k1[i] = a.corners[(size_t)row * 24 + i];
    for (int c = c0; c < c1; ++c) {
      const int col = order[g.first + c];
      if (!nms_box_ok(a, col)) continue;
      const float iou = iou_by_metric(k1, a.corners + (size_t)col * 24, a.metric);
      const unsigned long long bit = 1ull << (c - 64 * w);
#pragma unroll
      for (int k = 0; k < KMAX; ++k)
        if (k < K && iou > th.t[k]) bits[k] |= bit;      // a NaN compares false
    }
  }
  unsigned long long* out = mask + ((size_t)p * W + w) * K;
#pragma unroll
  for (int k = 0; k < KMAX; ++k)
    if (k < K) out[k] = bits[k];
}

}  // namespace
