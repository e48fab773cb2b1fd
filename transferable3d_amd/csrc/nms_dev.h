// Device code that t3d_detect_nms (nms.hip) and t3d_detect_nms_sweep (nms_sweep.hip) share: the group of a list position, a box's key and
// the order of every group by counting.  The sweep ranks its boxes with the very kernel the single suppression ranks them with.
// t3d_detect_soft_nms (soft_nms.hip) takes NMS_THREADS, nms_group_at and nms_box_ok from here: it has no fixed order to share.
#pragma once
#include "common.h"

namespace {

constexpr int NMS_THREADS = 256;

struct NmsGroup { int first, size; };      // size < 0: no group (past the lists, or a list that breaks the contract)

// Group g of the lists, as the caller declared them: {first, size}, or size < 0 for a g past the lists and for offsets that break the
// contract (descending, leaving [0, n], a group larger than max_group).  An empty group has size 0.
template <class Args>      // t3d_detect_nms_args, or a struct with its leading fields (t3d_detect_soft_nms_args)
__device__ __forceinline__ NmsGroup nms_group_at(const Args& a, int g) {
  if (g < 0 || g >= a.n_groups) return {0, -1};
  const int f = a.group_offsets[g], e = a.group_offsets[g + 1];
  if (f < 0 || e < f || e > a.n || e - f > a.max_group) return {0, -1};
  return {f, e - f};
}

// The group that holds position p of the concatenated lists: the first g with group_offsets[g + 1] > p (empty groups are stepped over).
template <class Args>
__device__ __forceinline__ NmsGroup nms_group_of(const Args& a, int p) {
  int lo = 0, hi = a.n_groups;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (a.group_offsets[mid + 1] <= p) lo = mid + 1; else hi = mid;
  }
  if (lo >= a.n_groups) return {0, -1};
  const int f = a.group_offsets[lo], e = a.group_offsets[lo + 1];
  if (f < 0 || f > p || e <= p || e > a.n || e - f > a.max_group) return {0, -1};
  return {f, e - f};
}

template <class Args>      // t3d_detect_nms_args, or a struct with its leading fields (t3d_detect_soft_nms_args)
__device__ __forceinline__ bool nms_box_ok(const Args& a, int box) { return (unsigned)box < (unsigned)a.n; }

__device__ __forceinline__ float nms_key(const t3d_detect_nms_args& a, int box) {
  const float s = nms_box_ok(a, box) ? a.score[box] : 0.f;
  return s != s ? -__builtin_inff() : s;
}

#ifndef NMS_DEV_NO_ORDER      // (a unit that ranks nothing defines it: soft_nms.hip)
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
#endif

}  // namespace
