// The lists of groups that t3d_detect_nms (nms.hip), t3d_detect_nms_sweep (nms_sweep.hip), t3d_detect_soft_nms (soft_nms.hip) and
// t3d_detect_fuse (fuse.hip) take, in one place for the device and for the host: the group of a list position and its contract, the
// lockstep walk of the groups that share a wave, and what the four launchers refuse and carve alike.  The order of a group and its pair
// bits, which only the two hard suppressions compute, are in nms_pairs_dev.h.
// Every template over `Args` takes t3d_detect_nms_args or a struct that has the fields it reads under the same names.
#pragma once
#include <type_traits>
#include "common.h"

namespace {

constexpr int NMS_THREADS = 256;

struct NmsGroup { int first, size; };      // size < 0: no group (past the lists, or a list that breaks the contract)

// Group g of the lists, as the caller declared them: {first, size}, or size < 0 for a g past the lists and for offsets that break the
// contract (descending, leaving [0, n], a group larger than max_group).  An empty group has size 0.
template <class Args>
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

template <class Args>
__device__ __forceinline__ bool nms_box_ok(const Args& a, int box) { return (unsigned)box < (unsigned)a.n; }

// The steps of a walk whose groups have LPG lanes each and share a wave: the largest `size` among the wave's groups.  The groups walk in
// lockstep, because the shuffles of a step need every lane: the count is wave-uniform, and nothing may leave an iteration early.
__device__ __forceinline__ int nms_wave_steps(int size) {
  int steps = size;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) steps = max(steps, __shfl_xor(steps, o, 64));
  return steps;
}

// The columns 64 w .. 64 w + nc - 1 of a group's bit rows as a mask of word w: the low nc bits, 0 <= nc <= 64.  Only these name boxes of
// the group: a row that k_nms_pairs did not write, under lists that break the contract, names no box outside it.
__device__ __forceinline__ unsigned long long nms_cols(int nc) { return nc >= 64 ? ~0ull : (1ull << nc) - 1ull; }

// ---- the host side ----

// What every launcher over the lists refuses before it looks at anything else, in the order the four entry points have always answered:
// T3D_ERR_ARG for a null struct, a negative n, n_groups or max_group and an unknown metric, then T3D_ERR_ARG where the entry point's own
// options are not in order (`options_ok`, which the caller evaluates behind `a &&`), then T3D_ERR_SHAPE for a max_group beyond
// T3D_DETECT_NMS_MAX_GROUP.  T3D_OK: go on, and *empty says whether there is a box to look at (a call without one launches nothing that
// reads the lists, whatever its pointers are).
template <class Args>
int nms_lists_gate(const Args* a, bool options_ok, bool* empty) {
  if (!a) return T3D_ERR_ARG;
  if (a->n < 0 || a->n_groups < 0 || a->max_group < 0) return T3D_ERR_ARG;
  if (a->metric != T3D_NMS_IOU3D && a->metric != T3D_NMS_IOU2D) return T3D_ERR_ARG;
  if (!options_ok) return T3D_ERR_ARG;
  if (a->max_group > T3D_DETECT_NMS_MAX_GROUP) return T3D_ERR_SHAPE;
  *empty = a->n == 0 || a->n_groups == 0 || a->max_group == 0;
  return T3D_OK;
}

// A workspace that holds an order starts with it: n int32, one per list position, padded to 8 bytes.  *rest: what follows, the unit's own.
template <class T>
int32_t* nms_carve(void* workspace, int n, T** rest) {
  *rest = reinterpret_cast<T*>(static_cast<char*>(workspace) + ((uint64_t)n + 1) / 2 * 8);
  return static_cast<int32_t*>(workspace);
}

// launch(std::integral_constant<int, LPG>, blocks) for a kernel that gives every group LPG lanes: LPG is the power of two >= lanes, at
// most MAX_LPG, and `blocks` workgroups of NMS_THREADS / LPG groups cover n_groups.
template <int MAX_LPG, int LPG = 1, class Launch>
void nms_for_lanes(int lanes, int n_groups, Launch&& launch) {
  if constexpr (LPG < MAX_LPG) {
    if (lanes > LPG) return nms_for_lanes<MAX_LPG, 2 * LPG>(lanes, n_groups, launch);
  }
  constexpr int GPB = NMS_THREADS / LPG;      // groups per workgroup
  launch(std::integral_constant<int, LPG>{}, (n_groups + GPB - 1) / GPB);
}

}  // namespace
