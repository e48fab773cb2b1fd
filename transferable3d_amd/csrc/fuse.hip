// Box voting behind t3d_detect_nms (t3d.h t3d_detect_fuse): every kept box takes the weighted mean geometry of the cluster it suppressed.
// The reference has no such step; it is opt-in.  The semantics are stated in t3d.h and executed in fp64 NumPy by tests/fake_fuse.py.
//
// As in nms.hip nothing is laid out per group: both kernels run one thread per POSITION of the concatenated member lists and find
// their group by a binary search of group_offsets (nms_dev.h nms_group_of, under t3d_detect_nms's contract).  The IoUs are computed where every lane has one to compute, the sums where they
// have to be in order:
//   k_fuse_votes   the thread of box b writes order[first(g) + rank[b]] = b (the rank order of every group, rebuilt from what
//                  t3d_detect_nms answered) and, where b is suppressed, its vote at that same slot: the IoU with the box that suppressed
//                  it, the quarter turn that aligns it and the heading difference that is left -- or "no vote".  One IoU per suppressed
//                  box in all (against the size^2 / 2 of the NMS), no lane waiting for another's;
//   k_fuse         the thread of a suppressed box copies its label and corners; the thread of a kept box walks the later ranks of its
//                  group, takes the votes cast for it, sums in fp64 in rank order and writes the fused label and its corners.
// (A first form had the kept box's thread compute the IoUs of its cluster while walking: the lanes of a wave met their members at
// different steps, so the IoU code ran once per step for a lane or two -- 1.57 ms on the load of tools/bench_detect_fuse.py.)
// No atomics, no LDS, no dependence on the grid: a group's outputs are a function of its own boxes.
#include "common.h"
#include "detbox_dev.h"
#include "nms_dev.h"

#pragma clang fp contract(off)

namespace {

constexpr int FUSE_THREADS = 256;

struct FuseVote { double delta; float iou; int k; };      // iou < 0: no vote

__global__ __launch_bounds__(FUSE_THREADS) void k_fuse_votes(const t3d_detect_fuse_args a, int32_t* order, FuseVote* vote) {
  const int p = blockIdx.x * FUSE_THREADS + threadIdx.x;
  if (p >= a.n) return;
  const NmsGroup g = nms_group_of(a, p);
  if (g.size < 0) return;
  const int j = a.members[p];
  if (!nms_box_ok(a, j)) return;
  const int r = a.rank[j];
  if (r < 0 || r >= g.size) return;             // (not a rank of this group: the slot keeps what it held, k_fuse checks what it reads)
  order[g.first + r] = j;
  FuseVote v = {0.0, -1.f, 0};
  const int i = a.suppressed_by[j];
  const float* lj = a.label + (size_t)j * 7;
  if (a.keep[j] == 0 && nms_box_ok(a, i) && i != j && detbox_label_ok(lj)) {
    // both boxes relative to the anchor's first corner: box3d_iou_corners sums rectangle areas on the coordinates as they stand, which
    // tens of metres from the origin costs the ground-plane IoU some 4e-5 -- nothing to a threshold, but it is this vote's weight
    float k1[24], k2[24];
    const float ox = a.corners[(size_t)i * 24], oy = a.corners[(size_t)i * 24 + 1], oz = a.corners[(size_t)i * 24 + 2];
#pragma unroll
    for (int c = 0; c < 24; ++c) {
      const float o = c % 3 == 0 ? ox : (c % 3 == 1 ? oy : oz);
      k1[c] = a.corners[(size_t)i * 24 + c] - o;
      k2[c] = a.corners[(size_t)j * 24 + c] - o;
    }
    const float iou = iou_by_metric(k1, k2, a.metric);
    if (iou > a.vote_threshold) {               // (a NaN does not vote)
      const double HALF_PI = 3.14159265358979323846 / 2.0;
      const double d = (double)lj[6] - (double)a.label[(size_t)i * 7 + 6];
      v.iou = iou;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const double wr = detbox_wrap(d + (double)k * HALF_PI);
        if (k == 0 || fabs(wr) < fabs(v.delta)) { v.delta = wr; v.k = k; }
      }
    }
  }
  vote[g.first + r] = v;
}

__global__ __launch_bounds__(FUSE_THREADS) void k_fuse(const t3d_detect_fuse_args a, const int32_t* order, const FuseVote* vote) {
  const int p = blockIdx.x * FUSE_THREADS + threadIdx.x;
  if (p >= a.n) return;
  const NmsGroup g = nms_group_of(a, p);
  if (g.size < 0) return;
  const int i = a.members[p];
  if (!nms_box_ok(a, i)) return;
  const float* li = a.label + (size_t)i * 7;
  float* lo = a.label_out + (size_t)i * 7;
  float* ko = a.corners_out + (size_t)i * 24;

  const bool kept = a.keep[i] != 0;
  const double h_i = li[0], w_i = li[1], l_i = li[2], ry_i = li[6];
  const double cx_i = li[3], cy_i = (double)li[4] - h_i / 2.0, cz_i = li[5];
  int votes = 0;
  const double wa = detbox_weight(a.weight[i]);
  double W = wa, sx = wa * cx_i, sy = wa * cy_i, sz = wa * cz_i, sl = wa * l_i, sw = wa * w_i, sh = wa * h_i, sd = 0.0;
  const int r = a.rank[i];
  if (kept && detbox_label_ok(li) && r >= 0 && r < g.size) {
    for (int s = r + 1; s < g.size; ++s) {
      const int j = order[g.first + s];
      if (!nms_box_ok(a, j) || j == i || a.keep[j] != 0 || a.suppressed_by[j] != i) continue;
      const FuseVote v = vote[g.first + s];
      if (!(v.iou >= 0.f)) continue;
      ++votes;
      const float* lj = a.label + (size_t)j * 7;
      const double h_j = lj[0];
      const double l_j = (v.k & 1) ? lj[1] : lj[2], w_j = (v.k & 1) ? lj[2] : lj[1];      // (l and w exchanged for an odd quarter turn)
      const double wj = detbox_weight(a.weight[j]) * (double)v.iou;
      W = W + wj;
      sx = sx + wj * (double)lj[3];
      sy = sy + wj * ((double)lj[4] - h_j / 2.0);
      sz = sz + wj * (double)lj[5];
      sl = sl + wj * l_j;
      sw = sw + wj * w_j;
      sh = sh + wj * h_j;
      sd = sd + wj * v.delta;
    }
  }
  a.n_votes[i] = kept ? votes : -1;
  if (votes == 0 || !(W > 0.0) || !detbox_finite(W)) {      // nothing to fuse: byte copies
#pragma unroll
    for (int c = 0; c < 7; ++c) lo[c] = li[c];
#pragma unroll
    for (int c = 0; c < 24; ++c) ko[c] = a.corners[(size_t)i * 24 + c];
    return;
  }
  const double hd = sh / W, cyd = sy / W;
  const float h = (float)hd, w = (float)(sw / W), l = (float)(sl / W);
  const float tx = (float)(sx / W), ty = (float)(cyd + hd / 2.0), tz = (float)(sz / W), ry = (float)(ry_i + sd / W);
  lo[0] = h; lo[1] = w; lo[2] = l; lo[3] = tx; lo[4] = ty; lo[5] = tz; lo[6] = ry;
  detbox_corners(h, w, l, ry, tx, ty - h / 2.0f, tz, ko);      // from the rounded label
}

}  // namespace

extern "C" int t3d_detect_fuse(const t3d_detect_fuse_args* a, t3d_stream_t stream) {
  T3D_ABI_TAKE(detect_fuse_args, a);
  bool empty;
  if (const int refused = nms_lists_gate(a, a && a->vote_threshold >= 0.f && a->vote_threshold <= 1.f, &empty)) return refused;      // (a NaN fails both)
  if (empty) return T3D_OK;
  if (!a->group_offsets || !a->members || !a->keep || !a->suppressed_by || !a->rank || !a->label || !a->corners || !a->weight ||
      !a->workspace || !a->label_out || !a->corners_out || !a->n_votes)
    return T3D_ERR_ARG;
  if (a->workspace_bytes < T3D_DETECT_FUSE_WORKSPACE_BYTES(a->n) || (reinterpret_cast<uintptr_t>(a->workspace) & 7u)) return T3D_ERR_ARG;
  FuseVote* vote;
  int32_t* order = nms_carve(a->workspace, a->n, &vote);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int blocks = (a->n + FUSE_THREADS - 1) / FUSE_THREADS;
  T3D_LAUNCH(k_fuse_votes, dim3(blocks), dim3(FUSE_THREADS), 0, st, *a, order, vote);
  T3D_CHECK_LAUNCH();
  T3D_LAUNCH(k_fuse, dim3(blocks), dim3(FUSE_THREADS), 0, st, *a, order, vote);
  T3D_CHECK_LAUNCH();
  return T3D_OK;
}
