// Greedy non-maximum suppression of decoded 3-D boxes over many small independent groups (t3d.h t3d_detect_nms): one group is the boxes
// of one class in one image.  The reference has no such step (test_semisup.py writes one box per 2-D detection); it is opt-in.
//
// Real groups are a handful of boxes and there are tens of thousands of them, so nothing here is laid out per group.  The first two
// kernels run one thread per POSITION of the concatenated member lists (a wave covers 64 consecutive positions = several whole groups;
// a thread finds its group by a binary search of group_offsets); the sweep gives a group as many lanes as its bit rows have words:
//   k_nms_order   position p of group g: the rank of its box by counting the boxes of g that come before it (size^2 comparisons per
//                 group, as k_order of sunrgbd_eval.hip); order[first(g) + rank] = box;
//   k_nms_pairs   (sorted position s of g, word w): bit c of mask[first(g) + s][w] = IoU(box at s, box at 64 w + c) > threshold, for the
//                 columns 64 w + c > s only; words wholly below the diagonal are neither computed nor written (nor read by the sweep).
//                 blockIdx.y is w: the lanes of a wave walk the same columns of the same few groups, the column loads are broadcasts;
//   k_nms_sweep   LPG = ceil(max_group / 64) rounded up to a power of two lanes per group, lane w holds word w of the group's "removed"
//                 set in a register; the 64 / LPG groups of a wave walk their ranks in lockstep.  A kept row's words are OR-ed in, the
//                 bits that are new name the boxes it suppresses.
// Rows are W = ceil(max_group / 64) words apart, whatever the group's own size: a row's address needs no per-group prefix sum.
// No atomics, no LDS, no dependence on the grid: a group's outputs are a function of its own boxes.
// nms_group_of, nms_key and k_nms_order are in nms_dev.h, which the sweep over many configurations (nms_sweep.hip) shares.
#include "common.h"
#include "boxgeom_dev.h"
#include "nms_dev.h"

namespace {

__global__ __launch_bounds__(NMS_THREADS) void k_nms_pairs(const t3d_detect_nms_args a, const int32_t* order, unsigned long long* mask,
                                                            int W) {
  const int p = blockIdx.x * NMS_THREADS + threadIdx.x, w = blockIdx.y;
  if (p >= a.n) return;
  const NmsGroup g = nms_group_of(a, p);
  if (g.size < 0) return;
  const int s = p - g.first;                    // this row's sorted position
  const int c0 = max(s + 1, 64 * w), c1 = min(g.size, 64 * w + 64);
  if (64 * w + 63 < s || 64 * w >= g.size) return;       // wholly below the diagonal, or past the group: never read
  unsigned long long bits = 0;
  const int row = order[p];
  if (nms_box_ok(a, row)) {
    float k1[24];
#pragma unroll
    for (int i = 0; i < 24; ++i) k1[i] = a.corners[(size_t)row * 24 + i];
    for (int c = c0; c < c1; ++c) {
      const int col = order[g.first + c];
      if (!nms_box_ok(a, col)) continue;
      float iou2d;
      const float iou3d = boxgeom::box3d_iou_corners(k1, a.corners + (size_t)col * 24, &iou2d);
      const float iou = a.metric == T3D_NMS_IOU2D ? iou2d : iou3d;
      if (iou > a.threshold) bits |= 1ull << (c - 64 * w);      // a NaN compares false
    }
  }
  mask[(size_t)p * W + w] = bits;
}

template <int LPG>      // lanes per group: a power of two, >= W
__global__ __launch_bounds__(NMS_THREADS) void k_nms_sweep(const t3d_detect_nms_args a, const int32_t* order, const unsigned long long* mask,
                                                            int W) {
  constexpr int GPB = NMS_THREADS / LPG;        // groups per workgroup
  const int gi = blockIdx.x * GPB + threadIdx.x / LPG, w = threadIdx.x % LPG;
  int first = 0, size = 0;
  if (gi < a.n_groups) {
    const int f = a.group_offsets[gi], e = a.group_offsets[gi + 1];
    if (f >= 0 && e >= f && e <= a.n && e - f <= a.max_group) { first = f; size = e - f; }
  }
  int steps = size;                              // the groups of a wave walk in lockstep: the shuffles below need every lane
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) steps = max(steps, __shfl_xor(steps, o, 64));
  const bool has_word = 64 * w < size;           // (implies w < W)
  unsigned long long removed = 0;
  for (int s = 0; s < steps; ++s) {
    const int sw = s >> 6;
    // the word of `removed` that holds bit s, from the lane that owns it (every lane of the wave is here: `steps` is wave-uniform and
    // nothing below leaves the iteration early)
    const unsigned long long owner = LPG == 1 ? removed : __shfl(removed, sw, LPG);
    const bool kept = s < size && !((owner >> (s & 63)) & 1ull);
    if (kept) {
      const int box = order[first + s];
      if (w == sw && nms_box_ok(a, box)) {
        a.keep[box] = 1;
        a.suppressed_by[box] = -1;
      }
      if (has_word && w >= sw) {
        // (only columns of the group: a row that k_nms_pairs did not write, under lists that break the contract, names no box outside)
        const unsigned long long cols = size - 64 * w >= 64 ? ~0ull : (1ull << (size - 64 * w)) - 1ull;
        const unsigned long long m = mask[(size_t)(first + s) * W + w] & cols;
        unsigned long long fresh = m & ~removed;
        removed |= m;
        while (fresh) {
          const int c = __ffsll((long long)fresh) - 1;
          fresh &= fresh - 1;
          const int victim = order[first + 64 * w + c];
          if (nms_box_ok(a, victim)) {
            a.keep[victim] = 0;
            a.suppressed_by[victim] = box;
          }
        }
      }
    }
  }
}

}  // namespace

extern "C" int t3d_detect_nms(const t3d_detect_nms_args* a, t3d_stream_t stream) {
  T3D_ABI_TAKE(detect_nms_args, a);
  if (!a) return T3D_ERR_ARG;
  if (a->n < 0 || a->n_groups < 0 || a->max_group < 0) return T3D_ERR_ARG;
  if (a->metric != T3D_NMS_IOU3D && a->metric != T3D_NMS_IOU2D) return T3D_ERR_ARG;
  if (a->max_group > T3D_DETECT_NMS_MAX_GROUP) return T3D_ERR_SHAPE;
  if (a->n == 0 || a->n_groups == 0 || a->max_group == 0) return T3D_OK;
  if (!a->corners || !a->score || !a->group_offsets || !a->members || !a->keep || !a->suppressed_by || !a->workspace) return T3D_ERR_ARG;
  if (a->workspace_bytes < T3D_DETECT_NMS_WORKSPACE_BYTES(a->n, a->max_group) || (reinterpret_cast<uintptr_t>(a->workspace) & 7u))
    return T3D_ERR_ARG;
  const int W = (a->max_group + 63) / 64;
  int32_t* order = static_cast<int32_t*>(a->workspace);
  unsigned long long* mask = reinterpret_cast<unsigned long long*>(static_cast<char*>(a->workspace) + ((uint64_t)a->n + 1) / 2 * 8);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int blocks = (a->n + NMS_THREADS - 1) / NMS_THREADS;
  T3D_LAUNCH(k_nms_order, dim3(blocks), dim3(NMS_THREADS), 0, st, *a, order);
  T3D_CHECK_LAUNCH();
  T3D_LAUNCH(k_nms_pairs, dim3(blocks, W), dim3(NMS_THREADS), 0, st, *a, order, mask, W);
  T3D_CHECK_LAUNCH();
#define NMS_SWEEP(LPG)                                                                                                          \
  T3D_LAUNCH(k_nms_sweep<LPG>, dim3((a->n_groups + NMS_THREADS / LPG - 1) / (NMS_THREADS / LPG)), dim3(NMS_THREADS), 0, st, *a, order, \
             mask, W)
  if (W <= 1) NMS_SWEEP(1);
  else if (W <= 2) NMS_SWEEP(2);
  else if (W <= 4) NMS_SWEEP(4);
  else if (W <= 8) NMS_SWEEP(8);
  else NMS_SWEEP(16);
#undef NMS_SWEEP
  T3D_CHECK_LAUNCH();
  return T3D_OK;
}
