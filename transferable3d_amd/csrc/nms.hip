// Greedy non-maximum suppression of decoded 3-D boxes over many small independent groups (t3d.h t3d_detect_nms): one group is the boxes
// of one class in one image.  The reference has no such step (test_semisup.py writes one box per 2-D detection); it is opt-in.
//
// Real groups are a handful of boxes and there are tens of thousands of them, so nothing here is laid out per group.  The first two
// kernels run one thread per POSITION of the concatenated member lists (a wave covers 64 consecutive positions = several whole groups;
// a thread finds its group by a binary search of group_offsets); the sweep gives a group as many lanes as its bit rows have words:
//   k_nms_order      (nms_pairs_dev.h) position p of group g: the rank of its box by counting; order[first(g) + rank] = box;
//   k_nms_pairs<1>   (nms_pairs_dev.h) (sorted position s of g, word w): bit c of mask[first(g) + s][w] = IoU(box at s, box at 64 w + c) >
//                    threshold, for the columns 64 w + c > s only;
//   k_nms_sweep      LPG = ceil(max_group / 64) rounded up to a power of two lanes per group, lane w holds word w of the group's
//                    "removed" set in a register; the 64 / LPG groups of a wave walk their ranks in lockstep.  A kept row's words are
//                    OR-ed in, the bits that are new name the boxes it suppresses.
// No atomics, no LDS, no dependence on the grid: a group's outputs are a function of its own boxes.
// The first two kernels are shared with the sweep over many configurations (nms_sweep.hip); the lists, the lockstep walk and the
// launchers' common gate are in nms_dev.h.
#include "nms_pairs_dev.h"

namespace {

template <int LPG>      // lanes per group: a power of two, >= W
__global__ __launch_bounds__(NMS_THREADS) void k_nms_sweep(const t3d_detect_nms_args a, const int32_t* order, const unsigned long long* mask,
                                                            int W) {
  constexpr int GPB = NMS_THREADS / LPG;        // groups per workgroup
  const int gi = blockIdx.x * GPB + threadIdx.x / LPG, w = threadIdx.x % LPG;
  const NmsGroup g = nms_group_at(a, gi);       // (a group that breaks the contract is not visited)
  const int first = g.first, size = max(g.size, 0);
  const int steps = nms_wave_steps(size);
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
        const unsigned long long m = mask[(size_t)(first + s) * W + w] & nms_cols(size - 64 * w);
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
  bool empty;
  if (const int refused = nms_lists_gate(a, true, &empty)) return refused;
  if (empty) return T3D_OK;
  if (!a->corners || !a->score || !a->group_offsets || !a->members || !a->keep || !a->suppressed_by || !a->workspace) return T3D_ERR_ARG;
  if (a->workspace_bytes < T3D_DETECT_NMS_WORKSPACE_BYTES(a->n, a->max_group) || (reinterpret_cast<uintptr_t>(a->workspace) & 7u))
    return T3D_ERR_ARG;
  const int W = (a->max_group + 63) / 64;
  unsigned long long* mask;
  int32_t* order = nms_carve(a->workspace, a->n, &mask);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int blocks = (a->n + NMS_THREADS - 1) / NMS_THREADS;
  T3D_LAUNCH(k_nms_order, dim3(blocks), dim3(NMS_THREADS), 0, st, *a, order);
  T3D_CHECK_LAUNCH();
  NmsThresholds th = {};
  th.t[0] = a->threshold;
  T3D_LAUNCH(k_nms_pairs<1>, dim3(blocks, W), dim3(NMS_THREADS), 0, st, *a, order, mask, W, 1, th);
  T3D_CHECK_LAUNCH();
  nms_for_lanes<16>(W, a->n_groups, [&](auto lpg, int group_blocks) {
    T3D_LAUNCH(k_nms_sweep<decltype(lpg)::value>, dim3(group_blocks), dim3(NMS_THREADS), 0, st, *a, order, mask, W);
  });
  T3D_CHECK_LAUNCH();
  return T3D_OK;
}
