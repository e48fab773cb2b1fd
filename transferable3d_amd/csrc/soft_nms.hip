// Soft-NMS of decoded 3-D boxes over many small independent groups (t3d.h t3d_detect_soft_nms; Bodla et al., ICCV 2017): a box that
// overlaps a better one is not dropped, its confidence is multiplied down by a function of the IoU.  The groups, the metrics and the IoU
// are those of t3d_detect_nms (nms.hip); the rule is written out in t3d.h.
//
// Unlike the hard suppression, the order of a group is not known up front -- every selection changes the scores the next one ranks by --
// so there is no sort and no bit matrix: one kernel selects and decays, step by step.
//   k_soft_nms<LPG>   a group has LPG lanes (the power of two >= max_group / 4, at most 64; NMS_THREADS / LPG groups per workgroup) and a
//                     lane owns the boxes at list positions lane, lane + LPG, ... of its group: up to 4 when max_group <= 256, at most
//                     T3D_DETECT_NMS_MAX_GROUP / 64 = 16.  (One box per lane left two lanes in three idle on groups of 1 to 40 and took
//                     4.09 ms where this takes 3.19 ms: docs/EXPERIMENTS.md.)  Their live bits are a register; the working scores live in score_out, which only
//                     the owning lane reads and writes.  The groups of a wave walk their selections in lockstep, as k_nms_sweep walks
//                     its ranks: the step count is made wave-uniform first and nothing leaves an iteration early, because the shuffles
//                     need every lane.  Per step each lane finds its best live box, a butterfly of __shfl_xor over the LPG lanes finds
//                     the group's (score descending, box index ascending), every lane reads the winner's corners (one address: a
//                     broadcast) and decays and prunes its own live boxes.
// Every live pair of a group costs one IoU, (selected, live) -- at most the pairs above the diagonal that k_nms_pairs computes, fewer
// where boxes are pruned -- except the pairs whose centres lie too far apart to touch: their IoU is 0 and the polygon clipping is skipped
// (in a group of 1024 boxes of 256 objects nearly all of them).
// No workspace, no LDS, no atomics, no dependence on the grid: a group's outputs are a function of its own boxes.
#include "detbox_dev.h"
#include "nms_dev.h"

namespace {

constexpr int SOFT_OWN = 4;                 // boxes per lane up to which a group gets fewer than 64 lanes (the launcher)
constexpr int SOFT_NONE = 0x7fffffff;      // "no live box" in a (score, box, position) triple: it loses against every box

// (s, box, pos) comes before (s2, box2, pos2): score descending, box index ascending; the list position decides between two entries of one
// box (lists that break the contract), so that every lane of a group names the same winner
__device__ __forceinline__ bool soft_before(float s, int box, int pos, float s2, int box2, int pos2) {
  return s > s2 || (s == s2 && (box < box2 || (box == box2 && pos < pos2)));
}

template <int LPG>
__global__ __launch_bounds__(NMS_THREADS) void k_soft_nms(const t3d_detect_soft_nms_args a) {
  constexpr int GPB = NMS_THREADS / LPG;        // groups per workgroup
  const int gi = blockIdx.x * GPB + threadIdx.x / LPG, l = threadIdx.x % LPG;
  const NmsGroup g = nms_group_at(a, gi);       // (a group that breaks the contract is not visited)
  const int first = g.first, size = max(g.size, 0);
  const int own = size > l ? (size - l + LPG - 1) / LPG : 0;      // this lane's positions l + k LPG, k < own (<= 16: size <= 1024)
  unsigned live = 0;
  const uint32_t* score_bits = reinterpret_cast<const uint32_t*>(a.score);
  for (int k = 0; k < own; ++k) {
    const int box = a.members[first + l + k * LPG];
    if (!nms_box_ok(a, box)) continue;
    const uint32_t bits = score_bits[box];
    const float s = __uint_as_float(bits);
    reinterpret_cast<uint32_t*>(a.score_out)[box] = bits;
    a.n_decays[box] = 0;
    if (s > 0.f && s < __builtin_inff()) {       // (a NaN compares false)
      live |= 1u << k;
    } else {                                      // takes no part
      a.keep[box] = 1;
      a.suppressed_by[box] = -1;
    }
  }
  const int steps = nms_wave_steps(size);
  for (int st = 0; st < steps; ++st) {           // (a selection takes one live box out of its group: `steps` selections empty every group)
    if (!__any(live != 0)) break;                // the same answer in every lane of the wave
    float bs = -1.f;
    int bb = SOFT_NONE, bp = SOFT_NONE;
    for (int k = 0; k < own; ++k) {
      if (!((live >> k) & 1u)) continue;
      const int pos = l + k * LPG, box = a.members[first + pos];
      const float s = a.score_out[box];
      if (soft_before(s, box, pos, bs, bb, bp)) { bs = s; bb = box; bp = pos; }
    }
#pragma unroll
    for (int o = LPG / 2; o > 0; o >>= 1) {      // every lane of the wave is here
      const float s2 = __shfl_xor(bs, o, LPG);
      const int b2 = __shfl_xor(bb, o, LPG), p2 = __shfl_xor(bp, o, LPG);
      if (soft_before(s2, b2, p2, bs, bb, bp)) { bs = s2; bb = b2; bp = p2; }
    }
    if (bp != SOFT_NONE) {                        // (the same in every lane of the group)
      if (bp % LPG == l) {                        // the owner: the box is selected with the working score score_out holds
        live &= ~(1u << (bp / LPG));
        a.keep[bb] = 1;
        a.suppressed_by[bb] = -1;
      }
      if (live != 0) {
        float k1[24];
#pragma unroll
        for (int i = 0; i < 24; ++i) k1[i] = a.corners[(size_t)bb * 24 + i];
        // corners 0 and 6 are opposite: their midpoint is the centre, half their distance the half diagonal
        const float cx = 0.5f * (k1[0] + k1[18]), cy = 0.5f * (k1[1] + k1[19]), cz = 0.5f * (k1[2] + k1[20]);
        const float dx1 = k1[0] - k1[18], dy1 = k1[1] - k1[19], dz1 = k1[2] - k1[20];
        const float h1 = 0.5f * sqrtf(dx1 * dx1 + dy1 * dy1 + dz1 * dz1);
        // Both boxes go to the IoU with the selected box's first corner as the origin of the ground plane.  box3d_iou_corners takes the
        // two rectangle areas by the shoelace formula on the coordinates as they come, which loses digits far from the origin (6e-5
        // of the area at x = 42); the differences below are exact or within half an ulp of a small number.
        const float ox = k1[0], oz = k1[2];
#pragma unroll
        for (int i = 0; i < 8; ++i) { k1[3 * i] -= ox; k1[3 * i + 2] -= oz; }
        for (int k = 0; k < own; ++k) {
          if (!((live >> k) & 1u)) continue;
          const int box = a.members[first + l + k * LPG];
          const float* k2 = a.corners + (size_t)box * 24;
          const float ex = k2[0] - k2[18], ey = k2[1] - k2[19], ez = k2[2] - k2[20];
          const float h2 = 0.5f * sqrtf(ex * ex + ey * ey + ez * ez);
          const float gx = 0.5f * (k2[0] + k2[18]) - cx, gy = 0.5f * (k2[1] + k2[19]) - cy, gz = 0.5f * (k2[2] + k2[20]) - cz;
          // too far apart to touch, with room for the rounding of both sides: IoU 0, which decays nothing under either method
          // (a NaN on either side compares false and goes on to the IoU)
          if (sqrtf(gx * gx + gy * gy + gz * gz) > (h1 + h2) * 1.0001f + 1e-6f) continue;
          float k2s[24];
#pragma unroll
          for (int i = 0; i < 8; ++i) { k2s[3 * i] = k2[3 * i] - ox; k2s[3 * i + 1] = k2[3 * i + 1]; k2s[3 * i + 2] = k2[3 * i + 2] - oz; }
          const float iou = iou_by_metric(k1, k2s, a.metric);
          float factor = 1.f;
          bool decay = false;
          if (a.method == T3D_SOFT_NMS_GAUSSIAN) {
            if (iou > 0.f) { factor = expf(-(iou * iou) / a.sigma); decay = true; }      // a NaN compares false
          } else if (iou > a.threshold) {
            factor = 1.f - iou;
            decay = true;
          }
          if (decay) {
            const float s = a.score_out[box] * factor;
            a.score_out[box] = s;
            a.n_decays[box] += 1;
            if (s < a.min_score) {
              live &= ~(1u << k);
              a.keep[box] = 0;
              a.suppressed_by[box] = bb;
            }
          }
        }
      }
    }
  }
}

bool soft_options_ok(const t3d_detect_soft_nms_args& a) {
  if (a.method != T3D_SOFT_NMS_GAUSSIAN && a.method != T3D_SOFT_NMS_LINEAR) return false;
  if (a.method == T3D_SOFT_NMS_GAUSSIAN && !(a.sigma > 0.f && a.sigma < __builtin_inff())) return false;
  return a.min_score >= 0.f;      // (false for a NaN)
}

}  // namespace

extern "C" int t3d_detect_soft_nms(const t3d_detect_soft_nms_args* a, t3d_stream_t stream) {
  T3D_ABI_TAKE(detect_soft_nms_args, a);
  bool empty;
  if (const int refused = nms_lists_gate(a, a && soft_options_ok(*a), &empty)) return refused;
  if (empty) return T3D_OK;
  if (!a->corners || !a->score || !a->group_offsets || !a->members || !a->score_out || !a->keep || !a->suppressed_by || !a->n_decays)
    return T3D_ERR_ARG;
  const uint64_t need = T3D_DETECT_SOFT_NMS_WORKSPACE_BYTES(a->n, a->max_group);
  if (a->workspace_bytes < need || (need > 0 && (!a->workspace || (reinterpret_cast<uintptr_t>(a->workspace) & 7u)))) return T3D_ERR_ARG;
  hipStream_t st = static_cast<hipStream_t>(stream);
  // a lane of a small group owns up to SOFT_OWN boxes
  nms_for_lanes<64>((a->max_group + SOFT_OWN - 1) / SOFT_OWN, a->n_groups, [&](auto lpg, int group_blocks) {
    T3D_LAUNCH(k_soft_nms<decltype(lpg)::value>, dim3(group_blocks), dim3(NMS_THREADS), 0, st, *a);
  });
  T3D_CHECK_LAUNCH();
  return T3D_OK;
}
