// Detection decode of one inference batch (t3d.h t3d_detect_decode), in place of the reference's per-batch host post-processing
// (sunrgbd/sunrgbd_detection/test_semisup.py:236-262: two-way softmax, masked mean, two more softmaxes, arg-max decode) and its
// per-detection loops (roi_seg_box3d_dataset.py from_prediction_to_label_format 461-466, get_3d_box 86-101).  One launch, one workgroup
// per frustum:
//   all four waves   the [N, 2] logits as coalesced float2: hard mask, count, sum of the foreground probabilities (a sigmoid of the
//                    logit difference); every thread in point order, 64 lanes by shuffles, the four partials through LDS in index order;
//   wave 0           the 12-way and 10-way soft-max / arg-max over lanes, the score, the decoded box, its label-format row; lanes 0-7 one
//                    corner each.
// No atomics, nothing depends on the grid: a frustum's outputs are a function of its own inputs only.
#include "common.h"
#include "detbox_dev.h"

// the host code this replaces is NumPy, elementwise: no fused multiply-adds, so that the same inputs round the same way whatever the
// surrounding code looks like to the optimiser
#pragma clang fp contract(off)

namespace {

constexpr int DD_THREADS = 256;
constexpr int DD_NH = 12;       // heading bins
constexpr int DD_NS = 10;       // size clusters
constexpr int DD_BOX = 3 + 2 * DD_NH + 4 * DD_NS;      // 67

__device__ const float kMeanDet[10][3] = {   // class2type order (roi_seg_box3d_dataset.py:18-31): l, w, h
    {2.114256f, 1.620300f, 0.927272f}, {0.791118f, 1.279516f, 0.718182f}, {0.923508f, 1.867419f, 0.845495f},
    {0.591958f, 0.552978f, 0.827272f}, {0.699104f, 0.454178f, 0.756250f}, {0.695190f, 1.346299f, 0.736364f},
    {0.528526f, 1.002642f, 1.172878f}, {0.500618f, 0.632163f, 0.683424f}, {0.404671f, 1.071108f, 1.688889f},
    {0.765840f, 1.398258f, 0.472728f}};

__device__ __forceinline__ float dd_wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}

// np.argmax over the first n lanes: the first NaN if there is one, else the lowest lane that holds the maximum.  Always in [0, n).
__device__ __forceinline__ int dd_argmax(float v, float vmax, int lane, int n) {
  const bool in = lane < n;
  unsigned long long m = __ballot(in && v != v);
  if (m == 0) m = __ballot(in && v == vmax);
  return m ? __ffsll((long long)m) - 1 : 0;
}

__global__ __launch_bounds__(DD_THREADS) void k_detect_decode(const t3d_detect_decode_args p) {
  const int b = blockIdx.x;                  // the grid is min(B, n_valid)
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  __shared__ float part_sum[DD_THREADS / 64];
  __shared__ int part_cnt[DD_THREADS / 64];

  const float2* lg = reinterpret_cast<const float2*>(p.logits) + (size_t)b * p.N;
  uint8_t* seg = p.seg ? p.seg + (size_t)b * p.N : nullptr;
  float sum = 0.f;
  int cnt = 0;
  for (int n = t; n < p.N; n += DD_THREADS) {
    const float2 l = lg[n];
    const bool fg = l.y > l.x;
    if (fg) {
      sum += 1.0f / (1.0f + expf(l.x - l.y));      // softmax(l)[1]
      ++cnt;
    }
    if (seg) seg[n] = fg ? 1 : 0;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    sum += __shfl_down(sum, o, 64);
    cnt += __shfl_down(cnt, o, 64);
  }
  if (lane == 0) {
    part_sum[wv] = sum;
    part_cnt[wv] = cnt;
  }
  __syncthreads();
  if (wv != 0) return;

  const float msum = ((part_sum[0] + part_sum[1]) + part_sum[2]) + part_sum[3];
  const int mcnt = part_cnt[0] + part_cnt[1] + part_cnt[2] + part_cnt[3];
  const float mask_mean_prob = msum / (float)(mcnt + 1);

  const float* bo = p.box_out + (size_t)b * p.ld_box;
  const float ninf = -__builtin_inff();
  const float hv = lane < DD_NH ? bo[3 + lane] : ninf;
  const float sv = lane < DD_NS ? bo[3 + 2 * DD_NH + lane] : ninf;
  const float hmax = dd_wave_max(hv), smax = dd_wave_max(sv);
  const int hcls = dd_argmax(hv, hmax, lane, DD_NH);
  const int scls = dd_argmax(sv, smax, lane, DD_NS);
  const float hsum = wave_sum(lane < DD_NH ? expf(hv - hmax) : 0.f);      // the largest soft-max term is exp(0) / sum
  const float ssum = wave_sum(lane < DD_NS ? expf(sv - smax) : 0.f);
  float score = logf(mask_mean_prob + 0.01f) + logf(1.0f / hsum + 0.01f) + logf(1.0f / ssum + 0.01f);
  if (p.fit_prob) score += logf(p.fit_prob[b] + 0.01f);

  const float* td = p.total_delta ? p.total_delta + (size_t)b * 7 : nullptr;
  const float* s1 = p.stage1_center + (size_t)b * 3;
  const float dl[7] = {td ? td[0] : 0.f, td ? td[1] : 0.f, td ? td[2] : 0.f, td ? td[3] : 0.f, td ? td[4] : 0.f, td ? td[5] : 0.f,
                       td ? td[6] : 0.f};
  const float cx = (bo[0] + s1[0]) - dl[0], cy = (bo[1] + s1[1]) - dl[1], cz = (bo[2] + s1[2]) - dl[2];
  const float PI = 3.14159265358979323846f;
  const float hres = bo[3 + DD_NH + hcls] * (float)(3.14159265358979323846 / DD_NH) - dl[6];
  const float* srn = bo + 3 + 2 * DD_NH + DD_NS + 3 * scls;
  const float sr0 = srn[0] * kMeanDet[scls][0] - dl[3];
  const float sr1 = srn[1] * kMeanDet[scls][1] - dl[4];
  const float sr2 = srn[2] * kMeanDet[scls][2] - dl[5];
  const float l = kMeanDet[scls][0] + sr0, w = kMeanDet[scls][1] + sr1, h = kMeanDet[scls][2] + sr2;
  const float rot = p.rot_angle ? p.rot_angle[b] : 0.f;
  float ry = (float)hcls * (float)(2.0 * 3.14159265358979323846 / DD_NH) + hres;
  if (ry > PI) ry -= 2.0f * PI;
  ry += rot;
  const float c = cosf(-rot), s = sinf(-rot);             // rotate_pc_along_y(center, -rot_angle)
  const float tx = c * cx - s * cz, ty = cy + h / 2.0f, tz = s * cx + c * cz;

  if (lane == 0) {
    p.score[b] = score;
    p.mask_count[b] = mcnt;
    p.heading_cls[b] = hcls;
    p.size_cls[b] = scls;
    float* o = p.center + (size_t)b * 3;
    o[0] = cx; o[1] = cy; o[2] = cz;
    p.heading_res[b] = hres;
    o = p.size_res + (size_t)b * 3;
    o[0] = sr0; o[1] = sr1; o[2] = sr2;
    o = p.label + (size_t)b * 7;
    o[0] = h; o[1] = w; o[2] = l; o[3] = tx; o[4] = ty; o[5] = tz; o[6] = ry;
  }
  if (lane < 8)          // get_3d_box((l, w, h), ry, (tx, ty - h/2, tz))
    detbox_corner(h, w, l, cosf(ry), sinf(ry), tx, ty - h / 2.0f, tz, lane, p.corners + ((size_t)b * 8 + lane) * 3);
}

}  // namespace

extern "C" int t3d_detect_decode(const t3d_detect_decode_args* a, t3d_stream_t stream) {
  T3D_ABI_TAKE(detect_decode_args, a);
  if (!a) return T3D_ERR_ARG;
  if (a->B <= 0 || a->N <= 0 || a->n_valid < 0 || a->ld_box < DD_BOX) return T3D_ERR_SHAPE;
  if (!a->logits || !a->box_out || !a->stage1_center || !a->score || !a->mask_count || !a->heading_cls || !a->size_cls || !a->center ||
      !a->heading_res || !a->size_res || !a->label || !a->corners)
    return T3D_ERR_ARG;
  if (reinterpret_cast<uintptr_t>(a->logits) & 7u) return T3D_ERR_ARG;      // read as float2
  const int n = a->n_valid < a->B ? a->n_valid : a->B;
  if (n == 0) return T3D_OK;
  T3D_LAUNCH(k_detect_decode, dim3(n), dim3(DD_THREADS), 0, static_cast<hipStream_t>(stream), *a);
  T3D_CHECK_LAUNCH();
  return T3D_OK;
}
