// Test-time augmentation behind t3d_detect_decode (t3d.h t3d_detect_ensemble): the V decoded boxes of every detection -> how well they
// agree, and their weighted mean around the view that agrees best with the others.  The reference has no such step; it is opt-in.  The
// semantics are stated in t3d.h and executed in fp64 NumPy by tests/fake_ensemble.py.
//
// As in fuse.hip the IoUs are computed where every lane has one to compute, the sums where they have to be in order:
//   k_ensemble_pairs   one thread per (detection, pair u < v), detection-major, so a wave covers the pairs of several detections: it
//                      brings both views back from their mirror, builds both corner sets relative to box u and writes one IoU (0 for
//                      a NaN, and where a view is not valid);
//   k_ensemble         one thread per detection: reads its V(V-1)/2 IoUs, picks the medoid, takes the votes in ascending view order
//                      and writes the six outputs.
// Every loop over views runs to the compile-time maximum under a `v < V` guard, so that the view labels and the IoUs are indexed
// statically and stay in registers.  No atomics, no LDS, no dependence on the grid: a detection's outputs are a function of its own rows.
#include "common.h"
#include "detbox_dev.h"

#pragma clang fp contract(off)

namespace {

constexpr int ENS_THREADS = 256;
constexpr int ENS_MAXV = T3D_DETECT_ENSEMBLE_MAX_VIEWS;

struct EnsLabel { float h, w, l, tx, ty, tz, ry; };

__device__ __forceinline__ bool ens_label_ok(const EnsLabel& b) {
  return detbox_finite((double)b.h) && detbox_finite((double)b.w) && detbox_finite((double)b.l) && detbox_finite((double)b.tx) &&
         detbox_finite((double)b.ty) && detbox_finite((double)b.tz) && detbox_finite((double)b.ry);
}

// The view label of t3d.h: row i of `label`, mirrored back where the view was assembled mirrored (c, s: cos and sin of rot_angle[i]).
__device__ __forceinline__ EnsLabel ens_view_label(const float* label, size_t i, bool flipped, double a, double c, double s) {
  const float* p = label + i * 7;
  EnsLabel b = {p[0], p[1], p[2], p[3], p[4], p[5], p[6]};
  if (flipped) {
    const double PI = 3.14159265358979323846;
    const double tx = (double)b.tx, tz = (double)b.tz;
    const double xc = tx * c - tz * s, zc = tx * s + tz * c;
    b.tx = (float)(-xc * c + zc * s);
    b.tz = (float)(xc * s + zc * c);
    b.ry = (float)detbox_wrap((PI - (double)b.ry) + 2.0 * a);
  }
  return b;
}

// detbox_corners of a label whose centre is (tx, yc, tz)
__device__ __forceinline__ void ens_corners(const EnsLabel& b, float tx, float yc, float tz, float* k) {
  detbox_corners(b.h, b.w, b.l, b.ry, tx, yc, tz, k);
}

__global__ __launch_bounds__(ENS_THREADS) void k_ensemble_pairs(const t3d_detect_ensemble_args a, float* iou_out, int P) {
  const int64_t t = (int64_t)blockIdx.x * ENS_THREADS + threadIdx.x;
  if (t >= (int64_t)a.n * P) return;
  const size_t i = (size_t)(t / P);
  int rem = (int)(t - (int64_t)i * P), pu = 0;
  while (rem >= a.V - 1 - pu) { rem -= a.V - 1 - pu; ++pu; }      // pair `rem` of the lexicographic list -> (pu, pv)
  const int pv = pu + 1 + rem;
  const double ang = a.rot_angle ? (double)a.rot_angle[i] : 0.0;
  const double c = cos(ang), s = sin(ang);
  EnsLabel bu = {}, bv = {};
#pragma unroll
  for (int v = 0; v < ENS_MAXV; ++v) {                            // (label[] lives in the kernel arguments: a static index)
    if (v == pu) bu = ens_view_label(a.label[v], i, (a.flip_mask >> v) & 1u, ang, c, s);
    if (v == pv) bv = ens_view_label(a.label[v], i, (a.flip_mask >> v) & 1u, ang, c, s);
  }
  float iou = 0.f;
  if (ens_label_ok(bu) && ens_label_ok(bv)) {
    float k1[24], k2[24];
    ens_corners(bu, 0.f, 0.f, 0.f, k1);
    ens_corners(bv, bv.tx - bu.tx, (bv.ty - bv.h / 2.0f) - (bu.ty - bu.h / 2.0f), bv.tz - bu.tz, k2);
    iou = iou_by_metric(k1, k2, a.metric);
    iou = iou == iou ? iou : 0.f;                                 // (a NaN counts as 0)
  }
  iou_out[t] = iou;
}

__global__ __launch_bounds__(ENS_THREADS) void k_ensemble(const t3d_detect_ensemble_args a, const float* iou_in, int P) {
  const int64_t t = (int64_t)blockIdx.x * ENS_THREADS + threadIdx.x;
  if (t >= (int64_t)a.n) return;
  const size_t i = (size_t)t;
  const int V = a.V;
  const double ang = a.rot_angle ? (double)a.rot_angle[i] : 0.0;
  const double c = cos(ang), s = sin(ang);
  EnsLabel L[ENS_MAXV];
  bool ok[ENS_MAXV];
  int m = 0;
#pragma unroll
  for (int v = 0; v < ENS_MAXV; ++v) {
    L[v] = EnsLabel{};
    ok[v] = false;
    if (v < V) {
      L[v] = ens_view_label(a.label[v], i, (a.flip_mask >> v) & 1u, ang, c, s);
      ok[v] = ens_label_ok(L[v]);
      m += ok[v] ? 1 : 0;
    }
  }
  // the pair IoUs; per view the sum with the others (for a view x the pairs (u, x) come before the pairs (x, v): ascending order)
  float iou[ENS_MAXV * (ENS_MAXV - 1) / 2];
  double sum[ENS_MAXV];
#pragma unroll
  for (int v = 0; v < ENS_MAXV; ++v) sum[v] = 0.0;
  double total = 0.0;
  float lowest = 0.f;
  int pairs = 0;
  {
    const float* row = iou_in + i * (size_t)P;
    int p = 0, q = 0;                                             // p: position in this call's list of pairs, q: in the list of 8 views
#pragma unroll
    for (int u = 0; u < ENS_MAXV; ++u)
#pragma unroll
      for (int v = u + 1; v < ENS_MAXV; ++v, ++q) {
        iou[q] = 0.f;
        if (v < V) {                                              // (u < v < V)
          const float x = row[p++];
          if (ok[u] && ok[v]) {
            iou[q] = x;
            sum[u] = sum[u] + (double)x;
            sum[v] = sum[v] + (double)x;
            total = total + (double)x;
            lowest = pairs == 0 ? x : (x < lowest ? x : lowest);
            ++pairs;
          }
        }
      }
  }
  a.agreement[i] = pairs > 0 ? (float)(total / (double)pairs) : 0.f;
  a.min_iou[i] = pairs > 0 ? lowest : 0.f;
  // the medoid
  int anchor = -1;
  double best = 0.0;
#pragma unroll
  for (int v = 0; v < ENS_MAXV; ++v) {
    if (v < V && ok[v]) {
      const double mean = m > 1 ? sum[v] / (double)(m - 1) : 0.0;
      if (anchor < 0 || mean > best) { anchor = v; best = mean; }
    }
  }
  a.anchor[i] = anchor;
  float* lo = a.label_out + i * 7;
  float* ko = a.corners_out + i * 24;
  // the anchor's label and every view's IoU with it
  EnsLabel A = EnsLabel{};
  float ia[ENS_MAXV];
#pragma unroll
  for (int v = 0; v < ENS_MAXV; ++v) {
    ia[v] = -1.f;
    if (v == anchor) A = L[v];
  }
  {
    int q = 0;
#pragma unroll
    for (int u = 0; u < ENS_MAXV; ++u)
#pragma unroll
      for (int v = u + 1; v < ENS_MAXV; ++v, ++q) {
        if (u == anchor && ok[v]) ia[v] = iou[q];
        if (v == anchor && ok[u]) ia[u] = iou[q];
      }
  }
  const double h_a = A.h, ry_a = A.ry;
  double w_anchor = 0.0;
#pragma unroll
  for (int v = 0; v < ENS_MAXV; ++v)                              // (weight[] lives in the kernel arguments: a static index)
    if (v == anchor) w_anchor = detbox_weight(a.weight[v][i]);
  double W = w_anchor, sx = w_anchor * (double)A.tx, sy = w_anchor * ((double)A.ty - h_a / 2.0), sz = w_anchor * (double)A.tz;
  double sl = w_anchor * (double)A.l, sw = w_anchor * (double)A.w, sh = w_anchor * h_a, sd = 0.0;
  int votes = 0;
#pragma unroll
  for (int v = 0; v < ENS_MAXV; ++v) {
    if (v < V && v != anchor && anchor >= 0 && ok[v] && ia[v] > a.vote_threshold) {
      ++votes;
      const double PI = 3.14159265358979323846, HALF_PI = PI / 2.0;
      const double d = (double)L[v].ry - ry_a;
      double delta = 0.0;
      int kq = 0;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const double wr = detbox_wrap(d + (double)k * HALF_PI);
        if (k == 0 || fabs(wr) < fabs(delta)) { delta = wr; kq = k; }
      }
      const double h_v = L[v].h;
      const double l_v = (kq & 1) ? L[v].w : L[v].l, w_v = (kq & 1) ? L[v].l : L[v].w;      // (l and w exchanged for an odd quarter turn)
      const double wv = detbox_weight(a.weight[v][i]) * (double)ia[v];
      W = W + wv;
      sx = sx + wv * (double)L[v].tx;
      sy = sy + wv * ((double)L[v].ty - h_v / 2.0);
      sz = sz + wv * (double)L[v].tz;
      sl = sl + wv * l_v;
      sw = sw + wv * w_v;
      sh = sh + wv * h_v;
      sd = sd + wv * delta;
    }
  }
  a.n_votes[i] = votes;
  const bool fused = votes > 0 && W > 0.0 && detbox_finite(W);
  if (!fused && anchor <= 0) {                                    // view 0, or no valid view: byte copies
    const float* l0 = a.label[0] + i * 7;
#pragma unroll
    for (int k = 0; k < 7; ++k) lo[k] = l0[k];
#pragma unroll
    for (int k = 0; k < 24; ++k) ko[k] = a.corners0[i * 24 + k];
    return;
  }
  EnsLabel R = A;                                                 // another anchor, nothing fused: its view label
  if (fused) {
    const double hd = sh / W, cyd = sy / W;
    R.h = (float)hd; R.w = (float)(sw / W); R.l = (float)(sl / W);
    R.tx = (float)(sx / W); R.ty = (float)(cyd + hd / 2.0); R.tz = (float)(sz / W); R.ry = (float)(ry_a + sd / W);
  }
  lo[0] = R.h; lo[1] = R.w; lo[2] = R.l; lo[3] = R.tx; lo[4] = R.ty; lo[5] = R.tz; lo[6] = R.ry;
  ens_corners(R, R.tx, R.ty - R.h / 2.0f, R.tz, ko);
}

}  // namespace

extern "C" int t3d_detect_ensemble(const t3d_detect_ensemble_args* a, t3d_stream_t stream) {
  T3D_ABI_TAKE(detect_ensemble_args, a);
  if (!a) return T3D_ERR_ARG;
  if (a->n < 0 || a->V < 1) return T3D_ERR_ARG;
  if (a->V > T3D_DETECT_ENSEMBLE_MAX_VIEWS) return T3D_ERR_SHAPE;
  if (a->metric != T3D_NMS_IOU3D && a->metric != T3D_NMS_IOU2D) return T3D_ERR_ARG;
  if ((a->flip_mask & 1u) || (a->flip_mask >> a->V) != 0u) return T3D_ERR_ARG;
  if (!(a->vote_threshold >= 0.f && a->vote_threshold <= 1.f)) return T3D_ERR_ARG;      // (a NaN fails both)
  if (a->n == 0) return T3D_OK;
  for (int v = 0; v < a->V; ++v)
    if (!a->label[v] || !a->weight[v]) return T3D_ERR_ARG;
  if (!a->corners0 || !a->label_out || !a->corners_out || !a->agreement || !a->min_iou || !a->anchor || !a->n_votes) return T3D_ERR_ARG;
  const uint64_t need = T3D_DETECT_ENSEMBLE_WORKSPACE_BYTES(a->n, a->V);
  if (a->workspace_bytes < need || (need > 0 && !a->workspace) || (reinterpret_cast<uintptr_t>(a->workspace) & 7u)) return T3D_ERR_ARG;
  const int P = a->V * (a->V - 1) / 2;
  float* iou = static_cast<float*>(a->workspace);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int64_t pair_threads = (int64_t)a->n * P;
  if (pair_threads > 0) {
    if ((pair_threads + ENS_THREADS - 1) / ENS_THREADS > 0x7fffffffLL) return T3D_ERR_SHAPE;
    T3D_LAUNCH(k_ensemble_pairs, dim3((unsigned)((pair_threads + ENS_THREADS - 1) / ENS_THREADS)), dim3(ENS_THREADS), 0, st, *a, iou, P);
    T3D_CHECK_LAUNCH();
  }
  T3D_LAUNCH(k_ensemble, dim3((unsigned)((a->n + ENS_THREADS - 1) / ENS_THREADS)), dim3(ENS_THREADS), 0, st, *a, iou, P);
  T3D_CHECK_LAUNCH();
  return T3D_OK;
}
