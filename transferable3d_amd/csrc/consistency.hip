// Label-free consistency of decoded detections (t3d.h t3d_detect_consistency): how well a 3-D box reprojects onto the 2-D box it came
// from, and how well it sits on the points the network segmented.  One launch behind t3d_detect_decode, one workgroup per detection:
//   all four waves   the N points in fp64: the hard mask (as the decode's), the closed point-in-parallelepiped test against corner 0 and
//                    its three edges, three integer counts; 64 lanes by shuffles, the four partials through LDS;
//   wave 0           lanes 0-7 project one corner each (upright camera -> upright depth -> image, sunrgbd_data/utils.py); lane 0 folds the
//                    eight in corner order into the rectangle, clips it, and takes the IoU with the 2-D box.
// Integer sums only, no atomics: a detection's outputs are a function of its own inputs.
#include "common.h"

// the specification is NumPy, elementwise, fp64: every product and sum its own operation, so that equal inputs round the same way
#pragma clang fp contract(off)

namespace {

constexpr int DC_THREADS = 256;
constexpr int DC_CALIB = 20;      // Rtilt (9), K (9), image W, image H

__device__ __forceinline__ bool dc_finite(double v) { return v - v == 0.0; }

__global__ __launch_bounds__(DC_THREADS) void k_detect_consistency(const t3d_detect_consistency_args p) {
  const int b = blockIdx.x;                  // the grid is min(B, n_valid)
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  __shared__ int part[DC_THREADS / 64][3];
  __shared__ double proj[8][3];              // u, v, depth of the eight corners

  const float* kf = p.corners + (size_t)b * 24;
  const double k0x = (double)kf[0], k0y = (double)kf[1], k0z = (double)kf[2];
  double e[3][3], dd[3];
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const float* kj = kf + 3 * (j == 0 ? 1 : j == 1 ? 3 : 4);      // the edges to corners 1, 3, 4: w, l, h of get_3d_box
    e[j][0] = (double)kj[0] - k0x;
    e[j][1] = (double)kj[1] - k0y;
    e[j][2] = (double)kj[2] - k0z;
    dd[j] = (e[j][0] * e[j][0] + e[j][1] * e[j][1]) + e[j][2] * e[j][2];
  }
  const bool turned = p.rot_angle != nullptr;
  double c = 1.0, s = 0.0;
  if (turned) {
    const double rot = (double)p.rot_angle[b];
    sincos(-rot, &s, &c);
  }

  const float2* lg = reinterpret_cast<const float2*>(p.logits) + (size_t)b * p.N;
  const float* pts = p.xyz + (size_t)b * p.N * p.ld_xyz;
  int n_mask = 0, n_box = 0, n_both = 0;
#pragma unroll 1      // (unrolled, the fp64 loop body takes every register there is: 256 VGPRs and spills, against 70)
  for (int n = t; n < p.N; n += DC_THREADS) {
    const float2 l = lg[n];
    const bool fg = l.y > l.x;
    const float* pf = pts + (size_t)n * p.ld_xyz;
    const double x = (double)pf[0], y = (double)pf[1], z = (double)pf[2];
    double px = x, pz = z;
    if (turned) {
      px = c * x - s * z;
      pz = s * x + c * z;
    }
    const double q0 = px - k0x, q1 = y - k0y, q2 = pz - k0z;
    bool in = true;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const double dv = (q0 * e[j][0] + q1 * e[j][1]) + q2 * e[j][2];
      in = in && 0.0 <= dv && dv <= dd[j];      // a NaN fails both
    }
    n_mask += fg ? 1 : 0;
    n_box += in ? 1 : 0;
    n_both += (fg && in) ? 1 : 0;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    n_mask += __shfl_down(n_mask, o, 64);
    n_box += __shfl_down(n_box, o, 64);
    n_both += __shfl_down(n_both, o, 64);
  }
  if (lane == 0) {
    part[wv][0] = n_mask;
    part[wv][1] = n_box;
    part[wv][2] = n_both;
  }

  const int ci = p.calib_index[b];
  const bool calib_ok = ci >= 0 && ci < p.n_calib;
  const double* cal = p.calib + (size_t)(calib_ok ? ci : 0) * DC_CALIB;      // read only where calib_ok
  if (wv == 0 && lane < 8 && calib_ok) {
    const float* kc = kf + 3 * lane;
    const double X = (double)kc[0], Y = (double)kc[1], Z = (double)kc[2];
    const double d0 = X, d1 = Z, d2 = -Y;                                     // upright camera -> upright depth
    double tt[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) tt[i] = (cal[i] * d0 + cal[3 + i] * d1) + cal[6 + i] * d2;      // Rtilt^T d
    const double cam0 = tt[0], cam1 = -tt[2], cam2 = tt[1];
    double w[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) w[i] = (cal[9 + 3 * i] * cam0 + cal[10 + 3 * i] * cam1) + cal[11 + 3 * i] * cam2;
    proj[lane][0] = w[0] / w[2];
    proj[lane][1] = w[1] / w[2];
    proj[lane][2] = cam2;
  }
  __syncthreads();
  if (t != 0) return;

  n_mask = part[0][0] + part[1][0] + part[2][0] + part[3][0];
  n_box = part[0][1] + part[1][1] + part[2][1] + part[3][1];
  n_both = part[0][2] + part[1][2] + part[2][2] + part[3][2];
  int flags = (n_mask == 0 ? 2 : 0) | (calib_ok ? 0 : 4);
  double r[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
  if (calib_ok) {
    bool bad = false;
    double xmin = proj[0][0], ymin = proj[0][1], xmax = xmin, ymax = ymin;
    for (int k = 0; k < 8; ++k) {
      const double u = proj[k][0], v = proj[k][1];
      bad = bad || proj[k][2] <= 0.0 || !dc_finite(u) || !dc_finite(v);
      xmin = u < xmin ? u : xmin;
      xmax = u > xmax ? u : xmax;
      ymin = v < ymin ? v : ymin;
      ymax = v > ymax ? v : ymax;
    }
    if (bad) {
      flags |= 1;
    } else {
      const double W = cal[18], H = cal[19];
      if (W > 0.0 && H > 0.0) {
        const double xh = W - 1.0, yh = H - 1.0;
        xmin = xmin < 0.0 ? 0.0 : (xmin > xh ? xh : xmin);
        xmax = xmax < 0.0 ? 0.0 : (xmax > xh ? xh : xmax);
        ymin = ymin < 0.0 ? 0.0 : (ymin > yh ? yh : ymin);
        ymax = ymax < 0.0 ? 0.0 : (ymax > yh ? yh : ymax);
      }
      const double* g = p.box2d + (size_t)b * 4;
      const double gx0 = g[0], gy0 = g[1], gx1 = g[2], gy1 = g[3];
      const double iw = (xmax < gx1 ? xmax : gx1) - (xmin > gx0 ? xmin : gx0);
      const double ih = (ymax < gy1 ? ymax : gy1) - (ymin > gy0 ? ymin : gy0);
      const double inter = (iw > 0.0 && ih > 0.0) ? iw * ih : 0.0;
      const double aa = (xmax - xmin) * (ymax - ymin), ab = (gx1 - gx0) * (gy1 - gy0);
      const double uni = (aa + ab) - inter;
      r[0] = xmin; r[1] = ymin; r[2] = xmax; r[3] = ymax;
      r[4] = uni > 0.0 ? inter / uni : 0.0;
    }
  }
  int32_t* oc = p.counts + (size_t)b * 4;
  oc[0] = n_mask; oc[1] = n_box; oc[2] = n_both; oc[3] = flags;
  double* orr = p.reproj + (size_t)b * 5;
#pragma unroll
  for (int i = 0; i < 5; ++i) orr[i] = r[i];
}

}  // namespace

extern "C" int t3d_detect_consistency(const t3d_detect_consistency_args* a, t3d_stream_t stream) {
  T3D_ABI_TAKE(detect_consistency_args, a);
  if (!a) return T3D_ERR_ARG;
  if (a->B <= 0 || a->N <= 0 || a->n_valid < 0 || a->ld_xyz < 3 || a->n_calib < 0) return T3D_ERR_SHAPE;
  if (!a->xyz || !a->logits || !a->corners || !a->box2d || !a->calib_index || !a->calib || !a->counts || !a->reproj) return T3D_ERR_ARG;
  if (reinterpret_cast<uintptr_t>(a->logits) & 7u) return T3D_ERR_ARG;      // read as float2
  const int n = a->n_valid < a->B ? a->n_valid : a->B;
  if (n == 0) return T3D_OK;
  T3D_LAUNCH(k_detect_consistency, dim3(n), dim3(DC_THREADS), 0, static_cast<hipStream_t>(stream), *a);
  T3D_CHECK_LAUNCH();
  return T3D_OK;
}
