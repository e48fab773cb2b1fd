// Headless software rasteriser (t3d.h t3d_render): z-buffered point splats, 3-D box wireframes and 2-D rectangles of many small views
// in three launches, every rule of which is written out in the header.  Memory-bound, no MFMA, no LDS.
//   k_render_clear    one thread per workspace pixel: the depth word to "empty", the ordinal to 0, the view's background into `out`;
//   k_render_paint    the first blocks run one thread per POSITION of the concatenated point ranges (a thread finds its range by a binary
//                     search of pos_first, as csrc/nms.hip finds a group): transform, visibility, 64-bit atomicMin of (bits(D) << 32 |
//                     point index) over the splat square; the other blocks run one wave per segment (12 per box entry, 4 per
//                     rectangle): lanes 0-7 transform the box's corners, the endpoints travel by shuffles, the wave clips against the
//                     near plane and strides over the major-axis steps that can touch the view, a 32-bit atomicMax of the primitive's
//                     ordinal per stamped pixel;
//   k_render_resolve  one thread per workspace pixel: the ordinal's colour, else the depth winner's colour, else nothing (the background
//                     of the first launch stays).
// Integer min / max atomics only: the picture does not depend on the order in which threads arrive.  Every table entry is validated
// on the device as well (an entry that breaks the contract paints nothing and nothing is written outside a view's own bytes).
// Contraction is off in this translation unit: the header documents every product and sum as its own fp32 operation.
#pragma clang fp contract(off)
#include "common.h"

namespace {

constexpr int RENDER_THREADS = 256;
constexpr unsigned long long Z_EMPTY = ~0ull;
constexpr int PIX_CLAMP = 1 << 20;

__device__ __forceinline__ bool finite_f(float v) { return fabsf(v) <= 3.402823466e38f; }      // (a NaN compares false)

__device__ __forceinline__ float row_dot(const float* p, float x, float y, float z) { return ((p[0] * x + p[1] * y) + p[2] * z) + p[3]; }

__device__ __forceinline__ uint8_t to_byte(float c) {
  const float v = floorf(c * 255.f + 0.5f);
  return (uint8_t)fminf(255.f, fmaxf(0.f, v));      // (fmaxf drops a NaN: 0)
}

__device__ __forceinline__ bool view_ok(const t3d_render_args& a, int v) {
  if ((unsigned)v >= (unsigned)a.n_views) return false;
  const t3d_render_view& w = a.views[v];
  if (w.H <= 0 || w.W <= 0 || w.pixel_first < 0 || w.out_offset < 0) return false;
  const long long px = (long long)w.H * w.W;
  return px <= a.total_pixels - w.pixel_first && (unsigned long long)w.out_offset + 3ull * px <= a.out_bytes;
}

// The view whose workspace pixels hold p (views lie back to back, in table order), or -1.
__device__ __forceinline__ int view_of_pixel(const t3d_render_args& a, long long p) {
  int lo = 0, hi = a.n_views;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (a.views[mid].pixel_first <= p) lo = mid + 1; else hi = mid;
  }
  const int v = lo - 1;
  if (v < 0 || !view_ok(a, v)) return -1;
  return p - a.views[v].pixel_first < (long long)a.views[v].H * a.views[v].W ? v : -1;
}

__device__ __forceinline__ bool range_ok(const t3d_render_args& a, const t3d_render_points& r) {
  if (r.first < 0 || r.count < 0 || r.count > a.n_points - r.first || !a.xyz) return false;
  if (r.splat != 1 && r.splat != 3 && r.splat != 5) return false;
  if (r.mode == T3D_RENDER_RGB) return a.rgb != nullptr;
  if (r.mode == T3D_RENDER_LABEL) return a.label != nullptr;
  return r.mode == T3D_RENDER_FLAT;
}

__global__ __launch_bounds__(RENDER_THREADS) void k_render_clear(const t3d_render_args a, unsigned long long* zbuf, int32_t* ord) {
  const long long p = (long long)blockIdx.x * RENDER_THREADS + threadIdx.x;
  if (p >= a.total_pixels) return;
  zbuf[p] = Z_EMPTY;
  ord[p] = 0;
  const int v = view_of_pixel(a, p);
  if (v < 0) return;
  const t3d_render_view& w = a.views[v];
  const long long q = p - w.pixel_first;
  uint8_t* o = a.out + w.out_offset + 3 * q;
  if (w.bg_offset >= 0 && a.bg && (unsigned long long)w.bg_offset + 3ull * w.H * w.W <= a.bg_bytes) {
    const uint8_t* b = a.bg + w.bg_offset + 3 * q;
    o[0] = b[0]; o[1] = b[1]; o[2] = b[2];
  } else {
    o[0] = to_byte(w.bg_colour[0]); o[1] = to_byte(w.bg_colour[1]); o[2] = to_byte(w.bg_colour[2]);
  }
}

__device__ __forceinline__ void paint_point(const t3d_render_args& a, long long item, unsigned long long* zbuf) {
  int lo = 0, hi = a.n_ranges;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (a.ranges[mid].pos_first <= item) lo = mid + 1; else hi = mid;
  }
  // (ranges of no points share a pos_first with their successor: the search lands on the last of them, which is the one with points)
  if (lo == 0) return;
  const t3d_render_points& r = a.ranges[lo - 1];
  const long long k = item - r.pos_first;
  if (k < 0 || k >= r.count || !range_ok(a, r) || !view_ok(a, r.view)) return;
  const t3d_render_view& w = a.views[r.view];
  const int idx = r.first + (int)k;
  const float* pt = a.xyz + (long long)idx * a.ld_xyz;
  const float x = pt[0], y = pt[1], z = pt[2];
  const float X = row_dot(w.P, x, y, z), Y = row_dot(w.P + 4, x, y, z), D = row_dot(w.P + 8, x, y, z), Wc = row_dot(w.P + 12, x, y, z);
  if (!(finite_f(X) && finite_f(Y) && finite_f(D) && finite_f(Wc))) return;
  if (!(Wc >= w.w_near) || !(D >= 0.f)) return;
  const float fu = floorf(X / Wc + 0.5f), fv = floorf(Y / Wc + 0.5f);
  if (!(fu >= -4.f && fu <= (float)w.W + 4.f && fv >= -4.f && fv <= (float)w.H + 4.f)) return;      // (cannot touch the view; NaN and inf too)
  const int px = (int)fu, py = (int)fv, h = r.splat >> 1;
  const unsigned long long key = ((unsigned long long)__float_as_uint(D == 0.f ? 0.f : D) << 32) | (unsigned)idx;
  for (int yy = max(py - h, 0); yy <= min(py + h, w.H - 1); ++yy)
    for (int xx = max(px - h, 0); xx <= min(px + h, w.W - 1); ++xx)
      atomicMin(&zbuf[w.pixel_first + (long long)yy * w.W + xx], key);
}

// One wave per segment `s`: 12 per box entry (entries first), then 4 per rectangle.
__device__ __forceinline__ void paint_segment(const t3d_render_args& a, long long s, int lane, int32_t* ord) {
  const long long box_segments = 12ll * a.n_boxes;
  int view, thickness, ordinal;
  float ua, va, ub, vb;
  if (s < box_segments) {
    const int e = (int)(s / 12), k = (int)(s % 12);
    const t3d_render_box& b = a.boxes[e];
    view = b.view; thickness = b.thickness; ordinal = 1 + e;
    if (!view_ok(a, view) || (unsigned)b.box >= (unsigned)a.n_corner_boxes || !a.corners) return;      // (wave-uniform)
    const t3d_render_view& w = a.views[view];
    const float* c = a.corners + (long long)b.box * 24 + 3 * (lane & 7);
    const float x = c[0], y = c[1], z = c[2];
    const float X = row_dot(w.P, x, y, z), Y = row_dot(w.P + 4, x, y, z), D = row_dot(w.P + 8, x, y, z), Wc = row_dot(w.P + 12, x, y, z);
    const bool fin = finite_f(X) && finite_f(Y) && finite_f(D) && finite_f(Wc);
    if (__ballot(fin) != ~0ull) return;            // a corner with a non-finite coordinate: the box is dropped (every lane holds one of the 8)
    const int i = k & 3;
    const int ia = k < 4 ? i : k < 8 ? 4 + i : i, ib = k < 4 ? (i + 1) & 3 : k < 8 ? 4 + ((i + 1) & 3) : i + 4;
    float Xa = __shfl(X, ia, 64), Ya = __shfl(Y, ia, 64), Wa = __shfl(Wc, ia, 64);
    float Xb = __shfl(X, ib, 64), Yb = __shfl(Y, ib, 64), Wb = __shfl(Wc, ib, 64);
    const float wn = w.w_near;
    const bool behind_a = Wa < wn, behind_b = Wb < wn;
    if (behind_a && behind_b) return;
    if (behind_a || behind_b) {
      const float t = (wn - Wa) / (Wb - Wa);
      const float Xc = Xa + t * (Xb - Xa), Yc = Ya + t * (Yb - Ya);
      if (behind_a) { Xa = Xc; Ya = Yc; Wa = wn; } else { Xb = Xc; Yb = Yc; Wb = wn; }
    }
    ua = Xa / Wa; va = Ya / Wa; ub = Xb / Wb; vb = Yb / Wb;
  } else {
    const long long q = s - box_segments;
    const int e = (int)(q / 4), k = (int)(q % 4);
    const t3d_render_rect& r = a.rects[e];
    view = r.view; thickness = r.thickness; ordinal = 1 + a.n_boxes + e;
    if (!view_ok(a, view)) return;
    if (!(finite_f(r.xmin) && finite_f(r.ymin) && finite_f(r.xmax) && finite_f(r.ymax))) return;
    ua = (k == 0 || k == 3) ? r.xmin : r.xmax;      // (xmin,ymin) -> (xmax,ymin) -> (xmax,ymax) -> (xmin,ymax) -> back
    va = (k == 0 || k == 1) ? r.ymin : r.ymax;
    ub = (k == 0 || k == 1) ? r.xmax : r.xmin;
    vb = (k == 1 || k == 2) ? r.ymax : r.ymin;
  }
  if (thickness < 1 || thickness > 5) return;
  if (!(finite_f(ua) && finite_f(va) && finite_f(ub) && finite_f(vb))) return;
  const t3d_render_view& w = a.views[view];
  const float lim = (float)PIX_CLAMP;
  int ax = (int)fminf(lim, fmaxf(-lim, floorf(ua + 0.5f))), ay = (int)fminf(lim, fmaxf(-lim, floorf(va + 0.5f)));
  int bx = (int)fminf(lim, fmaxf(-lim, floorf(ub + 0.5f))), by = (int)fminf(lim, fmaxf(-lim, floorf(vb + 0.5f)));
  const bool x_major = abs(bx - ax) >= abs(by - ay);
  // in (major, minor) coordinates, A the endpoint of the smaller major coordinate (the smaller minor on a tie)
  int a_maj = x_major ? ax : ay, a_min = x_major ? ay : ax, b_maj = x_major ? bx : by, b_min = x_major ? by : bx;
  if (b_maj < a_maj || (b_maj == a_maj && b_min < a_min)) {
    int t = a_maj; a_maj = b_maj; b_maj = t;
    t = a_min; a_min = b_min; b_min = t;
  }
  const int n_maj = x_major ? w.W : w.H, n_min = x_major ? w.H : w.W;
  const int o_lo = -((thickness - 1) / 2), o_hi = thickness / 2;
  const long long d_maj = (long long)b_maj - a_maj, d_min = (long long)b_min - a_min;
  const int m0 = max(a_maj, -o_hi), m1 = min(b_maj, n_maj - 1 - o_lo);      // the steps whose stamp can reach the view
  for (int m = m0 + lane; m <= m1; m += 64) {
    int mn = a_min;
    if (d_maj > 0) {
      const long long num = 2 * (long long)(m - a_maj) * d_min + d_maj, den = 2 * d_maj;
      long long f = num / den;
      if (num % den != 0 && num < 0) --f;           // floor division
      mn = a_min + (int)f;
    }
    for (int oj = o_lo; oj <= o_hi; ++oj) {
      const int pm = m + oj;
      if (pm < 0 || pm >= n_maj) continue;
      for (int oi = o_lo; oi <= o_hi; ++oi) {
        const int pn = mn + oi;
        if (pn < 0 || pn >= n_min) continue;
        const int xx = x_major ? pm : pn, yy = x_major ? pn : pm;
        atomicMax(&ord[w.pixel_first + (long long)yy * w.W + xx], ordinal);
      }
    }
  }
}

__global__ __launch_bounds__(RENDER_THREADS) void k_render_paint(const t3d_render_args a, unsigned long long* zbuf, int32_t* ord, int point_blocks) {
  if ((int)blockIdx.x < point_blocks) {
    const long long item = (long long)blockIdx.x * RENDER_THREADS + threadIdx.x;
    if (item < a.total_point_items) paint_point(a, item, zbuf);
    return;
  }
  const long long s = (long long)(blockIdx.x - point_blocks) * (RENDER_THREADS / 64) + threadIdx.x / 64;
  if (s < 12ll * a.n_boxes + 4ll * a.n_rects) paint_segment(a, s, threadIdx.x & 63, ord);
}

__global__ __launch_bounds__(RENDER_THREADS) void k_render_resolve(const t3d_render_args a, const unsigned long long* zbuf, const int32_t* ord) {
  const long long p = (long long)blockIdx.x * RENDER_THREADS + threadIdx.x;
  if (p >= a.total_pixels) return;
  const int o = ord[p];
  const unsigned long long z = zbuf[p];
  if (o <= 0 && z == Z_EMPTY) return;
  const int v = view_of_pixel(a, p);
  if (v < 0) return;
  const t3d_render_view& w = a.views[v];
  float c0, c1, c2;
  if (o > 0) {
    const float* c = o - 1 < a.n_boxes ? a.boxes[o - 1].colour : a.rects[o - 1 - a.n_boxes].colour;
    c0 = c[0]; c1 = c[1]; c2 = c[2];
  } else {
    const int idx = (int)(unsigned)(z & 0xffffffffull);
    int r = 0;      // the first range of this view that holds the point
    for (; r < a.n_ranges; ++r) {
      const t3d_render_points& g = a.ranges[r];
      if (g.view == v && idx >= g.first && idx - g.first < g.count && range_ok(a, g)) break;
    }
    if (r == a.n_ranges) return;
    const t3d_render_points& g = a.ranges[r];
    const float* c = g.colour0;
    if (g.mode == T3D_RENDER_RGB) c = a.rgb + 3ll * idx;
    else if (g.mode == T3D_RENDER_LABEL && a.label[idx] != 0) c = g.colour1;
    c0 = c[0]; c1 = c[1]; c2 = c[2];
  }
  uint8_t* out = a.out + w.out_offset + 3 * (p - w.pixel_first);
  out[0] = to_byte(c0); out[1] = to_byte(c1); out[2] = to_byte(c2);
}

// The host mirrors of the tables, where the caller passes them: what the header lists as T3D_ERR_ARG.
int check_mirrors(const t3d_render_args* a) {
  if (a->views_host) {
    long long at = 0;
    for (int v = 0; v < a->n_views; ++v) {
      const t3d_render_view& w = a->views_host[v];
      if (w.H <= 0 || w.W <= 0 || w.pixel_first != at || w.out_offset < 0) return T3D_ERR_ARG;
      const unsigned long long bytes = 3ull * (unsigned long long)w.H * (unsigned long long)w.W;
      if ((unsigned long long)w.out_offset + bytes > a->out_bytes) return T3D_ERR_ARG;
      if (w.bg_offset < -1 || (w.bg_offset >= 0 && (!a->bg || (unsigned long long)w.bg_offset + bytes > a->bg_bytes))) return T3D_ERR_ARG;
      at += (long long)w.H * w.W;
    }
    if (at != a->total_pixels) return T3D_ERR_ARG;
  }
  if (a->ranges_host) {
    long long at = 0;
    for (int r = 0; r < a->n_ranges; ++r) {
      const t3d_render_points& g = a->ranges_host[r];
      if ((unsigned)g.view >= (unsigned)a->n_views || g.first < 0 || g.count < 0 || g.count > a->n_points - g.first || g.pos_first != at) return T3D_ERR_ARG;
      if (g.splat != 1 && g.splat != 3 && g.splat != 5) return T3D_ERR_ARG;
      if (g.mode != T3D_RENDER_RGB && g.mode != T3D_RENDER_LABEL && g.mode != T3D_RENDER_FLAT) return T3D_ERR_ARG;
      if ((g.mode == T3D_RENDER_RGB && !a->rgb) || (g.mode == T3D_RENDER_LABEL && !a->label)) return T3D_ERR_ARG;
      at += g.count;
    }
    if (at != a->total_point_items) return T3D_ERR_ARG;
  }
  if (a->boxes_host)
    for (int b = 0; b < a->n_boxes; ++b) {
      const t3d_render_box& e = a->boxes_host[b];
      if ((unsigned)e.view >= (unsigned)a->n_views || (unsigned)e.box >= (unsigned)a->n_corner_boxes || e.thickness < 1 || e.thickness > 5) return T3D_ERR_ARG;
    }
  if (a->rects_host)
    for (int r = 0; r < a->n_rects; ++r) {
      const t3d_render_rect& e = a->rects_host[r];
      if ((unsigned)e.view >= (unsigned)a->n_views || e.thickness < 1 || e.thickness > 5) return T3D_ERR_ARG;
    }
  return T3D_OK;
}

}  // namespace

extern "C" int t3d_render(const t3d_render_args* a, t3d_stream_t stream) {
  T3D_ABI_TAKE(render_args, a);
  if (!a) return T3D_ERR_ARG;
  if (a->n_views < 0 || a->n_points < 0 || a->n_ranges < 0 || a->n_corner_boxes < 0 || a->n_boxes < 0 || a->n_rects < 0) return T3D_ERR_ARG;
  if (a->total_pixels < 0 || a->total_point_items < 0 || a->ld_xyz < 0) return T3D_ERR_ARG;
  if (a->n_views == 0) return T3D_OK;
  if (!a->views || !a->out || !a->workspace) return T3D_ERR_ARG;
  if (a->total_pixels == 0) return T3D_ERR_ARG;                          // (a view has at least one pixel)
  if ((a->n_ranges > 0 && (!a->ranges || !a->xyz || a->ld_xyz < 3)) || (a->n_boxes > 0 && (!a->boxes || !a->corners)) || (a->n_rects > 0 && !a->rects))
    return T3D_ERR_ARG;
  if (a->n_ranges == 0 && a->total_point_items != 0) return T3D_ERR_ARG;
  if (a->total_pixels > 0x7fffffffll || (long long)a->n_boxes + a->n_rects > 0x7ffffffell) return T3D_ERR_SHAPE;      // (an ordinal is an int32)
  if (a->workspace_bytes < T3D_RENDER_WORKSPACE_BYTES(a->total_pixels) || (reinterpret_cast<uintptr_t>(a->workspace) & 7u)) return T3D_ERR_ARG;
  const int e = check_mirrors(a);
  if (e != T3D_OK) return e;
  unsigned long long* zbuf = static_cast<unsigned long long*>(a->workspace);
  int32_t* ord = reinterpret_cast<int32_t*>(zbuf + a->total_pixels);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const long long pixel_blocks = (a->total_pixels + RENDER_THREADS - 1) / RENDER_THREADS;
  const long long point_blocks = (a->total_point_items + RENDER_THREADS - 1) / RENDER_THREADS;
  const long long segments = 12ll * a->n_boxes + 4ll * a->n_rects;
  const long long paint_blocks = point_blocks + (segments + RENDER_THREADS / 64 - 1) / (RENDER_THREADS / 64);
  if (paint_blocks > 0x7fffffffll) return T3D_ERR_SHAPE;
  T3D_LAUNCH(k_render_clear, dim3((unsigned)pixel_blocks), dim3(RENDER_THREADS), 0, st, *a, zbuf, ord);
  T3D_CHECK_LAUNCH();
  if (paint_blocks > 0) {
    T3D_LAUNCH(k_render_paint, dim3((unsigned)paint_blocks), dim3(RENDER_THREADS), 0, st, *a, zbuf, ord, (int)point_blocks);
    T3D_CHECK_LAUNCH();
  }
  T3D_LAUNCH(k_render_resolve, dim3((unsigned)pixel_blocks), dim3(RENDER_THREADS), 0, st, *a, zbuf, ord);
  T3D_CHECK_LAUNCH();
  return T3D_OK;
}
