// Scene synthesis by ray casting (t3d.h t3d_scene_raycast): what a depth camera at the origin sees of a room of oriented boxes, for a
// batch of scenes.  Three launches, no host synchronisation between them:
//   k_scene_cast     one workgroup per T3D_SCENE_BLOCK_PIXELS consecutive pixels of a scene: the scene's parts staged in LDS (the camera
//                    is the origin, so the origin in a part's frame is staged with it), one ray per thread and pass against every part and
//                    the room -> hit, image, and the workgroup's count of emitted pixels;
//   k_scene_scan     one workgroup: exclusive scan of the counts in (scene, workgroup) order -> every workgroup's first row, scene_offsets;
//                    it also clears visible / vis_box, which only the third launch touches;
//   k_scene_scatter  the grid of the first launch: the rank of every emitted pixel within its workgroup, its depth recomputed from the
//                    one surface `hit` names (the same device function, the same bits), the row written at its rank; per object the
//                    emitted pixels and the extent of all its valid pixels, by integer LDS atomics, then integer global atomics.
// The position of a row is its rank in (scene, v, u) order and the statistics are integer minima, maxima and counts: nothing depends on
// which workgroup ran first.  The random numbers are a counter-based hash of (seed, scene id, pixel).
#include <float.h>

#include "common.h"

// The specification (t3d.h, tests/fake_scene.py) is elementwise fp64 in a stated order: no fused multiply-adds.
#pragma clang fp contract(off)

namespace {

constexpr int SC_THREADS = 256;
constexpr int SC_PASSES = T3D_SCENE_BLOCK_PIXELS / SC_THREADS;
static_assert(T3D_SCENE_BLOCK_PIXELS % SC_THREADS == 0, "a workgroup covers whole passes");

__device__ const double SC_SHADES[6] = T3D_SCENE_SHADES;

struct ScPart {          // a part as the cast reads it: the camera in the part's frame, the half-extents, the rotation
  double o[3], half[3], c, s;
};

__device__ __forceinline__ uint32_t sc_mix(uint64_t x) {      // the finaliser of frustum.hip's hash
  x ^= x >> 33; x *= 0xff51afd7ed558ccdULL;
  x ^= x >> 33; x *= 0xc4ceb9fe1a85ec53ULL;
  x ^= x >> 33;
  return (uint32_t)(x >> 16);
}
__device__ __forceinline__ uint64_t sc_base(uint32_t seed, int32_t scene_id, uint32_t pixel) {
  return ((uint64_t)seed << 32) ^ ((uint64_t)(uint32_t)scene_id * 0x9E3779B97F4A7C15ULL) ^ ((uint64_t)(pixel + 1u) * 0xC2B2AE3D27D4EB4FULL);
}
__device__ __forceinline__ double sc_uniform(uint64_t base, int j) {
  return ((double)sc_mix((base ^ 0x94D049BB133111EBULL) + (uint64_t)(j + 1) * 0xBF58476D1CE4E5B9ULL) + 0.5) * (1.0 / 4294967296.0);
}

// Box-Muller normal of two uniforms.  Not inlined: log and cos bring their own constants, which would share the scatter kernel's
// scalar registers with its arguments.
__device__ __noinline__ double sc_normal(double u1, double u2) { return sqrt(-2.0 * log(u1)) * cos(6.283185307179586 * u2); }

__device__ __forceinline__ ScPart sc_stage(const t3d_scene_part& p) {
  ScPart q;
  const double nx = -p.centre[0], ny = -p.centre[1];
  q.o[0] = p.cos_r * nx + p.sin_r * ny;
  q.o[1] = p.cos_r * ny - p.sin_r * nx;
  q.o[2] = -p.centre[2];
  q.half[0] = p.half[0]; q.half[1] = p.half[1]; q.half[2] = p.half[2];
  q.c = p.cos_r; q.s = p.sin_r;
  return q;
}

__device__ __forceinline__ void sc_ray(const double* R, const double* K, int u, int v, double d[3]) {
  const double cx = ((double)u - K[2]) / K[0], cy = ((double)v - K[5]) / K[4];
  const double q0 = cx, q1 = 1.0, q2 = -cy;
  for (int i = 0; i < 3; ++i) d[i] = (R[3 * i] * q0 + R[3 * i + 1] * q1) + R[3 * i + 2] * q2;
}

// The slab test of t3d.h.  True for a hit; t_in, the entered face 2k + (sign > 0) and nd = e[k] of it.
__device__ __forceinline__ bool sc_hit_part(const ScPart& p, const double d[3], double& t_in, int& face, double& nd) {
  const double e[3] = {p.c * d[0] + p.s * d[1], p.c * d[1] - p.s * d[0], d[2]};
  double tin = -DBL_MAX, tout = DBL_MAX, n = 0.0;
  int f = 0;
  bool miss = false;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const double h = p.half[k], o = p.o[k];
    if (e[k] == 0.0) {
      miss = miss || o < -h || o > h;
    } else {
      const double ta = (-h - o) / e[k], tb = (h - o) / e[k];
      const bool pos = e[k] > 0.0;
      const double tn = pos ? ta : tb, tf = pos ? tb : ta;
      if (tn > tin) { tin = tn; f = 2 * k + (pos ? 0 : 1); n = e[k]; }
      if (tf < tout) tout = tf;
    }
  }
  t_in = tin; face = f; nd = n;
  return !miss && tin > 0.0 && tin <= tout;
}

// The wall the ray leaves the room through.  False when no component of d is non-zero.
__device__ __forceinline__ bool sc_hit_room(const double* room, const double d[3], double& t_room, int& face, double& nd) {
  double t = DBL_MAX, n = 0.0;
  int f = 0;
  bool any = false;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    if (d[k] != 0.0) {
      const bool pos = d[k] > 0.0;
      const double tw = (pos ? room[2 * k + 1] : room[2 * k]) / d[k];
      if (tw < t) { t = tw; f = 2 * k + (pos ? 1 : 0); n = d[k]; }
      any = true;
    }
  }
  t_room = t; face = f; nd = n;
  return any;
}

__device__ __forceinline__ uint8_t sc_byte(double colour, int face) {
  double x = colour * SC_SHADES[face] + 0.5;
  x = x < 0.0 ? 0.0 : x;
  x = x > 255.0 ? 255.0 : x;
  return (uint8_t)(int)x;
}

// Sum over the 256 threads of the workgroup; `wsum`: 4 ints of LDS.
__device__ __forceinline__ int sc_block_sum(int v, int* wsum) {
  int x = v;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, 64);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = x;
  __syncthreads();
  return wsum[0] + wsum[1] + wsum[2] + wsum[3];
}

// Exclusive prefix sum over the 256 threads of the workgroup; `total` receives the sum.  `wsum`: 4 ints of LDS.
__device__ __forceinline__ int sc_block_scan(int v, int* wsum, int& total) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  int x = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int y = __shfl_up(x, o, 64);
    if (lane >= o) x += y;
  }
  __syncthreads();
  if (lane == 63) wsum[w] = x;
  __syncthreads();
  int off = 0;
  for (int k = 0; k < w; ++k) off += wsum[k];
  total = wsum[0] + wsum[1] + wsum[2] + wsum[3];
  return off + x - v;
}

__device__ __forceinline__ bool sc_emitted(const t3d_scene_raycast_args& p, int32_t scene_id, int u, int v, int pix, int hit) {
  if (hit < T3D_SCENE_HIT_ROOM || u % p.stride != 0 || v % p.stride != 0) return false;
  return !(sc_uniform(sc_base(p.seed, scene_id, (uint32_t)pix), 0) < p.p_drop);
}

__device__ __forceinline__ int64_t* sc_block_offset(const t3d_scene_raycast_args& p) { return static_cast<int64_t*>(p.workspace); }
__device__ __forceinline__ int32_t* sc_block_count(const t3d_scene_raycast_args& p, int64_t n_blocks) {
  return reinterpret_cast<int32_t*>(static_cast<int64_t*>(p.workspace) + n_blocks);
}

__global__ __launch_bounds__(SC_THREADS) void k_scene_cast(const t3d_scene_raycast_args p) {
  __shared__ ScPart parts[T3D_SCENE_MAX_PARTS];
  __shared__ int wsum[4];
  const int s = blockIdx.y, HW = p.H * p.W;
  const int first = p.part_offsets[s];
  const int n_parts = min(max(p.part_offsets[s + 1] - first, 0), T3D_SCENE_MAX_PARTS);
  for (int k = threadIdx.x; k < n_parts; k += SC_THREADS) parts[k] = sc_stage(p.parts[first + k]);
  __syncthreads();
  const double* R = p.rtilt + (size_t)s * 9;
  const double* K = p.K + (size_t)s * 9;
  const double* room = p.room + (size_t)s * 6;
  const int32_t scene_id = p.scene_id[s];
  int n_emit = 0;
  for (int r = 0; r < SC_PASSES; ++r) {
    const int pix = blockIdx.x * T3D_SCENE_BLOCK_PIXELS + r * SC_THREADS + threadIdx.x;
    if (pix >= HW) continue;
    const int v = pix / p.W, u = pix - v * p.W;
    double d[3];
    sc_ray(R, K, u, v, d);
    double t_best = DBL_MAX, nd_best = 0.0;
    int best = -1, face_best = 0;
    for (int k = 0; k < n_parts; ++k) {
      double t, nd;
      int face;
      if (sc_hit_part(parts[k], d, t, face, nd) && (best < 0 || t < t_best)) { best = k; t_best = t; face_best = face; nd_best = nd; }
    }
    double t_room, nd_room;
    int face_room;
    const bool wall = sc_hit_room(room, d, t_room, face_room, nd_room);
    int hit = T3D_SCENE_HIT_INVALID, face = 0;
    double t = 0.0, nd = 0.0;
    bool surface = false;
    if (best >= 0 && (!wall || t_best <= t_room)) { hit = best; t = t_best; nd = nd_best; face = face_best; surface = true; }
    else if (wall) { hit = T3D_SCENE_HIT_ROOM; t = t_room; nd = nd_room; face = face_room; surface = true; }
    const double dd = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2];
    if (!(surface && t <= p.max_range && nd * nd >= p.min_cos2 * dd)) hit = T3D_SCENE_HIT_INVALID;
    const size_t o = (size_t)s * HW + pix;
    p.hit[o] = hit;
    uint8_t* px = p.image + o * 3;
    if (hit == T3D_SCENE_HIT_INVALID) {
      px[0] = 0; px[1] = 0; px[2] = 0;
    } else if (hit == T3D_SCENE_HIT_ROOM) {
      const uint8_t b = sc_byte(T3D_SCENE_ROOM_COLOUR, face);
      px[0] = b; px[1] = b; px[2] = b;
    } else {
      const double* col = p.parts[first + hit].colour;
      for (int c = 0; c < 3; ++c) px[c] = sc_byte(col[c], face);
    }
    n_emit += sc_emitted(p, scene_id, u, v, pix, hit) ? 1 : 0;
  }
  const int total = sc_block_sum(n_emit, wsum);
  if (threadIdx.x == 0) sc_block_count(p, (int64_t)gridDim.x * gridDim.y)[(size_t)s * gridDim.x + blockIdx.x] = total;
}

__global__ __launch_bounds__(SC_THREADS) void k_scene_scan(const t3d_scene_raycast_args p, int blocks_per_scene) {
  __shared__ int wsum[4];
  const int64_t n = (int64_t)p.n_scenes * blocks_per_scene;
  const int32_t* count = sc_block_count(p, n);
  int64_t* offset = sc_block_offset(p);
  int64_t carry = 0;
  for (int64_t i0 = 0; i0 < n; i0 += SC_THREADS) {
    const int64_t i = i0 + threadIdx.x;
    int tot;
    const int e = sc_block_scan(i < n ? count[i] : 0, wsum, tot);
    if (i < n) {
      offset[i] = carry + e;
      if (i % blocks_per_scene == 0) p.scene_offsets[i / blocks_per_scene] = carry + e;
    }
    carry += tot;
  }
  if (threadIdx.x == 0) p.scene_offsets[p.n_scenes] = carry;
  const int64_t n_obj = (int64_t)p.n_scenes * T3D_SCENE_MAX_OBJECTS;
  for (int64_t i = threadIdx.x; i < n_obj; i += SC_THREADS) {
    p.visible[i] = 0;
    p.vis_box[i * 4] = p.W; p.vis_box[i * 4 + 1] = p.H; p.vis_box[i * 4 + 2] = -1; p.vis_box[i * 4 + 3] = -1;
  }
}

__global__ __launch_bounds__(SC_THREADS) void k_scene_scatter(const t3d_scene_raycast_args p) {
  __shared__ int wsum[4];
  __shared__ int vis[T3D_SCENE_MAX_OBJECTS];
  __shared__ int box[T3D_SCENE_MAX_OBJECTS][4];
  __shared__ double cam[24];          // rtilt, K, room of the scene: read as vector operands (as scalars they crowd the scalar file)
  const int s = blockIdx.y, HW = p.H * p.W;
  if (threadIdx.x >= 64 && threadIdx.x < 64 + 24) {
    const int k = threadIdx.x - 64;
    cam[k] = k < 9 ? p.rtilt[(size_t)s * 9 + k] : k < 18 ? p.K[(size_t)s * 9 + k - 9] : p.room[(size_t)s * 6 + k - 18];
  }
  if (threadIdx.x < T3D_SCENE_MAX_OBJECTS) {
    vis[threadIdx.x] = 0;
    box[threadIdx.x][0] = p.W; box[threadIdx.x][1] = p.H; box[threadIdx.x][2] = -1; box[threadIdx.x][3] = -1;
  }
  __syncthreads();
  const int first = p.part_offsets[s];
  const double* R = cam, * K = cam + 9, * room = cam + 18;
  const int32_t scene_id = p.scene_id[s];
  int64_t row0 = sc_block_offset(p)[(size_t)s * gridDim.x + blockIdx.x];
#pragma unroll 1
  for (int r = 0; r < SC_PASSES; ++r) {
    const int pix = blockIdx.x * T3D_SCENE_BLOCK_PIXELS + r * SC_THREADS + threadIdx.x;
    const bool in = pix < HW;
    const int v = in ? pix / p.W : 0, u = in ? pix - v * p.W : 0;
    const size_t o = (size_t)s * HW + (in ? pix : 0);
    const int hit = in ? p.hit[o] : T3D_SCENE_HIT_INVALID;
    const bool emit = in && sc_emitted(p, scene_id, u, v, pix, hit);
    int owner = -1;
    if (hit >= 0) owner = p.parts[first + hit].owner;
    if ((unsigned)owner < (unsigned)T3D_SCENE_MAX_OBJECTS) {      // counts, minima and maxima of integers: any order gives the same
      atomicMin(&box[owner][0], u); atomicMin(&box[owner][1], v);
      atomicMax(&box[owner][2], u); atomicMax(&box[owner][3], v);
      if (emit) atomicAdd(&vis[owner], 1);
    }
    int tot;
    const int rank = sc_block_scan(emit ? 1 : 0, wsum, tot);
    if (emit && row0 + rank < p.points_capacity) {
      double d[3], t, nd;
      int face;
      sc_ray(R, K, u, v, d);
      if (hit >= 0) {
        const ScPart q = sc_stage(p.parts[first + hit]);
        sc_hit_part(q, d, t, face, nd);
      } else {
        sc_hit_room(room, d, t, face, nd);
      }
      double m = t;
      if (p.noise_a != 0.0) {
        const uint64_t base = sc_base(p.seed, scene_id, (uint32_t)pix);
        const double g = sc_normal(sc_uniform(base, 1), sc_uniform(base, 2));
        m = t + ((p.noise_a * (t * t)) * g);
      }
      double* dst = p.points + (size_t)(row0 + rank) * 6;
      const uint8_t* px = p.image + o * 3;
      for (int i = 0; i < 3; ++i) dst[i] = d[i] * m;
      for (int c = 0; c < 3; ++c) dst[3 + c] = (double)px[c] / 255.0;
      if (p.point_pixel) p.point_pixel[row0 + rank] = pix;
    }
    row0 += tot;
  }
  __syncthreads();
  if (threadIdx.x < T3D_SCENE_MAX_OBJECTS && box[threadIdx.x][2] >= 0) {
    const size_t k = (size_t)s * T3D_SCENE_MAX_OBJECTS + threadIdx.x;
    atomicMin(&p.vis_box[k * 4], box[threadIdx.x][0]); atomicMin(&p.vis_box[k * 4 + 1], box[threadIdx.x][1]);
    atomicMax(&p.vis_box[k * 4 + 2], box[threadIdx.x][2]); atomicMax(&p.vis_box[k * 4 + 3], box[threadIdx.x][3]);
    if (vis[threadIdx.x] > 0) atomicAdd(&p.visible[k], vis[threadIdx.x]);
  }
}

}  // namespace

extern "C" int t3d_scene_raycast(const t3d_scene_raycast_args* a, t3d_stream_t stream) {
  T3D_ABI_TAKE(scene_raycast_args, a);
  if (!a || !a->rtilt || !a->K || !a->scene_id || !a->room || !a->part_offsets || !a->room_host || !a->part_offsets_host ||
      !a->n_objects_host || !a->hit || !a->image || !a->points || !a->scene_offsets || !a->visible || !a->vis_box || a->reserved != 0)
    return T3D_ERR_ARG;
  if (a->n_scenes < 1 || a->n_scenes > 65535 || a->H < 1 || a->W < 1 || (int64_t)a->H * a->W > (1 << 24) || a->stride < 1) return T3D_ERR_SHAPE;
  if (a->part_offsets_host[0] != 0) return T3D_ERR_SHAPE;
  for (int s = 0; s < a->n_scenes; ++s) {
    const int n = a->part_offsets_host[s + 1] - a->part_offsets_host[s];
    if (n < 0 || n > T3D_SCENE_MAX_PARTS || a->n_objects_host[s] < 0 || a->n_objects_host[s] > T3D_SCENE_MAX_OBJECTS) return T3D_ERR_SHAPE;
  }
  if (a->part_offsets_host[a->n_scenes] > 0 && !a->parts) return T3D_ERR_ARG;
  for (int s = 0; s < a->n_scenes; ++s)
    for (int k = 0; k < 3; ++k)
      if (!(a->room_host[s * 6 + 2 * k] < 0.0 && a->room_host[s * 6 + 2 * k + 1] > 0.0)) return T3D_ERR_ARG;
  if (!(a->p_drop >= 0.0) || !(a->noise_a >= 0.0) || !(a->max_range > 0.0) || !(a->min_cos2 >= 0.0 && a->min_cos2 <= 1.0)) return T3D_ERR_ARG;
  const uint64_t need = T3D_SCENE_WORKSPACE_BYTES(a->n_scenes, a->H, a->W);
  if (!a->workspace || (reinterpret_cast<uintptr_t>(a->workspace) & 7u) != 0 || a->workspace_bytes < need) return T3D_ERR_ARG;
  const int64_t hs = (a->H + a->stride - 1) / a->stride, ws = (a->W + a->stride - 1) / a->stride;
  if (a->points_capacity < (int64_t)a->n_scenes * hs * ws) return T3D_ERR_ARG;
  const hipStream_t st = static_cast<hipStream_t>(stream);
  const int nb = (int)T3D_SCENE_BLOCKS(a->H, a->W);
  T3D_LAUNCH(k_scene_cast, dim3(nb, a->n_scenes), dim3(SC_THREADS), 0, st, *a);
  T3D_CHECK_LAUNCH();
  T3D_LAUNCH(k_scene_scan, dim3(1), dim3(SC_THREADS), 0, st, *a, nb);
  T3D_CHECK_LAUNCH();
  T3D_LAUNCH(k_scene_scatter, dim3(nb, a->n_scenes), dim3(SC_THREADS), 0, st, *a);
  T3D_CHECK_LAUNCH();
  return T3D_OK;
}
