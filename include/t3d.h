/*
 * t3d.h -- C ABI of the MI355X-native Frustum-PointNet training path (libt3d.so).
 *
 * The reference (yewsiang/Transferable3D) has no FFI layer: its hot path is stock TensorFlow-1 ops
 * reached through the Python wrappers in models/tf_util.py.  Each entry point below therefore cites
 * the reference call site(s) whose arithmetic it replaces; the Python side of the boundary
 * (transferable3d_amd/tf_util.py, semisup_models.py, ...) keeps the reference's function names.
 *
 * Conventions
 *   - extern "C", plain pointers and sizes, `int` return: 0 = T3D_OK, negative = T3D_ERR_*.
 *   - every buffer is a caller-owned DEVICE pointer (the library never allocates or frees);
 *     scratch (partials, slabs) is passed in explicitly.
 *   - all matrices are row-major, channel fastest: a (B, N, C) point tensor is an (M = B*N, C)
 *     matrix, exactly the reference's NHWC layout with H = N, W = 1.
 *   - `stream` is a hipStream_t; kernels are enqueued, never synchronised (one exception, outside the training step:
 *     t3d_label_subset).  No global state.
 *   - "partials" are per-128-row-tile column reductions ([M/128, C], T3D_TILE_ROWS rows each) that a
 *     finalize kernel combines deterministically (no float atomics anywhere on the path).
 *   - M must be a multiple of T3D_TILE_ROWS and rows_per_frustum (the point count N) a multiple of
 *     T3D_TILE_ROWS, so that a tile never straddles two frustums.
 */
#ifndef T3D_H_
#define T3D_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define T3D_OK 0
#define T3D_ERR_ARG (-1)     /* null / inconsistent argument */
#define T3D_ERR_SHAPE (-2)   /* unsupported shape (alignment, divisibility) */
#define T3D_ERR_LAUNCH (-3)  /* HIP launch failure */
#define T3D_ERR_ABI (-4)     /* an argument struct of another size than this library was built for (see `struct_size`) */

/* ABI versions 2 and 3.  Version 1 structs were plain; fields appended to four of them in round 4 (w_x3, oracle_mask, rowmask) made a caller
 * built against the older header pass structs the library read past.  Since version 2 every argument struct that has grown, or may
 * grow, starts with `struct_size`: the caller stores sizeof(the struct as ITS header declares it) there.  New fields are only ever
 * appended, and 0 is the documented default of every appended field.  An entry point that takes such a struct accepts
 *     struct_size == the library's sizeof          the same header;
 *     T3D_V2_SIZE_<struct> <= struct_size < sizeof  an OLDER caller: the fields it does not know read 0 (csrc/abi_take.h copies the
 *                                                   caller's bytes into a zeroed struct of the library's own declaration);
 *     struct_size > sizeof, every byte beyond 0     a NEWER caller that uses none of the fields this library does not know;
 * and returns T3D_ERR_ABI for anything else (a struct shorter than its version-2 size; a newer caller's non-zero unknown field).
 * (Until round 5 the test was equality: every append would have refused every older caller.)  The structs WITHOUT `struct_size` are
 * frozen: they never grow -- a change to one of them is a new struct behind a new entry point. */
#define T3D_ABI_VERSION 3      /* 3: `w_x3` means fragment-order planes (t3d_split_x3_frag); layouts and sizes as version 2 */
/* sizeof of the growable structs at ABI version 2 (the smallest struct_size an entry point accepts) */
#define T3D_V2_SIZE_pointmlp_fwd_args 200
#define T3D_V2_SIZE_pointmlp_dgrad_args 168
#define T3D_V2_SIZE_pointmlp_wgrad_args 144
#define T3D_V2_SIZE_pointmlp_dgrad_gram_args 168
#define T3D_V2_SIZE_pointmlp_gram_args 96
#define T3D_V2_SIZE_seg_head_args 208
#define T3D_V2_SIZE_boxpc_rep_args 104

#define T3D_TILE_ROWS 128

typedef void* t3d_stream_t;

enum { T3D_ACT_NONE = 0, T3D_ACT_RELU = 1, T3D_ACT_LEAKY_RELU = 2, T3D_ACT_TANH = 3 };

/* Element type of the per-point [M, C] layer tensors (raw conv outputs y, gradients dz) and, with it, the arithmetic of the GEMM
 * that produces or consumes them (BASELINE.json configs[1..3] vs configs[4]):
 *   T3D_F32   fp32 storage, v_mfma_f32_32x32x2_f32 (exact fp32)
 *   T3D_BF16  bf16 storage (2 bytes per element in HBM), operands rounded to bf16 while they are staged into LDS,
 *             v_mfma_f32_32x32x16_bf16 with fp32 accumulation; statistics, partials, weights, weight gradients, the sparse
 *             arg-max rows, the per-frustum [B, C] tensors, the optimiser and the raw inputs (point cloud, Box-PC
 *             representation) stay fp32.
 * Every `dtype` field below takes one of these; 0 (fp32) is what a zero-initialised struct means. */
enum { T3D_F32 = 0, T3D_BF16 = 1 };

/* Arithmetic of an fp32 (dtype = T3D_F32) per-point GEMM launch -- the `arith` field of the GEMM argument structs:
 *   T3D_ARITH_FP32_MFMA  v_mfma_f32_32x32x2_f32: the fp32 fma chain, 157 TFLOP/s peak
 *   T3D_ARITH_BF16X3     every fp32 operand as the exact sum of three bf16 terms, six v_mfma_f32_32x32x16_bf16 per multiply-add with
 *                        fp32 accumulation (csrc/pointmlp.hip, "fp32 GEMMs on the bf16 matrix pipe"); a launch whose shape has no such
 *                        kernel, or for which the launcher's rule prefers the fp32 MFMA (t3d_gemm_arithmetic says which), takes that.
 *                        Two differences from the fp32 MFMA a caller should know: an operand of magnitude >= 3.39e38 (above bf16's
 *                        largest finite value; fp32 itself reaches 3.40e38) has an infinite leading term and yields inf / NaN where
 *                        the fma chain would still be finite; and the bf16 MFMA's accumulation is not rounded to nearest -- results
 *                        lie a little below the exact sum (about -3e-7 of the mean |dW| on a 32768-row weight gradient, bounded in
 *                        tests/test_kernels_gpu.py), where the fma chain shows no offset
 *   T3D_ARITH_AUTO       (0, a zero-initialised struct) the library's default = T3D_ARITH_BF16X3; the only value for which the
 *                        experiment variables T3D_X3 / T3D_X3_MINKN of the tools are consulted
 * A host fixes the value when it builds its plan (transferable3d_amd.engine.Runtime.gemm_arithmetic), so a captured graph, an eager
 * launch and the line bench.py prints cannot disagree.  Ignored by T3D_BF16 launches. */
enum { T3D_ARITH_AUTO = 0, T3D_ARITH_FP32_MFMA = 1, T3D_ARITH_BF16X3 = 2, T3D_ARITH_BF16 = 3 };
/* The arithmetic a per-point GEMM launch of this request takes: T3D_ARITH_FP32_MFMA, T3D_ARITH_BF16X3 or T3D_ARITH_BF16 (dtype =
 * T3D_BF16).  K x N: the layer's weight matrix (a Gram-form launch: N = K); backward != 0: a data / weight gradient launch. */
/* `kind`: which launcher is asked (0 and 1 are what round 5's `backward` flag meant) */
enum { T3D_GEMM_FWD = 0, T3D_GEMM_BWD = 1, T3D_GEMM_DGRAD = 2, T3D_GEMM_WGRAD = 3, T3D_GEMM_GRAM = 4, T3D_GEMM_DGRAD_GRAM = 5 };
int t3d_gemm_arithmetic(int arith, int dtype, int K, int N, int kind);

int t3d_abi_version(void);
/* Hash (16 hex digits + NUL) over the HIP sources and this header the library was built from (csrc/version.hip; "unknown" for a
 * build outside transferable3d_amd/build.py).  `cap` >= 17.  The host side refuses a library whose hash differs from the sources
 * next to it (abi.load). */
int t3d_source_hash(char* out, int cap);

/* ---- operand descriptors ------------------------------------------------------------------ */

/* A per-point activation operand produced lazily from the RAW output of the previous layer:
 *   a[m,k] = relu?( x[m, coff+k] * scale[k] + shift[k] ) - sub[b(m), k]
 * scale/shift (batch-norm apply, tf_util.py:1316-1322) and sub (per-frustum recentring,
 * semisup_models.py:159,207) are optional (NULL).  ldx and coff must be multiples of 4 (of 8 for a T3D_BF16 source: 16-byte reads). */
typedef struct {
  const float* x;
  int ldx;
  int coff;
  const float* scale;
  const float* shift;
  int relu;
  const float* sub;      /* [B, sub_ld] */
  int sub_ld;
  int dtype;             /* element type of x (T3D_F32 / T3D_BF16: `x` then points at bf16 elements; ldx, coff in elements) */
} t3d_act_src;

/* The gradient w.r.t. a layer's RAW conv output, produced lazily while loading:
 *   dy[m,n] = coef[0,n]*dz[m,n] + coef[1,n]*y[m,n] + coef[2,n]
 * (training-mode batch-norm backward folded into three per-channel constants by
 * t3d_bn_bwd_finalize).  dz is either dense [M,N] or, for a max-pooled layer, sparse:
 * dz[m,n] = dpool[b,n] if argidx[b,n] == m - b*rows_per_frustum else 0. */
typedef struct {
  const float* dz;        /* dense [M,N], or NULL for the pooled-sparse form */
  const float* y;         /* [M,N] raw conv output of this layer */
  const float* coef;      /* [3,N] */
  const int32_t* argidx;  /* [B,N] (pooled-sparse form) */
  const float* dpool;     /* [B,N] (pooled-sparse form) */
  int dtype;              /* element type of dz and y; T3D_BF16 supports the dense form only (pooled layers: K11e) */
} t3d_dy_src;

/* ---- K1: per-point shared-MLP layer, forward ---------------------------------------------------
 * Replaces tf_util.conv2d's tf.nn.conv2d(1x1 | [1,D], VALID) + bias_add (tf_util.py:1308-1314) at
 * semisup_models.py:76-95,115-130 (seg), 172-183 (T-Net), 224-239 (box), 354-369 (Box-PC); the
 * batch-norm + ReLU of the PREVIOUS layer is applied while loading `a` (t3d_act_src), this layer's
 * batch-norm statistics are reduced in the epilogue, and conv6's tile+concat of the global feature
 * (semisup_models.py:107-108) enters as the per-frustum `rowbias` (= global . W[64:]).
 *   y[m,n] = sum_k a[m,k] w[k,n] + bias[n] + rowbias[b(m), n]
 *   psum[t,n] = sum_{m in tile t} y[m,n];  psumsq[t,n] = sum y^2
 * Optional max-pool partials over the rows with rowmask != 0 (tf_util.max_pool2d over N after the
 * mask multiply, semisup_models.py:96,184-188,240-244,375): per tile the max and min of raw y and
 * their row indices within the frustum (the finalize kernel picks max or min by the sign of the
 * batch-norm scale). */
typedef struct {
  uint32_t struct_size;    /* = sizeof(t3d_pointmlp_fwd_args) of the caller's header (see T3D_ABI_VERSION) */
  t3d_act_src a;
  const float* w;        /* [K,N] */
  const float* bias;     /* [N] or NULL */
  const float* rowbias;  /* [B,N] or NULL */
  float* y;              /* [M,N], or NULL: statistics and pool partials only (Gram-form backward) */
  float* psum;           /* [M/128, N] */
  float* psumsq;         /* [M/128, N] */
  const float* rowmask;  /* [M] or NULL (pool over all rows) */
  float* pmax;           /* [M/128, N] or NULL (no pooling) */
  float* pmin;
  int32_t* pamax;
  int32_t* pamin;
  int M, K, N;
  int rows_per_frustum;
  int dtype;             /* element type of y and arithmetic of the GEMM (a.dtype may still be T3D_F32: the raw inputs) */
  /* optional (fp32 layers on the three-term bf16 path): the same [K,N] matrix already split into three bf16 planes IN FRAGMENT ORDER,
   * FORWARD arrangement (t3d_split_x3_frag: planes_fwd + the matrix's offset), plane p at w_x3 + p * w_x3_stride (bf16 elements).
   * The kernel then reads the weight operand of every MFMA straight from these planes (one 16-byte load per lane), without an LDS
   * image.  NULL: the kernel splits w while it stages it through LDS -- same results bit for bit.  (ABI version 3: until version 2 the
   * planes were row-major copies of w, t3d_split_x3.) */
  const void* w_x3;
  int64_t w_x3_stride;
  int arith;               /* T3D_ARITH_* (fp32 launches) */
} t3d_pointmlp_fwd_args;
int t3d_pointmlp_fwd(const t3d_pointmlp_fwd_args* args, t3d_stream_t stream);

/* ---- K2: batch-norm statistics -> per-channel scale/shift (+ EMA) ------------------------------
 * Replaces tf.contrib.layers.batch_norm (tf_util.py:1660-1664; eps 1e-3, updates_collections=None).
 * Training: mean/biased variance from the partials, scale = gamma/sqrt(var+eps),
 * shift = beta - mean*scale, moving <- moving*decay + batch*(1-decay) (variance Bessel-corrected
 * when `unbiased_ema`).  Eval: scale/shift from the moving statistics.  `decay` is a DEVICE scalar
 * (it follows the step counter under graph replay). */
typedef struct {
  const float* psum;
  const float* psumsq;
  int n_tiles;
  int count;             /* rows reduced = M */
  int N;
  const float* gamma;
  const float* beta;
  float* moving_mean;
  float* moving_var;
  const float* decay;    /* device scalar */
  float eps;
  int is_training;
  int unbiased_ema;
  float* scale;          /* [N] out */
  float* shift;          /* [N] out */
  float* mean;           /* [N] out (saved for backward) */
  float* invstd;         /* [N] out */
  /* optional: K3 (t3d_pool_finalize) for the same channels in the same launch; pool_pmax == NULL: none */
  const float* pool_pmax; const float* pool_pmin; const int32_t* pool_pamax; const int32_t* pool_pamin;
  int pool_B, pool_tiles_per_frustum;
  float* pooled; int ld_pooled;      /* [B, ld_pooled] */
  int32_t* argidx;                   /* [B,N] */
  float* ysel;                       /* [B,N] */
} t3d_bn_fwd_finalize_args;
int t3d_bn_fwd_finalize(const t3d_bn_fwd_finalize_args* args, t3d_stream_t stream);

/* ---- K3: masked global max-pool finalize -------------------------------------------------------
 * pooled[b,n] = max_m mask*relu(scale*y+shift)  (tf_util.py:1519-1523 after semisup_models.py:185).
 * argidx[b,n] = row (within the frustum) that receives the gradient, -1 when pooled == 0. */
typedef struct {
  const float* scale;
  const float* shift;
  const float* pmax;
  const float* pmin;
  const int32_t* pamax;
  const int32_t* pamin;
  int B, N, tiles_per_frustum;
  float* pooled;         /* [B, ld_pooled] */
  int ld_pooled;
  int32_t* argidx;       /* [B,N] */
  float* ysel;           /* [B,N] raw y at argidx */
} t3d_pool_finalize_args;
int t3d_pool_finalize(const t3d_pool_finalize_args* args, t3d_stream_t stream);

/* ---- K11a: per-point layer, data gradient ------------------------------------------------------
 * The dgrad twin of K1 (autodiff of tf_util.conv2d, train_semisup.py:249):
 *   da[m,k] = sum_n dy[m,n] w[k,n]  (+ add_in[m,k])
 * and, when the producer of `a` has batch-norm + ReLU (prev_y != NULL), the ReLU mask and the
 * producer's batch-norm-backward partials in the epilogue:
 *   out = da * 1[prev_y*prev_scale + prev_shift > 0];  psum_dz = sum out;  psum_dzy = sum out*prev_y */
typedef struct {
  uint32_t struct_size;    /* = sizeof(t3d_pointmlp_dgrad_args) of the caller's header (see T3D_ABI_VERSION) */
  t3d_dy_src dy;
  const float* w;          /* [K,N] */
  const float* add_in;     /* [M,K] or NULL */
  const float* prev_y;     /* [M,K] or NULL */
  const float* prev_scale; /* [K] */
  const float* prev_shift; /* [K] */
  float* out;              /* [M,K] */
  float* psum_dz;          /* [M/128,K] or NULL */
  float* psum_dzy;         /* [M/128,K] or NULL */
  int M, K, N;
  int rows_per_frustum;
  int dtype;               /* element type of prev_y, out and add_in, and the arithmetic; must equal dy.dtype */
  const void* w_x3;        /* optional: w as three bf16 fragment-order planes, DATA-GRADIENT arrangement (t3d_split_x3_frag: planes_dgrad + offset) */
  int64_t w_x3_stride;
  int arith;               /* T3D_ARITH_* (fp32 launches) */
} t3d_pointmlp_dgrad_args;
int t3d_pointmlp_dgrad(const t3d_pointmlp_dgrad_args* args, t3d_stream_t stream);

/* ---- K11b: per-point layer, weight gradient (split over rows) ----------------------------------
 *   slab[s,k,n] = sum_{m in split s} a[m,k] dy[m,n],  s = 0 .. M/rows_per_split - 1
 * t3d_reduce_slabs sums the slabs in a fixed order (deterministic). rows_per_split % 32 == 0. */
typedef struct {
  uint32_t struct_size;    /* = sizeof(t3d_pointmlp_wgrad_args) of the caller's header (see T3D_ABI_VERSION) */
  t3d_act_src a;
  t3d_dy_src dy;
  float* slabs;            /* [M/rows_per_split, K, N] */
  int M, K, N;
  int rows_per_frustum;
  int rows_per_split;      /* the arithmetic follows dy.dtype (bf16: rows_per_split % 64 == 0); slabs are fp32 either way */
  int arith;               /* T3D_ARITH_* (fp32 launches) */
} t3d_pointmlp_wgrad_args;
int t3d_pointmlp_wgrad(const t3d_pointmlp_wgrad_args* args, t3d_stream_t stream);
/* K11a + K11b of one dense layer in ONE launch (the two are independent; sharing a launch saves a kernel's fill/drain
 * latency per layer and lets both kinds of tile share the CUs).  Same arguments and results as the two separate calls;
 * dense dy only (dy.dz != NULL in both), same M, K, N. */
int t3d_pointmlp_bwd(const t3d_pointmlp_dgrad_args* dgrad, const t3d_pointmlp_wgrad_args* wgrad, t3d_stream_t stream);
/* Recommended row split (and the tile the launcher will then use) for a K x N weight gradient over M rows.  One exception: a
 * T3D_BF16 source with K % tile_k != 0 (K = 192, 320, ...) runs 64-row k-tiles, since its loader neither clamps nor masks columns. */
int t3d_wgrad_plan(int M, int K, int N, int* rows_per_split, int* tile_k, int* tile_n);
/* Recommended row split for t3d_pointmlp_bwd.  bf16 layers (dtype = T3D_BF16 for dy, the input and the output) with K and N in
 * {64, 128}, or K x N = 256 x 128 / 128 x 256, run ONE-PASS (*one_pass = 1): one workgroup per split walks its 128-row tiles, reads dz, y and the input once, keeps
 * dW in registers across the tiles and writes one slab at the end; t3d_pointmlp_bwd takes that form whenever the shape is eligible
 * and M / rows_per_split >= min(256, M / 128).  Everything else: t3d_wgrad_plan's split (*one_pass = 0).  The results are those of
 * the two separate calls up to the fp32 summation order.  fp32 layers with K, N in {64, 128} have a one-pass form too (64-row tiles); it is
 * planned when a workgroup gets at least 256 rows (M >= 65536) or when M < 32768 -- at M = 32768 the split form ties and stays. */
int t3d_bwd_plan(int M, int K, int N, int dtype, int* rows_per_split, int* one_pass);

/* ---- K11c: batch-norm backward statistics -> dgamma, dbeta and the three dy coefficients -------
 * dense form: from the dgrad epilogue partials.  pooled form (psum_dz == NULL): from the gradient
 * of the pooled feature, dpool_in[B,N]; writes the ReLU-masked dpool[B,N] the sparse dy form reads.
 * `frozen` (eval-mode batch-norm, stage c): dy = scale*dz, no batch terms, no dgamma/dbeta. */
typedef struct {
  const float* psum_dz;
  const float* psum_dzy;
  int n_tiles;
  const float* dpool_in;   /* [B, ld_dpool_in] (pooled form) */
  int ld_dpool_in;
  const float* pooled;     /* [B, ld_pooled] */
  int ld_pooled;
  const float* ysel;       /* [B,N] */
  float* dpool;            /* [B,N] out */
  int B;
  int count;               /* M */
  int N;
  const float* gamma;
  const float* mean;
  const float* invstd;
  const float* scale;      /* used when frozen */
  int frozen;
  float* dgamma;           /* [N] or NULL */
  float* dbeta;            /* [N] or NULL */
  float* coef;             /* [3,N] */
} t3d_bn_bwd_finalize_args;
int t3d_bn_bwd_finalize(const t3d_bn_bwd_finalize_args* args, t3d_stream_t stream);

/* Per-frustum column sums of a dense dy, from partials only:
 *   out[b,n] = alpha * ( coef0*sum_dz + coef1*sum_y + coef2*rows_per_frustum )
 * (gradient of a per-frustum broadcast: conv6's global feature, semisup_models.py:107-108, and
 * box_est's `xyz - stage1_center`, semisup_models.py:207). */
typedef struct {
  const float* psum_dz;    /* [M/128,N] */
  const float* psum_y;     /* [M/128,N] forward psum of the same layer */
  const float* coef;       /* [3,N] */
  int B, N, tiles_per_frustum, rows_per_frustum;
  float alpha;
  float* out;              /* [B,N] */
} t3d_dy_colsum_args;
int t3d_dy_colsum(const t3d_dy_colsum_args* args, t3d_stream_t stream);

/* ---- K11e: backward of a max-pooled layer in "Gram form" ------------------------------------------
 * The three pooled layers (seg conv5 128->1024, T-Net conv3 128->256, box conv4 256->512;
 * semisup_models.py:92-96, 180-188, 236-244) are the widest of their nets.  Their dy is
 *   dy = c0*dz_sparse + c1*y + c2   with  y = a.w + bias  and dz_sparse non-zero in one row per (b,n),
 * so both gradients factor through the K x K Gram matrix of the layer INPUT and never touch [M,N]:
 *   da = a.P + rowconst + S          P = w diag(c1) w^T,  rowconst = w.(c1*bias + c2)
 *        S[m,:] = sum_{n : argidx[b,n] = m - b*rpf} dpool[b,n] * wc[n,:],   wc[n,k] = c0[n]*w[k,n]
 *   dw = c1*(G.w + abar (x) bias) + abar (x) c2 + c0 * sum_b dpool[b,n] * a[b*rpf + argidx[b,n], :]
 *        G = a^T a,  abar = column sums of a
 * which replaces 4*M*K*N flops by 4*M*K*K and lets the forward pass skip the [M,N] store (y = NULL
 * in t3d_pointmlp_fwd).  Same autodiff semantics as K11a/K11b (train_semisup.py:249). */
typedef struct {
  const float* w;          /* [K,N] */
  const float* bias;       /* [N] or NULL */
  const float* coef;       /* [3,N] from t3d_bn_bwd_finalize */
  int K, N;
  float* p_slabs;          /* [ceil(N/128), K, K] out: partial P per chunk of 128 columns n (sum with t3d_reduce_slabs) */
  float* rc_slabs;         /* [ceil(N/128), K] out: partial rowconst */
  float* wc;               /* [N,K] out, or NULL */
} t3d_pool_bwd_prep_args;
int t3d_pool_bwd_prep(const t3d_pool_bwd_prep_args* args, t3d_stream_t stream);

typedef struct {
  const int32_t* argidx;   /* [B,N] row within the frustum, -1 = no gradient */
  const float* dpool;      /* [B,N] */
  const float* wc;         /* [N,K] */
  int B, N, K;
  int rows_per_frustum;
  float* s;                /* [B*rows_per_frustum, K] out (every row written when row_live is NULL) */
  int32_t* row_live;       /* [B*rows_per_frustum] out or NULL: 1 where the row received a hit, else 0.  When given, rows of `s`
                            * without a hit are NOT written (a few percent of the rows carry arg-max hits; the dense zero rows
                            * were most of this kernel's HBM traffic) and the reader must gate on it (add_live below). */
} t3d_pool_sparse_rows_args;
int t3d_pool_sparse_rows(const t3d_pool_sparse_rows_args* args, t3d_stream_t stream);

/* out = (a.p + rowconst + add_in) * 1[prev_y*prev_scale + prev_shift > 0], with the producer's
 * batch-norm-backward partials, exactly like the epilogue of K11a. */
typedef struct {
  uint32_t struct_size;    /* = sizeof(t3d_pointmlp_dgrad_gram_args) of the caller's header (see T3D_ABI_VERSION) */
  t3d_act_src a;           /* [M,K] input of the pooled layer */
  const float* p;          /* [K,K] */
  const float* rowconst;   /* [K] or NULL */
  const float* add_in;     /* [M,K] or NULL (the sparse rows S) */
  const int32_t* add_live; /* [M] or NULL: add_in is read only on rows whose flag is non-zero (row_live of t3d_pool_sparse_rows) */
  const float* prev_y;     /* [M,K] or NULL */
  const float* prev_scale;
  const float* prev_shift;
  float* out;              /* [M,K] */
  float* psum_dz;          /* [M/128,K] or NULL */
  float* psum_dzy;
  int M, K;
  int rows_per_frustum;
  int dtype;               /* element type of prev_y and out, and the arithmetic (a.dtype gives the operand's); add_in with
                            * add_live (the sparse rows S) is fp32 either way, a dense add_in has this type */
  int arith;               /* T3D_ARITH_* (fp32 launches) */
} t3d_pointmlp_dgrad_gram_args;
int t3d_pointmlp_dgrad_gram(const t3d_pointmlp_dgrad_gram_args* args, t3d_stream_t stream);

/* slab[s] = a_s^T a_s over the rows of split s; rows_per_split from t3d_wgrad_plan(M, K, K). */
typedef struct {
  uint32_t struct_size;    /* = sizeof(t3d_pointmlp_gram_args) of the caller's header (see T3D_ABI_VERSION) */
  t3d_act_src a;
  float* slabs;            /* [M/rows_per_split, K, K] */
  int M, K;
  int rows_per_frustum;
  int rows_per_split;      /* the arithmetic follows a.dtype */
  int arith;               /* T3D_ARITH_* (fp32 launches) */
} t3d_pointmlp_gram_args;
int t3d_pointmlp_gram(const t3d_pointmlp_gram_args* args, t3d_stream_t stream);

/* Recommended row split of the Gram slabs.  bf16 inputs with K = 128 or 256 take the ONE-PASS kernels (*one_pass = 1): t3d_pointmlp_gram
 * / stage 1 with one workgroup per split (the input read and activated once, the per-tile column sums of t3d_act_colsum from the same
 * pass) whenever M / rows_per_split >= min(256, M / 128); t3d_pointmlp_dgrad_gram / stage 2 likewise when prev_y is the input
 * tensor itself (a.x, dense rows) and add_in is absent or the sparse form (add_live).  Otherwise t3d_wgrad_plan(M, K, K)'s split. */
int t3d_gram_plan(int M, int K, int dtype, int* rows_per_split, int* one_pass);

/* part[t,k] = sum over the 128 rows of tile t of a[m,k]. */
typedef struct {
  t3d_act_src a;
  int M, K;
  int rows_per_frustum;
  float* part;             /* [M/128, K] */
} t3d_act_colsum_args;
int t3d_act_colsum(const t3d_act_colsum_args* args, t3d_stream_t stream);

typedef struct {
  t3d_act_src a;
  const int32_t* argidx;   /* [B,N] */
  const float* dpool;      /* [B,N] */
  const float* coef;       /* [3,N] */
  const float* w;          /* [K,N] */
  const float* bias;       /* [N] or NULL */
  const float* g;          /* [K,K] reduced Gram matrix */
  const float* abar;       /* [K] column sums of a (t3d_act_colsum partials, reduced) */
  int B, K, N;
  int rows_per_frustum;
  float* dw;               /* [K,N] out */
} t3d_pool_wgrad_finish_args;
int t3d_pool_wgrad_finish(const t3d_pool_wgrad_finish_args* args, t3d_stream_t stream);

/* The K11e launches that are independent of each other, fused (same arguments and results as the separate calls):
 * stage 1 = t3d_pointmlp_gram + t3d_act_colsum + t3d_pool_bwd_prep; after the slab reduction,
 * stage 2 = t3d_pool_wgrad_finish + t3d_pointmlp_dgrad_gram. */
int t3d_pool_bwd_stage1(const t3d_pointmlp_gram_args* gram, const t3d_act_colsum_args* colsum,
                        const t3d_pool_bwd_prep_args* prep, t3d_stream_t stream);
int t3d_pool_bwd_stage2(const t3d_pool_wgrad_finish_args* finish, const t3d_pointmlp_dgrad_gram_args* dgrad,
                        t3d_stream_t stream);

/* ---- K6: per-frustum fully-connected layer -----------------------------------------------------
 * Replaces tf_util.fully_connected (tf_util.py:1463-1499: matmul + bias [+ batch_norm over the B
 * rows] [+ activation]) and the tf_util.dropout that follows it in mlps_with_dropout /
 * combined_box_pc_mask_features_model (semisup_models.py:56-62, 385-390).
 *   y = [in | in2] . w + bias ; z = BN(y) ; out = dropout(act(z)) (+ add_in on the first add_n cols)
 * drop_mask holds 0/1 keep flags; out *= mask/keep_prob. */
typedef struct {
  const float* in;  int ld_in;  int K;
  const float* in2; int ld_in2; int K2;      /* optional concat (one_hot_vec), K2 = 0 if none (in2 is then not read, whatever it holds) */
  const float* w;                            /* [K+K2, N]; NULL = identity (K == N, K2 == 0): y = in, i.e. a standalone
                                              * tf_util.batch_norm_for_fc (tf_util.py:1666-1677) / tf_util.dropout (1720-1741) node */
  const float* bias;                         /* [N] or NULL */
  const float* gamma; const float* beta;     /* NULL -> no batch-norm */
  float* moving_mean; float* moving_var;
  const float* decay;                        /* device scalar */
  float eps; int is_training; int unbiased_ema;
  int act; float leaky_alpha;
  const float* drop_mask; float keep_prob;   /* [B,N] or NULL */
  const float* add_in; int ld_add; int add_n;
  float* y;                                  /* [B,N] raw (pre-BN), may be NULL when no BN */
  float* out; int ld_out;                    /* [B, ld_out] */
  float* mean; float* invstd;                /* [N] saved for backward */
  int B, N;
} t3d_fc_fwd_args;
int t3d_fc_fwd(const t3d_fc_fwd_args* args, t3d_stream_t stream);

/* Backward of one fully-connected layer for all of its columns.  The incoming gradient w.r.t. `out`
 * is either `dout` or formed on the fly as dy_next . w_next^T (the next layer's input gradient).
 * Writes dy (grad w.r.t. the raw matmul output), dW, dbias, dgamma, dbeta. */
typedef struct {
  const float* dout; int ld_dout;                         /* [B, ld_dout] or NULL */
  const float* dy_next; const float* w_next; int N_next;  /* [B,N_next], [*, N_next] rows 0..N-1 */
  const float* in;  int ld_in;  int K;
  const float* in2; int ld_in2; int K2;
  const float* y; const float* out; int ld_out;
  const float* gamma; const float* beta; const float* mean; const float* invstd;
  int bn_training;                                         /* 0: gamma*invstd only (frozen): dy = gamma * invstd * dz.  With batch-norm and
                                                            * bn_training == 0, dbias is written as 0 and dgamma / dbeta are left untouched --
                                                            * not the gradients of a frozen layer's parameters (those would be sum dz * gamma *
                                                            * invstd, sum dz * xhat, sum dz).  No plan asks for them: a frozen net runs without
                                                            * parameter gradients (dw = dbias = dgamma = dbeta = NULL). */
  int act; float leaky_alpha;
  const float* drop_mask; float keep_prob;
  float* dy;                                               /* [B,N] */
  float* dw; float* dbias; float* dgamma; float* dbeta;    /* NULL -> not computed (frozen net) */
  int B, N;
} t3d_fc_bwd_args;
int t3d_fc_bwd(const t3d_fc_bwd_args* args, t3d_stream_t stream);

/* din[b,k] = alpha * sum_n dy[b,n] w[k,n] (+ add_in[b,k]) : the input gradient of an FC layer
 * (pooled-feature gradient, stage1_center gradient, global-feature gradient). */
typedef struct {
  const float* dy; int N;       /* [B,N] */
  const float* w;               /* [K,N] */
  const float* add_in; int ld_add;
  float alpha;
  float* din; int ld_din;
  int B, K;
  /* optional: the pooled form of K11c (t3d_bn_bwd_finalize) on din's columns in the same launch -- din is the gradient
   * of a max-pooled feature and column k is all that channel k's batch-norm backward needs; bn_coef == NULL: none */
  const float* bn_pooled; int bn_ld_pooled;   /* [B, ld] */
  const float* bn_ysel;                       /* [B,K] */
  float* bn_dpool;                            /* [B,K] out */
  int bn_count;
  const float* bn_gamma; const float* bn_mean; const float* bn_invstd; const float* bn_scale;
  int bn_frozen;
  float* bn_dgamma; float* bn_dbeta;          /* [K] or NULL */
  float* bn_coef;                             /* [3,K] out */
} t3d_fc_dinput_args;
int t3d_fc_dinput(const t3d_fc_dinput_args* args, t3d_stream_t stream);

/* ---- K5 + K7 + K10: segmentation head, forward + backward in one pass --------------------------
 * Replaces, for the last seg layer: tf_util.dropout (semisup_models.py:131), conv10 128->2 without
 * BN/activation (133-135), sparse_softmax_cross_entropy_with_logits (semisup_v1_sunrgbd.py:430),
 * the hard mask and masked xyz sums of subtract_points_mean (semisup_models.py:150-158), and their
 * gradients back to conv9's batch-norm output.
 * Per-frustum loss weight: w_b = ce_weight * (1 - is_data_2D[b]) / (B * rows_per_frustum). */
typedef struct {
  uint32_t struct_size;    /* = sizeof(t3d_seg_head_args) of the caller's header (see T3D_ABI_VERSION) */
  const float* y;            /* [M,K] raw conv9 output */
  const float* scale; const float* shift;
  const float* drop_mask;    /* [M,K] 0/1 or NULL */
  float keep_prob;
  const float* w;            /* [K,2] */
  const float* bias;         /* [2] */
  const int32_t* labels;     /* [M] or NULL (inference) */
  const int32_t* is_data_2D; /* [B] */
  const float* pc; int ld_pc;/* [M, ld_pc] xyz in cols 0..2 */
  float ce_weight;
  float* logits;             /* [M,2] */
  float* mask;               /* [M] */
  float* part;               /* [M/128, 8]: ce_sum, mask_cnt, sx, sy, sz, db0, db1, n_correct */
  float* dz;                 /* [M,K] grad wrt conv9 BN output (ReLU-masked) or NULL (no backward) */
  float* psum_dz;            /* [M/128,K] */
  float* psum_dzy;           /* [M/128,K] */
  float* dw_part;            /* [M/128,K,2] */
  int M, K, rows_per_frustum, B;
  /* drop_mask == NULL, keep_prob < 1, drop_hyper != NULL: the keep mask is generated where it is consumed, element (m,k) from
   * (drop_seed, step = drop_hyper[0], index m*K + k) with the generator of t3d_dropout_mask -- no [M,K] mask tensor in HBM. */
  uint32_t drop_seed;
  const float* drop_hyper;
  int dtype;                 /* element type of y and dz (T3D_F32 / T3D_BF16) */
  /* optional: d loss / d soft_mask[m] (soft_mask = softmax(logits)[:,1]) from t3d_weak_loss, added to the logit gradients -- the
   * head is then run a second time, behind the box losses, and rewrites dz, the partials and dw_part (NULL: none) */
  const float* dsoft;        /* [M] or NULL */
  /* optional: the `oracle_mask` of get_semi_model_final (semisup_v1_sunrgbd.py:161-162; test_semisup.py:75 feeds y_seg): the
   * logits that leave the head -- written, masked on, fed to the cross-entropy -- are stack([1 - m, m]) instead of conv10's; no
   * gradient reaches conv9 then (the stacked tensor is a constant of the graph). */
  const int32_t* oracle_mask; /* [M] or NULL */
} t3d_seg_head_args;
int t3d_seg_head(const t3d_seg_head_args* args, t3d_stream_t stream);

/* Combines the seg-head tile partials per frustum: mask_xyz_mean[B,3] (semisup_models.py:157-158),
 * seg CE per frustum (mean over points), and the conv10 weight/bias gradient. */
typedef struct {
  const float* part; const float* dw_part;
  int B, tiles_per_frustum, rows_per_frustum, K;
  float* mask_xyz_mean;      /* [B,3] */
  float* seg_loss;           /* [B] mean CE per frustum */
  float* dw;                 /* [K,2] or NULL */
  float* dbias;              /* [2] or NULL */
  float* n_correct;          /* [1] or NULL */
} t3d_seg_finalize_args;
int t3d_seg_finalize(const t3d_seg_finalize_args* args, t3d_stream_t stream);

/* ---- K9 + K10: box losses, forward + backward ---------------------------------------------------
 * Replaces get_strong_loss (semisup_v1_sunrgbd.py:423-553), huber_loss (555-564), the corner boxes of
 * model_util.get_box3d_corners_sunrgbd / _helper (model_util.py:94-119,145-167) and the anchor->reg
 * conversion tf_convert_box_params_from_anchor_to_reg_format_multi (tf_util.py:1001-1041), for the
 * 67-wide head output `box` and the T-Net centre.  total[b] = w3d[b]*(seg_w*seg_loss[b] + box_l[b]),
 * loss = sum_b total[b] * (mean_over_B ? 1/B : 1/(sum w3d + 1e-3)).   w3d = 1 - is_data_2D. */
typedef struct {
  float center, orient_cls, orient_reg, dims_cls, dims_reg, tnet_center, corner, box_multiplier,
        cross_entropy;
} t3d_strong_weights;
typedef struct {
  const float* box; int ld_box;          /* [B,67] head output (centre residual first), rows ld_box >= 67 floats apart (less: T3D_ERR_SHAPE) */
  const float* stage1_center;            /* [B,3] */
  const float* seg_loss;                 /* [B] or NULL */
  const float* y_center; const int32_t* y_orient_cls; const float* y_orient_reg;
  const int32_t* y_dims_cls; const float* y_dims_reg; const int32_t* is_data_2D;
  t3d_strong_weights wts;
  int normalize_by_3d_count;             /* 0: mean over B (model A); 1: /(sum w3d + 1e-3) (model F) */
  float* dbox;                           /* [B,67] */
  float* dstage1;                        /* [B,3] */
  float* terms;                          /* [B,8]: mask, center, stage1, hcls, hres, scls, sres, corner */
  float* total_losses;                   /* [B] */
  float* loss;                           /* [1] */
  float* center;                         /* [B,3] end_points['center'] */
  float* reg_dims;                       /* [B,3] anchor->reg dims */
  float* reg_theta;                      /* [B] */
  /* optional per-frustum IoU of the predicted box (arg-max bins) with the label box: the tf.py_func summary
   * get_iou_summary / compute_box3d_iou (semisup_v1_sunrgbd.py:236-246, roi_seg_box3d_dataset.py:103-140).  NULL: skipped. */
  float* iou2d;                          /* [B] ground-plane IoU */
  float* iou3d;                          /* [B] */
  int B;
} t3d_strong_loss_args;
int t3d_strong_loss(const t3d_strong_loss_args* args, t3d_stream_t stream);

/* ---- K9b: weak box losses of get_semi_loss_backbone, forward + backward ------------------------------------------------
 * Replaces weak_losses.get_reprojection_loss (models/weak_losses.py:69-229, with tf_util.tf_rot_box_params_multi 1045-1072,
 * tf_create_3D_box_by_vertices_multi 841-891, tf_get_2D_bbox_of_(softmax_)projection_sunrgbd_multi 364-449, tf_dilate_2D_bboxes
 * 486-514, tf_clip_2D_bbox_to_image_dims_multi 517-540) and weak_losses.get_surface_loss (231-259, with
 * tf_distance_to_closest_3D_box_surface_multi, tf_util.py:610-719) as called at semisup_v1_sunrgbd.py:270-311 on
 * S_pred_box_reg = (center, reg_dims, reg_theta) -- the outputs of t3d_strong_loss:
 *   weak[b] = w_reproj * reprojection[b] + w_surface * surface[b]
 *   total_losses[b] += is_data_2D[b] * multiplier * weak[b];   loss += mean_b of that term
 *   dbox7[b] = d loss / d (center, reg_dims, reg_theta)[b]     (feed t3d_anchor_reg_bwd)
 *   dsoft[m] = d loss / d soft_mask[m]   (soft_mask = softmax(logits)[:,1]; the reference multiplies the surface loss by the
 *              soft mask itself, so this gradient exists whatever WEAK_TRAIN_SEG_W_SURFACE says: feed t3d_seg_head.dsoft)
 * Run after t3d_strong_loss / t3d_semi_final_loss (in/out: total_losses, loss).  Two launches (per-point surface distances; per-frustum finish).
 * A loss is evaluated whenever its inputs are given (pc + logits; Rtilt .. img_dim), whatever its weight -- the reference logs both. */
typedef struct {
  const float* center;       /* [B,3] */
  const float* reg_dims;     /* [B,3] */
  const float* reg_theta;    /* [B] */
  const float* pc; int ld_pc;/* [B*N, ld_pc] xyz in cols 0..2 (surface loss) */
  const float* logits;       /* [B*N,2] (surface loss) */
  const float* Rtilt;        /* [B,3,3] */
  const float* K;            /* [B,3,3] */
  const float* rot_frust;    /* [B] */
  const float* box2D;        /* [B,4] left, top, right, bottom */
  const float* img_dim;      /* [B,2] rows, cols */
  const int32_t* is_data_2D; /* [B], or NULL: every sample counts (get_semi_loss_final without WEAK_REPROJECTION_ONLY_ON_2D_CLS) */
  float w_reproj, w_surface; /* WEAK_WEIGHT_REPROJECTION, WEAK_WEIGHT_SURFACE */
  float multiplier;          /* SEMI_MULTIPLIER_FOR_WEAK_LOSS */
  int use_softmax_proj; float softmax_scale;      /* WEAK_REPROJECTION_USE_SOFTMAX_PROJ, _SOFTMAX_SCALE */
  float dilate;              /* WEAK_REPROJECTION_DILATE_FACTOR */
  int clip_lower_b_loss, clip_pred_box;           /* WEAK_REPROJECTION_CLIP_LOWERB_LOSS, _CLIP_PRED_BOX */
  int loss_mse;              /* WEAK_REPROJECTION_LOSS_TYPE: 0 huber, 1 mse */
  int32_t train_box_reproj[3];                    /* WEAK_TRAIN_BOX_W_REPROJECTION (centre, dims, theta) */
  int32_t train_box_surface[3];                   /* WEAK_TRAIN_BOX_W_SURFACE */
  float surface_margin, surface_scale_dims;       /* WEAK_SURFACE_MARGIN, WEAK_SURFACE_LOSS_SCALE_DIMS */
  float* surf_part;          /* [B, N/128, 8] scratch */
  float* dsoft;              /* [B*N] out or NULL */
  float* reproj;             /* [B] out or NULL */
  float* surface;            /* [B] out or NULL */
  float* dbox7;              /* [B,7] out */
  float* total_losses;       /* [B] in/out or NULL */
  float* loss;               /* [1] in/out */
  int B, N;
  /* stage c (get_semi_loss_final, semisup_v1_sunrgbd.py:345-359): the inactive-volume loss of the box dims per class
   * (weak_losses.get_inactive_volume_loss_v1, weak_losses.py:39-67): loss += multiplier * w_inactive * mean over the trained classes
   * of mean_{b in class} max(0, margin[class] - l*w*h); its gradient joins dbox7[:,3:6].  w_inactive == 0: none */
  const float* one_hot;      /* [B,10] class one-hot (class_ids = arg-max) or NULL */
  float w_inactive;          /* WEAK_WEIGHT_INACTIVE_VOLUME */
  float inactive_margins[10];/* WEAK_INACTIVE_VOL_LOSS_MARGINS */
  int32_t inactive_train[10];/* end_points['inactive_vol_train_classes'] */
  float* inactive;           /* [1] out or NULL */
} t3d_weak_loss_args;
int t3d_weak_loss(const t3d_weak_loss_args* args, t3d_stream_t stream);

/* ---- K8: Box-PC representation ----------------------------------------------------------------------
 * Replaces tf_get_box_pc_representation (tf_util.py:764-795) + tf_create_3D_box_by_surface_centers_multi
 * (893-955): rep[m, 0:C] = pc[m, 0:C]; rep[m, C:C+6] = the six signed point-to-face distances of point m to the
 * box of its frustum (centre, dims (l,w,h), heading); columns C+6 .. ld_rep-1 are zero padding.
 * Box in regression form (center, dims, theta), or, when y_dims_cls != NULL, in label form: dims/theta hold the
 * residuals and the box is max(anchor[cls] + res, 1e-5) / bin[cls] + res (boxpc_sunrgbd.py:206-230).
 * box_out[B,7] (optional) receives (cx,cy,cz,l,w,h,theta) for the backward.  rows_per_frustum % 256 == 0. */
typedef struct {
  uint32_t struct_size;    /* = sizeof(t3d_boxpc_rep_args) of the caller's header (see T3D_ABI_VERSION) */
  const float* pc; int ld_pc; int C;
  const float* center;            /* [B,3] */
  const float* dims;              /* [B,3] */
  const float* theta;             /* [B]   */
  const int32_t* y_dims_cls;      /* [B] or NULL */
  const int32_t* y_orient_cls;    /* [B] or NULL */
  float* rep; int ld_rep;         /* [M, ld_rep] */
  float* box_out;                 /* [B,7] or NULL */
  int M, rows_per_frustum;
  /* optional: `--mask_pc_for_boxpc` of test_semisup.py:103-105 -- the net sees pc * mask (every channel of a background point is 0,
   * so its six distances are those of the origin) */
  const float* rowmask;           /* [M] 0/1 or NULL */
} t3d_boxpc_rep_args;
int t3d_boxpc_rep(const t3d_boxpc_rep_args* args, t3d_stream_t stream);

/* Representation B (independent_box_pc_mask_features_model, semisup_models.py:400-470) reads the box as a 7-vector and the RAW point
 * cloud, so this writes only that:
 *   box_out[B,7] = (cx,cy,cz,l,w,h,theta) of the box in either form of t3d_boxpc_rep (label form when y_dims_cls != NULL), when
 *                  box_out != NULL (center / dims / theta then required);
 *   pc_out[m, 0:C] = pc[m, 0:C] * rowmask[m] (--mask_pc_for_boxpc, test_semisup.py:103-105; columns C .. ld_out-1 zeroed), when
 *                  rowmask != NULL (pc, pc_out, ld_out >= C required).  Without a row mask the net reads pc in place.
 * At least one of the two; M = B * rows_per_frustum.  (An entry point of its own rather than a field appended to t3d_boxpc_rep_args:
 * that struct keeps its version-2 size, below which a caller's struct is refused.)  Frozen struct. */
typedef struct {
  const float* center;            /* [B,3] */
  const float* dims;              /* [B,3] */
  const float* theta;             /* [B]   */
  const int32_t* y_dims_cls;      /* [B] or NULL */
  const int32_t* y_orient_cls;    /* [B] or NULL */
  float* box_out;                 /* [B,7] or NULL */
  const float* pc; int ld_pc; int C;
  const float* rowmask;           /* [M] 0/1 or NULL */
  float* pc_out; int ld_out;      /* [M, ld_out] */
  int B, rows_per_frustum;
} t3d_boxpc_rep_b_args;
int t3d_boxpc_rep_b(const t3d_boxpc_rep_b_args* args, t3d_stream_t stream);

/* Gradient of the representation w.r.t. the box: dbox[B,7] = d(cx,cy,cz,l,w,h,theta), reduced over the points,
 * from drep[m, coff .. coff+5] = gradient w.r.t. the six distance channels (stage c: train_semisup_adv.py:331-411). */
typedef struct {
  const float* pc; int ld_pc;
  const float* box;               /* [B,7] from t3d_boxpc_rep */
  const float* drep; int ld_drep; int coff;
  float* dbox;                    /* [B,7] */
  int B, rows_per_frustum;
} t3d_boxpc_rep_bwd_args;
int t3d_boxpc_rep_bwd(const t3d_boxpc_rep_bwd_args* args, t3d_stream_t stream);

/* Box-PC loss, forward + backward (boxpc_sunrgbd.py:106-193, huber form): out[B,9] = [dcentre(3), dsize(3), dangle,
 * fit logits(2)];  loss = mean_b( w_cls*CE(logits, iou > fit_bound) + w_delta*wl*(w_center*mean3 Huber + w_size*mean3
 * Huber + w_angle*Huber) ).  terms[B,4] = (CE, delta loss, p_fit, total).
 * weigh_pred_by_cls_conf (BOXPC_WEIGH_DELTA_PRED_BY_CLS_CONF, boxpc_sunrgbd.py:84-92): the Huber terms see the PREDICTED deltas
 * times (1 - p_fit).  grad_cls_via_delta = !BOXPC_STOP_GRAD_OF_CLS_VIA_DELTA (boxpc_sunrgbd.py:73-74): p_fit inside wl / the
 * prediction weight is differentiated (the gradient reaches the fit logits); 0 = stop_gradient, the recipes' setting. */
typedef struct {
  const float* out;               /* [B,9] */
  const float* y_box_iou; const float* y_center_delta; const float* y_dims_delta; const float* y_orient_delta;
  float fit_bound, w_cls, w_delta, w_center, w_size, w_angle;
  int weigh_by_cls_conf, weigh_by_cls_gt;
  float* dout;                    /* [B,9] */
  float* terms;                   /* [B,4] */
  float* loss;                    /* [1] */
  int B;
  int weigh_pred_by_cls_conf, grad_cls_via_delta;
  int delta_loss_mse;             /* BOXPC_DELTA_LOSS_TYPE == 'mse' (boxpc_sunrgbd.py:158-164): squared error instead of Huber */
} t3d_boxpc_loss_args;
int t3d_boxpc_loss(const t3d_boxpc_loss_args* args, t3d_stream_t stream);

/* ---- stage-c glue (SEMI_MODEL F with the frozen Box-PC net; train_semisup_adv.py:331-411) ---------------- */

/* Input gradient of a per-point layer restricted to kn <= 8 input channels k0..k0+kn-1 (dense dy only):
 * out[m, j] = sum_n dy[m,n] w[k0+j, n].  Used for the six distance channels of the Box-PC representation.
 * M % 64 == 0, N % 128 == 0. */
typedef struct {
  t3d_dy_src dy;
  const float* w;          /* [K,N] */
  int k0, kn;
  float* out; int ld_out;  /* [M, ld_out] */
  int M, N;
} t3d_pointmlp_dgrad_narrow_args;
int t3d_pointmlp_dgrad_narrow(const t3d_pointmlp_dgrad_narrow_args* args, t3d_stream_t stream);

/* get_semi_loss_final's weak terms (semisup_v1_sunrgbd.py:343-407) on top of the strong loss already computed by
 * t3d_strong_loss(normalize_by_3d_count = 1):
 *   loss = strong + w_weak * intraclass(reg_dims | class) + w_fit * mean_b(-log(0.01 + p_fit[b]) * (fit_only_2d ? is2D : 1))
 * with w_weak = SEMI_MULTIPLIER_FOR_WEAK_LOSS * WEAK_WEIGHT_INTRACLASSVAR, the intraclass-variance loss of
 * weak_losses.py:267-291 (huber), p_fit = softmax(out9[:,7:9])[:,1].  Writes the gradients w.r.t. reg_dims and out9. */
typedef struct {
  const float* strong_loss;       /* [1] device scalar */
  const float* reg_dims;          /* [B,3] */
  const float* one_hot;           /* [B,10] class one-hot (class_ids = argmax) */
  const int32_t* is_data_2D;      /* [B] */
  const float* out9;              /* [B,9] Box-PC output */
  int32_t train_classes[10];
  float w_weak, w_fit;
  int fit_only_2d;
  float* d_dims;                  /* [B,3] */
  float* dout9;                   /* [B,9] */
  float* fit_prob;                /* [B] end_points['boxpc_fit_prob'] */
  float* terms;                   /* [2]: intraclass loss, fit loss */
  float* loss;                    /* [1] */
  int B;
} t3d_semi_final_loss_args;
int t3d_semi_final_loss(const t3d_semi_final_loss_args* args, t3d_stream_t stream);

/* Backward of the anchor->reg conversion (tf_util.py:1017-1031): accumulates the gradient of (centre, dims, theta)
 * -- dbox7[B,7] from the Box-PC path and/or d_dims[B,3] -- into dbox[B,67] and dstage1[B,3] (both in/out). */
typedef struct {
  const float* box; int ld_box;   /* [B,67] head output (scores pick the bins), rows ld_box >= 67 floats apart (less: T3D_ERR_SHAPE) */
  const float* dbox7;             /* [B,7] or NULL */
  const float* d_dims;            /* [B,3] or NULL */
  float* dbox;                    /* [B,67] in/out */
  float* dstage1;                 /* [B,3] in/out */
  int B;
} t3d_anchor_reg_bwd_args;
int t3d_anchor_reg_bwd(const t3d_anchor_reg_bwd_args* args, t3d_stream_t stream);

/* One step of the iterated Box-PC refinement of the inference graph (test_semisup.py:101-134):
 *   p_fit = softmax(out9[:,7:9])[:,1];  w = (1 - p_fit)^weigh_by_conf, weigh_by_conf = 0, 1 or 2: one factor for
 *   SEMI_WEIGH_BOXPC_DELTA_DURING_TEST (test_semisup.py:119-121), one for BOXPC_WEIGH_DELTA_PRED_BY_CLS_CONF (the Box-PC
 *   model's own weighting of its predicted deltas, boxpc_sunrgbd.py:84-92)
 *   box_out = box_in - w * out9[:,0:7]  (centre 0:3, size 3:6, angle 6);  total (+)= w * out9[:,0:7]  (`first`: =)
 * The F2_ heads are the F_ heads minus `total` (test_semisup.py:136-142). */
typedef struct {
  const float* out9;              /* [B,9] Box-PC net output */
  const float* center_in; const float* dims_in; const float* theta_in;   /* [B,3],[B,3],[B] */
  float* center_out; float* dims_out; float* theta_out;                  /* may alias the inputs */
  float* total;                   /* [B,7] accumulated deltas */
  float* fit_prob;                /* [B] or NULL */
  int weigh_by_conf;
  int first;
  int B;
} t3d_box_refine_step_args;
int t3d_box_refine_step(const t3d_box_refine_step_args* args, t3d_stream_t stream);

/* Backward of one refinement step inside the TRAINING graph (train_semisup_adv.py:362-386 with SEMI_REFINE_USING_BOXPC_DELTA_NUM > 1
 * and SEMI_BOXPC_MIN_FIT_LOSS_AFT_REFINE: the fit loss reads the Box-PC evaluation of the box refined NUM-1 times, so its gradient
 * runs back through every step  box_next = box - w * out9[:,0:7],  w = (1 - p_fit)^weigh_by_conf):
 *   tot = dbox_rep + carry            gradient w.r.t. box_next: through the next evaluation's representation (t3d_boxpc_rep_bwd)
 *                                     + what flows past it to the steps behind (carry, NULL at the last step)
 *   tot_out = tot                     (the identity path: the carry of the step before)
 *   dout9[:,0:7] = -w * tot;  dout9[:,7:9] = (grad_via_conf ? d w / d logits . sum_k tot_k * (-out9_k) : 0)
 * With out9 == NULL only tot_out is written (the total gradient w.r.t. the unrefined box). */
typedef struct {
  const float* out9;              /* [B,9] Box-PC output of THIS step's evaluation, or NULL */
  const float* dbox_rep;          /* [B,7] */
  const float* carry;             /* [B,7] or NULL */
  float* tot_out;                 /* [B,7] (may alias carry or dbox_rep) */
  float* dout9;                   /* [B,9], required with out9 */
  int weigh_by_conf;              /* as t3d_box_refine_step */
  int grad_via_conf;              /* !BOXPC_STOP_GRAD_OF_CLS_VIA_DELTA (boxpc_sunrgbd.py:73-74) */
  int B;
} t3d_box_refine_step_bwd_args;
int t3d_box_refine_step_bwd(const t3d_box_refine_step_bwd_args* args, t3d_stream_t stream);

/* ---- K13: 3-D IoU of upright boxes ---------------------------------------------------------------------
 * Replaces box_util.box3d_iou (the Frustum-PointNets module the reference imports but does not ship) at its call sites:
 * roi_seg_box3d_dataset.py:103-140 (per-step IoU summary), box_pc_fit_dataset.py:38-42,211-244 (perturb a box until its IoU
 * falls inside the fit / no-fit bounds), eval_det.py:60-66 (detection matching).  Ground-plane rectangle intersection (area of
 * the clipped polygon), height overlap, iou3d = inter_vol / (vol1 + vol2 - inter_vol), iou2d = inter / (a1 + a2 - inter).
 * Parameter form: centre (x,y,z), size (l,w,h), heading about y, as get_3d_box takes them (roi_seg_box3d_dataset.py:86-101);
 * negative l / w count by magnitude (a mirrored rectangle), a negative h gives iou3d = 0 (inverted height range), as the
 * reference's get_3d_box + box3d_iou behave on the sizes an untrained head produces. */
typedef struct {
  const float* center1; const float* size1; const float* heading1;      /* [n,3], [n,3], [n] */
  const float* center2; const float* size2; const float* heading2;
  float* iou3d; float* iou2d;                                           /* [n]; iou2d may be NULL */
  int n;
} t3d_box3d_iou_args;
int t3d_box3d_iou(const t3d_box3d_iou_args* args, t3d_stream_t stream);

/* Corner form, box3d_iou's own signature: corners[n,8,3] in get_3d_box order (0-3 the y-max face, 4-7 the y-min face). */
typedef struct {
  const float* corners1; const float* corners2;                         /* [n,8,3] */
  float* iou3d; float* iou2d;
  int n;
} t3d_box3d_iou_corners_args;
int t3d_box3d_iou_corners(const t3d_box3d_iou_corners_args* args, t3d_stream_t stream);

/* The extra fully-connected input columns of v1_tnet / v1_box_est under USE_NORMALIZED_BOX2D_AS_FEATS
 * (semisup_models.py:192-195, 249-252: concat [pooled | one_hot | norm_box2D]): out[B, n_oh + 4] = [one_hot (n_oh = 0 or 10) |
 * tf_util.tf_normalize_2D_bboxes(box2D, img_dim) (tf_util.py:466-484) = left/cols, top/rows, right/cols, bottom/rows with
 * img_dim = (rows, cols)].  Inputs are placeholders: no gradient. */
typedef struct {
  const float* one_hot; int n_oh;        /* [B, n_oh] or NULL with n_oh = 0 */
  const float* box2D;                    /* [B,4] */
  const float* img_dim;                  /* [B,2] */
  float* out;                            /* [B, n_oh + 4] */
  int B;
} t3d_box2d_feats_args;
int t3d_box2d_feats(const t3d_box2d_feats_args* args, t3d_stream_t stream);

/* compute_box3d_iou on raw box heads (roi_seg_box3d_dataset.py:103-140): box[B,67] = [centre - stage1_center (3), heading scores
 * (12), normalised heading residuals (12), size scores (10), normalised size residuals (10x3)]; predicted box from the arg-max
 * bins (class2angle / class2size), label box from the label bins + residuals. */
typedef struct {
  const float* box; int ld_box;
  const float* stage1_center;            /* [B,3] or NULL (centre already absolute) */
  const float* y_center; const int32_t* y_orient_cls; const float* y_orient_reg; const int32_t* y_dims_cls; const float* y_dims_reg;
  float* iou2d; float* iou3d;            /* [B] */
  int B;
} t3d_box_head_iou_args;
int t3d_box_head_iou(const t3d_box_head_iou_args* args, t3d_stream_t stream);

/* ---- device-side batch assembly -------------------------------------------------------------------------------
 * Replaces the host loop ROISemiDataset.get_batch -> get_classes3D (roi_semi_dataset.py:283-347, 482-535; helpers
 * roi_seg_box3d_dataset.py:37-77, 346-368) for a data set of ragged frustums resident in HBM.  Per batch slot b with
 * frustum f = sample[b]: N points drawn with replacement (np.random.choice(count, N, replace=True), 301-303), rotated to
 * the centre view (rot = pi/2 + frustum_angle; [x,z] <- [x c - z s, x s + z c]), flipped in x with probability 1/2,
 * shifted along z by clip(randn*dist*0.05, 0.8 dist, 1.2 dist) with dist = |centre.xy| (the reference's bounds, as
 * written) and along y by U(-0.2, 0.2); labels: rotated/flipped/shifted box centre, heading -> (bin, residual) by
 * angle2class over 12 bins, size -> (class, size - mean size of the class), one-hot class.
 * Draws: `choice` [B,N] and `aug` [B,3] = (flip, randn, u) when given (parity tests), else generated from
 * (seed, hyper[0] = step, b, n) -- so the whole input pipeline can sit inside the captured step.
 * Every frustum a launch can sample holds at least one point (offsets[f+1] > offsets[f]): of a frustum without points the
 * generated draw is row offsets[f], which is the next frustum's, or behind `points` and `seg` for the last one; a given
 * `choice` holds values in [0, count).  Neither is checked on the device (dataset.DeviceFrustumSet refuses such a set).
 * ALTERNATE_BATCH (train_semisup_adv.py:538-565, sample_pure_from_2D_cls / _3D_cls 589-596): see sample2. */
typedef struct {
  const float* points;         /* [total, C_src] all frustums, concatenated; xyz in columns 0..2 */
  const int32_t* seg;          /* [total] per-point labels */
  const int64_t* offsets;      /* [F+1] */
  const float* frustum_angle;  /* [F] */
  const float* box_center;     /* [F,3] */
  const float* heading;        /* [F] */
  const float* size;           /* [F,3] (l,w,h) */
  const int32_t* cls;          /* [F] class id */
  const int32_t* sample;       /* [B] frustum index per batch slot, or (sample_len > 0) a permutation [sample_len] of which slot b
                                  of step s takes entry (s*B + b) mod sample_len */
  int sample_len;
  const int32_t* choice;       /* [B,N] or NULL */
  const float* aug;            /* [B,3] or NULL */
  int C_src, C, B, N;
  int rotate_to_center, random_flip, random_shift;
  uint32_t seed;
  const float* hyper;          /* device step counter (hyper[0]); required when choice == NULL */
  float* pc;                   /* [B,N,C] out */
  int32_t* y_seg;              /* [B,N] out */
  float* y_center;             /* [B,3] */
  int32_t* y_orient_cls;       /* [B] */
  float* y_orient_reg;         /* [B] */
  int32_t* y_dims_cls;         /* [B] */
  float* y_dims_reg;           /* [B,3] */
  float* one_hot;              /* [B,10] */
  float* rot_angle;            /* [B] or NULL */
  const int32_t* sample2;      /* NULL, or the second list of ALTERNATE_BATCH sampling: even steps take slot b from
                                  sample[((s/2)*B + b) mod sample_len] (2-D-label classes, is_data_2D = 1), odd steps from
                                  sample2[((s/2)*B + b) mod sample2_len] (3-D-label classes, is_data_2D = 0) */
  int sample2_len;
  int32_t* is_data_2D;         /* [B] or NULL */
  const int32_t* frustum_is_2D; /* [F] or NULL: per-frustum flag of a combined data set (SEMI_SAMPLING_METHOD BATCH: get_batch walks the
                                  3-D-label list followed by the 2-D-label list, roi_semi_dataset.py:482-535); when given it decides
                                  is_data_2D in the one-list modes */
  int ld_pc;                   /* row stride of pc in floats (>= C; 0 = C).  A multiple of 4 when the layers read pc (C = 6: xyz + rgb
                                  rows padded to 8 floats; the padding is written as zeros) */
  const int32_t* slot_is_2D;   /* [B] or NULL: per-slot flag written earlier in the step by t3d_sample_equal_classes (its is_data_2D)
                                  when neither sample2 nor frustum_is_2D decides */
  /* A slot that holds a frustum of the 2-D-label list is assembled the way ROISemiDataset.get_classes2D does it
   * (roi_semi_dataset.py:383-452): resampled and rotated to the centre view, but NOT flipped or shifted ("2D Classes cannot be
   * augmented because the projection will no longer be accurate"), and every 3-D label (y_seg, y_center, orientation and size
   * class / residual) is written as zero; one_hot and rot_angle are kept. */
  /* optional camera side of the weak losses: per-frustum calibration and 2-D box of the data set (roi_semi_dataset.py:243-246,
   * 355-359) copied to the batch slot (the frustum rotation the reprojection loss undoes is rot_angle).  cam_rtilt == NULL: none */
  const float* cam_rtilt;      /* [F,9] */
  const float* cam_k;          /* [F,9] */
  const float* cam_box2d;      /* [F,4] left, top, right, bottom */
  const float* cam_img_dim;    /* [F,2] rows, cols */
  float* Rtilt;                /* [B,9] out */
  float* K;                    /* [B,9] out */
  float* box2D;                /* [B,4] out */
  float* img_dim;              /* [B,2] out */
} t3d_batch_assemble_args;
int t3d_batch_assemble(const t3d_batch_assemble_args* args, t3d_stream_t stream);

/* Class-balanced batch composition: `equal_samples_per_class` of ROISemiDataset.sample_from_set (roi_semi_dataset.py:558-567) and
 * BoxPCFitDataset.sample_batch (box_pc_fit_dataset.py:367-377).  The B slots are split over the n class groups like
 * np.array_split([1]*B, n) -- B mod n groups get one slot more, WHICH groups is random per step (random.shuffle of the split) --
 * slots are laid out group after group, and each slot draws a frustum of its group with replacement.  Writes sample[B] (the
 * frustum index per slot) for t3d_batch_assemble's explicit-sample mode (sample_len = 0).
 * Two sets = ALTERNATE_BATCH (train_semisup_adv.py:538-565): even steps draw from set[0] (classes with 2-D labels only,
 * is_data_2D = 1), odd steps from set[1] (is_data_2D = 0). */
typedef struct {
  const int32_t* members;        /* frustum indices, grouped by class */
  const int32_t* offsets;        /* [n_groups + 1] into members; every group non-empty */
  int n_groups;                  /* 1..32; 0 = set not used */
  const int32_t* perm;           /* [perm_len] epoch permutation of the set's frustums (the not-balanced batches), or NULL */
  int perm_len;
} t3d_class_groups;
typedef struct {
  t3d_class_groups set[2];
  int B;                         /* <= 1024 */
  uint32_t seed;
  const float* hyper;            /* device step counter (hyper[0]) */
  const float* order_draws;      /* [n_groups] keys: the groups with the smallest keys take the larger share; NULL: generated */
  const float* member_draws;     /* [B] uniforms in [0,1) picking the member; NULL: generated */
  float equal_prob;              /* *_SAMPLE_EQUAL_CLASS_WITH_PROB: a step is class-balanced when its uniform draw < equal_prob
                                    (train_semisup.py:357, train_boxpc.py:323-328); otherwise B distinct frustums,
                                    np.random.choice(len, B, replace=False): slot b takes perm[(steps_of_this_set * B + b) mod perm_len] */
  const float* prob_draw;        /* [1] that uniform, or NULL (generated) */
  int32_t* sample;               /* [B] out */
  int32_t* is_data_2D;           /* [B] out, or NULL */
} t3d_sample_equal_classes_args;
int t3d_sample_equal_classes(const t3d_sample_equal_classes_args* args, t3d_stream_t stream);

/* How a semi-supervised batch is drawn: SEMI_SAMPLING_METHOD over the two lists of ROISemiDataset (roi_semi_dataset.py:204-275: the
 * 3-D-label list of TRAIN_CLS and the 2-D-label list of `classes2D`, which holds TRAIN_CLS too under SEMI_USE_LABELS2D_OF_CLASSES3D, so
 * a frustum may be in both).  One launch per step writes sample[B] (frustum id per slot, for t3d_batch_assemble's explicit-sample mode)
 * and is_data_2D[B] (for its slot_is_2D); nothing is allocated or synchronised, the step is read from hyper[0] on the device.
 *   T3D_SEMI_BATCH            get_batch (482-535) over the epoch permutation of the concatenation [list3d | list2d]: slot b of step s
 *                             takes entry e = perm[(s*B + b) mod perm_len]; e < len3D: list3d[e], flag 0; else list2d[e - len3D], flag 1.
 *   T3D_SEMI_ALTERNATE_BATCH  (train_semisup.py:351-366) even steps draw all B slots from list2d (flag 1), odd steps from list3d (flag 0).
 *   T3D_SEMI_MIXED_BATCH      sample_mixed (606-637): slots 0..B/2-1 from list2d (flag 1), slots B/2..B-1 from list3d (flag 0); B even.
 * A draw of n slots from a list (sample_from_set, 557-569) follows one coin per step, u < equal_prob (the same coin for both halves of
 * a mixed batch):
 *   false  n distinct positions of the list, np.random.choice(len, n, replace=False): the first n steps of a Fisher-Yates shuffle of
 *          0..len-1, step i swapping position i with position i + floor(r_i * (len - i) / 2^32);
 *   true   "equal classes": the n slots are split over the list's k classes like np.array_split([1]*n, k) -- n mod k classes take one
 *          slot more, WHICH ones is random (the classes whose key ranks among the n mod k smallest) -- slots are laid out class after
 *          class and every slot draws a member of its class with replacement.
 * Every draw comes from the counter-based hash of the other data kernels, keyed by (seed, step, half, slot): a replay is bit-reproducible.
 * T3D_ERR_SHAPE: B outside 1..256, an odd B under MIXED_BATCH, more than 32 classes, and a list shorter than the slots asked of it
 * when the coin can come up false (equal_prob < 1; numpy raises there too). */
enum { T3D_SEMI_BATCH = 0, T3D_SEMI_ALTERNATE_BATCH = 1, T3D_SEMI_MIXED_BATCH = 2 };
#define T3D_SEMI_SAMPLE_MAX_B 256
typedef struct {
  const int32_t* ids;            /* [len] frustum ids of the list, in list order */
  int len;
  const int32_t* members;        /* [len] the same ids grouped by class */
  const int32_t* offsets;        /* [n_groups + 1] into members; every group non-empty */
  int n_groups;                  /* 0..32 (0: no class groups; the list then cannot serve an equal-classes draw) */
} t3d_semi_list;
typedef struct {
  uint32_t struct_size;    /* = sizeof(t3d_semi_sample_args) of the caller's header (see T3D_ABI_VERSION) */
  int method;                    /* T3D_SEMI_* */
  t3d_semi_list list3d;          /* is_data_2D = 0 */
  t3d_semi_list list2d;          /* is_data_2D = 1 */
  const int32_t* perm;           /* BATCH: [perm_len] entries in [0, len3D + len2D) */
  int perm_len;
  int B;                         /* <= T3D_SEMI_SAMPLE_MAX_B */
  uint32_t seed;
  float equal_prob;              /* SEMI_SAMPLE_EQUAL_CLASS_WITH_PROB (not read under BATCH) */
  const float* hyper;            /* device step counter (hyper[0]) */
  int32_t* sample;               /* [B] out */
  int32_t* is_data_2D;           /* [B] out */
} t3d_semi_sample_args;
#define T3D_V2_SIZE_semi_sample_args 136
int t3d_semi_sample(const t3d_semi_sample_args* args, t3d_stream_t stream);

/* The lists and class groups of a data set object, built where the data set lives: the membership pass of ROISemiDataset.__init__
 * (roi_semi_dataset.py:226-274: idx_3Dl / idx_2Dl and cls_to_idx_map3D / cls_to_idx_map2D) and of BoxPCFitDataset.__init__
 * (box_pc_fit_dataset.py:71-100: idx_l, cls_to_idx_map).  It replaces the host constructions of DeviceFrustumSet.semi_lists and
 * split_by_class (transferable3d_amd/dataset.py), which copied cls[F] to the host and uploaded the lists again, and serves the new
 * DeviceFrustumSet.restrict; none of the older constructions could leave a frustum of a 3-D class out of the 3-D list
 * (--train_data3D_keep_prob, --add3D_for_classes2D_prob, --classes_to_drop_prob).
 * Which frustums are selected:
 *   member != NULL  frustum f iff member[f] != 0.  The reference decides membership with a serial, short-circuiting walk of the global
 *                   np.random stream; dataset.reference_label_subset / reference_drop_subset replay it on the host and hand the
 *                   flags in.
 *   member == NULL  frustum f iff (class_mask[cls[f]] != 0 and u1 <= keep_prob) or u2 < add_prob, u1 and u2 two draws of the
 *                   counter-based hash of the other data kernels keyed by (seed, f): the same distribution without the serial
 *                   dependence, for seeded subsets that need not be NumPy's.
 * One launch of one workgroup (F is tens of thousands at the most): a pass of wave ballots counts the selected frustums per class,
 * a second pass ranks every selected frustum inside its 1024-frustum chunk (ballot, population count below the lane, the totals of
 * the waves before it through LDS) and stores it at its place.  No atomic decides a place: equal input gives equal bytes.
 *   ids[0 .. len)             the selected frustum ids in file order (a stable compaction)
 *   members[0 .. len)         the same ids grouped by class in ascending class id, file order inside a class
 *   offsets[0 .. n_groups]    start of every group in members, over the classes present only; offsets[n_groups .. NUM_CLASS] = len
 *   present[c]                1 iff a selected frustum has class c
 *   summary[0..3]             len, n_groups, 1 iff some cls[f] lies outside [0, T3D_NUM_CLASS), 0
 * ids and members are filled with -1 behind len.  ids / members / offsets / n_groups are the fields of t3d_semi_list and
 * t3d_class_groups.  This entry point belongs to the construction of a data set, not to a step: it is the one call of the library
 * that waits for its launch (it reads `summary` back), so that it can answer T3D_ERR_ARG for a class id outside the range, and it
 * must not be called while a stream is captured.  T3D_ERR_SHAPE: F <= 0. */
#define T3D_NUM_CLASS 10
typedef struct {
  uint32_t struct_size;    /* = sizeof(t3d_label_subset_args) of the caller's header (see T3D_ABI_VERSION) */
  int F;
  const int32_t* cls;            /* [F] */
  const uint8_t* member;         /* [F] flags, or NULL: hash draws */
  const int32_t* class_mask;     /* [T3D_NUM_CLASS] (member == NULL) */
  float keep_prob;               /* train_data3D_keep_prob (member == NULL) */
  float add_prob;                /* add3D_for_classes2D_prob (member == NULL) */
  uint32_t seed;
  int reserved;                  /* 0 */
  int32_t* ids;                  /* [F] out */
  int32_t* members;              /* [F] out */
  int32_t* offsets;              /* [T3D_NUM_CLASS + 1] out */
  int32_t* present;              /* [T3D_NUM_CLASS] out */
  int32_t* summary;              /* [4] out */
} t3d_label_subset_args;
#define T3D_V2_SIZE_label_subset_args 88
int t3d_label_subset(const t3d_label_subset_args* args, t3d_stream_t stream);

/* Box-PC Fit training samples (box_pc_fit_dataset.py:105-185 `get`, 211-244 `perturb_box_to_diff_ious`, fed by
 * train_boxpc.py:343-355): each frustum's label box is perturbed until its 3-D IoU with the label box falls strictly inside the
 * "fit" bounds (with probability proportion_fit) or the "no-fit" bounds.  Candidate t of frustum b:
 *   centre + U(-cp,cp)^3,  size + size*U(-sp,sp)^3,  heading + U(0,ap),   (cp,sp,ap) = perturbation * (1 - mean(bounds)).
 * The reference draws candidates one after another; here the 64 lanes of a wave each test one candidate per round and the lowest
 * accepted candidate index wins -- the same first-accepted law over the same candidate stream.  After max_rounds*64 rejected
 * candidates the last candidate of lane 0 is taken and its true IoU reported (the reference would loop on).
 * In place on the label buffers written by t3d_batch_assemble: centre / heading bin+residual / size residual become the
 * perturbed box (the net's x_* inputs); the class is unchanged (size2class keeps the label's type, 179-180). */
typedef struct {
  float* center;                 /* [B,3] in: label centre; out: perturbed centre */
  int32_t* orient_cls;           /* [B]   in/out heading bin  (angle2class of the perturbed heading) */
  float* orient_reg;             /* [B]   in/out heading residual */
  const int32_t* dims_cls;       /* [B]   size class */
  float* dims_reg;               /* [B,3] in/out size residual w.r.t. the class mean size */
  float* y_box_iou;              /* [B] out */
  float* y_center_delta;         /* [B,3] out: perturbed - label */
  float* y_dims_delta;           /* [B,3] out */
  float* y_orient_delta;         /* [B] out */
  float center_perturbation, size_perturbation, angle_perturbation;     /* BOXPC_*_PERTURBATION (config.py:27-29) */
  float fit_lo, fit_hi, nofit_lo, nofit_hi, proportion_fit;              /* BOXPC_FIT_BOUNDS, BOXPC_NOFIT_BOUNDS, BOXPC_PROPORTION_OF_BOXPC_FIT */
  const float* fit_draw;         /* [B] uniforms deciding fit / no-fit, or NULL (generated) */
  const float* cand_draws;       /* [B, max_rounds*64, 7] uniforms in [0,1) of the candidates, or NULL (generated) */
  int max_rounds;
  uint32_t seed;
  const float* hyper;            /* device step counter; required when draws are generated */
  int B;
} t3d_boxpc_perturb_args;
int t3d_boxpc_perturb(const t3d_boxpc_perturb_args* args, t3d_stream_t stream);

/* ---- K11d / K12 / schedules --------------------------------------------------------------------- */

/* grad[off_i + e] = sum_s slabs_i[s, e]  for every tensor i of a device-side table. */
typedef struct { int64_t slab_off; int64_t grad_off; int32_t numel; int32_t n_slabs; } t3d_slab_desc;
int t3d_reduce_slabs(const float* slab_base, float* grad_base, const t3d_slab_desc* table_dev,
                     int n_tensors, int max_numel, t3d_stream_t stream);
/* t3d_reduce_slabs + t3d_pool_sparse_rows (both wait only for stage 1) in one launch. */
int t3d_pool_bwd_mid(const float* slab_base, float* grad_base, const t3d_slab_desc* table_dev, int n_tensors, int max_numel,
                     const t3d_pool_sparse_rows_args* sparse, t3d_stream_t stream);

/* hyper[0] = step (as float, incremented), [1] = lr, [2] = bn_decay, [3] = adam lr_t.
 * Replaces tf.train.exponential_decay(staircase) for lr and bn momentum (train_semisup.py:127-145)
 * and the Adam bias correction.  Device-resident so a captured graph advances by itself. */
typedef struct {
  float base_lr, lr_decay_rate, lr_decay_step;
  float bn_init_decay, bn_decay_rate, bn_decay_step, bn_decay_clip;
  float beta1, beta2;
  int batch_size;
  int step_offset;         /* the step this call runs is hyper[0] + step_offset (0: every call advances one counter; 1: two counters
                            * advance alternately -- the two contexts of the software-pipelined step, step.PipelinedStep) */
} t3d_schedule;
int t3d_schedule_step(float* hyper, const t3d_schedule* s, t3d_stream_t stream);

/* tf.train.AdamOptimizer (train_semisup.py:230), TF form: w -= lr_t * m / (sqrt(v) + eps).
 * `grad_scale` divides the (all-reduced) gradient sum by the world size. */
int t3d_adam_tf_step(float* params, const float* grads, float* m, float* v, int64_t n,
                     const float* hyper, float beta1, float beta2, float eps, float grad_scale,
                     t3d_stream_t stream);

/* t3d_reduce_slabs + t3d_adam_tf_step in one pass over the elements (single replica, Adam over every variable): the workgroups that
 * sum a slab tensor's elements (t3d_reduce_slabs' grid, order and accumulators) write the gradient and apply the update to the same
 * elements from registers; `n_range_blocks` more workgroups apply it to the elements no slab tensor covers, whose gradients were
 * written directly: range i = [off, off + n) of the flat buffers, its first workgroup blk0 (ascending over the table; a range owns
 * ceil(n / 1024) workgroups, n_range_blocks = their sum).  params / m / v share grad_base's element offsets.  The caller guarantees
 * that slab tensors and ranges are disjoint: every element is updated once.  Same bits as the two separate launches. */
typedef struct { int64_t off; int64_t n; int32_t blk0; int32_t reserved; } t3d_adam_range;
int t3d_reduce_slabs_adam(const float* slab_base, float* grad_base, const t3d_slab_desc* table_dev, int n_tensors, int max_numel,
                          float* params, float* m, float* v, const t3d_adam_range* ranges_dev, int n_ranges, int n_range_blocks,
                          const float* hyper, float beta1, float beta2, float eps, float grad_scale, t3d_stream_t stream);

/* fp32 GEMMs on the bf16 matrix pipe (csrc/pointmlp.hip PathX3): x = h + m + l exactly with h = bf16(x), m = bf16(x - h),
 * l = bf16(x - h - m).  Writes the three planes of src[0..n): planes[p * plane_stride + i] (bf16 elements, plane_stride >= n).  The
 * optimiser's fp32 weights are split ONCE per step this way instead of once per tile that stages them. */
int t3d_split_x3(const float* src, void* planes, int64_t n, int64_t plane_stride, t3d_stream_t stream);

/* ... and in MFMA-FRAGMENT ORDER, which is what the x3 GEMM kernels take as `w_x3` (ABI version 3): for every [K, N] matrix of the
 * device table (K % 32 == 0, N % 32 == 0, off % 8 == 0) the three planes are written at planes_*[p * plane_stride + off ...] as
 *     fragment f = (rt * NB + nb) * 64 + lane  ->  eight bf16 at element off + 8 f:  Op[nb * 32 + (lane & 31)][rt * 16 + 8 * (lane >> 5) + j]
 * with Op[n][k] = w[k][n], NB = N / 32 (planes_fwd: the forward's weight operand) and Op[k][n] = w[k][n], NB = K / 32 (planes_dgrad:
 * the data gradient's) -- the B operand of one v_mfma_f32_32x32x16_bf16 per 64 x 16 bytes.  One launch for every layer, once per step
 * behind the optimiser.  `fwd` / `dgrad` select the arrangements an entry needs.  Replaces nothing in the reference: TensorFlow's
 * conv2d reads its fp32 weights (models/tf_util.py:1308). */
typedef struct {
  int64_t off;             /* element offset of the matrix in `params` (and of its planes in every plane buffer) */
  int32_t K, N;
  int32_t fwd, dgrad;      /* write the forward / the data-gradient arrangement */
  int32_t blk0;            /* first workgroup of this matrix: ascending over the table, matrix e owns ceil(K N / 2048) workgroups */
  int32_t reserved;
} t3d_x3_frag_entry;
/* n_blocks = the sum of ceil(K N / 2048) over the table (one 256-thread workgroup per 256 eight-element fragments) */
int t3d_split_x3_frag(const float* params, void* planes_fwd, void* planes_dgrad, int64_t plane_stride, const t3d_x3_frag_entry* table,
                      int n_entries, int n_blocks, t3d_stream_t stream);

/* The head of a training step in one launch: t3d_schedule_step, t3d_split_x3_frag and the forward of a net's first layer
 * (t3d_pointmlp_fwd on fp32 with K <= 4, N = 64 or 128 and a raw input -- no scale / shift / sub: the register kernel, which reads the fp32 weights) are independent of each
 * other -- none reads `hyper` or the planes -- and run as workgroup roles: M / 128 forward tiles, then n_blocks split workgroups,
 * then one workgroup for the schedule.  Same bits as the three launches.  T3D_ERR_ARG if `fwd` is not such a layer. */
/* 1 / 0: would t3d_step_head accept this forward struct (the library's own statement of which launch is such a layer) */
int t3d_step_head_takes(const t3d_pointmlp_fwd_args* fwd);
int t3d_step_head(const t3d_pointmlp_fwd_args* fwd, const float* params, void* planes_fwd, void* planes_dgrad, int64_t plane_stride,
                  const t3d_x3_frag_entry* table, int n_entries, int n_blocks, float* hyper, const t3d_schedule* sched,
                  t3d_stream_t stream);

/* tf.train.MomentumOptimizer(learning_rate, momentum) of `--optimizer momentum` (train_semisup.py:226-228, train_boxpc.py:247,
 * train_semisup_adv.py:296), TF form without Nesterov: accum = momentum * accum + g * grad_scale;  w -= lr * accum, with
 * lr = hyper[1] (the staircase schedule t3d_schedule_step evaluates).  `accum` is the variable's `Momentum` slot. */
int t3d_momentum_step(float* params, const float* grads, float* accum, int64_t n, const float* hyper, float momentum,
                      float grad_scale, t3d_stream_t stream);

/* Standalone tf_util.dropout on a per-point tensor (tf_util.py:1720-1741; the reference's one call site, conv9 -> dp1 -> conv10 of
 * v1_inst_seg, semisup_models.py:131, is fused into t3d_seg_head on the hot path): materialises
 *   out[m,k] = act(a)[m,k] * mask[m,k] / keep_prob          (mask == NULL or keep_prob >= 1: out = act(a))
 * from the lazy activation operand, fp32 [M,K] row-major. */
typedef struct {
  t3d_act_src a;
  const float* mask;       /* [M,K] 0/1 keep flags or NULL */
  float keep_prob;
  float* out;              /* [M,K] */
  int M, K;
  int rows_per_frustum;
} t3d_act_dropout_args;
int t3d_act_dropout(const t3d_act_dropout_args* args, t3d_stream_t stream);

/* dst[i] = bf16(src[i]): the copy of the weights the T3D_BF16 GEMMs read (`w` of t3d_pointmlp_fwd / _dgrad / _bwd then points into
 * it); run once per step after the optimiser.  The fp32 master copy stays what Adam updates and what checkpoints hold. */
int t3d_cast_bf16(const float* src, void* dst, int64_t n, t3d_stream_t stream);

/* tf.nn.dropout keep mask (tf_util.py:1738-1740): mask[i] = 1[u_i < keep], u from a counter-based
 * generator keyed by (seed, hyper step, i).  Tests inject masks instead. */
int t3d_dropout_mask(float* mask, int64_t n, float keep_prob, uint32_t seed, const float* hyper,
                     t3d_stream_t stream);

/* ---- two independent small launches in one ---------------------------------------------------------------------------
 * a and b must not depend on each other (the box / T-Net backward and the segmentation-net backward: semisup_models.py:150-151).
 * Same arguments, same results (bit for bit) as the two stand-alone calls; what is saved is one kernel boundary (~3-5 us).
 * Kinds: t3d_bn_bwd_finalize (up to 512 row tiles), t3d_fc_bwd, t3d_fc_dinput, t3d_dy_colsum.
 * Each op passes the argument checks of its stand-alone launcher first, and the pair answers what that launcher would (a's before b's);
 * then T3D_ERR_ARG for NULL, another kind or a dense finalizer of more than 512 tiles, T3D_ERR_SHAPE for an FC op of at most 32 rows beside one
 * of more.  Nothing is launched when the pair is refused. */
enum { T3D_SMALL_BN_BWD_FINALIZE = 1, T3D_SMALL_FC_BWD = 2, T3D_SMALL_FC_DINPUT = 3, T3D_SMALL_DY_COLSUM = 4,
       T3D_SMALL_BN_FWD_FINALIZE = 5, T3D_SMALL_FC_FWD = 6, T3D_SMALL_POOL_BWD_MID = 7 };      /* 5 .. 7: rider sets only */
/* the arguments of t3d_pool_bwd_mid as a struct (kind 7: a WIDE rider -- hundreds of workgroups, alone in its set, no barrier) */
typedef struct {
  const float* slab_base;
  float* grad_base;
  const t3d_slab_desc* table_dev;
  int n_tensors, max_numel;
  t3d_pool_sparse_rows_args sparse;
} t3d_pool_bwd_mid_args;
typedef struct {
  int kind;
  int depends;            /* rider sets: 1 = reads what the PREVIOUS op of its set wrote (a barrier among the set's workgroups goes in
                             front of it); 0 = independent of it.  Ignored by t3d_small_pair. */
  union {
    t3d_bn_bwd_finalize_args bn_bwd;
    t3d_fc_bwd_args fc_bwd;
    t3d_fc_dinput_args fc_dinput;
    t3d_dy_colsum_args dy_colsum;
    t3d_bn_fwd_finalize_args bn_fwd;
    t3d_fc_fwd_args fc_fwd;
    t3d_pool_bwd_mid_args mid;
  } u;
} t3d_small_op;
int t3d_small_pair(const t3d_small_op* a, const t3d_small_op* b, t3d_stream_t stream);

/* ---- riders: small launches of one chain inside the GEMM launches of an independent chain ---------------------------------------
 * The reference runs its graph op by op (sess.run, train_semisup.py:405-411) and TensorFlow's executor overlaps whatever is
 * independent.  Here the independence that matters is one: nothing the T-Net / box net compute (forward, loss, backward) reaches the
 * segmentation net's backward -- `mask` is a hard comparison (semisup_models.py:150-151).  A rider SET is a run of small ops
 * (batch-norm finalizers, FC heads and their backward, column sums: the kinds above) executed in order by the first `n_wg`
 * 256-thread workgroups of a GEMM launch that does not depend on them and that they do not depend on; the GEMM's own tiles are the
 * workgroups behind.  An op with `depends` waits for its predecessor behind a barrier among the rider workgroups (agent-scope
 * release / acquire; the GEMM's workgroups never wait).  Results are bit-identical to the stand-alone launches of the same ops.
 *   ops        the set, in chain order (passed to the kernel by value: at most T3D_RIDER_MAX_OPS of them)
 *   n_wg       rider workgroups (<= 32; a set that is ONE t3d_pool_bwd_mid -- slab reduction + sparse arg-max rows of a pooled layer's
 *              backward, hundreds of latency-bound workgroups that use a fraction of the chip -- gets one workgroup per block) and
 *   lds_bytes  dynamic LDS the rider bodies need: both filled in by t3d_riders_plan
 *   sync       DEVICE, 2 * T3D_RIDER_MAX_OPS + 2 zero-initialised 32-bit words owned by this set (self-resetting: graph replays need
 *              no memset); the last but one word is set to 1 if a barrier ever gave up waiting (poisoned state; results invalid)
 * The `_r` launchers take `riders == NULL` (then they ARE the plain entry points).  Where the kernel variant a launch selects has no
 * rider form (bf16 kernels, the one-pass backward, the activation-resident pooled forward) the set runs as its own launch in front
 * of the GEMM (t3d_run_riders) -- same results, nothing hidden. */
#define T3D_RIDER_MAX_OPS 10
typedef struct {
  t3d_small_op ops[T3D_RIDER_MAX_OPS];
  int n_ops;
  int n_wg;
  int lds_bytes;
  unsigned* sync;
} t3d_rider_set;
/* validates the set's ops (kinds, shapes that can ride: B <= 32 for the FC ops, <= 512 row tiles for the finalizers) and fills in n_wg and
 * lds_bytes (and clears `in2` of an FC op of the set whose K2 is 0); T3D_ERR_ARG / T3D_ERR_SHAPE if one of them cannot ride */
int t3d_riders_plan(t3d_rider_set* riders);
int t3d_run_riders(const t3d_rider_set* riders, t3d_stream_t stream);      /* the set as a launch of its own */
int t3d_pointmlp_fwd_r(const t3d_pointmlp_fwd_args* args, const t3d_rider_set* riders, t3d_stream_t stream);
int t3d_pointmlp_wgrad_r(const t3d_pointmlp_wgrad_args* args, const t3d_rider_set* riders, t3d_stream_t stream);
int t3d_pointmlp_bwd_r(const t3d_pointmlp_dgrad_args* dgrad, const t3d_pointmlp_wgrad_args* wgrad, const t3d_rider_set* riders,
                       t3d_stream_t stream);
int t3d_pool_bwd_stage1_r(const t3d_pointmlp_gram_args* gram, const t3d_act_colsum_args* colsum, const t3d_pool_bwd_prep_args* prep,
                          const t3d_rider_set* riders, t3d_stream_t stream);
int t3d_pool_bwd_stage2_r(const t3d_pool_wgrad_finish_args* finish, const t3d_pointmlp_dgrad_gram_args* dgrad,
                          const t3d_rider_set* riders, t3d_stream_t stream);
/* Would the `_r` launcher run a rider set INSIDE the GEMM launch for these arguments (1), or as a launch of its own in front of it
 * (0)?  Answered by the launchers' own selection step (kernel variant, T3D_X3, tile widths, ...: what the launcher runs before it
 * touches a stream), so a scheduler needs no copy of those rules; it launches nothing and reads through no pointer of the structs.
 * Negative: the arguments would be rejected -- without exception: the launcher refuses with this code whatever the rider set, and
 * before it runs the set.  (What only the x3 launch step sees -- fragment-order planes `w_x3` of a shape or stride it cannot take,
 * T3D_ERR_SHAPE -- is refused by the launcher alone, set and GEMM together; the query answers for the variant.) */
int t3d_pointmlp_fwd_hosts_riders(const t3d_pointmlp_fwd_args* args);
int t3d_pointmlp_wgrad_hosts_riders(const t3d_pointmlp_wgrad_args* args);
int t3d_pointmlp_bwd_hosts_riders(const t3d_pointmlp_dgrad_args* dgrad, const t3d_pointmlp_wgrad_args* wgrad);
int t3d_pool_bwd_stage1_hosts_riders(const t3d_pointmlp_gram_args* gram, const t3d_act_colsum_args* colsum, const t3d_pool_bwd_prep_args* prep);
int t3d_pool_bwd_stage2_hosts_riders(const t3d_pool_wgrad_finish_args* finish, const t3d_pointmlp_dgrad_gram_args* dgrad);

/* ---- Frustum extraction from SUN-RGBD scenes (csrc/frustum.hip; sunrgbd_data.py extract_roi_seg / _from_rgb_detection) ----
 * A batch of scenes: their depth clouds concatenated (upright depth xyz + C_src-3 more channels, fp64), and a list of jobs, one per
 * (scene, 2-D box, augmentation index), the jobs of scene s at scene_jobs[s] .. scene_jobs[s+1]-1.  Per job:
 *   box2d_out      the 2-D box used: box2d, or random_shift_box2d of it (utils.py:198-211) when perturb_box2d, on the 4 uniforms of
 *                  perturb_draws[j] or, when that is NULL, of the hash of job_key[j];
 *   frustum_angle  -arctan2(z, x) of the box centre back-projected to depth 20 in upright camera coordinates;
 *   n_in_box       n, the number of points whose image uv lies in the box (xmin <= u < xmax, ymin <= v < ymax), fp64 projection;
 *   count          min(n, num_points);
 *   index          [num_points] the scene-local indices of the kept points (-1 beyond count): all n in the cloud's order when
 *                  n <= num_points; otherwise the frustum points of ranks choice[j][0..num_points) (ranks in [0, n), the reference's
 *                  np.random.choice) when choice != NULL and choice[j][0] >= 0, else the num_points ranks of smallest hash key
 *                  mix(seed, job_key[j], rank), in rank order;
 *   out_points     [num_points, C] the kept points in upright camera coordinates (x, -z, y, channels 3 .. C-1);
 *   label          [num_points] 1 where the point lies inside or on the 3-D box of corners box3d[j] (8x3, upright camera, corner order of
 *                  utils.compute_box_3d), else 0; box3d == NULL (detections): label may be NULL.
 * masks / seg_prefix are scratch of mask_offsets[n_jobs] entries: job j owns ceil(points of its scene / 64) of them from mask_offsets[j].
 * Nothing is synchronised with the host.  num_points <= 4096. */
typedef struct {
  uint32_t struct_size;    /* = sizeof(t3d_frustum_extract_args) of the caller's header (see T3D_ABI_VERSION) */
  const double* points;           /* [P, C_src] */
  const int64_t* scene_offsets;   /* [n_scenes + 1] */
  const double* rtilt;            /* [n_scenes, 9] row-major */
  const double* K;                /* [n_scenes, 9] row-major */
  const int32_t* scene_jobs;      /* [n_scenes + 1] */
  int n_scenes; int max_scene_points; int C_src; int C; int n_jobs; int num_points;
  const double* box2d;            /* [J,4] xmin ymin xmax ymax */
  int perturb_box2d;
  const double* perturb_draws;    /* [J,4] uniforms or NULL (hash) */
  const double* box3d;            /* [J,8,3] or NULL */
  const int32_t* job_key;         /* [J,3] scene id, job ordinal within the scene, augmentation index */
  uint32_t seed;
  const int32_t* choice;          /* [J, num_points] or NULL */
  const int64_t* mask_offsets;    /* [J + 1] */
  uint64_t* masks;                /* scratch */
  int32_t* seg_prefix;            /* scratch */
  double* box2d_out;              /* [J,4] */
  double* frustum_angle;          /* [J] */
  int32_t* n_in_box;              /* [J] */
  int32_t* count;                 /* [J] */
  int32_t* index;                 /* [J, num_points] */
  double* out_points;             /* [J, num_points, C] */
  int32_t* label;                 /* [J, num_points] or NULL */
} t3d_frustum_extract_args;
#define T3D_V2_SIZE_frustum_extract_args 208
int t3d_frustum_extract(const t3d_frustum_extract_args* args, t3d_stream_t stream);

/* ---- Official SUN-RGBD detection evaluation of one class (csrc/sunrgbd_eval.hip; evaluate_sunrgbd.py compute_pr_curve_3d) ----
 * The MATLAB protocol of evaluation/sunrgbd/detection/script_3Deval.m for one class, fp64 throughout:
 *   computePRCurve3D.m:20        stable descending order of the confidences (NaN first, ties in file order) -> order;
 *   bb3dOverlapCloseForm.m:17-58 with get_corners_of_bb3d.m:14-44, cuboidVolume.m:3-5, cuboidIntersectionVolume.c:62-88: the overlap
 *                                (intersection over union of two upright prisms on convex quadrilateral footprints) of every detection
 *                                with the ground truth OF ITS OWN IMAGE -- computePRCurve3D.m:30-31 zeroes every other entry;
 *   computePRCurve3D.m:32-36     max_overlap and gt_idx (1-based, first index on ties; 0 where the maximum < eps = 2^-52: `gtIdxAll`);
 *   computePRCurve3D.m:39-75     a box goes to the first detection in sorted order that chose it with an overlap >= threshold: is_tp;
 *                                is_fp = not tp; a "difficult" box takes its detection out of both; gt_assignment (the claimed box, 1-based,
 *                                for the first claimer only); is_missed (a box nobody claimed);
 *   computePRCurve3D.m:78-81     recall = cumsum(tp) / sum(~difficult), precision = cumsum(tp) / (cumsum(fp) + cumsum(tp)), in sorted
 *                                order, from integer counts.  0 / 0 (a leading "difficult" match) is NaN, as in MATLAB;
 *   get_average_precision.m:15-23 ap.
 * A box is {centroid, basis (3 rows), coeffs (half sizes)}; get_corners_of_bb3d orders the rows, turns them towards the viewer and takes
 * abs(coeffs), so row order, row signs and coeff signs do not matter.  A box of zero volume overlaps nothing: 0 / union as
 * in the script, and, as a deliberate difference from it, 0 also for two such boxes (MATLAB: 0 / 0 = NaN).
 * The ground truth comes grouped by image: image_ids (ascending, distinct), image_gt_offsets, and image_gt, the box indices of image
 * k at image_gt_offsets[k] .. image_gt_offsets[k+1]-1 in ascending order (the tie rule needs it).
 * P == 0 or G == 0 are valid (bb3dOverlapCloseForm returns []): every detection is a false positive, every box missed, recall 0 when
 * G == 0, ap 0.  overlaps != NULL: detection i writes the overlaps with its image's boxes, in image_gt order, from overlap_offsets[i]
 * (at most overlap_offsets[i+1] - overlap_offsets[i] of them), and the box indices to overlap_gt.
 * P, G <= T3D_SUNRGBD_EVAL_MAX_BOXES (T3D_ERR_SHAPE beyond): the order is found by counting, P^2 comparisons in one launch, which is meant
 * for the tens of thousands of detections a class has, not for millions.
 * workspace: T3D_SUNRGBD_EVAL_WORKSPACE_BYTES(P, G) bytes, 8-byte aligned.  Nothing is allocated or synchronised with the host; the only
 * atomics are integer minima, so equal inputs give equal bytes. */
#define T3D_SUNRGBD_EVAL_MAX_BOXES (1 << 20)
#define T3D_SUNRGBD_EVAL_WORKSPACE_BYTES(P, G) (((uint64_t)(P) + (uint64_t)(G)) * 92u + 8u)
typedef struct {
  uint32_t struct_size;    /* = sizeof(t3d_sunrgbd_eval_args) of the caller's header (see T3D_ABI_VERSION) */
  int P; int G;
  const double* det_centroid;      /* [P,3] detections in file order */
  const double* det_basis;         /* [P,9] three rows */
  const double* det_coeffs;        /* [P,3] */
  const double* det_confidence;    /* [P] */
  const int32_t* det_image;        /* [P] */
  const double* gt_centroid;       /* [G,3] */
  const double* gt_basis;          /* [G,9] */
  const double* gt_coeffs;         /* [G,3] */
  const int32_t* gt_image;         /* [G] */
  const uint8_t* gt_difficult;     /* [G] or NULL: none */
  int n_images;
  const int32_t* image_ids;        /* [n_images] */
  const int32_t* image_gt_offsets; /* [n_images + 1] */
  const int32_t* image_gt;         /* [G] */
  double threshold;                /* 0.25 in the script */
  void* workspace;
  uint64_t workspace_bytes;
  int32_t* order;                  /* [P] out: sorted position -> file index */
  double* max_overlap;             /* [P] out, file order */
  int32_t* gt_idx;                 /* [P] out, file order */
  uint8_t* is_tp;                  /* [P] out, file order */
  uint8_t* is_fp;                  /* [P] out, file order */
  int32_t* gt_assignment;          /* [P] out, file order */
  uint8_t* is_missed;              /* [G] out */
  double* precision;               /* [P] out, sorted order */
  double* recall;                  /* [P] out, sorted order */
  double* ap;                      /* [1] out */
  const int64_t* overlap_offsets;  /* [P + 1], read when overlaps != NULL */
  double* overlaps;                /* out or NULL */
  int32_t* overlap_gt;             /* out, with overlaps */
} t3d_sunrgbd_eval_args;
#define T3D_V2_SIZE_sunrgbd_eval_args 256
int t3d_sunrgbd_eval(const t3d_sunrgbd_eval_args* args, t3d_stream_t stream);

/* ---- Diagnosis of one class's detection errors (csrc/sunrgbd_diagnose.hip; evaluate_sunrgbd.py diagnose_class) ----
 * The error breakdown of Bolya et al., "TIDE" (ECCV 2020), restated for the protocol above: its prism overlap, its argmax-then-claim
 * matching, its VOC2011 AP.  `eval` is one class's evaluation exactly as t3d_sunrgbd_eval takes it, and every one of its outputs is
 * written with the bytes t3d_sunrgbd_eval writes for the same input; eval->gt_difficult must be NULL (a diagnosis with "difficult"
 * boxes is not defined), eval->overlaps may be NULL.  eval->threshold is t_f, diag->bg_threshold is t_b, 0 <= t_b < t_f.
 * diag adds the ground truth of the OTHER evaluated classes, Go boxes grouped by image as eval's own are: other_image_ids (ascending,
 * distinct), other_image_offsets, other_image_list.  All arithmetic is fp64; the overlap is the evaluation's own, on its footprints.
 * Per detection i, in file order:
 *   other_overlap[i]  the largest overlap with an other-class box of its own image; other_gt[i] that box, 1-based into the other list,
 *                     the first in other_image_list order on ties, 0 where the maximum < eps = 2^-52 (the rules of max_overlap / gt_idx);
 *   kind[i]           with o_s = max_overlap[i], o_o = other_overlap[i], own-class evidence first, as in TIDE:
 *                       T3D_DIAG_TP   is_tp;
 *                       T3D_DIAG_DUP  is_fp and o_s >= t_f: its box was claimed by a better-ranked detection;
 *                       T3D_DIAG_LOC  is_fp and t_b <= o_s < t_f;
 *                       T3D_DIAG_CLS  is_fp, o_s < t_b, o_o >= t_f;
 *                       T3D_DIAG_BOTH is_fp, o_s < t_b, t_b <= o_o < t_f;
 *                       T3D_DIAG_BKG  every other false positive (a detection whose image has no ground truth among them).
 * Per own-class box g: gt_state[g] = 1 claimed; 2 missed but localised (is_missed, and a LOC detection has gt_idx == g + 1); 3 missed.
 * counts[6]: the detections of each kind 0..5; gt_counts[3]: the boxes in states 1..3.
 * ap_fixed[8]: the AP of eight variants of the evaluation, each by the curve code that computes `ap` (integer cumulative sums in rank
 * order, recall = ctp / n_pos, precision = ctp / (cfp + ctp), the VOC2011 envelope, the same fixed summation tree); a removed detection
 * counts in neither sum, like a "difficult" match:
 *   T3D_DIAG_FIX_CLS, _BOTH, _DUP, _BKG  the detections of that kind are removed;
 *   T3D_DIAG_FIX_LOC     per box g in state 2 the best-ranked LOC detection with gt_idx == g + 1 becomes a true positive (an integer
 *                        minimum over ranks, as the first claimer is found); every other LOC detection is removed;
 *   T3D_DIAG_FIX_MISSED  the boxes in state 3 leave the ground truth: n_pos = G minus their number;
 *   T3D_DIAG_FIX_FP      every false positive is removed;
 *   T3D_DIAG_FIX_FN      every missed box (states 2 and 3) leaves the ground truth.
 * A variant whose ground truth is empty has AP 0 (so every variant when G == 0), and so has every variant when P == 0; then every box
 * is in state 3.  Go == 0 is valid: no CLS, no BOTH.  dAP = ap_fixed - ap is left to the host.
 * Deliberate differences from TIDE: classes are diagnosed independently, so CLS is fixed by removal, not by re-labelling; and a missed
 * box that a detection of another class covers is still "missed" for its own class.
 * workspace: T3D_SUNRGBD_DIAGNOSE_WORKSPACE_BYTES(P, G, Go) bytes, 8-byte aligned, separate from eval->workspace (which is read).
 * Four launches behind the evaluation's, the eight curves one workgroup each in one of them.  Nothing is allocated or synchronised
 * with the host; the only atomics are integer minima, so equal inputs give equal bytes.
 * T3D_ERR_ABI: a struct of another size (either one).  T3D_ERR_ARG: a NULL struct or array, gt_difficult != NULL, not 0 <= t_b < t_f,
 * a workspace that is too small, and whatever t3d_sunrgbd_eval refuses.  T3D_ERR_SHAPE: Go < 0 or > T3D_SUNRGBD_EVAL_MAX_BOXES,
 * n_other_images < 0, and eval's shapes.  Nothing is launched then. */
#define T3D_DIAG_TP 0
#define T3D_DIAG_CLS 1
#define T3D_DIAG_LOC 2
#define T3D_DIAG_BOTH 3
#define T3D_DIAG_DUP 4
#define T3D_DIAG_BKG 5
#define T3D_DIAG_FIX_CLS 0
#define T3D_DIAG_FIX_LOC 1
#define T3D_DIAG_FIX_BOTH 2
#define T3D_DIAG_FIX_DUP 3
#define T3D_DIAG_FIX_BKG 4
#define T3D_DIAG_FIX_MISSED 5
#define T3D_DIAG_FIX_FP 6
#define T3D_DIAG_FIX_FN 7
#define T3D_SUNRGBD_DIAGNOSE_WORKSPACE_BYTES(P, G, Go) ((uint64_t)(Go) * 88u + (uint64_t)(G) * 4u + (uint64_t)(P) * 0u + 8u)
typedef struct {
  uint32_t struct_size;    /* = sizeof(t3d_sunrgbd_diagnose_args) of the caller's header (see T3D_ABI_VERSION) */
  int Go;
  const double* other_centroid;        /* [Go,3] ground truth of the other evaluated classes */
  const double* other_basis;           /* [Go,9] */
  const double* other_coeffs;          /* [Go,3] */
  const int32_t* other_image;          /* [Go] */
  int n_other_images;
  const int32_t* other_image_ids;      /* [n_other_images] */
  const int32_t* other_image_offsets;  /* [n_other_images + 1] */
  const int32_t* other_image_list;     /* [Go] */
  double bg_threshold;                 /* t_b */
  void* workspace;
  uint64_t workspace_bytes;
  double* other_overlap;               /* [P] out, file order */
  int32_t* other_gt;                   /* [P] out, file order */
  uint8_t* kind;                       /* [P] out, file order: T3D_DIAG_* */
  uint8_t* gt_state;                   /* [G] out */
  int32_t* counts;                     /* [6] out */
  int32_t* gt_counts;                  /* [3] out */
  double* ap_fixed;                    /* [8] out: T3D_DIAG_FIX_* */
} t3d_sunrgbd_diagnose_args;
#define T3D_V2_SIZE_sunrgbd_diagnose_args 152
int t3d_sunrgbd_diagnose(const t3d_sunrgbd_eval_args* eval, const t3d_sunrgbd_diagnose_args* diag, t3d_stream_t stream);

/* ---- Detection decode of one inference batch (csrc/detect.hip; semisup_infer.inference(decode='device'), detect.Detector) ----
 * What the reference does on the host after every batch (test_semisup.py:236-262, roi_seg_box3d_dataset.py:86-101, 461-466), in one
 * launch, one workgroup of 256 threads per frustum, fp32 throughout:
 *   seg[n]         = logits[n][1] > logits[n][0]                      (np.argmax: a tie is background)
 *   mask_count     = sum_n seg[n];  mask_mean_prob = sum_n seg[n] * softmax(logits[n])[1] / (mask_count + 1)   (the "+ 1" is the reference's)
 *   heading_cls    = argmax box_out[3:15], size_cls = argmax box_out[27:37]   (the lowest index on ties, as np.argmax; a NaN wins)
 *   score          = log(mask_mean_prob + .01) + log(max softmax(heading scores) + .01) + log(max softmax(size scores) + .01)
 *                    [+ log(fit_prob + .01)]
 *   center         = box_out[0:3] + stage1_center - total_delta[0:3]
 *   heading_res    = box_out[15 + heading_cls] * pi/12 - total_delta[6]
 *   size_res       = box_out[37 + 3*size_cls ..] * mean_size[size_cls] - total_delta[3:6]
 *   label          = (h, w, l, tx, ty, tz, ry) of from_prediction_to_label_format: (l, w, h) = mean_size[size_cls] + size_res,
 *                    ry = heading_cls * 2pi/12 + heading_res, minus 2pi where it exceeds pi, plus rot_angle; (tx, tz) = the centre turned
 *                    by -rot_angle about y; ty = center y + h/2 (the bottom of the box)
 *   corners        = get_3d_box((l, w, h), ry, (tx, ty - h/2, tz)): rows 0-3 the +h/2 face
 * box_out is a head output in BoxHeads order (centre 3, heading scores 12, normalised heading residuals 12, size scores 10, normalised
 * size residuals 30), rows ld_box floats apart.  total_delta NULL: no F2_ refinement (zeros); fit_prob NULL: the three-term score;
 * rot_angle NULL: 0; seg NULL: the mask is not written.  Frustums >= n_valid (the padding of a last batch) are not visited: their
 * outputs keep what they held.  logits must be 8-byte aligned.  The mask sum is a fixed tree (per thread in point order, 64 lanes by
 * shuffles, four waves in index order): equal inputs give equal bits, whatever B is.  No atomics, no host synchronisation. */
typedef struct {
  uint32_t struct_size;    /* = sizeof(t3d_detect_decode_args) of the caller's header (see T3D_ABI_VERSION) */
  int B; int N; int n_valid; int ld_box;
  const float* logits;          /* [B, N, 2] */
  const float* box_out;         /* [B, ld_box], ld_box >= 67 */
  const float* stage1_center;   /* [B, 3] */
  const float* total_delta;     /* [B, 7] or NULL */
  const float* fit_prob;        /* [B] or NULL */
  const float* rot_angle;       /* [B] or NULL */
  uint8_t* seg;                 /* [B, N] out or NULL */
  float* score;                 /* [B] out */
  int32_t* mask_count;          /* [B] out */
  int32_t* heading_cls;         /* [B] out */
  int32_t* size_cls;            /* [B] out */
  float* center;                /* [B, 3] out */
  float* heading_res;           /* [B] out */
  float* size_res;              /* [B, 3] out */
  float* label;                 /* [B, 7] out */
  float* corners;               /* [B, 8, 3] out */
} t3d_detect_decode_args;
#define T3D_V2_SIZE_detect_decode_args 152
int t3d_detect_decode(const t3d_detect_decode_args* args, t3d_stream_t stream);

/* ---- Greedy non-maximum suppression of decoded 3-D boxes, many small groups in one call (csrc/nms.hip; nms.DeviceNms, detect
 *      --nms_iou) ----
 * A group is the boxes of one class in one image: group g holds the box indices members[group_offsets[g] .. group_offsets[g+1]-1].
 * The reference has no such step; it is opt-in (a duplicate 2-D detection becomes a duplicate 3-D box, which script_3Deval.m counts as
 * a false positive).  fp32 throughout; the IoU is box3d_iou_corners of csrc/boxgeom_dev.h, the one t3d_box3d_iou_corners returns:
 * metric T3D_NMS_IOU3D the volume IoU, T3D_NMS_IOU2D that of the ground-plane rectangles (bird's-eye view).
 *   Order within a group   a comes before b iff score[a] > score[b], or the scores are equal and a < b.  A NaN score counts as -inf
 *                          (so it ties with a real -inf, and the box index decides).  rank[a] = a's position in that order.
 *   Sweep                  the group is walked in that order.  Box j is suppressed iff some EARLIER KEPT box i has IoU(i, j) > threshold,
 *                          strictly, where IoU(i, j) is computed with i as the first argument.  A NaN IoU (two boxes of zero volume)
 *                          suppresses nothing.  keep[j] = 0 and suppressed_by[j] = the best-ranked such i; a kept box gets 1 and -1.
 *                          A box that a suppressed box would have suppressed is kept (A > B > C, A covers B, B covers C, A not C: C stays).
 *   Groups                 a group of one keeps its box; an empty group is valid.
 *   Unlisted boxes         a box in no group is not visited: its outputs keep what they held (as the frustums >= n_valid of the decode).
 *   Empty input            n == 0, n_groups == 0 or max_group == 0: T3D_OK without a launch.
 *   max_group              the size of the largest group, declared by the caller (who built the lists): the entry point cannot read
 *                          device memory without waiting for it.  It sets the row stride of the workspace.  max_group >
 *                          T3D_DETECT_NMS_MAX_GROUP is T3D_ERR_SHAPE, before anything is launched; a group that turns out larger than
 *                          declared, or a list that leaves [0, n), is not visited.
 *   workspace              T3D_DETECT_NMS_WORKSPACE_BYTES(n, max_group) bytes, 8-byte aligned: the sorted order of every group and one
 *                          bit per (earlier, later) pair of a group, ceil(max_group / 64) 64-bit words per box.  T3D_ERR_ARG if smaller
 *                          or misaligned, and for a null corners / score / group_offsets / members / keep / suppressed_by, n or n_groups
 *                          < 0, or an unknown metric.
 * Three launches on `stream`: the order by counting (size^2 comparisons per group, as t3d_sunrgbd_eval); the pair bits, one thread per
 * (box, 64 later boxes), consecutive lanes on consecutive boxes of the concatenated lists, so that a wave covers several small groups and
 * nothing below the diagonal is computed; the sweep, ceil(max_group / 64) lanes (rounded up to a power of two) per group, 64 groups per
 * wave when every group has at most 64 boxes.  No allocation, no host synchronisation, no atomics: equal inputs give equal bytes, and a
 * group's answers depend on its own boxes only, wherever they sit in the call. */
#define T3D_NMS_IOU3D 0
#define T3D_NMS_IOU2D 1
#define T3D_DETECT_NMS_MAX_GROUP 1024
#define T3D_DETECT_NMS_WORKSPACE_BYTES(n, max_group) \
  ((((uint64_t)(n) + 1u) / 2u) * 8u + (uint64_t)(n) * ((((uint64_t)(max_group)) + 63u) / 64u) * 8u)
typedef struct {
  uint32_t struct_size;    /* = sizeof(t3d_detect_nms_args) of the caller's header (see T3D_ABI_VERSION) */
  int n; int n_groups; int metric;
  const float* corners;            /* [n,8,3], get_3d_box order: what t3d_detect_decode writes */
  const float* score;              /* [n] */
  const int32_t* group_offsets;    /* [n_groups + 1], ascending from 0, the last <= n */
  const int32_t* members;          /* [group_offsets[n_groups]] box indices; a box appears at most once */
  float threshold;
  int max_group;
  void* workspace;
  uint64_t workspace_bytes;
  uint8_t* keep;                   /* [n] out */
  int32_t* suppressed_by;          /* [n] out: -1 for a kept box, else the box index of the best-ranked kept box that suppresses it */
  int32_t* rank;                   /* [n] out or NULL */
} t3d_detect_nms_args;
#define T3D_V2_SIZE_detect_nms_args 96
int t3d_detect_nms(const t3d_detect_nms_args* args, t3d_stream_t stream);

/* ---- Headless rasteriser: z-buffered points, 3-D box wireframes and 2-D rectangles into uint8 RGB images (csrc/render.hip;
 *      render.Renderer, detect --vis_dir) ----
 * One call paints n_views pictures ("views") into the caller's `out`.  Every table is a device array with a count; fp32 throughout,
 * every product and sum below is its own fp32 operation (no contraction), in the order written.
 *   Transform        (X, Y, D, W) = P . (x, y, z, 1), P row-major 4x4: each component ((p0*x + p1*y) + p2*z) + p3.  A primitive (a point,
 *                    a box, a rectangle) with a non-finite transformed coordinate -- for a box, of any of its 8 corners -- is dropped.
 *   Pixels           u = X / W, v = Y / W; pixel centres sit on integers: px = floor(u + 0.5), py = floor(v + 0.5), px a column in
 *                    [0, W_view), py a row in [0, H_view).  Images are row-major, 3 bytes (R, G, B) per pixel.
 *   Points           a point range {view, first, count, mode, colour0, colour1, splat} shows the points first .. first+count-1 of the
 *                    point array (xyz rows ld_xyz floats apart) in one view.  A point is visible iff W >= w_near and D >= 0.  Per
 *                    pixel the visible point of the smallest D wins, on equal D (-0 is 0) the lowest index in the point array: a 64-bit
 *                    atomicMin of (bits(D) << 32) | index.  splat 1, 3 or 5 stamps that square centred on (px, py), clipped to the view.
 *                    Colour by mode: T3D_RENDER_RGB rgb[index] (fp32 in [0,1], rows of 3), T3D_RENDER_LABEL colour1 where label[index]
 *                    != 0 else colour0, T3D_RENDER_FLAT colour0.  The ranges of one view should not overlap in the point array (where
 *                    they do, the first range in table order that holds the winning index colours it).
 *   Segments         the 12 edges of a box entry {view, box, colour, thickness} over corners[box] ([8,3], get_3d_box order, what
 *                    t3d_detect_decode writes): (i, (i+1)%4), (4+i, 4+(i+1)%4), (i, i+4) for i = 0..3; the 4 sides of a rectangle
 *                    entry {view, xmin, ymin, xmax, ymax, colour, thickness}, whose corners are pixel coordinates (u, v) as they stand
 *                    (no transform, no near plane).  An endpoint a with Wa < w_near is moved to the crossing with the other endpoint b:
 *                    t = (w_near - Wa) / (Wb - Wa), X = Xa + t*(Xb - Xa), Y likewise, W = w_near; both behind: the segment is dropped.
 *                    u, v non-finite after the division: dropped.  Endpoints are rounded to pixels as above and clamped to +-2^20.
 *                    The pixel set is all-integer: the major axis is x when |dx| >= |dy|, else y; A is the endpoint of the smaller
 *                    major coordinate (the smaller minor one on a tie); for every major coordinate m from A's to B's the minor one
 *                    is a_minor + floor((2*(m - a_major)*d_minor + d_major) / (2*d_major)) (64-bit, floor division); dx = dy = 0 is
 *                    the single pixel.  Thickness t (1..5) stamps the offsets -floor((t-1)/2) .. +floor(t/2) in both axes.
 *   Painting order   the background (the view's image in `bg` where bg_offset >= 0, else bg_colour), then the z-buffered points, then
 *                    the box entries in table order, then the rectangles in table order, each later one over the earlier: a 32-bit
 *                    atomicMax of the primitive's ordinal (1 + box entry, 1 + n_boxes + rectangle) per pixel, then a resolve pass.
 *   Colours          a float colour c becomes the byte min(255, max(0, floor(c*255 + 0.5))) (a NaN: 0).
 *   Reproducible     integer min / max atomics only, no float atomics: equal inputs give equal bytes.
 *   Untouched        bytes of `out` outside the listed views keep what they held; a view with no primitives shows its background.
 *   Layout           the caller lays the views out back to back in the workspace, in table order: view.pixel_first = the sum of H*W of
 *                    the views before it, total_pixels the sum over all; likewise range.pos_first = the sum of `count` of the ranges
 *                    before it and total_point_items the sum over all (the entry point cannot read device memory without waiting for
 *                    it, and the launches are sized from the two totals).
 *   workspace        T3D_RENDER_WORKSPACE_BYTES(total_pixels) = 12 bytes per pixel (a 64-bit depth word and a 32-bit ordinal),
 *                    8-byte aligned.
 *   Errors           n_views == 0: T3D_OK without a launch.  T3D_ERR_ARG: a null args / views / out / workspace, a null table or
 *                    point / corner array with a positive count, a negative count or total, total_pixels == 0, a workspace that is
 *                    smaller or misaligned.  The tables themselves live on the device; a caller that still holds them on the host
 *                    passes the same bytes as views_host / ranges_host / boxes_host / rects_host (each may be NULL), and then
 *                    T3D_ERR_ARG is also: H*W == 0 (or H, W < 0), an entry naming a view >= n_views, a box >= n_corner_boxes, a
 *                    range outside [0, n_points), a splat other than 1, 3, 5, a thickness outside 1..5, an unknown mode, a mode whose
 *                    array is NULL, a pixel_first / pos_first / total that is not the running sum, an image that leaves out_bytes /
 *                    bg_bytes.  Independently, the kernels check every entry again: one that breaks these rules paints nothing, and
 *                    nothing is ever written outside [out, out + out_bytes) and the workspace.
 * Three launches on `stream`: clear (depth words, ordinals, backgrounds), paint (a thread per position of the concatenated point
 * ranges, then a wave per segment striding over the major-axis steps that can touch the view), resolve.  No allocation, no host
 * synchronisation. */
#define T3D_RENDER_RGB 0
#define T3D_RENDER_LABEL 1
#define T3D_RENDER_FLAT 2
#define T3D_RENDER_WORKSPACE_BYTES(pixels) ((uint64_t)(pixels) * 12u)
typedef struct {
  float P[16];             /* row-major 4x4 */
  float w_near;
  int H; int W;
  int pixel_first;         /* the view's first pixel in the workspace (see Layout) */
  int64_t out_offset;      /* byte offset of the view's image [H,W,3] in out */
  int64_t bg_offset;       /* byte offset of its background image [H,W,3] in bg, or -1: bg_colour */
  float bg_colour[3];
  int reserved;
} t3d_render_view;
typedef struct {
  int view; int first; int count; int mode;
  float colour0[3]; float colour1[3];
  int splat;
  int reserved;
  int64_t pos_first;       /* the sum of `count` of the ranges before this one (see Layout) */
} t3d_render_points;
typedef struct { int view; int box; float colour[3]; int thickness; } t3d_render_box;
typedef struct { int view; float xmin; float ymin; float xmax; float ymax; float colour[3]; int thickness; } t3d_render_rect;
typedef struct {
  uint32_t struct_size;    /* = sizeof(t3d_render_args) of the caller's header (see T3D_ABI_VERSION) */
  int n_views; int n_points; int n_ranges; int n_corner_boxes; int n_boxes; int n_rects;
  int ld_xyz;                          /* floats between two rows of xyz, >= 3 */
  const t3d_render_view* views;        /* [n_views] */
  const float* xyz;                    /* [n_points, ld_xyz] */
  const float* rgb;                    /* [n_points, 3] or NULL */
  const uint8_t* label;                /* [n_points] or NULL */
  const t3d_render_points* ranges;     /* [n_ranges] */
  const float* corners;                /* [n_corner_boxes, 8, 3] */
  const t3d_render_box* boxes;         /* [n_boxes] box entries */
  const t3d_render_rect* rects;        /* [n_rects] */
  int64_t total_pixels;
  int64_t total_point_items;
  const uint8_t* bg;                   /* background images or NULL */
  uint64_t bg_bytes;
  uint8_t* out;
  uint64_t out_bytes;
  void* workspace;
  uint64_t workspace_bytes;
  const t3d_render_view* views_host;   /* host copies of the four tables, each or NULL (see Errors) */
  const t3d_render_points* ranges_host;
  const t3d_render_box* boxes_host;
  const t3d_render_rect* rects_host;
} t3d_render_args;
#define T3D_V2_SIZE_render_args 192
int t3d_render(const t3d_render_args* args, t3d_stream_t stream);

/* ---- Label-free consistency of decoded detections (csrc/consistency.hip; consistency.DeviceConsistency, detect --consistency,
 *      autolabel) ----
 * A 3-D box that came from a 2-D box has to reproject onto that 2-D box, and it has to sit on the points the network segmented.  One
 * launch behind t3d_detect_decode, one workgroup of 256 threads per detection b < min(n_valid, B); rows at or past n_valid keep what
 * they held.  Every arithmetic step is fp64 (the fp32 inputs are widened first); each product and each sum below is its own operation
 * (no contraction), in the order written, so that a NumPy fp64 transcription gives the same bits.
 *   Mask             mask[n] = logits[n][1] > logits[n][0] (a tie is background, as in t3d_detect_decode); n_mask = sum mask, which
 *                    equals the decode's mask_count.
 *   Point frame      rot_angle != NULL: c = cos(-(double)rot), s = sin(-(double)rot); x' = c*x - s*z, y' = y, z' = s*x + c*z (the way the
 *                    decode turns the centre).  NULL: the point as it stands, no multiplication.
 *   In the box       the closed parallelepiped at corner K0 with the edges to corners 1, 3 and 4 (get_3d_box order: w, l, h).
 *                    q = p' - K0; per edge e = Kj - K0: dv = (q0*e0 + q1*e1) + q2*e2, dd = (e0*e0 + e1*e1) + e2*e2; inside iff
 *                    0 <= dv && dv <= dd for all three edges (a NaN anywhere: not inside).  n_box counts the points inside, n_both
 *                    those inside that are also masked, both with multiplicity (the network's draw repeats points).
 *   Projection       project_upright_camera_to_upright_depth then project_upright_depth_to_image of sunrgbd_data/utils.py.  Per
 *                    corner (X, Y, Z): d = (X, Z, -Y); t_i = (R[0][i]*d0 + R[1][i]*d1) + R[2][i]*d2 (Rtilt^T d); cam = (t0, -t2, t1);
 *                    w_i = (K[i][0]*cam0 + K[i][1]*cam1) + K[i][2]*cam2; u = w0/w2, v = w1/w2; the depth is cam2.
 *   Rectangle        xmin = u of corner 0, then for corners 0..7 in order xmin = u < xmin ? u : xmin; xmax, ymin, ymax likewise.  Where
 *                    image W > 0 and H > 0, x values are clamped to [0, W-1] and y values to [0, H-1]: x < 0 ? 0 : (x > W-1 ? W-1 : x).
 *   IoU with box2d   iw = min(xmax_a, xmax_b) - max(xmin_a, xmin_b), ih likewise (min(a, b) = a < b ? a : b, max(a, b) = a > b ? a : b,
 *                    a the rectangle); inter = (iw > 0 && ih > 0) ? iw*ih : 0; areas (xmax - xmin)*(ymax - ymin);
 *                    uni = (area_a + area_b) - inter; IoU = uni > 0 ? inter/uni : 0.
 *   flags            bit 1: some corner has depth <= 0 or a non-finite u or v -- the five reproj values are then 0.
 *                    bit 2: n_mask == 0.
 *                    bit 4: calib_index outside [0, n_calib) -- the five reproj values are then 0 and no calibration row is read; the
 *                    counts are computed all the same.
 *   calib            rows of 20 fp64: Rtilt row-major (9), K row-major (9), image W, image H (W <= 0 or H <= 0: do not clip).  Several
 *                    detections may name one row.
 *   Errors           before any launch: T3D_ERR_SHAPE for B <= 0, N <= 0, n_valid < 0, ld_xyz < 3 or n_calib < 0; T3D_ERR_ARG for a null
 *                    pointer other than rot_angle, or logits that are not 8-byte aligned.  n_valid == 0: T3D_OK without a launch.
 * The counts are integer sums over a fixed tree (per thread, 64 lanes by shuffles, four waves in index order).  No atomics, no
 * allocation, no host synchronisation: equal inputs give equal bytes, whatever B is. */
typedef struct {
  uint32_t struct_size;    /* = sizeof(t3d_detect_consistency_args) of the caller's header (see T3D_ABI_VERSION) */
  int B; int N; int n_valid; int ld_xyz;
  const float* xyz;             /* [B, N, ld_xyz], ld_xyz >= 3: the points the network saw; columns 0..2 are read */
  const float* logits;          /* [B, N, 2] */
  const float* corners;         /* [B, 8, 3]: what t3d_detect_decode wrote */
  const float* rot_angle;       /* [B] or NULL */
  const double* box2d;          /* [B, 4]: xmin, ymin, xmax, ymax */
  const int32_t* calib_index;   /* [B] */
  const double* calib;          /* [n_calib, 20] */
  int n_calib;
  int32_t* counts;              /* [B, 4] out: n_mask, n_box, n_both, flags */
  double* reproj;               /* [B, 5] out: xmin, ymin, xmax, ymax, IoU */
} t3d_detect_consistency_args;
#define T3D_V2_SIZE_detect_consistency_args 104
int t3d_detect_consistency(const t3d_detect_consistency_args* args, t3d_stream_t stream);

/* ---- Box voting: every box t3d_detect_nms kept takes the weighted mean geometry of the boxes it suppressed (csrc/fuse.hip;
 *      nms.DeviceFuse, detect --nms_iou T --nms_fuse) ----
 * A 2-D detector reports one object several times, each report becomes a frustum of its own and a 3-D estimate of its own;
 * t3d_detect_nms keeps the best-ranked one and names, per suppressed box, the kept box that suppressed it.  This entry point runs behind
 * it on the same stream and the same buffers and leaves the decision who survives alone: it writes, into buffers of its own, the kept
 * box's geometry fused with that of its cluster (Gidaris & Komodakis, ICCV 2015; weighted box fusion), for oriented 3-D boxes.  The
 * reference has no such step; it is opt-in.  n, n_groups, group_offsets, members and max_group are those of the t3d_detect_nms call, under
 * the same contract; keep, suppressed_by and rank are what it wrote (rank is needed here), label and corners what t3d_detect_decode wrote.
 *   Cluster        of a listed box i with keep[i] != 0: i (the anchor) and every listed box j of its group with keep[j] == 0 and
 *                  suppressed_by[j] == i.
 *   Voters         member j != i votes iff all 7 entries of label[j] are finite and IoU(i, j) > vote_threshold, strictly, where the IoU
 *                  is the fp32 box3d_iou_corners(corners[i], corners[j]) of csrc/boxgeom_dev.h with i as the first argument: the volume
 *                  IoU for metric T3D_NMS_IOU3D, that of the ground rectangles for T3D_NMS_IOU2D.  A NaN IoU does not vote.  Both
 *                  boxes are handed over relative to corner 0 of box i (each fp32 coordinate minus that corner's): the IoU does not
 *                  depend on where the pair lies, its fp32 rounding does, and here the value is a weight, not only a decision.
 *   Weights        s(x) = x where x is finite and >= 0, else 0.  w_i = s(weight[i]); w_j = s(weight[j]) * IoU(i, j).
 *   Alignment      a box equals itself turned by pi, and turned by pi/2 with l and w exchanged.  With d = ry_j - ry_i and
 *                  wrap(x) = x - 2pi * ceil((x - pi) / 2pi) (into (-pi, pi]), the candidates are k = 0, 1, 2, 3: wrap(d + k * pi/2),
 *                  (l_j, w_j) exchanged for odd k.  The k of the smallest |wrap(d + k * pi/2)| is taken, on a tie the lowest;
 *                  delta_j is that wrapped difference and (l'_j, w'_j) the dimensions after the exchange.
 *   Fusion         W = w_i + sum w_j.  cx, cy, cz, l, w, h = the w-weighted means over the anchor and the voters of (tx, ty - h/2, tz),
 *                  l', w', h: (w_i * x_i + sum w_j * x_j) / W.  ry = ry_i + (sum w_j * delta_j) / W, not wrapped again: it stays
 *                  continuous with the kept box.  label_out[i] = (h, w, l, cx, cy + h/2, cz, ry).
 *   Precision      the label entries and weights are widened to fp64, every step above is fp64, the sums run over the voters in
 *                  ascending rank, the anchor first; the 7 results are rounded to fp32 once.  The IoU is computed in fp32 and widened.
 *   corners_out    from the fp32 label_out[i] by the fp32 formula of t3d_detect_decode: get_3d_box((l, w, h), ry, (tx, ty - h/2, tz)),
 *                  corner c: x = (c & 2 ? -l : l) / 2, y = (c < 4 ? h : -h) / 2, z = ((c + 1) & 2 ? -w : w) / 2;
 *                  ((cos ry * x + sin ry * z) + tx, y + (ty - h/2), (-sin ry * x + cos ry * z) + tz).
 *   Unchanged      label_out[i] and corners_out[i] are byte copies of label[i] and corners[i] for: a kept box without voters; a kept
 *                  box with W == 0 or W not finite; a kept box with a non-finite entry in its own label; every listed suppressed box.
 *   n_votes        the number of voters (0, 1, ...) of a kept box whatever their weights (0 where its own label is not finite: nobody
 *                  is asked); -1 for a listed suppressed box.
 *   Unlisted       a box in no group is not visited: none of its three outputs is written.  Neither is a box of a group that breaks
 *                  the contract of t3d_detect_nms (larger than max_group, or leaving [0, n)).
 *   Empty input    n == 0, n_groups == 0 or max_group == 0: T3D_OK without a launch.
 *   Errors         before anything is launched: T3D_ERR_SHAPE for max_group > T3D_DETECT_NMS_MAX_GROUP; T3D_ERR_ARG for n, n_groups or
 *                  max_group < 0, an unknown metric, a vote_threshold that is NaN or outside [0, 1], a null pointer, a workspace smaller
 *                  than T3D_DETECT_FUSE_WORKSPACE_BYTES(n) or not 8-byte aligned.
 *   workspace      per position of the lists an int32 and a 16-byte vote: every group's boxes in rank order, rebuilt from `rank`, and
 *                  what each suppressed box says of the box that suppressed it (nothing of the workspace of t3d_detect_nms is read,
 *                  whose layout stays private).
 * The inputs are never written, the outputs are buffers of their own.  Two launches on `stream`, both one thread per POSITION of the
 * concatenated lists (a wave covers several whole small groups).  The first writes order[first(g) + rank[box]] = box and, for a
 * suppressed box, its vote: the IoU with its suppressor, the aligning quarter turn and the heading difference -- one IoU per suppressed
 * box in all, every lane busy with its own.  In the second the thread of a kept box walks the later ranks of its own group, takes the
 * votes cast for it and sums them in rank order.  No atomics, no allocation, no host synchronisation: a group's outputs depend on its
 * own boxes only, and equal inputs give equal bytes. */
#define T3D_DETECT_FUSE_WORKSPACE_BYTES(n) ((((uint64_t)(n) + 1u) / 2u) * 8u + (uint64_t)(n) * 16u)
typedef struct {
  uint32_t struct_size;    /* = sizeof(t3d_detect_fuse_args) of the caller's header (see T3D_ABI_VERSION) */
  int n; int n_groups; int metric;
  const int32_t* group_offsets;    /* [n_groups + 1], as for t3d_detect_nms */
  const int32_t* members;          /* [group_offsets[n_groups]] */
  const uint8_t* keep;             /* [n]: what t3d_detect_nms wrote */
  const int32_t* suppressed_by;    /* [n]: likewise */
  const int32_t* rank;             /* [n]: likewise */
  const float* label;              /* [n,7] (h, w, l, tx, ty, tz, ry), ty the bottom of the box: what t3d_detect_decode wrote */
  const float* corners;            /* [n,8,3], get_3d_box order: likewise */
  const float* weight;             /* [n]: what a box's vote counts, usually what ranked it */
  float vote_threshold;            /* in [0, 1] */
  int max_group;
  void* workspace;
  uint64_t workspace_bytes;
  float* label_out;                /* [n,7] out */
  float* corners_out;              /* [n,8,3] out */
  int32_t* n_votes;                /* [n] out */
} t3d_detect_fuse_args;
#define T3D_V2_SIZE_detect_fuse_args 128
int t3d_detect_fuse(const t3d_detect_fuse_args* args, t3d_stream_t stream);

/* ---- Test-time augmentation: the V decoded boxes of every detection -> one fused box and how well the views agree
 *      (csrc/ensemble.hip; ensemble.DeviceEnsemble, detect --tta K [--tta_flip]) ----
 * `detect` can send every frustum through the network V times -- each view on a point draw of its own, some mirrored by
 * t3d_batch_assemble -- and t3d_detect_decode writes a label row per view.  This entry point runs once behind the last decode, before the
 * consistency filter's rejection, t3d_detect_nms and t3d_detect_fuse: it brings the mirrored views back, measures how far the V boxes
 * of a detection agree (stability under augmentation, the label-free criterion of semi-supervised detection) and writes their weighted
 * mean around the view that agrees best with the others.  The reference has no such step; it is opt-in.  Per detection i < n:
 *   View label     of a view v whose flip_mask bit is clear: label[v][i] as it stands.  Of a mirrored view: the box mirrored back across
 *                  the vertical plane t3d_batch_assemble's flip used (x -> -x, heading -> pi - heading in the centre view, csrc/data.hip),
 *                  in fp64 on the widened fp32 entries, every product and sum its own operation: a = rot_angle[i] (0 for NULL),
 *                  c = cos a, s = sin a; x_c = tx*c - tz*s, z_c = tx*s + tz*c; tx' = -x_c*c + z_c*s, tz' = x_c*s + z_c*c;
 *                  ry' = wrap((pi - ry) + 2*a) with wrap of t3d_detect_fuse; h, w, l and ty stay.  The three results are rounded to fp32
 *                  once; everything below reads this fp32 view label (h, w, l, tx', ty, tz', ry').
 *   Valid views    a view is valid when all 7 entries of its view label are finite (a non-finite entry of label[v][i] leaves at least
 *                  one, so does a non-finite rot_angle in a mirrored view); m is their number.
 *   Pair IoUs      for every pair of valid views u < v the fp32 box3d_iou_corners(k_u, k_v) of csrc/boxgeom_dev.h, u the first argument:
 *                  the volume IoU for metric T3D_NMS_IOU3D, that of the ground rectangles for T3D_NMS_IOU2D.  Both corner sets are
 *                  built from the view labels by the fp32 corner formula of t3d_detect_decode (quoted under corners_out of
 *                  t3d_detect_fuse), box u at the translation (0, 0, 0) and box v at the fp32 differences of the two centres
 *                  (tx_v - tx_u, (ty_v - h_v/2) - (ty_u - h_u/2), tz_v - tz_u): the IoU does not depend on where the pair lies, its fp32
 *                  rounding does (csrc/fuse.hip), and here the value is a weight and an output.  A NaN IoU counts as 0 everywhere
 *                  below.  IoU(x, y) below is the value of the pair (min(x, y), max(x, y)).
 *   agreement      the mean, and min_iou the minimum, of the pair IoUs over all valid pairs: the sum is fp64 over (u, v) in
 *                  lexicographic order, divided by the number of pairs and rounded to fp32 once.  Both are 0 for m < 2.
 *   anchor         the medoid: the valid view whose mean IoU with the other valid views (fp64 sum in ascending view order, divided by
 *                  m - 1) is largest, the lowest view on a tie -- so V = 2 anchors on view 0 whenever view 0 is valid.  The only valid
 *                  view for m == 1; -1 for m == 0.
 *   Voters         a valid view v != anchor votes iff IoU(anchor, v) > vote_threshold, strictly; n_votes[i] is their number, whatever
 *                  their weights.
 *   Fusion         Weights, Alignment, Fusion and Precision of t3d_detect_fuse with the anchor in the place of the kept box, on the
 *                  view labels: w_a = s(weight[a][i]), w_v = s(weight[v][i]) * IoU(anchor, v); the quarter turn that aligns a voter is
 *                  chosen on the view labels' headings; the fp64 sums run anchor first, then the voters in ascending view index; the 7
 *                  results are rounded to fp32 once and corners_out[i] comes from the rounded label_out[i] by the decode's formula.
 *   Unchanged      nothing is fused when there is no voter, or W is 0 or not finite.  Then, with the anchor view 0, and for m == 0:
 *                  label_out[i] and corners_out[i] are byte copies of label[0][i] and corners0[i] (view 0 is never mirrored).  With another
 *                  anchor: its fp32 view label and the corners the decode's formula builds from it.  So V == 1 is a byte copy with
 *                  agreement 0, min_iou 0, anchor 0 (-1 for a non-finite label) and n_votes 0.
 *   Errors         before anything is launched: T3D_ERR_SHAPE for V > T3D_DETECT_ENSEMBLE_MAX_VIEWS; T3D_ERR_ARG for n < 0, V < 1, an
 *                  unknown metric, bit 0 or a bit at position V or above set in flip_mask, a vote_threshold that is NaN or outside
 *                  [0, 1], a null pointer among label[0 .. V-1], weight[0 .. V-1], corners0 or the six outputs, a workspace smaller than
 *                  T3D_DETECT_ENSEMBLE_WORKSPACE_BYTES(n, V) (or null where that is not 0) or not 8-byte aligned.  label[v] and
 *                  weight[v] for v >= V are not looked at.  n == 0: T3D_OK without a launch, whatever the pointers and the workspace are.
 *   workspace      one fp32 per (detection, pair), detection-major.
 * The inputs are never written, the outputs are buffers of their own.  Two launches on `stream`: the first one thread per (detection,
 * pair) -- every lane busy with one IoU, none walking 28 polygon clips in a row --, the second one thread per detection, which reads its
 * V(V-1)/2 IoUs, picks the anchor, sums and writes.  No atomics, no allocation, no host synchronisation: a detection's outputs depend
 * on its own rows only, and equal inputs give equal bytes. */
#define T3D_DETECT_ENSEMBLE_MAX_VIEWS 8
#define T3D_DETECT_ENSEMBLE_WORKSPACE_BYTES(n, V) ((((uint64_t)(n) * (uint64_t)((V) * ((V) - 1) / 2) + 1u) / 2u) * 8u)
typedef struct {
  uint32_t struct_size;    /* = sizeof(t3d_detect_ensemble_args) of the caller's header (see T3D_ABI_VERSION) */
  int n; int V; int metric;
  const float* label[T3D_DETECT_ENSEMBLE_MAX_VIEWS];     /* per view [n,7] (h, w, l, tx, ty, tz, ry): what t3d_detect_decode wrote for it */
  const float* weight[T3D_DETECT_ENSEMBLE_MAX_VIEWS];    /* per view [n]: what the view's vote counts */
  uint32_t flip_mask;              /* bit v: view v was assembled mirrored; bit 0 clear */
  float vote_threshold;            /* in [0, 1] */
  const float* rot_angle;          /* [n] or NULL: the angle t3d_batch_assemble turned the frustum to its centre view by */
  const float* corners0;           /* [n,8,3]: view 0's decoded corners (read for the byte copies only) */
  void* workspace;
  uint64_t workspace_bytes;
  float* label_out;                /* [n,7] out */
  float* corners_out;              /* [n,8,3] out */
  float* agreement;                /* [n] out */
  float* min_iou;                  /* [n] out */
  int32_t* anchor;                 /* [n] out */
  int32_t* n_votes;                /* [n] out */
} t3d_detect_ensemble_args;
#define T3D_V2_SIZE_detect_ensemble_args 232
int t3d_detect_ensemble(const t3d_detect_ensemble_args* args, t3d_stream_t stream);

/* ---- Threshold sweep, part 1: t3d_detect_nms for many configurations in one call (csrc/nms_sweep.hip; nms.DeviceNmsSweep, detect
 *      --sweep) ----
 * Choosing --nms_iou and the --min_* thresholds means scoring a grid of a few hundred configurations, and nothing up to the decoded
 * boxes depends on them.  n, n_groups, metric, corners, score, group_offsets, members and max_group are those of t3d_detect_nms, under
 * the same contract; the groups list every candidate box.  A configuration m of the M given is
 *   config_threshold[m]    an index into thresholds[0 .. n_thresholds-1], or -1: no suppression.  Any other value is no
 *                          configuration: its keep row and its n_kept are 0;
 *   listed[m, box] != 0    the boxes that take part in it (rows listed_stride >= n bytes apart); listed == NULL: every box, in every
 *                          configuration.
 *   keep[m, 0 .. n)        byte for byte what t3d_detect_nms writes into a zero-filled `keep` when it is called with the threshold
 *                          thresholds[config_threshold[m]] and every group restricted to its boxes with listed[m, box] != 0 (rows
 *                          keep_stride >= n bytes apart; the bytes of a row past n are not touched).  The order of a restricted group is
 *                          the order of the whole group with the other boxes left out, so the order is computed once.  With
 *                          config_threshold[m] == -1 a listed box of a group gets 1.  A box in no group, or not listed, gets 0.
 *   n_kept[m]              the number of ones in row m, by integer sums and one integer atomic per wave.
 * box3d_iou_corners runs once per (earlier, later) pair of a group, whatever M and n_thresholds are, by the call of t3d_detect_nms with
 * the same argument order: the fp32 value that decides is the same value, so no configuration can differ from the single call by a
 * rounding.  Per pair one bit in each of n_thresholds bit rows (IoU > thresholds[k], strictly; a NaN IoU sets none).
 *   Empty input            n == 0, n_groups == 0 or max_group == 0: one launch that zeroes n_kept[0 .. M) and, where keep != NULL, the
 *                          rows keep[m, 0 .. n): what t3d_detect_nms leaves of a zero-filled keep.  Only n_kept is required then.
 *   Errors                 before anything is launched: T3D_ERR_SHAPE for max_group > T3D_DETECT_NMS_MAX_GROUP, M outside
 *                          [1, T3D_SWEEP_MAX_CONFIGS], n_thresholds outside [1, T3D_NMS_SWEEP_MAX_THRESHOLDS]; T3D_ERR_ARG for n,
 *                          n_groups or max_group < 0, an unknown metric, a NaN among thresholds[0 .. n_thresholds), a null n_kept /
 *                          corners / score / group_offsets / members / config_threshold / keep / workspace, keep_stride or (with listed)
 *                          listed_stride < n, a workspace smaller than T3D_DETECT_NMS_SWEEP_WORKSPACE_BYTES(n, max_group, n_thresholds)
 *                          or not 8-byte aligned.
 *   workspace              the sorted order of every group and n_thresholds bits per (earlier, later) pair of a group:
 *                          ceil(max_group / 64) * n_thresholds 64-bit words per box.
 * Four launches on `stream`: the rows are zeroed; the order (the kernel of t3d_detect_nms); the pair bits, one thread per (box, 64 later
 * boxes); the walk, one launch for all (configuration, group) pairs with the configuration in the grid's y / z and the lanes of
 * t3d_detect_nms's sweep per group, so a configuration's work is spread over as many workgroups as the single call's is.  No allocation,
 * no host synchronisation; the only atomics are integer additions, so equal inputs give equal bytes. */
#define T3D_NMS_SWEEP_MAX_THRESHOLDS 16
#define T3D_SWEEP_MAX_CONFIGS 65536
#define T3D_DETECT_NMS_SWEEP_WORKSPACE_BYTES(n, max_group, n_thresholds) \
  ((((uint64_t)(n) + 1u) / 2u) * 8u + (uint64_t)(n) * ((((uint64_t)(max_group)) + 63u) / 64u) * (uint64_t)(n_thresholds) * 8u)
typedef struct {
  uint32_t struct_size;    /* = sizeof(t3d_detect_nms_sweep_args) of the caller's header (see T3D_ABI_VERSION) */
  int n; int n_groups; int metric;
  const float* corners;            /* [n,8,3], as for t3d_detect_nms */
  const float* score;              /* [n] */
  const int32_t* group_offsets;    /* [n_groups + 1] */
  const int32_t* members;          /* [group_offsets[n_groups]] */
  int max_group;
  int n_thresholds;                /* K */
  float thresholds[16];            /* the first K are read (T3D_NMS_SWEEP_MAX_THRESHOLDS entries) */
  int M;
  int listed_stride;
  int keep_stride;
  const int32_t* config_threshold; /* [M] device: -1 or an index into thresholds */
  const uint8_t* listed;           /* [M, listed_stride] device, or NULL */
  void* workspace;
  uint64_t workspace_bytes;
  uint8_t* keep;                   /* [M, keep_stride] out */
  int32_t* n_kept;                 /* [M] out */
} t3d_detect_nms_sweep_args;
#define T3D_V2_SIZE_detect_nms_sweep_args 184
int t3d_detect_nms_sweep(const t3d_detect_nms_sweep_args* args, t3d_stream_t stream);

/* ---- Threshold sweep, part 2: the official evaluation of one class for many subsets of its detections (csrc/sunrgbd_sweep.hip;
 *      evaluate_sunrgbd.sweep_class, detect --sweep) ----
 * `eval` is one class's evaluation exactly as t3d_sunrgbd_eval takes it, and every one of its outputs is written with the bytes
 * t3d_sunrgbd_eval writes for the same input (the entry point calls it); eval->gt_difficult must be NULL.  Configuration m of the M
 * given is the evaluation of the detections i with mask[m, det_index[i]] != 0 alone, in file order (det_index == NULL: column i; a
 * column outside [0, mask_stride) selects nothing).  det_index lets one matrix over the detections of all classes -- the `keep` of
 * t3d_detect_nms_sweep -- serve every class without a gather.  max_overlap and gt_idx of a detection do not depend on the other
 * detections, and the stable order of a subset is the induced order, so per configuration:
 *   a selected detection claims box gt_idx - 1 iff gt_idx > 0 and max_overlap >= eval->threshold; it is a true positive iff it also has
 *   the smallest rank among the selected claimers of that box (an integer minimum, as the evaluation finds its first claimer); every
 *   other selected detection is a false positive; an unselected detection counts in neither sum.
 *   ap[m]       by the curve code that computes eval->ap, over the full order, with n_pos = G (integer cumulative sums, recall =
 *               ctp / G, precision = ctp / (cfp + ctp), the VOC2011 envelope, the same fixed summation tree).  A row of ones therefore
 *               gives the bytes of eval->ap.  P == 0, G == 0 or an empty row give 0.
 *   n_det[m], n_tp[m], n_fp[m]   the selected detections, and the true and false positives among them.
 * workspace: T3D_SUNRGBD_SWEEP_WORKSPACE_BYTES(M, G) bytes, 8-byte aligned, separate from eval->workspace (which is read): the first
 * claimer's rank per (configuration, box).  Not read when G == 0.
 * Three launches behind the evaluation's: the claims are cleared, made (one thread per configuration and detection), and the curves
 * run one workgroup per configuration.  Nothing is allocated or synchronised with the host; the only atomics are integer minima, so
 * equal inputs give equal bytes.
 * T3D_ERR_ABI: a struct of another size (either one).  T3D_ERR_ARG: a NULL struct or output array, gt_difficult != NULL, a NULL mask or
 * a mask_stride < P (< 1 with det_index) when P > 0, a workspace that is missing, too small or misaligned when G > 0, and whatever
 * t3d_sunrgbd_eval refuses.  T3D_ERR_SHAPE: M outside [1, T3D_SWEEP_MAX_CONFIGS], and eval's shapes.  Nothing is launched then. */
#define T3D_SUNRGBD_SWEEP_WORKSPACE_BYTES(M, G) ((uint64_t)(M) * (uint64_t)(G) * 4u + 8u)
typedef struct {
  uint32_t struct_size;    /* = sizeof(t3d_sunrgbd_sweep_args) of the caller's header (see T3D_ABI_VERSION) */
  int M;
  const uint8_t* mask;             /* [M, mask_stride] device */
  const int32_t* det_index;        /* [P] device: the column of detection i, or NULL for i */
  int mask_stride;
  void* workspace;
  uint64_t workspace_bytes;
  double* ap;                      /* [M] out */
  int32_t* n_det;                  /* [M] out */
  int32_t* n_tp;                   /* [M] out */
  int32_t* n_fp;                   /* [M] out */
} t3d_sunrgbd_sweep_args;
#define T3D_V2_SIZE_sunrgbd_sweep_args 80
int t3d_sunrgbd_eval_sweep(const t3d_sunrgbd_eval_args* eval, const t3d_sunrgbd_sweep_args* sweep, t3d_stream_t stream);

/* ---- Bootstrap over images, part 1: the resampling weights (csrc/sunrgbd_bootstrap.hip; bootstrap.Weights) ----
 * weights[r, c], r < R, c < n_images: how often column c is drawn when replicate r draws n_images columns with replacement.  Draw d of
 * replicate r is, in unsigned 64-bit arithmetic (wrapping),
 *     key = (((uint64)seed << 32) | (uint64)r) * 0x9E3779B97F4A7C15 + ((uint64)d + 1) * 0xD6E8FEB86659FD93
 *     u   = mix_u32(key)                     the finaliser of data.hip / frustum.hip:  x ^= x >> 33; x *= 0xff51afd7ed558ccd;
 *                                            x ^= x >> 33; x *= 0xc4ceb9fe1a85ec53; x ^= x >> 33; u = (uint32)(x >> 16)
 *     column = ((uint64)u * (uint64)n_images) >> 32
 * The columns n_images .. stride-1 of a row are written 0.  Two launches: the matrix is cleared, then one thread per (replicate, draw)
 * counts with an integer atomic add -- the only atomics, so equal inputs give equal bytes, and every row sums to n_images.  Nothing is
 * allocated or synchronised with the host.
 * T3D_ERR_ABI: a struct of another size.  T3D_ERR_ARG: a NULL struct or matrix, stride < n_images.  T3D_ERR_SHAPE: R outside
 * [1, T3D_BOOTSTRAP_MAX_REPLICATES], n_images < 1.  Nothing is launched then. */
#define T3D_BOOTSTRAP_MAX_REPLICATES (1 << 16)
typedef struct {
  uint32_t struct_size;    /* = sizeof(t3d_bootstrap_weights_args) of the caller's header (see T3D_ABI_VERSION) */
  uint32_t seed;
  int R;
  int n_images;
  int stride;                      /* elements between two rows, >= n_images */
  int32_t* weights;                /* [R, stride] out, device */
} t3d_bootstrap_weights_args;
#define T3D_V2_SIZE_bootstrap_weights_args 32
int t3d_bootstrap_weights(const t3d_bootstrap_weights_args* args, t3d_stream_t stream);

/* ---- Bootstrap over images, part 2: the official AP of one class on R resampled image lists (csrc/sunrgbd_bootstrap.hip;
 *      evaluate_sunrgbd.bootstrap_class, --bootstrap) ----
 * `eval` is one class's evaluation exactly as t3d_sunrgbd_eval takes it, and every one of its outputs is written with the bytes
 * t3d_sunrgbd_eval writes for the same input (the entry point calls it); eval->gt_difficult must be NULL.  A detection is matched only
 * against the boxes of its own image, so max_overlap, gt_idx, is_tp and is_fp are the same in every copy of its image: a replicate in
 * which the image of weight column c occurs weights[r, c] times is the same ranked list with integer weights, and only the curve is new.
 * det_col[i] / gt_col[g]: the weight column of the image of detection i / of box g; a column outside [0, weight_stride) has weight 0.
 * Replicate r, with w_i = weights[r, det_col[i]], over the full stable order eval->order:
 *   detection i adds w_i * is_tp[i] to the true-positive cumulative sum and w_i * is_fp[i] to the false-positive one;
 *   n_pos[r] = the sum of weights[r, gt_col[g]] over the boxes; n_tp[r], n_fp[r] the two totals; all counts are 64-bit;
 *   ap[r]    recall = ctp / n_pos, precision = ctp / (cfp + ctp) (0 / 0 is NaN, which the running maximum ignores), the VOC2011
 *            envelope and the area as the curve code that computes eval->ap forms them, with its chunking (ceil(P / 1024) consecutive
 *            ranks per thread) and its fixed summation tree for the same P.  A row of ones therefore gives the bytes of eval->ap.
 *            n_pos[r] == 0 or P == 0 give 0.
 * This equals the literal evaluation of the resampled data set: every image copy becomes a distinct image, and the copies of a
 * detection are adjacent in file order.  Inside a block of m copies of a true positive the precision rises.  Inside a block of false
 * positives it falls and the recall does not move.  So only block ends reach the envelope, and the block contributes
 * (m / n_pos) * envelope.  (The literal sum adds the block's m steps of 1 / n_pos one by one: the two differ by rounding alone.)
 * workspace: T3D_SUNRGBD_BOOTSTRAP_WORKSPACE_BYTES(P) bytes, 8-byte aligned, separate from eval->workspace: the rank-ordered stream
 * det_col << 1 | is_tp per detection, -1 for one that counts in neither sum.  Not read when P == 0.
 * Two launches behind the evaluation's: the stream is written, then the curves run one workgroup of 1024 threads per replicate, one
 * replicate per pass over the stream.  The workgroup stages its weight row in LDS when 4 * weight_stride bytes fit beside the scan
 * scratch in the 160 KiB of a CU, and gathers from global memory otherwise; both paths give the same bytes.  Nothing is allocated or
 * synchronised with the host and there are no atomics of its own, so equal inputs give equal bytes.
 * T3D_ERR_ABI: a struct of another size (either one).  T3D_ERR_ARG: a NULL struct, weight matrix or output array, gt_difficult != NULL,
 * det_col NULL when P > 0, gt_col NULL when G > 0, a workspace that is missing, too small or misaligned when P > 0, and whatever
 * t3d_sunrgbd_eval refuses.  T3D_ERR_SHAPE: R outside [1, T3D_BOOTSTRAP_MAX_REPLICATES], weight_stride outside [1, 2^30], and eval's
 * shapes.  Nothing is launched then. */
#define T3D_SUNRGBD_BOOTSTRAP_WORKSPACE_BYTES(P) ((uint64_t)(P) * 4u + 8u)
typedef struct {
  uint32_t struct_size;    /* = sizeof(t3d_sunrgbd_bootstrap_args) of the caller's header (see T3D_ABI_VERSION) */
  int R;
  const int32_t* weights;          /* [R, weight_stride] device */
  int weight_stride;
  const int32_t* det_col;          /* [P] device */
  const int32_t* gt_col;           /* [G] device */
  void* workspace;
  uint64_t workspace_bytes;
  double* ap;                      /* [R] out */
  int64_t* n_pos;                  /* [R] out */
  int64_t* n_tp;                   /* [R] out */
  int64_t* n_fp;                   /* [R] out */
} t3d_sunrgbd_bootstrap_args;
#define T3D_V2_SIZE_sunrgbd_bootstrap_args 88
int t3d_sunrgbd_eval_bootstrap(const t3d_sunrgbd_eval_args* eval, const t3d_sunrgbd_bootstrap_args* boot, t3d_stream_t stream);

/* ---- Soft-NMS: a box that overlaps a better one keeps its place and loses confidence (Bodla et al., ICCV 2017; csrc/soft_nms.hip;
 *      nms.DeviceSoftNms, detect --soft_nms) ----
 * t3d_detect_nms makes one decision per pair, so a threshold low enough to remove a duplicate report also removes a true neighbour
 * (chairs in a row).  Here the confidence of an overlapped box is multiplied down by a function of the IoU: the duplicate moves to the
 * tail of the ranked list, the neighbour with moderate overlap keeps most of its confidence.  The reference has no such step; it is
 * opt-in.  n, n_groups, metric, corners, score, group_offsets, members and max_group are those of t3d_detect_nms, under the same contract
 * and with the same leading layout; the IoU is the same box3d_iou_corners.  Per group:
 *   1 Working score   every box starts with its input score.  A listed box whose score is not a finite number above 0 takes no part:
 *                     it decays nothing and is never decayed, and comes back kept -- keep 1, suppressed_by -1, score_out the input
 *                     bits, n_decays 0.  The others are live.
 *   2 Selection       until no box is live: the live box with the largest working score is selected; on equal scores the lower box
 *                     index wins, as in t3d_detect_nms.  It is kept (keep 1, suppressed_by -1), is live no longer, and its score_out is
 *                     its working score at that moment.
 *   3 Decay           for every box j still live, IoU(selected, j) under `metric`, THE SELECTED BOX AS THE FIRST ARGUMENT (both boxes
 *                     and their order are the group's own: nothing outside the group enters).  A NaN IoU decays nothing.
 *                       T3D_SOFT_NMS_GAUSSIAN   if IoU > 0:          score *= exp(-IoU^2 / sigma)
 *                       T3D_SOFT_NMS_LINEAR     if IoU > threshold:  score *= 1 - IoU
 *                     in fp32 (expf).  Two boxes whose centres lie farther apart than their half diagonals add up to cannot touch:
 *                     their IoU is 0 and is not computed.  Both boxes are handed to box3d_iou_corners with x and z relative to the
 *                     selected box's first corner: far from the origin the function's rectangle areas lose digits (1e-4 of the
 *                     ground-plane IoU at 45 m), which a decayed score would carry; t3d_detect_nms passes them as they come.
 *   4 Prune           a box whose working score falls below min_score (strictly) by a decay leaves the group: keep 0, suppressed_by =
 *                     the selected box whose decay took it below the floor, score_out the value it fell to.  Only a decayed box is
 *                     pruned: a box nothing overlapped keeps its score bits, whatever they are.
 *   5 n_decays        n_decays[j] = the number of selected boxes that decayed j.
 *   6 Unlisted boxes  a box in no group is not visited: its four outputs keep what they held, as in t3d_detect_nms.
 * Consequences: with LINEAR, threshold T and a min_score above every score, every decayed box is pruned at its first decay, and keep /
 * suppressed_by are those of t3d_detect_nms at T and the same metric, byte for byte, for every box that takes part (where no IoU lies
 * within the rounding of the two calls, a few 1e-5, of T); and a group's outputs are a function of its own boxes only, wherever they
 * sit in the call.
 *   Errors            as t3d_detect_nms (T3D_ERR_SHAPE for max_group > T3D_DETECT_NMS_MAX_GROUP; T3D_ERR_ARG for n, n_groups or max_group
 *                     < 0, an unknown metric, a null corners / score / group_offsets / members / score_out / keep / suppressed_by /
 *                     n_decays on a call that is not empty), and T3D_ERR_ARG for an unknown method, for sigma not a finite number above
 *                     0 with GAUSSIAN, for min_score NaN or negative, and for a workspace smaller than
 *                     T3D_DETECT_SOFT_NMS_WORKSPACE_BYTES(n, max_group) or, where that is not 0, null or misaligned.  Nothing is
 *                     launched then.  n == 0, n_groups == 0 or max_group == 0: T3D_OK without a launch.
 * One launch on `stream`: a group has LPG lanes, the power of two >= max_group / 4, at most 64, so 64 / LPG groups share a wave and walk
 * their selections in lockstep; a lane owns the boxes at list positions lane, lane + LPG, ... of its group (up to 4 where max_group <=
 * 256, at most 16) and keeps their live bits in a register; the working scores live in score_out.  Per step each lane finds its best live box, a butterfly of shuffles
 * finds the group's, every lane reads the winner's corners (one address: a broadcast) and decays its own boxes.  No workspace (the
 * macro is 0 and `workspace` may be NULL; the fields are there for a form that stores IoUs), no LDS, no atomics, no allocation, no
 * host synchronisation: equal inputs give equal bytes. */
#define T3D_SOFT_NMS_GAUSSIAN 0
#define T3D_SOFT_NMS_LINEAR 1
#define T3D_DETECT_SOFT_NMS_WORKSPACE_BYTES(n, max_group) ((uint64_t)0 * ((uint64_t)(n) + (uint64_t)(max_group)))
typedef struct {
  uint32_t struct_size;    /* = sizeof(t3d_detect_soft_nms_args) of the caller's header (see T3D_ABI_VERSION) */
  int n; int n_groups; int metric;
  const float* corners;            /* [n,8,3], as for t3d_detect_nms */
  const float* score;              /* [n] */
  const int32_t* group_offsets;    /* [n_groups + 1] */
  const int32_t* members;          /* [group_offsets[n_groups]] */
  float threshold;                 /* LINEAR: the IoU above which a box is decayed; GAUSSIAN: not read */
  int max_group;
  int method;                      /* T3D_SOFT_NMS_* */
  float sigma;                     /* GAUSSIAN: > 0; LINEAR: not read */
  float min_score;                 /* >= 0: the floor below which a decayed box is pruned */
  int reserved;                    /* 0 */
  void* workspace;
  uint64_t workspace_bytes;
  float* score_out;                /* [n] out: the working score a box was selected or pruned with */
  uint8_t* keep;                   /* [n] out: 0 for a pruned box */
  int32_t* suppressed_by;          /* [n] out: -1, or the selected box whose decay pruned this one */
  int32_t* n_decays;               /* [n] out */
} t3d_detect_soft_nms_args;
#define T3D_V2_SIZE_detect_soft_nms_args 120
int t3d_detect_soft_nms(const t3d_detect_soft_nms_args* args, t3d_stream_t stream);

/* ---- Localisation errors split into centre, size and heading (csrc/sunrgbd_locparts.hip; evaluate_sunrgbd.py
 *      diagnose_class(parts=True), --diagnose_parts) ----
 * T3D_DIAG_LOC says a detection sits on its own box but too loosely (t_b <= overlap < t_f).  This call says which parameter group of
 * the box is to blame: TIDE's idea one level down, after the true-positive metrics of nuScenes (translation, scale, orientation error),
 * restated for this protocol's prism overlap, its matching and its VOC2011 AP.
 * It first calls t3d_sunrgbd_diagnose(eval, diag, stream): every output of both structs has the bytes that call writes, and whatever it
 * refuses is refused here.  Then, for upright boxes (what both parsers produce), per detection i with g = gt_idx[i] - 1 >= 0 -- the
 * detection is A, its arg-max box is B:
 *   Rows        the vertical row of a box is the basis row with the largest |z component|, the first on ties; the other two, in row
 *               order, are its horizontal rows a0, a1 (of B: b0, b1).  A row's size is |coeff|.
 *   Pairing     on the xy components p = |a0 . b0|, q = |a0 . b1|: p >= q pairs a0 with b0 and a1 with b1, otherwise a0 with b1 and a1
 *               with b0 (a box equals itself turned by pi/2 with l and w exchanged).  The vertical rows pair with each other.
 *   loc_error   [i][0] hypot(Ax - Bx, Ay - By); [1] Az - Bz, signed; [2..4] log(size of the partner row of A / size) for b0, b1 and the
 *               vertical row of B, signed (l, w, h for ground truth from label files); [5] the heading error atan2(min(p, q),
 *               max(p, q)) in [0, pi/4].
 *   Counterfactual boxes, one per part:
 *     T3D_LOCPART_XY       A with B's x and y;
 *     T3D_LOCPART_Z        A with B's z;
 *     T3D_LOCPART_CENTRE   A with B's centroid;
 *     T3D_LOCPART_SIZE     A's centroid and basis, each row's size replaced by its partner's;
 *     T3D_LOCPART_HEADING  A's centroid and B's basis, each row of B carrying the size of its partner row of A.
 *   part_overlap[i][f]     the evaluation's own overlap (ev_overlap of the ev_footprints) of counterfactual box f with B; a box of
 *                          zero volume overlaps nothing, here as there.
 *   Where gt_idx[i] == 0 the five overlaps are 0 and the six errors NaN.
 * A LOC detection is REPAIRED BY f iff part_overlap[i][f] >= t_f.  ap_part[f] is the AP of that variant, by the curve code and the
 * summation tree of `ap` and `ap_fixed`: true positives stay; per box in state 2 the best-ranked repaired detection that chose it
 * becomes a true positive (an integer minimum over ranks); every other repaired detection -- one on a claimed box included -- is
 * removed and counts in neither sum; unrepaired LOC detections and all other false positives stay false positives; n_pos = G.
 * part_counts[f]: the repaired LOC detections; part_boxes[f]: the boxes that gain a true positive.
 * P == 0 or G == 0: all zeros, as ap_fixed.  A part that repairs nothing has the bytes of `ap`; one that repairs every LOC detection
 * those of ap_fixed[T3D_DIAG_FIX_LOC].
 * THE PARTS DO NOT ADD UP: a box off in xy and in z may be repaired by either fix alone, or only by CENTRE; a detection may be repaired
 * by several parts or by none, so neither the counts nor the AP gains sum to those of T3D_DIAG_FIX_LOC.
 * workspace: T3D_SUNRGBD_LOCPARTS_WORKSPACE_BYTES(P, G) bytes (five int32[G] arrays of ranks), separate from the other two.
 * Three launches behind the diagnosis': the rank arrays; one thread per (detection, part), so that a lane clips once; six workgroups,
 * five curves and the counts.  Everything is fp64.  Nothing is allocated or synchronised with the host; the only atomics are integer
 * minima, so equal inputs give equal bytes.
 * T3D_ERR_ABI: a struct of another size (any of the three).  T3D_ERR_ARG: a NULL struct or output, reserved != 0, a workspace that is
 * NULL or too small where G > 0, and whatever t3d_sunrgbd_diagnose refuses; T3D_ERR_SHAPE: its shapes.  Nothing is launched then. */
#define T3D_LOCPART_XY 0
#define T3D_LOCPART_Z 1
#define T3D_LOCPART_CENTRE 2
#define T3D_LOCPART_SIZE 3
#define T3D_LOCPART_HEADING 4
#define T3D_SUNRGBD_LOCPARTS_WORKSPACE_BYTES(P, G) ((uint64_t)(G) * 20u + (uint64_t)(P) * 0u + 8u)
typedef struct {
  uint32_t struct_size;    /* = sizeof(t3d_sunrgbd_locparts_args) of the caller's header (see T3D_ABI_VERSION) */
  int reserved;                        /* 0 */
  void* workspace;
  uint64_t workspace_bytes;
  double* part_overlap;                /* [P,5] out, file order: T3D_LOCPART_* */
  double* loc_error;                   /* [P,6] out, file order */
  int32_t* part_counts;                /* [5] out */
  int32_t* part_boxes;                 /* [5] out */
  double* ap_part;                     /* [5] out */
} t3d_sunrgbd_locparts_args;
#define T3D_V2_SIZE_sunrgbd_locparts_args 64
int t3d_sunrgbd_locparts(const t3d_sunrgbd_eval_args* eval, const t3d_sunrgbd_diagnose_args* diag,
                         const t3d_sunrgbd_locparts_args* parts, t3d_stream_t stream);

/* ---- Rescoring: one confidence from the label-free measures of a detection (csrc/rescore.hip; transferable3d_amd/rescore.py) ----
 * The decode, t3d_detect_consistency and t3d_detect_ensemble each say something about a finished 3-D box; the confidence the result
 * files carry is still the 2-D detector's.  These three calls turn the measures into one number: a feature matrix built from the stage
 * buffers where they lie, an L2-regularised logistic regression fitted on the detections whose class has 3-D labels (y: what
 * t3d_sunrgbd_eval says about them), and the model applied to every detection.  The reference has no such step; it is opt-in.
 * Everything is fp64.  No floating-point atomics (none at all), no allocation, no host synchronisation: equal inputs give equal bytes.
 *
 * t3d_rescore_features -- X[i][k], row stride ld, k counting the set bits of feature_mask in ascending bit order.  Per detection i < n,
 * every operation below its own fp64 operation (no contraction):
 *   bit 0 logit_prob   p = (double)prob[i]; p = p < 1e-6 ? 1e-6 : p; p = p > 1 - 1e-6 ? 1 - 1e-6 : p (a NaN stays);  log(p / (1 - p))
 *   bit 1 score        (double)score[i]
 *   bit 2 reproj_iou   reproj[i][4]                                            (t3d_detect_consistency's `reproj`, [n,5])
 *   bit 3 mask_in_box  n_mask > 0 ? (double)n_both / (double)n_mask : 0        (its `counts` [n,4]: n_mask, n_box, n_both, flags)
 *   bit 4 seg_box_iou  u = n_mask + n_box - n_both (64-bit integer);  u > 0 ? (double)n_both / (double)u : 0
 *   bit 5 log_mask     log1p((double)n_mask)
 *   bit 6 view_iou     (double)view_iou[i]                                     (t3d_detect_ensemble's `agreement`)
 * Columns 1, 2, 3, 4 and 6 have the bits a NumPy transcription gives.  Columns 0 and 5 go through log / log1p of two libraries, each
 * within 1 ulp of the true value: within 2 ulps of each other.  Columns k >= popcount(feature_mask) of a row are not written.
 * T3D_ERR_ARG: a NULL struct or X, feature_mask 0 or with a bit above 6, a NULL input that a selected feature reads (view_iou selected
 * and NULL included); T3D_ERR_SHAPE: n < 0, ld < popcount(feature_mask).  n == 0: T3D_OK without a launch.
 *
 * t3d_rescore_fit -- minimises over (w [F], b), on the rows with r[i] > 0 (a row with r[i] == 0, or a NaN weight, takes no part whatever
 * it holds), W = sum r:
 *     J(w, b) = (1/W) sum_i r_i ( log(1 + exp(z_i)) - y_i z_i ) + lambda/2 |w|^2,   z_i = b + sum_j w_j xs_ij,   y_i = (y[i] != 0)
 * on the standardised columns xs_ij = (X[i][j] - mean_j) * (1 / scale_j).  The intercept b is not penalised (lambda enters the
 * gradient and the diagonal of the Hessian for the F feature coefficients only).
 *   Standardisation  one kernel: per slice the weighted sum, then the weighted squared deviations from the slice's own mean (the slice
 *                    is read twice by the workgroup that holds it), the minimum and the maximum of every column; the slices are
 *                    merged in slice order by the pairwise update of Chan, Golub and LeVeque.  mean_j is the weighted mean, scale_j
 *                    the square root of (weighted squared deviations / W).  A column with minimum == maximum (or a deviation that is
 *                    not above 0) gets scale 1 -- and, where minimum == maximum, that value as its mean, so its standardised column
 *                    is exactly 0 -- and sets T3D_RESCORE_CONSTANT_COLUMN.
 *   Start            w = 0, b = log(Wy / (W - Wy)), Wy = sum r_i y_i.
 *   Iteration        max_iter evaluations are enqueued (0: the default 30), each a launch over the slices and a one-workgroup launch.
 *                    An evaluation at the trial point gives J, the gradient and the Hessian  (1/W) Xs^T diag(r p (1-p)) Xs + lambda I_F.
 *                    The first evaluation, and every one whose J is <= the J of the last accepted point, is ACCEPTED: J is appended to
 *                    `loss`, the point becomes the accepted point, and -- unless |gradient|_inf <= gtol (0: the default 1e-9), which
 *                    ends the fit -- the next trial point is accepted + step, step = -Hessian^-1 gradient by Cholesky.  Otherwise
 *                    (J larger, or not a number) the step is halved and the next trial point is accepted + step; after
 *                    T3D_RESCORE_MAX_HALVINGS halvings in a row the fit ends unconverged.  So loss[0 .. n_iter-1] never increases.
 *                    A Hessian that Cholesky refuses ends the fit unconverged too.  Once the fit has ended the remaining launches
 *                    return at their first instruction; the host never reads the flag.
 *   Reduction        a workgroup of 256 threads owns one slice of T3D_RESCORE_SLICE consecutive rows -- the cuts depend on n alone,
 *                    never on the number of CUs -- and writes the slice's sums to the workspace; the one-workgroup launch adds the
 *                    slices in slice order.  The Gram matrix of a slice is accumulated by v_mfma_f64_16x16x4_f64, four rows at a
 *                    time per wave, the four waves' matrices added in wave order.
 *   Outputs          coef_std [F+1]: w then b on the standardised columns, at the last accepted point; coef [F+1]: the same model in
 *                    raw feature units, coef[j] = w_j * (1 / scale_j) and coef[F] = b - sum_j coef[j] mean_j (ascending j), what
 *                    t3d_rescore_apply reads; mean [F], scale [F]; loss [max_iter]: the accepted J's, NaN behind them; n_iter: how
 *                    many were accepted; n_rows, n_pos: the rows with r > 0 and those of them with y != 0; status: T3D_RESCORE_* bits.
 *   T3D_RESCORE_NO_ROWS          W is not above 0.  mean 0, scale 1, every coefficient 0.  (T3D_OK: the call itself succeeded.)
 *   T3D_RESCORE_ONE_CLASS        n_pos == 0 or n_pos == n_rows.  No iteration runs; w = 0 and b = logit((Wy + 0.5) / (W + 1)).
 *   T3D_RESCORE_CONSTANT_COLUMN  above.  The fit runs; the column's coefficient is 0 (its standardised column is 0, the ridge does the rest).
 *   T3D_RESCORE_NOT_CONVERGED    the enqueued evaluations ran out, the halvings did, or Cholesky refused.
 *   T3D_RESCORE_NONFINITE        a row with r > 0 holds a NaN or an Inf in one of its F columns or in r.  No iteration runs and the
 *                                coefficients are 0: the result is not to be used.
 *   Equal bytes      two calls on equal inputs give equal bytes.  The SAME weighted rows interleaved with zero-weight rows in a larger
 *                    call fall into other slices, so the sums are formed in another order: the coefficients then agree within the
 *                    rounding of the sums (the tests bound it), not byte for byte.
 *   workspace        T3D_RESCORE_FIT_WORKSPACE_BYTES(n) bytes, 8-byte aligned; its content means nothing before or after the call.
 * T3D_ERR_ARG: a NULL struct, reserved != 0, lambda not above 0 (NaN included), gtol < 0 or NaN, max_iter < 0 or > 1000, a NULL output, a NULL
 * X, y or r where n > 0, a workspace that is NULL, misaligned or too small.  T3D_ERR_SHAPE: n < 0, F < 1, F > T3D_RESCORE_MAX_FEATURES,
 * ld < F.  n == 0 is a fit without rows: T3D_RESCORE_NO_ROWS.
 *
 * t3d_rescore_apply -- per row i < n_valid:  z = coef[F];  z = z + coef[j] * X[i][j] for j = 0 .. F-1 in this order, the product and
 * the sum each rounded (no fused multiply-add);  out[i] = 1 / (1 + exp(-z)).  exp is within 1 ulp of the true value here and in the
 * NumPy transcription, so the two differ by at most 4 u in exp, 6 u in the sum and 8 u = 2^-50 relative in out (u = 2^-53).
 * out32[i] = (float)out[i] where out32 is not NULL: the ranking the suppression stages read.  Rows n_valid .. n-1 keep what they held.
 * coef is device memory (what the fit wrote).  T3D_ERR_ARG: a NULL struct, X, coef or out, reserved != 0; T3D_ERR_SHAPE: n < 0,
 * n_valid < 0 or > n, F < 1 or > T3D_RESCORE_MAX_FEATURES, ld < F.  n_valid == 0: T3D_OK without a launch. */
#define T3D_RESCORE_MAX_FEATURES 15
#define T3D_RESCORE_SLICE 2048
#define T3D_RESCORE_MAX_HALVINGS 30
#define T3D_RESCORE_N_FEATURES 7         /* the named features: bits 0 .. 6 of feature_mask */
#define T3D_RESCORE_F_LOGIT_PROB 1u
#define T3D_RESCORE_F_SCORE 2u
#define T3D_RESCORE_F_REPROJ_IOU 4u
#define T3D_RESCORE_F_MASK_IN_BOX 8u
#define T3D_RESCORE_F_SEG_BOX_IOU 16u
#define T3D_RESCORE_F_LOG_MASK 32u
#define T3D_RESCORE_F_VIEW_IOU 64u
#define T3D_RESCORE_NO_ROWS 1u
#define T3D_RESCORE_ONE_CLASS 2u
#define T3D_RESCORE_CONSTANT_COLUMN 4u
#define T3D_RESCORE_NOT_CONVERGED 8u
#define T3D_RESCORE_NONFINITE 16u
#define T3D_RESCORE_SLICES(n) (((uint64_t)(n) + T3D_RESCORE_SLICE - 1u) / T3D_RESCORE_SLICE)
/* 128 doubles of state, and per slice 80 doubles of column statistics and 288 of one evaluation's sums */
#define T3D_RESCORE_FIT_WORKSPACE_BYTES(n) ((128u + T3D_RESCORE_SLICES(n) * 368u) * 8u)
typedef struct {
  uint32_t struct_size;    /* = sizeof(t3d_rescore_features_args) of the caller's header (see T3D_ABI_VERSION) */
  int n; int ld;
  uint32_t feature_mask;               /* T3D_RESCORE_F_* */
  const float* prob;                   /* [n] the 2-D detector's confidence */
  const float* score;                  /* [n] what t3d_detect_decode wrote */
  const double* reproj;                /* [n,5] what t3d_detect_consistency wrote */
  const int32_t* counts;               /* [n,4] what t3d_detect_consistency wrote */
  const float* view_iou;               /* [n] t3d_detect_ensemble's agreement, or NULL */
  double* X;                           /* [n,ld] out */
} t3d_rescore_features_args;
#define T3D_V2_SIZE_rescore_features_args 64
int t3d_rescore_features(const t3d_rescore_features_args* args, t3d_stream_t stream);

typedef struct {
  uint32_t struct_size;    /* = sizeof(t3d_rescore_fit_args) of the caller's header (see T3D_ABI_VERSION) */
  int n; int F; int ld;
  int max_iter;                        /* evaluations to enqueue; 0: 30 */
  int reserved;                        /* 0 */
  const double* X;                     /* [n,ld] */
  const uint8_t* y;                    /* [n] */
  const double* r;                     /* [n] row weights, >= 0 */
  double lambda;                       /* > 0 */
  double gtol;                         /* 0: 1e-9 */
  void* workspace;
  uint64_t workspace_bytes;
  double* coef;                        /* [F+1] out: raw units, the intercept last */
  double* coef_std;                    /* [F+1] out: standardised units, the intercept last */
  double* mean;                        /* [F] out */
  double* scale;                       /* [F] out */
  double* loss;                        /* [max_iter] out */
  int32_t* n_iter;                     /* [1] out */
  uint32_t* status;                    /* [1] out */
  int64_t* n_rows;                     /* [1] out */
  int64_t* n_pos;                      /* [1] out */
} t3d_rescore_fit_args;
#define T3D_V2_SIZE_rescore_fit_args 152
int t3d_rescore_fit(const t3d_rescore_fit_args* args, t3d_stream_t stream);

typedef struct {
  uint32_t struct_size;    /* = sizeof(t3d_rescore_apply_args) of the caller's header (see T3D_ABI_VERSION) */
  int n; int n_valid; int F; int ld;
  int reserved;                        /* 0 */
  const double* X;                     /* [n,ld] */
  const double* coef;                  /* [F+1] device memory: raw units, the intercept last */
  double* out;                         /* [n] out */
  float* out32;                        /* [n] out, or NULL */
} t3d_rescore_apply_args;
#define T3D_V2_SIZE_rescore_apply_args 56
int t3d_rescore_apply(const t3d_rescore_apply_args* args, t3d_stream_t stream);

/* ---- Scene synthesis: depth points, image and visibility of box scenes by ray casting (csrc/scene_synth.hip;
 *      transferable3d_amd/synth_scenes.py) ----
 * t3d_scene_raycast casts one ray per pixel of an H x W image against the oriented boxes ("parts") of each scene of a batch and the
 * axis-aligned room around them, and writes what a depth camera at the origin would see: which surface every pixel shows, a shaded
 * image, and the compacted rows `x y z r g b` of the strided pixels in upright depth coordinates -- the layout of a SUN-RGBD depth file,
 * the exact inverse of the projection t3d_frustum_extract applies.  Everything is fp64, no operation is contracted into a fused
 * multiply-add, every random number is a counter-based hash of (seed, scene id, pixel): a scene's outputs are a function of its inputs
 * and its scene id, never of the batch it is cast in or of the order of anything.  Three launches, no host synchronisation, no
 * floating-point atomic (the integer minima, maxima and counts of `vis_box` / `visible` do not depend on order).
 *
 *   Scene s < n_scenes   rtilt[s][9], K[s][9] row-major;  scene_id[s];  room[s][6] = x0, x1, y0, y1, z0, z1 with lo < 0 < hi on every
 *                        axis (the camera is the origin, strictly inside);  its parts are part_offsets[s] .. part_offsets[s+1]-1 of
 *                        `parts`, at most T3D_SCENE_MAX_PARTS of them, staged in LDS once per workgroup;  n_objects_host[s] <=
 *                        T3D_SCENE_MAX_OBJECTS.  A part index below is the index within the scene.
 *   Part                 centre, half (half-extents along its own axes), cos_r and sin_r of its rotation r about the up axis z (its own
 *                        x axis is (cos_r, sin_r, 0) in the scene), colour[3] in [0, 255], owner: the ordinal of the object it belongs
 *                        to; an owner outside [0, T3D_SCENE_MAX_OBJECTS) belongs to nothing (it is seen, and counted for nobody).
 *   Ray of pixel (u, v)  cx = (u - K[2]) / K[0];  cy = (v - K[5]) / K[4];  q = (cx, 1, -cy);
 *                        d[i] = (rtilt[3i] * q[0] + rtilt[3i+1] * q[1]) + rtilt[3i+2] * q[2].  d is not normalised: the parameter t of
 *                        the point t * d is the depth along the camera's forward axis.  dd = (d0*d0 + d1*d1) + d2*d2.
 *   Hit of a part        the origin and the direction in the part's frame:
 *                          o = (cos_r * -centre[0] + sin_r * -centre[1],  cos_r * -centre[1] - sin_r * -centre[0],  -centre[2])
 *                          e = (cos_r * d0 + sin_r * d1,                  cos_r * d1 - sin_r * d0,                  d2)
 *                        t_in = -DBL_MAX, t_out = DBL_MAX (compared, never computed with).  Per axis k = 0, 1, 2 in this order:
 *                          e[k] == 0:  a miss if o[k] < -half[k] or o[k] > half[k], no constraint otherwise (nothing is divided);
 *                          else  ta = (-half[k] - o[k]) / e[k],  tb = (half[k] - o[k]) / e[k];  the near one tn = e[k] > 0 ? ta : tb
 *                                and the far one tf the other;  tn > t_in: t_in = tn, the entered face is (k, sign = e[k] > 0 ? -1 : +1);
 *                                tf < t_out: t_out = tf.
 *                        A hit: t_in > 0 and t_in <= t_out.  (A part that contains the camera has t_in <= 0: it is ignored, and so is
 *                        one wholly behind the camera.)  nd = e[k] of the entered face's axis.
 *   Room                 per axis k in order with d[k] != 0: tw = (d[k] > 0 ? hi[k] : lo[k]) / d[k];  tw < t_room: t_room = tw, the wall
 *                        is (k, sign = d[k] > 0 ? +1 : -1), nd = d[k].  (No axis with d[k] != 0: the pixel is invalid.)
 *   Choice               over the parts in ascending index the first hit with the smallest t_in (a later part replaces an earlier one
 *                        only when its t_in is smaller: on equal t the lower index wins);  it is the surface if t_in <= t_room, else
 *                        the wall is;  t = that t_in or t_room.  The pixel is valid iff t <= max_range and nd * nd >= min_cos2 * dd
 *                        (min_cos2: the squared cosine between ray and normal below which a sensor sees nothing).
 *   hit [S,H,W]          the part index, T3D_SCENE_HIT_ROOM (-1) or T3D_SCENE_HIT_INVALID (-2).  Being comparisons of + - * / results
 *                        in a stated order, it equals a NumPy transcription bit for bit; so do image, scene_offsets, visible, vis_box.
 *   image [S,H,W,3]      noise-free uint8:  x = colour[c] * T3D_SCENE_SHADES[2k + (sign > 0)] + 0.5, clamped to [0, 255], truncated;  the
 *                        room's colour is T3D_SCENE_ROOM_COLOUR on every channel;  an invalid pixel is 0 0 0.
 *   Random numbers       base = ((uint64)seed << 32) ^ ((uint64)(uint32)scene_id * 0x9E3779B97F4A7C15)
 *                               ^ ((uint64)(v * W + u + 1) * 0xC2B2AE3D27D4EB4F);
 *                        U_j = ((double)mix((base ^ 0x94D049BB133111EB) + (uint64)(j + 1) * 0xBF58476D1CE4E5B9) + 0.5) * 2^-32, mix the
 *                        finaliser of t3d_frustum_extract's hash (x ^= x >> 33, x *= 0xff51afd7ed558ccd, x ^= x >> 33,
 *                        x *= 0xc4ceb9fe1a85ec53, x ^= x >> 33, bits 16..47).  0 < U_j < 1.
 *   points               a pixel is EMITTED iff u % stride == 0, v % stride == 0, it is valid and not U_0 < p_drop.  Its row:
 *                          noise_a == 0:  m = t  (no transcendental is evaluated)
 *                          else           g = sqrt(-2 * log(U_1)) * cos(6.283185307179586 * U_2);   m = t + ((noise_a * (t * t)) * g)
 *                          x y z = d[i] * m;   r g b = (its image bytes) / 255.0
 *                        Rows are compacted in (scene, v, u) order: a count per workgroup, one scan, a scatter -- the position of a row
 *                        is its rank, whatever ran first.  scene_offsets[S+1] (int64) is written on the device; point_pixel (NULL: not
 *                        wanted) receives v * W + u of every row.  points_capacity >= S * ceil(H/stride) * ceil(W/stride) rows.
 *                        With noise_a == 0 the rows equal the NumPy transcription bit for bit.  With noise, the two sides call two
 *                        libraries: log within 1 ulp on both (2 between them, 1 after the square root halves it), sqrt correctly
 *                        rounded on both (0.5 + 0.5), cos within 2 ulps on the device and 1 on the host (3), the product 0.5 + 0.5:
 *                        g differs by at most 6 ulps, bounded as 8 * 2^-52 * |g| with the second-order terms.  m then differs by
 *                        that times noise_a * t * t plus one ulp of m for its two roundings, and a coordinate by one ulp more:
 *                            |x_device - x_numpy| <= 2^-52 * (8 * |d[i]| * noise_a * t * t * |g| + 3 * |x|)
 *                        (the third |x| covers |d[i]| * |m| against |x| and every second-order term).  Derived, not measured.
 *   visible [S,64]       per object: the emitted pixels whose part it owns.
 *   vis_box [S,64,4]     per object: umin, vmin, umax, vmax over ALL valid pixels (stride 1) whose part it owns; W, H, -1, -1 for none.
 *   workspace            T3D_SCENE_WORKSPACE_BYTES(S, H, W) bytes, 8-byte aligned; its content means nothing before or after the call.
 * T3D_ERR_ARG: a NULL struct, input, output (point_pixel excepted) or host array, reserved != 0, a workspace that is NULL, misaligned or
 * too small, points_capacity too small, a room that does not strictly contain the origin (a NaN bound included), p_drop or noise_a
 * negative or NaN, max_range not above 0, min_cos2 outside [0, 1].  T3D_ERR_SHAPE: n_scenes outside [1, 65535], H or W < 1,
 * H * W > 2^24, stride < 1, part_offsets_host not starting at 0 or decreasing, more than T3D_SCENE_MAX_PARTS parts or than
 * T3D_SCENE_MAX_OBJECTS objects (or fewer than 0) in a scene.  Nothing is launched then.  The *_host arrays are host memory holding what
 * the device arrays of the same name hold (they are read for these refusals and the grid alone). */
#define T3D_SCENE_MAX_PARTS 512
#define T3D_SCENE_MAX_OBJECTS 64
#define T3D_SCENE_BLOCK_PIXELS 1024      /* consecutive pixels (row-major) of one scene per workgroup */
#define T3D_SCENE_HIT_ROOM (-1)
#define T3D_SCENE_HIT_INVALID (-2)
#define T3D_SCENE_ROOM_COLOUR 200.0
#define T3D_SCENE_SHADES {0.70, 0.80, 0.60, 0.90, 0.50, 1.00}      /* faces -x +x -y +y -z +z */
#define T3D_SCENE_BLOCKS(H, W) (((uint64_t)(H) * (uint64_t)(W) + T3D_SCENE_BLOCK_PIXELS - 1u) / T3D_SCENE_BLOCK_PIXELS)
/* per workgroup an int64 offset and an int32 count (rounded up to 8 bytes together) */
#define T3D_SCENE_WORKSPACE_BYTES(S, H, W) ((uint64_t)(S) * T3D_SCENE_BLOCKS(H, W) * 16u)
typedef struct {
  double centre[3];
  double half[3];
  double cos_r, sin_r;
  double colour[3];
  int32_t owner;
  int32_t reserved;                    /* 0 */
} t3d_scene_part;

typedef struct {
  uint32_t struct_size;    /* = sizeof(t3d_scene_raycast_args) of the caller's header (see T3D_ABI_VERSION) */
  int n_scenes; int H; int W; int stride;
  uint32_t seed;
  int reserved;                        /* 0 */
  const double* rtilt;                 /* [S,9] */
  const double* K;                     /* [S,9] */
  const int32_t* scene_id;             /* [S] */
  const double* room;                  /* [S,6] */
  const int32_t* part_offsets;         /* [S+1] */
  const t3d_scene_part* parts;         /* [part_offsets[S]] (may be NULL when that is 0) */
  const double* room_host;             /* [S,6] host */
  const int32_t* part_offsets_host;    /* [S+1] host */
  const int32_t* n_objects_host;       /* [S] host */
  double noise_a; double p_drop; double max_range; double min_cos2;
  void* workspace;
  uint64_t workspace_bytes;
  int64_t points_capacity;             /* rows of `points` (and of point_pixel) */
  int32_t* hit;                        /* [S,H,W] out */
  uint8_t* image;                      /* [S,H,W,3] out */
  double* points;                      /* [points_capacity,6] out */
  int32_t* point_pixel;                /* [points_capacity] out, or NULL */
  int64_t* scene_offsets;              /* [S+1] out */
  int32_t* visible;                    /* [S,64] out */
  int32_t* vis_box;                    /* [S,64,4] out */
} t3d_scene_raycast_args;
#define T3D_V2_SIZE_scene_raycast_args 216
int t3d_scene_raycast(const t3d_scene_raycast_args* args, t3d_stream_t stream);

/* ---- The floor of a scene and how a detection stands on it (csrc/floor.hip; transferable3d_amd/floor.py, detect --floor) ----
 * t3d_scene_floor estimates, per scene of a batch, the floor plane Z = a X + b Y + c from the scene's depth points (upright depth
 * coordinates: X right, Y forward, Z up, the camera at the origin) where the extraction left them.  Everything is fp64, every product
 * and sum is an operation of its own (nothing is contracted), the histogram is summed by integer atomics and no floating-point atomic
 * exists: a scene's bytes are a function of its own points and the options, never of S or its place in the batch.
 *
 *   points [sum n_s, ld]   row-major, ld >= 3, columns 0..2 = X Y Z;  scene s is rows scene_offsets[s] .. scene_offsets[s+1]-1 (a negative
 *                          offset is taken as 0, an end before the start as the start; the offsets live on the device, so the caller
 *                          answers for their not exceeding the rows of `points`).
 *   A point counts         iff x, y and z are finite;  n_finite is their number.
 *   hist [S, n_bins]       t = (z - z_lo) * inv_bin;  a counting point is binned iff t >= 0 && t < n_bins, into (int)floor(t).
 *   c3[b]                  for 0 <= b < n_bins: hist[b-1] + hist[b] + hist[b+1], bins outside the histogram counting 0;  for every other
 *                          b: 0 (so bin 0 competes with c3[-1] = 0, not with the window hist[0] alone).
 *   The floor bin          the smallest b with (double)c3[b] >= min_share * (double)n_finite, c3[b] >= min_inliers, c3[b] > c3[j] for
 *                          j in [b-2, b) and c3[b] >= c3[j] for j in (b, b+2] (c3 outside the histogram: 0).  None: flag
 *                          T3D_FLOOR_NONE, the plane row is zeros, counts = (n_finite, 0, -1, T3D_FLOOR_NONE).
 *   z0                     z_lo + ((double)b + 0.5) * bin.  The inliers are the counting points with |z - z0| <= band;  n1 is their
 *                          number.  n1 == 0 (a band narrower than the bins): T3D_FLOOR_NONE as above, but counts[2] = b.
 *   Level pass             Sx, Sy, Sz over the inliers;  mx = Sx / (double)n1, my, mz alike.
 *   Moment pass            dx = x - mx, dy = y - my, dz = z - mz;  Sxx, Sxy, Syy, Sxz, Syz, Szz of the products dx * dx, ...
 *   Order of every sum     chunk k of a scene is its points 4096 k .. 4096 k + 4095.  In a chunk, lane t < 256 starts from 0.0 and adds
 *                          the terms of its inliers t, t + 256, ... in ascending order;  the lanes are combined by the halving tree
 *                          v[t] = v[t] + v[t+s] for t < s, s = 128 ... 1.  Workgroup j < T3D_SCENE_FLOOR_BLOCKS of the scene starts from
 *                          0.0 and adds v[0] of the chunks j, j + T3D_SCENE_FLOOR_BLOCKS, ... in ascending order (none: it stays 0.0);  the
 *                          sum is 0.0 plus the workgroups' sums in ascending j.  tests/fake_floor.py replicates it.
 *   Fit                    det = Sxx * Syy - Sxy * Sxy;  a = (Sxz * Syy - Syz * Sxy) / det;  b = (Syz * Sxx - Sxz * Sxy) / det.  Accepted
 *                          iff a and b are finite, a * a + b * b <= max_slope2, Sxx >= ((double)n1 * min_spread) * min_spread and Syy
 *                          alike, det >= min_det_ratio * (Sxx * Syy).  Otherwise a = b = 0 and flag T3D_FLOOR_LEVEL (a floor seen as a
 *                          strip, a wrongly tilted peak).  c = mz - (a * mx + b * my);  r = Szz - (a * Sxz + b * Syz);
 *                          msr = (r > 0 ? r : 0) / (double)n1 (the host takes the square root).
 *   plane [S, 8]           a, b, c, mx, my, mz, msr, z0.      counts [S, 4]   n_finite, n1, the floor bin or -1, flags.
 *   workspace              T3D_SCENE_FLOOR_WORKSPACE_BYTES(S) bytes, 8-byte aligned; its content means nothing before or after.
 * T3D_ERR_ARG: a NULL struct or pointer, S < 0, reserved != 0, n_bins < 1, bin or inv_bin not finite or not above 0, z_hi <= z_lo (or a
 * NaN), min_share outside [0, 1], band, max_slope2, min_spread or min_det_ratio negative or NaN, min_inliers < 0, a workspace that is
 * misaligned or too small.  T3D_ERR_SHAPE: n_bins > T3D_SCENE_FLOOR_MAX_BINS, ld < 3, S > 65535.  S == 0: T3D_OK without a launch.  Nothing is
 * launched after a refusal.  One clearing of hist and counts and five launches, no host synchronisation. */
#define T3D_SCENE_FLOOR_MAX_BINS 1024
#define T3D_SCENE_FLOOR_CHUNK 4096       /* consecutive points of a scene per step of a workgroup */
#define T3D_SCENE_FLOOR_BLOCKS 64        /* workgroups per scene */
#define T3D_SCENE_FLOOR_WORKSPACE_BYTES(S) ((uint64_t)(S) * T3D_SCENE_FLOOR_BLOCKS * 80u)
#define T3D_FLOOR_NONE 1
#define T3D_FLOOR_LEVEL 2
typedef struct {
  uint32_t struct_size;    /* = sizeof(t3d_scene_floor_args) of the caller's header (see T3D_ABI_VERSION) */
  int n_scenes; int ld; int n_bins;
  const double* points;                /* [sum n_s, ld] */
  const int64_t* scene_offsets;        /* [S+1] */
  double z_lo; double z_hi; double bin; double inv_bin; double min_share;
  int min_inliers;
  int reserved;                        /* 0 */
  double band; double max_slope2; double min_spread; double min_det_ratio;
  void* workspace;
  uint64_t workspace_bytes;
  double* plane;                       /* [S,8] out */
  int32_t* counts;                     /* [S,4] out */
  int32_t* hist;                       /* [S,n_bins] out */
} t3d_scene_floor_args;
#define T3D_V2_SIZE_scene_floor_args 152
int t3d_scene_floor(const t3d_scene_floor_args* args, t3d_stream_t stream);

/* t3d_detect_floor: how far the bottom of every decoded box lies from its scene's floor, and on request the box standing on it.  One
 * thread per detection, fp64 on the widened fp32 entries, nothing contracted; inputs are never written, equal inputs give equal bytes.
 *
 *   label [n,7]        h, w, l, tx, ty, tz, ry (t3d_detect_decode): ty is the bottom of the box, y points down.  The upright camera's
 *                      (x, y, z) is the depth frame's (X, -Z, Y).
 *   yf                 -((a * tx + b * tz) + c) of the plane row scene_index[i] names;  gap = yf - ty: positive, the box floats above the
 *                      floor; negative, it sinks into it.
 *   flags              T3D_DETECT_FLOOR_NO_FLOOR: scene_index outside [0, n_scenes) or the scene's T3D_FLOOR_NONE; NOT_FINITE: a label entry
 *                      that is not finite.  Either: gap is the NaN 0x7FF8000000000000 and no other flag is set.  Otherwise TOO_FAR:
 *                      |gap| > max_snap;  INVERTED (mode 2 only): h' below is not above 0;  SNAPPED: mode != 0 and no other flag.
 *   mode 0             measure.  label_out / corners_out may be NULL; where given they receive copies.
 *   mode 1 (shift)     a snapped row: ty' = (float)yf, h' = h.
 *   mode 2 (stretch)   a snapped row: ty' = (float)yf, h' = (float)(yf - ((double)ty - (double)h)): the top face stays.
 *   label_out          label with h', ty' in a snapped row;  corners_out [n,8,3]: corners with, in a snapped row, the y of corner k
 *                      rebuilt in fp32 as the decode does, (k < 4 ? h' : -h') / 2 + (ty' - h' / 2); x and z are copied.  A row that is
 *                      not snapped is a copy of its input, byte for byte.
 * T3D_ERR_ARG: a NULL struct, label, corners, scene_index, gap or flags, a NULL plane or counts where n_scenes > 0, n < 0, n_scenes < 0,
 * reserved != 0, a mode outside 0..2, a NULL label_out or corners_out in mode 1 or 2, max_snap negative or NaN.  n == 0: T3D_OK without
 * a launch. */
#define T3D_DETECT_FLOOR_NO_FLOOR 1
#define T3D_DETECT_FLOOR_NOT_FINITE 2
#define T3D_DETECT_FLOOR_TOO_FAR 4
#define T3D_DETECT_FLOOR_INVERTED 8
#define T3D_DETECT_FLOOR_SNAPPED 16
typedef struct {
  uint32_t struct_size;    /* = sizeof(t3d_detect_floor_args) of the caller's header (see T3D_ABI_VERSION) */
  int n; int n_scenes; int mode;
  const float* label;                  /* [n,7] */
  const float* corners;                /* [n,8,3] */
  const int32_t* scene_index;          /* [n]: the row of plane / counts, -1 for none */
  const double* plane;                 /* [n_scenes,8] what t3d_scene_floor wrote */
  const int32_t* counts;               /* [n_scenes,4] what t3d_scene_floor wrote */
  double max_snap;
  int reserved;                        /* 0 */
  double* gap;                         /* [n] out */
  int32_t* flags;                      /* [n] out */
  float* label_out;                    /* [n,7] out, or NULL (mode 0) */
  float* corners_out;                  /* [n,8,3] out, or NULL (mode 0) */
} t3d_detect_floor_args;
#define T3D_V2_SIZE_detect_floor_args 104
int t3d_detect_floor(const t3d_detect_floor_args* args, t3d_stream_t stream);

/* ---- The free space of a scene and how a detection stands in it (csrc/range.hip; transferable3d_amd/visibility.py, detect
 *      --visibility) ----
 * Every pixel of a depth image says that the space between the camera and its return is empty.  t3d_scene_range keeps that of each
 * scene of an extraction launch as a range map -- per cell of `cell` x `cell` pixels the smallest camera depth of the points that
 * project into it, as an fp32 -- from the scene's depth points (upright depth coordinates) where the extraction left them.  The map
 * holds fp32 values that are not negative, whose bit patterns order as unsigned integers: it is a minimum by integer atomics, and a
 * scene's bytes are a function of its own points, its calibration row and `cell`, never of S, of its place in the batch or of the
 * order of anything.  Everything is fp64, every product and sum an operation of its own (nothing is contracted).
 *
 *   points, scene_offsets  as t3d_scene_floor reads them.
 *   Scene s                its calibration is row calib_index[s] of `calib` (the 20 doubles t3d_detect_consistency reads: Rtilt (9), K
 *                          (9), image W, H; W and H are not read here);  its grid is gw = grid_dims[s][0] by gh = grid_dims[s][1] cells,
 *                          row-major (cell (cx, cy) at grid_offsets[s] + cy * gw + cx of `range`).  The caller chooses gw = ceil(W / cell)
 *                          and gh alike.  GW = (double)gw * (double)cell, GH alike.
 *   Scene flags            T3D_RANGE_NO_CALIB: calib_index[s] outside [0, n_calib).  T3D_RANGE_BAD_GRID: gw < 1, gh < 1, gw * gh >
 *                          T3D_RANGE_MAX_CELLS, grid_offsets[s] < 0 or grid_offsets[s] + gw * gh > n_cells.  With either no point of the
 *                          scene is binned and no cell of `range` is written for it.
 *   A point counts         iff x, y and z are finite;  n_finite is their number (whatever the flags).
 *   Projection             the paragraph "Projection" of t3d_detect_consistency with d = (x, y, z), the point:  t_i = (R[0][i]*d0 +
 *                          R[1][i]*d1) + R[2][i]*d2;  cam = (t0, -t2, t1);  w_i = (K[i][0]*cam0 + K[i][1]*cam1) + K[i][2]*cam2;  u = w0/w2,
 *                          v = w1/w2;  depth = cam2.
 *   A point is binned      iff it counts, depth > 0, the bit pattern of (float)depth lies below T3D_RANGE_EMPTY (the depth does not
 *                          round to infinity), u and v are finite, 0 <= u < GW and 0 <= v < GH.  cx = (int)floor(u / (double)cell),
 *                          taken as gw - 1 where the quotient rounds up to gw;  cy alike.  The cell becomes the smaller of what it
 *                          holds and the bit pattern of (float)depth.
 *   range [n_cells]        uint32;  every cell is T3D_RANGE_EMPTY (the bits of +infinity) before the points are binned, cells that belong
 *                          to no scene included.
 *   counts [S, 4]          n_finite, the points binned, the cells that hold a depth, the scene flags.
 * T3D_ERR_ARG: a NULL struct or pointer (`range` may be NULL where n_cells == 0), S < 0, cell < 1, n_calib < 0, n_cells < 0,
 * reserved != 0.  T3D_ERR_SHAPE: ld < 3, S > 65535, n_cells > 2^31 - 1.  S == 0: T3D_OK without a launch.  Nothing is launched after a
 * refusal.  Two launches (the fill, the points), no host synchronisation; the offsets and the grids live on the device, so the
 * caller answers for the rows of `points` as for t3d_scene_floor -- a grid that does not fit `range` is refused by its flag. */
#define T3D_RANGE_EMPTY 0x7F800000u
#define T3D_RANGE_BLOCKS 64              /* workgroups per scene */
#define T3D_RANGE_MAX_CELLS (1 << 24)    /* cells of one scene's grid */
#define T3D_RANGE_NO_CALIB 1
#define T3D_RANGE_BAD_GRID 2
typedef struct {
  uint32_t struct_size;    /* = sizeof(t3d_scene_range_args) of the caller's header (see T3D_ABI_VERSION) */
  int n_scenes; int ld; int cell; int n_calib;
  const double* points;                /* [sum n_s, ld] */
  const int64_t* scene_offsets;        /* [S+1] */
  const double* calib;                 /* [n_calib,20] */
  const int32_t* calib_index;          /* [S] */
  const int32_t* grid_dims;            /* [S,2]: gw, gh */
  const int64_t* grid_offsets;         /* [S+1] */
  int64_t n_cells;                     /* cells of `range` */
  int reserved;                        /* 0 */
  uint32_t* range;                     /* [n_cells] out */
  int32_t* counts;                     /* [S,4] out */
} t3d_scene_range_args;
#define T3D_V2_SIZE_scene_range_args 104
int t3d_scene_range(const t3d_scene_range_args* args, t3d_stream_t stream);

/* t3d_detect_visibility: every decoded box against the range map of its scene.  A box pulled towards the camera has the surface behind
 * it seen THROUGH it, a box pushed away has every return IN FRONT of it, a box in mid-air is seen through entirely.  One workgroup of
 * 256 threads per detection; fp64 on the widened fp32 entries, nothing contracted, each product and sum in the order written; the
 * counts are integers, so no order of lanes matters; inputs are never written, equal inputs give equal bytes.
 *
 *   label [n,7], corners [n,8,3]   as t3d_detect_decode wrote them (upright camera coordinates; tx = label[3], tz = label[5]).
 *   Scene                  s = scene_index[i] names row s of `calib` (20 doubles as above), of grid_dims and of grid_offsets.  Flag
 *                          T3D_VIS_NO_SCENE: s outside [0, n_scenes) or a grid that t3d_scene_range would flag T3D_RANGE_BAD_GRID.
 *                          T3D_VIS_NOT_FINITE: an entry of the label or the corners that is not finite.  With either nothing is
 *                          measured: the profile and the measures are 0, choice is (K - 1) / 2, the row is copied.
 *   Candidate k < K        offsets[k] is a relative depth offset: K odd, 1 <= K <= T3D_VIS_MAX_OFFSETS, ascending, all above -1,
 *                          offsets[(K-1)/2] == 0.  Corner c of candidate k is (X, Y, Z) = ((double)x_c + offsets[k] * (double)tx,
 *                          (double)y_c, (double)z_c + offsets[k] * (double)tz): a slide along the horizontal viewing ray by a fraction
 *                          of the distance -- no square root, every decision stays in + - * /.  mid = (K - 1) / 2 is the box itself.
 *   Rectangle              the eight corners are projected as "Projection" of t3d_detect_consistency states (d = (X, Z, -Y)).  A
 *                          candidate is MEASURED iff every corner has depth > 0 and finite u and v; one that is not has a profile of
 *                          zeros and cannot be chosen.  xmin = u of corner 0, then for corners 0..7 in order xmin = u < xmin ? u : xmin;
 *                          xmax, ymin, ymax likewise.  No cell where xmax < 0, xmin >= GW, ymax < 0 or ymin >= GH.  Otherwise the cells
 *                          cx0 .. cx1 by cy0 .. cy1:  cx0 = xmin < 0 ? 0 : (int)floor(xmin / (double)cell) (gw - 1 where the quotient
 *                          rounds up to gw),  cx1 = xmax >= GW ? gw - 1 : (int)floor(xmax / (double)cell);  cy0, cy1 alike.
 *   Ray of cell (cx, cy)   pu = ((double)cx + 0.5) * (double)cell, pv alike;  as t3d_scene_raycast inverts the projection:
 *                          rx = (pu - K[0][2]) / K[0][0];  ry = (pv - K[1][2]) / K[1][1];  q = (rx, 1, -ry);
 *                          d_i = (R[i][0]*q0 + R[i][1]*q1) + R[i][2]*q2;  in upright camera coordinates g = (d0, -d2, d1).  The point t * g
 *                          has camera depth t.
 *   Intersection           with the parallelepiped at corner 0 (K0) with the edges e to corners 1, 3 and 4, in this order.  Per edge:
 *                          a = (g0*e0 + g1*e1) + g2*e2;  b = (K0x*e0 + K0y*e1) + K0z*e2;  dd = (e0*e0 + e1*e1) + e2*e2.
 *                          a == 0: a miss unless 0 <= -b && -b <= dd, no constraint otherwise.  Else r0 = b / a, r1 = (dd + b) / a,
 *                          lo = r0 < r1 ? r0 : r1, hi = r0 < r1 ? r1 : r0;  t_in = lo > t_in ? lo : t_in (from 0);  t_out = hi < t_out ?
 *                          hi : t_out (from +infinity).  A hit iff no edge misses and t_in < t_out.
 *   Category of a hit      t_out - t_in < min_chord: GRAZE.  Otherwise a RAY; with z the cell's depth widened: UNKNOWN where the cell is
 *                          T3D_RANGE_EMPTY, else FRONT where z < t_in - margin, else THROUGH where z > t_out + margin, else INSIDE.
 *   profile [n,K,6]        rays, unknown, front, inside, through, graze of every candidate (rays = unknown + front + inside + through).
 *   measures [n,3]         of candidate mid:  see_through = (double)through / (double)(through + inside);  occluded = (double)front /
 *                          (double)rays;  support = (double)inside / (double)rays;  0 where the denominator is 0.
 *   flags                  also T3D_VIS_BEHIND: candidate mid is not measured (the measures are 0);  where none of these three is set,
 *                          T3D_VIS_NO_RAYS: rays of mid == 0;  T3D_VIS_NO_EVIDENCE: through + inside of mid == 0.
 *   choice [n]             score_k = inside_k - through_k.  Over the measured candidates the largest score; among equal scores the
 *                          smaller |k - mid|, then the lower k.  mid where mid is not measured.
 *   mode 0                 measure.  label_out / corners_out may be NULL; where given they receive copies.
 *   mode 1 (snap)          the box moves iff none of NO_SCENE, NOT_FINITE, BEHIND is set, choice != mid and score_choice - score_mid >=
 *                          min_gain: flag T3D_VIS_SNAPPED.  label_out of a moved row: tx' = (float)((double)tx + offsets[choice] *
 *                          (double)tx), tz' alike with tz;  corners_out: every x' = (float)((double)x + offsets[choice] * (double)tx),
 *                          every z' alike with tz;  everything else, and every row that did not move, is a copy byte for byte.
 * T3D_ERR_ARG: a NULL struct, label, corners, scene_index, profile, measures, choice or flags, a NULL calib, grid_dims or grid_offsets
 * where n_scenes > 0, a NULL range where n_cells > 0, n < 0, n_scenes < 0, n_cells < 0, reserved != 0, a mode outside 0..1, a NULL
 * label_out or corners_out in mode 1, cell < 1, min_gain < 0, margin or min_chord negative, NaN or infinite, offsets that are not
 * ascending, not above -1 or not 0 at mid.  T3D_ERR_SHAPE: K even or outside [1, T3D_VIS_MAX_OFFSETS].  n == 0: T3D_OK without a launch. */
#define T3D_VIS_MAX_OFFSETS 17
#define T3D_VIS_NO_SCENE 1
#define T3D_VIS_NOT_FINITE 2
#define T3D_VIS_BEHIND 4
#define T3D_VIS_NO_RAYS 8
#define T3D_VIS_NO_EVIDENCE 16
#define T3D_VIS_SNAPPED 32
typedef struct {
  uint32_t struct_size;    /* = sizeof(t3d_detect_visibility_args) of the caller's header (see T3D_ABI_VERSION) */
  int n; int n_scenes; int mode; int K; int cell; int min_gain;
  int reserved;                        /* 0 */
  const float* label;                  /* [n,7] */
  const float* corners;                /* [n,8,3] */
  const int32_t* scene_index;          /* [n]: the scene's row, -1 for none */
  const double* calib;                 /* [n_scenes,20] */
  const int32_t* grid_dims;            /* [n_scenes,2] */
  const int64_t* grid_offsets;         /* [n_scenes+1] */
  const uint32_t* range;               /* [n_cells] what t3d_scene_range wrote */
  int64_t n_cells;
  double margin; double min_chord;
  double offsets[T3D_VIS_MAX_OFFSETS]; /* the first K are read */
  int32_t* profile;                    /* [n,K,6] out */
  double* measures;                    /* [n,3] out */
  int32_t* choice;                     /* [n] out */
  int32_t* flags;                      /* [n] out */
  float* label_out;                    /* [n,7] out, or NULL (mode 0) */
  float* corners_out;                  /* [n,8,3] out, or NULL (mode 0) */
} t3d_detect_visibility_args;
#define T3D_V2_SIZE_detect_visibility_args 296
int t3d_detect_visibility(const t3d_detect_visibility_args* args, t3d_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* T3D_H_ */
