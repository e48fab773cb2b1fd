// Rescoring (t3d.h t3d_rescore_features / t3d_rescore_fit / t3d_rescore_apply): a logistic model from the label-free measures of a
// detection to "this box is right", fitted and applied on the device next to the buffers it reads.
//   k_rescore_features  one thread per detection: the selected features, in table order, from the stage buffers where they lie;
//   k_rescore_moments   one workgroup per slice of T3D_RESCORE_SLICE rows: weighted sums, then squared deviations from the slice's own
//                       mean, minimum, maximum, row counts; lane (row group, column), so that a wave reads four whole rows at a time;
//   k_rescore_stats     one wave: the slices merged in slice order (Chan's pairwise update), mean and scale, the status bits, the start;
//   k_rescore_eval      one workgroup per slice, at the trial point: first a thread per row -- z, the loss term, r p (1-p) and r (p - y)
//                       into LDS --, then the slice's Gram matrix by v_mfma_f64_16x16x4_f64: a lane loads X[row][column] once, and
//                       that one value, standardised, is its B operand and, times r p (1-p), its A operand; the gradient rides along
//                       as one multiply-add per lane.  The four waves' results are added in wave order;
//   k_rescore_step      one workgroup: the slices' sums in slice order, accept or halve, the convergence test, Cholesky and the two
//                       triangular solves in LDS (a thread per matrix entry), the next trial point, the outputs.
// Every sum has one order fixed by n alone; there is no atomic.  Once the fit has ended k_rescore_eval and k_rescore_step return at
// their first instruction, so the host enqueues a fixed number of them and never reads back.
#include "common.h"

// t3d_rescore_features and t3d_rescore_apply are specified operation by operation (NumPy, elementwise, fp64)
#pragma clang fp contract(off)

namespace {

constexpr int RS_THREADS = 256, RS_SLICE = T3D_RESCORE_SLICE, RS_D = 16;
constexpr int RS_STATE = 128, RS_STAT = 80, RS_EVAL = 288;      // doubles: T3D_RESCORE_FIT_WORKSPACE_BYTES
static_assert(RS_D == T3D_RESCORE_MAX_FEATURES + 1 && RS_SLICE % RS_THREADS == 0, "one lane per (row group, column)");
// the state, in doubles: trial point, accepted point, step (each w then b at index F), mean and 1 / scale per column, the accepted
// loss, W; behind them four ints
enum { ST_W = 0, ST_WACC = 16, ST_STEP = 32, ST_MEAN = 48, ST_INV = 64, ST_LOSS = 80, ST_WSUM = 81, ST_INTS = 96 };
enum { SI_DONE = 0, SI_HALVINGS = 1, SI_ACCEPTED = 2, SI_STATUS = 3 };
// a slice's statistics: mean [16], squared deviations [16], min [16], max [16], W, Wy, rows, positives, non-finite
enum { SS_MEAN = 0, SS_M2 = 16, SS_MIN = 32, SS_MAX = 48, SS_W = 64, SS_WY = 65, SS_ROWS = 66, SS_POS = 67, SS_BAD = 68 };
// a slice's evaluation: Hessian [16][16], gradient [16], loss
enum { SE_H = 0, SE_G = 256, SE_LOSS = 272 };

typedef double f64x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ double* rs_state(void* ws) { return static_cast<double*>(ws); }
__device__ __forceinline__ int* rs_ints(void* ws) { return reinterpret_cast<int*>(static_cast<double*>(ws) + ST_INTS); }
__device__ __forceinline__ double* rs_stat(void* ws, int s) { return static_cast<double*>(ws) + RS_STATE + (size_t)s * RS_STAT; }
__device__ __forceinline__ double* rs_eval(void* ws, int S, int s) {
  return static_cast<double*>(ws) + RS_STATE + (size_t)S * RS_STAT + (size_t)s * RS_EVAL;
}
__host__ __device__ __forceinline__ bool rs_finite(double v) { return v - v == 0.0; }

__global__ __launch_bounds__(RS_THREADS) void k_rescore_features(const t3d_rescore_features_args p) {
  const int i = blockIdx.x * RS_THREADS + threadIdx.x;
  if (i >= p.n) return;
  double* x = p.X + (size_t)i * p.ld;
  const uint32_t m = p.feature_mask;
  int k = 0;
  if (m & T3D_RESCORE_F_LOGIT_PROB) {
    double q = (double)p.prob[i];
    q = q < 1e-6 ? 1e-6 : q;
    q = q > 1.0 - 1e-6 ? 1.0 - 1e-6 : q;
    x[k++] = log(q / (1.0 - q));
  }
  if (m & T3D_RESCORE_F_SCORE) x[k++] = (double)p.score[i];
  if (m & T3D_RESCORE_F_REPROJ_IOU) x[k++] = p.reproj[(size_t)i * 5 + 4];
  if (m & (T3D_RESCORE_F_MASK_IN_BOX | T3D_RESCORE_F_SEG_BOX_IOU | T3D_RESCORE_F_LOG_MASK)) {
    const int32_t* c = p.counts + (size_t)i * 4;
    const long long n_mask = c[0], n_box = c[1], n_both = c[2];
    const long long u = n_mask + n_box - n_both;
    if (m & T3D_RESCORE_F_MASK_IN_BOX) x[k++] = n_mask > 0 ? (double)n_both / (double)n_mask : 0.0;
    if (m & T3D_RESCORE_F_SEG_BOX_IOU) x[k++] = u > 0 ? (double)n_both / (double)u : 0.0;
    if (m & T3D_RESCORE_F_LOG_MASK) x[k++] = log1p((double)n_mask);
  }
  if (m & T3D_RESCORE_F_VIEW_IOU) x[k++] = (double)p.view_iou[i];
}

__global__ __launch_bounds__(RS_THREADS) void k_rescore_apply(const t3d_rescore_apply_args p) {
  const int i = blockIdx.x * RS_THREADS + threadIdx.x;
  if (i >= p.n_valid) return;
  const double* x = p.X + (size_t)i * p.ld;
  double z = p.coef[p.F];
  for (int j = 0; j < p.F; ++j) z = z + p.coef[j] * x[j];
  const double v = 1.0 / (1.0 + exp(-z));
  p.out[i] = v;
  if (p.out32) p.out32[i] = (float)v;
}

// column c's fold over the 16 row groups, in group order; every thread gets it
__device__ __forceinline__ double rs_fold_sum(double (*sh)[RS_D], int g, int c, double v) {
  __syncthreads();
  sh[g][c] = v;
  __syncthreads();
  double a = sh[0][c];
  for (int k = 1; k < 16; ++k) a += sh[k][c];
  return a;
}
__device__ __forceinline__ double rs_fold_min(double (*sh)[RS_D], int g, int c, double v, double sign) {
  __syncthreads();
  sh[g][c] = v;
  __syncthreads();
  double a = sh[0][c];
  for (int k = 1; k < 16; ++k) a = sign > 0.0 ? fmin(a, sh[k][c]) : fmax(a, sh[k][c]);
  return a;
}

__global__ __launch_bounds__(RS_THREADS) void k_rescore_moments(const t3d_rescore_fit_args p) {
  __shared__ double sh[16][RS_D];
  const int t = threadIdx.x, c = t & 15, g = t >> 4;      // row group g = 4 * wave + lane / 16: a wave reads four consecutive rows
  const int row0 = blockIdx.x * RS_SLICE;
  const int rows = min(RS_SLICE, p.n - row0);
  const bool col = c < p.F;
  const double inf = __longlong_as_double(0x7ff0000000000000LL);
  double sum = 0.0, w = 0.0, wy = 0.0, cnt = 0.0, pos = 0.0, mn = inf, mx = -inf, bad = 0.0;
  for (int i = g; i < rows; i += 16) {
    const size_t row = (size_t)row0 + i;
    const double rr = p.r[row];
    if (!(rr > 0.0)) continue;
    const double yy = p.y[row] != 0 ? 1.0 : 0.0;
    if (!rs_finite(rr)) bad = 1.0;
    w += rr; wy += rr * yy; cnt += 1.0; pos += yy;
    if (col) {
      const double x = p.X[row * p.ld + c];
      if (!rs_finite(x)) bad = 1.0;
      sum += rr * x;
      mn = fmin(mn, x);
      mx = fmax(mx, x);
    }
  }
  const double W = rs_fold_sum(sh, g, c, w), Sum = rs_fold_sum(sh, g, c, sum);
  const double mean = W > 0.0 ? Sum / W : 0.0;
  double m2 = 0.0;
  if (col) {
    for (int i = g; i < rows; i += 16) {
      const size_t row = (size_t)row0 + i;
      const double rr = p.r[row];
      if (!(rr > 0.0)) continue;
      const double d = p.X[row * p.ld + c] - mean;
      m2 += rr * (d * d);
    }
  }
  const double M2 = rs_fold_sum(sh, g, c, m2), Wy = rs_fold_sum(sh, g, c, wy), Rows = rs_fold_sum(sh, g, c, cnt);
  const double Pos = rs_fold_sum(sh, g, c, pos);
  const double Bad = __syncthreads_or(bad != 0.0) ? 1.0 : 0.0;      // of any column (the other sums are the same in every column)
  const double Mn = rs_fold_min(sh, g, c, mn, 1.0), Mx = rs_fold_min(sh, g, c, mx, -1.0);
  double* st = rs_stat(p.workspace, blockIdx.x);
  if (g == 0) {
    st[SS_MEAN + c] = mean; st[SS_M2 + c] = M2; st[SS_MIN + c] = Mn; st[SS_MAX + c] = Mx;
    if (c == 0) { st[SS_W] = W; st[SS_WY] = Wy; st[SS_ROWS] = Rows; st[SS_POS] = Pos; st[SS_BAD] = Bad; }
  }
}

// one wave; lane c < 16 owns column c (the lanes behind run along and write nothing)
__global__ __launch_bounds__(64) void k_rescore_stats(const t3d_rescore_fit_args p, int S, int max_iter) {
  const int c = threadIdx.x, F = p.F;
  const bool col = c < F;
  const double inf = __longlong_as_double(0x7ff0000000000000LL), nan = __longlong_as_double(0x7ff8000000000000LL);
  double W = 0.0, mean = 0.0, M2 = 0.0, mn = inf, mx = -inf, Wy = 0.0, cnt = 0.0, pos = 0.0, bad = 0.0;
  for (int s = 0; s < S; ++s) {
    const double* st = rs_stat(p.workspace, s);
    const double Ws = st[SS_W];
    Wy += st[SS_WY]; cnt += st[SS_ROWS]; pos += st[SS_POS]; bad += st[SS_BAD];
    if (!(Ws > 0.0)) continue;
    if (col) {                                      // Chan, Golub, LeVeque: two sets of rows merged
      const double Wn = W + Ws, delta = st[SS_MEAN + c] - mean;
      mean = mean + delta * (Ws / Wn);
      M2 = M2 + st[SS_M2 + c] + delta * delta * (W * Ws / Wn);
      mn = fmin(mn, st[SS_MIN + c]);
      mx = fmax(mx, st[SS_MAX + c]);
    }
    W += Ws;
  }
  const bool nonfinite = bad > 0.0, no_rows = !nonfinite && !(W > 0.0), one_class = !nonfinite && !no_rows && (pos == 0.0 || pos == cnt);
  double scale = 1.0;
  bool constant = false;
  if (col && !no_rows) {
    const double sd = sqrt(M2 / W);
    constant = mn == mx || !(sd > 0.0);
    if (mn == mx) mean = mn;
    scale = constant ? 1.0 : sd;
  }
  if (no_rows) mean = 0.0;
  const bool any_constant = __ballot(constant && !nonfinite) != 0ull;
  double b0 = 0.0;
  if (one_class) {
    const double q = (Wy + 0.5) / (W + 1.0);
    b0 = log(q / (1.0 - q));
  } else if (!nonfinite && !no_rows) {
    b0 = log(Wy / (W - Wy));
  }
  const bool done = nonfinite || no_rows || one_class;
  const uint32_t status = (nonfinite ? T3D_RESCORE_NONFINITE : 0u) | (no_rows ? T3D_RESCORE_NO_ROWS : 0u) | (one_class ? T3D_RESCORE_ONE_CLASS : 0u) |
                          (any_constant ? T3D_RESCORE_CONSTANT_COLUMN : 0u) | (done ? 0u : T3D_RESCORE_NOT_CONVERGED);
  double* st = rs_state(p.workspace);
  if (c < RS_D) {
    const double w0 = c == F ? b0 : 0.0;
    st[ST_W + c] = w0; st[ST_WACC + c] = w0; st[ST_STEP + c] = 0.0;
    st[ST_MEAN + c] = col ? mean : 0.0;
    st[ST_INV + c] = col ? 1.0 / scale : 0.0;
    if (col) { p.mean[c] = mean; p.scale[c] = scale; }
    if (c <= F) { p.coef_std[c] = w0; p.coef[c] = w0; }
  }
  if (c == 0) {
    st[ST_LOSS] = 0.0; st[ST_WSUM] = W;
    int* si = rs_ints(p.workspace);
    si[SI_DONE] = done ? 1 : 0; si[SI_HALVINGS] = 0; si[SI_ACCEPTED] = 0; si[SI_STATUS] = (int)status;
    *p.n_iter = 0; *p.status = status; *p.n_rows = (int64_t)cnt; *p.n_pos = (int64_t)pos;
  }
  for (int k = c; k < max_iter; k += 64) p.loss[k] = nan;
}

__global__ __launch_bounds__(RS_THREADS) void k_rescore_eval(const t3d_rescore_fit_args p, int S) {
  if (rs_ints(p.workspace)[SI_DONE]) return;
  __shared__ double sS[RS_SLICE], sD[RS_SLICE];      // r p (1-p) and r (p - y) per row of the slice; 0 for a row that takes no part
  __shared__ double shH[RS_THREADS / 64][RS_D * RS_D];
  __shared__ double shG[16][RS_D];
  __shared__ double shL[RS_THREADS];
  const double* st = rs_state(p.workspace);
  const int t = threadIdx.x, F = p.F;
  const size_t ld = (size_t)p.ld;
  const int row0 = blockIdx.x * RS_SLICE;
  const int rows = min(RS_SLICE, p.n - row0);
  double loss = 0.0;
  for (int i = t; i < RS_SLICE; i += RS_THREADS) {
    double s = 0.0, d = 0.0;
    if (i < rows) {
      const size_t row = (size_t)row0 + i;
      const double rr = p.r[row];
      if (rr > 0.0) {
        const double* x = p.X + row * ld;
        double z = st[ST_W + F];
        for (int j = 0; j < F; ++j) z += st[ST_W + j] * ((x[j] - st[ST_MEAN + j]) * st[ST_INV + j]);
        const double yy = p.y[row] != 0 ? 1.0 : 0.0;
        const double e = exp(-fabs(z)), q = 1.0 / (1.0 + e);
        const double pr = z >= 0.0 ? q : e * q;      // the sigmoid, and p (1 - p) = e q^2, without cancellation at either end
        loss += rr * (fmax(z, 0.0) - yy * z + log1p(e));
        s = rr * (e * q * q);
        d = rr * (pr - yy);
      }
    }
    sS[i] = s;
    sD[i] = d;
  }
  shL[t] = loss;
  __syncthreads();
  for (int o = RS_THREADS / 2; o > 0; o >>= 1) {      // a fixed tree
    if (t < o) shL[t] += shL[t + o];
    __syncthreads();
  }
  // the Gram matrix: per MFMA a wave takes four rows; lane (k, c) holds row k's column c
  const int lane = t & 63, wv = t >> 6, c = lane & 15, k = lane >> 4;
  const double mean = c < F ? st[ST_MEAN + c] : 0.0, inv = c < F ? st[ST_INV + c] : 0.0;
  f64x4 acc = {0.0, 0.0, 0.0, 0.0};
  double gacc = 0.0;
  const int steps = (rows + 15) >> 4;
  for (int m = 0; m < steps; ++m) {
    const int i = m * 16 + wv * 4 + k;                // < RS_SLICE
    const double s = sS[i], d = sD[i];
    double xs = 0.0;                                  // a row that takes no part is a row of zeros, whatever it holds
    if (s != 0.0 || d != 0.0) xs = c < F ? (p.X[((size_t)row0 + i) * ld + c] - mean) * inv : (c == F ? 1.0 : 0.0);
    acc = __builtin_amdgcn_mfma_f64_16x16x4f64(s * xs, xs, acc, 0, 0, 0);
    gacc += d * xs;
  }
#pragma unroll
  for (int v = 0; v < 4; ++v) shH[wv][(k + 4 * v) * RS_D + c] = acc[v];      // C/D: row = lane / 16 + 4 v, column = lane % 16
  shG[wv * 4 + k][c] = gacc;
  __syncthreads();
  double* out = rs_eval(p.workspace, S, blockIdx.x);
  out[SE_H + t] = ((shH[0][t] + shH[1][t]) + shH[2][t]) + shH[3][t];
  if (t < RS_D) {
    double a = shG[0][t];
    for (int q = 1; q < 16; ++q) a += shG[q][t];
    out[SE_G + t] = a;
  }
  if (t == 0) out[SE_LOSS] = shL[0];
}

__global__ __launch_bounds__(RS_THREADS) void k_rescore_step(const t3d_rescore_fit_args p, int S, double gtol) {
  int* si = rs_ints(p.workspace);
  if (si[SI_DONE]) return;
  __shared__ double A[RS_D][RS_D + 1];
  __shared__ double gr[RS_D], dl[RS_D];
  __shared__ double Lsum;
  __shared__ int mode, fail;      // mode 0: halve; 1: accepted and converged; 2: accepted, a Newton step follows; 3: give up
  double* st = rs_state(p.workspace);
  const int t = threadIdx.x, F = p.F, D = F + 1, i = t >> 4, j = t & 15;
  double h = 0.0;
  for (int s = 0; s < S; ++s) h += rs_eval(p.workspace, S, s)[SE_H + t];
  A[i][j] = h;
  if (t < RS_D) {
    double g = 0.0;
    for (int s = 0; s < S; ++s) g += rs_eval(p.workspace, S, s)[SE_G + t];
    gr[t] = g;
  }
  if (t == RS_D) {
    double l = 0.0;
    for (int s = 0; s < S; ++s) l += rs_eval(p.workspace, S, s)[SE_LOSS];
    Lsum = l;
  }
  __syncthreads();
  const double invW = 1.0 / st[ST_WSUM], lam = p.lambda;
  if (t == 0) {
    double pen = 0.0;
    for (int q = 0; q < F; ++q) pen += st[ST_W + q] * st[ST_W + q];
    const double J = Lsum * invW + 0.5 * lam * pen;
    const int nacc = si[SI_ACCEPTED];
    fail = 0;
    if (nacc == 0 ? J == J : J <= st[ST_LOSS]) {
      st[ST_LOSS] = J;
      p.loss[nacc] = J;                               // nacc < max_iter: a launch accepts once at most
      si[SI_ACCEPTED] = nacc + 1;
      si[SI_HALVINGS] = 0;
      mode = 2;
    } else if (nacc == 0) {
      mode = 3;
    } else {
      const int halvings = si[SI_HALVINGS] + 1;
      si[SI_HALVINGS] = halvings;
      mode = halvings > T3D_RESCORE_MAX_HALVINGS ? 3 : 0;
    }
  }
  __syncthreads();
  if (mode == 2) {
    A[i][j] = A[i][j] * invW + ((i == j && i < F) ? lam : 0.0);
    if (t < RS_D) gr[t] = t < D ? gr[t] * invW + (t < F ? lam * st[ST_W + t] : 0.0) : 0.0;
    __syncthreads();
    if (t == 0) {
      bool small = true;
      for (int q = 0; q < D; ++q) small = small && fabs(gr[q]) <= gtol;      // (a NaN is not small)
      if (small) mode = 1;
    }
    __syncthreads();
  }
  if (mode == 2) {                                    // A = L L^T in place (the lower triangle), then L y = -g and L^T x = y
    for (int q = 0; q < D; ++q) {
      if (t == 0) {
        const double piv = A[q][q];
        if (!(piv > 0.0)) fail = 1;
        A[q][q] = sqrt(piv);
      }
      __syncthreads();
      if (t > q && t < D) A[t][q] = A[t][q] / A[q][q];
      __syncthreads();
      if (i > q && i < D && j > q && j <= i) A[i][j] -= A[i][q] * A[j][q];
      __syncthreads();
    }
    if (t < RS_D) dl[t] = t < D ? -gr[t] : 0.0;
    __syncthreads();
    for (int q = 0; q < D; ++q) {
      if (t == 0) dl[q] = dl[q] / A[q][q];
      __syncthreads();
      if (t > q && t < D) dl[t] -= A[t][q] * dl[q];
      __syncthreads();
    }
    for (int q = D - 1; q >= 0; --q) {
      if (t == 0) dl[q] = dl[q] / A[q][q];
      __syncthreads();
      if (t < q) dl[t] -= A[q][t] * dl[q];
      __syncthreads();
    }
  }
  const int md = mode;
  const bool accepted = md == 1 || md == 2, newton = md == 2 && fail == 0;
  if (accepted) {                                     // the outputs: the point just accepted
    if (t < D) p.coef_std[t] = st[ST_W + t];
    if (t < F) p.coef[t] = st[ST_W + t] * st[ST_INV + t];
    if (t == F) {
      double b = st[ST_W + F];
      for (int q = 0; q < F; ++q) b = b - (st[ST_W + q] * st[ST_INV + q]) * st[ST_MEAN + q];
      p.coef[F] = b;
    }
  }
  __syncthreads();
  if (t < RS_D) {
    if (accepted) st[ST_WACC + t] = st[ST_W + t];
    if (newton) {
      st[ST_STEP + t] = dl[t];
      st[ST_W + t] = st[ST_W + t] + dl[t];
    } else if (md == 0) {
      const double step = 0.5 * st[ST_STEP + t];
      st[ST_STEP + t] = step;
      st[ST_W + t] = st[ST_WACC + t] + step;
    }
  }
  if (t == 0) {
    uint32_t status = (uint32_t)si[SI_STATUS];
    if (md == 1) status &= ~T3D_RESCORE_NOT_CONVERGED;
    if (md == 1 || md == 3 || (md == 2 && fail != 0)) si[SI_DONE] = 1;
    si[SI_STATUS] = (int)status;
    *p.status = status;
    *p.n_iter = si[SI_ACCEPTED];
  }
}

inline int rs_popcount(uint32_t m) { int n = 0; for (; m; m &= m - 1) ++n; return n; }

}  // namespace

extern "C" int t3d_rescore_features(const t3d_rescore_features_args* a, t3d_stream_t stream) {
  T3D_ABI_TAKE(rescore_features_args, a);
  if (!a || !a->X) return T3D_ERR_ARG;
  const uint32_t m = a->feature_mask;
  if (m == 0u || (m >> T3D_RESCORE_N_FEATURES) != 0u) return T3D_ERR_ARG;
  if (a->n < 0 || a->ld < rs_popcount(m)) return T3D_ERR_SHAPE;
  if ((m & T3D_RESCORE_F_LOGIT_PROB) && !a->prob) return T3D_ERR_ARG;
  if ((m & T3D_RESCORE_F_SCORE) && !a->score) return T3D_ERR_ARG;
  if ((m & T3D_RESCORE_F_REPROJ_IOU) && !a->reproj) return T3D_ERR_ARG;
  if ((m & (T3D_RESCORE_F_MASK_IN_BOX | T3D_RESCORE_F_SEG_BOX_IOU | T3D_RESCORE_F_LOG_MASK)) && !a->counts) return T3D_ERR_ARG;
  if ((m & T3D_RESCORE_F_VIEW_IOU) && !a->view_iou) return T3D_ERR_ARG;
  if (a->n == 0) return T3D_OK;
  T3D_LAUNCH(k_rescore_features, dim3((a->n + RS_THREADS - 1) / RS_THREADS), dim3(RS_THREADS), 0, static_cast<hipStream_t>(stream), *a);
  T3D_CHECK_LAUNCH();
  return T3D_OK;
}

extern "C" int t3d_rescore_fit(const t3d_rescore_fit_args* a, t3d_stream_t stream) {
  T3D_ABI_TAKE(rescore_fit_args, a);
  if (!a || a->reserved != 0) return T3D_ERR_ARG;
  if (a->n < 0 || a->F < 1 || a->F > T3D_RESCORE_MAX_FEATURES || a->ld < a->F) return T3D_ERR_SHAPE;
  if (!(a->lambda > 0.0) || !rs_finite(a->lambda) || !(a->gtol >= 0.0) || a->max_iter < 0 || a->max_iter > 1000) return T3D_ERR_ARG;
  if (!a->coef || !a->coef_std || !a->mean || !a->scale || !a->loss || !a->n_iter || !a->status || !a->n_rows || !a->n_pos) return T3D_ERR_ARG;
  if (a->n > 0 && (!a->X || !a->y || !a->r)) return T3D_ERR_ARG;
  if (!a->workspace || (reinterpret_cast<uintptr_t>(a->workspace) & 7u) || a->workspace_bytes < T3D_RESCORE_FIT_WORKSPACE_BYTES(a->n)) return T3D_ERR_ARG;
  const int S = (int)T3D_RESCORE_SLICES(a->n), max_iter = a->max_iter ? a->max_iter : 30;
  const double gtol = a->gtol > 0.0 ? a->gtol : 1e-9;
  const hipStream_t st = static_cast<hipStream_t>(stream);
  if (S > 0) {
    T3D_LAUNCH(k_rescore_moments, dim3(S), dim3(RS_THREADS), 0, st, *a);
    T3D_CHECK_LAUNCH();
  }
  T3D_LAUNCH(k_rescore_stats, dim3(1), dim3(64), 0, st, *a, S, max_iter);
  T3D_CHECK_LAUNCH();
  for (int it = 0; S > 0 && it < max_iter; ++it) {
    T3D_LAUNCH(k_rescore_eval, dim3(S), dim3(RS_THREADS), 0, st, *a, S);
    T3D_CHECK_LAUNCH();
    T3D_LAUNCH(k_rescore_step, dim3(1), dim3(RS_THREADS), 0, st, *a, S, gtol);
    T3D_CHECK_LAUNCH();
  }
  return T3D_OK;
}

extern "C" int t3d_rescore_apply(const t3d_rescore_apply_args* a, t3d_stream_t stream) {
  T3D_ABI_TAKE(rescore_apply_args, a);
  if (!a || a->reserved != 0 || !a->X || !a->coef || !a->out) return T3D_ERR_ARG;
  if (a->n < 0 || a->n_valid < 0 || a->n_valid > a->n || a->F < 1 || a->F > T3D_RESCORE_MAX_FEATURES || a->ld < a->F) return T3D_ERR_SHAPE;
  if (a->n_valid == 0) return T3D_OK;
  T3D_LAUNCH(k_rescore_apply, dim3((a->n_valid + RS_THREADS - 1) / RS_THREADS), dim3(RS_THREADS), 0, static_cast<hipStream_t>(stream), *a);
  T3D_CHECK_LAUNCH();
  return T3D_OK;
}
