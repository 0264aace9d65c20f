// ML-utility evaluator (eval/utility_device.py DeviceUtility): a class-balanced, L2-regularised multinomial logistic
// regression fitted on a decoded table by a fixed number of bound-preconditioned accelerated gradient steps, and its
// confusion matrix on held-out rows, on the device.  Features F = [standardised continuous | one-hot(codes) | 1]; the
// one-hot blocks never exist in memory.
//
//  util_pack_kernel      one pass over the row-major table: (v - mean) / sd into a dense [n, n_cont] buffer, feature
//                        codes into int32 [n_cat, ld] rows (overflow bin K_c), the target's code into y and its class
//                        counted with an integer atomic
//  util_weights_kernel   balanced class weights from the counts (class order), s per row, [n_valid, present, S]
//  util_gram_kernel      F^T diag(s) F per row group through the fp64 MFMA, both operands made in registers
//  util_gram_fold_kernel M = (the groups' partials in group order / 2 + diag(reg)) / S
//  util_factor_kernel    one workgroup: ridge, Cholesky factor, its inverse, M^-1 = L^-T L^-1
//  util_grad_kernel      per row group, 64 rows at a time: logits F P (dense part on the MFMA, one-hot part as gathered
//                        rows of P), masked softmax and residual s (P - Y) in LDS, F^T R on the MFMA into the group's
//                        partial, the group's loss term
//  util_fold_kernel      G = (partials in group order + reg P) / S, and f(P)
//  util_update_kernel    W' = V - M^-1 G, V' = W' + beta (W' - W), one wave per entry
//  util_predict_kernel   logits of the held-out rows, argmax over the present classes, confusion matrix by integer
//                        atomics; util_scores_kernel: accuracy, weighted F1, max |G|
//
// Integer adds commute and every fp64 sum has an order fixed by the shapes alone, so a table scores bit-identically on
// every run.  Codes are clamped before they index anything.  An iteration is ordinary launches on one stream.
#include "common.h"
#include "eval_common.h"
#include "launch.h"
#include "util_feat.h"

#include <math.h>
#include <stdexcept>
#include <string>

namespace fedtgan {

constexpr int UTIL_THREADS = 256;
constexpr int UTIL_WAVES = UTIL_THREADS / WAVE;
constexpr int UTIL_FACTOR_THREADS = 1024;
constexpr int UTIL_ZLD = UTIL_MAX_CLASSES + 1;
constexpr int UTIL_MFMA_TILE = 32;
typedef double util_d4 __attribute__((ext_vector_type(4)));

static_assert(UTIL_MAX_FEATURES <= UTIL_FACTOR_THREADS, "a lane of util_factor_kernel owns one column");
static_assert(UTIL_ROWS == 64 && UTIL_THREADS == 256 && UTIL_SLAB == 16 * 4 * UTIL_WAVES, "util_grad_kernel's tiling");
static_assert(UTIL_CHUNK % UTIL_ROWS == 0 && UTIL_MAX_CLASSES == 64, "row blocks; one lane per class");

static int64_t util_chunks(int64_t n) {
  const int64_t chunks = (n + UTIL_CHUNK - 1) / UTIL_CHUNK;
  return chunks > 1 ? chunks : 1;
}

static int64_t util_group_cap(int64_t n, int64_t cells) {
  const int64_t chunks = util_chunks(n);
  int64_t cap = UTIL_PART_TARGET / (cells > 0 ? cells : 1);
  if (cap < 1) cap = 1;
  return chunks < cap ? chunks : cap;
}

CorrGroups util_groups(int64_t n, int64_t cells) {
  const int64_t chunks = util_chunks(n);
  const int64_t g0 = util_group_cap(n, cells);
  const int64_t per = (chunks + g0 - 1) / g0;
  CorrGroups g;
  g.groups = (int)((chunks + per - 1) / per);
  g.rows = (int)(per * UTIL_CHUNK);
  return g;
}

int64_t util_part_doubles(int64_t n_max, int64_t D, int64_t K) {
  const int64_t a = util_group_cap(n_max, D * D) * D * D, b = util_group_cap(n_max, D * K) * D * K;
  return a > b ? a : b;
}

static void util_check_table(const UtilTable& t, const char* what) {
  if (t.n < 1 || t.n_cont < 0 || t.n_cat < 0 || t.ldk < t.n || t.K < 1 || t.K > UTIL_MAX_CLASSES || t.D < 1 ||
      t.D > UTIL_MAX_FEATURES || t.D < t.n_cont + 2 * t.n_cat + 1)
    throw std::runtime_error(std::string(what) + ": table sizes");
}

// ============================================================================ pack
__global__ __launch_bounds__(UTIL_THREADS) void util_zero_kernel(int* p, int n) {
  const int i = blockIdx.x * UTIL_THREADS + threadIdx.x;
  if (i < n) p[i] = 0;
}

__global__ __launch_bounds__(UTIL_THREADS) void util_pack_kernel(UtilPackArgs a) {
  const UtilTable& t = a.t;
  const long long i = (long long)blockIdx.x * UTIL_THREADS + threadIdx.x;
  if (i >= (long long)t.n * a.n_cols) return;
  const long long r = i / a.n_cols;
  const int c = (int)(i - r * a.n_cols);
  const int k = a.kind[c], s = a.slot[c];
  const double v = a.values[i];
  if (k == UTIL_TARGET) {
    const int code = code_or_overflow(v, t.K);
    t.y[r] = code;
    if (is_code(v, t.K)) atomicAdd(&t.counts[code], 1);
  } else if (k == UTIL_CAT) {
    if (s >= 0 && s < t.n_cat) t.cat_t[(size_t)s * t.ldk + r] = code_or_overflow(v, t.card[s]);
  } else if (s >= 0 && s < t.n_cont) {
    t.cont[r * t.n_cont + s] = (v - a.mean[s]) / a.sd[s];
  }
}

__global__ __launch_bounds__(UTIL_THREADS) void util_weights_kernel(UtilTable t) {
  __shared__ double cw[UTIL_MAX_CLASSES];
  __shared__ int head[2];
  const int tid = threadIdx.x;
  if (tid == 0) class_head(t.counts, t.K, head[0], head[1]);
  __syncthreads();
  if (tid < t.K) cw[tid] = balanced_weight(head[0], head[1], t.counts[tid]);
  __syncthreads();
  if (blockIdx.x == 0 && tid == 0) {
    double S = 0.0;
    for (int c = 0; c < t.K; ++c) S += (double)t.counts[c] * cw[c];
    t.info[0] = (double)head[0];
    t.info[1] = (double)head[1];
    t.info[2] = S > 0.0 ? S : 1.0;
    t.info[3] = 0.0;
  }
  const int r = blockIdx.x * UTIL_THREADS + tid;
  if (r < t.n) {
    const int y = t.y[r];
    t.s[r] = (y >= 0 && y < t.K) ? cw[y] : 0.0;
  }
}

void launch_util_pack(const UtilPackArgs& a, hipStream_t stream) {
  require_unbatched("util_pack");
  const UtilTable& t = a.t;
  util_check_table(t, "util_pack");
  if (a.n_cols != t.n_cont + t.n_cat + 1) throw std::runtime_error("util_pack: n_cont + n_cat + 1 must be n_cols");
  const long long cells = (long long)t.n * a.n_cols;
  if (cells >= (long long)INT32_MAX) throw std::runtime_error("util_pack: table too large");
  hipLaunchKernelGGL(util_zero_kernel, dim3(1), dim3(UTIL_THREADS), 0, stream, t.counts, t.K);
  hipLaunchKernelGGL(util_pack_kernel, dim3((unsigned)((cells + UTIL_THREADS - 1) / UTIL_THREADS)), dim3(UTIL_THREADS),
                     0, stream, a);
  hipLaunchKernelGGL(util_weights_kernel, dim3((unsigned)((t.n + UTIL_THREADS - 1) / UTIL_THREADS)),
                     dim3(UTIL_THREADS), 0, stream, t);
}

// ============================================================================ gram
// part[g] = F^T diag(s) F over the rows of group g.  v_mfma_f64_16x16x4_f64: lane l feeds A[i = l & 15][k = l >> 4] and
// B[k = l >> 4][j = l & 15] and holds D[(l >> 4) + 4 reg][l & 15]; k is a table row, and both operands are the lane's
// feature of that row, read (continuous) or made from the code (one-hot) in registers.  A wave owns a 32 x 32 tile as
// 2 x 2 MFMA tiles; the four waves take the group's row quads round-robin and are added in wave order through LDS.
__global__ __launch_bounds__(UTIL_THREADS) void util_gram_kernel(UtilTable t, double* part, int rows_per_group) {
  __shared__ double red[UTIL_WAVES][UTIL_MFMA_TILE][UTIL_MFMA_TILE + 1];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, li = lane & 15, lk = lane >> 4;
  const int j0 = blockIdx.x * UTIL_MFMA_TILE, i0 = blockIdx.y * UTIL_MFMA_TILE, g = blockIdx.z;
  const int r0 = g * rows_per_group, r1 = min(t.n, r0 + rows_per_group);
  UFeat fd[4];      // the lane's two rows (t = 0, 1) and two columns (t = 2, 3) of the tile
#pragma unroll
  for (int q = 0; q < 4; ++q) fd[q] = util_feat(t, (q < 2 ? i0 : j0) + (q & 1) * 16 + li);
  util_d4 acc[2][2];
#pragma unroll
  for (int u = 0; u < 2; ++u)
#pragma unroll
    for (int v = 0; v < 2; ++v) acc[u][v] = (util_d4){0.0, 0.0, 0.0, 0.0};
  for (int r = r0 + 4 * w; r < r1; r += 4 * UTIL_WAVES) {      // (uniform over the wave: every lane reaches the MFMA)
    const int row = r + lk;
    const bool live = row < r1;
    const double sv = live ? t.s[row] : 0.0;
    double x[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) x[q] = live ? util_fval(t, fd[q], row) : 0.0;
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
      for (int v = 0; v < 2; ++v)
        acc[u][v] = __builtin_amdgcn_mfma_f64_16x16x4f64(x[u] * sv, x[2 + v], acc[u][v], 0, 0, 0);
  }
#pragma unroll
  for (int u = 0; u < 2; ++u)
#pragma unroll
    for (int v = 0; v < 2; ++v)
#pragma unroll
      for (int q = 0; q < 4; ++q) red[w][u * 16 + lk + 4 * q][v * 16 + li] = acc[u][v][q];
  __syncthreads();
  double* out = part + (size_t)g * t.D * t.D;
  for (int e = tid; e < UTIL_MFMA_TILE * UTIL_MFMA_TILE; e += UTIL_THREADS) {
    const int ii = e / UTIL_MFMA_TILE, jj = e - ii * UTIL_MFMA_TILE;
    const int i = i0 + ii, j = j0 + jj;
    if (i < t.D && j < t.D)
      out[(size_t)i * t.D + j] = ((red[0][ii][jj] + red[1][ii][jj]) + red[2][ii][jj]) + red[3][ii][jj];
  }
}

__global__ __launch_bounds__(UTIL_THREADS) void util_gram_fold_kernel(const double* part, int groups, int D,
                                                                       const double* info, double* M) {
  const int e = blockIdx.x * UTIL_THREADS + threadIdx.x;
  const int cells = D * D;
  if (e >= cells) return;
  double acc = 0.0;
  for (int g = 0; g < groups; ++g) acc += part[(size_t)g * cells + e];
  const int i = e / D, j = e - i * D;
  M[e] = (0.5 * acc + ((i == j && i != D - 1) ? 1.0 : 0.0)) / info[2];
}

void launch_util_gram(const UtilTable& t, double* M, double* part, hipStream_t stream) {
  require_unbatched("util_gram");
  util_check_table(t, "util_gram");
  const CorrGroups gr = util_groups(t.n, (int64_t)t.D * t.D);
  const unsigned tiles = (unsigned)((t.D + UTIL_MFMA_TILE - 1) / UTIL_MFMA_TILE);
  if (gr.groups > 65535) throw std::runtime_error("util_gram: too many rows");
  hipLaunchKernelGGL(util_gram_kernel, dim3(tiles, tiles, (unsigned)gr.groups), dim3(UTIL_THREADS), 0, stream, t, part,
                     gr.rows);
  hipLaunchKernelGGL(util_gram_fold_kernel, dim3((unsigned)((t.D * t.D + UTIL_THREADS - 1) / UTIL_THREADS)),
                     dim3(UTIL_THREADS), 0, stream, part, gr.groups, t.D, t.info, M);
}

// ============================================================================ factor
// One workgroup; lane i owns column i.  Lt[k][i] = L[i][k] (the factor, transposed so that a column step reads
// consecutive addresses), X = L^-1 (lower triangle), Minv[i][j] = sum over k >= max(i, j) of X[k][i] X[k][j].  Every
// sum runs over k ascending.
__global__ __launch_bounds__(UTIL_FACTOR_THREADS) void util_factor_kernel(const double* M, int D, double* Lt, double* X,
                                                                           double* Minv) {
  __shared__ double sh_d;
  const int i = threadIdx.x;
  if (i == 0) {
    double tr = 0.0;
    for (int k = 0; k < D; ++k) tr += M[(size_t)k * D + k];
    sh_d = 1e-10 * tr / (double)D;
  }
  __syncthreads();
  const double ridge = sh_d;
  __syncthreads();
  for (int j = 0; j < D; ++j) {
    double v = 0.0;
    if (i >= j && i < D) {
      v = M[(size_t)j * D + i] + (i == j ? ridge : 0.0);
      for (int k = 0; k < j; ++k) v -= Lt[(size_t)k * D + i] * Lt[(size_t)k * D + j];
      if (i == j) sh_d = sqrt(v > 1e-300 ? v : 1e-300);
    }
    __syncthreads();
    if (i >= j && i < D) Lt[(size_t)j * D + i] = i == j ? sh_d : v / sh_d;
    __syncthreads();
  }
  if (i < D) {
    for (int r = 0; r < i; ++r) X[(size_t)r * D + i] = 0.0;
    X[(size_t)i * D + i] = 1.0 / Lt[(size_t)i * D + i];
    for (int r = i + 1; r < D; ++r) {
      double acc = 0.0;
      for (int k = i; k < r; ++k) acc += Lt[(size_t)k * D + r] * X[(size_t)k * D + i];
      X[(size_t)r * D + i] = -acc / Lt[(size_t)r * D + r];
    }
  }
  __syncthreads();
  for (int e = i; e < D * D; e += UTIL_FACTOR_THREADS) {
    const int a = e / D, b = e - a * D;
    double acc = 0.0;
    for (int k = max(a, b); k < D; ++k) acc += X[(size_t)k * D + a] * X[(size_t)k * D + b];
    Minv[e] = acc;
  }
}

void launch_util_factor(const double* M, int D, double* Lt, double* X, double* Minv, hipStream_t stream) {
  require_unbatched("util_factor");
  if (D < 1 || D > UTIL_MAX_FEATURES) throw std::runtime_error("util_factor: matrix size");
  hipLaunchKernelGGL(util_factor_kernel, dim3(1), dim3(UTIL_FACTOR_THREADS), 0, stream, M, D, Lt, X, Minv);
}

// ============================================================================ logits of a block of 64 rows
// Z[r][c] = F[rb + r] . P[:, c] for the rows below r1.  Wave w owns rows 16 w .. 16 w + 15: the continuous part is an
// MFMA product over k = continuous column (A = 16 rows x 4 columns of cont, B = 4 rows x 16 classes of P); then four
// lanes per row add the rows of P that the row's codes select, column by column, and the intercept's
// (util_logits_row).  This first half leaves the dense part in Z and ends with a barrier.  CT = tiles of 16 classes.
template <int CT>
__device__ __forceinline__ void util_logits_dense(const UtilTable& t, const double* P, int rb, int r1,
                                            double (*Z)[UTIL_ZLD]) {
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, li = lane & 15, lk = lane >> 4;
  const int nc = t.n_cont, K = t.K;
  util_d4 acc[CT];
#pragma unroll
  for (int ct = 0; ct < CT; ++ct) acc[ct] = (util_d4){0.0, 0.0, 0.0, 0.0};
  const int arow = rb + 16 * w + li;
  const bool alive = arow < r1;
  for (int k0 = 0; k0 < nc; k0 += 4) {
    const int kk = k0 + lk;
    const bool kin = kk < nc;
    const double a = (alive && kin) ? t.cont[(size_t)arow * nc + kk] : 0.0;
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) {
      const int cls = ct * 16 + li;
      const double b = (kin && cls < K) ? P[(size_t)kk * K + cls] : 0.0;
      acc[ct] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc[ct], 0, 0, 0);
    }
  }
#pragma unroll
  for (int ct = 0; ct < CT; ++ct)
#pragma unroll
    for (int q = 0; q < 4; ++q) Z[16 * w + lk + 4 * q][ct * 16 + li] = acc[ct][q];
  __syncthreads();
}

// the second half, for lane (row zr = tid >> 2, class quarter cq = tid & 3) with rb + zr < r1: the lane's logits
// z[e] of the classes cq + 4 e (0 past K), the dense part from Z plus the one-hot rows and the intercept
template <int CT>
__device__ __forceinline__ void util_logits_row(const UtilTable& t, const double* P, int row, int zr, int cq,
                                                double (*Z)[UTIL_ZLD], double* z) {
  const int nc = t.n_cont, K = t.K;
#pragma unroll
  for (int e = 0; e < CT * 4; ++e) z[e] = cq + 4 * e < K ? Z[zr][cq + 4 * e] : 0.0;
  for (int cc = 0; cc < t.n_cat; ++cc) {
    const int f = nc + t.offs[cc] + code_clamp(t.cat_t[(size_t)cc * t.ldk + row], t.card[cc]);
    if (f >= nc && f < t.D - 1) {
      const double* base = P + (size_t)f * K;
#pragma unroll
      for (int e = 0; e < CT * 4; ++e)
        if (cq + 4 * e < K) z[e] += base[cq + 4 * e];
    }
  }
  const double* base = P + (size_t)(t.D - 1) * K;
#pragma unroll
  for (int e = 0; e < CT * 4; ++e)
    if (cq + 4 * e < K) z[e] += base[cq + 4 * e];
}

// a sum / maximum over the four lanes of a row (lanes 4 r .. 4 r + 3 of a wave), in a fixed order
__device__ __forceinline__ double util_quad_sum(double v) {
  v += __shfl_xor(v, 1, WAVE);
  return v + __shfl_xor(v, 2, WAVE);
}
__device__ __forceinline__ double util_quad_max(double v) {
  v = fmax(v, __shfl_xor(v, 1, WAVE));
  return fmax(v, __shfl_xor(v, 2, WAVE));
}

// ============================================================================ gradient
// grid (slabs of UTIL_SLAB features, row groups).  A workgroup walks its group 64 rows at a time; wave w accumulates
// the feature tiles w, w + 4, w + 8, w + 12 of its slab over all of them, so a partial is written once per group.
template <int CT>
__global__ __launch_bounds__(UTIL_THREADS) void util_grad_kernel(UtilTable t, const double* P, double* part,
                                                                  double* lossp, int rows_per_group) {
  __shared__ double Z[UTIL_ROWS][UTIL_ZLD];
  __shared__ double lrow[UTIL_ROWS];
  __shared__ int pres[UTIL_MAX_CLASSES];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, li = lane & 15, lk = lane >> 4;
  const int K = t.K, D = t.D;
  const int fs = blockIdx.x * UTIL_SLAB, g = blockIdx.y;
  const int r0 = g * rows_per_group, r1 = min(t.n, r0 + rows_per_group);
  if (tid < UTIL_MAX_CLASSES) pres[tid] = tid < K && t.counts[tid] > 0;
  UFeat fd[4];
#pragma unroll
  for (int u = 0; u < 4; ++u) fd[u] = util_feat(t, fs + 16 * (w + 4 * u) + li);
  util_d4 acc[4][CT];
#pragma unroll
  for (int u = 0; u < 4; ++u)
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) acc[u][ct] = (util_d4){0.0, 0.0, 0.0, 0.0};
  double gl = 0.0;
  for (int rb = r0; rb < r1; rb += UTIL_ROWS) {
    util_logits_dense<CT>(t, P, rb, r1, Z);
    {       // four lanes per row: the rest of the logits, the masked softmax, the row's loss, Z := s (P - Y)
      const int zr = tid >> 2, cq = tid & 3, row = rb + zr;
      const double sv = row < r1 ? t.s[row] : 0.0;
      const int yy = row < r1 ? t.y[row] : K;
      double lo = 0.0;
      if (sv > 0.0 && yy >= 0 && yy < K) {          // (the same for the four lanes of a row)
        double z[CT * 4];
        util_logits_row<CT>(t, P, row, zr, cq, Z, z);
        double mx = -INFINITY, zy = 0.0, sum = 0.0;
#pragma unroll
        for (int e = 0; e < CT * 4; ++e) {
          const int c = cq + 4 * e;
          if (pres[c]) mx = fmax(mx, z[e]);
          if (c == yy) zy = z[e];
        }
        mx = util_quad_max(mx);
        zy = util_quad_sum(zy);
#pragma unroll
        for (int e = 0; e < CT * 4; ++e) {
          z[e] = pres[cq + 4 * e] ? exp(z[e] - mx) : 0.0;
          sum += z[e];
        }
        sum = util_quad_sum(sum);
        lo = sv * (log(sum) + mx - zy);
#pragma unroll
        for (int e = 0; e < CT * 4; ++e) Z[zr][cq + 4 * e] = sv * (z[e] / sum - (cq + 4 * e == yy ? 1.0 : 0.0));
      } else {
#pragma unroll
        for (int e = 0; e < CT * 4; ++e) Z[zr][cq + 4 * e] = 0.0;
      }
      if (cq == 0) lrow[zr] = lo;
    }
    __syncthreads();
    if (tid == 0)
      for (int r = 0; r < UTIL_ROWS; ++r) gl += lrow[r];
#pragma unroll 4
    for (int q = 0; q < UTIL_ROWS / 4; ++q) {
      const int row = rb + 4 * q + lk;
      const bool live = row < r1;
      double b[CT];
#pragma unroll
      for (int ct = 0; ct < CT; ++ct) b[ct] = Z[4 * q + lk][ct * 16 + li];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        if (fs + 16 * (w + 4 * u) < D) {          // (uniform over the wave)
          const double a = live ? util_fval(t, fd[u], row) : 0.0;
#pragma unroll
          for (int ct = 0; ct < CT; ++ct) acc[u][ct] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b[ct], acc[u][ct], 0, 0, 0);
        }
      }
    }
    __syncthreads();
  }
  double* out = part + (size_t)g * D * K;
#pragma unroll
  for (int u = 0; u < 4; ++u)
#pragma unroll
    for (int ct = 0; ct < CT; ++ct)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int f = fs + 16 * (w + 4 * u) + lk + 4 * q, c = ct * 16 + li;
        if (f < D && c < K) out[(size_t)f * K + c] = acc[u][ct][q];
      }
  if (blockIdx.x == 0 && tid == 0) lossp[g] = gl;
}

// the last workgroup sums the loss: lanes stride over the groups and over P, then a fixed tree
__global__ __launch_bounds__(UTIL_THREADS) void util_fold_kernel(const double* part, int groups, const double* lossp,
                                                                  const double* P, int D, int K, const double* info,
                                                                  double* G, double* loss) {
  __shared__ double sh[UTIL_THREADS];
  const int tid = threadIdx.x, cells = D * K;
  const double S = info[2];
  if (blockIdx.x + 1 < gridDim.x) {      // 16 elements x 16 slices of the groups; the slices are added in order
    const int el = tid & 15, q = tid >> 4, e = blockIdx.x * 16 + el;
    double acc = 0.0;
    if (e < cells)
      for (int g = q; g < groups; g += 16) acc += part[(size_t)g * cells + e];
    sh[tid] = acc;
    __syncthreads();
    if (q == 0 && e < cells) {
      acc = 0.0;
      for (int k = 0; k < 16; ++k) acc += sh[k * 16 + el];
      G[e] = (acc + (e / K != D - 1 ? P[e] : 0.0)) / S;
    }
    return;
  }
  double a = 0.0, q = 0.0;
  for (int g = tid; g < groups; g += UTIL_THREADS) a += lossp[g];
  for (int e = tid; e < cells - K; e += UTIL_THREADS) q += P[e] * P[e];
  sh[tid] = a + 0.5 * q;
  __syncthreads();
  for (int s = UTIL_THREADS / 2; s > 0; s >>= 1) {
    if (tid < s) sh[tid] += sh[tid + s];
    __syncthreads();
  }
  if (tid == 0) loss[0] = sh[0] / S;
}

void launch_util_grad(const UtilTable& t, const double* P, double* G, double* loss, double* part, double* lossp,
                      hipStream_t stream) {
  require_unbatched("util_grad");
  util_check_table(t, "util_grad");
  const CorrGroups gr = util_groups(t.n, (int64_t)t.D * t.K);
  if (gr.groups > 65535) throw std::runtime_error("util_grad: too many rows");
  const dim3 grid((unsigned)((t.D + UTIL_SLAB - 1) / UTIL_SLAB), (unsigned)gr.groups);
  if (t.K <= 16)
    hipLaunchKernelGGL(util_grad_kernel<1>, grid, dim3(UTIL_THREADS), 0, stream, t, P, part, lossp, gr.rows);
  else if (t.K <= 32)
    hipLaunchKernelGGL(util_grad_kernel<2>, grid, dim3(UTIL_THREADS), 0, stream, t, P, part, lossp, gr.rows);
  else
    hipLaunchKernelGGL(util_grad_kernel<4>, grid, dim3(UTIL_THREADS), 0, stream, t, P, part, lossp, gr.rows);
  hipLaunchKernelGGL(util_fold_kernel, dim3((unsigned)((t.D * t.K + 15) / 16) + 1),
                     dim3(UTIL_THREADS), 0, stream, part, gr.groups, lossp, P, t.D, t.K, t.info, G, loss);
}

// ============================================================================ update
// one wave per entry: the lanes stride over M^-1's row, the wave folds them in a fixed tree
__global__ __launch_bounds__(UTIL_THREADS) void util_update_kernel(double* V, double* W, const double* Minv,
                                                                    const double* G, int D, int K, double beta) {
  const int lane = threadIdx.x & 63, e = blockIdx.x * UTIL_WAVES + (threadIdx.x >> 6);
  if (e >= D * K) return;                    // (uniform over the wave)
  const int f = e / K, c = e - f * K;
  double d = 0.0;
  for (int j = lane; j < D; j += WAVE) d += Minv[(size_t)f * D + j] * G[(size_t)j * K + c];
  d = wave_sum_d(d);
  if (lane == 0) {
    const double wn = V[e] - d;
    V[e] = wn + beta * (wn - W[e]);
    W[e] = wn;
  }
}

void launch_util_update(double* V, double* W, const double* Minv, const double* G, int D, int K, double beta,
                        hipStream_t stream) {
  require_unbatched("util_update");
  if (D < 1 || D > UTIL_MAX_FEATURES || K < 1 || K > UTIL_MAX_CLASSES) throw std::runtime_error("util_update: sizes");
  hipLaunchKernelGGL(util_update_kernel, dim3((unsigned)((D * K + UTIL_WAVES - 1) / UTIL_WAVES)),
                     dim3(UTIL_THREADS), 0, stream, V, W, Minv, G, D, K, beta);
}

// ============================================================================ predict
template <int CT>
__global__ __launch_bounds__(UTIL_THREADS) void util_predict_kernel(UtilTable t, const int* train_counts,
                                                                     const double* W, int* conf) {
  __shared__ double Z[UTIL_ROWS][UTIL_ZLD];
  __shared__ int pres[UTIL_MAX_CLASSES];
  const int tid = threadIdx.x, K = t.K;
  if (tid < UTIL_MAX_CLASSES) pres[tid] = tid < K && train_counts[tid] > 0;
  const int rb = blockIdx.x * UTIL_ROWS;
  util_logits_dense<CT>(t, W, rb, t.n, Z);
  {
    const int zr = tid >> 2, cq = tid & 3;
    if (rb + zr < t.n) {
      double z[CT * 4];
      util_logits_row<CT>(t, W, rb + zr, zr, cq, Z, z);
#pragma unroll
      for (int e = 0; e < CT * 4; ++e) Z[zr][cq + 4 * e] = z[e];
    }
  }
  __syncthreads();
  const int row = rb + tid;
  if (tid < UTIL_ROWS && row < t.n) {
    const int yy = t.y[row];
    if (yy >= 0 && yy < K) {
      int best = -1;
      double bv = 0.0;
      for (int c = 0; c < K; ++c)
        if (pres[c] && (best < 0 || Z[tid][c] > bv)) {       // (strictly greater: a tie stays with the lower class)
          best = c;
          bv = Z[tid][c];
        }
      atomicAdd(&conf[yy * K + (best < 0 ? 0 : best)], 1);
    }
  }
}

__global__ __launch_bounds__(UTIL_THREADS) void util_scores_kernel(const int* conf, int K, const double* G, int cells,
                                                                    const double* loss, const double* real,
                                                                    double* out) {
  __shared__ double sm[UTIL_THREADS];
  __shared__ int tp[UTIL_MAX_CLASSES], rs[UTIL_MAX_CLASSES], cs[UTIL_MAX_CLASSES];
  const int tid = threadIdx.x;
  double m = 0.0;
  for (int e = tid; e < cells; e += UTIL_THREADS) m = fmax(m, fabs(G[e]));
  sm[tid] = m;
  if (tid < K) {
    int r = 0, c = 0;
    for (int j = 0; j < K; ++j) {
      r += conf[tid * K + j];
      c += conf[j * K + tid];
    }
    rs[tid] = r;
    cs[tid] = c;
    tp[tid] = conf[tid * K + tid];
  }
  __syncthreads();
  for (int s = UTIL_THREADS / 2; s > 0; s >>= 1) {
    if (tid < s) sm[tid] = fmax(sm[tid], sm[tid + s]);
    __syncthreads();
  }
  if (tid == 0) {
    confusion_scores(rs, cs, tp, K, real, out);
    out[6] = loss[0];
    out[7] = sm[0];
  }
}

void launch_util_predict(const UtilTable& t, const int* train_counts, const double* W, int* conf, const double* G,
                         const double* loss, const double* real, double* out, hipStream_t stream) {
  require_unbatched("util_predict");
  util_check_table(t, "util_predict");
  hipLaunchKernelGGL(util_zero_kernel, dim3((unsigned)((t.K * t.K + UTIL_THREADS - 1) / UTIL_THREADS)),
                     dim3(UTIL_THREADS), 0, stream, conf, t.K * t.K);
  const dim3 grid((unsigned)((t.n + UTIL_ROWS - 1) / UTIL_ROWS));
  if (t.K <= 16)
    hipLaunchKernelGGL(util_predict_kernel<1>, grid, dim3(UTIL_THREADS), 0, stream, t, train_counts, W, conf);
  else if (t.K <= 32)
    hipLaunchKernelGGL(util_predict_kernel<2>, grid, dim3(UTIL_THREADS), 0, stream, t, train_counts, W, conf);
  else
    hipLaunchKernelGGL(util_predict_kernel<4>, grid, dim3(UTIL_THREADS), 0, stream, t, train_counts, W, conf);
  hipLaunchKernelGGL(util_scores_kernel, dim3(1), dim3(UTIL_THREADS), 0, stream, conf, t.K, G, t.D * t.K, loss, real,
                     out);
}

}  // namespace fedtgan
