// MLP-utility evaluator (eval/mlp_device.py DeviceMLP): a one-hidden-layer network h = relu(F W1), z = [h | 1] W2
// trained on a decoded table by a fixed number of Adam steps over strided batches, its loss over the whole table and its
// confusion matrix on held-out rows, on the device.  Features F = [standardised continuous | one-hot(codes) | 1] of
// the packed table of utility.hip (util_pack fills it); the one-hot blocks never exist in memory.  theta = [W1 [D, H] |
// W2 [H + 1, K]], the last rows the biases.
//
//  mlp_forward_kernel<MLP_STEP>     a block of 64 rows of the batch: h's dense part on the fp64 MFMA, its one-hot part
//                                   as gathered rows of W1, relu; z = [h | 1] W2 on the MFMA; the masked softmax and
//                                   dZ in LDS; dH = (dZ W2^T) . (h > 0) on the MFMA; h, dZ, dH of the block go to
//                                   global scratch, and the block's count of valid rows
//  mlp_grad_adam_kernel             one wave per 16 x 16 tile of W1's gradient F^T dH (A made in registers: util_feat /
//                                   util_fval) or of W2's [h | 1]^T dZ: all batch rows in row order on the MFMA, the L2
//                                   term, the division by the valid rows (the blocks' counts in block order), Adam on
//                                   the tile's own entries of theta and the moments
//  mlp_forward_kernel<MLP_LOSS>     the same forward over all rows; the blocks' loss sums, folded in block order by
//                                   mlp_loss_fold_kernel with the L2 term
//  mlp_forward_kernel<MLP_PREDICT>  the same forward over the held-out rows, argmax over the present classes,
//                                   confusion matrix by integer atomics; mlp_scores_kernel: accuracy, weighted F1
//
// A step is these two launches.  The block's h [64, 128] and z [64, 64] are 98 KiB of static LDS: one workgroup per
// CU, chosen over tiling H because a batch is at most 16 blocks, far fewer than there are CUs.
// Integer adds commute and every fp64 sum has an order fixed by the shapes alone, so a table scores bit-identically on
// every run.  Codes are clamped before they index anything, rows past the end are masked, and so are the columns of
// H and K beyond the last multiple of 16.  Ordinary launches on one stream.
#include "common.h"
#include "eval_common.h"
#include "launch.h"
#include "util_feat.h"

#include <math.h>
#include <stdexcept>
#include <string>

namespace fedtgan {

constexpr int MLP_THREADS = 256;
constexpr int MLP_WAVES = MLP_THREADS / WAVE;
constexpr int MLP_HLD = MLP_MAX_HIDDEN + 1;
constexpr int MLP_ZLD = UTIL_MAX_CLASSES + 1;
enum MlpMode : int { MLP_STEP = 0, MLP_LOSS = 1, MLP_PREDICT = 2 };
typedef double mlp_d4 __attribute__((ext_vector_type(4)));

static_assert(MLP_ROWS == 64 && MLP_THREADS == 256 && UTIL_MAX_CLASSES == 64, "mlp_forward_kernel's tiling");
static_assert(MLP_MAX_HIDDEN % 16 == 0 && MLP_MAX_BATCH % MLP_ROWS == 0, "whole MFMA tiles, whole row blocks");

// the rows of a pass: table rows base + j stride for j < count (a batch: b, nb; a whole table: 0, 1, n)
struct MlpRows {
  int base, stride, count;
};

struct MlpFwdArgs {
  UtilTable t;
  MlpRows rows;
  const double* theta;
  int H;
  const int* counts;      // [K] the classes with counts > 0 are present
  double* h;              // STEP: [count, H]
  double* dz;             // STEP: [count, K]
  double* dh;             // STEP: [count, H]
  int* cnt;               // STEP: [blocks]
  double* lossp;          // LOSS: [blocks]
  int* conf;              // PREDICT: [K, K]
};

__device__ __forceinline__ double mlp_quad_sum(double v) {
  v += __shfl_xor(v, 1, WAVE);
  return v + __shfl_xor(v, 2, WAVE);
}
__device__ __forceinline__ double mlp_quad_max(double v) {
  v = fmax(v, __shfl_xor(v, 1, WAVE));
  return fmax(v, __shfl_xor(v, 2, WAVE));
}

__global__ __launch_bounds__(MLP_THREADS) void mlp_zero_kernel(int* p, int n) {
  const int i = blockIdx.x * MLP_THREADS + threadIdx.x;
  if (i < n) p[i] = 0;
}

// ============================================================================ forward (and backward to dH)
// v_mfma_f64_16x16x4_f64: lane l feeds A[i = l & 15][k = l >> 4] and B[k = l >> 4][j = l & 15] and holds
// D[(l >> 4) + 4 reg][l & 15].  Wave w owns the block's rows 16 w .. 16 w + 15 in every product.
template <int MODE>
__global__ __launch_bounds__(MLP_THREADS) void mlp_forward_kernel(MlpFwdArgs a) {
  __shared__ double Hs[MLP_ROWS][MLP_HLD];
  __shared__ double Z[MLP_ROWS][MLP_ZLD];
  __shared__ double lrow[MLP_ROWS];
  __shared__ int vrow[MLP_ROWS];
  __shared__ int pres[UTIL_MAX_CLASSES];
  const UtilTable& t = a.t;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, li = lane & 15, lk = lane >> 4;
  const int H = a.H, K = t.K, D = t.D, nc = t.n_cont;
  const int HT = (H + 15) >> 4, CT = (K + 15) >> 4;
  const double* W1 = a.theta;
  const double* W2 = a.theta + (size_t)D * H;
  const int j0 = blockIdx.x * MLP_ROWS, count = a.rows.count;
  if (tid < UTIL_MAX_CLASSES) pres[tid] = tid < K && a.counts[tid] > 0;
  {       // h's dense part: A = 16 rows x 4 columns of cont, B = 4 rows x 16 columns of W1
    const int aj = j0 + 16 * w + li;
    const bool alive = aj < count;
    const size_t arow = alive ? (size_t)(a.rows.base + aj * a.rows.stride) : 0;
    for (int ht = 0; ht < HT; ++ht) {
      const int hc = ht * 16 + li;
      mlp_d4 acc = (mlp_d4){0.0, 0.0, 0.0, 0.0};
      for (int k0 = 0; k0 < nc; k0 += 4) {
        const int kk = k0 + lk;
        const bool kin = kk < nc;
        const double av = (alive && kin) ? t.cont[arow * nc + kk] : 0.0;
        const double bv = (kin && hc < H) ? W1[(size_t)kk * H + hc] : 0.0;
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, acc, 0, 0, 0);
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) Hs[16 * w + lk + 4 * q][hc] = acc[q];
    }
  }
  __syncthreads();
  // four lanes per row from here to the softmax: lane (row zr, quarter cq) owns the columns cq, cq + 4, ...
  const int zr = tid >> 2, cq = tid & 3, zj = j0 + zr;
  const bool live = zj < count;
  const int row = live ? a.rows.base + zj * a.rows.stride : 0;
  if (live) {     // the one-hot part: the rows of W1 that the row's codes select, column by column; the bias; relu
    for (int cc = 0; cc < t.n_cat; ++cc) {
      const int f = nc + t.offs[cc] + code_clamp(t.cat_t[(size_t)cc * t.ldk + row], t.card[cc]);
      if (f >= nc && f < D - 1) {
        const double* wrow = W1 + (size_t)f * H;
        for (int hc = cq; hc < H; hc += 4) Hs[zr][hc] += wrow[hc];
      }
    }
    const double* bias = W1 + (size_t)(D - 1) * H;
    for (int hc = cq; hc < H; hc += 4) {
      double v = Hs[zr][hc] + bias[hc];
      v = v > 0.0 ? v : 0.0;
      Hs[zr][hc] = v;
      if (MODE == MLP_STEP) a.h[(size_t)zj * H + hc] = v;
    }
  } else {
    for (int hc = cq; hc < H; hc += 4) Hs[zr][hc] = 0.0;
  }
  __syncthreads();
  for (int ct = 0; ct < CT; ++ct) {       // z = [h | 1] W2: k runs over H + 1, the last the bias row
    const int cls = ct * 16 + li;
    mlp_d4 acc = (mlp_d4){0.0, 0.0, 0.0, 0.0};
    for (int k0 = 0; k0 < H + 1; k0 += 4) {
      const int kk = k0 + lk;
      const double av = kk < H ? Hs[16 * w + li][kk] : (kk == H ? 1.0 : 0.0);
      const double bv = (kk <= H && cls < K) ? W2[(size_t)kk * K + cls] : 0.0;
      acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, acc, 0, 0, 0);
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) Z[16 * w + lk + 4 * q][cls] = acc[q];
  }
  __syncthreads();
  if (MODE == MLP_PREDICT) {
    const int pj = j0 + tid;
    if (tid < MLP_ROWS && pj < count) {
      const int yy = t.y[a.rows.base + pj * a.rows.stride];
      if (yy >= 0 && yy < K) {
        int best = -1;
        double bv = 0.0;
        for (int c = 0; c < K; ++c)
          if (pres[c] && (best < 0 || Z[tid][c] > bv)) {       // (strictly greater: a tie stays with the lower class)
            best = c;
            bv = Z[tid][c];
          }
        atomicAdd(&a.conf[yy * K + (best < 0 ? 0 : best)], 1);
      }
    }
    return;
  }
  {       // the masked softmax, the row's loss, Z := dZ = P - Y (0 for a row that is not valid)
    const int yy = live ? t.y[row] : K;
    const bool valid = live && yy >= 0 && yy < K;          // (the same for the four lanes of a row)
    double lo = 0.0;
    if (valid) {
      double mx = -INFINITY, zy = 0.0, sum = 0.0;
      for (int c = cq; c < K; c += 4) {
        const double z = Z[zr][c];
        if (pres[c]) mx = fmax(mx, z);
        if (c == yy) zy = z;
      }
      mx = mlp_quad_max(mx);
      zy = mlp_quad_sum(zy);
      for (int c = cq; c < K; c += 4) {
        const double e = pres[c] ? exp(Z[zr][c] - mx) : 0.0;
        Z[zr][c] = e;
        sum += e;
      }
      sum = mlp_quad_sum(sum);
      lo = log(sum) + mx - zy;
      for (int c = cq; c < K; c += 4) Z[zr][c] = Z[zr][c] / sum - (c == yy ? 1.0 : 0.0);
    } else {
      for (int c = cq; c < K; c += 4) Z[zr][c] = 0.0;
    }
    if (MODE == MLP_STEP && live)
      for (int c = cq; c < K; c += 4) a.dz[(size_t)zj * K + c] = Z[zr][c];
    if (cq == 0) {
      lrow[zr] = lo;
      vrow[zr] = valid ? 1 : 0;
    }
  }
  __syncthreads();
  if (MODE == MLP_LOSS) {
    if (tid == 0) {
      double gl = 0.0;
      for (int r = 0; r < MLP_ROWS; ++r) gl += lrow[r];
      a.lossp[blockIdx.x] = gl;
    }
    return;
  }
  if (tid == 0) {
    int nv = 0;
    for (int r = 0; r < MLP_ROWS; ++r) nv += vrow[r];
    a.cnt[blockIdx.x] = nv;
  }
  for (int ht = 0; ht < HT; ++ht) {       // dH = (dZ W2^T) . (h > 0): k runs over the classes
    const int hc = ht * 16 + li;
    mlp_d4 acc = (mlp_d4){0.0, 0.0, 0.0, 0.0};
    for (int c0 = 0; c0 < K; c0 += 4) {
      const int cc = c0 + lk;
      const double av = cc < K ? Z[16 * w + li][cc] : 0.0;
      const double bv = (cc < K && hc < H) ? W2[(size_t)hc * K + cc] : 0.0;
      acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, acc, 0, 0, 0);
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int r = 16 * w + lk + 4 * q;
      if (j0 + r < count && hc < H) a.dh[(size_t)(j0 + r) * H + hc] = Hs[r][hc] > 0.0 ? acc[q] : 0.0;
    }
  }
}

// ============================================================================ gradient tile + Adam
__device__ __forceinline__ void mlp_adam(const MlpStepArgs& a, size_t e, double g) {
  const double mm = 0.9 * a.mom[e] + 0.1 * g;
  const double vv = 0.999 * a.var[e] + 0.001 * (g * g);
  a.mom[e] = mm;
  a.var[e] = vv;
  a.theta[e] -= a.lr_t * mm / (sqrt(vv) + 1e-8);
}

// Wave `tile` owns one 16 x 16 tile: the first tiles1 are W1's (feature tile major), the rest W2's.  k is a batch row;
// the accumulator runs over all of them in row order.  No other wave reads or writes the tile's entries of theta.
__global__ __launch_bounds__(MLP_THREADS) void mlp_grad_adam_kernel(MlpStepArgs a, int rows, int blocks, int tiles1,
                                                                     int tiles) {
  const UtilTable& t = a.t;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, li = lane & 15, lk = lane >> 4;
  const int tile = blockIdx.x * MLP_WAVES + w;
  if (tile >= tiles) return;              // (uniform over the wave)
  const int H = a.H, K = t.K, D = t.D;
  const int HT = (H + 15) >> 4, CT = (K + 15) >> 4;
  int nv = 0;
  for (int b = 0; b < blocks; ++b) nv += a.cnt[b];
  const double m = nv > 0 ? (double)nv : 1.0;
  mlp_d4 acc = (mlp_d4){0.0, 0.0, 0.0, 0.0};
  if (tile < tiles1) {                    // F^T dH: A = the lane's feature of 4 rows, made in registers
    const int f0 = (tile / HT) * 16, hc = (tile % HT) * 16 + li;
    const UFeat fd = util_feat(t, f0 + li);
    for (int j = 0; j < rows; j += 4) {
      const int jj = j + lk;
      const bool on = jj < rows;
      const double av = on ? util_fval(t, fd, a.b + jj * a.nb) : 0.0;
      const double bv = (on && hc < H) ? a.dh[(size_t)jj * H + hc] : 0.0;
      acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, acc, 0, 0, 0);
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int f = f0 + lk + 4 * q;
      if (f < D && hc < H) {
        const size_t e = (size_t)f * H + hc;
        mlp_adam(a, e, (acc[q] + (f != D - 1 ? a.alpha * a.theta[e] : 0.0)) / m);
      }
    }
  } else {                                // [h | 1]^T dZ
    const int t2 = tile - tiles1;
    const int r0 = (t2 / CT) * 16, cls = (t2 % CT) * 16 + li, hr = r0 + li;
    for (int j = 0; j < rows; j += 4) {
      const int jj = j + lk;
      const bool on = jj < rows;
      const double av = on ? (hr < H ? a.h[(size_t)jj * H + hr] : (hr == H ? 1.0 : 0.0)) : 0.0;
      const double bv = (on && cls < K) ? a.dz[(size_t)jj * K + cls] : 0.0;
      acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, acc, 0, 0, 0);
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int r = r0 + lk + 4 * q;
      if (r <= H && cls < K) {
        const size_t e = (size_t)D * H + (size_t)r * K + cls;
        mlp_adam(a, e, (acc[q] + (r != H ? a.alpha * a.theta[e] : 0.0)) / m);
      }
    }
  }
}

// ============================================================================ loss, scores
// one workgroup: lanes stride over the blocks' sums and over the weights without their bias rows, then a fixed tree
__global__ __launch_bounds__(MLP_THREADS) void mlp_loss_fold_kernel(const double* lossp, int blocks,
                                                                     const double* theta, int D, int H, int K,
                                                                     const int* counts, double alpha, double* loss) {
  __shared__ double sh[MLP_THREADS];
  const int tid = threadIdx.x;
  const double* W2 = theta + (size_t)D * H;
  double s = 0.0, q = 0.0;
  for (int g = tid; g < blocks; g += MLP_THREADS) s += lossp[g];
  for (int e = tid; e < (D - 1) * H; e += MLP_THREADS) q += theta[e] * theta[e];
  for (int e = tid; e < H * K; e += MLP_THREADS) q += W2[e] * W2[e];
  sh[tid] = s + 0.5 * alpha * q;
  __syncthreads();
  for (int st = MLP_THREADS / 2; st > 0; st >>= 1) {
    if (tid < st) sh[tid] += sh[tid + st];
    __syncthreads();
  }
  if (tid == 0) {
    int nv = 0;
    for (int c = 0; c < K; ++c) nv += counts[c];
    loss[0] = sh[0] / (nv > 0 ? (double)nv : 1.0);
  }
}

__global__ __launch_bounds__(WAVE) void mlp_scores_kernel(const int* conf, int K, const double* loss,
                                                          const double* real, double* out) {
  __shared__ int tp[UTIL_MAX_CLASSES], rs[UTIL_MAX_CLASSES], cs[UTIL_MAX_CLASSES];
  const int tid = threadIdx.x;
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
  if (tid == 0) {
    confusion_scores(rs, cs, tp, K, real, out);
    out[6] = loss[0];
  }
}

// ============================================================================ launches
static void mlp_check_table(const UtilTable& t, int H, const char* what) {
  if (t.n < 1 || t.n_cont < 0 || t.n_cat < 0 || t.ldk < t.n || t.K < 1 || t.K > UTIL_MAX_CLASSES || t.D < 1 ||
      t.D > UTIL_MAX_FEATURES || t.D < t.n_cont + 2 * t.n_cat + 1 || H < 1 || H > MLP_MAX_HIDDEN)
    throw std::runtime_error(std::string(what) + ": table sizes");
}

void launch_mlp_step(const MlpStepArgs& a, hipStream_t stream) {
  require_unbatched("mlp_step");
  const UtilTable& t = a.t;
  mlp_check_table(t, a.H, "mlp_step");
  if (a.nb < 1 || a.nb > t.n || a.b < 0 || a.b >= a.nb) throw std::runtime_error("mlp_step: batch index");
  const int rows = mlp_batch_rows(t.n, a.b, a.nb);
  if (rows < 1 || rows > MLP_MAX_BATCH) throw std::runtime_error("mlp_step: rows of the batch");
  const int blocks = (rows + MLP_ROWS - 1) / MLP_ROWS;
  MlpFwdArgs f{};
  f.t = t;
  f.rows = MlpRows{a.b, a.nb, rows};
  f.theta = a.theta;
  f.H = a.H;
  f.counts = t.counts;
  f.h = a.h;
  f.dz = a.dz;
  f.dh = a.dh;
  f.cnt = a.cnt;
  hipLaunchKernelGGL(mlp_forward_kernel<MLP_STEP>, dim3((unsigned)blocks), dim3(MLP_THREADS), 0, stream, f);
  const int HT = (a.H + 15) / 16, CT = (t.K + 15) / 16;
  const int tiles1 = ((t.D + 15) / 16) * HT, tiles = tiles1 + ((a.H + 1 + 15) / 16) * CT;
  hipLaunchKernelGGL(mlp_grad_adam_kernel, dim3((unsigned)((tiles + MLP_WAVES - 1) / MLP_WAVES)), dim3(MLP_THREADS), 0,
                     stream, a, rows, blocks, tiles1, tiles);
}

void launch_mlp_loss(const UtilTable& t, const double* theta, int H, double alpha, double* loss, hipStream_t stream) {
  require_unbatched("mlp_loss");
  mlp_check_table(t, H, "mlp_loss");
  const int blocks = (t.n + MLP_ROWS - 1) / MLP_ROWS;
  MlpFwdArgs f{};
  f.t = t;
  f.rows = MlpRows{0, 1, t.n};
  f.theta = theta;
  f.H = H;
  f.counts = t.counts;
  f.lossp = loss + 1;
  hipLaunchKernelGGL(mlp_forward_kernel<MLP_LOSS>, dim3((unsigned)blocks), dim3(MLP_THREADS), 0, stream, f);
  hipLaunchKernelGGL(mlp_loss_fold_kernel, dim3(1), dim3(MLP_THREADS), 0, stream, loss + 1, blocks, theta, t.D, H, t.K,
                     t.counts, alpha, loss);
}

void launch_mlp_predict(const UtilTable& t, const int* train_counts, const double* theta, int H, int* conf,
                        const double* loss, const double* real, double* out, hipStream_t stream) {
  require_unbatched("mlp_predict");
  mlp_check_table(t, H, "mlp_predict");
  hipLaunchKernelGGL(mlp_zero_kernel, dim3((unsigned)((t.K * t.K + MLP_THREADS - 1) / MLP_THREADS)),
                     dim3(MLP_THREADS), 0, stream, conf, t.K * t.K);
  MlpFwdArgs f{};
  f.t = t;
  f.rows = MlpRows{0, 1, t.n};
  f.theta = theta;
  f.H = H;
  f.counts = train_counts;
  f.conf = conf;
  hipLaunchKernelGGL(mlp_forward_kernel<MLP_PREDICT>, dim3((unsigned)((t.n + MLP_ROWS - 1) / MLP_ROWS)),
                     dim3(MLP_THREADS), 0, stream, f);
  hipLaunchKernelGGL(mlp_scores_kernel, dim3(1), dim3(WAVE), 0, stream, conf, t.K, loss, real, out);
}

}  // namespace fedtgan
