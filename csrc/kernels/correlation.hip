// Correlation evaluator (eval/correlation.py DeviceCorrelation): the pairwise association matrix of a decoded table
// (Pearson r between continuous columns, Theil's U between categorical ones, the correlation ratio between the two
// kinds) and its distance to the real table's matrix, on the device.
//
//  corr_pack_kernel      one pass over the row-major table: continuous columns into a dense [n, n_cont] fp64 buffer,
//                        codes into int32 [n_cat, ld] rows with anything that is no code of [0, K) in the overflow bin K
//  corr_colsum_kernel    per-chunk column sums; corr_mean_kernel folds them in chunk order into the means
//  corr_moments_kernel   G = F^T Xc per row group with F = [Xc | one-hot(codes)], through the fp64 MFMA; the one-hot
//                        operand is made from the codes in registers
//  corr_reduce_kernel    G = the row groups' partials, in group order
//  corr_counts_kernel    contingency tables of the categorical pairs and the columns' margins: LDS histograms with
//                        integer LDS atomics per (pair, row group), merged into the global int32 tables with vector
//                        atomics; a table of more than CORR_LDS_BINS bins counts in global memory directly
//  corr_matrix_kernel    one wave per entry of A: lanes stride over a table's bins, the wave folds them in a fixed tree
//  corr_diff_kernel      Frobenius distance, mean and maximum absolute off-diagonal difference of two matrices
//
// Integer adds commute and every fp64 sum has an order fixed by the shapes alone, so a table scores bit-identically
// on every run.  Codes are clamped before they index anything.
#include "common.h"
#include "eval_common.h"
#include "launch.h"

#include <math.h>
#include <stdexcept>

namespace fedtgan {

constexpr int CORR_THREADS = 256;
constexpr int CORR_WAVES = CORR_THREADS / WAVE;

int64_t g_corr_part_target = CORR_PART_TARGET;

static int64_t corr_chunks(int64_t n) {
  const int64_t chunks = (n + CORR_CHUNK - 1) / CORR_CHUNK;
  return chunks > 1 ? chunks : 1;
}

// the most row groups a table of up to n rows is split into: one per chunk, capped so that the groups' partials
// [groups, W, n_cont] stay within g_corr_part_target doubles.  corr_groups and corr_part_doubles both start here.
static int64_t corr_group_cap(int64_t n, int64_t W, int64_t n_cont) {
  const int64_t chunks = corr_chunks(n);
  const int64_t cells = W * n_cont > 0 ? W * n_cont : 1;
  int64_t cap = g_corr_part_target / cells;
  if (cap < 1) cap = 1;
  return chunks < cap ? chunks : cap;
}

CorrGroups corr_groups(int64_t n, int64_t W, int64_t n_cont) {
  const int64_t chunks = corr_chunks(n);
  const int64_t g0 = corr_group_cap(n, W, n_cont);
  const int64_t per = (chunks + g0 - 1) / g0;         // chunks per group: the groups are equal but for the last
  CorrGroups g;
  g.groups = (int)((chunks + per - 1) / per);          // <= g0
  g.rows = (int)(per * CORR_CHUNK);
  return g;
}

int64_t corr_part_doubles(int64_t n_max, int64_t W, int64_t n_cont) {
  // corr_moments: any n <= n_max uses at most corr_group_cap(n_max) groups; corr_pack: one sum per chunk and column
  const int64_t a = corr_group_cap(n_max, W, n_cont) * W * n_cont, b = corr_chunks(n_max) * n_cont;
  const int64_t m = a > b ? a : b;
  return m > 0 ? m : 1;
}

// ============================================================================ pack
__global__ __launch_bounds__(CORR_THREADS) void corr_pack_kernel(CorrPackArgs a) {
  const long long i = (long long)blockIdx.x * CORR_THREADS + threadIdx.x;
  if (i >= (long long)a.rows * a.n_cols) return;
  const long long r = i / a.n_cols;
  const int c = (int)(i - r * a.n_cols);
  const int k = a.kind[c], s = a.slot[c];
  const double v = a.values[i];
  if (k == CORR_CAT) {
    if (s >= 0 && s < a.n_cat) {
      a.cat_t[(size_t)s * a.ldk + r] = code_or_overflow(v, a.card[s]);
    }
  } else if (s >= 0 && s < a.n_cont) {
    a.cont[r * a.n_cont + s] = v;
  }
}

// grid (column blocks, chunks); thread = (row slice s of 4, column j of 64): rows r0 + s, r0 + s + 4, ... in order,
// then the four slices in order
__global__ __launch_bounds__(CORR_THREADS) void corr_colsum_kernel(const double* cont, int n, int n_cont,
                                                                    double* part) {
  __shared__ double sh[CORR_WAVES][CORR_COL_TILE];
  const int lane = threadIdx.x & 63, s = threadIdx.x >> 6;
  const int col = blockIdx.x * CORR_COL_TILE + lane;
  const int r0 = blockIdx.y * CORR_CHUNK, r1 = min(n, r0 + CORR_CHUNK);
  double acc = 0.0;
  if (col < n_cont)
    for (int r = r0 + s; r < r1; r += CORR_WAVES) acc += cont[(size_t)r * n_cont + col];
  sh[s][lane] = acc;
  __syncthreads();
  if (s == 0 && col < n_cont) part[(size_t)blockIdx.y * n_cont + col] = ((sh[0][lane] + sh[1][lane]) + sh[2][lane]) + sh[3][lane];
}

__global__ __launch_bounds__(CORR_THREADS) void corr_mean_kernel(const double* part, int chunks, int n, int n_cont,
                                                                  double* mean) {
  const int col = blockIdx.x * CORR_THREADS + threadIdx.x;
  if (col >= n_cont) return;
  double acc = 0.0;
  for (int c = 0; c < chunks; ++c) acc += part[(size_t)c * n_cont + col];
  mean[col] = acc / (double)n;
}

void launch_corr_pack(const CorrPackArgs& a, hipStream_t stream) {
  require_unbatched("corr_pack");
  if (a.rows < 1 || a.n_cols <= 0 || a.n_cont < 0 || a.n_cat < 0 || a.ldk < a.rows)
    throw std::runtime_error("corr_pack: table sizes");
  const long long cells = (long long)a.rows * a.n_cols;
  if (cells >= (long long)INT32_MAX * CORR_THREADS) throw std::runtime_error("corr_pack: table too large");
  hipLaunchKernelGGL(corr_pack_kernel, dim3((unsigned)((cells + CORR_THREADS - 1) / CORR_THREADS)), dim3(CORR_THREADS),
                     0, stream, a);
  if (a.n_cont == 0) return;
  const int chunks = (a.rows + CORR_CHUNK - 1) / CORR_CHUNK;
  if (chunks > 65535) throw std::runtime_error("corr_pack: too many rows");
  const unsigned jb = (unsigned)((a.n_cont + CORR_COL_TILE - 1) / CORR_COL_TILE);
  hipLaunchKernelGGL(corr_colsum_kernel, dim3(jb, (unsigned)chunks), dim3(CORR_THREADS), 0, stream, a.cont, a.rows,
                     a.n_cont, a.part);
  hipLaunchKernelGGL(corr_mean_kernel, dim3((unsigned)((a.n_cont + CORR_THREADS - 1) / CORR_THREADS)),
                     dim3(CORR_THREADS), 0, stream, a.part, chunks, a.rows, a.n_cont, a.mean);
}

// ============================================================================ moments
// part[g] = F^T Xc over the rows of group g, all of it one fp64 MFMA product.  v_mfma_f64_16x16x4_f64: lane l feeds
// A[i = l & 15][k = l >> 4] and B[k = l >> 4][j = l & 15], one fp64 each, and holds D[(l >> 4) + 4 reg][l & 15] in
// reg = 0..3.  With k a table row, the B operand and the continuous rows of A are four rows of 16 consecutive columns
// of the row-major table, read from global memory directly and centred in registers; a one-hot row of A is made from
// the codes on the fly (1.0 where the row's code is the lane's bin) and never exists in memory.  A wave owns a 32 x 32
// tile of G as 2 x 2 MFMA tiles; the four waves of a workgroup take the group's row quads round-robin and their
// tiles are added in wave order through LDS.  grid (tiles of 32 columns of G, tiles of 32 rows of G, groups).
typedef double corr_d4 __attribute__((ext_vector_type(4)));
constexpr int CORR_MFMA_TILE = 32;

__global__ __launch_bounds__(CORR_THREADS) void corr_moments_kernel(CorrMomentsArgs a, int rows_per_group) {
  __shared__ double red[CORR_WAVES][CORR_MFMA_TILE][CORR_MFMA_TILE + 1];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, li = lane & 15, lk = lane >> 4;
  const int j0 = blockIdx.x * CORR_MFMA_TILE, i0 = blockIdx.y * CORR_MFMA_TILE, g = blockIdx.z;
  const int r0 = g * rows_per_group, r1 = min(a.n, r0 + rows_per_group);
  int col[4];       // the lane's two rows of G (t = 0, 1) and two columns of G (t = 2, 3)
  bool ok[4];
  double m[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    col[t] = (t < 2 ? i0 : j0) + (t & 1) * 16 + li;
    ok[t] = col[t] < a.n_cont;
    m[t] = ok[t] ? a.mean[col[t]] : 0.0;
  }
  // rows of G past the continuous block: (categorical column, bin) of one-hot row col[t] - n_cont; offs is ascending
  int hcol[2], hbin[2], hcard[2];
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    hcol[t] = -1;
    hbin[t] = hcard[t] = 0;
    const int wv = col[t] - a.n_cont;
    if (wv >= 0 && col[t] < a.W && a.n_cat > 0) {
      int lo = 0, hi = a.n_cat - 1;
      while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (a.offs[mid] <= wv) lo = mid; else hi = mid - 1;
      }
      const int k = wv - a.offs[lo], K = a.card[lo];
      if (k >= 0 && k <= K) {
        hcol[t] = lo;
        hbin[t] = k;
        hcard[t] = K;
      }
    }
  }
  corr_d4 acc[2][2];
#pragma unroll
  for (int u = 0; u < 2; ++u)
#pragma unroll
    for (int v = 0; v < 2; ++v) acc[u][v] = (corr_d4){0.0, 0.0, 0.0, 0.0};
  for (int r = r0 + 4 * w; r < r1; r += 4 * CORR_WAVES) {      // (uniform over the wave: every lane reaches the MFMA)
    const int row = r + lk;
    const bool live = row < r1;
    double x[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) x[t] = (live && ok[t]) ? a.cont[(size_t)row * a.n_cont + col[t]] - m[t] : 0.0;
#pragma unroll
    for (int t = 0; t < 2; ++t)
      if (live && hcol[t] >= 0)
        x[t] = code_clamp(a.cat_t[(size_t)hcol[t] * a.ldk + row], hcard[t]) == hbin[t] ? 1.0 : 0.0;
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
      for (int v = 0; v < 2; ++v) acc[u][v] = __builtin_amdgcn_mfma_f64_16x16x4f64(x[u], x[2 + v], acc[u][v], 0, 0, 0);
  }
#pragma unroll
  for (int u = 0; u < 2; ++u)
#pragma unroll
    for (int v = 0; v < 2; ++v)
#pragma unroll
      for (int q = 0; q < 4; ++q) red[w][u * 16 + lk + 4 * q][v * 16 + li] = acc[u][v][q];
  __syncthreads();
  double* out = a.part + (size_t)g * a.W * a.n_cont;
  for (int e = tid; e < CORR_MFMA_TILE * CORR_MFMA_TILE; e += CORR_THREADS) {
    const int ii = e / CORR_MFMA_TILE, jj = e - ii * CORR_MFMA_TILE;
    const int i = i0 + ii, j = j0 + jj;
    if (i < a.W && j < a.n_cont)
      out[(size_t)i * a.n_cont + j] = ((red[0][ii][jj] + red[1][ii][jj]) + red[2][ii][jj]) + red[3][ii][jj];
  }
}

__global__ __launch_bounds__(CORR_THREADS) void corr_reduce_kernel(const double* part, int groups, long long cells,
                                                                    double* G) {
  const long long e = (long long)blockIdx.x * CORR_THREADS + threadIdx.x;
  if (e >= cells) return;
  double acc = 0.0;
  for (int g = 0; g < groups; ++g) acc += part[(size_t)g * cells + e];
  G[e] = acc;
}

void launch_corr_moments(const CorrMomentsArgs& a, hipStream_t stream) {
  require_unbatched("corr_moments");
  if (a.n < 1 || a.n_cont < 0 || a.n_cat < 0 || a.W < a.n_cont || a.ldk < a.n)
    throw std::runtime_error("corr_moments: table sizes");
  if (a.n_cont == 0) return;
  const CorrGroups gr = corr_groups(a.n, a.W, a.n_cont);
  const unsigned jt = (unsigned)((a.n_cont + CORR_MFMA_TILE - 1) / CORR_MFMA_TILE);
  const unsigned it = (unsigned)((a.W + CORR_MFMA_TILE - 1) / CORR_MFMA_TILE);
  if (gr.groups > 65535 || it > 65535) throw std::runtime_error("corr_moments: too many rows or one-hot rows");
  hipLaunchKernelGGL(corr_moments_kernel, dim3(jt, it, (unsigned)gr.groups), dim3(CORR_THREADS), 0, stream, a, gr.rows);
  const long long cells = (long long)a.W * a.n_cont;
  hipLaunchKernelGGL(corr_reduce_kernel, dim3((unsigned)((cells + CORR_THREADS - 1) / CORR_THREADS)),
                     dim3(CORR_THREADS), 0, stream, a.part, gr.groups, cells, a.G);
}

// ============================================================================ contingency tables
__global__ __launch_bounds__(CORR_THREADS) void corr_zero_kernel(int* p, long long n) {
  const long long i = (long long)blockIdx.x * CORR_THREADS + threadIdx.x;
  if (i < n) p[i] = 0;
}

// grid (pairs, row groups of CORR_COUNT_ROWS).  A pair's description is validated before anything is indexed with it.
__global__ __launch_bounds__(CORR_THREADS) void corr_counts_kernel(CorrCountsArgs a) {
  extern __shared__ int hist[];
  const int p = blockIdx.x, tid = threadIdx.x;
  const int ca = a.pairs[4 * p], cb = a.pairs[4 * p + 1], ka = a.pairs[4 * p + 2], kb = a.pairs[4 * p + 3];
  const long long off = a.poff[p];
  const long long bins = (long long)ka * kb;
  if (ca < 0 || ca >= a.n_cat || cb >= a.n_cat || ka < 1 || kb < 1 || (cb < 0 && kb != 1) || off < 0 ||
      off + bins > a.total)
    return;
  const int r0 = blockIdx.y * CORR_COUNT_ROWS, r1 = min(a.n, r0 + CORR_COUNT_ROWS);
  const int* pa = a.cat_t + (size_t)ca * a.ldk;
  const int* pb = cb >= 0 ? a.cat_t + (size_t)cb * a.ldk : nullptr;
  int* table = a.counts + off;
  if (bins <= (long long)a.lds_bins) {
    const int nb = (int)bins;
    for (int i = tid; i < nb; i += CORR_THREADS) hist[i] = 0;
    __syncthreads();
    for (int r = r0 + tid; r < r1; r += CORR_THREADS) {
      const int x = code_clamp(pa[r], ka - 1);
      const int y = pb ? code_clamp(pb[r], kb - 1) : 0;
      atomicAdd(&hist[x * kb + y], 1);
    }
    __syncthreads();
    for (int i = tid; i < nb; i += CORR_THREADS) {
      const int h = hist[i];
      if (h) atomicAdd(&table[i], h);
    }
  } else {
    for (int r = r0 + tid; r < r1; r += CORR_THREADS) {
      const int x = code_clamp(pa[r], ka - 1);
      const int y = pb ? code_clamp(pb[r], kb - 1) : 0;
      atomicAdd(&table[(long long)x * kb + y], 1);
    }
  }
}

void launch_corr_counts(const CorrCountsArgs& a, hipStream_t stream) {
  require_unbatched("corr_counts");
  if (a.n < 1 || a.n_cat < 0 || a.n_pairs < 0 || a.total < 0 || a.ldk < a.n || a.lds_bins < 1 ||
      a.lds_bins > CORR_LDS_BINS)
    throw std::runtime_error("corr_counts: table sizes");
  if (a.total > 0) {
    if (a.total >= (long long)INT32_MAX * CORR_THREADS) throw std::runtime_error("corr_counts: tables too large");
    hipLaunchKernelGGL(corr_zero_kernel, dim3((unsigned)((a.total + CORR_THREADS - 1) / CORR_THREADS)),
                       dim3(CORR_THREADS), 0, stream, a.counts, (long long)a.total);
  }
  if (a.n_pairs == 0) return;
  const int rg = (a.n + CORR_COUNT_ROWS - 1) / CORR_COUNT_ROWS;
  if (rg > 65535) throw std::runtime_error("corr_counts: too many rows");
  hipLaunchKernelGGL(corr_counts_kernel, dim3((unsigned)a.n_pairs, (unsigned)rg), dim3(CORR_THREADS),
                     (size_t)a.lds_bins * sizeof(int), stream, a);
}

// ============================================================================ the matrix
// one wave per entry (i, j) of A.  The pair tables follow the n_cat margins in row-major order of a < b.
__global__ __launch_bounds__(WAVE) void corr_matrix_kernel(CorrMatrixArgs a) {
  const int i = blockIdx.x / a.C, j = blockIdx.x - i * a.C;
  const int lane = threadIdx.x;
  double* out = a.A + (size_t)i * a.C + j;
  if (i == j) {
    if (lane == 0) *out = 1.0;
    return;
  }
  const int ki = a.kind[i], kj = a.kind[j], si = a.slot[i], sj = a.slot[j];
  const double n = (double)a.n;
  double res = 0.0;
  if (ki == CORR_CONT && kj == CORR_CONT) {
    if (si < 0 || si >= a.n_cont || sj < 0 || sj >= a.n_cont) return;
    const double sxx = a.G[(size_t)si * a.n_cont + si], syy = a.G[(size_t)sj * a.n_cont + sj];
    if (sxx > 0.0 && syy > 0.0) {
      const double r = a.G[(size_t)si * a.n_cont + sj] / sqrt(sxx * syy);
      res = fmin(1.0, fmax(-1.0, r));
    }
  } else if (ki == CORR_CAT && kj == CORR_CAT) {
    if (si < 0 || si >= a.n_cat || sj < 0 || sj >= a.n_cat) return;
    const int lo = min(si, sj), hi = max(si, sj);
    const long long p = (long long)a.n_cat + (long long)lo * a.n_cat - (long long)lo * (lo + 1) / 2 + (hi - lo - 1);
    const int klo = a.card[lo] + 1, khi = a.card[hi] + 1;
    if (p >= a.n_pairs) return;
    const long long off = a.poff[p], oi = a.poff[si], oj = a.poff[sj];
    if (off < 0 || off + (long long)klo * khi > a.total || oi < 0 || oi + a.card[si] + 1 > a.total || oj < 0 ||
        oj + a.card[sj] + 1 > a.total)
      return;
    const int* mi = a.counts + oi;
    const int* mj = a.counts + oj;
    const int* t = a.counts + off;
    double hi_ = 0.0;                                // H(i)
    for (int k = lane; k <= a.card[si]; k += WAVE) {
      const int c = mi[k];
      if (c > 0) {
        const double pk = (double)c / n;
        hi_ -= pk * log(pk);
      }
    }
    hi_ = wave_sum_d(hi_);
    double hc = 0.0;                                 // H(i | j)
    const int nb = klo * khi;
    for (int e = lane; e < nb; e += WAVE) {
      const int c = t[e];
      if (c > 0) {
        const int l = (sj == hi) ? e % khi : e / khi;
        hc += ((double)c / n) * log((double)mj[l] / (double)c);
      }
    }
    hc = wave_sum_d(hc);
    res = hi_ > 0.0 ? fmin(1.0, fmax(0.0, (hi_ - hc) / hi_)) : 1.0;
  } else {
    const int sc = ki == CORR_CAT ? si : sj, sx = ki == CORR_CAT ? sj : si;
    if (sc < 0 || sc >= a.n_cat || sx < 0 || sx >= a.n_cont) return;
    const long long om = a.poff[sc];
    const int K = a.card[sc];
    if (om < 0 || om + K + 1 > a.total || K < 0 || a.offs[sc] < 0 || a.n_cont + a.offs[sc] + K + 1 > a.W) return;
    const int* mk = a.counts + om;
    const double* S = a.G + ((size_t)a.n_cont + a.offs[sc]) * a.n_cont + sx;
    double acc = 0.0;
    for (int k = lane; k <= K; k += WAVE) {
      const int c = mk[k];
      if (c > 0) {
        const double s = S[(size_t)k * a.n_cont];
        acc += s * s / (double)c;
      }
    }
    acc = wave_sum_d(acc);
    const double sxx = a.G[(size_t)sx * a.n_cont + sx];
    if (sxx > 0.0) res = fmin(1.0, fmax(0.0, sqrt(acc / sxx)));
  }
  if (lane == 0) *out = res;
}

void launch_corr_matrix(const CorrMatrixArgs& a, hipStream_t stream) {
  require_unbatched("corr_matrix");
  if (a.n < 1 || a.C < 1 || a.n_cont < 0 || a.n_cat < 0 || a.n_cont + a.n_cat != a.C || a.C > 46340 ||
      a.n_pairs < a.n_cat || a.W < a.n_cont)
    throw std::runtime_error("corr_matrix: table sizes");
  hipLaunchKernelGGL(corr_matrix_kernel, dim3((unsigned)(a.C * a.C)), dim3(WAVE), 0, stream, a);
}

// ============================================================================ the scores
__global__ __launch_bounds__(CORR_THREADS) void corr_diff_kernel(const double* A, const double* B, int C, double* out) {
  __shared__ double s2[CORR_THREADS], s1[CORR_THREADS], sm[CORR_THREADS];
  const int tid = threadIdx.x;
  const long long cells = (long long)C * C;
  double q = 0.0, l = 0.0, m = 0.0;
  for (long long e = tid; e < cells; e += CORR_THREADS) {
    const double d = fabs(A[e] - B[e]);
    q += d * d;
    if (e / C != e % C) {
      l += d;
      m = fmax(m, d);
    }
  }
  s2[tid] = q;
  s1[tid] = l;
  sm[tid] = m;
  __syncthreads();
  for (int s = CORR_THREADS / 2; s > 0; s >>= 1) {
    if (tid < s) {
      s2[tid] += s2[tid + s];
      s1[tid] += s1[tid + s];
      sm[tid] = fmax(sm[tid], sm[tid + s]);
    }
    __syncthreads();
  }
  if (tid == 0) {
    out[0] = sqrt(s2[0]);
    out[1] = C > 1 ? s1[0] / ((double)C * (double)(C - 1)) : 0.0;
    out[2] = sm[0];
  }
}

void launch_corr_diff(const double* A, const double* B, int C, double* out, hipStream_t stream) {
  require_unbatched("corr_diff");
  if (C < 1 || C > 46340) throw std::runtime_error("corr_diff: matrix size");
  hipLaunchKernelGGL(corr_diff_kernel, dim3(1), dim3(CORR_THREADS), 0, stream, A, B, C, out);
}

}  // namespace fedtgan
