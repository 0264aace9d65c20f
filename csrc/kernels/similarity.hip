// Similarity evaluator (eval/device.py DeviceSimilarity): Avg_JSD / Avg_WD of a decoded table, on the device.
//
//  sim_zero_kernel       the per-column integer counters of a pass
//  sim_prepare_kernel    one pass over the row-major decoded table: continuous columns become column-major fp64 key
//                        rows in the value space of the CSV (+inf where the CSV carries no number), categorical codes
//                        are counted (LDS histogram, then integer atomics)
//  sim_tile_sort_kernel  bitonic sort of SIM_SORT_TILE keys in LDS, grid = (tiles, columns)
//  sim_merge_kernel      one merge pass over runs of w keys: every workgroup produces one output tile of its pair of
//                        runs, found by a merge-path search; an unpaired run is a merge with an empty partner
//  sim_w1_kernel         W1 of the sorted real and fake keys after the real column's min-max scaling: every element
//                        owns the interval up to the next distinct point of the merged sequence, the other CDF comes
//                        from a binary search; per-workgroup partial sums in fixed slots
//  sim_w1_finish_kernel  the partials of a column summed in a fixed order
//  sim_jsd_kernel        base-2 Jensen-Shannon distance of the count vectors with eval/similarity.py column_jsd's quirks
//  sim_mean_kernel       [avg_jsd, avg_wd] from the per-column values
//
// Counts are integers (LDS and global integer atomics, ballots), and every fp64 sum runs over fixed slots in a fixed
// order: the scores of a table do not depend on the order in which workgroups or waves run.  No workgroup waits on
// another, nothing is allocated and the host reads nothing back, so a pass can be captured in a hipGraph.
#include "common.h"
#include "launch.h"

#include <math.h>
#include <stdexcept>

namespace fedtgan {

#if FT_CHECKED
__device__ unsigned g_check_sim = 0u;
unsigned check_status_similarity() {
  unsigned v = 0u, z = 0u;
  (void)hipMemcpyFromSymbol(&v, HIP_SYMBOL(g_check_sim), sizeof(v));
  (void)hipMemcpyToSymbol(HIP_SYMBOL(g_check_sim), &z, sizeof(z));
  return v;
}
#else
unsigned check_status_similarity() { return 0u; }
#endif

constexpr int SIM_THREADS = 256;
constexpr int SIM_HIST_MAX = 8192;   // ints of the prepare kernel's LDS histogram (32 KB); wider tables count in global memory
constexpr int SIM_T = SIM_SORT_TILE;
constexpr int SIM_PER = SIM_T / SIM_THREADS;   // merged outputs per thread
constexpr int W1_PER = 4;                       // elements per thread of the W1 pass
constexpr int W1_CHUNK = SIM_THREADS * W1_PER;

__device__ __forceinline__ double sim_inf() { return __longlong_as_double(0x7ff0000000000000ll); }

// fixed-order sum over the workgroup (every thread calls it; the result is valid in every thread)
__device__ __forceinline__ double block_sum(double v, double* red) {
  const int tid = threadIdx.x;
  __syncthreads();
  red[tid] = v;
  __syncthreads();
  for (int s = SIM_THREADS / 2; s > 0; s >>= 1) {
    if (tid < s) red[tid] += red[tid + s];
    __syncthreads();
  }
  return red[0];
}

// ============================================================================ prepare
__global__ __launch_bounds__(SIM_THREADS) void sim_zero_kernel(int* valid, int n_valid, int* counts, int n_counts) {
  const int i = blockIdx.x * SIM_THREADS + threadIdx.x;
  if (i < n_valid) valid[i] = 0;
  if (i < n_counts) counts[i] = 0;
}

// one row per thread; the column loop is uniform over the workgroup (kind / slot are per column)
__global__ __launch_bounds__(SIM_THREADS) void sim_prepare_kernel(SimPrepareArgs a, int lds_hist) {
  __shared__ int hist[SIM_HIST_MAX];
  const int tid = threadIdx.x, lane = tid & 63;
  const int nh = a.n_cat * a.ldc;
  if (lds_hist) {
    for (int i = tid; i < nh; i += SIM_THREADS) hist[i] = 0;
    __syncthreads();
  }
  const int r = blockIdx.x * SIM_THREADS + tid;
  const bool live = r < a.rows;
  const double* row = a.values + (size_t)(live ? r : 0) * a.n_cols;
  for (int c = 0; c < a.n_cols; ++c) {
    const int k = a.kind[c], s = a.slot[c];
    if (k == SIM_CAT) {
      if (s < 0 || s >= a.n_cat) continue;
      if (live) {
        const double v = row[c];
        const int V = min(a.vocab[s], a.ldc);
        const bool ok = v >= 0.0 && v < (double)V;     // (a NaN code fails both compares)
        FT_CHECK(&g_check_sim, ok, CHK_SIM_CODE);
        if (ok) {
          const int code = (int)v;
          if (lds_hist) atomicAdd(&hist[s * a.ldc + code], 1);
          else atomicAdd(&a.counts[(size_t)s * a.ldc + code], 1);
        }
      }
    } else {
      if (s < 0 || s >= a.n_cont) continue;
      double v = live ? row[c] : sim_inf();
      if (k == SIM_NONNEG) {          // data/decode.py nonneg_inverse; exactly -1 is a blank field in the CSV
        v = exp(v) - 1.0;
        if (v < 0.0) v = ceil(v);
        if (v == -1.0) v = sim_inf();
      }
      const bool fin = live && isfinite(v);
      if (!fin) v = sim_inf();
      if (live) a.keys[(size_t)s * a.ldk + r] = v;
      const int cnt = __popcll(__ballot(fin));
      if (lane == 0 && cnt) atomicAdd(&a.valid[s], cnt);
    }
  }
  if (lds_hist) {
    __syncthreads();
    for (int i = tid; i < nh; i += SIM_THREADS) {
      const int h = hist[i];
      if (h) atomicAdd(&a.counts[i], h);
    }
  }
}

void launch_sim_prepare(const SimPrepareArgs& a, hipStream_t stream) {
  require_unbatched("sim_prepare");
  if (a.rows < 0 || a.n_cols <= 0 || a.ldk < a.rows) throw std::runtime_error("sim_prepare: table / key row sizes");
  const int64_t nh = (int64_t)a.n_cat * a.ldc;
  if (nh >= (int64_t)INT32_MAX) throw std::runtime_error("sim_prepare: count table too large");
  const int nz = (int)(nh > a.n_cont ? nh : a.n_cont);
  if (nz > 0)
    hipLaunchKernelGGL(sim_zero_kernel, dim3((unsigned)((nz + SIM_THREADS - 1) / SIM_THREADS)), dim3(SIM_THREADS), 0,
                       stream, a.valid, a.n_cont, a.counts, (int)nh);
  if (a.rows == 0) return;
  hipLaunchKernelGGL(sim_prepare_kernel, dim3((unsigned)((a.rows + SIM_THREADS - 1) / SIM_THREADS)),
                     dim3(SIM_THREADS), 0, stream, a, (int)(nh <= SIM_HIST_MAX));
}

// ============================================================================ segmented sort
__global__ __launch_bounds__(SIM_THREADS) void sim_tile_sort_kernel(const double* src, double* dst, int64_t ld, int n) {
  __shared__ double s[SIM_T];
  const int tid = threadIdx.x;
  const int base = blockIdx.x * SIM_T;
  const int len = min(SIM_T, n - base);
  const double* in = src + (size_t)blockIdx.y * ld + base;
  for (int i = tid; i < SIM_T; i += SIM_THREADS) s[i] = i < len ? in[i] : sim_inf();
  __syncthreads();
  for (int k = 2; k <= SIM_T; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int t = tid; t < SIM_T / 2; t += SIM_THREADS) {
        const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1));
        const int l = i + j;
        const bool up = (i & k) == 0;
        const double x = s[i], y = s[l];
        if ((x > y) == up) {
          s[i] = y;
          s[l] = x;
        }
      }
      __syncthreads();
    }
  }
  double* out = dst + (size_t)blockIdx.y * ld + base;
  for (int i = tid; i < len; i += SIM_THREADS) out[i] = s[i];
}

// how many of the first d merged elements come from A (ties: A first)
__device__ __forceinline__ int merge_path(const double* A, int na, const double* B, int nb, int d) {
  int lo = max(0, d - nb), hi = min(d, na);
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (A[mid] <= B[d - 1 - mid]) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

__global__ __launch_bounds__(SIM_THREADS) void sim_merge_kernel(const double* src, double* dst, int64_t ld, int n,
                                                                long long w) {
  __shared__ double s[SIM_T];
  __shared__ double so[SIM_T];
  __shared__ int cut[2];
  const int tid = threadIdx.x;
  const long long o0 = (long long)blockIdx.x * SIM_T;       // first output element of this workgroup, < n
  const long long p0 = o0 / (2 * w) * (2 * w);              // first element of its pair of runs
  const int lenA = (int)min(w, (long long)n - p0);
  const int lenB = (int)max(0ll, min(w, (long long)n - p0 - w));
  const double* A = src + (size_t)blockIdx.y * ld + p0;
  const double* B = A + w;                                  // (read only where lenB > 0)
  const int d0 = (int)(o0 - p0);
  const int d1 = min(d0 + SIM_T, lenA + lenB);
  if (tid < 2) cut[tid] = merge_path(A, lenA, B, lenB, tid ? d1 : d0);
  __syncthreads();
  const int a0 = cut[0], a1 = cut[1];
  const int b0 = d0 - a0, b1 = d1 - a1;
  const int na = a1 - a0, nb = b1 - b0, cnt = d1 - d0;      // na + nb == cnt <= SIM_T
  for (int i = tid; i < na; i += SIM_THREADS) s[i] = A[a0 + i];
  for (int i = tid; i < nb; i += SIM_THREADS) s[na + i] = B[b0 + i];
  __syncthreads();
  const int dl = tid * SIM_PER;
  if (dl < cnt) {
    int i = merge_path(s, na, s + na, nb, dl);
    int j = dl - i;
    for (int e = 0; e < SIM_PER && dl + e < cnt; ++e) {
      const bool ta = j >= nb || (i < na && s[i] <= s[na + j]);
      so[dl + e] = ta ? s[i++] : s[na + j++];
    }
  }
  __syncthreads();
  double* out = dst + (size_t)blockIdx.y * ld + o0;
  for (int i = tid; i < cnt; i += SIM_THREADS) out[i] = so[i];
}

void launch_sim_sort(double* keys, double* tmp, int n_seg, int64_t ld, int n, hipStream_t stream) {
  require_unbatched("sim_sort");
  if (n_seg <= 0 || n <= 0) return;
  if (ld < n || n_seg > 65535) throw std::runtime_error("sim_sort: segment length / count");
  const int tiles = (n + SIM_T - 1) / SIM_T;
  int passes = 0;
  for (long long w = SIM_T; w < n; w <<= 1) ++passes;
  // an odd number of merge passes: the tiles go to tmp first, so the last pass lands in keys
  double* cur = (passes & 1) ? tmp : keys;
  double* oth = (passes & 1) ? keys : tmp;
  const dim3 grid((unsigned)tiles, (unsigned)n_seg);
  hipLaunchKernelGGL(sim_tile_sort_kernel, grid, dim3(SIM_THREADS), 0, stream, (const double*)keys, cur, ld, n);
  for (long long w = SIM_T; w < n; w <<= 1) {
    hipLaunchKernelGGL(sim_merge_kernel, grid, dim3(SIM_THREADS), 0, stream, (const double*)cur, oth, ld, n, w);
    double* t = cur;
    cur = oth;
    oth = t;
  }
}

// ============================================================================ W1
// first index in [0, n) with x[i] > v  (UPPER) / x[i] >= v
template <bool UPPER>
__device__ __forceinline__ int sim_bound(const double* x, int n, double v) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    const bool right = UPPER ? (x[mid] <= v) : (x[mid] < v);
    if (right) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// Element e of a column is real value e (e < nr) or fake value e - nr.  It owns the interval from its value to the
// next distinct point of the merged sequence.  Equal values: among reals / among fakes the last one owns it (the
// others see their successor at distance zero); a real and a fake that tie: the real one (the fake searches the
// reals with <, finds its equal and sees it at distance zero; the real searches the fakes with <=, past the tie).
__global__ __launch_bounds__(SIM_THREADS) void sim_w1_kernel(SimW1Args a, int chunks) {
  __shared__ double red[SIM_THREADS];
  const int c = blockIdx.y, tid = threadIdx.x;
  const int nr = min(max(a.n_real[c], 0), a.max_real), m = min(max(a.n_fake[c], 0), a.max_fake);
  const double* R = a.real + (size_t)c * a.ldr;
  const double* F = a.fake + (size_t)c * a.ldf;
  double acc = 0.0;
  if (nr > 0 && m > 0) {
    const double lo = R[0], hi = R[nr - 1];
    const double scale = hi > lo ? hi - lo : 1.0;
    const double dnr = (double)nr, dm = (double)m;
#pragma unroll
    for (int u = 0; u < W1_PER; ++u) {
      const long long e = (long long)blockIdx.x * W1_CHUNK + u * SIM_THREADS + tid;
      double x = 0.0, nxt = 0.0, cu = 0.0, cv = 0.0;
      bool has = false;
      if (e < nr) {
        const int i = (int)e;
        x = R[i];
        const int j = sim_bound<true>(F, m, x);
        if (i + 1 < nr) {
          nxt = R[i + 1];
          has = true;
        }
        if (j < m) {
          const double f = F[j];
          nxt = has ? fmin(nxt, f) : f;
          has = true;
        }
        cu = (double)(i + 1) / dnr;
        cv = (double)j / dm;
      } else if (e < (long long)nr + m) {
        const int j = (int)(e - nr);
        x = F[j];
        const int i = sim_bound<false>(R, nr, x);
        if (j + 1 < m) {
          nxt = F[j + 1];
          has = true;
        }
        if (i < nr) {
          const double rv = R[i];
          nxt = has ? fmin(nxt, rv) : rv;
          has = true;
        }
        cu = (double)i / dnr;
        cv = (double)(j + 1) / dm;
      }
      if (has) acc += fabs(cu - cv) * ((nxt - lo) / scale - (x - lo) / scale);
    }
  }
  const double sum = block_sum(acc, red);
  if (tid == 0) a.part[(size_t)c * chunks + blockIdx.x] = sum;
}

__global__ __launch_bounds__(SIM_THREADS) void sim_w1_finish_kernel(SimW1Args a, int chunks) {
  __shared__ double red[SIM_THREADS];
  const int c = blockIdx.x, tid = threadIdx.x;
  double acc = 0.0;
  for (int i = tid; i < chunks; i += SIM_THREADS) acc += a.part[(size_t)c * chunks + i];
  const double sum = block_sum(acc, red);
  // no real or no valid fake value: the CPU evaluator's 0 / 0
  if (tid == 0) a.out[c] = (a.n_real[c] > 0 && a.n_fake[c] > 0) ? sum : __longlong_as_double(0x7ff8000000000000ll);
}

int sim_w1_chunks(int64_t n) {
  const int64_t c = (n + W1_CHUNK - 1) / W1_CHUNK;
  return c > 0 ? (int)c : 1;
}

void launch_sim_w1(const SimW1Args& a, hipStream_t stream) {
  require_unbatched("sim_w1");
  if (a.n_cont <= 0) return;
  if (a.n_cont > 65535 || a.max_real < 0 || a.max_fake < 0 || a.ldr < a.max_real || a.ldf < a.max_fake)
    throw std::runtime_error("sim_w1: column count / row lengths");
  const int chunks = sim_w1_chunks((int64_t)a.max_real + a.max_fake);
  hipLaunchKernelGGL(sim_w1_kernel, dim3((unsigned)chunks, (unsigned)a.n_cont), dim3(SIM_THREADS), 0, stream, a, chunks);
  hipLaunchKernelGGL(sim_w1_finish_kernel, dim3((unsigned)a.n_cont), dim3(SIM_THREADS), 0, stream, a, chunks);
}

// ============================================================================ JSD
// eval/similarity.py column_jsd on count vectors: frequencies over the real categories (real count > 0); a real
// category the fake table misses enters both vectors twice; fake-only categories only enter the fake total; no real
// category in the fake column: 1.
__global__ __launch_bounds__(SIM_THREADS) void sim_jsd_kernel(SimJsdArgs a) {
  __shared__ double red[SIM_THREADS];
  __shared__ long long tot[2];
  const int c = blockIdx.x, tid = threadIdx.x;
  const int* rc = a.real + (size_t)c * a.ldc;
  const int* fc = a.fake + (size_t)c * a.ldc;
  if (tid < 2) {           // the two totals in integers (exact in any order; one thread each keeps it simple)
    const int* x = tid ? fc : rc;
    long long t = 0;
    for (int k = 0; k < a.ldc; ++k) t += x[k] > 0 ? x[k] : 0;
    tot[tid] = t;
  }
  __syncthreads();
  const double rs = (double)tot[0], fs = (double)tot[1];
  double sp = 0.0, sq = 0.0;
  for (int k = tid; k < a.ldc; k += SIM_THREADS) {
    const int r = rc[k], f = fc[k];
    if (r > 0) {
      const double rp = (double)r / rs;
      sp += rp;
      if (f > 0) sq += (double)f / fs;
      else sp += rp;
    }
  }
  sp = block_sum(sp, red);
  sq = block_sum(sq, red);
  if (!(sq > 0.0)) {
    if (tid == 0) a.out[c] = 1.0;
    return;
  }
  double kp = 0.0, kq = 0.0;
  for (int k = tid; k < a.ldc; k += SIM_THREADS) {
    const int r = rc[k], f = fc[k];
    if (r > 0) {
      const double p = ((double)r / rs) / sp;
      if (f > 0) {
        const double q = ((double)f / fs) / sq;
        const double mm = 0.5 * (p + q);
        kp += p * log(p / mm);
        kq += q * log(q / mm);
      } else {
        const double t = p * log(p / (0.5 * (p + 0.0)));
        kp += t;
        kp += t;
      }
    }
  }
  kp = block_sum(kp, red);
  kq = block_sum(kq, red);
  if (tid == 0) {
    const double js = 0.5 * (kp + kq) / log(2.0);
    a.out[c] = sqrt(js > 0.0 ? js : 0.0);
  }
}

void launch_sim_jsd(const SimJsdArgs& a, hipStream_t stream) {
  require_unbatched("sim_jsd");
  if (a.n_cat <= 0) return;
  if (a.ldc <= 0) throw std::runtime_error("sim_jsd: empty count rows");
  hipLaunchKernelGGL(sim_jsd_kernel, dim3((unsigned)a.n_cat), dim3(SIM_THREADS), 0, stream, a);
}

// ============================================================================ means
__global__ void sim_mean_kernel(double* scores, int n_cat, int n_cont) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const double nan = __longlong_as_double(0x7ff8000000000000ll);
  double sj = 0.0, sw = 0.0;
  for (int i = 0; i < n_cat; ++i) sj += scores[2 + i];
  for (int i = 0; i < n_cont; ++i) sw += scores[2 + n_cat + i];
  scores[0] = n_cat > 0 ? sj / (double)n_cat : nan;
  scores[1] = n_cont > 0 ? sw / (double)n_cont : nan;
}

void launch_sim_mean(double* scores, int n_cat, int n_cont, hipStream_t stream) {
  require_unbatched("sim_mean");
  hipLaunchKernelGGL(sim_mean_kernel, dim3(1), dim3(WAVE), 0, stream, scores, n_cat, n_cont);
}

}  // namespace fedtgan
