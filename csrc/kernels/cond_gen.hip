// Conditional generation (CTGANEngine.generate_decoded_where): rows with requested category values.
//
//  cond_request_kernel   after the generation sampler: every row's condition is replaced by the driving span
//                        and the option of a bin drawn in proportion to the bins' open quota
//  cond_flag_kernel      after the decode: which rows carry every requested value (exact f64 compares) and, per
//                        workgroup and bin, how many (LDS histogram)
//  cond_scatter_kernel   order-preserving ranks (rows of a bin kept before the pass + in earlier workgroups + earlier
//                        in this workgroup) and the copy of the ranked rows into their bin's quota segment
//  cond_finish_kernel    one workgroup: the bins' filled counters and the two statistics advance
//
// A request lives in device buffers (CondReq), so one captured pass serves every request of the same size.  No
// workgroup waits on another: the scatter reads the filled counters as they stood before the pass, and only the
// finish launch -- after it in stream order -- writes them.  Counting is in integers (LDS atomics on a histogram,
// ballots for the ranks), so the result does not depend on the order in which workgroups or waves run.
#include "common.h"
#include "launch.h"

#include <stdexcept>

namespace fedtgan {

#if FT_CHECKED
__device__ unsigned g_check_cond = 0u;
unsigned check_status_cond_gen() {
  unsigned v = 0u, z = 0u;
  (void)hipMemcpyFromSymbol(&v, HIP_SYMBOL(g_check_cond), sizeof(v));
  (void)hipMemcpyToSymbol(HIP_SYMBOL(g_check_cond), &z, sizeof(z));
  return v;
}
#else
unsigned check_status_cond_gen() { return 0u; }
#endif

constexpr int COND_THREADS = 256;                 // one row per thread
constexpr int COND_WAVES = COND_THREADS / WAVE;

// ============================================================================ request
// Row b draws r = floor(u * total) over the open quota (remaining_i = quota_i - filled_i, total their sum) and takes
// the first bin whose running sum exceeds r -- in integers, so a full bin (remaining 0) is never drawn.
__global__ __launch_bounds__(COND_THREADS) void cond_request_kernel(CondRequestArgs a) {
  __shared__ long long rem[COND_MAX_BINS];
  __shared__ long long total_s;
  const int tid = threadIdx.x;
  if (tid < a.req.n_bins) {
    const long long q = a.req.quota[tid] - a.req.filled[tid];
    rem[tid] = q > 0 ? q : 0;
  }
  __syncthreads();
  if (tid == 0) {
    long long t = 0;
    for (int i = 0; i < a.req.n_bins; ++i) t += rem[i];
    total_s = t;
  }
  __syncthreads();
  const int b = blockIdx.x * COND_THREADS + tid;
  if (b >= a.rows) return;
  const long long total = total_s;
  if (total <= 0) {          // every quota is full: no target, the sampler's condition stays
    a.tgt[b] = -1;
    return;
  }
  RngArgs rng{a.seed, a.rng_ctr, a.rng_stream};
  const uint64_t step = a.rng_ctr ? *a.rng_ctr : 0ull;
  const uint4 w = rng4(rng, step, (uint64_t)b);
  long long r = (long long)(u01d(w.x, w.y) * (double)total);
  if (r >= total) r = total - 1;
  int t = a.req.n_bins - 1;
  long long run = 0;
  for (int i = 0; i < a.req.n_bins; ++i) {
    run += rem[i];
    if (run > r) { t = i; break; }
  }
  const int span = a.req.drive[0];
  const int o = a.req.bin_opt[t];
  // the requested option's place in the conditional vector; a request that points outside it is flagged by the
  // checked build and, in every build, leaves the row without a target (nothing downstream gathers with it)
  const bool span_ok = span >= 0 && span < a.n_span && o >= 0 && o < a.cond_w[min(max(span, 0), a.n_span - 1)];
  FT_CHECK(&g_check_cond, span_ok, CHK_COND_REQUEST);
  if (!span_ok) {
    a.tgt[b] = -1;
    return;
  }
  if (a.h) {
    // fp32 activation buffer: the sampler wrote a one-hot block; move the row's hot element (two stores)
    const int co = a.col[b], oo = a.opt[b];
    const int was = (co >= 0 && co < a.n_span) ? a.cond_off[co] + oo : -1;
    const int now = a.cond_off[span] + o;
    FT_CHECK(&g_check_cond, was >= 0 && was < a.C && now >= 0 && now < a.C, CHK_COND_REQUEST);
    float* hrow = a.h + (size_t)b * a.ldh + a.cc;
    if (was >= 0 && was < a.C) hrow[was] = 0.f;
    if (now >= 0 && now < a.C) hrow[now] = 1.f;
  }
  a.col[b] = span;
  a.opt[b] = o;
  a.tgt[b] = t;
}

void launch_cond_request(const CondRequestArgs& a, hipStream_t stream) {
  require_unbatched("cond_request");
  if (a.req.n_bins < 1 || a.req.n_bins > COND_MAX_BINS) throw std::runtime_error("cond_request: 1..64 bins");
  if (a.rows <= 0) return;
  hipLaunchKernelGGL(cond_request_kernel, dim3((unsigned)((a.rows + COND_THREADS - 1) / COND_THREADS)),
                     dim3(COND_THREADS), 0, stream, a);
}

// ============================================================================ partition
// (1) keep[r] = the row's bin if it carries every requested value, else -1; counts[workgroup][bin]
__global__ __launch_bounds__(COND_THREADS) void cond_flag_kernel(CondPartitionArgs a) {
  __shared__ int hist[COND_MAX_BINS];
  const int tid = threadIdx.x;
  if (tid < COND_MAX_BINS) hist[tid] = 0;
  __syncthreads();
  const int r = blockIdx.x * COND_THREADS + tid;
  if (r < a.rows) {
    const int t = a.tgt[r];
    bool keep = t >= 0 && t < a.req.n_bins;
#if FT_CHECKED
    FT_CHECK(&g_check_cond, t >= -1 && t < a.req.n_bins, CHK_COND_REQUEST);
#endif
    if (keep && !a.any_value) {
      const double* row = a.out + (size_t)r * a.n_cols;
      const int dj = a.req.drive[1];
      keep = dj >= 0 && dj < a.n_cols && row[dj] == a.req.bin_code[t];
#if FT_CHECKED
      FT_CHECK(&g_check_cond, dj >= 0 && dj < a.n_cols, CHK_COND_REQUEST);
#endif
      for (int k = 0; keep && k < a.req.n_fixed; ++k) {
        const int j = a.req.fixed_j[k];
#if FT_CHECKED
        FT_CHECK(&g_check_cond, j >= 0 && j < a.n_cols, CHK_COND_REQUEST);
#endif
        keep = j >= 0 && j < a.n_cols && row[j] == a.req.fixed_code[k];
      }
    }
    a.keep[r] = keep ? t : -1;
    if (keep) atomicAdd(&hist[t], 1);
  }
  __syncthreads();
  if (tid < a.req.n_bins) a.counts[(size_t)blockIdx.x * a.req.n_bins + tid] = hist[tid];
}

// (2) ranks and the copy.  base[t] = filled[t] (before the pass) + the kept rows of bin t in earlier workgroups;
// inside the workgroup a wave ranks its rows bin by bin with ballots (as many rounds as the wave holds distinct
// bins), and the waves' per-bin counts, in wave order, rank the waves.  Rows then move with the whole workgroup
// striding over (row, column): reads of the decoded table are contiguous, writes contiguous per row.
__global__ __launch_bounds__(COND_THREADS) void cond_scatter_kernel(CondPartitionArgs a) {
  __shared__ long long base[COND_WAVES][COND_MAX_BINS];
  __shared__ int wcount[COND_WAVES][COND_MAX_BINS];
  __shared__ long long dest[COND_THREADS];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int nb = a.req.n_bins;
  // every wave sums a quarter of the earlier workgroups' counts, lane = bin
  long long s = 0;
  if (lane < nb)
    for (int w = wv; w < (int)blockIdx.x; w += COND_WAVES) s += a.counts[(size_t)w * nb + lane];
  base[wv][lane] = s;
  wcount[wv][lane] = 0;
  __syncthreads();
  const int r = blockIdx.x * COND_THREADS + tid;
  const int t = r < a.rows ? a.keep[r] : -1;
  int rank = 0;
  unsigned long long todo = __ballot(t >= 0);
  while (todo) {
    const int lead = __ffsll((long long)todo) - 1;
    const int tb = __shfl(t, lead, WAVE);
    const unsigned long long same = __ballot(t == tb);
    if (t == tb) rank = __popcll(same & ((1ull << lane) - 1ull));
    if (lane == lead) wcount[wv][tb] = __popcll(same);
    todo &= ~same;
  }
  __syncthreads();
  long long d = -1;
  if (t >= 0) {
    long long rk = a.req.filled[t] + rank;
    for (int w = 0; w < COND_WAVES; ++w) rk += base[w][t];
    for (int w = 0; w < wv; ++w) rk += wcount[w][t];
    if (rk < a.req.quota[t]) d = a.req.seg_off[t] + rk;
#if FT_CHECKED
    FT_CHECK(&g_check_cond, d < a.n_dst, CHK_COND_REQUEST);
#endif
    if (d >= a.n_dst) d = -1;      // (a request whose segments do not fit dst: never written)
  }
  dest[tid] = d;
  __syncthreads();
  const int row0 = blockIdx.x * COND_THREADS;
  const int nrow = min(COND_THREADS, a.rows - row0);
  const int nel = nrow * a.n_cols;
  // CP loads in flight per lane before their stores (a plain strided loop waits one memory round trip per
  // element: the compiler cannot move a load of `src` above a store to `dst`)
  const double* __restrict__ src = a.out + (size_t)row0 * a.n_cols;
  double* __restrict__ dst = a.dst;
  constexpr int CP = 8;
  for (int i0 = tid; i0 < nel; i0 += COND_THREADS * CP) {
    double v[CP];
#pragma unroll
    for (int u = 0; u < CP; ++u) v[u] = src[min(i0 + u * COND_THREADS, nel - 1)];
#pragma unroll
    for (int u = 0; u < CP; ++u) {
      const int i = i0 + u * COND_THREADS;
      if (i < nel) {
        const int lr = i / a.n_cols, c = i - lr * a.n_cols;
        const long long dr = dest[lr];
        if (dr >= 0) dst[(size_t)dr * a.n_cols + c] = v[u];
      }
    }
  }
}

// (3) filled[t] = min(quota[t], filled[t] + kept_t); statistics: rows generated, rows that passed the predicate
__global__ __launch_bounds__(COND_THREADS) void cond_finish_kernel(CondPartitionArgs a, int n_wg) {
  __shared__ long long part[COND_WAVES][COND_MAX_BINS];
  __shared__ long long kept[COND_MAX_BINS];
  const int t = threadIdx.x & 63, wv = threadIdx.x >> 6;
  long long s = 0;                 // lane = bin; every wave sums a quarter of the workgroups' counts
  if (t < a.req.n_bins)
    for (int w = wv; w < n_wg; w += COND_WAVES) s += a.counts[(size_t)w * a.req.n_bins + t];
  part[wv][t] = s;
  __syncthreads();
  if (wv == 0) {
    long long k = 0;
    for (int w = 0; w < COND_WAVES; ++w) k += part[w][t];
    if (t < a.req.n_bins) {
      const long long q = a.req.quota[t], f = a.req.filled[t] + k;
      a.req.filled[t] = f < q ? f : q;
    }
    kept[t] = k;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    long long all = 0;
    for (int i = 0; i < a.req.n_bins; ++i) all += kept[i];
    a.req.stats[0] += (long long)a.rows;
    a.req.stats[1] += all;
  }
}

void launch_cond_partition(const CondPartitionArgs& a, hipStream_t stream) {
  require_unbatched("cond_partition");
  if (a.req.n_bins < 1 || a.req.n_bins > COND_MAX_BINS) throw std::runtime_error("cond_partition: 1..64 bins");
  if (a.rows <= 0) return;
  const int n_wg = (a.rows + COND_THREADS - 1) / COND_THREADS;
  hipLaunchKernelGGL(cond_flag_kernel, dim3((unsigned)n_wg), dim3(COND_THREADS), 0, stream, a);
  hipLaunchKernelGGL(cond_scatter_kernel, dim3((unsigned)n_wg), dim3(COND_THREADS), 0, stream, a);
  hipLaunchKernelGGL(cond_finish_kernel, dim3(1), dim3(COND_THREADS), 0, stream, a, n_wg);
}

int cond_partition_workgroups(int rows) { return (rows + COND_THREADS - 1) / COND_THREADS; }

}  // namespace fedtgan
