// Range and set predicates of a conditional request (CTGANEngine.generate_decoded_where / _guarded).
//
//  pred_request_kernel   after the generation sampler, when a predicate drives: every row's condition becomes the
//                        driving span and one of its options, drawn by weight (a bisection of the cumulative
//                        weights in global memory: M doubles, L2-resident, M bounded by the span width alone)
//  pred_mark_kernel      after the decode: a row that has a target is tested against the predicates in request order
//                        (exact f64 compares); the first one that fails clears the target, and the counters advance
//
// Counting is in integers: an LDS histogram per workgroup, then one vector atomic per counter and workgroup, so the
// counters do not depend on the order in which workgroups run.
#include "common.h"
#include "launch.h"

#include <stdexcept>

namespace fedtgan {

#if FT_CHECKED
__device__ unsigned g_check_pred = 0u;
unsigned check_status_cond_pred() {
  unsigned v = 0u, z = 0u;
  (void)hipMemcpyFromSymbol(&v, HIP_SYMBOL(g_check_pred), sizeof(v));
  (void)hipMemcpyToSymbol(HIP_SYMBOL(g_check_pred), &z, sizeof(z));
  return v;
}
#else
unsigned check_status_cond_pred() { return 0u; }
#endif

constexpr int PRED_THREADS = 256;                 // one row per thread

// ============================================================================ request
// Row b draws u (the words and the double of cond_request_kernel) and takes option k = #{i : drv_cum[i] <= u},
// clamped to M - 1 (u01d can round to exactly 1.0).  Only options with positive weight are in the table.
__global__ __launch_bounds__(PRED_THREADS) void pred_request_kernel(PredRequestArgs a) {
  const int b = blockIdx.x * PRED_THREADS + threadIdx.x;
  if (b >= a.rows) return;
  if (a.quota[0] - a.filled[0] <= 0) {          // the quota is full: no target, the sampler's condition stays
    a.tgt[b] = -1;
    return;
  }
  RngArgs rng{a.seed, a.rng_ctr, a.rng_stream};
  const uint64_t step = a.rng_ctr ? *a.rng_ctr : 0ull;
  const uint4 w = rng4(rng, step, (uint64_t)b);
  const double u = u01d(w.x, w.y);
  int lo = 0, hi = a.M;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (a.drv_cum[mid] <= u) lo = mid + 1; else hi = mid;
  }
  const int k = min(lo, a.M - 1);
  const int span = a.drv[0];
  const int o = a.drv_opt[k];
  // as cond_request_kernel: a driver that points outside the span tables is flagged by the checked build and, in
  // every build, leaves the row without a target
  const bool span_ok = span >= 0 && span < a.n_span && o >= 0 && o < a.cond_w[min(max(span, 0), a.n_span - 1)];
  FT_CHECK(&g_check_pred, span_ok, CHK_COND_REQUEST);
  if (!span_ok) {
    a.tgt[b] = -1;
    return;
  }
  if (a.h) {
    // fp32 activation buffer: the sampler wrote a one-hot block; move the row's hot element (two stores)
    const int co = a.col[b], oo = a.opt[b];
    const int was = (co >= 0 && co < a.n_span) ? a.cond_off[co] + oo : -1;
    const int now = a.cond_off[span] + o;
    FT_CHECK(&g_check_pred, was >= 0 && was < a.C && now >= 0 && now < a.C, CHK_COND_REQUEST);
    float* hrow = a.h + (size_t)b * a.ldh + a.cc;
    if (was >= 0 && was < a.C) hrow[was] = 0.f;
    if (now >= 0 && now < a.C) hrow[now] = 1.f;
  }
  a.col[b] = span;
  a.opt[b] = o;
  a.tgt[b] = 0;
}

void launch_pred_request(const PredRequestArgs& a, hipStream_t stream) {
  require_unbatched("pred_request");
  if (a.M < 1) throw std::runtime_error("pred_request: an empty driver table");
  if (a.rows <= 0) return;
  hipLaunchKernelGGL(pred_request_kernel, dim3((unsigned)((a.rows + PRED_THREADS - 1) / PRED_THREADS)),
                     dim3(PRED_THREADS), 0, stream, a);
}

// ============================================================================ mark
__global__ __launch_bounds__(PRED_THREADS) void pred_mark_kernel(PredMarkArgs a) {
  __shared__ int hist[2 + PRED_MAX];
  const int tid = threadIdx.x;
  if (tid < 2 + PRED_MAX) hist[tid] = 0;
  __syncthreads();
  const int r = blockIdx.x * PRED_THREADS + tid;
  if (r < a.rows && a.tgt[r] >= 0) {
    const double* row = a.out + (size_t)r * a.n_cols;
    int fail = -1;
    for (int k = 0; k < a.p.n_pred && fail < 0; ++k) {
      const int j = a.p.j[k];
      // a column or a table slice outside its buffer: flagged by the checked build; in every build the predicate
      // fails and nothing is read
      const bool j_ok = j >= 0 && j < a.n_cols;
      FT_CHECK(&g_check_pred, j_ok, CHK_COND_REQUEST);
      bool pass = false;
      if (j_ok) {
        const double v = row[j];
        if (a.p.kind[k] == 0) {
          pass = v >= a.p.lo[k] && v <= a.p.hi[k];
        } else {
          const int off = a.p.lut_off[k], len = a.p.lut_len[k];
          const bool lut_ok = off >= 0 && len >= 0 && (long long)off + len <= (long long)a.p.lut_total;
          FT_CHECK(&g_check_pred, lut_ok, CHK_COND_REQUEST);
          if (lut_ok && v == trunc(v) && v >= 0.0 && v < (double)len) pass = a.p.lut[off + (int)v] != 0;
        }
      }
      if (!pass) fail = k;
    }
    atomicAdd(&hist[0], 1);
    if (fail >= 0) {
      a.tgt[r] = -1;
      atomicAdd(&hist[1], 1);
      atomicAdd(&hist[2 + fail], 1);
    }
  }
  __syncthreads();
  if (tid < 2 + PRED_MAX && hist[tid])
    atomicAdd((unsigned long long*)a.p.stats + tid, (unsigned long long)hist[tid]);
}

void launch_pred_mark(const PredMarkArgs& a, hipStream_t stream) {
  require_unbatched("pred_mark");
  if (a.p.n_pred < 0 || a.p.n_pred > PRED_MAX) throw std::runtime_error("pred_mark: 0..16 predicates");
  if (a.rows <= 0 || a.p.n_pred == 0) return;
  hipLaunchKernelGGL(pred_mark_kernel, dim3((unsigned)((a.rows + PRED_THREADS - 1) / PRED_THREADS)),
                     dim3(PRED_THREADS), 0, stream, a);
}

}  // namespace fedtgan
