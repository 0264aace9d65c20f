// Completion of partial rows (CTGANEngine.generate_decoded_known): generate the unknown cells of a known table.
//
//  known_request_kernel  after the generation sampler: the rows of slot s (tries consecutive rows of the pass) take
//                        the condition of the slot's query -- its driving span and option, chosen once per table
//                        on the host -- unless the slot is idle or the query has no driver.  No random numbers.
//  known_match_kernel    after the decode: one workgroup per slot.  The query's known cells are compacted into LDS
//                        (column, kind, value, scale, in column order), the slot's candidates pass through LDS in
//                        coalesced tiles, a thread judges one candidate of a tile, and the lowest candidate with the
//                        smallest distance replaces the query's best so far if it is strictly closer; the wave that
//                        holds it writes the completed row (known cells from the input, the rest from the candidate).
//
// The distance is the privacy evaluator's mixed d2 over the known cells alone: continuous columns in column order,
// d = (known - cand) * scale (a subtraction, then a product: nothing to contract), acc = fma(d, d, acc) as
// nn_within_kernel writes it, plus the count of known categorical cells whose code differs (codes are compared,
// never used as an index).  Queries are independent and a query appears at most once in a pass, so no workgroup
// waits on another and the result does not depend on the order in which workgroups run.
#include "common.h"
#include "launch.h"

#include <stdexcept>

namespace fedtgan {

#if FT_CHECKED
__device__ unsigned g_check_known = 0u;
unsigned check_status_known_gen() {
  unsigned v = 0u, z = 0u;
  (void)hipMemcpyFromSymbol(&v, HIP_SYMBOL(g_check_known), sizeof(v));
  (void)hipMemcpyToSymbol(HIP_SYMBOL(g_check_known), &z, sizeof(z));
  return v;
}
#else
unsigned check_status_known_gen() { return 0u; }
#endif

constexpr int KNOWN_THREADS = 256;
constexpr int KNOWN_WAVES = KNOWN_THREADS / WAVE;
constexpr int KNOWN_TILE = 4096;                  // doubles of a staged tile (32 KB), rows padded to an odd stride
constexpr int KNOWN_MAX_COLS = 1024;              // the compacted query shares the workgroup's 64 KB of LDS
constexpr int KNOWN_CAT = 1 << 30;                // flag on a compacted column index: categorical
constexpr int KNOWN_LD = 8;                       // loads in flight per lane before their LDS stores

// ============================================================================ request
__global__ __launch_bounds__(KNOWN_THREADS) void known_request_kernel(KnownRequestArgs a) {
  const int64_t b = (int64_t)blockIdx.x * KNOWN_THREADS + threadIdx.x;
  if (b >= (int64_t)a.n_slots * a.tries) return;
  const int s = (int)(b / a.tries);
  const int i = a.qidx[s];
  FT_CHECK(&g_check_known, i >= -1 && i < a.n_query, CHK_COND_REQUEST);
  if (i < 0 || i >= a.n_query) return;            // idle slot: the sampler's draw stays
  const int span = a.drv_span[i];
  if (span < 0) return;                           // nothing known drives this query
  const int o = a.drv_opt[i];
  // as cond_request_kernel: a driver outside the span tables is flagged by the checked build and, in every build,
  // leaves the row as the sampler drew it
  const bool span_ok = span < a.n_span && o >= 0 && o < a.cond_w[min(span, a.n_span - 1)];
  FT_CHECK(&g_check_known, span_ok, CHK_COND_REQUEST);
  if (!span_ok) return;
  if (a.h) {
    // fp32 activation buffer: the sampler wrote a one-hot block; move the row's hot element (two stores)
    const int co = a.col[b], oo = a.opt[b];
    const int was = (co >= 0 && co < a.n_span) ? a.cond_off[co] + oo : -1;
    const int now = a.cond_off[span] + o;
    FT_CHECK(&g_check_known, was >= 0 && was < a.C && now >= 0 && now < a.C, CHK_COND_REQUEST);
    float* hrow = a.h + (size_t)b * a.ldh + a.cc;
    if (was >= 0 && was < a.C) hrow[was] = 0.f;
    if (now >= 0 && now < a.C) hrow[now] = 1.f;
  }
  a.col[b] = span;
  a.opt[b] = o;
}

void launch_known_request(const KnownRequestArgs& a, hipStream_t stream) {
  require_unbatched("known_request");
  if (a.tries < 1 || a.tries > KNOWN_MAX_TRIES) throw std::runtime_error("known_request: 1..1024 tries");
  const int64_t rows = (int64_t)a.n_slots * a.tries;
  if (rows <= 0) return;
  hipLaunchKernelGGL(known_request_kernel, dim3((unsigned)((rows + KNOWN_THREADS - 1) / KNOWN_THREADS)),
                     dim3(KNOWN_THREADS), 0, stream, a);
}

// ============================================================================ match
// LDS of a workgroup: [tile: KNOWN_TILE + KNOWN_THREADS doubles][kval: n_cols][kscale: n_cols][reduction: 2 *
// KNOWN_WAVES doubles][kidx: n_cols ints][wave counts: KNOWN_WAVES ints].
//
// A tile holds TR = min(tries, 256) candidates x CT columns, CT = min(n_cols, 4096 / TR): with 64 tries and the 42
// columns of the Intrusion table the whole slot is one contiguous 21.5 KB read.  LDS rows have the odd stride CT | 1,
// so the 32 lanes of a half-wave that read one column of 32 candidates (ds_read_b64) hit 32 different bank pairs.
// A table wider than a tile is walked in column tiles, the thread keeping its candidate's sum across them: the
// column order of the sum never changes.  A column tile without a known cell is not loaded.
__device__ __forceinline__ bool known_less(double d, int t, double od, int ot) { return od < d || (od == d && ot < t); }

__global__ __launch_bounds__(KNOWN_THREADS) void known_match_kernel(KnownMatchArgs a) {
  extern __shared__ __attribute__((aligned(16))) double known_smem[];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int s = blockIdx.x;
  const int i = a.qidx[s];
  FT_CHECK(&g_check_known, i >= -1 && i < a.n_query, CHK_COND_REQUEST);
  if (i < 0 || i >= a.n_query) return;            // idle slot (uniform over the workgroup): nothing is written
  const int n = a.n_cols;
  double* tile = known_smem;
  double* kval = tile + KNOWN_TILE + KNOWN_THREADS;
  double* kscale = kval + n;
  double* rd2 = kscale + n;
  int* rt = (int*)(rd2 + KNOWN_WAVES);
  int* kidx = rt + 2 * KNOWN_WAVES;
  int* wcnt = kidx + n;

  // ---- the query's known cells, compacted in column order (ballot ranks inside a wave, wave counts across)
  const double* krow = a.known + (size_t)i * n;
  const uint8_t* mrow = a.mask + (size_t)i * n;
  int nk = 0;
  for (int j0 = 0; j0 < n; j0 += KNOWN_THREADS) {
    const int j = j0 + tid;
    const bool on = j < n && mrow[j] != 0;
    const unsigned long long bal = __ballot(on);
    if (lane == 0) wcnt[wv] = __popcll(bal);
    __syncthreads();
    int at = nk, all = 0;
#pragma unroll
    for (int w = 0; w < KNOWN_WAVES; ++w) {
      if (w < wv) at += wcnt[w];
      all += wcnt[w];
    }
    if (on) {
      at += __popcll(bal & ((1ull << lane) - 1ull));
      const bool cat = a.kind[j] != 0;
      kidx[at] = cat ? (j | KNOWN_CAT) : j;
      kval[at] = krow[j];
      kscale[at] = cat ? 0.0 : a.scale[j];
    }
    nk += all;
    __syncthreads();
  }

  // ---- the slot's candidates
  const int R = a.tries;
  const int TR = min(R, KNOWN_THREADS);
  const int CT = min(n, max(1, KNOWN_TILE / TR));
  const int stride = CT | 1;
  const double* __restrict__ src = a.cand + (size_t)s * R * n;
  double bd2 = __builtin_inf(), bdc = 0.0;
  int bt = tid < R ? tid : 2147483647, bms = 0;
  for (int r0 = 0; r0 < R; r0 += TR) {
    const int trn = min(TR, R - r0);
    double acc = 0.0;
    int ms = 0, kp = 0;
    for (int c0 = 0; c0 < n && kp < nk; c0 += CT) {
      const int ct = min(CT, n - c0);
      if ((kidx[kp] & (KNOWN_CAT - 1)) >= c0 + ct) continue;      // no known cell in these columns (uniform)
      // stage rows r0 .. r0 + trn, columns c0 .. c0 + ct: element e = (row e / ct, column e % ct), the lanes of a
      // wave on consecutive elements; (row, column) advance by 256 elements without a division
      const int ne = trn * ct;
      const int dr = KNOWN_THREADS / ct, dcn = KNOWN_THREADS - dr * ct;
      int r = tid / ct, c = tid - r * ct;
      for (int e0 = tid; e0 < ne; e0 += KNOWN_THREADS * KNOWN_LD) {
        double v[KNOWN_LD];
        int li[KNOWN_LD];
#pragma unroll
        for (int u = 0; u < KNOWN_LD; ++u) {
          const bool ok = e0 + u * KNOWN_THREADS < ne;
          v[u] = src[ok ? (size_t)(r0 + r) * n + (c0 + c) : (size_t)0];
          li[u] = r * stride + c;
          c += dcn;
          r += dr;
          if (c >= ct) {
            c -= ct;
            ++r;
          }
        }
#pragma unroll
        for (int u = 0; u < KNOWN_LD; ++u)
          if (e0 + u * KNOWN_THREADS < ne) tile[li[u]] = v[u];
      }
      __syncthreads();
      const int tb = tid * stride - c0;
      while (kp < nk) {                                           // (uniform: every thread walks the same list)
        const int kj = kidx[kp];
        const int j = kj & (KNOWN_CAT - 1);
        if (j >= c0 + ct) break;
        if (tid < trn) {
          const double v = tile[tb + j];
          if (kj & KNOWN_CAT) {
            ms += (v != kval[kp]) ? 1 : 0;
          } else {
            const double d = (kval[kp] - v) * kscale[kp];
            acc = fma(d, d, acc);
          }
        }
        ++kp;
      }
      __syncthreads();                                            // the tile may be overwritten
    }
    if (tid < trn) {
      const double d2 = acc + (double)ms;
      if (d2 < bd2 || r0 == 0) {          // ascending candidates, strict <: the lowest of equal ones stays
        bdc = acc;
        bms = ms;
        bt = r0 + tid;
      }
      if (d2 < bd2) bd2 = d2;             // (a NaN distance never wins)
    }
  }

  // ---- the lowest candidate with the smallest distance: across the wave, then across the waves
  double wd2 = bd2;
  int wt = bt;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const double od = __shfl_xor(wd2, o, WAVE);
    const int ot = __shfl_xor(wt, o, WAVE);
    if (known_less(wd2, wt, od, ot)) {
      wd2 = od;
      wt = ot;
    }
  }
  if (lane == 0) {
    rd2[wv] = wd2;
    rt[wv] = wt;
  }
  __syncthreads();
  wd2 = rd2[0];
  wt = rt[0];
#pragma unroll
  for (int w = 1; w < KNOWN_WAVES; ++w)
    if (known_less(wd2, wt, rd2[w], rt[w])) {
      wd2 = rd2[w];
      wt = rt[w];
    }
  FT_CHECK(&g_check_known, wt >= 0 && wt < R, CHK_COND_REQUEST);
  wt = min(max(wt, 0), R - 1);
  if (wv != ((wt % KNOWN_THREADS) >> 6)) return;  // the wave that holds the winner finishes alone (no barrier below)
  const bool upd = wd2 < a.best[i];                // strict: an equal later candidate does not replace an earlier one
  if (upd) {
    const double* crow = src + (size_t)wt * n;
    double* drow = a.dst + (size_t)i * n;
    for (int j = lane; j < n; j += WAVE) drow[j] = mrow[j] != 0 ? krow[j] : crow[j];
  }
  if (tid == wt % KNOWN_THREADS) {
    const int64_t seen = a.seen[i];
    if (upd) {
      a.best[i] = wd2;
      a.dc[i] = bdc;
      a.miss[i] = bms;
      a.pick[i] = seen + wt;
    }
    a.seen[i] = seen + R;
  }
}

static size_t known_match_lds(int n_cols) {
  return (size_t)(KNOWN_TILE + KNOWN_THREADS + 2 * n_cols + KNOWN_WAVES) * sizeof(double) +
         (size_t)(2 * KNOWN_WAVES + n_cols + KNOWN_WAVES) * sizeof(int);
}

void launch_known_match(const KnownMatchArgs& a, hipStream_t stream) {
  require_unbatched("known_match");
  if (a.tries < 1 || a.tries > KNOWN_MAX_TRIES) throw std::runtime_error("known_match: 1..1024 tries");
  if (a.n_cols < 1 || a.n_cols > KNOWN_MAX_COLS) throw std::runtime_error("known_match: 1..1024 columns");
  if (a.n_slots <= 0) return;
  hipLaunchKernelGGL(known_match_kernel, dim3((unsigned)a.n_slots), dim3(KNOWN_THREADS), known_match_lds(a.n_cols),
                     stream, a);
}

}  // namespace fedtgan
