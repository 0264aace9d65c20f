// Fidelity evaluator (eval/fidelity.py DeviceFidelity): precision / recall / density / coverage of a decoded table
// against a real one (Naeem et al., Reliable Fidelity and Diversity Metrics for Generative Models, ICML 2020), in the
// row space and metric of the privacy evaluator (privacy.hip: nn_pack packs both tables).
//
//  nn_topk_kernel         all pairs on nn_top2's grid (query tiles x reference chunks): a thread owns one query row
//                         in registers, the workgroup a tile of NN_REF_TILE reference rows column-major in LDS; every
//                         (query, chunk) pair leaves its k smallest d2, ascending, in scratch
//  nn_topk_merge_kernel   the lists of a query folded in chunk order; the k-th value is the squared radius
//  nn_ball_kernel         the same grid with per-reference radii, staged into LDS beside the tile's columns: per
//                         (query, chunk) the number of reference rows with d2 <= rad2[r] (int32) and the smallest d2
//  nn_ball_merge_kernel   counts summed and minima taken in chunk order
//  prdc_reduce_kernel     the four scores from the two passes' counts and minima: integer sums, one division each
//
// d2(q, r) = sum over continuous columns of (q_c - r_c)^2, in column order, plus the number of categorical columns
// whose codes differ.  The metrics compare a distance of one pass with a radius of another (a generated copy of the
// real row X_a has to land exactly on the boundary of the ball whose k-th neighbour is X_a), so every distance here
// comes out of fid_tile_d2 and nowhere else: acc = fma(d, d, acc) per column, then fid_d2's acc + (double)cnt.  d is
// a direct difference, so d2(q, r) == d2(r, q) bit for bit.  A NaN distance compares false everywhere: it is inside
// no ball, is never a minimum and never enters a list.  Nothing is allocated, no floating-point atomics, every
// partial meets its neighbours in chunk order, and the host reads nothing back.
#include "common.h"
#include "launch.h"

#include <math.h>
#include <stdexcept>
#include <string>

namespace fedtgan {

constexpr int FID_THREADS = NN_QUERY_TILE;    // one query row per thread
constexpr int FID_QC = 24;                    // continuous columns of a query held in registers at a time
constexpr int FID_QK = 24;                    // categorical columns
constexpr int FID_PAD_C = NN_REF_TILE + 2;    // LDS rows padded, still 16-B aligned for the wide broadcast reads
constexpr int FID_PAD_K = NN_REF_TILE + 4;

struct FidLds {
  double sc[FID_QC][FID_PAD_C];     // the reference tile, [column][row]
  int sk[FID_QK][FID_PAD_K];
  double rad[NN_REF_TILE];          // nn_ball: the tile's squared radii
};

struct FidQuery {
  const double* qc;                 // the thread's query row (row 0 for a thread past the table)
  const int* qk;
  double qv[FID_QC];                // the current column block of it
  int qi[FID_QK];
};

__device__ __forceinline__ double fid_inf() { return __longlong_as_double(0x7ff0000000000000ll); }

__device__ __forceinline__ void fid_load_query(const NnPairs& p, FidQuery& fq, int b) {
#pragma unroll
  for (int c = 0; c < FID_QC; ++c) {
    const int col = b * FID_QC + c;
    fq.qv[c] = col < p.n_cont ? fq.qc[col] : 0.0;
  }
#pragma unroll
  for (int c = 0; c < FID_QK; ++c) {
    const int col = b * FID_QK + c;
    fq.qi[c] = col < p.n_cat ? fq.qk[col] : 0;
  }
}

// the last step of every distance
__device__ __forceinline__ double fid_d2(double acc, int cnt) { return acc + (double)cnt; }

// The one arithmetic: d[r] = d2(the thread's query, reference row jt + r) for the NN_REF_TILE rows of a tile (rows
// at or past j1 are staged as zeros; the caller masks them).  Columns go in blocks of FID_QC continuous + FID_QK
// categorical ones as in nn_top2_kernel: a table of up to 24 + 24 columns is one block and its query row is loaded
// once, a wider row reloads its block per tile while acc / cnt carry the partial sums, so the continuous terms still
// add up in column order.  Called by all threads of the workgroup (it holds barriers); with RAD the tile's radii are
// in s.rad when it returns.
template <bool RAD>
__device__ __forceinline__ void fid_tile_d2(const NnPairs& p, const double* r_rad2, FidLds& s, FidQuery& fq, int jt,
                                            int j1, double (&d)[NN_REF_TILE]) {
  const int tid = threadIdx.x;
  const int nbc = (p.n_cont + FID_QC - 1) / FID_QC, nbk = (p.n_cat + FID_QK - 1) / FID_QK;
  const int nblk = max(max(nbc, nbk), 1);
  double acc[NN_REF_TILE];
  int cnt[NN_REF_TILE];
#pragma unroll
  for (int r = 0; r < NN_REF_TILE; ++r) {
    acc[r] = 0.0;
    cnt[r] = 0;
  }
  for (int b = 0; b < nblk; ++b) {
    const int ncb = min(FID_QC, p.n_cont - b * FID_QC);     // columns of this block (<= 0: none)
    const int nkb = min(FID_QK, p.n_cat - b * FID_QK);
    __syncthreads();                                        // the previous tile / block has been consumed
    if (nblk > 1) fid_load_query(p, fq, b);
    for (int e = tid; e < NN_REF_TILE * FID_QC; e += FID_THREADS) {
      const int r = e / FID_QC, c = e - r * FID_QC;
      const int j = jt + r, col = b * FID_QC + c;
      s.sc[c][r] = (j < j1 && col < p.n_cont) ? p.r_cont[(size_t)j * p.n_cont + col] : 0.0;
    }
    for (int e = tid; e < NN_REF_TILE * FID_QK; e += FID_THREADS) {
      const int r = e / FID_QK, c = e - r * FID_QK;
      const int j = jt + r, col = b * FID_QK + c;
      s.sk[c][r] = (j < j1 && col < p.n_cat) ? p.r_cat[(size_t)j * p.n_cat + col] : 0;
    }
    if (RAD && b == 0 && tid < NN_REF_TILE) s.rad[tid] = (jt + tid < j1) ? r_rad2[jt + tid] : 0.0;
    __syncthreads();
#pragma unroll
    for (int c = 0; c < FID_QC; ++c) {
      if (c < ncb) {                                        // (uniform over the workgroup)
        const double x = fq.qv[c];
#pragma unroll
        for (int r = 0; r < NN_REF_TILE; ++r) {
          const double df = x - s.sc[c][r];
          acc[r] = fma(df, df, acc[r]);
        }
      }
    }
#pragma unroll
    for (int c = 0; c < FID_QK; ++c) {
      if (c < nkb) {
        const int x = fq.qi[c];
#pragma unroll
        for (int r = 0; r < NN_REF_TILE; ++r) cnt[r] += (x != s.sk[c][r]) ? 1 : 0;
      }
    }
  }
#pragma unroll
  for (int r = 0; r < NN_REF_TILE; ++r) d[r] = fid_d2(acc[r], cnt[r]);
}

// v < best[K - 1] (so v is no NaN) into the ascending list: best[i] = min(best[i], max(best[i - 1], v)), from the top
// down so that every step reads the old best[i - 1].  min / max move values, they round nothing.
template <int K>
__device__ __forceinline__ void fid_insert(double (&best)[K], double v) {
#pragma unroll
  for (int i = K - 1; i > 0; --i) best[i] = fmin(best[i], fmax(best[i - 1], v));
  best[0] = fmin(best[0], v);
}

__device__ __forceinline__ void fid_query_rows(const NnPairs& p, int q, FidQuery& fq) {
  const bool live = q < p.nq;
  fq.qc = p.q_cont + (size_t)(live ? q : 0) * p.n_cont;
  fq.qk = p.q_cat + (size_t)(live ? q : 0) * p.n_cat;
  fid_load_query(p, fq, 0);
}

// ============================================================================ k-th neighbour
// The list lives in K registers (K is a template parameter: no list is ever indexed by a run-time value, which would
// send it to scratch memory).
template <int K>
__global__ __launch_bounds__(FID_THREADS) void nn_topk_kernel(NnTopkArgs a) {
  __shared__ __attribute__((aligned(16))) FidLds s;
  const NnPairs& p = a.p;
  const int q = blockIdx.x * NN_QUERY_TILE + threadIdx.x;
  const int chunk = blockIdx.y;
  const int j0 = chunk * NN_CHUNK_ROWS;
  const int j1 = min(p.nr, j0 + NN_CHUNK_ROWS);
  FidQuery fq;
  fid_query_rows(p, q, fq);
  double best[K];
#pragma unroll
  for (int i = 0; i < K; ++i) best[i] = fid_inf();
  for (int jt = j0; jt < j1; jt += NN_REF_TILE) {
    double d[NN_REF_TILE];
    fid_tile_d2<false>(p, nullptr, s, fq, jt, j1, d);
#pragma unroll
    for (int r = 0; r < NN_REF_TILE; ++r) {
      const int j = jt + r;
      const bool ok = j < j1 && !(a.exclude_self && j == q);
      const double v = ok ? d[r] : fid_inf();
      if (v < best[K - 1]) fid_insert<K>(best, v);
    }
  }
  if (q < p.nq) {
#pragma unroll
    for (int i = 0; i < K; ++i) a.part[((size_t)chunk * K + i) * p.nq + q] = best[i];
  }
}

// the k smallest overall are among the chunks' k smallest: the merged list's entry k - 1 is the k-th neighbour
__global__ __launch_bounds__(FID_THREADS) void nn_topk_merge_kernel(NnTopkArgs a) {
  const int q = blockIdx.x * FID_THREADS + threadIdx.x;
  if (q >= a.p.nq) return;
  double best[FID_MAX_K];
#pragma unroll
  for (int i = 0; i < FID_MAX_K; ++i) best[i] = fid_inf();
  for (int c = 0; c < a.p.chunks; ++c) {
    for (int i = 0; i < a.k; ++i) {
      const double v = a.part[((size_t)c * a.k + i) * a.p.nq + q];
      if (v < best[FID_MAX_K - 1]) fid_insert<FID_MAX_K>(best, v);
    }
  }
  double kth = best[0];
#pragma unroll
  for (int i = 1; i < FID_MAX_K; ++i)
    if (i == a.k - 1) kth = best[i];
  a.out[q] = kth;
}

int64_t nn_topk_scratch_doubles(int64_t nq, int64_t nr, int k) {
  const int64_t n = (int64_t)k * nq * nn_chunks(nr);
  return n > 0 ? n : 1;
}

static void fid_check_sizes(const NnPairs& p, const char* what) {
  if (p.nq < 0 || p.nr < 1 || p.n_cont < 0 || p.n_cat < 0 || p.n_cont + p.n_cat < 1)
    throw std::runtime_error(std::string(what) + ": table sizes");
  if (nn_chunks(p.nr) > 65535) throw std::runtime_error(std::string(what) + ": too many reference rows");
}

template <int K>
static void fid_launch_topk(const NnTopkArgs& a, dim3 grid, hipStream_t stream) {
  hipLaunchKernelGGL(nn_topk_kernel<K>, grid, dim3(FID_THREADS), 0, stream, a);
}

void launch_nn_topk(NnTopkArgs a, double* scratch, hipStream_t stream) {
  require_unbatched("nn_topk");
  fid_check_sizes(a.p, "nn_topk");
  if (a.k < 1 || a.k > FID_MAX_K) throw std::runtime_error("nn_topk: k outside 1..FID_MAX_K");
  if (a.p.nq == 0) return;
  a.p.chunks = nn_chunks(a.p.nr);
  a.part = scratch;
  const unsigned tiles = (unsigned)((a.p.nq + NN_QUERY_TILE - 1) / NN_QUERY_TILE);
  const dim3 grid(tiles, (unsigned)a.p.chunks);
  switch (a.k) {
    case 1: fid_launch_topk<1>(a, grid, stream); break;
    case 2: fid_launch_topk<2>(a, grid, stream); break;
    case 3: fid_launch_topk<3>(a, grid, stream); break;
    case 4: fid_launch_topk<4>(a, grid, stream); break;
    case 5: fid_launch_topk<5>(a, grid, stream); break;
    case 6: fid_launch_topk<6>(a, grid, stream); break;
    case 7: fid_launch_topk<7>(a, grid, stream); break;
    default: fid_launch_topk<8>(a, grid, stream); break;
  }
  hipLaunchKernelGGL(nn_topk_merge_kernel, dim3(tiles), dim3(FID_THREADS), 0, stream, a);
}

// ============================================================================ balls
// <= is inclusive; a reference row's radius of +inf holds every query whose distance to it is no NaN.
__global__ __launch_bounds__(FID_THREADS) void nn_ball_kernel(NnBallArgs a) {
  __shared__ __attribute__((aligned(16))) FidLds s;
  const NnPairs& p = a.p;
  const int q = blockIdx.x * NN_QUERY_TILE + threadIdx.x;
  const int chunk = blockIdx.y;
  const int j0 = chunk * NN_CHUNK_ROWS;
  const int j1 = min(p.nr, j0 + NN_CHUNK_ROWS);
  FidQuery fq;
  fid_query_rows(p, q, fq);
  int cnt = 0;
  double dmin = fid_inf();
  for (int jt = j0; jt < j1; jt += NN_REF_TILE) {
    double d[NN_REF_TILE];
    fid_tile_d2<true>(p, a.r_rad2, s, fq, jt, j1, d);
#pragma unroll
    for (int r = 0; r < NN_REF_TILE; ++r) {
      const bool ok = jt + r < j1;
      cnt += (ok && d[r] <= s.rad[r]) ? 1 : 0;
      if (ok && d[r] < dmin) dmin = d[r];
    }
  }
  if (q < p.nq) {
    const size_t o = (size_t)chunk * p.nq + q;
    a.part_cnt[o] = cnt;
    a.part_min[o] = dmin;
  }
}

__global__ __launch_bounds__(FID_THREADS) void nn_ball_merge_kernel(NnBallArgs a) {
  const int q = blockIdx.x * FID_THREADS + threadIdx.x;
  if (q >= a.p.nq) return;
  int cnt = 0;
  double dmin = fid_inf();
  for (int c = 0; c < a.p.chunks; ++c) {
    const size_t o = (size_t)c * a.p.nq + q;
    cnt += a.part_cnt[o];
    const double v = a.part_min[o];
    if (v < dmin) dmin = v;
  }
  a.cnt[q] = cnt;
  a.dmin[q] = dmin;
}

int64_t nn_ball_scratch_doubles(int64_t nq, int64_t nr) {
  const int64_t slots = nq * nn_chunks(nr);
  const int64_t n = slots + (slots + 1) / 2;     // the minima, and the counts as int32
  return n > 0 ? n : 1;
}

void launch_nn_ball(NnBallArgs a, double* scratch, hipStream_t stream) {
  require_unbatched("nn_ball");
  fid_check_sizes(a.p, "nn_ball");
  if (a.p.nq == 0) return;
  a.p.chunks = nn_chunks(a.p.nr);
  const size_t slots = (size_t)a.p.nq * a.p.chunks;
  a.part_min = scratch;
  a.part_cnt = (int*)(scratch + slots);
  const unsigned tiles = (unsigned)((a.p.nq + NN_QUERY_TILE - 1) / NN_QUERY_TILE);
  hipLaunchKernelGGL(nn_ball_kernel, dim3(tiles, (unsigned)a.p.chunks), dim3(FID_THREADS), 0, stream, a);
  hipLaunchKernelGGL(nn_ball_merge_kernel, dim3(tiles), dim3(FID_THREADS), 0, stream, a);
}

// ============================================================================ the four scores
// one workgroup: a thread sums its strided share in int64, the shares meet in a tree of fixed shape (integer sums:
// any order gives the same value), and thread 0 divides once per score
__global__ __launch_bounds__(FID_THREADS) void prdc_reduce_kernel(PrdcArgs a) {
  __shared__ long long sum[4][FID_THREADS];
  const int tid = threadIdx.x;
  long long inside = 0, balls = 0, recalled = 0, covered = 0;
  for (int j = tid; j < a.n; j += FID_THREADS) {
    const int c = a.cnt_a[j];
    inside += c > 0 ? 1 : 0;
    balls += c;
  }
  for (int i = tid; i < a.m; i += FID_THREADS) {
    recalled += a.cnt_b[i] > 0 ? 1 : 0;
    covered += a.dmin_b[i] <= a.rr[i] ? 1 : 0;
  }
  sum[0][tid] = inside;
  sum[1][tid] = recalled;
  sum[2][tid] = balls;
  sum[3][tid] = covered;
  __syncthreads();
  for (int st = FID_THREADS / 2; st > 0; st >>= 1) {
    if (tid < st) {
#pragma unroll
      for (int v = 0; v < 4; ++v) sum[v][tid] += sum[v][tid + st];
    }
    __syncthreads();
  }
  if (tid == 0) {
    const double n = (double)a.n, m = (double)a.m;
    a.scores[0] = (double)sum[0][0] / n;                                          // precision
    a.scores[1] = (double)sum[1][0] / m;                                          // recall
    a.scores[2] = (double)sum[2][0] / (double)((long long)a.k * (long long)a.n);  // density
    a.scores[3] = (double)sum[3][0] / m;                                          // coverage
  }
}

void launch_prdc_reduce(const PrdcArgs& a, hipStream_t stream) {
  require_unbatched("prdc_reduce");
  if (a.n < 1 || a.m < 1 || a.k < 1 || a.k > FID_MAX_K) throw std::runtime_error("prdc_reduce: row counts / k");
  hipLaunchKernelGGL(prdc_reduce_kernel, dim3(1), dim3(FID_THREADS), 0, stream, a);
}

}  // namespace fedtgan
