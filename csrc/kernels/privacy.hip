// Privacy evaluator (eval/privacy.py DevicePrivacy): DCR / NNDR of a decoded table against a real one, on the device.
//
//  nn_pack_kernel         one pass over a row-major decoded table: continuous columns scaled by the real table's
//                         min-max into a dense fp64 [n, n_cont] buffer, categorical codes into an int32 [n, n_cat] one
//  nn_top2_kernel         all pairs, grid = (query tiles, reference chunks): a thread owns one query row (held in
//                         registers), the workgroup shares a tile of NN_REF_TILE reference rows staged in LDS, and every
//                         (query, chunk) pair leaves its partial (d1, d2, i1) in scratch
//  nn_merge_kernel        the partials of a query folded in chunk order (strict <: the lowest index wins a tie)
//  nn_within_kernel       the privacy guard's radius test on the same grid: the lowest reference row with d2 <= t2 per
//                         (query, chunk), candidates abandoned once out of range; nn_within_merge_kernel takes the
//                         first chunk with a hit, guard_mark_kernel clears the target of the rows that have one
//  nn_merge_shards_kernel the (d1, d2, i1) answers of K shards folded in client order into the answer over their union,
//                         with per-client counts; nn_within_merge_shards_kernel the same for the radius test
//  nn_stats_kernel        sqrt(d1) and the distance ratio into two key rows (sorted by launch_sim_sort afterwards);
//                         per-workgroup minimum and count of exact zeros in fixed slots
//  nn_percentile_kernel   the two interpolated 5th percentiles from the sorted rows, the minimum and the share of zeros
//
// d2(q, r) = sum over continuous columns of (q_c - r_c)^2, in column order, plus the number of categorical columns
// whose codes differ, all in fp64 from direct differences: a copied record is at exactly 0.  Codes are compared, never
// used as an index.  Every query's candidates are visited in ascending index order and partials meet in chunk order,
// so a table scores bit-identically on every run; nothing is allocated and the host reads nothing back.
#include "common.h"
#include "launch.h"

#include <math.h>
#include <stdexcept>

namespace fedtgan {

constexpr int NN_THREADS = NN_QUERY_TILE;   // one query row per thread
constexpr int NN_QC = 24;                   // continuous columns of a query held in registers at a time
constexpr int NN_QK = 24;                   // categorical columns
constexpr int NN_PAD_C = NN_REF_TILE + 2;   // LDS rows padded, still 16-B aligned for the wide broadcast reads
constexpr int NN_PAD_K = NN_REF_TILE + 4;

__device__ __forceinline__ double nn_inf() { return __longlong_as_double(0x7ff0000000000000ll); }

// ============================================================================ pack
// one thread per cell: the table is read coalesced.  (v - lo) * scale is a subtraction and then a product: there is
// no multiply-add in it for the compiler to contract, so the values equal the reference ops' bit for bit.
__global__ __launch_bounds__(NN_THREADS) void nn_pack_kernel(NnPackArgs a) {
  const long long i = (long long)blockIdx.x * NN_THREADS + threadIdx.x;
  if (i >= (long long)a.rows * a.n_cols) return;
  const long long r = i / a.n_cols;
  const int c = (int)(i - r * a.n_cols);
  const int k = a.kind[c], s = a.slot[c];
  const double v = a.values[i];
  if (k == NN_CAT) {
    // (a NaN or out-of-range value is no code at all: -1 equals no code of either table's valid range)
    if (s >= 0 && s < a.n_cat) a.cat[r * a.n_cat + s] = (v >= 0.0 && v < 2147483647.0) ? (int)v : -1;
  } else if (s >= 0 && s < a.n_cont) {
    a.cont[r * a.n_cont + s] = (v - a.lo[s]) * a.scale[s];
  }
}

void launch_nn_pack(const NnPackArgs& a, hipStream_t stream) {
  require_unbatched("nn_pack");
  if (a.rows < 0 || a.n_cols <= 0 || a.n_cont < 0 || a.n_cat < 0) throw std::runtime_error("nn_pack: table sizes");
  const long long cells = (long long)a.rows * a.n_cols;
  if (cells == 0) return;
  if (cells >= (long long)INT32_MAX * NN_THREADS) throw std::runtime_error("nn_pack: table too large");
  hipLaunchKernelGGL(nn_pack_kernel, dim3((unsigned)((cells + NN_THREADS - 1) / NN_THREADS)), dim3(NN_THREADS), 0,
                     stream, a);
}

// ============================================================================ all-pairs top-2
// Columns are processed in blocks of NN_QC continuous + NN_QK categorical columns (block b holds continuous columns
// [b NN_QC, ...) and categorical columns [b NN_QK, ...)); a table of up to 24 + 24 columns is one block and its query
// row is loaded once.  Wider rows reload the query block per tile, and the per-thread accumulators of the tile's
// NN_REF_TILE reference rows carry the partial sums across the blocks, so the continuous terms still add up in column
// order; the mismatch count is an integer and joins at the end.
//
// The reference tile sits in LDS column-major ([column][row]): all lanes of a wave read the same address (a
// broadcast, no bank conflict) and a column's 16 rows are contiguous for 16-byte reads.  The chunk is blockIdx.y, the
// slow grid dimension: workgroups are dealt round-robin over the XCDs by linear id, so at any time every XCD works
// on the same one or two chunks (0.5 MB each at 42 columns) and re-reads them from its own L2.
__global__ __launch_bounds__(NN_THREADS) void nn_top2_kernel(NnTop2Args a) {
  __shared__ __attribute__((aligned(16))) double sc[NN_QC][NN_PAD_C];
  __shared__ __attribute__((aligned(16))) int sk[NN_QK][NN_PAD_K];
  const int tid = threadIdx.x;
  const int q = blockIdx.x * NN_QUERY_TILE + tid;
  const bool live = q < a.nq;
  const int chunk = blockIdx.y;
  const int j0 = chunk * NN_CHUNK_ROWS;
  const int j1 = min(a.nr, j0 + NN_CHUNK_ROWS);
  const int nbc = (a.n_cont + NN_QC - 1) / NN_QC, nbk = (a.n_cat + NN_QK - 1) / NN_QK;
  const int nblk = max(max(nbc, nbk), 1);
  const double* qc = a.q_cont + (size_t)(live ? q : 0) * a.n_cont;
  const int* qk = a.q_cat + (size_t)(live ? q : 0) * a.n_cat;

  double qv[NN_QC];
  int qi[NN_QK];
  auto load_query = [&](int b) {
#pragma unroll
    for (int c = 0; c < NN_QC; ++c) {
      const int col = b * NN_QC + c;
      qv[c] = col < a.n_cont ? qc[col] : 0.0;
    }
#pragma unroll
    for (int c = 0; c < NN_QK; ++c) {
      const int col = b * NN_QK + c;
      qi[c] = col < a.n_cat ? qk[col] : 0;
    }
  };
  load_query(0);

  double d1 = nn_inf(), d2 = nn_inf();
  int i1 = -1;
  for (int jt = j0; jt < j1; jt += NN_REF_TILE) {
    double acc[NN_REF_TILE];
    int cnt[NN_REF_TILE];
#pragma unroll
    for (int r = 0; r < NN_REF_TILE; ++r) {
      acc[r] = 0.0;
      cnt[r] = 0;
    }
    for (int b = 0; b < nblk; ++b) {
      const int ncb = min(NN_QC, a.n_cont - b * NN_QC);     // columns of this block (<= 0: none)
      const int nkb = min(NN_QK, a.n_cat - b * NN_QK);
      __syncthreads();                                      // the previous tile / block has been consumed
      if (nblk > 1) load_query(b);
      for (int e = tid; e < NN_REF_TILE * NN_QC; e += NN_THREADS) {
        const int r = e / NN_QC, c = e - r * NN_QC;
        const int j = jt + r, col = b * NN_QC + c;
        sc[c][r] = (j < j1 && col < a.n_cont) ? a.r_cont[(size_t)j * a.n_cont + col] : 0.0;
      }
      for (int e = tid; e < NN_REF_TILE * NN_QK; e += NN_THREADS) {
        const int r = e / NN_QK, c = e - r * NN_QK;
        const int j = jt + r, col = b * NN_QK + c;
        sk[c][r] = (j < j1 && col < a.n_cat) ? a.r_cat[(size_t)j * a.n_cat + col] : 0;
      }
      __syncthreads();
#pragma unroll
      for (int c = 0; c < NN_QC; ++c) {
        if (c < ncb) {                                      // (uniform over the workgroup)
          const double x = qv[c];
#pragma unroll
          for (int r = 0; r < NN_REF_TILE; ++r) {
            const double d = x - sc[c][r];
            acc[r] += d * d;
          }
        }
      }
#pragma unroll
      for (int c = 0; c < NN_QK; ++c) {
        if (c < nkb) {
          const int x = qi[c];
#pragma unroll
          for (int r = 0; r < NN_REF_TILE; ++r) cnt[r] += (x != sk[c][r]) ? 1 : 0;
        }
      }
    }
    // candidates in ascending index order; strict <, so the first of equal distances keeps i1 and the second
    // becomes d2 (multiplicity)
#pragma unroll
    for (int r = 0; r < NN_REF_TILE; ++r) {
      const int j = jt + r;
      const bool ok = j < j1 && !(a.exclude_self && j == q);
      const double d = ok ? acc[r] + (double)cnt[r] : nn_inf();
      if (d < d1) {
        d2 = d1;
        d1 = d;
        i1 = j;
      } else if (d < d2) {
        d2 = d;
      }
    }
  }
  if (live) {
    const size_t o = (size_t)chunk * a.nq + q;
    a.part_d1[o] = d1;
    a.part_d2[o] = d2;
    a.part_i1[o] = i1;
  }
}

__global__ __launch_bounds__(NN_THREADS) void nn_merge_kernel(NnTop2Args a, double* out_d1, double* out_d2,
                                                              int* out_i1) {
  const int q = blockIdx.x * NN_THREADS + threadIdx.x;
  if (q >= a.nq) return;
  double d1 = nn_inf(), d2 = nn_inf();
  int i1 = -1;
  for (int c = 0; c < a.chunks; ++c) {          // chunk c holds indices below chunk c + 1's
    const size_t o = (size_t)c * a.nq + q;
    const double b1 = a.part_d1[o], b2 = a.part_d2[o];
    if (b1 < d1) {
      d2 = b2 < d1 ? b2 : d1;
      d1 = b1;
      i1 = a.part_i1[o];
    } else if (b1 < d2) {
      d2 = b1;
    }
  }
  out_d1[q] = d1;
  out_d2[q] = d2;
  out_i1[q] = i1;
}

int nn_chunks(int64_t nr) {
  const int64_t c = (nr + NN_CHUNK_ROWS - 1) / NN_CHUNK_ROWS;
  return c > 0 ? (int)c : 1;
}

int64_t nn_scratch_doubles(int64_t nq, int64_t nr) {
  const int64_t slots = nq * nn_chunks(nr);
  const int64_t n = 2 * slots + (slots + 1) / 2;     // d1, d2, and i1 as int32
  return n > 0 ? n : 1;
}

void launch_nn_top2(NnTop2Args a, double* d1, double* d2, int* i1, double* scratch, hipStream_t stream) {
  require_unbatched("nn_top2");
  if (a.nq < 0 || a.nr < 1 || a.n_cont < 0 || a.n_cat < 0 || a.n_cont + a.n_cat < 1)
    throw std::runtime_error("nn_top2: table sizes");
  if (a.nq == 0) return;
  a.chunks = nn_chunks(a.nr);
  if (a.chunks > 65535) throw std::runtime_error("nn_top2: too many reference rows");
  const size_t slots = (size_t)a.nq * a.chunks;
  a.part_d1 = scratch;
  a.part_d2 = scratch + slots;
  a.part_i1 = (int*)(scratch + 2 * slots);
  const unsigned tiles = (unsigned)((a.nq + NN_QUERY_TILE - 1) / NN_QUERY_TILE);
  hipLaunchKernelGGL(nn_top2_kernel, dim3(tiles, (unsigned)a.chunks), dim3(NN_THREADS), 0, stream, a);
  hipLaunchKernelGGL(nn_merge_kernel, dim3(tiles), dim3(NN_THREADS), 0, stream, a, d1, d2, i1);
}

// ============================================================================ radius test (the privacy guard)
// near[q] = the lowest index of a reference row with d2(q, r) <= t2, or -1: nn_top2's grid, tiles and column blocks,
// but no candidate needs an exact distance once it is out of range, and no query a second neighbour.
//
//  (1) a tile's categorical mismatches are counted first (all column blocks).  They are integers, and every
//      continuous term is >= 0, so a candidate with (double)cnt > t2 is dead, also while its count is still partial: a
//      wave whose candidates are all dead stops counting.  Where no thread of the workgroup has a candidate left,
//      the tile's continuous columns are not staged at all.
//  (2) the continuous columns add up as in nn_top2_kernel (column order, acc = fma(d, d, acc): the instruction the
//      compiler contracts nn_top2's `acc += d * d` to), NN_WITHIN_GROUP columns at a time; after a group a candidate
//      with acc + (double)cnt > t2 is dead.  That is exact: fp64 rounding is monotone and every term is >= 0, so the
//      final acc is no smaller than a partial one, and neither is the final acc + (double)cnt.  A wave without a
//      candidate left skips the block's remaining groups.
//  (3) candidates are visited in ascending index order, so the first hit of a chunk is its lowest: a query with a hit
//      has no candidates in later tiles, and a workgroup whose live queries all have hits leaves the chunk.
//
// A surviving candidate's distance is the very acc + (double)cnt nn_top2 computes, so a row this test keeps is a row
// the evaluator scores at d1 > t2.  A NaN distance never compares > t2, is never pruned and never hits.
constexpr int NN_WITHIN_GROUP = 4;
constexpr unsigned NN_TILE_MASK = (1u << NN_REF_TILE) - 1u;
constexpr int NN_CAT_PER_THREAD = (NN_REF_TILE * NN_QK + NN_THREADS - 1) / NN_THREADS;   // staged codes per thread

__global__ __launch_bounds__(NN_THREADS) void nn_within_kernel(NnWithinArgs a) {
  __shared__ __attribute__((aligned(16))) double sc[NN_QC][NN_PAD_C];
  __shared__ __attribute__((aligned(16))) int sk[NN_QK][NN_PAD_K];
  const int tid = threadIdx.x;
  const int q = blockIdx.x * NN_QUERY_TILE + tid;
  const bool live = q < a.nq;
  const int chunk = blockIdx.y;
  const int j0 = chunk * NN_CHUNK_ROWS;
  const int j1 = min(a.nr, j0 + NN_CHUNK_ROWS);
  const int nbc = (a.n_cont + NN_QC - 1) / NN_QC, nbk = (a.n_cat + NN_QK - 1) / NN_QK;
  const double* qc = a.q_cont + (size_t)(live ? q : 0) * a.n_cont;
  const int* qk = a.q_cat + (size_t)(live ? q : 0) * a.n_cat;
  const double t2 = *a.t2;
  // (double)cnt > t2 exactly when cnt > kmax, for every int cnt >= 0 (t2 = NaN: never, as the comparison)
  const int kmax = !(t2 < 2147483647.0) ? 2147483647 : (t2 < 0.0 ? -1 : (int)floor(t2));

  double qv[NN_QC];
  int qi[NN_QK];
  auto load_cont = [&](int b) {
#pragma unroll
    for (int c = 0; c < NN_QC; ++c) {
      const int col = b * NN_QC + c;
      qv[c] = col < a.n_cont ? qc[col] : 0.0;
    }
  };
  auto load_cat = [&](int b) {
#pragma unroll
    for (int c = 0; c < NN_QK; ++c) {
      const int col = b * NN_QK + c;
      qi[c] = col < a.n_cat ? qk[col] : 0;
    }
  };
  load_cont(0);
  load_cat(0);
  // this thread's share of a staged block of codes (rows past the chunk and columns past the table: 0, not read)
  int pre[NN_CAT_PER_THREAD];
  auto fetch_cat = [&](int jt, int b) {
#pragma unroll
    for (int i = 0; i < NN_CAT_PER_THREAD; ++i) {
      const int e = tid + i * NN_THREADS;
      const int r = e / NN_QK, c = e - r * NN_QK;
      const int j = jt + r, col = b * NN_QK + c;
      pre[i] = (r < NN_REF_TILE && j < j1 && col < a.n_cat) ? a.r_cat[(size_t)j * a.n_cat + col] : 0;
    }
  };
  fetch_cat(j0, 0);

  int hit = -1;
  for (int jt = j0; jt < j1; jt += NN_REF_TILE) {
    // (3) also the barrier after which the previous tile's LDS may be overwritten
    if (__syncthreads_and(!live || hit >= 0)) break;
    const int left = j1 - jt;                                // rows of this tile that exist
    unsigned alive = (live && hit < 0) ? (left >= NN_REF_TILE ? NN_TILE_MASK : (1u << left) - 1u) : 0u;
    int cnt[NN_REF_TILE];
#pragma unroll
    for (int r = 0; r < NN_REF_TILE; ++r) cnt[r] = 0;
    // (1) mismatch counts of every categorical block, NN_WITHIN_GROUP columns at a time: once the smallest count of
    // every query of the wave is past kmax all its candidates are dead, and counting them further changes nothing
    bool counting = __any(alive != 0u);                       // (uniform over the wave)
    for (int b = 0; b < nbk; ++b) {
      const int nkb = min(NN_QK, a.n_cat - b * NN_QK);
      if (b > 0) __syncthreads();
      if (nbk > 1) load_cat(b);
      // the codes fetched while the previous block / tile was counted go to LDS; the next ones are requested now, so
      // their latency hides behind this block's counting (a pruned tile is little else than this staging)
#pragma unroll
      for (int i = 0; i < NN_CAT_PER_THREAD; ++i) {
        const int e = tid + i * NN_THREADS;
        if (e < NN_REF_TILE * NN_QK) sk[e % NN_QK][e / NN_QK] = pre[i];
      }
      if (b + 1 < nbk) fetch_cat(jt, b + 1);
      else fetch_cat(jt + NN_REF_TILE, 0);
      __syncthreads();
#pragma unroll
      for (int g = 0; g < NN_QK; g += NN_WITHIN_GROUP) {
        if (g < nkb && counting) {                            // (no barrier inside)
#pragma unroll
          for (int c = g; c < g + NN_WITHIN_GROUP; ++c) {
            if (c < nkb) {                                    // (uniform over the workgroup)
              const int x = qi[c];
#pragma unroll
              for (int r = 0; r < NN_REF_TILE; ++r) cnt[r] += (x != sk[c][r]) ? 1 : 0;
            }
          }
          int least = cnt[0];
#pragma unroll
          for (int r = 1; r < NN_REF_TILE; ++r) least = min(least, cnt[r]);
          counting = __any(alive != 0u && least <= kmax);
        }
      }
    }
#pragma unroll
    for (int r = 0; r < NN_REF_TILE; ++r)
      if (cnt[r] > kmax) alive &= ~(1u << r);
    if (nbc > 0) {
      if (!__syncthreads_or(alive != 0u)) continue;          // the whole tile is dead for this workgroup
    }
    double acc[NN_REF_TILE];
#pragma unroll
    for (int r = 0; r < NN_REF_TILE; ++r) acc[r] = 0.0;
    // (2) continuous columns in column order
    for (int b = 0; b < nbc; ++b) {
      const int ncb = min(NN_QC, a.n_cont - b * NN_QC);
      if (b > 0) __syncthreads();
      if (nbc > 1) load_cont(b);
      for (int e = tid; e < NN_REF_TILE * NN_QC; e += NN_THREADS) {
        const int r = e / NN_QC, c = e - r * NN_QC;
        const int j = jt + r, col = b * NN_QC + c;
        sc[c][r] = (j < j1 && col < a.n_cont) ? a.r_cont[(size_t)j * a.n_cont + col] : 0.0;
      }
      __syncthreads();
#pragma unroll
      for (int g = 0; g < NN_QC; g += NN_WITHIN_GROUP) {
        if (g < ncb && __any(alive != 0u)) {                  // (uniform over the wave; no barrier inside)
#pragma unroll
          for (int c = g; c < g + NN_WITHIN_GROUP; ++c) {
            if (c < ncb) {
              const double x = qv[c];
#pragma unroll
              for (int r = 0; r < NN_REF_TILE; ++r) {
                const double d = x - sc[c][r];
                acc[r] = fma(d, d, acc[r]);
              }
            }
          }
#pragma unroll
          for (int r = 0; r < NN_REF_TILE; ++r)
            if (acc[r] + (double)cnt[r] > t2) alive &= ~(1u << r);
        }
      }
    }
    // a candidate still alive went through every column: its distance is complete
#pragma unroll
    for (int r = NN_REF_TILE - 1; r >= 0; --r)
      if (((alive >> r) & 1u) && acc[r] + (double)cnt[r] <= t2) hit = jt + r;
  }
  if (live) a.part[(size_t)chunk * a.nq + q] = hit;
}

// chunk c holds indices below chunk c + 1's: the first chunk with a hit has the lowest
__global__ __launch_bounds__(NN_THREADS) void nn_within_merge_kernel(NnWithinArgs a) {
  const int q = blockIdx.x * NN_THREADS + threadIdx.x;
  if (q >= a.nq) return;
  int hit = -1;
  for (int c = 0; c < a.chunks && hit < 0; ++c) hit = a.part[(size_t)c * a.nq + q];
  a.near[q] = hit;
}

void launch_nn_within(NnWithinArgs a, hipStream_t stream) {
  require_unbatched("nn_within");
  if (a.nq < 0 || a.nr < 1 || a.n_cont < 0 || a.n_cat < 0 || a.n_cont + a.n_cat < 1)
    throw std::runtime_error("nn_within: table sizes");
  if (a.nq == 0) return;
  a.chunks = nn_chunks(a.nr);
  if (a.chunks > 65535) throw std::runtime_error("nn_within: too many reference rows");
  const unsigned tiles = (unsigned)((a.nq + NN_QUERY_TILE - 1) / NN_QUERY_TILE);
  hipLaunchKernelGGL(nn_within_kernel, dim3(tiles, (unsigned)a.chunks), dim3(NN_THREADS), 0, stream, a);
  hipLaunchKernelGGL(nn_within_merge_kernel, dim3(tiles), dim3(NN_THREADS), 0, stream, a);
}

// tgt[i] = -1 where near[i] >= 0 (cond_flag_kernel keeps no such row); stats += [rows, rows with a hit], counted
// with ballots and integer atomics, so the sums do not depend on the order the workgroups run in
__global__ __launch_bounds__(NN_THREADS) void guard_mark_kernel(const int* near, int* tgt, int n,
                                                                unsigned long long* stats) {
  __shared__ int wsum[NN_THREADS / WAVE];
  const int tid = threadIdx.x;
  const int i = blockIdx.x * NN_THREADS + tid;
  const bool rej = i < n && near[i] >= 0;
  if (rej) tgt[i] = -1;
  const unsigned long long b = __ballot(rej);
  if ((tid & (WAVE - 1)) == 0) wsum[tid / WAVE] = __popcll(b);
  __syncthreads();
  if (tid == 0) {
    int s = 0;
    for (int w = 0; w < NN_THREADS / WAVE; ++w) s += wsum[w];
    if (s) atomicAdd(&stats[1], (unsigned long long)s);
    if (blockIdx.x == 0) atomicAdd(&stats[0], (unsigned long long)n);
  }
}

void launch_guard_mark(const int* near, int* tgt, int n, int64_t* stats, hipStream_t stream) {
  require_unbatched("guard_mark");
  if (n < 0) throw std::runtime_error("guard_mark: row count");
  if (n == 0) return;
  hipLaunchKernelGGL(guard_mark_kernel, dim3((unsigned)((n + NN_THREADS - 1) / NN_THREADS)), dim3(NN_THREADS), 0,
                     stream, near, tgt, n, (unsigned long long*)stats);
}

// ============================================================================ shard merges (eval/fed_privacy.py)
// The answers of K shards over the same query rows folded into the answer over the union of the shards.  One thread
// per query row walks the shards in client order exactly as nn_merge_kernel walks chunks: strict <, so the lowest
// global index wins a tie, and a shard's second distance competes with the others' first (two shards holding a copy
// each give d1 = d2 = 0).  A shard without a candidate carries d1 = +inf and wins nothing.  A thread reads its row's
// three doubles, so a wave reads 64 x 24 contiguous bytes per shard.  by_client: per-wave ballots into LDS counters,
// then one integer atomic per (workgroup, shard) with a non-zero count: the sums do not depend on workgroup order.
__global__ __launch_bounds__(NN_THREADS) void nn_merge_shards_kernel(NnMergeShardsArgs a) {
  __shared__ int cnt[2 * NN_MAX_SHARDS];
  const int tid = threadIdx.x;
  const int q = blockIdx.x * NN_THREADS + tid;
  const bool live = q < a.n;
  const bool lead = (tid & (WAVE - 1)) == 0;
  if (tid < 2 * NN_MAX_SHARDS) cnt[tid] = 0;
  __syncthreads();
  double d1 = nn_inf(), d2 = nn_inf();
  int i1 = -1, owner = -1;
  for (int s = 0; s < a.k; ++s) {                 // (uniform: every thread of a wave reaches the ballot)
    double b1 = nn_inf(), b2 = nn_inf(), bi = -1.0;
    if (live) {
      const double* p = a.parts + ((size_t)s * a.n + q) * 3;
      b1 = p[0];
      b2 = p[1];
      bi = p[2];
    }
    if (b1 < d1 && bi >= 0.0) {
      d2 = b2 < d1 ? b2 : d1;
      d1 = b1;
      i1 = (int)(a.offsets[s] + (long long)bi);
      owner = s;
    } else if (b1 < d2) {
      d2 = b1;
    }
    const unsigned long long copies = __ballot(live && b1 == 0.0);
    if (lead && copies) atomicAdd(&cnt[NN_MAX_SHARDS + s], __popcll(copies));
  }
  for (int s = 0; s < a.k; ++s) {
    const unsigned long long mine = __ballot(owner == s);
    if (lead && mine) atomicAdd(&cnt[s], __popcll(mine));
  }
  if (live) {
    a.d1[q] = d1;
    a.d2[q] = d2;
    a.i1[q] = i1;
    a.owner[q] = owner;
  }
  __syncthreads();
  if (tid < 2 * NN_MAX_SHARDS) {
    const int row = tid / NN_MAX_SHARDS, s = tid - row * NN_MAX_SHARDS;
    if (s < a.k && cnt[tid]) atomicAdd(&a.by_client[(size_t)row * a.k + s], (unsigned long long)cnt[tid]);
  }
}

// (a kernel, not a memset: in a captured pass the counters are cleared by a kernel node ahead of the merge's)
__global__ __launch_bounds__(2 * NN_MAX_SHARDS) void nn_clear_counts_kernel(unsigned long long* by_client, int slots) {
  if ((int)threadIdx.x < slots) by_client[threadIdx.x] = 0ull;
}

void launch_nn_merge_shards(const NnMergeShardsArgs& a, hipStream_t stream) {
  require_unbatched("nn_merge_shards");
  if (a.k < 1 || a.k > NN_MAX_SHARDS) throw std::runtime_error("nn_merge_shards: 1..64 shards");
  if (a.n < 0) throw std::runtime_error("nn_merge_shards: row count");
  hipLaunchKernelGGL(nn_clear_counts_kernel, dim3(1), dim3(2 * NN_MAX_SHARDS), 0, stream, a.by_client, 2 * a.k);
  if (a.n == 0) return;
  hipLaunchKernelGGL(nn_merge_shards_kernel, dim3((unsigned)((a.n + NN_THREADS - 1) / NN_THREADS)), dim3(NN_THREADS),
                     0, stream, a);
}

// the shards hold ascending ranges of the global index: the first shard with a hit has the lowest
__global__ __launch_bounds__(NN_THREADS) void nn_within_merge_shards_kernel(const int* near, const int64_t* offsets,
                                                                            int k, int n, int* near_out, int* owner) {
  const int q = blockIdx.x * NN_THREADS + threadIdx.x;
  if (q >= n) return;
  int hit = -1, own = -1;
  for (int s = 0; s < k && own < 0; ++s) {
    const int h = near[(size_t)s * n + q];
    if (h >= 0) {
      hit = (int)(offsets[s] + (long long)h);
      own = s;
    }
  }
  near_out[q] = hit;
  owner[q] = own;
}

void launch_nn_within_merge_shards(const int* near, const int64_t* offsets, int k, int n, int* near_out, int* owner,
                                   hipStream_t stream) {
  require_unbatched("nn_within_merge_shards");
  if (k < 1 || k > NN_MAX_SHARDS) throw std::runtime_error("nn_within_merge_shards: 1..64 shards");
  if (n < 0) throw std::runtime_error("nn_within_merge_shards: row count");
  if (n == 0) return;
  hipLaunchKernelGGL(nn_within_merge_shards_kernel, dim3((unsigned)((n + NN_THREADS - 1) / NN_THREADS)),
                     dim3(NN_THREADS), 0, stream, near, offsets, k, n, near_out, owner);
}

// ============================================================================ table scores
// keys row 0: DCR = sqrt(d1); row 1: NNDR = sqrt(d1 / d2), 1 where d2 == 0, 0 where d2 = +inf.
// part[b] = the workgroup's smallest DCR, part[blocks + b] = its count of d1 == 0 (an integer, exact as fp64)
__global__ __launch_bounds__(NN_THREADS) void nn_stats_kernel(const double* d1, const double* d2, int n, double* keys,
                                                              int64_t ld, double* part, int blocks) {
  __shared__ double smin[NN_THREADS];
  __shared__ int scnt[NN_THREADS];
  const int tid = threadIdx.x;
  const int i = blockIdx.x * NN_THREADS + tid;
  double dcr = nn_inf();
  int zero = 0;
  if (i < n) {
    const double a = d1[i], b = d2[i];
    dcr = sqrt(a);
    keys[i] = dcr;
    keys[ld + i] = b == 0.0 ? 1.0 : (isinf(b) ? 0.0 : sqrt(a / b));
    zero = a == 0.0 ? 1 : 0;
  }
  smin[tid] = dcr;
  scnt[tid] = zero;
  __syncthreads();
  for (int s = NN_THREADS / 2; s > 0; s >>= 1) {
    if (tid < s) {
      smin[tid] = fmin(smin[tid], smin[tid + s]);
      scnt[tid] += scnt[tid + s];
    }
    __syncthreads();
  }
  if (tid == 0) {
    part[blockIdx.x] = smin[0];
    part[blocks + blockIdx.x] = (double)scnt[0];
  }
}

// numpy's linear interpolation (function_base.py _lerp) at virtual index q (n - 1) of an ascending row
__device__ __forceinline__ double nn_percentile(const double* x, int n, double q) {
  const double pos = (double)(n - 1) * q;
  int lo = (int)floor(pos);
  lo = min(max(lo, 0), n - 1);
  const int hi = min(lo + 1, n - 1);
  const double t = pos - (double)lo;
  const double u = x[lo], v = x[hi];
  if (u == v || t == 0.0) return u;       // (also keeps an infinite neighbour out of an exact position)
  const double diff = v - u;
  return t >= 0.5 ? v - diff * (1.0 - t) : u + diff * t;
}

__global__ __launch_bounds__(NN_THREADS) void nn_percentile_kernel(const double* keys, int64_t ld, int n,
                                                                   const double* part, int blocks, double* out) {
  __shared__ double smin[NN_THREADS];
  __shared__ long long scnt[NN_THREADS];
  const int tid = threadIdx.x;
  double m = nn_inf();
  long long z = 0;
  for (int b = tid; b < blocks; b += NN_THREADS) {
    m = fmin(m, part[b]);
    z += (long long)part[blocks + b];
  }
  smin[tid] = m;
  scnt[tid] = z;
  __syncthreads();
  for (int s = NN_THREADS / 2; s > 0; s >>= 1) {
    if (tid < s) {
      smin[tid] = fmin(smin[tid], smin[tid + s]);
      scnt[tid] += scnt[tid + s];
    }
    __syncthreads();
  }
  if (tid == 0) {
    out[0] = nn_percentile(keys, n, 0.05);
    out[1] = nn_percentile(keys + ld, n, 0.05);
    out[2] = smin[0];
    out[3] = (double)scnt[0] / (double)n;
  }
}

int nn_stats_blocks(int64_t n) {
  const int64_t b = (n + NN_THREADS - 1) / NN_THREADS;
  return b > 0 ? (int)b : 1;
}

void launch_nn_stats(const double* d1, const double* d2, int n, double* keys, int64_t ld, double* part,
                     hipStream_t stream) {
  require_unbatched("nn_stats");
  if (n < 1 || ld < n) throw std::runtime_error("nn_stats: row count / key row length");
  const int blocks = nn_stats_blocks(n);
  hipLaunchKernelGGL(nn_stats_kernel, dim3((unsigned)blocks), dim3(NN_THREADS), 0, stream, d1, d2, n, keys, ld, part,
                     blocks);
}

void launch_nn_percentiles(const double* keys, int64_t ld, int n, const double* part, double* out,
                           hipStream_t stream) {
  require_unbatched("nn_percentiles");
  if (n < 1 || ld < n) throw std::runtime_error("nn_percentiles: row count / key row length");
  hipLaunchKernelGGL(nn_percentile_kernel, dim3(1), dim3(NN_THREADS), 0, stream, keys, ld, n, part,
                     nn_stats_blocks(n), out);
}

}  // namespace fedtgan
