// Tree-utility evaluator (eval/forest_device.py DeviceForest): a histogram decision tree and a random forest with
// balanced class weights, grown level by level on the binned decoded table, and their confusion matrices on held-out
// rows, on the device.  The tree index is a grid dimension everywhere; the decision tree is the one-tree call without
// bootstrap and with every feature a candidate.
//
//  tree_pack_kernel       one pass over the row-major table: a byte per (feature, row) (binary search of the column's
//                         edges, or the clamped code), the target's code into y and its class counted by integer atomics
//  tree_weights_kernel    balanced class weights from the counts
//  tree_draw_kernel       bootstrap: draw j of tree t is row mulhi32(Philox word(t, j), n), counted by integer atomics
//  tree_init_kernel       one workgroup per tree: the root's row list (rows with a multiplicity and a valid class, in
//                         ascending order), its class counts, the first level
//  per level:
//  tree_split_kernel      a workgroup per (tree, live node of the level), looping over the features: the [bins, K]
//                         histogram of the node's rows in LDS (ds_add_u32), an integer prefix over the bins, the
//                         criterion per boundary, the argmax in (score, lowest bin) order; then the features that
//                         compete (forest: the m smallest Philox keys among those with a valid candidate), the node's
//                         best in (score, lowest feature) order, and the left child's class counts.  No histogram and
//                         no per-feature candidate goes to global memory.
//  tree_number_kernel     one workgroup per tree: children numbered by a scan over the level's nodes in order, their
//                         heap indices and class counts, the next level
//  tree_partition_kernel  a workgroup per (tree, split node): order-preserving partition of the node's segment into
//                         its children's, from one row list into the other
//  tree_predict_kernel    a held-out row walks every tree by its bins; hard vote of the one tree or soft vote summed in
//                         tree order; confusion matrix by integer atomics; tree_scores_kernel: accuracy, weighted F1
//
// Live nodes are a device-side range per tree; the grids are fixed and their workgroups loop over it, so the number of
// launches depends on max_depth alone.  Every float operation of the criterion and the votes is a single rounded fp64
// operation in a stated order: this file compiles without contraction.
#include "common.h"
#include "launch.h"

#include <stdexcept>
#include <string>

#pragma clang fp contract(off)

#include "eval_common.h"      // below the pragma: its inline functions compile without contraction here

namespace fedtgan {

constexpr int TREE_THREADS = 256;
constexpr int TREE_WAVES = TREE_THREADS / WAVE;
constexpr int TREE_PRED_ROWS = 64;
constexpr uint32_t TREE_STREAM_DRAW = 0x74726231u;      // Philox stream ids no other call site uses
constexpr uint32_t TREE_STREAM_FEAT = 0x74726632u;

static_assert(TREE_MAX_BINS <= TREE_THREADS, "a lane per boundary");
static_assert(TREE_MAX_CLASSES <= WAVE, "a lane per class");

#if FT_CHECKED
__device__ unsigned g_check_tree = 0u;
unsigned check_status_forest() {
  unsigned v = 0u, z = 0u;
  (void)hipMemcpyFromSymbol(&v, HIP_SYMBOL(g_check_tree), sizeof(v));
  (void)hipMemcpyToSymbol(HIP_SYMBOL(g_check_tree), &z, sizeof(z));
  return v;
}
#define TREE_CHECK(cond) FT_CHECK(&g_check_tree, cond, CHK_TREE_INDEX)
#else
unsigned check_status_forest() { return 0u; }
#define TREE_CHECK(cond) ((void)0)
#endif

__device__ __forceinline__ int tree_clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

__device__ __forceinline__ uint32_t tree_word(uint64_t seed, uint32_t stream, uint32_t w, uint32_t hi, uint32_t lo) {
  const uint4 c = make_uint4(lo, hi, stream, w);
  const uint2 k = make_uint2((uint32_t)seed, (uint32_t)(seed >> 32));
  return philox4x32_10(c, k).x;
}

static void tree_check_table(const TreeTable& t, const char* what) {
  if (t.n < 1 || t.ld < t.n || t.F < 1 || t.F > TREE_MAX_FEATURES || t.K < 1 || t.K > TREE_MAX_CLASSES)
    throw std::runtime_error(std::string(what) + ": table sizes");
}

// ============================================================================ pack
__global__ __launch_bounds__(TREE_THREADS) void tree_pack_kernel(TreePackArgs a) {
  const TreeTable& t = a.t;
  const long long i = (long long)blockIdx.x * TREE_THREADS + threadIdx.x;
  if (i >= (long long)t.n * a.n_cols) return;
  const long long r = i / a.n_cols;
  const int c = (int)(i - r * a.n_cols);
  const int k = a.kind[c], f = a.slot[c];
  const double v = a.values[i];
  if (k == TREE_TARGET) {
    const int code = code_or_overflow(v, t.K);
    t.y[r] = code;
    if (is_code(v, t.K)) atomicAdd(&t.counts[code], 1);
    return;
  }
  if (f < 0 || f >= t.F) return;
  int b;
  if (k == TREE_CAT) {
    b = code_or_overflow(v, a.card[f]);
  } else {                                                  // the number of edges below v; a NaN is above none
    const int e0 = tree_clampi(a.eoff[f], 0, a.n_edges), e1 = tree_clampi(a.eoff[f + 1], e0, a.n_edges);
    int lo = e0, hi = e1;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (v > a.edges[mid]) lo = mid + 1; else hi = mid;
    }
    b = lo - e0;
  }
  TREE_CHECK(b >= 0 && b < TREE_MAX_BINS);
  t.bins[(size_t)f * t.ld + r] = (uint8_t)tree_clampi(b, 0, TREE_MAX_BINS - 1);
}

__global__ __launch_bounds__(WAVE) void tree_weights_kernel(TreeTable t) {
  __shared__ int head[2];
  const int tid = threadIdx.x;
  if (tid == 0) class_head(t.counts, t.K, head[0], head[1]);
  __syncthreads();
  if (tid < t.K) t.cw[tid] = balanced_weight(head[0], head[1], t.counts[tid]);
}

void launch_tree_pack(const TreePackArgs& a, hipStream_t stream) {
  require_unbatched("tree_pack");
  const TreeTable& t = a.t;
  tree_check_table(t, "tree_pack");
  if (a.n_cols != t.F + 1) throw std::runtime_error("tree_pack: F + 1 must be n_cols");
  const long long cells = (long long)t.n * a.n_cols;
  if (cells >= (long long)INT32_MAX) throw std::runtime_error("tree_pack: table too large");
  (void)hipMemsetAsync(t.counts, 0, sizeof(int) * t.K, stream);
  hipLaunchKernelGGL(tree_pack_kernel, dim3((unsigned)((cells + TREE_THREADS - 1) / TREE_THREADS)), dim3(TREE_THREADS),
                     0, stream, a);
  hipLaunchKernelGGL(tree_weights_kernel, dim3(1), dim3(WAVE), 0, stream, t);
}

// ============================================================================ bootstrap
__global__ __launch_bounds__(TREE_THREADS) void tree_fill_kernel(int* mult, int64_t ldr, int n, int v) {
  const int j = blockIdx.x * TREE_THREADS + threadIdx.x;
  if (j < n) mult[(size_t)blockIdx.y * ldr + j] = v;
}

__global__ __launch_bounds__(TREE_THREADS) void tree_draw_kernel(int* mult, int64_t ldr, int n, uint64_t seed) {
  const int j = blockIdx.x * TREE_THREADS + threadIdx.x, t = blockIdx.y;
  if (j >= n) return;
  const uint32_t w = tree_word(seed, TREE_STREAM_DRAW, 0u, (uint32_t)t, (uint32_t)j);
  const int row = (int)(((uint64_t)w * (uint64_t)(uint32_t)n) >> 32);          // < n
  atomicAdd(&mult[(size_t)t * ldr + row], 1);
}

void launch_tree_bootstrap(int* mult, int T, int64_t ldr, int n, int bootstrap, uint64_t seed, hipStream_t stream) {
  require_unbatched("tree_bootstrap");
  if (T < 1 || T > 65535 || n < 1 || ldr < n) throw std::runtime_error("tree_bootstrap: sizes");
  const dim3 grid((unsigned)((n + TREE_THREADS - 1) / TREE_THREADS), (unsigned)T);
  hipLaunchKernelGGL(tree_fill_kernel, grid, dim3(TREE_THREADS), 0, stream, mult, ldr, n, bootstrap ? 0 : 1);
  if (bootstrap) hipLaunchKernelGGL(tree_draw_kernel, grid, dim3(TREE_THREADS), 0, stream, mult, ldr, n, seed);
}

// ============================================================================ growth
// exclusive rank of the set flags over the workgroup in thread order, and their number (every thread calls it)
__device__ __forceinline__ int tree_block_rank(bool flag, int* wsum, int& total) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const unsigned long long m = __ballot(flag);
  const int pre = __popcll(m & ((1ull << lane) - 1ull));
  __syncthreads();
  if (lane == 0) wsum[w] = __popcll(m);
  __syncthreads();
  int base = 0, all = 0;
#pragma unroll
  for (int i = 0; i < TREE_WAVES; ++i) {
    base += i < w ? wsum[i] : 0;
    all += wsum[i];
  }
  total = all;
  return base + pre;
}

__global__ __launch_bounds__(TREE_THREADS) void tree_init_kernel(TreeGrowArgs a) {
  __shared__ int wsum[TREE_WAVES];
  __shared__ int cnt[TREE_MAX_CLASSES];
  const TreeTable& t = a.t;
  const int tid = threadIdx.x, tr = blockIdx.x;
  const int* mult = a.mult + (size_t)tr * a.ldr;
  int* dst = a.rows + (size_t)tr * a.ldr;
  if (tid < TREE_MAX_CLASSES) cnt[tid] = 0;
  __syncthreads();
  int base = 0;
  for (int r0 = 0; r0 < t.n; r0 += TREE_THREADS) {
    const int r = r0 + tid;
    int m = 0, y = t.K;
    if (r < t.n) {
      m = mult[r];
      y = t.y[r];
    }
    const bool keep = m > 0 && y >= 0 && y < t.K;
    int total;
    const int k = tree_block_rank(keep, wsum, total);
    if (keep) {
      dst[base + k] = r;
      atomicAdd(&cnt[y], m);
    }
    base += total;
  }
  __syncthreads();
  const size_t node0 = (size_t)tr * a.cap;
  if (tid < t.K) a.counts[node0 * t.K + tid] = cnt[tid];
  if (tid == 0) {
    a.heap[node0] = 1;
    a.seg[node0 * 2] = 0;
    a.seg[node0 * 2 + 1] = base;
    a.level[tr * 4] = 0;
    a.level[tr * 4 + 1] = 1;
    a.level[tr * 4 + 2] = 1;
    a.level[tr * 4 + 3] = 0;
  }
}

// is candidate (sa, ba) better than (sb, bb)?  bins < 0: no candidate; a tie goes to the lower bin
__device__ __forceinline__ bool tree_better(double sa, int ba, double sb, int bb) {
  return ba >= 0 && (bb < 0 || sa > sb || (sa == sb && ba < bb));
}

__global__ __launch_bounds__(TREE_THREADS) void tree_split_kernel(TreeGrowArgs a, int L) {
  extern __shared__ __align__(16) unsigned char tree_smem[];
  unsigned* hist = (unsigned*)tree_smem;                         // [bins, K] of the feature at hand
  double* cs = (double*)(tree_smem + a.hist_bytes);              // [F] a feature's best score
  int* cb = (int*)(cs + a.t.F);                                  // [F] and its bin, -1 without a valid candidate
  unsigned* ck = (unsigned*)(cb + a.t.F);                        // [F] the feature's key at this node
  int* cc = (int*)(ck + a.t.F);                                  // [F] does it compete?
  __shared__ int tot[TREE_MAX_CLASSES], lc[TREE_MAX_CLASSES];
  __shared__ double w[TREE_MAX_CLASSES];
  __shared__ double rs[TREE_WAVES];
  __shared__ int rb[TREE_WAVES];
  __shared__ int info[4];
  const TreeTable& t = a.t;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, tr = blockIdx.y, K = t.K, F = t.F;
  const int lvl_start = a.level[tr * 4], lvl_count = a.level[tr * 4 + 1];
  const int* src = a.rows + ((size_t)(L & 1) * a.T + tr) * a.ldr;
  const int* mult = a.mult + (size_t)tr * a.ldr;
  if (tid < TREE_MAX_CLASSES) w[tid] = tid < K ? t.cw[tid] : 0.0;
  if (L >= a.max_depth) return;
  for (int item = blockIdx.x; item < lvl_count; item += gridDim.x) {
    const int node = tree_clampi(lvl_start + item, 0, a.cap - 1);
    TREE_CHECK(lvl_start + item < a.cap && item < a.lvl_cap);
    const size_t gnode = (size_t)tr * a.cap + node;
    __syncthreads();
    if (tid < TREE_MAX_CLASSES) tot[tid] = tid < K ? a.counts[gnode * K + tid] : 0;
    __syncthreads();
    if (tid == 0) {
      int ncls = 0;
      for (int c = 0; c < K; ++c) ncls += tot[c] > 0;
      info[0] = ncls;
    }
    __syncthreads();
    if (info[0] <= 1) continue;                                  // (uniform) pure or empty: a leaf
    int s0 = a.seg[gnode * 2], len = a.seg[gnode * 2 + 1];
    TREE_CHECK(s0 >= 0 && len >= 0 && (int64_t)s0 + len <= (int64_t)t.n);
    s0 = tree_clampi(s0, 0, t.n);
    len = tree_clampi(len, 0, t.n - s0);
    for (int f = 0; f < F; ++f) {
      const int nb = tree_clampi(a.nbins[f], 0, TREE_MAX_BINS);
      if (nb < 2 || nb * K * (int)sizeof(unsigned) > a.hist_bytes) {      // (uniform) a constant feature
        if (tid == 0) cb[f] = -1;
        continue;
      }
      for (int e = tid; e < nb * K; e += TREE_THREADS) hist[e] = 0u;
      __syncthreads();
      const uint8_t* col = t.bins + (size_t)f * t.ld;
      for (int i = tid; i < len; i += TREE_THREADS) {
        int r = src[s0 + i];
        TREE_CHECK(r >= 0 && r < t.n);
        r = tree_clampi(r, 0, t.n - 1);
        int b = col[r], y = t.y[r];
        TREE_CHECK(b < nb && y >= 0 && y < K);
        b = b < nb ? b : nb - 1;
        y = tree_clampi(y, 0, K - 1);
        atomicAdd(&hist[b * K + y], (unsigned)mult[r]);
      }
      __syncthreads();
      if (tid < K) {                                             // integer prefix over the bins, a lane per class
        unsigned run = 0u;
        for (int b = 0; b < nb; ++b) {
          run += hist[b * K + tid];
          hist[b * K + tid] = run;
        }
      }
      __syncthreads();
      double sc = 0.0;
      int bb = -1;
      for (int bd = tid; bd < nb - 1; bd += TREE_THREADS) {           // boundary bd: left = "bin <= bd"
        long long nl = 0, nr = 0;
        double TL = 0.0, QL = 0.0, TR = 0.0, QR = 0.0;
        for (int c = 0; c < K; ++c) {
          const int l = (int)hist[bd * K + c], r = tot[c] - l;
          nl += l;
          nr += r;
          const double ml = (double)l * w[c], mr = (double)r * w[c];
          TL = TL + ml;
          QL = QL + ml * ml;
          TR = TR + mr;
          QR = QR + mr * mr;
        }
        if (nl >= a.min_leaf && nr >= a.min_leaf && TL > 0.0 && TR > 0.0) {
          const double sn = QL / TL + QR / TR;
          if (tree_better(sn, bd, sc, bb)) {
            sc = sn;
            bb = bd;
          }
        }
      }
#pragma unroll
      for (int o = 1; o < WAVE; o <<= 1) {
        const double so = __shfl_xor(sc, o, WAVE);
        const int bo = __shfl_xor(bb, o, WAVE);
        if (tree_better(so, bo, sc, bb)) {
          sc = so;
          bb = bo;
        }
      }
      if (lane == 0) {
        rs[wv] = sc;
        rb[wv] = bb;
      }
      __syncthreads();
      if (tid == 0) {
        for (int i = 1; i < TREE_WAVES; ++i)
          if (tree_better(rs[i], rb[i], sc, bb)) {
            sc = rs[i];
            bb = rb[i];
          }
        cs[f] = sc;
        cb[f] = bb;
      }
    }
    __syncthreads();
    // the features that compete: all with a valid candidate, or (forest) the m of them with the smallest (key, f)
    const bool sub = a.m_feat < F;
    if (sub)
      for (int f = tid; f < F; f += TREE_THREADS)
        ck[f] = tree_word(a.seed, TREE_STREAM_FEAT, (uint32_t)a.heap[gnode], (uint32_t)tr, (uint32_t)f);
    __syncthreads();
    for (int f = tid; f < F; f += TREE_THREADS) {
      int ok = cb[f] >= 0;
      if (ok && sub) {
        int rank = 0;
        for (int g = 0; g < F; ++g)
          if (cb[g] >= 0 && (ck[g] < ck[f] || (ck[g] == ck[f] && g < f))) ++rank;
        ok = rank < a.m_feat;
      }
      cc[f] = ok;
    }
    __syncthreads();
    if (tid == 0) {
      int bf = -1, bbin = 0;
      double bs = 0.0;
      for (int f = 0; f < F; ++f)
        if (cc[f] && (bf < 0 || cs[f] > bs)) {                   // strictly greater: a tie stays with the lower feature
          bf = f;
          bs = cs[f];
          bbin = cb[f];
        }
      info[1] = bf;
      info[2] = bbin;
    }
    if (tid < TREE_MAX_CLASSES) lc[tid] = 0;
    __syncthreads();
    const int bf = info[1], bbin = info[2];
    if (bf < 0) continue;                                        // (uniform) no valid candidate: a leaf
    const uint8_t* col = t.bins + (size_t)bf * t.ld;
    for (int i = tid; i < len; i += TREE_THREADS) {
      const int r = tree_clampi(src[s0 + i], 0, t.n - 1);
      if ((int)col[r] <= bbin) atomicAdd(&lc[tree_clampi(t.y[r], 0, K - 1)], mult[r]);
    }
    __syncthreads();
    const int slot = item < a.lvl_cap ? item : a.lvl_cap - 1;
    if (tid < K) a.lcounts[((size_t)tr * a.lvl_cap + slot) * K + tid] = lc[tid];
    if (tid == 0) {
      a.feature[gnode] = bf;
      a.bin[gnode] = bbin;
    }
  }
}

__global__ __launch_bounds__(TREE_THREADS) void tree_number_kernel(TreeGrowArgs a) {
  __shared__ int wsum[TREE_WAVES];
  const int tid = threadIdx.x, tr = blockIdx.x, K = a.t.K;
  const int lvl_start = a.level[tr * 4], lvl_count = a.level[tr * 4 + 1];
  const int next = lvl_start + lvl_count;
  int base = 0;
  for (int i0 = 0; i0 < lvl_count; i0 += TREE_THREADS) {
    const int item = i0 + tid, node = tree_clampi(lvl_start + item, 0, a.cap - 1);
    const size_t gnode = (size_t)tr * a.cap + node;
    const bool split = item < lvl_count && a.feature[gnode] >= 0;
    int total;
    const int k = base + tree_block_rank(split, wsum, total);
    if (split) {
      const int l = next + 2 * k;
      TREE_CHECK(l + 1 < a.cap);
      if (l + 1 < a.cap) {
        const size_t gl = (size_t)tr * a.cap + l;
        const int g = a.heap[gnode];
        a.left[gnode] = l;
        a.heap[gl] = 2 * g;
        a.heap[gl + 1] = 2 * g + 1;
        const int slot = item < a.lvl_cap ? item : a.lvl_cap - 1;
        const int* lc = a.lcounts + ((size_t)tr * a.lvl_cap + slot) * K;
        for (int c = 0; c < K; ++c) {
          const int v = lc[c];
          a.counts[gl * K + c] = v;
          a.counts[(gl + 1) * K + c] = a.counts[gnode * K + c] - v;
        }
      } else {
        a.feature[gnode] = -1;                                   // (never: a tree of n rows has at most 2 n - 1 nodes)
      }
    }
    base += total;
  }
  __syncthreads();
  if (tid == 0) {
    int cnt = 2 * base;
    if (next + cnt > a.cap) cnt = a.cap > next ? ((a.cap - next) & ~1) : 0;
    a.level[tr * 4] = next;
    a.level[tr * 4 + 1] = cnt;
    a.level[tr * 4 + 2] = next + cnt;
    a.level[tr * 4 + 3] = lvl_start;                             // the level just split, for the partition
  }
}

// the level that tree_number_kernel just closed: nodes [level[3], level[0]); the children were numbered there
__global__ __launch_bounds__(TREE_THREADS) void tree_partition_kernel(TreeGrowArgs a, int L) {
  __shared__ int wsum[TREE_WAVES];
  const TreeTable& t = a.t;
  const int tid = threadIdx.x, tr = blockIdx.y;
  const int lvl_start = a.level[tr * 4 + 3], lvl_count = a.level[tr * 4] - lvl_start;
  const int* src = a.rows + ((size_t)(L & 1) * a.T + tr) * a.ldr;
  int* dst = a.rows + ((size_t)((L + 1) & 1) * a.T + tr) * a.ldr;
  for (int item = blockIdx.x; item < lvl_count; item += gridDim.x) {
    const int node = tree_clampi(lvl_start + item, 0, a.cap - 1);
    const size_t gnode = (size_t)tr * a.cap + node;
    int f = a.feature[gnode];
    if (f < 0) continue;                                         // (uniform)
    TREE_CHECK(f < t.F);
    f = tree_clampi(f, 0, t.F - 1);
    const int bbin = a.bin[gnode];
    int l = a.left[gnode];
    TREE_CHECK(l > node && l + 1 < a.cap);
    l = tree_clampi(l, 0, a.cap - 2);
    int s0 = a.seg[gnode * 2], len = a.seg[gnode * 2 + 1];
    TREE_CHECK(s0 >= 0 && len >= 0 && (int64_t)s0 + len <= (int64_t)t.n);
    s0 = tree_clampi(s0, 0, t.n);
    len = tree_clampi(len, 0, t.n - s0);
    const uint8_t* col = t.bins + (size_t)f * t.ld;
    int nleft = 0;
    for (int i0 = 0; i0 < len; i0 += TREE_THREADS) {             // how many entries go left
      const int i = i0 + tid;
      const bool go = i < len && (int)col[tree_clampi(src[s0 + i], 0, t.n - 1)] <= bbin;
      int total;
      (void)tree_block_rank(go, wsum, total);
      nleft += total;
    }
    int lbase = 0, rbase = 0;
    for (int i0 = 0; i0 < len; i0 += TREE_THREADS) {
      const int i = i0 + tid;
      const bool in = i < len;
      const int r = in ? tree_clampi(src[s0 + i], 0, t.n - 1) : 0;
      const bool go = in && (int)col[r] <= bbin;
      int total;
      const int k = tree_block_rank(go, wsum, total);
      if (in) {
        if (go) dst[s0 + lbase + k] = r;
        else dst[s0 + nleft + rbase + (tid - k)] = r;
      }
      lbase += total;
      rbase += (len - i0 < TREE_THREADS ? len - i0 : TREE_THREADS) - total;
    }
    if (tid == 0) {
      const size_t gl = (size_t)tr * a.cap + l;
      a.seg[gl * 2] = s0;
      a.seg[gl * 2 + 1] = nleft;
      a.seg[gl * 2 + 2] = s0 + nleft;
      a.seg[gl * 2 + 3] = len - nleft;
    }
  }
}

static size_t tree_split_lds(const TreeGrowArgs& a) { return (size_t)a.hist_bytes + (size_t)a.t.F * 20; }

void launch_tree_grow(const TreeGrowArgs& a, hipStream_t stream) {
  require_unbatched("tree_grow");
  tree_check_table(a.t, "tree_grow");
  if (a.T < 1 || a.T > 65535 || a.cap < 1 || a.lvl_cap < 1 || a.ldr < a.t.n || a.max_depth < 0 ||
      a.max_depth > TREE_MAX_DEPTH || a.min_leaf < 1 || a.m_feat < 1 || a.hist_bytes < 0 || (a.hist_bytes & 7) ||
      a.hist_bytes > TREE_MAX_BINS * TREE_MAX_CLASSES * (int)sizeof(unsigned))
    throw std::runtime_error("tree_grow: sizes");
  const int64_t want = a.max_depth >= 31 ? INT32_MAX : (1ll << a.max_depth);
  const int64_t lvl_need = want < a.t.n ? want : a.t.n;
  int64_t cap_need = a.max_depth >= 30 ? INT32_MAX : (2ll << a.max_depth) - 1;
  if (cap_need > 2ll * a.t.n - 1) cap_need = 2ll * a.t.n - 1;
  if (a.lvl_cap < lvl_need || a.cap < cap_need) throw std::runtime_error("tree_grow: node capacity");
  const size_t nodes = (size_t)a.T * a.cap;
  (void)hipMemsetAsync(a.feature, 0xFF, sizeof(int) * nodes, stream);
  (void)hipMemsetAsync(a.bin, 0, sizeof(int) * nodes, stream);
  (void)hipMemsetAsync(a.left, 0, sizeof(int) * nodes, stream);
  (void)hipMemsetAsync(a.heap, 0, sizeof(int) * nodes, stream);
  (void)hipMemsetAsync(a.counts, 0, sizeof(int) * nodes * a.t.K, stream);
  (void)hipMemsetAsync(a.seg, 0, sizeof(int) * nodes * 2, stream);
  hipLaunchKernelGGL(tree_init_kernel, dim3((unsigned)a.T), dim3(TREE_THREADS), 0, stream, a);
  const size_t lds = tree_split_lds(a);
  static size_t lds_set = 0;
  if (lds > lds_set) {
    if (hipFuncSetAttribute((const void*)tree_split_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) !=
        hipSuccess)
      throw std::runtime_error("tree_grow: the histogram does not fit the LDS");
    lds_set = lds;
  }
  for (int L = 0; L < a.max_depth; ++L) {
    int64_t live = L >= 30 ? a.t.n : (1ll << L);                 // most nodes a level can hold
    if (live > a.t.n) live = a.t.n;
    int64_t gx = 8192 / a.T;                                     // a fixed grid; its workgroups loop over the live nodes
    if (gx < 8) gx = 8;
    if (gx > live) gx = live;
    const dim3 grid((unsigned)gx, (unsigned)a.T);
    hipLaunchKernelGGL(tree_split_kernel, grid, dim3(TREE_THREADS), lds, stream, a, L);
    hipLaunchKernelGGL(tree_number_kernel, dim3((unsigned)a.T), dim3(TREE_THREADS), 0, stream, a);
    hipLaunchKernelGGL(tree_partition_kernel, grid, dim3(TREE_THREADS), 0, stream, a, L);
  }
}

// ============================================================================ predict
__global__ __launch_bounds__(TREE_PRED_ROWS) void tree_predict_kernel(TreePredictArgs a) {
  __shared__ double acc[TREE_PRED_ROWS][TREE_MAX_CLASSES + 1];
  __shared__ double w[TREE_MAX_CLASSES];
  const TreeTable& t = a.t;
  const int tid = threadIdx.x, K = t.K;
  w[tid] = tid < K ? t.cw[tid] : 0.0;
  __syncthreads();
  const int row = blockIdx.x * TREE_PRED_ROWS + tid;
  if (row >= t.n) return;
  const int yy = t.y[row];
  if (yy < 0 || yy >= K) return;
  for (int c = 0; c < K; ++c) acc[tid][c] = 0.0;
  for (int tr = 0; tr < a.T; ++tr) {
    const size_t base = (size_t)tr * a.cap;
    int node = 0;
    for (int step = 0; step <= TREE_MAX_DEPTH; ++step) {
      int f = a.feature[base + node];
      if (f < 0) break;
      TREE_CHECK(f < t.F);
      f = tree_clampi(f, 0, t.F - 1);
      const int b = t.bins[(size_t)f * t.ld + row];
      const int nx = a.left[base + node] + (b > a.bin[base + node] ? 1 : 0);
      TREE_CHECK(nx > node && nx < a.cap);
      node = tree_clampi(nx, 0, a.cap - 1);
    }
    const int* cnt = a.counts + (base + node) * K;
    if (a.soft) {
      double T = 0.0;
      for (int c = 0; c < K; ++c) T = T + (double)cnt[c] * w[c];
      if (T > 0.0)
        for (int c = 0; c < K; ++c) acc[tid][c] = acc[tid][c] + ((double)cnt[c] * w[c]) / T;
    } else {
      for (int c = 0; c < K; ++c) acc[tid][c] = (double)cnt[c] * w[c];
    }
  }
  int best = 0;
  double bv = acc[tid][0];
  for (int c = 1; c < K; ++c)
    if (acc[tid][c] > bv) {                                      // strictly greater: a tie stays with the lower class
      best = c;
      bv = acc[tid][c];
    }
  atomicAdd(&a.conf[yy * K + best], 1);
}

void launch_tree_predict(const TreePredictArgs& a, hipStream_t stream) {
  require_unbatched("tree_predict");
  tree_check_table(a.t, "tree_predict");
  if (a.T < 1 || a.cap < 1 || (!a.soft && a.T != 1)) throw std::runtime_error("tree_predict: sizes");
  (void)hipMemsetAsync(a.conf, 0, sizeof(int) * a.t.K * a.t.K, stream);
  hipLaunchKernelGGL(tree_predict_kernel, dim3((unsigned)((a.t.n + TREE_PRED_ROWS - 1) / TREE_PRED_ROWS)),
                     dim3(TREE_PRED_ROWS), 0, stream, a);
}

__global__ __launch_bounds__(WAVE) void tree_scores_kernel(const int* conf, int K, const double* real, double* out) {
  __shared__ int tp[TREE_MAX_CLASSES], rs[TREE_MAX_CLASSES], cs[TREE_MAX_CLASSES];
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
  if (tid == 0) confusion_scores(rs, cs, tp, K, real, out);
}

void launch_tree_scores(const int* conf, int K, const double* real, double* out, hipStream_t stream) {
  require_unbatched("tree_scores");
  if (K < 1 || K > TREE_MAX_CLASSES) throw std::runtime_error("tree_scores: classes");
  hipLaunchKernelGGL(tree_scores_kernel, dim3(1), dim3(WAVE), 0, stream, conf, K, real, out);
}

}  // namespace fedtgan
