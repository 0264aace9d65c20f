// torch.ops.fedtgan.* — PyTorch bindings of the gfx950 kernels and the native host code.
// Every op validates shapes/strides on the host before launching (a wrong shape must never
// reach a kernel) and launches on the current HIP stream so hipGraph capture works.
#include <ATen/ATen.h>
#include <c10/hip/HIPStream.h>
#include <torch/library.h>

#include <cstring>
#include <utility>
#include <string>
#include <vector>

#include "comm/rccl_comm.h"
#include "host/csv_writer.h"
#include "kernels/launch.h"

using at::Tensor;
using c10::optional;

namespace {

hipStream_t cur_stream() { return c10::hip::getCurrentHIPStream().stream(); }

void check_f32_2d(const Tensor& t, const char* name) {
  TORCH_CHECK(t.is_cuda(), name, " must be a GPU tensor");
  TORCH_CHECK(t.scalar_type() == at::kFloat, name, " must be float32");
  TORCH_CHECK(t.dim() == 2, name, " must be 2-D");
  TORCH_CHECK(t.size(1) <= 1 || t.stride(1) == 1, name, " must have unit column stride");
}

int ld_of(const Tensor& t) { return (int)(t.size(0) <= 1 ? std::max<int64_t>(t.size(1), 1) : t.stride(0)); }

// May a GEMM operand be read with 16-B loads?  Base 16-B aligned, ld % 4 == 0, and every row's
// contiguous extent rounded up to a multiple of 4 fits in ld and -- for the last row -- inside
// the tensor's storage (reads past the logical edge hit padding or the next row, which staging
// zeroes; never memory outside the storage).
bool vec_ok(const Tensor& t) {
  const int64_t ld = ld_of(t);
  const int64_t ext4 = (t.size(1) + 3) / 4 * 4;
  if (reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 != 0 || ld % 4 != 0 || ext4 > ld) return false;
  const int64_t storage = (int64_t)(t.storage().nbytes() / sizeof(float));
  return t.storage_offset() + (t.size(0) - 1) * ld + ext4 <= storage;
}

// bf16 GEMM operand (GemmArgs::bin): k-contiguous rows, 16-B aligned base, ld % 8 == 0, and every
// row's extent rounded up to 8 inside the storage (the kernel's 16-B loads are clamped to that).
void check_bf16_operand(const Tensor& t, const char* name) {
  TORCH_CHECK(t.is_cuda() && t.scalar_type() == at::kBFloat16 && t.dim() == 2, name, " must be a 2-D bf16 GPU tensor");
  TORCH_CHECK(t.size(1) <= 1 || t.stride(1) == 1, name, " must have unit column stride");
  const int64_t ld = ld_of(t);
  const int64_t ext8 = (t.size(1) + 7) / 8 * 8;
  TORCH_CHECK(reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0 && ld % 8 == 0 && ext8 <= ld, name,
              ": bf16 operands need a 16-B aligned base and a leading dimension divisible by 8 covering the row");
  const int64_t storage = (int64_t)(t.storage().nbytes() / 2);
  TORCH_CHECK(t.storage_offset() + (t.size(0) - 1) * ld + ext8 <= storage, name, ": rows padded to 8 must fit the storage");
}

uint16_t* hp(const Tensor& t) { return reinterpret_cast<uint16_t*>(t.data_ptr()); }

float* fp(const Tensor& t) { return t.data_ptr<float>(); }
const float* cfp(const Tensor& t) { return t.data_ptr<float>(); }
template <typename T>
T* optp(const optional<Tensor>& t) {
  return (t.has_value() && t->defined()) ? t->data_ptr<T>() : nullptr;
}
const uint64_t* ctr_ptr(const optional<Tensor>& t) {
  if (!t.has_value() || !t->defined()) return nullptr;
  TORCH_CHECK(t->scalar_type() == at::kLong && t->numel() >= 1 && t->is_cuda(), "rng_ctr must be a cuda int64 tensor");
  return reinterpret_cast<const uint64_t*>(t->data_ptr<int64_t>());
}

// pairing state of gemm(..., group): a GEMM held for launch_gemm_pair (group 1 / 2) or for the next
// adam_cs launch (group 3)
thread_local fedtgan::GemmArgs held{};
thread_local bool has_held = false;
thread_local hipStream_t held_stream = nullptr;
struct AdamHeld {
  fedtgan::GemmArgs g;
  hipStream_t stream;
  float* c;
  int64_t M, N, ldc;
  bool active;
};
thread_local AdamHeld g_adam_held{};
// a short-K weight gradient held for the next adam_cs launch (gemm(..., group=6)): launched just before it, with
// Adam in its own epilogue (launch_gemm_shortk_adam), its range cut out of the optimizer launch
thread_local AdamHeld g_adam_pre{};
// a chain tail (gemm(..., group=4)) waiting for its head (gemm(..., chain=True)); the head's launch copies
// the tail's arguments by value when it enqueues the reduction kernel
struct ChainTail {
  fedtgan::GemmArgs g;
  const void* a;
  int64_t M, K;
  bool active;
};
thread_local ChainTail g_chain_tail{};
thread_local fedtgan::GemmArgs g_chain_args{};

// The fused A-chain for the NEXT chain tail held by this thread (gemm_achain_next, launch.h GemmArgs::ach_*)
struct AchPending {
  Tensor out, ws, cnt;
  bool active;
};
thread_local AchPending g_ach{};

// drop every GEMM held by this thread (pairing, chain tail, Adam fusion) without launching it: called at
// the start of every step and when a step raises between a hold and its consumer, so a stale held GEMM
// (whose operand pointers may since have been freed) can never be launched or block the next step.
// Returns the number of holds that were dropped.
void pool_sample(const Tensor& pool, const Tensor& seg_off, const Tensor& mean, const Tensor& sd, int64_t seed) {
  TORCH_CHECK(pool.is_cuda() && pool.scalar_type() == at::kDouble && pool.is_contiguous(), "pool_sample: pool");
  TORCH_CHECK(seg_off.is_cuda() && seg_off.scalar_type() == at::kLong && seg_off.is_contiguous() && seg_off.numel() >= 2,
              "pool_sample: seg_off");
  const int64_t nseg = seg_off.numel() - 1;
  TORCH_CHECK(mean.is_cuda() && sd.is_cuda() && mean.scalar_type() == at::kDouble && sd.scalar_type() == at::kDouble &&
                  mean.is_contiguous() && sd.is_contiguous() && mean.numel() == nseg && sd.numel() == nseg,
              "pool_sample: mean / sd [nseg] fp64");
  fedtgan::PoolSampleArgs a{pool.data_ptr<double>(), seg_off.data_ptr<int64_t>(), mean.data_ptr<double>(),
                            sd.data_ptr<double>(), (int)nseg, pool.numel(), (uint64_t)seed};
  fedtgan::launch_pool_sample(a, cur_stream());
}

void row_center(const Tensor& x, const Tensor& shift) {
  TORCH_CHECK(x.is_cuda() && x.scalar_type() == at::kDouble && x.dim() == 2 && x.is_contiguous(), "row_center: x");
  TORCH_CHECK(shift.is_cuda() && shift.scalar_type() == at::kDouble && shift.numel() == x.size(0) && shift.is_contiguous(),
              "row_center: shift [rows] fp64");
  fedtgan::launch_row_center(x.data_ptr<double>(), shift.data_ptr<double>(), (int)x.size(0), x.size(1), cur_stream());
}

void csr_rows(const Tensor& opt, const Tensor& width, int64_t maxw, const Tensor& part, const Tensor& count,
              const Tensor& offset, const Tensor& rows, int64_t chunk) {
  TORCH_CHECK(opt.is_cuda() && opt.scalar_type() == at::kInt && opt.dim() == 2 && opt.stride(1) == 1, "csr_rows: opt");
  const int64_t n = opt.size(0), n_col = opt.size(1);
  const int64_t chunks = (n + chunk - 1) / std::max<int64_t>(chunk, 1);
  TORCH_CHECK(chunk > 0 && maxw > 0, "csr_rows: chunk / maxw");
  TORCH_CHECK(width.is_cuda() && width.scalar_type() == at::kInt && width.numel() == n_col, "csr_rows: width");
  TORCH_CHECK(part.is_cuda() && part.scalar_type() == at::kInt && part.is_contiguous() && part.numel() >= n_col * chunks * maxw,
              "csr_rows: part scratch [n_col, chunks, maxw] int32");
  for (const Tensor* t : {&count, &offset})
    TORCH_CHECK(t->is_cuda() && t->scalar_type() == at::kLong && t->is_contiguous() && t->numel() == n_col * maxw,
                "csr_rows: count / offset [n_col, maxw] int64");
  TORCH_CHECK(rows.is_cuda() && rows.scalar_type() == at::kLong && rows.is_contiguous() && rows.numel() == n * n_col,
              "csr_rows: rows [n_col * n] int64");
  fedtgan::CsrArgs a{opt.data_ptr<int>(), (int)opt.stride(0), width.data_ptr<int>(), (int)n, (int)n_col, (int)maxw,
                     (int)chunk, (int)chunks, part.data_ptr<int>(), count.data_ptr<int64_t>(), offset.data_ptr<int64_t>(),
                     rows.data_ptr<int64_t>()};
  fedtgan::launch_csr_rows(a, cur_stream());
}

// hipDeviceSynchronize + hipDeviceReset of the current device: the process' HIP queues, events and memory are
// torn down NOW, while every component attached to the runtime (e.g. rocprofv3's tool library) is still live,
// instead of by libamdhip64's exit-time destructor (bench.py --device-reset-at-exit; profiles/exit_r6.txt).
// Nothing may touch the device afterwards; returns the hipError_t of the reset.
int64_t device_reset() {
  (void)hipDeviceSynchronize();
  return (int64_t)hipDeviceReset();
}

int64_t reset_held() {
  const int64_t n = (has_held ? 1 : 0) + (g_adam_held.active ? 1 : 0) + (g_adam_pre.active ? 1 : 0) +
                    (g_chain_tail.active ? 1 : 0) +
                    (g_ach.active ? 1 : 0);
  g_ach = AchPending{};
  has_held = false;
  held_stream = nullptr;
  g_adam_held.active = false;
  g_adam_pre.active = false;
  g_chain_tail.active = false;
  return n;
}

// Batched clients (kernels/launch.h ClientBatch): the calling thread's launches from here on run K clients at
// once -- client c's buffers `stride` bytes after client c-1's (one arena, identical layouts), its Philox seed
// seed + c * seed_step; base = client 0's slab start (every pointer of a batched launch is checked to lie in
// [base, base + stride)).  k = 1 restores plain launches.  Returns the previous k.
int64_t set_client_batch(int64_t k, int64_t stride, int64_t seed_step, int64_t base) {
  TORCH_CHECK(k >= 1 && k <= 65535, "set_client_batch: k");
  TORCH_CHECK(k == 1 || (stride > 0 && stride % 256 == 0 && base != 0),
              "set_client_batch: a batched context needs a 256-B aligned slab stride and a base");
  fedtgan::ClientBatch& cb = fedtgan::client_batch();
  const int64_t prev = cb.k;
  cb.k = (int)k;
  cb.stride = k > 1 ? stride : 0;
  cb.seed_step = k > 1 ? (uint64_t)seed_step : 0;
  cb.base = k > 1 ? reinterpret_cast<const char*>(base) : nullptr;
  cb.xcd = k > 1 ? fedtgan::g_xcd_clients : 0;
  return prev;
}

// The next chain tail (gemm(..., group=4) with a head seed head_a = A1 [M, N1], weights W1 [N1, K1]) also forms
// out [M, K1] = (A1 W1) . MS0 in the chain launch, MS0 = the chain head's mask; ws = fp32 scratch of at least
// ceil(N1 / 64) * M * K1 elements, cnt = int32 counters, at least one per head row, all zero (kept zero by the kernel).
void gemm_achain_next(const Tensor& out, const Tensor& ws, const Tensor& cnt) {
  TORCH_CHECK(!g_ach.active, "gemm_achain_next: already pending");
  TORCH_CHECK(out.is_cuda() && out.scalar_type() == at::kFloat && out.dim() == 2 && out.stride(1) == 1,
              "gemm_achain_next: out fp32 [M, K] rows");
  TORCH_CHECK(ws.is_cuda() && ws.scalar_type() == at::kFloat && ws.is_contiguous(), "gemm_achain_next: ws fp32");
  TORCH_CHECK(cnt.is_cuda() && cnt.scalar_type() == at::kInt && cnt.is_contiguous(), "gemm_achain_next: cnt int32");
  TORCH_CHECK(fedtgan::client_batch().k == 1, "gemm_achain_next: one client");
  g_ach = AchPending{out, ws, cnt, true};
}

void gemm(const Tensor& a, const Tensor& b, const Tensor& c, bool ta, bool tb, double alpha, double beta,
          const optional<Tensor>& bias, int64_t epi, const optional<Tensor>& ms, double slope, double p_drop,
          const optional<Tensor>& ws, int64_t splitk, int64_t seed, const optional<Tensor>& rng_ctr, int64_t stream,
          const optional<Tensor>& bn_gamma, const optional<Tensor>& bn_beta, const optional<Tensor>& bn_rm,
          const optional<Tensor>& bn_rv, double bn_eps, bool f32, const optional<Tensor>& head_coef,
          const optional<Tensor>& head_v, const optional<Tensor>& head_a, int64_t tile, int64_t group,
          const optional<Tensor>& oh_w, const optional<Tensor>& oh_col, const optional<Tensor>& oh_opt,
          const optional<Tensor>& oh_off, bool oh_trans, const optional<Tensor>& bn_part, int64_t bn_rpg,
          const optional<Tensor>& tile_cnt, bool chain) {
  const bool bin = a.scalar_type() == at::kBFloat16;
  const bool cbf = c.scalar_type() == at::kBFloat16;
  // op(A) = A^T (weight gradients): the kernels' A^T instantiations carry no epilogue code
  TORCH_CHECK(!ta || epi == fedtgan::EPI_NONE, "gemm: op(A) = A^T takes the plain epilogue only (bias / alpha / beta)");
  if (bin) {
    TORCH_CHECK(!ta && tb && !f32, "gemm: bf16 operands need C = A B^T on the bf16 MFMA path");
    check_bf16_operand(a, "a");
    check_bf16_operand(b, "b");
  } else {
    check_f32_2d(a, "a");
    check_f32_2d(b, "b");
  }
  if (cbf) {
    TORCH_CHECK(c.is_cuda() && c.dim() == 2 && (c.size(1) <= 1 || c.stride(1) == 1), "gemm: c");
    TORCH_CHECK(beta == 0.0 && (epi == fedtgan::EPI_NONE || epi == fedtgan::EPI_RELU || epi == fedtgan::EPI_BN_EVAL_RELU) &&
                    !(head_a.has_value() && head_a->defined()) && !(bn_part.has_value() && bn_part->defined()) &&
                    group == 0,
                "gemm: a bf16 output takes beta = 0 and the NONE / RELU / BN_EVAL_RELU epilogues, unpaired");
  } else {
    check_f32_2d(c, "c");
  }
  const int64_t M = ta ? a.size(1) : a.size(0);
  const int64_t K = ta ? a.size(0) : a.size(1);
  const int64_t Kb = tb ? b.size(1) : b.size(0);
  const int64_t N = tb ? b.size(0) : b.size(1);
  TORCH_CHECK(K == Kb, "gemm: inner dims differ (", K, " vs ", Kb, ")");
  TORCH_CHECK(c.size(0) == M && c.size(1) == N, "gemm: c is ", c.sizes(), " expected [", M, ", ", N, "]");
  if (bias.has_value() && bias->defined()) TORCH_CHECK(bias->numel() == N && bias->is_contiguous(), "gemm: bias");
  fedtgan::GemmArgs g{};
  if (bin) {
    g.a16 = hp(a);
    g.b16 = hp(b);
    g.bin = 1;
  } else {
    g.a = cfp(a);
    g.b = cfp(b);
  }
  if (cbf) g.c16 = hp(c);
  else g.c = fp(c);
  g.bias = optp<float>(bias);
  g.M = (int)M; g.N = (int)N; g.K = (int)K;
  g.lda = ld_of(a); g.ldb = ld_of(b); g.ldc = ld_of(c);
  g.ta = ta; g.tb = tb;
  g.alpha = (float)alpha; g.beta = (float)beta;
  g.epi = (int)epi;
  g.slope = (float)slope; g.p_drop = (float)p_drop;
  if (epi == fedtgan::EPI_MASK || epi == fedtgan::EPI_LRELU_DROPOUT) {
    TORCH_CHECK(ms.has_value() && ms->defined(), "gemm: epilogue needs ms");
    check_f32_2d(*ms, "ms");
    TORCH_CHECK(ms->size(0) == M && ms->size(1) == N, "gemm: ms shape");
    g.ms = fp(*ms);
    g.ldms = ld_of(*ms);
  }
  if (epi == fedtgan::EPI_BN_EVAL_RELU) {
    TORCH_CHECK(bn_gamma.has_value() && bn_beta.has_value() && bn_rm.has_value() && bn_rv.has_value(), "gemm: bn");
    g.bn_gamma = optp<float>(bn_gamma); g.bn_beta = optp<float>(bn_beta);
    g.bn_rm = optp<float>(bn_rm); g.bn_rv = optp<float>(bn_rv);
    g.bn_eps = (float)bn_eps;
  }
  g.splitk = (int)std::max<int64_t>(splitk, 1);
  if (g.splitk > 1) {
    TORCH_CHECK(ws.has_value() && ws->defined() && ws->scalar_type() == at::kFloat, "gemm: split-K needs ws");
    // the launcher rounds K slices up to whole bursts, so the effective split count never exceeds splitk
    TORCH_CHECK(ws->numel() >= (int64_t)g.splitk * M * N, "gemm: workspace too small");
    g.ws = fp(*ws);
  }
  g.seed = (uint64_t)seed;
  g.rng_ctr = ctr_ptr(rng_ctr);
  g.rng_stream = (uint32_t)stream;
  g.f32 = f32 ? 1 : 0;
  TORCH_CHECK(tile == 32 || tile == 64 || tile == 128, "gemm: tile must be 32, 64 or 128");
  g.vec = bin ? 1 : ((vec_ok(a) && vec_ok(b)) ? 1 : 0);
  g.tile = (int)tile;
  if (head_a.has_value() && head_a->defined()) {
    TORCH_CHECK(epi == fedtgan::EPI_LRELU_DROPOUT, "gemm: the head seed needs the LeakyReLU+dropout epilogue");
    check_f32_2d(*head_a, "head_a");
    TORCH_CHECK(head_a->size(0) == M && head_a->size(1) == N, "gemm: head_a shape");
    TORCH_CHECK(head_coef.has_value() && head_coef->numel() == M && head_coef->is_contiguous() && head_v.has_value() &&
                    head_v->numel() == N && head_v->is_contiguous(), "gemm: head coef [M] / v [N]");
    g.head_a = fp(*head_a);
    g.ldha = ld_of(*head_a);
    g.head_coef = cfp(*head_coef);
    g.head_v = cfp(*head_v);
  }
  if (oh_w.has_value() && oh_w->defined()) {
    TORCH_CHECK(!ta, "gemm: the one-hot block needs row-major A (its rows carry the conditions)");
    TORCH_CHECK(alpha == 1.0, "gemm: the one-hot block needs alpha = 1 (it is folded into the accumulators)");
    check_f32_2d(*oh_w, "oh_w");
    TORCH_CHECK(oh_trans ? oh_w->size(1) == N : oh_w->size(0) == N, "gemm: oh_w must be [N, C] (or [C, N] transposed)");
    g.oh_trans = oh_trans ? 1 : 0;
    g.oh_c = (int)(oh_trans ? oh_w->size(0) : oh_w->size(1));
    TORCH_CHECK(oh_col.has_value() && oh_opt.has_value() && oh_off.has_value(), "gemm: one-hot needs col / opt / off");
    for (const auto* t : {&*oh_col, &*oh_opt, &*oh_off})
      TORCH_CHECK(t->is_cuda() && t->scalar_type() == at::kInt && t->is_contiguous(), "gemm: one-hot int32 tables");
    TORCH_CHECK(oh_col->numel() >= M && oh_opt->numel() >= M, "gemm: one-hot col / opt need M entries");
    g.oh_w = cfp(*oh_w);
    g.oh_ld = ld_of(*oh_w);
    g.oh_col = oh_col->data_ptr<int>();
    g.oh_opt = oh_opt->data_ptr<int>();
    g.oh_off = oh_off->data_ptr<int>();
  }
  if (bn_part.has_value() && bn_part->defined()) {
    TORCH_CHECK(!ta && !bin && !cbf && epi == fedtgan::EPI_NONE && alpha == 1.0 && beta == 0.0 && g.splitk == 1 &&
                    (tile == 32 || tile == 64) && group == 0 && g.vec,
                "gemm: BN partials need a plain unsplit C = A op(B) + bias on 32/64 tiles with 16-B operands");
    const int64_t tiles = (M + tile - 1) / tile;
    TORCH_CHECK(bn_part->is_cuda() && bn_part->scalar_type() == at::kFloat && bn_part->is_contiguous() &&
                    bn_part->numel() >= tiles * 6 * N, "gemm: bn_part must hold [m_tiles, 2, 3, N] floats");
    TORCH_CHECK(bn_rpg >= 1 && bn_rpg <= M, "gemm: bn_rpg");
    g.bn_part = fp(*bn_part);
    g.bn_rpg = (int)bn_rpg;
  }
  if (tile_cnt.has_value() && tile_cnt->defined() && g.splitk > 1) {
    // one arrival counter per output tile, all zero (the reducing workgroup re-zeroes its tile's)
    const int64_t tiles = ((M + tile - 1) / tile) * ((N + tile - 1) / tile);
    TORCH_CHECK(tile_cnt->is_cuda() && tile_cnt->scalar_type() == at::kInt && tile_cnt->is_contiguous() &&
                    tile_cnt->numel() >= tiles, "gemm: tile_cnt must hold one int32 per output tile");
    g.tile_cnt = reinterpret_cast<unsigned*>(tile_cnt->data_ptr<int>());
  }
  if (group == 4) {
    // the tail of a chain (held for the next gemm(..., chain=True), whose output is this GEMM's A): its
    // own epilogue, computed row by row in the head's reduction launch (chain_epilogue_kernel)
    TORCH_CHECK(!g_chain_tail.active, "gemm: a chain tail is already held");
    TORCH_CHECK(!ta && tb && !bin && !cbf && !g.oh_w && !g.bn_part && beta == 0.0 && K <= 1024 && K % 16 == 0 &&
                    ld_of(b) % 4 == 0 &&
                    (reinterpret_cast<uintptr_t>(b.data_ptr()) & 15) == 0,
                "gemm: a chain tail is C = A B^T with fp32 16-B aligned B rows (ld % 4 == 0), K <= 1024, K % 16 == 0, "
                "no one-hot block / BN partials");
    g.splitk = 1;
    if (g_ach.active) {
      AchPending q = g_ach;
      g_ach = AchPending{};
      TORCH_CHECK(g.head_a && epi == fedtgan::EPI_LRELU_DROPOUT, "gemm: the fused A-chain needs a tail with a head seed");
      TORCH_CHECK(q.out.size(0) == M && q.out.size(1) == K && q.ws.numel() >= ((N + 63) / 64) * M * K && q.cnt.numel() >= M,
                  "gemm: fused A-chain out [M, K] / ws [ceil(N / 64), M, K] / cnt [M]");
      g.ach_out = q.out.data_ptr<float>();
      g.ld_ach = (int)q.out.stride(0);
      g.ach_ws = q.ws.data_ptr<float>();
      g.ach_cnt = reinterpret_cast<unsigned*>(q.cnt.data_ptr<int>());
    }
    g_chain_tail = ChainTail{g, a.data_ptr(), (int64_t)M, (int64_t)K, true};
    return;
  }
  TORCH_CHECK(!g_ach.active, "gemm: gemm_achain_next is pending but this GEMM is no chain tail");
  if (chain) {
    TORCH_CHECK(g_chain_tail.active && group != 1, "gemm: chain=True needs a tail held with group=4 (and no group 1)");
    const ChainTail& t = g_chain_tail;
    TORCH_CHECK(t.a == c.data_ptr() && t.M == M && t.K == N && !cbf,
                "gemm: the chain tail's A must be this GEMM's fp32 output (same rows, K = N)");
    g_chain_args = t.g;
    g_chain_tail.active = false;
    g.chain = &g_chain_args;
  } else {
    TORCH_CHECK(!g_chain_tail.active || group == 1, "gemm: a chain tail is held; the next unpaired GEMM must be its head");
  }
  // group 1: hold this GEMM; group 2: launch it together with the held one (launch_gemm_pair: the two
  // must be independent -- neither reads what the other writes); group 3: hold it for the next
  // adam_cs launch on this stream (a weight gradient inside that optimizer's gradient buffer: the
  // two become one launch, gemm_adam_kernel); group 0: launch now
  const hipStream_t hs = cur_stream();
  if (group == 6 || group == 7) {
    // group 7: the same, with the gradient itself stored too (GemmArgs::adam_grad)
    TORCH_CHECK(!g_adam_pre.active, "gemm: a short-K GEMM is already held for the Adam launch");
    g.adam_grad = group == 7 ? 1 : 0;
    TORCH_CHECK(ta && !tb && epi == fedtgan::EPI_NONE && alpha == 1.0 && beta == 0.0 && !g.bias && !g.oh_w && !g.head_a &&
                    !g.bn_part && !cbf && !bin && !chain && fedtgan::client_batch().k == 1,
                "gemm: group 6 holds a plain C = A^T B weight gradient of one client (short-K Adam)");
    g_adam_pre = AdamHeld{g, hs, c.data_ptr<float>(), (int64_t)M, (int64_t)N, (int64_t)g.ldc, true};
    return;
  }
  if (group == 3) {
    TORCH_CHECK(!g_adam_held.active, "gemm: a GEMM is already held for the Adam launch");
    TORCH_CHECK(epi == fedtgan::EPI_NONE && beta == 0.0 && !g.bias && !g.oh_w && !g.head_a && !g.bn_part && !cbf && !bin,
                "gemm: a GEMM fused with Adam takes a plain epilogue (no bias / beta / one-hot / head / BN partials)");
    g_adam_held = AdamHeld{g, hs, c.data_ptr<float>(), (int64_t)M, (int64_t)N, (int64_t)g.ldc, true};
    return;
  }
  if (group == 1) {
    TORCH_CHECK(!has_held, "gemm: a GEMM is already held for pairing");
    held = g;
    has_held = true;
    held_stream = hs;
    return;
  }
  if (group == 2) {
    TORCH_CHECK(has_held && held_stream == hs, "gemm: group 2 needs a held GEMM on the same stream");
    TORCH_CHECK(!(held.splitk > 1 && g.splitk > 1 && held.ws == g.ws), "gemm: paired split-K GEMMs share a workspace");
    TORCH_CHECK(!(held.tile_cnt && g.tile_cnt && held.tile_cnt == g.tile_cnt), "gemm: paired GEMMs share tile counters");
    has_held = false;
    fedtgan::launch_gemm_pair(held, g, hs);
    return;
  }
  TORCH_CHECK(!has_held, "gemm: a held GEMM was never paired");
  fedtgan::launch_gemm(g, hs);
}

void sample(const Tensor& h, int64_t zc, int64_t cc, int64_t E, const optional<Tensor>& xf, const optional<Tensor>& xr,
            int64_t Dd, const Tensor& cdf, const Tensor& cond_off, const Tensor& cond_w, const optional<Tensor>& row_off,
            const optional<Tensor>& row_cnt, const optional<Tensor>& rows, const optional<Tensor>& data,
            const optional<Tensor>& col, const optional<Tensor>& opt, const optional<Tensor>& step_bump,
            const optional<Tensor>& step_bump2, const optional<Tensor>& metrics, bool zero_metrics, int64_t seed,
            const Tensor& rng_ctr, int64_t stream, int64_t draws, int64_t draw_h, int64_t draw_x, int64_t draw_col) {
  fedtgan::SampleArgs a{};
  const bool h16 = h.scalar_type() == at::kBFloat16;
  a.B = (int)h.size(0);
  a.E = (int)E;
  a.Dd = (int)Dd;
  a.n_col = (int)cond_w.numel();
  a.maxw = cdf.dim() == 2 ? (int)cdf.size(1) : 0;
  TORCH_CHECK(cond_off.scalar_type() == at::kInt && cond_w.scalar_type() == at::kInt, "sample: int32 tables");
  TORCH_CHECK(cdf.is_contiguous() && cdf.scalar_type() == at::kFloat, "sample: cdf");
  if (h16) {
    // generation into a bf16 activation buffer: only z is written (the condition goes to col / opt)
    TORCH_CHECK(h.is_cuda() && h.dim() == 2 && (h.size(1) <= 1 || h.stride(1) == 1), "sample: h");
    TORCH_CHECK(zc >= 0 && zc + E <= h.size(1), "sample: z columns");
    TORCH_CHECK(!(xf.has_value() && xf->defined()) && !(xr.has_value() && xr->defined()),
                "sample: a bf16 h takes no D-input blocks");
    TORCH_CHECK(a.n_col == 0 || (col.has_value() && opt.has_value()), "sample: a bf16 h needs col / opt outputs");
    a.h16 = hp(h); a.ldh16 = ld_of(h); a.zc16 = (int)zc;
  } else {
    check_f32_2d(h, "h");
    a.C = (int)(h.size(1) - cc);
    TORCH_CHECK(zc + E <= h.size(1) && cc <= h.size(1), "sample: column ranges");
    a.h = fp(h); a.ldh = ld_of(h); a.zc = (int)zc; a.cc = (int)cc;
  }
  a.ldx = 0;
  if (xf.has_value() && xf->defined()) {
    check_f32_2d(*xf, "xf");
    TORCH_CHECK(xf->size(0) == a.B && xf->size(1) == Dd + a.C, "sample: xf shape");
    a.xf = fp(*xf); a.ldx = ld_of(*xf);
  }
  if (xr.has_value() && xr->defined()) {
    check_f32_2d(*xr, "xr");
    // the real block may cover only the leading rows (a D-phase batch drawn together with a G-phase one)
    TORCH_CHECK(xr->size(0) >= 1 && xr->size(0) <= a.B && xr->size(1) == Dd + a.C, "sample: xr shape");
    a.n_real = (int)xr->size(0);
    TORCH_CHECK(row_off.has_value() && row_cnt.has_value() && rows.has_value() && data.has_value(), "sample: tables");
    TORCH_CHECK(data->size(1) == Dd && data->is_contiguous(), "sample: data");
    a.xr = fp(*xr);
    if (a.ldx == 0) a.ldx = ld_of(*xr);
    TORCH_CHECK(ld_of(*xr) == a.ldx, "sample: xf/xr strides differ");
    a.row_off = optp<int64_t>(row_off); a.row_cnt = optp<int64_t>(row_cnt); a.rows = optp<int64_t>(rows);
    a.n_entries = rows->numel();
    a.data = data->data_ptr<float>();
    a.n_rows = (int)data->size(0);
  }
  a.cdf = cfp(cdf);
  a.cond_off = cond_off.data_ptr<int>();
  a.cond_w = cond_w.data_ptr<int>();
  for (const auto* t : {&col, &opt})
    if (t->has_value() && (*t)->defined())
      TORCH_CHECK((*t)->is_cuda() && (*t)->scalar_type() == at::kInt && (*t)->is_contiguous() && (*t)->numel() >= a.B,
                  "sample: col / opt must be int32 with one entry per row");
  a.col = optp<int>(col);
  a.opt = optp<int>(opt);
  a.step_bump = optp<float>(step_bump);
  a.step_bump2 = optp<float>(step_bump2);
  a.metrics = optp<float>(metrics);
  a.zero_metrics = zero_metrics ? 1 : 0;
  a.seed = (uint64_t)seed;
  a.rng_ctr = ctr_ptr(rng_ctr);
  a.rng_stream = (uint32_t)stream;
  a.draws = (int)std::max<int64_t>(draws, 1);
  if (a.draws > 1) {
    // every draw's buffers must lie inside their tensors' storage: draw k writes at the same views + k x stride
    TORCH_CHECK(!h16 && draw_h > 0 && draw_col > 0 && (draw_x > 0 || !(xf.has_value() && xf->defined())),
                "sample: multi-step draws need fp32 h and positive strides");
    auto fits = [&](const Tensor& t, int64_t stride, const char* what) {
      const int64_t span = (t.size(0) - 1) * t.stride(0) + (t.dim() > 1 ? t.size(1) : 1);
      const int64_t last = t.storage_offset() + (a.draws - 1) * stride + span;
      TORCH_CHECK(last * (int64_t)t.element_size() <= (int64_t)t.storage().nbytes(), "sample: draw ", a.draws - 1,
                  " of ", what, " runs past its storage");
    };
    fits(h, draw_h, "h");
    if (xf.has_value() && xf->defined()) fits(*xf, draw_x, "xf");
    if (xr.has_value() && xr->defined()) fits(*xr, draw_x, "xr");
    for (const auto* t : {&col, &opt})
      if (t->has_value() && (*t)->defined()) fits(**t, draw_col, "col / opt");
    for (const auto* t : {&step_bump, &step_bump2})
      if (t->has_value() && (*t)->defined())
        TORCH_CHECK((*t)->numel() >= a.draws && (*t)->is_contiguous(), "sample: per-step counters need [draws]");
    if (metrics.has_value() && metrics->defined())
      TORCH_CHECK(metrics->numel() >= 4 * a.draws && metrics->is_contiguous(), "sample: metrics need [draws, 4]");
    a.draw_h = draw_h;
    a.draw_x = draw_x;
    a.draw_col = draw_col;
  }
  fedtgan::launch_sample(a, cur_stream());
}

fedtgan::SpanTables spans_of(const Tensor& start, const Tensor& width, const Tensor& kind, const Tensor& cidx,
                             const Tensor& packed, int64_t dim) {
  TORCH_CHECK(start.scalar_type() == at::kInt && width.scalar_type() == at::kInt && kind.scalar_type() == at::kInt &&
                  cidx.scalar_type() == at::kInt && packed.scalar_type() == at::kInt,
              "span tables must be int32");
  TORCH_CHECK(start.numel() == width.numel() && start.numel() == kind.numel() && start.numel() == cidx.numel(),
              "span tables: sizes");
  const int S = (int)start.numel();
  TORCH_CHECK(packed.is_contiguous() && packed.numel() == fedtgan::span_packed_len((int)dim, S) &&
                  reinterpret_cast<uintptr_t>(packed.data_ptr()) % 16 == 0,
              "span tables: packed table must hold [elem | kind | start | width | cidx] padded to 4 ints");
  fedtgan::SpanTables sp{start.data_ptr<int>(), width.data_ptr<int>(), kind.data_ptr<int>(), cidx.data_ptr<int>(),
                         packed.data_ptr<int>(), S, (int)dim};
  TORCH_CHECK(fedtgan::activation_smem_bytes(sp) <= 160 * 1024, "activation: row image exceeds the 160 KiB LDS");
  return sp;
}

void activate(const Tensor& logits, const Tensor& out, const Tensor& start, const Tensor& width, const Tensor& kind,
              const Tensor& cidx, const Tensor& elem, double tau, int64_t seed, const Tensor& rng_ctr, int64_t stream,
              const optional<Tensor>& slerp_real, const optional<Tensor>& slerp_out, int64_t slerp_cols,
              int64_t slerp_stream) {
  check_f32_2d(logits, "logits");
  check_f32_2d(out, "out");
  TORCH_CHECK(out.size(0) == logits.size(0) && out.size(1) >= logits.size(1), "activate: shapes");
  fedtgan::SlerpFuse sl{};
  if (slerp_real.has_value() && slerp_real->defined()) {
    TORCH_CHECK(slerp_out.has_value() && slerp_out->defined(), "activate: slerp needs an output");
    check_f32_2d(*slerp_real, "slerp real");
    check_f32_2d(*slerp_out, "slerp out");
    TORCH_CHECK(ld_of(*slerp_real) == ld_of(*slerp_out) && ld_of(*slerp_real) == ld_of(out), "activate: slerp strides");
    TORCH_CHECK(slerp_real->size(0) >= 1 && slerp_real->size(0) <= out.size(0) &&
                    slerp_out->size(0) == slerp_real->size(0) &&
                    slerp_real->size(1) == slerp_cols && slerp_out->size(1) == slerp_cols &&
                    slerp_cols >= logits.size(1) && slerp_cols <= ld_of(out), "activate: slerp shapes");
    sl.real = cfp(*slerp_real);
    sl.out = fp(*slerp_out);
    sl.ld = ld_of(out);
    sl.cols = (int)slerp_cols;
    sl.rows = (int)slerp_real->size(0);
    sl.stream = (uint32_t)slerp_stream;
  }
  fedtgan::launch_activate(cfp(logits), ld_of(logits), fp(out), ld_of(out), (int)logits.size(0),
                           spans_of(start, width, kind, cidx, elem, logits.size(1)), (float)tau, (uint64_t)seed, ctr_ptr(rng_ctr),
                           (uint32_t)stream, sl, cur_stream());
}

void act_bwd_ce(const Tensor& dact, const Tensor& act, const Tensor& logits, const Tensor& start, const Tensor& width,
                const Tensor& kind, const Tensor& cidx, const Tensor& elem, const Tensor& col, const Tensor& opt,
                const Tensor& dlogits, const Tensor& loss, double tau) {
  check_f32_2d(dact, "dact");
  check_f32_2d(act, "act");
  check_f32_2d(logits, "logits");
  check_f32_2d(dlogits, "dlogits");
  const int64_t rows = logits.size(0);
  TORCH_CHECK(dact.size(0) == rows && act.size(0) == rows && dlogits.size(0) == rows && col.numel() >= rows,
              "act_bwd_ce: rows");
  // loss with one entry per row: per-row terms (summed later), else accumulated into loss[0]
  const bool per_row = rows > 1 && loss.numel() == rows;
  TORCH_CHECK(per_row || loss.numel() >= 1, "act_bwd_ce: loss");
  fedtgan::launch_act_bwd_ce(cfp(dact), ld_of(dact), cfp(act), ld_of(act), cfp(logits), ld_of(logits),
                             spans_of(start, width, kind, cidx, elem, logits.size(1)), col.data_ptr<int>(), opt.data_ptr<int>(), fp(dlogits),
                             ld_of(dlogits), (int)rows, (float)tau, fp(loss), per_row ? 1 : 0, cur_stream());
}

void slerp(const Tensor& real, const Tensor& fake, const Tensor& out, int64_t seed, const Tensor& rng_ctr,
           int64_t stream) {
  check_f32_2d(real, "real");
  check_f32_2d(fake, "fake");
  check_f32_2d(out, "out");
  TORCH_CHECK(real.sizes() == fake.sizes() && real.sizes() == out.sizes(), "slerp: shapes");
  TORCH_CHECK(ld_of(real) == ld_of(fake) && ld_of(real) == ld_of(out), "slerp: strides");
  fedtgan::launch_slerp(cfp(real), cfp(fake), fp(out), (int)real.size(0), (int)real.size(1), ld_of(real),
                        (uint64_t)seed, ctr_ptr(rng_ctr), (uint32_t)stream, cur_stream());
}

void gp_scale(const Tensor& g, const Tensor& out, double lam, const Tensor& loss, const optional<Tensor>& ws) {
  check_f32_2d(g, "g");
  check_f32_2d(out, "out");
  TORCH_CHECK(g.sizes() == out.sizes(), "gp_scale: shapes");
  const bool per_row = g.size(0) > 1 && loss.numel() == g.size(0);   // per-pack terms, summed later
  float* wsp = nullptr;
  int64_t wsn = 0;
  if (ws.has_value()) {
    TORCH_CHECK(ws->is_cuda() && ws->scalar_type() == at::kFloat && ws->is_contiguous(), "gp_scale: float32 workspace");
    wsp = fp(*ws);
    wsn = ws->numel();
  }
  fedtgan::launch_gp_scale(cfp(g), ld_of(g), fp(out), ld_of(out), (int)g.size(0), (int)g.size(1), (float)lam,
                           fp(loss), per_row ? 1 : 0, wsp, wsn, cur_stream());
}

void onehot_wgrad(const std::vector<Tensor>& dy, const std::vector<Tensor>& w, const Tensor& col, const Tensor& opt,
                  const Tensor& cond_off, int64_t zero) {
  TORCH_CHECK(dy.size() == w.size() && !dy.empty() && dy.size() <= 4, "onehot_wgrad: 1-4 (dy, w) jobs");
  TORCH_CHECK(col.scalar_type() == at::kInt && opt.scalar_type() == at::kInt && cond_off.scalar_type() == at::kInt &&
                  col.is_contiguous() && opt.is_contiguous() && cond_off.is_contiguous(),
              "onehot_wgrad: int32 contiguous col / opt / cond_off");
  fedtgan::OnehotWBatch bt{};
  bt.n_jobs = (int)dy.size();
  bt.B = (int)dy[0].size(0);
  TORCH_CHECK(col.numel() >= bt.B && opt.numel() >= bt.B, "onehot_wgrad: col / opt rows");
  for (size_t j = 0; j < dy.size(); ++j) {
    check_f32_2d(dy[j], "dy");
    check_f32_2d(w[j], "w");
    TORCH_CHECK(dy[j].size(0) == bt.B && dy[j].size(1) == w[j].size(1), "onehot_wgrad: shapes");
    bt.jobs[j] = fedtgan::OnehotWJob{cfp(dy[j]), fp(w[j]), (int)ld_of(dy[j]), (int)ld_of(w[j]), (int)w[j].size(1)};
  }
  bt.col = col.data_ptr<int>();
  bt.opt = opt.data_ptr<int>();
  bt.cond_off = cond_off.data_ptr<int>();
  fedtgan::launch_onehot_wgrad(bt, (int)zero, cur_stream());
}

void d_head(const Tensor& d, const Tensor& ms, const Tensor& v, const Tensor& e, const Tensor& coef,
            const Tensor& wloss, const Tensor& y, const Tensor& a, const Tensor& loss) {
  check_f32_2d(d, "d");
  check_f32_2d(ms, "ms");
  check_f32_2d(a, "a");
  const int64_t rows = d.size(0), cols = d.size(1);
  TORCH_CHECK(ms.sizes() == d.sizes() && a.sizes() == d.sizes() && v.numel() == cols && coef.numel() >= rows &&
                  wloss.numel() >= rows && y.numel() >= rows,
              "d_head: shapes");
  fedtgan::launch_d_head(cfp(d), ld_of(d), cfp(ms), ld_of(ms), cfp(v), cfp(e), cfp(coef), cfp(wloss), fp(y), fp(a),
                         ld_of(a), (int)rows, (int)cols, fp(loss), cur_stream());
}

std::vector<fedtgan::ColsumJob> colsum_jobs(at::TensorList srcs, const c10::List<optional<Tensor>>& outs,
                                            const c10::List<optional<Tensor>>& w,
                                            const c10::List<optional<Tensor>>& dot_v,
                                            const c10::List<optional<Tensor>>& dot_e,
                                            const c10::List<optional<Tensor>>& dot_out,
                                            const c10::List<optional<Tensor>>& dot_w) {
  const size_t n = srcs.size();
  TORCH_CHECK(n <= 8 && outs.size() == n && w.size() == n && dot_v.size() == n && dot_e.size() == n &&
                  dot_out.size() == n && dot_w.size() == n, "colsum_ex: up to 8 jobs, one entry per job in every list");
  std::vector<fedtgan::ColsumJob> jobs;
  for (size_t i = 0; i < n; ++i) {
    check_f32_2d(srcs[i], "colsum src");
    const int64_t rows = srcs[i].size(0), cols = srcs[i].size(1);
    fedtgan::ColsumJob j{cfp(srcs[i]), ld_of(srcs[i]), (int)rows, (int)cols, nullptr, nullptr, nullptr, nullptr, nullptr,
                         nullptr};
    const optional<Tensor> o = outs[i], wi = w[i], dv = dot_v[i], de = dot_e[i], dout = dot_out[i];
    if (o.has_value() && o->defined()) {
      TORCH_CHECK(o->numel() == cols && o->is_contiguous(), "colsum_ex: out");
      j.out = fp(*o);
    }
    if (wi.has_value() && wi->defined()) {
      TORCH_CHECK(wi->numel() == rows && wi->is_contiguous(), "colsum_ex: row weights");
      j.w = cfp(*wi);
    }
    if (dv.has_value() && dv->defined()) {
      TORCH_CHECK(dv->numel() == cols && dv->is_contiguous() && dout.has_value() && dout->defined(), "colsum_ex: dot");
      j.dot_v = cfp(*dv);
      j.dot_out = fp(*dout);
      if (de.has_value() && de->defined()) j.dot_e = cfp(*de);
      const optional<Tensor> dw = dot_w[i];
      if (dw.has_value() && dw->defined()) {
        TORCH_CHECK(dw->numel() == rows && dw->is_contiguous(), "colsum_ex: dot row weights");
        j.dot_w = cfp(*dw);
      }
    }
    jobs.push_back(j);
  }
  return jobs;
}

void colsum_ex(at::TensorList srcs, const c10::List<optional<Tensor>>& outs, const c10::List<optional<Tensor>>& w,
               const c10::List<optional<Tensor>>& dot_v, const c10::List<optional<Tensor>>& dot_e,
               const c10::List<optional<Tensor>>& dot_out, const c10::List<optional<Tensor>>& dot_w) {
  const auto jobs = colsum_jobs(srcs, outs, w, dot_v, dot_e, dot_out, dot_w);
  fedtgan::launch_colsum(jobs.data(), (int)jobs.size(), cur_stream());
}

void colsum(at::TensorList srcs, at::TensorList outs) {
  TORCH_CHECK(srcs.size() == outs.size() && srcs.size() <= 8, "colsum: up to 8 jobs");
  std::vector<fedtgan::ColsumJob> jobs;
  for (size_t i = 0; i < srcs.size(); ++i) {
    check_f32_2d(srcs[i], "colsum src");
    TORCH_CHECK(outs[i].numel() == srcs[i].size(1) && outs[i].is_contiguous(), "colsum: out");
    jobs.push_back({cfp(srcs[i]), ld_of(srcs[i]), (int)srcs[i].size(0), (int)srcs[i].size(1), fp(outs[i]), nullptr,
                    nullptr, nullptr, nullptr});
  }
  fedtgan::launch_colsum(jobs.data(), (int)jobs.size(), cur_stream());
}

void bn_relu_train(const Tensor& a, const Tensor& gamma, const Tensor& beta, const Tensor& out, const Tensor& nhat,
                   const Tensor& mean, const Tensor& invstd, const Tensor& rm, const Tensor& rv, double momentum,
                   double eps, int64_t groups) {
  check_f32_2d(a, "a");
  check_f32_2d(out, "out");
  check_f32_2d(nhat, "nhat");
  TORCH_CHECK(a.size(0) >= 1, "bn_relu_train: empty batch");
  TORCH_CHECK(groups == 1 || groups == 2, "bn_relu_train: 1 or 2 batches");
  TORCH_CHECK(a.size(0) % groups == 0 && a.size(0) / groups >= 1, "bn_relu_train: rows must split evenly");
  TORCH_CHECK(out.sizes() == a.sizes() && nhat.sizes() == a.sizes() && gamma.numel() == a.size(1), "bn: shapes");
  TORCH_CHECK(mean.is_contiguous() && invstd.is_contiguous() && mean.numel() == groups * a.size(1) &&
                  invstd.numel() == groups * a.size(1), "bn_relu_train: mean/invstd must be contiguous [groups, cols]");
  fedtgan::launch_bn_relu_train(cfp(a), ld_of(a), cfp(gamma), cfp(beta), fp(out), ld_of(out), fp(nhat), ld_of(nhat),
                                fp(mean), fp(invstd), fp(rm), fp(rv), (int)a.size(0), (int)a.size(1), (int)groups,
                                (float)momentum, (float)eps, cur_stream());
}

void bn_relu_apply(const Tensor& a, const Tensor& part, int64_t n_tiles, const Tensor& gamma, const Tensor& beta,
                   const Tensor& out, const Tensor& nhat, const Tensor& mean, const Tensor& invstd, const Tensor& rm,
                   const Tensor& rv, double momentum, double eps, int64_t groups) {
  check_f32_2d(a, "a");
  check_f32_2d(out, "out");
  check_f32_2d(nhat, "nhat");
  const int64_t rows = a.size(0), cols = a.size(1);
  TORCH_CHECK(groups == 1 || groups == 2, "bn_relu_apply: 1 or 2 batches");
  TORCH_CHECK(rows >= 1 && rows % groups == 0, "bn_relu_apply: rows must split evenly");
  TORCH_CHECK(out.sizes() == a.sizes() && nhat.sizes() == a.sizes() && gamma.numel() == cols && beta.numel() == cols &&
                  rm.numel() == cols && rv.numel() == cols, "bn_relu_apply: shapes");
  TORCH_CHECK(mean.is_contiguous() && invstd.is_contiguous() && mean.numel() == groups * cols &&
                  invstd.numel() == groups * cols, "bn_relu_apply: mean/invstd must be contiguous [groups, cols]");
  TORCH_CHECK(part.is_cuda() && part.scalar_type() == at::kFloat && part.is_contiguous() &&
                  part.numel() >= n_tiles * 6 * cols && n_tiles >= 1 && n_tiles <= 64,
              "bn_relu_apply: partials [n_tiles <= 64, 2, 3, cols]");
  fedtgan::launch_bn_relu_apply(cfp(a), ld_of(a), cfp(part), (int)n_tiles, cfp(gamma), cfp(beta), fp(out), ld_of(out),
                                fp(nhat), ld_of(nhat), fp(mean), fp(invstd), fp(rm), fp(rv), (int)rows, (int)cols,
                                (int)groups, (float)momentum, (float)eps, cur_stream());
}

// Linear -> BatchNorm(train) -> ReLU, one launch (kernels/bn_fused.hip).  x: the dense input columns
// [groups * rpg, K]; W: [N, K] (any strides); one-hot block as for gemm (oh_w [N, C], or [C, N] with
// oh_trans); stat: >= groups * 2 * N floats; cnt: >= ceil(N / 16) zeroed int32 counters.
void linear_bn_relu_colown(const Tensor& x, const Tensor& w, const optional<Tensor>& bias, const Tensor& gamma,
                           const Tensor& beta, const Tensor& out, const Tensor& nhat, const Tensor& mean,
                           const Tensor& invstd, const Tensor& rm, const Tensor& rv, double momentum, double eps,
                           int64_t groups, const optional<Tensor>& oh_w, const optional<Tensor>& oh_col,
                           const optional<Tensor>& oh_opt, const optional<Tensor>& oh_off, bool oh_trans,
                           const Tensor& stat, const Tensor& cnt) {
  check_f32_2d(x, "x");
  TORCH_CHECK(w.is_cuda() && w.scalar_type() == at::kFloat && w.dim() == 2, "colown: w must be a 2-D fp32 GPU tensor");
  check_f32_2d(out, "out");
  check_f32_2d(nhat, "nhat");
  const int64_t rows = x.size(0), K = x.size(1), N = w.size(0);
  TORCH_CHECK(groups == 1 || groups == 2, "colown: 1 or 2 batches");
  TORCH_CHECK(rows >= 2 && rows % groups == 0, "colown: rows must split evenly");
  TORCH_CHECK(K >= 1 && w.size(1) == K, "colown: w is ", w.sizes(), ", x has K = ", K);
  TORCH_CHECK(out.size(0) == rows && out.size(1) == N && nhat.size(0) == rows && nhat.size(1) == N, "colown: out / nhat");
  TORCH_CHECK(gamma.numel() == N && beta.numel() == N && rm.numel() == N && rv.numel() == N && gamma.is_contiguous() &&
                  beta.is_contiguous() && rm.is_contiguous() && rv.is_contiguous(), "colown: BN vectors");
  TORCH_CHECK(mean.is_contiguous() && invstd.is_contiguous() && mean.numel() == groups * N &&
                  invstd.numel() == groups * N, "colown: mean/invstd must be contiguous [groups, cols]");
  const int64_t rpg = rows / groups;
  TORCH_CHECK(fedtgan::colown_smem_bytes((int)K, (int)rpg) <= 64 * 1024, "colown: batch x K too large for LDS");
  TORCH_CHECK(stat.is_cuda() && stat.scalar_type() == at::kFloat && stat.is_contiguous() && stat.numel() >= groups * 2 * N,
              "colown: stat");
  TORCH_CHECK(cnt.is_cuda() && cnt.scalar_type() == at::kInt && cnt.is_contiguous() && cnt.numel() >= (N + 15) / 16,
              "colown: cnt");
  if (bias.has_value() && bias->defined()) TORCH_CHECK(bias->numel() == N && bias->is_contiguous(), "colown: bias");
  fedtgan::ColOwnArgs g{};
  g.x = cfp(x);
  g.ldx = (int)ld_of(x);
  g.w = w.data_ptr<float>();
  g.w_sn = w.stride(0);
  g.w_sk = w.stride(1);
  g.bias = optp<float>(bias);
  if (oh_w.has_value() && oh_w->defined()) {
    TORCH_CHECK(oh_col.has_value() && oh_opt.has_value() && oh_off.has_value(), "colown: one-hot needs col/opt/off");
    TORCH_CHECK(oh_col->numel() == rows && oh_opt->numel() == rows && oh_col->scalar_type() == at::kInt &&
                    oh_opt->scalar_type() == at::kInt && oh_off->scalar_type() == at::kInt, "colown: one-hot indices");
    TORCH_CHECK(oh_w->scalar_type() == at::kFloat && oh_w->dim() == 2 && oh_w->size(oh_trans ? 1 : 0) == N,
                "colown: one-hot block");
    g.oh_w = oh_w->data_ptr<float>();
    g.oh_sn = oh_trans ? oh_w->stride(1) : oh_w->stride(0);
    g.oh_sc = oh_trans ? oh_w->stride(0) : oh_w->stride(1);
    g.oh_col = oh_col->data_ptr<int>();
    g.oh_opt = oh_opt->data_ptr<int>();
    g.oh_off = oh_off->data_ptr<int>();
  }
  g.gamma = cfp(gamma);
  g.beta = cfp(beta);
  g.out = fp(out);
  g.ldo = (int)ld_of(out);
  g.nhat = fp(nhat);
  g.ldn = (int)ld_of(nhat);
  g.mean = fp(mean);
  g.invstd = fp(invstd);
  g.rm = fp(rm);
  g.rv = fp(rv);
  g.stat = fp(stat);
  g.cnt = reinterpret_cast<unsigned*>(cnt.data_ptr<int>());
  g.rpg = (int)rpg;
  g.groups = (int)groups;
  g.K = (int)K;
  g.N = (int)N;
  g.momentum = (float)momentum;
  g.eps = (float)eps;
  const bool vec = (reinterpret_cast<uintptr_t>(x.data_ptr()) & 15) == 0 && g.ldx % 4 == 0;
  fedtgan::launch_linear_bn_relu_colown(g, vec, cur_stream());
}

void bn_relu_bwd(const Tensor& dr, const Tensor& r, const Tensor& nhat, const Tensor& gamma, const Tensor& invstd,
                 const Tensor& da, const Tensor& dgamma, const Tensor& dbeta, const optional<Tensor>& dbias,
                 bool paired) {
  check_f32_2d(dr, "dr");
  check_f32_2d(r, "r");
  check_f32_2d(nhat, "nhat");
  check_f32_2d(da, "da");
  TORCH_CHECK(dr.size(0) >= 1, "bn_relu_bwd: empty batch");
  TORCH_CHECK(r.sizes() == dr.sizes() && nhat.sizes() == dr.sizes() && da.sizes() == dr.sizes(), "bn bwd: shapes");
  TORCH_CHECK(gamma.numel() >= dr.size(1) && invstd.numel() >= dr.size(1) && dgamma.numel() >= dr.size(1) &&
                  dbeta.numel() >= dr.size(1) && (!(dbias.has_value() && dbias->defined()) || dbias->numel() >= dr.size(1)),
              "bn bwd: per-column vectors");
  if (paired) {
    // the GEMM held with group=1 (an independent weight gradient) runs in the same launch (gemm_bnbwd_kernel)
    const hipStream_t hs = cur_stream();
    TORCH_CHECK(has_held && held_stream == hs, "bn_relu_bwd(paired=True) needs a GEMM held with group=1 on this stream");
    has_held = false;
    const fedtgan::BnBwdArgs b{cfp(dr), ld_of(dr), cfp(r), ld_of(r), cfp(nhat), ld_of(nhat), cfp(gamma), cfp(invstd),
                               fp(da), ld_of(da), fp(dgamma), fp(dbeta), optp<float>(dbias), (int)dr.size(0),
                               (int)dr.size(1)};
    if (fedtgan::launch_gemm_bnbwd(held, b, hs)) return;
    fedtgan::launch_gemm(held, hs);     // (a shape the fused launch does not take: two launches)
  }
  fedtgan::launch_bn_relu_bwd(cfp(dr), ld_of(dr), cfp(r), ld_of(r), cfp(nhat), ld_of(nhat), cfp(gamma), cfp(invstd),
                              fp(da), ld_of(da), fp(dgamma), fp(dbeta), optp<float>(dbias), (int)dr.size(0),
                              (int)dr.size(1), cur_stream());
}

void adam(const Tensor& p, const Tensor& g, const Tensor& m, const Tensor& v, const Tensor& step, double lr, double b1,
          double b2, double eps, double wd, const optional<Tensor>& rng_bump) {
  TORCH_CHECK(!g_adam_held.active && !g_adam_pre.active,
              "adam: a GEMM held for the Adam launch needs adam_cs (the column-sum form)");
  TORCH_CHECK(p.is_contiguous() && g.is_contiguous() && m.is_contiguous() && v.is_contiguous(), "adam: contiguous");
  TORCH_CHECK(p.numel() == g.numel() && p.numel() == m.numel() && p.numel() == v.numel(), "adam: sizes");
  TORCH_CHECK((reinterpret_cast<uintptr_t>(p.data_ptr()) & 15) == 0 && (reinterpret_cast<uintptr_t>(g.data_ptr()) & 15) == 0,
              "adam: buffers must be 16-byte aligned");
  uint64_t* bump = nullptr;
  if (rng_bump.has_value() && rng_bump->defined()) bump = reinterpret_cast<uint64_t*>(rng_bump->data_ptr<int64_t>());
  fedtgan::launch_adam(fp(p), cfp(g), fp(m), fp(v), cfp(step), p.numel(), (float)lr, (float)b1, (float)b2, (float)eps,
                       (float)wd, bump, cur_stream());
}

// adam + colsum_ex jobs in one launch.  A job whose output lies in g owns ceil4(cols) elements
// there (16-B aligned start; the flat layout pads every tensor to 4 floats) and gets its Adam
// update from the reduced sums; outputs elsewhere (metrics) are just written.
void adam_cs(const Tensor& p, const Tensor& g, const Tensor& m, const Tensor& v, const Tensor& step, double lr,
             double b1, double b2, double eps, double wd, const optional<Tensor>& rng_bump, at::TensorList srcs,
             const c10::List<optional<Tensor>>& outs, const c10::List<optional<Tensor>>& w,
             const c10::List<optional<Tensor>>& dot_v, const c10::List<optional<Tensor>>& dot_e,
             const c10::List<optional<Tensor>>& dot_out, const c10::List<optional<Tensor>>& dot_w) {
  TORCH_CHECK(p.is_contiguous() && g.is_contiguous() && m.is_contiguous() && v.is_contiguous(), "adam_cs: contiguous");
  TORCH_CHECK(p.numel() == g.numel() && p.numel() == m.numel() && p.numel() == v.numel(), "adam_cs: sizes");
  TORCH_CHECK(p.numel() % 4 == 0, "adam_cs: buffer length must be a multiple of 4");
  for (const Tensor* t : {&p, &g, &m, &v})
    TORCH_CHECK((reinterpret_cast<uintptr_t>(t->data_ptr()) & 15) == 0, "adam_cs: buffers must be 16-byte aligned");
  const auto jobs = colsum_jobs(srcs, outs, w, dot_v, dot_e, dot_out, dot_w);
  fedtgan::AdamColsum cs{};
  cs.n_jobs = (int)jobs.size();
  const float* g0 = cfp(g);
  const int64_t n = g.numel();
  for (int k = 0; k < cs.n_jobs; ++k) {
    cs.jobs[k] = jobs[k];
    cs.own_lo[k] = cs.own_hi[k] = 0;
    const int c4 = (jobs[k].cols + 3) / 4 * 4;
    cs.vec[k] = (reinterpret_cast<uintptr_t>(jobs[k].a) & 15) == 0 && jobs[k].lda % 4 == 0 &&
                (jobs[k].rows <= 1 || jobs[k].lda >= c4) &&
                srcs[k].storage().nbytes() >= (size_t)((char*)jobs[k].a - (char*)srcs[k].storage().data()) +
                    ((size_t)(jobs[k].rows - 1) * jobs[k].lda + c4) * sizeof(float);
    const float* o = jobs[k].out;
    if (o && o >= g0 && o < g0 + n) {
      const int64_t off = o - g0, len = ((int64_t)jobs[k].cols + 3) / 4 * 4;
      TORCH_CHECK(off % 4 == 0 && off + len <= n, "adam_cs: a job output inside the gradient buffer must start "
                  "4-aligned and own ceil4(cols) elements");
      for (int q = 0; q < k; ++q)
        TORCH_CHECK(off >= cs.own_hi[q] || off + len <= cs.own_lo[q], "adam_cs: overlapping job outputs");
      cs.own_lo[k] = off;
      cs.own_hi[k] = off + len;
    }
    // a dot over parameters this launch updates must be this job's own (read pre-update by
    // the updating lane); any other overlap with p would race with the update
    const float* p0 = cfp(p);
    const float* dv = jobs[k].dot_v;
    cs.dot_self[k] = dv && cs.own_hi[k] > cs.own_lo[k] && dv == p0 + cs.own_lo[k];
    TORCH_CHECK(!dv || cs.dot_self[k] || dv + jobs[k].cols <= p0 || dv >= p0 + n,
                "adam_cs: a dot over parameters updated by this launch must belong to the same job");
  }
  uint64_t* bump = nullptr;
  if (rng_bump.has_value() && rng_bump->defined()) bump = reinterpret_cast<uint64_t*>(rng_bump->data_ptr<int64_t>());
  const hipStream_t hs = cur_stream();
  if (g_adam_pre.active) {
    // the held short-K weight gradient applies Adam to its own block now (it reads only A, B and the step
    // counter, and writes only its block of p / m / v: independent of this launch's other elements)
    AdamHeld h = g_adam_pre;
    g_adam_pre.active = false;
    TORCH_CHECK(h.stream == hs, "adam_cs: the short-K GEMM held for it was issued on another stream");
    const int64_t off = h.c - g0;
    TORCH_CHECK(h.c >= g0 && off % 4 == 0 && h.ldc % 4 == 0 && off + h.M * h.ldc <= n,
                "adam_cs: the held short-K GEMM's output must be a 4-aligned block inside the gradient buffer");
    for (int k = 0; k < cs.n_jobs; ++k)
      TORCH_CHECK(off >= cs.own_hi[k] || off + h.M * h.ldc <= cs.own_lo[k], "adam_cs: the short-K GEMM overlaps a job");
    fedtgan::GemmArgs q = h.g;
    q.adam_p = fp(p) + off;
    q.adam_m = fp(m) + off;
    q.adam_v = fp(v) + off;
    q.adam_step = cfp(step);
    q.adam_lr = (float)lr;
    q.adam_b1 = (float)b1;
    q.adam_b2 = (float)b2;
    q.adam_eps = (float)eps;
    q.adam_wd = (float)wd;
    if (fedtgan::launch_gemm_shortk_adam(q, hs)) {
      cs.skip2_lo = off;
      cs.skip2_hi = off + h.M * h.ldc;
    } else {
      fedtgan::launch_gemm(h.g, hs);     // (a shape the short-K kernel does not take: the plain GEMM, Adam below)
    }
  }
  if (g_adam_held.active) {
    // the held weight-gradient GEMM (gemm(..., group=3)) writes rows [0, M) x [0, N) at stride ldc of a
    // block inside g: Adam over that whole block is left to the GEMM's tiles (elements of the block
    // outside M x N -- padding -- keep their values, as their gradient is zero)
    AdamHeld h = g_adam_held;
    g_adam_held.active = false;
    TORCH_CHECK(h.stream == hs, "adam_cs: the GEMM held for it was issued on another stream");
    const int64_t off = h.c - g0, len = (h.M - 1) * h.ldc + h.N;
    TORCH_CHECK(h.c >= g0 && off % 4 == 0 && h.ldc % 4 == 0 && off + (h.M * h.ldc) <= n && len > 0,
                "adam_cs: the held GEMM's output must be a 4-aligned block inside the gradient buffer");
    for (int k = 0; k < cs.n_jobs; ++k)
      TORCH_CHECK(off >= cs.own_hi[k] || off + h.M * h.ldc <= cs.own_lo[k], "adam_cs: the held GEMM overlaps a job output");
    TORCH_CHECK(cs.skip2_hi <= off || off + h.M * h.ldc <= cs.skip2_lo, "adam_cs: the two held GEMMs overlap");
    cs.skip_lo = off;
    cs.skip_hi = off + h.M * h.ldc;
    if (cs.skip2_hi > cs.skip2_lo && cs.skip2_lo < cs.skip_lo) {   // (adam_cs_body: the lower range first)
      std::swap(cs.skip_lo, cs.skip2_lo);
      std::swap(cs.skip_hi, cs.skip2_hi);
    }
    if (fedtgan::launch_gemm_adam(h.g, fp(p), cfp(g), fp(m), fp(v), cfp(step), n, (float)lr, (float)b1, (float)b2,
                                  (float)eps, (float)wd, bump, cs, hs))
      return;
    // shape not instantiated: the GEMM, then the plain launch (keeping the short-K range cut out, if any)
    if (cs.skip_lo == off) cs.skip_lo = cs.skip_hi = 0;
    else cs.skip2_lo = cs.skip2_hi = 0;
    if (cs.skip_hi <= cs.skip_lo && cs.skip2_hi > cs.skip2_lo) {
      std::swap(cs.skip_lo, cs.skip2_lo);
      std::swap(cs.skip_hi, cs.skip2_hi);
    }
    fedtgan::launch_gemm(h.g, hs);
  }
  fedtgan::launch_adam_colsum(fp(p), cfp(g), fp(m), fp(v), cfp(step), p.numel(), (float)lr, (float)b1, (float)b2,
                              (float)eps, (float)wd, bump, cs, hs);
}

void sample_decode(const Tensor& logits, const Tensor& out, const Tensor& kind, const Tensor& start,
                   const Tensor& width, const Tensor& cont, const Tensor& code_off, const Tensor& codes,
                   const Tensor& mu, const Tensor& sd, int64_t seed, const Tensor& rng_ctr, int64_t stream,
                   const optional<Tensor>& ecol, const optional<Tensor>& quads) {
  check_f32_2d(logits, "logits");
  TORCH_CHECK(out.scalar_type() == at::kDouble && out.is_contiguous() && out.dim() == 2, "decode: out f64");
  TORCH_CHECK(out.size(0) == logits.size(0) && out.size(1) == kind.numel(), "decode: shapes");
  TORCH_CHECK(mu.scalar_type() == at::kDouble && sd.scalar_type() == at::kDouble && codes.scalar_type() == at::kDouble,
              "decode: f64 tables");
  fedtgan::DecodeArgs a{};
  a.logits = cfp(logits);
  a.ldl = ld_of(logits);
  a.rows = (int)logits.size(0);
  a.n_cols = (int)kind.numel();
  a.kind = kind.data_ptr<int>();
  a.start = start.data_ptr<int>();
  a.width = width.data_ptr<int>();
  a.cont = cont.data_ptr<int>();
  a.code_off = code_off.data_ptr<int>();
  a.codes = codes.data_ptr<double>();
  a.n_codes = (int)codes.numel();
  a.mu = mu.data_ptr<double>();
  a.sd = sd.data_ptr<double>();
  a.K = mu.dim() == 2 ? (int)mu.size(1) : 1;
  a.out = out.data_ptr<double>();
  a.seed = (uint64_t)seed;
  a.rng_ctr = ctr_ptr(rng_ctr);
  a.rng_stream = (uint32_t)stream;
  a.dim = (int)logits.size(1);
  if (ecol.has_value() && ecol->defined()) {
    TORCH_CHECK(ecol->scalar_type() == at::kInt && ecol->is_contiguous() && ecol->numel() == logits.size(1),
                "decode: ecol must be int32 [data_dim]");
    // the row kernel keeps one 8-byte maximum per output column and wave in LDS
    if (a.n_cols * 4 * 8 <= 64 * 1024) a.ecol = ecol->data_ptr<int>();
  }
  if (quads.has_value() && quads->defined()) {
    TORCH_CHECK(quads->scalar_type() == at::kInt && quads->is_contiguous() && quads->dim() == 2 && quads->size(1) == 2,
                "decode: quads must be int32 [n, 2]");
    TORCH_CHECK(logits.size(1) < 65536, "decode: quads address positions below 65536");
    // every entry: a column, 1-4 logits inside the row and inside that column's span (host-built)
    a.quads = quads->data_ptr<int>();
    a.n_quads = (int)quads->size(0);
  }
  fedtgan::launch_sample_decode(a, cur_stream());
}

void gen_weight_prep(const std::vector<Tensor>& w, std::vector<int64_t> kd, const std::vector<Tensor>& w16,
                     const std::vector<Tensor>& wt) {
  const size_t n = w.size();
  TORCH_CHECK(n >= 1 && n <= 4 && kd.size() == n && w16.size() == n && wt.size() == n, "gen_weight_prep: 1-4 jobs");
  fedtgan::GenWeightPrep a{};
  a.n_jobs = (int)n;
  for (size_t j = 0; j < n; ++j) {
    // the weight as stored: [N, K] rows (unit k stride) or input-major (EngineConfig.g_wt: unit n stride)
    TORCH_CHECK(w[j].is_cuda() && w[j].scalar_type() == at::kFloat && w[j].dim() == 2 &&
                    (w[j].stride(1) == 1 || w[j].stride(0) == 1), "gen_weight_prep w: 2-D fp32, one unit stride");
    const int64_t N = w[j].size(0), K = w[j].size(1);
    TORCH_CHECK(kd[j] >= 0 && kd[j] <= K, "gen_weight_prep: kd");
    TORCH_CHECK(w16[j].is_cuda() && w16[j].scalar_type() == at::kBFloat16 && w16[j].dim() == 2 && w16[j].size(0) == N &&
                    w16[j].size(1) >= kd[j] && w16[j].stride(1) == 1, "gen_weight_prep: w16 [N, >= kd] bf16");
    check_f32_2d(wt[j], "gen_weight_prep wt");
    TORCH_CHECK(wt[j].is_contiguous() && wt[j].size(0) == K - kd[j] && wt[j].size(1) == N, "gen_weight_prep: wt [C, N]");
    const bool kmaj = w[j].stride(1) == 1;
    a.jobs[j] = fedtgan::GenWeightJob{cfp(w[j]), (int)N, kmaj ? ld_of(w[j]) : 1, kmaj ? 1 : (int)w[j].stride(1),
                                      (int)kd[j], (int)(K - kd[j]), hp(w16[j]),
                                      (int)w16[j].stride(0), fp(wt[j])};
  }
  fedtgan::launch_gen_weight_prep(a, cur_stream());
}

void rng_bump(const Tensor& ctr) {
  TORCH_CHECK(ctr.scalar_type() == at::kLong && ctr.is_cuda(), "rng_bump: cuda int64");
  fedtgan::launch_rng_bump(reinterpret_cast<uint64_t*>(ctr.data_ptr<int64_t>()), cur_stream());
}

// ----------------------------------------------------------------------------- conditional generation
// the request buffers of kernels/cond_gen.hip (CondReq), validated: every table on the device, one entry per bin
fedtgan::CondReq cond_req(const Tensor& drive, const Tensor& bin_opt, const Tensor& bin_code, const Tensor& quota,
                          const Tensor& filled, const Tensor& seg_off, const Tensor& fixed_j, const Tensor& fixed_code,
                          const Tensor& stats) {
  const int64_t nb = bin_opt.numel(), nf = fixed_j.numel();
  TORCH_CHECK(nb >= 1 && nb <= fedtgan::COND_MAX_BINS, "conditional request: 1..", fedtgan::COND_MAX_BINS, " bins, got ", nb);
  auto i32 = [](const Tensor& t) { return t.is_cuda() && t.scalar_type() == at::kInt && t.is_contiguous(); };
  auto i64 = [](const Tensor& t) { return t.is_cuda() && t.scalar_type() == at::kLong && t.is_contiguous(); };
  auto f64 = [](const Tensor& t) { return t.is_cuda() && t.scalar_type() == at::kDouble && t.is_contiguous(); };
  TORCH_CHECK(i32(drive) && drive.numel() == 2 && i32(bin_opt) && i32(fixed_j), "conditional request: int32 tables");
  TORCH_CHECK(f64(bin_code) && bin_code.numel() == nb && f64(fixed_code) && fixed_code.numel() == nf,
              "conditional request: float64 codes, one per bin / fixed column");
  TORCH_CHECK(i64(quota) && quota.numel() == nb && i64(filled) && filled.numel() == nb && i64(seg_off) &&
                  seg_off.numel() == nb && i64(stats) && stats.numel() == 2,
              "conditional request: int64 quota / filled / seg_off per bin and two statistics");
  fedtgan::CondReq r{};
  r.drive = drive.data_ptr<int>();
  r.n_bins = (int)nb;
  r.bin_opt = bin_opt.data_ptr<int>();
  r.bin_code = bin_code.data_ptr<double>();
  r.quota = quota.data_ptr<int64_t>();
  r.filled = filled.data_ptr<int64_t>();
  r.seg_off = seg_off.data_ptr<int64_t>();
  r.n_fixed = (int)nf;
  r.fixed_j = nf ? fixed_j.data_ptr<int>() : nullptr;
  r.fixed_code = nf ? fixed_code.data_ptr<double>() : nullptr;
  r.stats = stats.data_ptr<int64_t>();
  return r;
}

void cond_request(const Tensor& drive, const Tensor& bin_opt, const Tensor& bin_code, const Tensor& quota,
                  const Tensor& filled, const Tensor& seg_off, const Tensor& fixed_j, const Tensor& fixed_code,
                  const Tensor& stats, const Tensor& col, const Tensor& opt, const Tensor& tgt,
                  const optional<Tensor>& h, int64_t cc, const Tensor& cond_off, const Tensor& cond_w, int64_t seed,
                  const Tensor& rng_ctr, int64_t stream) {
  fedtgan::CondRequestArgs a{};
  a.req = cond_req(drive, bin_opt, bin_code, quota, filled, seg_off, fixed_j, fixed_code, stats);
  a.rows = (int)tgt.numel();
  for (const Tensor* t : {&col, &opt, &tgt})
    TORCH_CHECK(t->is_cuda() && t->scalar_type() == at::kInt && t->is_contiguous() && t->numel() >= a.rows,
                "cond_request: col / opt / tgt must be int32 with one entry per row");
  TORCH_CHECK(cond_off.is_cuda() && cond_off.scalar_type() == at::kInt && cond_off.is_contiguous() &&
                  cond_w.is_cuda() && cond_w.scalar_type() == at::kInt && cond_w.is_contiguous() &&
                  cond_w.numel() == cond_off.numel() && cond_off.numel() >= 1, "cond_request: int32 span tables");
  a.col = col.data_ptr<int>();
  a.opt = opt.data_ptr<int>();
  a.tgt = tgt.data_ptr<int>();
  a.cond_off = cond_off.data_ptr<int>();
  a.cond_w = cond_w.data_ptr<int>();
  a.n_span = (int)cond_off.numel();
  if (h.has_value() && h->defined()) {
    check_f32_2d(*h, "cond_request h");
    TORCH_CHECK(h->size(0) >= a.rows && cc >= 0 && cc < h->size(1), "cond_request: h rows / conditional block");
    a.h = fp(*h);
    a.ldh = ld_of(*h);
    a.cc = (int)cc;
    a.C = (int)(h->size(1) - cc);
  }
  a.seed = (uint64_t)seed;
  a.rng_ctr = ctr_ptr(rng_ctr);
  a.rng_stream = (uint32_t)stream;
  fedtgan::launch_cond_request(a, cur_stream());
}

void cond_partition(const Tensor& drive, const Tensor& bin_opt, const Tensor& bin_code, const Tensor& quota,
                    const Tensor& filled, const Tensor& seg_off, const Tensor& fixed_j, const Tensor& fixed_code,
                    const Tensor& stats, const Tensor& out, const Tensor& tgt, const Tensor& dst, const Tensor& keep,
                    const Tensor& counts, bool any_value) {
  fedtgan::CondPartitionArgs a{};
  a.any_value = any_value ? 1 : 0;
  a.req = cond_req(drive, bin_opt, bin_code, quota, filled, seg_off, fixed_j, fixed_code, stats);
  TORCH_CHECK(out.is_cuda() && out.scalar_type() == at::kDouble && out.is_contiguous() && out.dim() == 2,
              "cond_partition: out must be contiguous float64 [rows, n_cols]");
  TORCH_CHECK(dst.is_cuda() && dst.scalar_type() == at::kDouble && dst.is_contiguous() && dst.dim() == 2 &&
                  dst.size(1) == out.size(1), "cond_partition: dst must be contiguous float64 [n, n_cols]");
  TORCH_CHECK(out.numel() < (int64_t)INT32_MAX, "cond_partition: a pass holds fewer than 2^31 values");
  a.out = out.data_ptr<double>();
  a.rows = (int)out.size(0);
  a.n_cols = (int)out.size(1);
  a.dst = dst.data_ptr<double>();
  a.n_dst = dst.size(0);
  const int64_t n_wg = fedtgan::cond_partition_workgroups(a.rows);
  for (const Tensor* t : {&tgt, &keep, &counts})
    TORCH_CHECK(t->is_cuda() && t->scalar_type() == at::kInt && t->is_contiguous(), "cond_partition: int32 buffers");
  TORCH_CHECK(tgt.numel() >= a.rows && keep.numel() >= a.rows && counts.numel() >= n_wg * a.req.n_bins,
              "cond_partition: tgt / keep need one entry per row, counts one per workgroup and bin");
  a.tgt = tgt.data_ptr<int>();
  a.keep = keep.data_ptr<int>();
  a.counts = counts.data_ptr<int>();
  fedtgan::launch_cond_partition(a, cur_stream());
}

int64_t cond_partition_workgroups(int64_t rows) { return fedtgan::cond_partition_workgroups((int)rows); }

// range / set predicates of a conditional request (kernels/cond_pred.hip)
void pred_request(const Tensor& drv, const Tensor& drv_opt, const Tensor& drv_cum, const Tensor& quota,
                  const Tensor& filled, const Tensor& col, const Tensor& opt, const Tensor& tgt,
                  const optional<Tensor>& h, int64_t cc, const Tensor& cond_off, const Tensor& cond_w, int64_t seed,
                  const Tensor& rng_ctr, int64_t stream) {
  auto i32 = [](const Tensor& t) { return t.is_cuda() && t.scalar_type() == at::kInt && t.is_contiguous(); };
  auto i64 = [](const Tensor& t) { return t.is_cuda() && t.scalar_type() == at::kLong && t.is_contiguous(); };
  fedtgan::PredRequestArgs a{};
  a.M = (int)drv_opt.numel();
  TORCH_CHECK(i32(drv) && drv.numel() == 2 && i32(drv_opt) && a.M >= 1 && drv_cum.is_cuda() &&
                  drv_cum.scalar_type() == at::kDouble && drv_cum.is_contiguous() && drv_cum.numel() == a.M,
              "pred_request: drv int32 [2], drv_opt int32 [M], drv_cum float64 [M], M >= 1");
  TORCH_CHECK(i64(quota) && quota.numel() == 1 && i64(filled) && filled.numel() == 1,
              "pred_request: a predicate-driven request has one bin (int64 quota / filled)");
  a.rows = (int)tgt.numel();
  for (const Tensor* t : {&col, &opt, &tgt})
    TORCH_CHECK(i32(*t) && t->numel() >= a.rows, "pred_request: col / opt / tgt must be int32 with one entry per row");
  TORCH_CHECK(i32(cond_off) && i32(cond_w) && cond_w.numel() == cond_off.numel() && cond_off.numel() >= 1,
              "pred_request: int32 span tables");
  a.drv = drv.data_ptr<int>();
  a.drv_opt = drv_opt.data_ptr<int>();
  a.drv_cum = drv_cum.data_ptr<double>();
  a.quota = quota.data_ptr<int64_t>();
  a.filled = filled.data_ptr<int64_t>();
  a.col = col.data_ptr<int>();
  a.opt = opt.data_ptr<int>();
  a.tgt = tgt.data_ptr<int>();
  a.cond_off = cond_off.data_ptr<int>();
  a.cond_w = cond_w.data_ptr<int>();
  a.n_span = (int)cond_off.numel();
  if (h.has_value() && h->defined()) {
    check_f32_2d(*h, "pred_request h");
    TORCH_CHECK(h->size(0) >= a.rows && cc >= 0 && cc < h->size(1), "pred_request: h rows / conditional block");
    a.h = fp(*h);
    a.ldh = ld_of(*h);
    a.cc = (int)cc;
    a.C = (int)(h->size(1) - cc);
  }
  a.seed = (uint64_t)seed;
  a.rng_ctr = ctr_ptr(rng_ctr);
  a.rng_stream = (uint32_t)stream;
  fedtgan::launch_pred_request(a, cur_stream());
}

void pred_mark(const Tensor& pred_j, const Tensor& pred_kind, const Tensor& pred_lo, const Tensor& pred_hi,
               const Tensor& pred_lut_off, const Tensor& pred_lut_len, const Tensor& pred_lut,
               const Tensor& pred_stats, const Tensor& out, const Tensor& tgt) {
  auto i32 = [](const Tensor& t) { return t.is_cuda() && t.scalar_type() == at::kInt && t.is_contiguous(); };
  auto f64 = [](const Tensor& t) { return t.is_cuda() && t.scalar_type() == at::kDouble && t.is_contiguous(); };
  const int64_t np = pred_j.numel();
  TORCH_CHECK(np >= 0 && np <= fedtgan::PRED_MAX, "pred_mark: at most ", fedtgan::PRED_MAX, " predicates");
  TORCH_CHECK(i32(pred_j) && i32(pred_kind) && pred_kind.numel() == np && i32(pred_lut_off) &&
                  pred_lut_off.numel() == np && i32(pred_lut_len) && pred_lut_len.numel() == np,
              "pred_mark: int32 column / kind / table slice per predicate");
  TORCH_CHECK(f64(pred_lo) && pred_lo.numel() == np && f64(pred_hi) && pred_hi.numel() == np,
              "pred_mark: float64 bounds per predicate");
  TORCH_CHECK(pred_lut.is_cuda() && pred_lut.scalar_type() == at::kByte && pred_lut.is_contiguous() &&
                  pred_lut.numel() < (int64_t)INT32_MAX, "pred_mark: pred_lut uint8");
  TORCH_CHECK(pred_stats.is_cuda() && pred_stats.scalar_type() == at::kLong && pred_stats.is_contiguous() &&
                  pred_stats.numel() == 2 + fedtgan::PRED_MAX, "pred_mark: pred_stats int64 [2 + PRED_MAX]");
  TORCH_CHECK(out.is_cuda() && out.scalar_type() == at::kDouble && out.is_contiguous() && out.dim() == 2,
              "pred_mark: out must be contiguous float64 [rows, n_cols]");
  TORCH_CHECK(i32(tgt) && tgt.numel() >= out.size(0) && out.size(0) < (int64_t)INT32_MAX,
              "pred_mark: tgt int32, one entry per row");
  fedtgan::PredMarkArgs a{};
  a.p.n_pred = (int)np;
  a.p.j = pred_j.data_ptr<int>();
  a.p.kind = pred_kind.data_ptr<int>();
  a.p.lo = pred_lo.data_ptr<double>();
  a.p.hi = pred_hi.data_ptr<double>();
  a.p.lut_off = pred_lut_off.data_ptr<int>();
  a.p.lut_len = pred_lut_len.data_ptr<int>();
  a.p.lut = pred_lut.data_ptr<uint8_t>();
  a.p.lut_total = (int)pred_lut.numel();
  a.p.stats = pred_stats.data_ptr<int64_t>();
  a.out = out.data_ptr<double>();
  a.rows = (int)out.size(0);
  a.n_cols = (int)out.size(1);
  a.tgt = tgt.data_ptr<int>();
  fedtgan::launch_pred_mark(a, cur_stream());
}

// completion of partial rows (kernels/known_gen.hip)
void known_request(const Tensor& qidx, const Tensor& drv_span, const Tensor& drv_opt, int64_t tries, const Tensor& col,
                   const Tensor& opt, const optional<Tensor>& h, int64_t cc, const Tensor& cond_off,
                   const Tensor& cond_w) {
  auto i32 = [](const Tensor& t) { return t.is_cuda() && t.scalar_type() == at::kInt && t.is_contiguous(); };
  TORCH_CHECK(tries >= 1 && tries <= fedtgan::KNOWN_MAX_TRIES, "known_request: 1..", fedtgan::KNOWN_MAX_TRIES,
              " tries, got ", tries);
  TORCH_CHECK(i32(qidx) && i32(drv_span) && i32(drv_opt) && drv_opt.numel() == drv_span.numel(),
              "known_request: int32 qidx [slots] and drv_span / drv_opt [queries]");
  const int64_t rows = qidx.numel() * tries;
  TORCH_CHECK(rows < (int64_t)INT32_MAX, "known_request: a pass holds fewer than 2^31 rows");
  TORCH_CHECK(i32(col) && i32(opt) && col.numel() >= rows && opt.numel() >= rows,
              "known_request: col / opt must be int32 with one entry per row");
  TORCH_CHECK(i32(cond_off) && i32(cond_w) && cond_w.numel() == cond_off.numel() && cond_off.numel() >= 1,
              "known_request: int32 span tables");
  fedtgan::KnownRequestArgs a{};
  a.qidx = qidx.data_ptr<int>();
  a.n_slots = (int)qidx.numel();
  a.tries = (int)tries;
  a.n_query = drv_span.numel();
  a.drv_span = drv_span.data_ptr<int>();
  a.drv_opt = drv_opt.data_ptr<int>();
  a.col = col.data_ptr<int>();
  a.opt = opt.data_ptr<int>();
  a.cond_off = cond_off.data_ptr<int>();
  a.cond_w = cond_w.data_ptr<int>();
  a.n_span = (int)cond_off.numel();
  if (h.has_value() && h->defined()) {
    check_f32_2d(*h, "known_request h");
    TORCH_CHECK(h->size(0) >= rows && cc >= 0 && cc < h->size(1), "known_request: h rows / conditional block");
    a.h = fp(*h);
    a.ldh = ld_of(*h);
    a.cc = (int)cc;
    a.C = (int)(h->size(1) - cc);
  }
  fedtgan::launch_known_request(a, cur_stream());
}

void known_match(const Tensor& known, const Tensor& mask, const Tensor& qidx, int64_t tries, const Tensor& cand,
                 const Tensor& kind, const Tensor& scale, const Tensor& best, const Tensor& dc, const Tensor& miss,
                 const Tensor& seen, const Tensor& pick, const Tensor& dst) {
  auto dev = [](const Tensor& t, at::ScalarType ty) { return t.is_cuda() && t.scalar_type() == ty && t.is_contiguous(); };
  TORCH_CHECK(tries >= 1 && tries <= fedtgan::KNOWN_MAX_TRIES, "known_match: 1..", fedtgan::KNOWN_MAX_TRIES,
              " tries, got ", tries);
  TORCH_CHECK(dev(known, at::kDouble) && known.dim() == 2 && dev(mask, at::kByte) && mask.dim() == 2 &&
                  mask.size(0) == known.size(0) && mask.size(1) == known.size(1),
              "known_match: known float64 [queries, n_cols] and mask uint8 of the same shape");
  const int64_t nq = known.size(0), n_cols = known.size(1);
  TORCH_CHECK(n_cols >= 1 && n_cols <= 1024, "known_match: 1..1024 columns, got ", n_cols);
  TORCH_CHECK(nq < (int64_t)INT32_MAX, "known_match: fewer than 2^31 queries");
  TORCH_CHECK(dev(qidx, at::kInt), "known_match: qidx int32 [slots]");
  TORCH_CHECK(dev(cand, at::kDouble) && cand.dim() == 2 && cand.size(1) == n_cols &&
                  cand.size(0) >= qidx.numel() * tries && cand.numel() < (int64_t)INT32_MAX,
              "known_match: cand float64 [>= slots * tries, n_cols], fewer than 2^31 values");
  TORCH_CHECK(dev(kind, at::kInt) && kind.numel() == n_cols && dev(scale, at::kDouble) && scale.numel() == n_cols,
              "known_match: int32 kind and float64 scale, one entry per column");
  TORCH_CHECK(dev(best, at::kDouble) && dev(dc, at::kDouble) && dev(miss, at::kInt) && dev(seen, at::kLong) &&
                  dev(pick, at::kLong) && best.numel() >= nq && dc.numel() >= nq && miss.numel() >= nq &&
                  seen.numel() >= nq && pick.numel() >= nq,
              "known_match: best / dc float64, miss int32, seen / pick int64, one entry per query");
  TORCH_CHECK(dev(dst, at::kDouble) && dst.dim() == 2 && dst.size(0) >= nq && dst.size(1) == n_cols,
              "known_match: dst float64 [queries, n_cols]");
  fedtgan::KnownMatchArgs a{};
  a.known = known.data_ptr<double>();
  a.mask = mask.data_ptr<uint8_t>();
  a.n_query = nq;
  a.n_cols = (int)n_cols;
  a.qidx = qidx.data_ptr<int>();
  a.n_slots = (int)qidx.numel();
  a.tries = (int)tries;
  a.cand = cand.data_ptr<double>();
  a.kind = kind.data_ptr<int>();
  a.scale = scale.data_ptr<double>();
  a.best = best.data_ptr<double>();
  a.dc = dc.data_ptr<double>();
  a.miss = miss.data_ptr<int>();
  a.seen = seen.data_ptr<int64_t>();
  a.pick = pick.data_ptr<int64_t>();
  a.dst = dst.data_ptr<double>();
  fedtgan::launch_known_match(a, cur_stream());
}

// ----------------------------------------------------------------------------- similarity evaluator
namespace {
bool sim_i32(const Tensor& t) { return t.is_cuda() && t.scalar_type() == at::kInt && t.is_contiguous(); }
bool sim_f64(const Tensor& t) { return t.is_cuda() && t.scalar_type() == at::kDouble && t.is_contiguous(); }
}  // namespace

void sim_prepare(const Tensor& values, const Tensor& kind, const Tensor& slot, const Tensor& vocab, const Tensor& keys,
                 const Tensor& valid, const Tensor& counts) {
  TORCH_CHECK(sim_f64(values) && values.dim() == 2 && values.size(1) >= 1,
              "sim_prepare: values must be contiguous float64 [rows, n_cols]");
  TORCH_CHECK(values.numel() < (int64_t)INT32_MAX, "sim_prepare: a table holds fewer than 2^31 values");
  TORCH_CHECK(sim_i32(kind) && sim_i32(slot) && kind.numel() == values.size(1) && slot.numel() == values.size(1),
              "sim_prepare: int32 kind / slot, one entry per column");
  TORCH_CHECK(sim_f64(keys) && keys.dim() == 2 && keys.size(1) >= values.size(0) && sim_i32(valid) &&
                  valid.numel() == keys.size(0), "sim_prepare: keys float64 [n_cont, >= rows], valid int32 [n_cont]");
  TORCH_CHECK(sim_i32(counts) && counts.dim() == 2 && sim_i32(vocab) && vocab.numel() == counts.size(0),
              "sim_prepare: counts int32 [n_cat, width], vocab int32 [n_cat]");
  fedtgan::SimPrepareArgs a{};
  a.values = values.data_ptr<double>();
  a.rows = (int)values.size(0);
  a.n_cols = (int)values.size(1);
  a.kind = kind.data_ptr<int>();
  a.slot = slot.data_ptr<int>();
  a.n_cont = (int)keys.size(0);
  a.n_cat = (int)counts.size(0);
  a.vocab = a.n_cat ? vocab.data_ptr<int>() : nullptr;
  a.keys = a.n_cont ? keys.data_ptr<double>() : nullptr;
  a.ldk = keys.size(1);
  a.valid = a.n_cont ? valid.data_ptr<int>() : nullptr;
  a.counts = a.n_cat ? counts.data_ptr<int>() : nullptr;
  a.ldc = (int)counts.size(1);
  fedtgan::launch_sim_prepare(a, cur_stream());
}

void sim_sort(const Tensor& keys, const Tensor& tmp, int64_t n) {
  TORCH_CHECK(sim_f64(keys) && keys.dim() == 2 && sim_f64(tmp) && tmp.dim() == 2 && tmp.size(0) == keys.size(0) &&
                  tmp.size(1) == keys.size(1), "sim_sort: keys / tmp must be contiguous float64 of one shape");
  TORCH_CHECK(n >= 0 && n <= keys.size(1) && n < (int64_t)INT32_MAX, "sim_sort: n outside the key rows");
  if (keys.size(0) == 0 || n == 0) return;
  fedtgan::launch_sim_sort(keys.data_ptr<double>(), tmp.data_ptr<double>(), (int)keys.size(0), keys.size(1), (int)n,
                           cur_stream());
}

void sim_w1(const Tensor& real, const Tensor& n_real, const Tensor& fake, const Tensor& n_fake, int64_t max_fake,
            const Tensor& part, const Tensor& out) {
  TORCH_CHECK(sim_f64(real) && real.dim() == 2 && sim_f64(fake) && fake.dim() == 2 && fake.size(0) == real.size(0),
              "sim_w1: real / fake must be contiguous float64 [n_cont, rows]");
  const int64_t nc = real.size(0);
  TORCH_CHECK(sim_i32(n_real) && n_real.numel() == nc && sim_i32(n_fake) && n_fake.numel() == nc,
              "sim_w1: int32 value counts, one per column");
  TORCH_CHECK(max_fake >= 0 && max_fake <= fake.size(1) && real.size(1) + max_fake < (int64_t)INT32_MAX,
              "sim_w1: max_fake outside the fake rows");
  TORCH_CHECK(sim_f64(out) && out.numel() == nc, "sim_w1: out float64 [n_cont]");
  if (nc == 0) return;
  const int64_t chunks = fedtgan::sim_w1_chunks(real.size(1) + max_fake);
  TORCH_CHECK(sim_f64(part) && part.numel() >= nc * chunks, "sim_w1: part needs ", nc * chunks, " float64");
  fedtgan::SimW1Args a{};
  a.real = real.data_ptr<double>();
  a.ldr = real.size(1);
  a.n_real = n_real.data_ptr<int>();
  a.fake = fake.data_ptr<double>();
  a.ldf = fake.size(1);
  a.n_fake = n_fake.data_ptr<int>();
  a.n_cont = (int)nc;
  a.max_real = (int)real.size(1);
  a.max_fake = (int)max_fake;
  a.part = part.data_ptr<double>();
  a.out = out.data_ptr<double>();
  fedtgan::launch_sim_w1(a, cur_stream());
}

void sim_jsd(const Tensor& real, const Tensor& fake, const Tensor& out) {
  TORCH_CHECK(sim_i32(real) && real.dim() == 2 && sim_i32(fake) && fake.dim() == 2 && fake.size(0) == real.size(0) &&
                  fake.size(1) == real.size(1), "sim_jsd: real / fake counts must be contiguous int32 of one shape");
  TORCH_CHECK(sim_f64(out) && out.numel() == real.size(0), "sim_jsd: out float64 [n_cat]");
  if (real.size(0) == 0) return;
  fedtgan::SimJsdArgs a{};
  a.real = real.data_ptr<int>();
  a.fake = fake.data_ptr<int>();
  a.ldc = (int)real.size(1);
  a.n_cat = (int)real.size(0);
  a.out = out.data_ptr<double>();
  fedtgan::launch_sim_jsd(a, cur_stream());
}

void sim_mean(const Tensor& scores, int64_t n_cat, int64_t n_cont) {
  TORCH_CHECK(sim_f64(scores) && n_cat >= 0 && n_cont >= 0 && scores.numel() == 2 + n_cat + n_cont,
              "sim_mean: scores float64 [2 + n_cat + n_cont]");
  fedtgan::launch_sim_mean(scores.data_ptr<double>(), (int)n_cat, (int)n_cont, cur_stream());
}

int64_t sim_sort_tile() { return fedtgan::SIM_SORT_TILE; }
int64_t sim_w1_chunks(int64_t n) { return fedtgan::sim_w1_chunks(n); }

// ----------------------------------------------------------------------------- privacy evaluator
void nn_pack(const Tensor& values, const Tensor& kind, const Tensor& slot, const Tensor& lo, const Tensor& scale,
             const Tensor& cont, const Tensor& cat) {
  TORCH_CHECK(sim_f64(values) && values.dim() == 2 && values.size(1) >= 1,
              "nn_pack: values must be contiguous float64 [rows, n_cols]");
  TORCH_CHECK(values.numel() < (int64_t)INT32_MAX, "nn_pack: a table holds fewer than 2^31 values");
  TORCH_CHECK(sim_i32(kind) && sim_i32(slot) && kind.numel() == values.size(1) && slot.numel() == values.size(1),
              "nn_pack: int32 kind / slot, one entry per column");
  TORCH_CHECK(sim_f64(cont) && cont.dim() == 2 && cont.size(0) >= values.size(0) && sim_i32(cat) && cat.dim() == 2 &&
                  cat.size(0) >= values.size(0), "nn_pack: cont float64 [>= rows, n_cont], cat int32 [>= rows, n_cat]");
  TORCH_CHECK(sim_f64(lo) && sim_f64(scale) && lo.numel() == cont.size(1) && scale.numel() == cont.size(1),
              "nn_pack: lo / scale float64 [n_cont]");
  fedtgan::NnPackArgs a{};
  a.values = values.data_ptr<double>();
  a.rows = (int)values.size(0);
  a.n_cols = (int)values.size(1);
  a.kind = kind.data_ptr<int>();
  a.slot = slot.data_ptr<int>();
  a.n_cont = (int)cont.size(1);
  a.n_cat = (int)cat.size(1);
  a.lo = a.n_cont ? lo.data_ptr<double>() : nullptr;
  a.scale = a.n_cont ? scale.data_ptr<double>() : nullptr;
  a.cont = a.n_cont ? cont.data_ptr<double>() : nullptr;
  a.cat = a.n_cat ? cat.data_ptr<int>() : nullptr;
  fedtgan::launch_nn_pack(a, cur_stream());
}

void nn_top2(const Tensor& q_cont, const Tensor& q_cat, const Tensor& r_cont, const Tensor& r_cat, bool exclude_self,
             const Tensor& d1, const Tensor& d2, const Tensor& i1, const Tensor& scratch) {
  TORCH_CHECK(sim_f64(q_cont) && q_cont.dim() == 2 && sim_i32(q_cat) && q_cat.dim() == 2 &&
                  q_cat.size(0) == q_cont.size(0), "nn_top2: queries float64 [nq, n_cont] and int32 [nq, n_cat]");
  TORCH_CHECK(sim_f64(r_cont) && r_cont.dim() == 2 && sim_i32(r_cat) && r_cat.dim() == 2 &&
                  r_cat.size(0) == r_cont.size(0) && r_cont.size(1) == q_cont.size(1) &&
                  r_cat.size(1) == q_cat.size(1), "nn_top2: reference rows with the queries' columns");
  const int64_t nq = q_cont.size(0), nr = r_cont.size(0);
  TORCH_CHECK(nr >= 1 && nr < (int64_t)INT32_MAX && nq < (int64_t)INT32_MAX && q_cont.size(1) + q_cat.size(1) >= 1,
              "nn_top2: at least one reference row and one column");
  TORCH_CHECK(!exclude_self || nq == nr, "nn_top2: exclude_self compares a table with itself");
  TORCH_CHECK(sim_f64(d1) && sim_f64(d2) && sim_i32(i1) && d1.numel() >= nq && d2.numel() >= nq && i1.numel() >= nq,
              "nn_top2: d1 / d2 float64 and i1 int32, one entry per query");
  TORCH_CHECK(sim_f64(scratch) && scratch.numel() >= fedtgan::nn_scratch_doubles(nq, nr), "nn_top2: scratch needs ",
              fedtgan::nn_scratch_doubles(nq, nr), " float64");
  if (nq == 0) return;
  fedtgan::NnTop2Args a{};
  a.nq = (int)nq;
  a.nr = (int)nr;
  a.n_cont = (int)q_cont.size(1);
  a.n_cat = (int)q_cat.size(1);
  a.q_cont = a.n_cont ? q_cont.data_ptr<double>() : nullptr;
  a.r_cont = a.n_cont ? r_cont.data_ptr<double>() : nullptr;
  a.q_cat = a.n_cat ? q_cat.data_ptr<int>() : nullptr;
  a.r_cat = a.n_cat ? r_cat.data_ptr<int>() : nullptr;
  a.exclude_self = exclude_self ? 1 : 0;
  fedtgan::launch_nn_top2(a, d1.data_ptr<double>(), d2.data_ptr<double>(), i1.data_ptr<int>(),
                          scratch.data_ptr<double>(), cur_stream());
}

void nn_within(const Tensor& q_cont, const Tensor& q_cat, const Tensor& r_cont, const Tensor& r_cat, const Tensor& t2,
               const Tensor& near, const Tensor& scratch) {
  TORCH_CHECK(sim_f64(q_cont) && q_cont.dim() == 2 && sim_i32(q_cat) && q_cat.dim() == 2 &&
                  q_cat.size(0) == q_cont.size(0), "nn_within: queries float64 [nq, n_cont] and int32 [nq, n_cat]");
  TORCH_CHECK(sim_f64(r_cont) && r_cont.dim() == 2 && sim_i32(r_cat) && r_cat.dim() == 2 &&
                  r_cat.size(0) == r_cont.size(0) && r_cont.size(1) == q_cont.size(1) &&
                  r_cat.size(1) == q_cat.size(1), "nn_within: reference rows with the queries' columns");
  const int64_t nq = q_cont.size(0), nr = r_cont.size(0);
  TORCH_CHECK(nr >= 1 && nr < (int64_t)INT32_MAX && nq < (int64_t)INT32_MAX && q_cont.size(1) + q_cat.size(1) >= 1,
              "nn_within: at least one reference row and one column");
  TORCH_CHECK(sim_f64(t2) && t2.numel() == 1, "nn_within: t2 is one float64 on the device");
  TORCH_CHECK(sim_i32(near) && near.numel() >= nq, "nn_within: near int32, one entry per query");
  // (the partials are int32: two to a float64 of the scratch nn_top2 uses)
  const int64_t slots = nq * fedtgan::nn_chunks(nr);
  TORCH_CHECK(sim_f64(scratch) && 2 * scratch.numel() >= slots, "nn_within: scratch needs ", (slots + 1) / 2,
              " float64");
  if (nq == 0) return;
  fedtgan::NnWithinArgs a{};
  a.nq = (int)nq;
  a.nr = (int)nr;
  a.n_cont = (int)q_cont.size(1);
  a.n_cat = (int)q_cat.size(1);
  a.q_cont = a.n_cont ? q_cont.data_ptr<double>() : nullptr;
  a.r_cont = a.n_cont ? r_cont.data_ptr<double>() : nullptr;
  a.q_cat = a.n_cat ? q_cat.data_ptr<int>() : nullptr;
  a.r_cat = a.n_cat ? r_cat.data_ptr<int>() : nullptr;
  a.t2 = t2.data_ptr<double>();
  a.near = near.data_ptr<int>();
  a.part = (int*)scratch.data_ptr<double>();
  fedtgan::launch_nn_within(a, cur_stream());
}

void guard_mark(const Tensor& near, const Tensor& tgt, const Tensor& stats) {
  const int64_t n = tgt.numel();
  TORCH_CHECK(sim_i32(near) && sim_i32(tgt) && near.numel() >= n && n < (int64_t)INT32_MAX,
              "guard_mark: near / tgt int32, one entry per row");
  TORCH_CHECK(stats.is_cuda() && stats.scalar_type() == at::kLong && stats.is_contiguous() && stats.numel() == 2,
              "guard_mark: stats int64 [2]");
  fedtgan::launch_guard_mark(near.data_ptr<int>(), tgt.data_ptr<int>(), (int)n, stats.data_ptr<int64_t>(),
                             cur_stream());
}

namespace {
bool nn_offsets(const Tensor& t, int64_t k) {
  return t.is_cuda() && t.scalar_type() == at::kLong && t.is_contiguous() && t.numel() == k;
}
}  // namespace

void nn_merge_shards(const Tensor& parts, const Tensor& offsets, const Tensor& d1, const Tensor& d2, const Tensor& i1,
                     const Tensor& owner, const Tensor& by_client) {
  TORCH_CHECK(sim_f64(parts) && parts.dim() == 3 && parts.size(2) == 3,
              "nn_merge_shards: parts must be contiguous float64 [K, n, 3]");
  const int64_t k = parts.size(0), n = parts.size(1);
  TORCH_CHECK(k >= 1 && k <= fedtgan::NN_MAX_SHARDS, "nn_merge_shards: 1..", fedtgan::NN_MAX_SHARDS, " shards, got ",
              k);
  TORCH_CHECK(n < (int64_t)INT32_MAX / 3, "nn_merge_shards: too many rows");
  TORCH_CHECK(nn_offsets(offsets, k), "nn_merge_shards: offsets int64 [K] on the device");
  TORCH_CHECK(sim_f64(d1) && sim_f64(d2) && sim_i32(i1) && sim_i32(owner) && d1.numel() >= n && d2.numel() >= n &&
                  i1.numel() >= n && owner.numel() >= n,
              "nn_merge_shards: d1 / d2 float64 and i1 / owner int32, one entry per row");
  TORCH_CHECK(by_client.is_cuda() && by_client.scalar_type() == at::kLong && by_client.is_contiguous() &&
                  by_client.numel() == 2 * k, "nn_merge_shards: by_client int64 [2, K]");
  fedtgan::NnMergeShardsArgs a{};
  a.parts = parts.data_ptr<double>();
  a.offsets = offsets.data_ptr<int64_t>();
  a.k = (int)k;
  a.n = (int)n;
  a.d1 = d1.data_ptr<double>();
  a.d2 = d2.data_ptr<double>();
  a.i1 = i1.data_ptr<int>();
  a.owner = owner.data_ptr<int>();
  a.by_client = (unsigned long long*)by_client.data_ptr<int64_t>();
  fedtgan::launch_nn_merge_shards(a, cur_stream());
}

void nn_within_merge_shards(const Tensor& near, const Tensor& offsets, const Tensor& near_out, const Tensor& owner) {
  TORCH_CHECK(sim_i32(near) && near.dim() == 2, "nn_within_merge_shards: near must be contiguous int32 [K, n]");
  const int64_t k = near.size(0), n = near.size(1);
  TORCH_CHECK(k >= 1 && k <= fedtgan::NN_MAX_SHARDS, "nn_within_merge_shards: 1..", fedtgan::NN_MAX_SHARDS,
              " shards, got ", k);
  TORCH_CHECK(n < (int64_t)INT32_MAX, "nn_within_merge_shards: too many rows");
  TORCH_CHECK(nn_offsets(offsets, k), "nn_within_merge_shards: offsets int64 [K] on the device");
  TORCH_CHECK(sim_i32(near_out) && sim_i32(owner) && near_out.numel() >= n && owner.numel() >= n,
              "nn_within_merge_shards: near_out / owner int32, one entry per row");
  fedtgan::launch_nn_within_merge_shards(near.data_ptr<int>(), offsets.data_ptr<int64_t>(), (int)k, (int)n,
                                         near_out.data_ptr<int>(), owner.data_ptr<int>(), cur_stream());
}

void nn_stats(const Tensor& d1, const Tensor& d2, int64_t n, const Tensor& keys, const Tensor& part) {
  TORCH_CHECK(sim_f64(d1) && sim_f64(d2) && n >= 1 && n < (int64_t)INT32_MAX && d1.numel() >= n && d2.numel() >= n,
              "nn_stats: d1 / d2 float64 with n >= 1 entries");
  TORCH_CHECK(sim_f64(keys) && keys.dim() == 2 && keys.size(0) == 2 && keys.size(1) >= n,
              "nn_stats: keys float64 [2, >= n]");
  TORCH_CHECK(sim_f64(part) && part.numel() >= 2 * (int64_t)fedtgan::nn_stats_blocks(n), "nn_stats: part needs ",
              2 * (int64_t)fedtgan::nn_stats_blocks(n), " float64");
  fedtgan::launch_nn_stats(d1.data_ptr<double>(), d2.data_ptr<double>(), (int)n, keys.data_ptr<double>(), keys.size(1),
                           part.data_ptr<double>(), cur_stream());
}

void nn_percentiles(const Tensor& keys, int64_t n, const Tensor& part, const Tensor& out) {
  TORCH_CHECK(sim_f64(keys) && keys.dim() == 2 && keys.size(0) == 2 && n >= 1 && keys.size(1) >= n &&
                  n < (int64_t)INT32_MAX, "nn_percentiles: keys float64 [2, >= n]");
  TORCH_CHECK(sim_f64(part) && part.numel() >= 2 * (int64_t)fedtgan::nn_stats_blocks(n) && sim_f64(out) &&
                  out.numel() >= 4, "nn_percentiles: part as nn_stats wrote it, out float64 [>= 4]");
  fedtgan::launch_nn_percentiles(keys.data_ptr<double>(), keys.size(1), (int)n, part.data_ptr<double>(),
                                 out.data_ptr<double>(), cur_stream());
}

int64_t nn_query_tile() { return fedtgan::NN_QUERY_TILE; }
int64_t nn_ref_tile() { return fedtgan::NN_REF_TILE; }
int64_t nn_chunk_rows() { return fedtgan::NN_CHUNK_ROWS; }
int64_t nn_chunks(int64_t nr) { return fedtgan::nn_chunks(nr); }
int64_t nn_scratch(int64_t nq, int64_t nr) { return fedtgan::nn_scratch_doubles(nq, nr); }
int64_t nn_stats_part(int64_t n) { return 2 * (int64_t)fedtgan::nn_stats_blocks(n); }

// ----------------------------------------------------------------------------- fidelity evaluator
namespace {
fedtgan::NnPairs nn_pairs(const char* what, const Tensor& q_cont, const Tensor& q_cat, const Tensor& r_cont,
                          const Tensor& r_cat) {
  TORCH_CHECK(sim_f64(q_cont) && q_cont.dim() == 2 && sim_i32(q_cat) && q_cat.dim() == 2 &&
                  q_cat.size(0) == q_cont.size(0), what, ": queries float64 [nq, n_cont] and int32 [nq, n_cat]");
  TORCH_CHECK(sim_f64(r_cont) && r_cont.dim() == 2 && sim_i32(r_cat) && r_cat.dim() == 2 &&
                  r_cat.size(0) == r_cont.size(0) && r_cont.size(1) == q_cont.size(1) &&
                  r_cat.size(1) == q_cat.size(1), what, ": reference rows with the queries' columns");
  const int64_t nq = q_cont.size(0), nr = r_cont.size(0);
  TORCH_CHECK(nr >= 1 && nr < (int64_t)INT32_MAX && nq < (int64_t)INT32_MAX && q_cont.size(1) + q_cat.size(1) >= 1,
              what, ": at least one reference row and one column");
  fedtgan::NnPairs p{};
  p.nq = (int)nq;
  p.nr = (int)nr;
  p.n_cont = (int)q_cont.size(1);
  p.n_cat = (int)q_cat.size(1);
  p.q_cont = p.n_cont ? q_cont.data_ptr<double>() : nullptr;
  p.r_cont = p.n_cont ? r_cont.data_ptr<double>() : nullptr;
  p.q_cat = p.n_cat ? q_cat.data_ptr<int>() : nullptr;
  p.r_cat = p.n_cat ? r_cat.data_ptr<int>() : nullptr;
  return p;
}
}  // namespace

void nn_topk(const Tensor& q_cont, const Tensor& q_cat, const Tensor& r_cont, const Tensor& r_cat, bool exclude_self,
             int64_t k, const Tensor& out, const Tensor& scratch) {
  fedtgan::NnTopkArgs a{};
  a.p = nn_pairs("nn_topk", q_cont, q_cat, r_cont, r_cat);
  TORCH_CHECK(k >= 1 && k <= fedtgan::FID_MAX_K, "nn_topk: k is 1..", fedtgan::FID_MAX_K, ", got ", k);
  TORCH_CHECK(!exclude_self || a.p.nq == a.p.nr, "nn_topk: exclude_self compares a table with itself");
  TORCH_CHECK(sim_f64(out) && out.numel() >= a.p.nq, "nn_topk: out float64, one entry per query");
  const int64_t need = fedtgan::nn_topk_scratch_doubles(a.p.nq, a.p.nr, (int)k);
  TORCH_CHECK(sim_f64(scratch) && scratch.numel() >= need, "nn_topk: scratch needs ", need, " float64");
  if (a.p.nq == 0) return;
  a.exclude_self = exclude_self ? 1 : 0;
  a.k = (int)k;
  a.out = out.data_ptr<double>();
  fedtgan::launch_nn_topk(a, scratch.data_ptr<double>(), cur_stream());
}

void nn_ball(const Tensor& q_cont, const Tensor& q_cat, const Tensor& r_cont, const Tensor& r_cat, const Tensor& r_rad2,
             const Tensor& cnt, const Tensor& dmin, const Tensor& scratch) {
  fedtgan::NnBallArgs a{};
  a.p = nn_pairs("nn_ball", q_cont, q_cat, r_cont, r_cat);
  TORCH_CHECK(sim_f64(r_rad2) && r_rad2.numel() >= a.p.nr, "nn_ball: r_rad2 float64, one entry per reference row");
  TORCH_CHECK(sim_i32(cnt) && cnt.numel() >= a.p.nq && sim_f64(dmin) && dmin.numel() >= a.p.nq,
              "nn_ball: cnt int32 and dmin float64, one entry per query");
  const int64_t need = fedtgan::nn_ball_scratch_doubles(a.p.nq, a.p.nr);
  TORCH_CHECK(sim_f64(scratch) && scratch.numel() >= need, "nn_ball: scratch needs ", need, " float64");
  if (a.p.nq == 0) return;
  a.r_rad2 = r_rad2.data_ptr<double>();
  a.cnt = cnt.data_ptr<int>();
  a.dmin = dmin.data_ptr<double>();
  fedtgan::launch_nn_ball(a, scratch.data_ptr<double>(), cur_stream());
}

void prdc_reduce(const Tensor& cnt_a, const Tensor& cnt_b, const Tensor& dmin_b, const Tensor& rr, int64_t n, int64_t m,
                 int64_t k, const Tensor& scores) {
  TORCH_CHECK(n >= 1 && m >= 1 && n < (int64_t)INT32_MAX && m < (int64_t)INT32_MAX && k >= 1 &&
                  k <= fedtgan::FID_MAX_K, "prdc_reduce: n >= 1, m >= 1, k in 1..", fedtgan::FID_MAX_K);
  TORCH_CHECK(sim_i32(cnt_a) && cnt_a.numel() >= n, "prdc_reduce: cnt_a int32 [>= n]");
  TORCH_CHECK(sim_i32(cnt_b) && cnt_b.numel() >= m && sim_f64(dmin_b) && dmin_b.numel() >= m && sim_f64(rr) &&
                  rr.numel() >= m, "prdc_reduce: cnt_b int32, dmin_b / rr float64, [>= m] each");
  TORCH_CHECK(sim_f64(scores) && scores.numel() >= 4, "prdc_reduce: scores float64 [>= 4]");
  fedtgan::PrdcArgs a{};
  a.cnt_a = cnt_a.data_ptr<int>();
  a.cnt_b = cnt_b.data_ptr<int>();
  a.dmin_b = dmin_b.data_ptr<double>();
  a.rr = rr.data_ptr<double>();
  a.n = (int)n;
  a.m = (int)m;
  a.k = (int)k;
  a.scores = scores.data_ptr<double>();
  fedtgan::launch_prdc_reduce(a, cur_stream());
}

int64_t fid_max_k() { return fedtgan::FID_MAX_K; }
int64_t nn_topk_scratch(int64_t nq, int64_t nr, int64_t k) {
  TORCH_CHECK(k >= 1 && k <= fedtgan::FID_MAX_K, "nn_topk_scratch: k is 1..", fedtgan::FID_MAX_K);
  return fedtgan::nn_topk_scratch_doubles(nq, nr, (int)k);
}
int64_t nn_ball_scratch(int64_t nq, int64_t nr) { return fedtgan::nn_ball_scratch_doubles(nq, nr); }

// ----------------------------------------------------------------------------- correlation evaluator
namespace {
bool corr_i64(const Tensor& t) { return t.is_cuda() && t.scalar_type() == at::kLong && t.is_contiguous(); }
}  // namespace

void corr_pack(const Tensor& values, const Tensor& kind, const Tensor& slot, const Tensor& card, const Tensor& cont,
               const Tensor& cat_t, const Tensor& mean, const Tensor& part) {
  TORCH_CHECK(sim_f64(values) && values.dim() == 2 && values.size(0) >= 1 && values.size(1) >= 1,
              "corr_pack: values must be contiguous float64 [rows >= 1, n_cols]");
  TORCH_CHECK(values.numel() < (int64_t)INT32_MAX, "corr_pack: a table holds fewer than 2^31 values");
  const int64_t rows = values.size(0);
  TORCH_CHECK(sim_i32(kind) && sim_i32(slot) && kind.numel() == values.size(1) && slot.numel() == values.size(1),
              "corr_pack: int32 kind / slot, one entry per column");
  TORCH_CHECK(sim_f64(cont) && cont.dim() == 2 && cont.size(0) >= rows && sim_i32(cat_t) && cat_t.dim() == 2 &&
                  cat_t.size(1) >= rows, "corr_pack: cont float64 [>= rows, n_cont], cat_t int32 [n_cat, >= rows]");
  TORCH_CHECK(cont.size(1) + cat_t.size(0) == values.size(1), "corr_pack: n_cont + n_cat must be n_cols");
  TORCH_CHECK(sim_i32(card) && card.numel() == cat_t.size(0) && sim_f64(mean) && mean.numel() == cont.size(1),
              "corr_pack: card int32 [n_cat], mean float64 [n_cont]");
  const int64_t chunks = (rows + fedtgan::CORR_CHUNK - 1) / fedtgan::CORR_CHUNK;
  TORCH_CHECK(sim_f64(part) && part.numel() >= chunks * cont.size(1), "corr_pack: part needs ", chunks * cont.size(1),
              " float64");
  fedtgan::CorrPackArgs a{};
  a.values = values.data_ptr<double>();
  a.rows = (int)rows;
  a.n_cols = (int)values.size(1);
  a.kind = kind.data_ptr<int>();
  a.slot = slot.data_ptr<int>();
  a.n_cont = (int)cont.size(1);
  a.n_cat = (int)cat_t.size(0);
  a.card = a.n_cat ? card.data_ptr<int>() : nullptr;
  a.cont = a.n_cont ? cont.data_ptr<double>() : nullptr;
  a.cat_t = a.n_cat ? cat_t.data_ptr<int>() : nullptr;
  a.ldk = cat_t.size(1);
  a.mean = a.n_cont ? mean.data_ptr<double>() : nullptr;
  a.part = part.data_ptr<double>();
  fedtgan::launch_corr_pack(a, cur_stream());
}

void corr_moments(const Tensor& cont, const Tensor& cat_t, int64_t n, const Tensor& mean, const Tensor& card,
                  const Tensor& offs, const Tensor& G, const Tensor& part) {
  TORCH_CHECK(sim_f64(cont) && cont.dim() == 2 && sim_i32(cat_t) && cat_t.dim() == 2 && n >= 1 && cont.size(0) >= n &&
                  cat_t.size(1) >= n && n < (int64_t)INT32_MAX,
              "corr_moments: cont float64 [>= n, n_cont], cat_t int32 [n_cat, >= n]");
  const int64_t n_cont = cont.size(1), n_cat = cat_t.size(0);
  TORCH_CHECK(sim_f64(mean) && mean.numel() == n_cont && sim_i32(card) && card.numel() == n_cat && sim_i32(offs) &&
                  offs.numel() == n_cat + 1, "corr_moments: mean [n_cont], card [n_cat], offs [n_cat + 1]");
  TORCH_CHECK(sim_f64(G) && G.dim() == 2 && G.size(1) == n_cont && G.size(0) >= n_cont,
              "corr_moments: G float64 [W, n_cont]");
  const int64_t W = G.size(0);
  TORCH_CHECK(W < (int64_t)INT32_MAX && W * n_cont < (int64_t)INT32_MAX, "corr_moments: G too large");
  const fedtgan::CorrGroups gr = fedtgan::corr_groups(n, W, n_cont);
  TORCH_CHECK(sim_f64(part) && part.numel() >= (int64_t)gr.groups * W * n_cont, "corr_moments: part needs ",
              (int64_t)gr.groups * W * n_cont, " float64");
  if (n_cont == 0) return;
  fedtgan::CorrMomentsArgs a{};
  a.cont = cont.data_ptr<double>();
  a.cat_t = n_cat ? cat_t.data_ptr<int>() : nullptr;
  a.ldk = cat_t.size(1);
  a.n = (int)n;
  a.n_cont = (int)n_cont;
  a.n_cat = (int)n_cat;
  a.W = (int)W;
  a.mean = mean.data_ptr<double>();
  a.card = n_cat ? card.data_ptr<int>() : nullptr;
  a.offs = offs.data_ptr<int>();
  a.G = G.data_ptr<double>();
  a.part = part.data_ptr<double>();
  fedtgan::launch_corr_moments(a, cur_stream());
}

void corr_counts(const Tensor& cat_t, int64_t n, const Tensor& pairs, const Tensor& poff, const Tensor& counts,
                 int64_t lds_bins) {
  TORCH_CHECK(sim_i32(cat_t) && cat_t.dim() == 2 && n >= 1 && cat_t.size(1) >= n && n < (int64_t)INT32_MAX,
              "corr_counts: cat_t int32 [n_cat, >= n]");
  TORCH_CHECK(sim_i32(pairs) && pairs.dim() == 2 && pairs.size(1) == 4 && corr_i64(poff) &&
                  poff.numel() == pairs.size(0) + 1 && pairs.size(0) < (int64_t)INT32_MAX,
              "corr_counts: pairs int32 [P, 4], poff int64 [P + 1]");
  TORCH_CHECK(sim_i32(counts) && lds_bins >= 1 && lds_bins <= fedtgan::CORR_LDS_BINS,
              "corr_counts: counts int32, lds_bins in 1..CORR_LDS_BINS");
  fedtgan::CorrCountsArgs a{};
  a.cat_t = cat_t.data_ptr<int>();
  a.ldk = cat_t.size(1);
  a.n = (int)n;
  a.n_cat = (int)cat_t.size(0);
  a.n_pairs = (int)pairs.size(0);
  a.pairs = pairs.data_ptr<int>();
  a.poff = poff.data_ptr<int64_t>();
  a.counts = counts.data_ptr<int>();
  a.total = counts.numel();
  a.lds_bins = (int)lds_bins;
  fedtgan::launch_corr_counts(a, cur_stream());
}

void corr_matrix(const Tensor& G, const Tensor& counts, const Tensor& poff, const Tensor& kind, const Tensor& slot,
                 const Tensor& card, const Tensor& offs, int64_t n, const Tensor& A) {
  TORCH_CHECK(sim_f64(A) && A.dim() == 2 && A.size(0) == A.size(1) && A.size(0) >= 1, "corr_matrix: A float64 [C, C]");
  const int64_t C = A.size(0);
  TORCH_CHECK(sim_i32(kind) && sim_i32(slot) && kind.numel() == C && slot.numel() == C,
              "corr_matrix: int32 kind / slot, one entry per column");
  const int64_t n_cat = card.numel(), n_cont = C - n_cat;
  TORCH_CHECK(sim_i32(card) && sim_i32(offs) && n_cont >= 0 && offs.numel() == n_cat + 1,
              "corr_matrix: card int32 [n_cat], offs int32 [n_cat + 1]");
  // (G must also cover n_cont + offs[n_cat] rows; offs lives on the device, so the kernel checks that per entry)
  TORCH_CHECK(sim_f64(G) && G.dim() == 2 && G.size(1) == n_cont && G.size(0) >= n_cont,
              "corr_matrix: G float64 [W >= n_cont, n_cont]");
  TORCH_CHECK(sim_i32(counts) && corr_i64(poff) && poff.numel() == 1 + n_cat + n_cat * (n_cat - 1) / 2,
              "corr_matrix: counts int32, poff int64 [1 + n_cat + n_cat (n_cat - 1) / 2]");
  TORCH_CHECK(n >= 1 && n < (int64_t)INT32_MAX, "corr_matrix: n");
  fedtgan::CorrMatrixArgs a{};
  a.G = G.data_ptr<double>();
  a.counts = counts.data_ptr<int>();
  a.poff = poff.data_ptr<int64_t>();
  a.total = counts.numel();
  a.n_pairs = (int)poff.numel() - 1;
  a.kind = kind.data_ptr<int>();
  a.slot = slot.data_ptr<int>();
  a.card = n_cat ? card.data_ptr<int>() : nullptr;
  a.offs = offs.data_ptr<int>();
  a.n = (int)n;
  a.C = (int)C;
  a.n_cont = (int)n_cont;
  a.n_cat = (int)n_cat;
  a.W = (int)G.size(0);
  a.A = A.data_ptr<double>();
  fedtgan::launch_corr_matrix(a, cur_stream());
}

void corr_diff(const Tensor& A, const Tensor& B, const Tensor& out) {
  TORCH_CHECK(sim_f64(A) && sim_f64(B) && A.dim() == 2 && A.size(0) == A.size(1) && A.size(0) >= 1 && B.dim() == 2 &&
                  B.size(0) == A.size(0) && B.size(1) == A.size(0), "corr_diff: two float64 [C, C] matrices");
  TORCH_CHECK(sim_f64(out) && out.numel() >= 3, "corr_diff: out float64 [>= 3]");
  fedtgan::launch_corr_diff(A.data_ptr<double>(), B.data_ptr<double>(), (int)A.size(0), out.data_ptr<double>(),
                            cur_stream());
}

int64_t corr_chunk() { return fedtgan::CORR_CHUNK; }
int64_t corr_lds_bins() { return fedtgan::CORR_LDS_BINS; }
int64_t corr_part(int64_t n_max, int64_t W, int64_t n_cont) { return fedtgan::corr_part_doubles(n_max, W, n_cont); }
int64_t corr_groups(int64_t n, int64_t W, int64_t n_cont) { return fedtgan::corr_groups(n, W, n_cont).groups; }

// ----------------------------------------------------------------------------- ML-utility evaluator
namespace {
// the packed table of the util_* ops: cont [>= n, n_cont], cat_t [n_cat, >= n], y / s [>= n], counts [K], info [4]
fedtgan::UtilTable util_table(const char* what, const Tensor& cont, const Tensor& cat_t, const Tensor& y,
                              const Tensor& s, const Tensor& counts, const Tensor& info, const Tensor& card,
                              const Tensor& offs, int64_t n, int64_t D) {
  TORCH_CHECK(n >= 1 && n < (int64_t)INT32_MAX, what, ": n");
  TORCH_CHECK(sim_f64(cont) && cont.dim() == 2 && cont.size(0) >= n && sim_i32(cat_t) && cat_t.dim() == 2 &&
                  cat_t.size(1) >= n, what, ": cont float64 [>= n, n_cont], cat_t int32 [n_cat, >= n]");
  TORCH_CHECK(sim_i32(y) && y.numel() >= n && sim_f64(s) && s.numel() >= n, what, ": y int32 [>= n], s float64 [>= n]");
  const int64_t n_cat = cat_t.size(0), n_cont = cont.size(1), K = counts.numel();
  TORCH_CHECK(sim_i32(counts) && K >= 1 && K <= fedtgan::UTIL_MAX_CLASSES && sim_f64(info) && info.numel() >= 4, what,
              ": counts int32 [K <= UTIL_MAX_CLASSES], info float64 [4]");
  TORCH_CHECK(sim_i32(card) && card.numel() == n_cat && sim_i32(offs) && offs.numel() == n_cat + 1, what,
              ": card int32 [n_cat], offs int32 [n_cat + 1]");
  TORCH_CHECK(D >= n_cont + 2 * n_cat + 1 && D <= fedtgan::UTIL_MAX_FEATURES, what,
              ": D must cover the features and stay within UTIL_MAX_FEATURES");
  fedtgan::UtilTable t{};
  t.cont = n_cont ? cont.data_ptr<double>() : nullptr;
  t.cat_t = n_cat ? cat_t.data_ptr<int>() : nullptr;
  t.y = y.data_ptr<int>();
  t.s = s.data_ptr<double>();
  t.counts = counts.data_ptr<int>();
  t.info = info.data_ptr<double>();
  t.ldk = cat_t.size(1);
  t.n = (int)n;
  t.n_cont = (int)n_cont;
  t.n_cat = (int)n_cat;
  t.D = (int)D;
  t.K = (int)K;
  t.card = n_cat ? card.data_ptr<int>() : nullptr;
  t.offs = offs.data_ptr<int>();
  return t;
}

void util_check_point(const char* what, const Tensor& P, int64_t D, int64_t K) {
  TORCH_CHECK(sim_f64(P) && P.dim() == 2 && P.size(0) == D && P.size(1) == K, what, ": float64 [D, K] expected");
}
}  // namespace

void util_pack(const Tensor& values, const Tensor& kind, const Tensor& slot, const Tensor& card, const Tensor& offs,
               const Tensor& mean, const Tensor& sd, int64_t D, const Tensor& cont, const Tensor& cat_t,
               const Tensor& y, const Tensor& s, const Tensor& counts, const Tensor& info) {
  TORCH_CHECK(sim_f64(values) && values.dim() == 2 && values.size(0) >= 1 && values.size(1) >= 1,
              "util_pack: values must be contiguous float64 [rows >= 1, n_cols]");
  TORCH_CHECK(values.numel() < (int64_t)INT32_MAX, "util_pack: a table holds fewer than 2^31 values");
  TORCH_CHECK(sim_i32(kind) && sim_i32(slot) && kind.numel() == values.size(1) && slot.numel() == values.size(1),
              "util_pack: int32 kind / slot, one entry per column");
  fedtgan::UtilPackArgs a{};
  a.t = util_table("util_pack", cont, cat_t, y, s, counts, info, card, offs, values.size(0), D);
  TORCH_CHECK(cont.size(1) + cat_t.size(0) + 1 == values.size(1), "util_pack: n_cont + n_cat + 1 must be n_cols");
  TORCH_CHECK(sim_f64(mean) && sim_f64(sd) && mean.numel() == cont.size(1) && sd.numel() == cont.size(1),
              "util_pack: mean / sd float64 [n_cont]");
  a.values = values.data_ptr<double>();
  a.n_cols = (int)values.size(1);
  a.kind = kind.data_ptr<int>();
  a.slot = slot.data_ptr<int>();
  a.mean = a.t.n_cont ? mean.data_ptr<double>() : nullptr;
  a.sd = a.t.n_cont ? sd.data_ptr<double>() : nullptr;
  fedtgan::launch_util_pack(a, cur_stream());
}

void util_gram(const Tensor& cont, const Tensor& cat_t, const Tensor& y, const Tensor& s, const Tensor& counts,
               const Tensor& info, const Tensor& card, const Tensor& offs, int64_t n, const Tensor& M,
               const Tensor& part) {
  TORCH_CHECK(sim_f64(M) && M.dim() == 2 && M.size(0) == M.size(1) && M.size(0) >= 1, "util_gram: M float64 [D, D]");
  const int64_t D = M.size(0);
  const fedtgan::UtilTable t = util_table("util_gram", cont, cat_t, y, s, counts, info, card, offs, n, D);
  const int64_t need = (int64_t)fedtgan::util_groups(n, D * D).groups * D * D;
  TORCH_CHECK(sim_f64(part) && part.numel() >= need, "util_gram: part needs ", need, " float64");
  fedtgan::launch_util_gram(t, M.data_ptr<double>(), part.data_ptr<double>(), cur_stream());
}

void util_factor(const Tensor& M, const Tensor& Lt, const Tensor& X, const Tensor& Minv) {
  TORCH_CHECK(sim_f64(M) && M.dim() == 2 && M.size(0) == M.size(1) && M.size(0) >= 1 &&
                  M.size(0) <= fedtgan::UTIL_MAX_FEATURES, "util_factor: M float64 [D, D], D <= UTIL_MAX_FEATURES");
  for (const Tensor* t : {&Lt, &X, &Minv})
    TORCH_CHECK(sim_f64(*t) && t->numel() == M.numel(), "util_factor: Lt, X, Minv float64 [D, D]");
  fedtgan::launch_util_factor(M.data_ptr<double>(), (int)M.size(0), Lt.data_ptr<double>(), X.data_ptr<double>(),
                              Minv.data_ptr<double>(), cur_stream());
}

void util_grad(const Tensor& cont, const Tensor& cat_t, const Tensor& y, const Tensor& s, const Tensor& counts,
               const Tensor& info, const Tensor& card, const Tensor& offs, int64_t n, const Tensor& P, const Tensor& G,
               const Tensor& loss, const Tensor& part, const Tensor& lossp) {
  TORCH_CHECK(P.dim() == 2, "util_grad: P float64 [D, K]");
  const int64_t D = P.size(0), K = counts.numel();
  const fedtgan::UtilTable t = util_table("util_grad", cont, cat_t, y, s, counts, info, card, offs, n, D);
  util_check_point("util_grad: P", P, D, K);
  util_check_point("util_grad: G", G, D, K);
  const int64_t groups = fedtgan::util_groups(n, D * K).groups;
  TORCH_CHECK(sim_f64(part) && part.numel() >= groups * D * K && sim_f64(lossp) && lossp.numel() >= groups,
              "util_grad: part needs ", groups * D * K, " float64, lossp ", groups);
  TORCH_CHECK(sim_f64(loss) && loss.numel() >= 1, "util_grad: loss float64 [1]");
  fedtgan::launch_util_grad(t, P.data_ptr<double>(), G.data_ptr<double>(), loss.data_ptr<double>(),
                            part.data_ptr<double>(), lossp.data_ptr<double>(), cur_stream());
}

void util_step(const Tensor& cont, const Tensor& cat_t, const Tensor& y, const Tensor& s, const Tensor& counts,
               const Tensor& info, const Tensor& card, const Tensor& offs, int64_t n, const Tensor& V, const Tensor& W,
               const Tensor& Minv, const Tensor& G, const Tensor& loss, const Tensor& part, const Tensor& lossp,
               double beta) {
  util_grad(cont, cat_t, y, s, counts, info, card, offs, n, V, G, loss, part, lossp);
  const int64_t D = V.size(0), K = V.size(1);
  util_check_point("util_step: W", W, D, K);
  TORCH_CHECK(sim_f64(Minv) && Minv.dim() == 2 && Minv.size(0) == D && Minv.size(1) == D,
              "util_step: Minv float64 [D, D]");
  fedtgan::launch_util_update(V.data_ptr<double>(), W.data_ptr<double>(), Minv.data_ptr<double>(),
                              G.data_ptr<double>(), (int)D, (int)K, beta, cur_stream());
}

void util_predict(const Tensor& cont, const Tensor& cat_t, const Tensor& y, const Tensor& s, const Tensor& counts,
                  const Tensor& info, const Tensor& card, const Tensor& offs, int64_t n, const Tensor& train_counts,
                  const Tensor& W, const Tensor& conf, const Tensor& G, const Tensor& loss, const Tensor& real,
                  const Tensor& out) {
  TORCH_CHECK(W.dim() == 2, "util_predict: W float64 [D, K]");
  const int64_t D = W.size(0), K = counts.numel();
  const fedtgan::UtilTable t = util_table("util_predict", cont, cat_t, y, s, counts, info, card, offs, n, D);
  util_check_point("util_predict: W", W, D, K);
  util_check_point("util_predict: G", G, D, K);
  TORCH_CHECK(sim_i32(train_counts) && train_counts.numel() == K && sim_i32(conf) && conf.numel() == K * K,
              "util_predict: train_counts int32 [K], conf int32 [K, K]");
  TORCH_CHECK(sim_f64(loss) && loss.numel() >= 1 && sim_f64(real) && real.numel() >= 2 && sim_f64(out) &&
                  out.numel() >= 8, "util_predict: loss [1], real [2], out [8] float64");
  fedtgan::launch_util_predict(t, train_counts.data_ptr<int>(), W.data_ptr<double>(), conf.data_ptr<int>(),
                               G.data_ptr<double>(), loss.data_ptr<double>(), real.data_ptr<double>(),
                               out.data_ptr<double>(), cur_stream());
}

int64_t util_max_features() { return fedtgan::UTIL_MAX_FEATURES; }
int64_t util_max_classes() { return fedtgan::UTIL_MAX_CLASSES; }
int64_t util_chunk() { return fedtgan::UTIL_CHUNK; }
int64_t util_part(int64_t n_max, int64_t D, int64_t K) { return fedtgan::util_part_doubles(n_max, D, K); }
int64_t util_groups(int64_t n, int64_t cells) { return fedtgan::util_groups(n, cells).groups; }

// ----------------------------------------------------------------------------- MLP-utility evaluator
namespace {
void mlp_check_theta(const char* what, const Tensor& theta, int64_t D, int64_t H, int64_t K) {
  TORCH_CHECK(H >= 1 && H <= fedtgan::MLP_MAX_HIDDEN, what, ": H must be 1 .. MLP_MAX_HIDDEN");
  TORCH_CHECK(sim_f64(theta) && theta.numel() == D * H + (H + 1) * K, what, ": float64 [D H + (H + 1) K] expected");
}
}  // namespace

void mlp_step(const Tensor& cont, const Tensor& cat_t, const Tensor& y, const Tensor& s, const Tensor& counts,
              const Tensor& info, const Tensor& card, const Tensor& offs, int64_t n, int64_t D, int64_t b, int64_t nb,
              const Tensor& theta, const Tensor& mom, const Tensor& var, const Tensor& h, const Tensor& dz,
              const Tensor& dh, const Tensor& cnt, int64_t H, double alpha, double lr_t) {
  fedtgan::MlpStepArgs a{};
  a.t = util_table("mlp_step", cont, cat_t, y, s, counts, info, card, offs, n, D);
  const int64_t K = counts.numel();
  mlp_check_theta("mlp_step: theta", theta, D, H, K);
  mlp_check_theta("mlp_step: m", mom, D, H, K);
  mlp_check_theta("mlp_step: v", var, D, H, K);
  TORCH_CHECK(nb >= 1 && nb <= n && b >= 0 && b < nb, "mlp_step: batch b of nb, 0 <= b < nb <= n");
  const int64_t rows = fedtgan::mlp_batch_rows(n, b, nb), blocks = (rows + fedtgan::MLP_ROWS - 1) / fedtgan::MLP_ROWS;
  TORCH_CHECK(rows >= 1 && rows <= fedtgan::MLP_MAX_BATCH, "mlp_step: a batch of ", rows,
              " rows; MLP_MAX_BATCH = ", fedtgan::MLP_MAX_BATCH);
  TORCH_CHECK(sim_f64(h) && h.numel() >= rows * H && sim_f64(dh) && dh.numel() >= rows * H && sim_f64(dz) &&
                  dz.numel() >= rows * K && sim_i32(cnt) && cnt.numel() >= blocks,
              "mlp_step: scratch h / dh float64 [rows, H], dz float64 [rows, K], cnt int32 [row blocks] for ", rows,
              " rows");
  a.b = (int)b;
  a.nb = (int)nb;
  a.H = (int)H;
  a.theta = theta.data_ptr<double>();
  a.mom = mom.data_ptr<double>();
  a.var = var.data_ptr<double>();
  a.h = h.data_ptr<double>();
  a.dz = dz.data_ptr<double>();
  a.dh = dh.data_ptr<double>();
  a.cnt = cnt.data_ptr<int>();
  a.alpha = alpha;
  a.lr_t = lr_t;
  fedtgan::launch_mlp_step(a, cur_stream());
}

void mlp_loss(const Tensor& cont, const Tensor& cat_t, const Tensor& y, const Tensor& s, const Tensor& counts,
              const Tensor& info, const Tensor& card, const Tensor& offs, int64_t n, int64_t D, const Tensor& theta,
              int64_t H, double alpha, const Tensor& loss) {
  const fedtgan::UtilTable t = util_table("mlp_loss", cont, cat_t, y, s, counts, info, card, offs, n, D);
  mlp_check_theta("mlp_loss: theta", theta, D, H, counts.numel());
  const int64_t need = 1 + (n + fedtgan::MLP_ROWS - 1) / fedtgan::MLP_ROWS;
  TORCH_CHECK(sim_f64(loss) && loss.numel() >= need, "mlp_loss: loss needs ", need, " float64");
  fedtgan::launch_mlp_loss(t, theta.data_ptr<double>(), (int)H, alpha, loss.data_ptr<double>(), cur_stream());
}

void mlp_predict(const Tensor& cont, const Tensor& cat_t, const Tensor& y, const Tensor& s, const Tensor& counts,
                 const Tensor& info, const Tensor& card, const Tensor& offs, int64_t n, int64_t D,
                 const Tensor& train_counts, const Tensor& theta, int64_t H, const Tensor& conf, const Tensor& loss,
                 const Tensor& real, const Tensor& out) {
  const fedtgan::UtilTable t = util_table("mlp_predict", cont, cat_t, y, s, counts, info, card, offs, n, D);
  const int64_t K = counts.numel();
  mlp_check_theta("mlp_predict: theta", theta, D, H, K);
  TORCH_CHECK(sim_i32(train_counts) && train_counts.numel() == K && sim_i32(conf) && conf.numel() == K * K,
              "mlp_predict: train_counts int32 [K], conf int32 [K, K]");
  TORCH_CHECK(sim_f64(loss) && loss.numel() >= 1 && sim_f64(real) && real.numel() >= 2 && sim_f64(out) &&
                  out.numel() >= 7, "mlp_predict: loss [1], real [2], out [7] float64");
  fedtgan::launch_mlp_predict(t, train_counts.data_ptr<int>(), theta.data_ptr<double>(), (int)H, conf.data_ptr<int>(),
                              loss.data_ptr<double>(), real.data_ptr<double>(), out.data_ptr<double>(), cur_stream());
}

int64_t mlp_max_hidden() { return fedtgan::MLP_MAX_HIDDEN; }
int64_t mlp_max_batch() { return fedtgan::MLP_MAX_BATCH; }
int64_t mlp_max_steps() { return fedtgan::MLP_MAX_STEPS; }
int64_t mlp_rows() { return fedtgan::MLP_ROWS; }

// ----------------------------------------------------------------------------- tree-utility evaluator
namespace {
bool tree_u8(const Tensor& t) { return t.is_cuda() && t.scalar_type() == at::kByte && t.is_contiguous(); }

// a binned table: bins uint8 [F, ld >= n], y int32 [>= n], counts int32 [K], cw float64 [K]
fedtgan::TreeTable tree_table(const char* what, const Tensor& bins, const Tensor& y, const Tensor& counts,
                              const Tensor& cw, int64_t n) {
  TORCH_CHECK(n >= 1 && n < (int64_t)INT32_MAX, what, ": n");
  TORCH_CHECK(tree_u8(bins) && bins.dim() == 2 && bins.size(0) >= 1 && bins.size(0) <= fedtgan::TREE_MAX_FEATURES &&
                  bins.size(1) >= n, what, ": bins uint8 [1 <= F <= TREE_MAX_FEATURES, >= n]");
  const int64_t K = cw.numel();
  TORCH_CHECK(sim_i32(y) && y.numel() >= n && sim_i32(counts) && counts.numel() == K && sim_f64(cw) && K >= 1 &&
                  K <= fedtgan::TREE_MAX_CLASSES, what, ": y int32 [>= n], counts int32 [K], cw float64 [K <= 64]");
  fedtgan::TreeTable t{};
  t.bins = bins.data_ptr<uint8_t>();
  t.y = y.data_ptr<int>();
  t.counts = counts.data_ptr<int>();
  t.cw = cw.data_ptr<double>();
  t.ld = bins.size(1);
  t.n = (int)n;
  t.F = (int)bins.size(0);
  t.K = (int)K;
  return t;
}

void tree_check_nodes(const char* what, const Tensor& feature, const Tensor& bin, const Tensor& left,
                      const Tensor& counts, int64_t K) {
  TORCH_CHECK(sim_i32(feature) && feature.dim() == 2 && feature.size(0) >= 1 && feature.size(0) <= 65535 &&
                  feature.size(1) >= 1, what, ": feature int32 [T <= 65535, cap]");
  for (const Tensor* t : {&bin, &left})
    TORCH_CHECK(sim_i32(*t) && t->sizes() == feature.sizes(), what, ": bin / left int32 [T, cap]");
  TORCH_CHECK(sim_i32(counts) && counts.dim() == 3 && counts.size(0) == feature.size(0) &&
                  counts.size(1) == feature.size(1) && counts.size(2) == K, what, ": counts int32 [T, cap, K]");
}
}  // namespace

void tree_pack(const Tensor& values, const Tensor& kind, const Tensor& slot, const Tensor& card, const Tensor& edges,
               const Tensor& eoff, const Tensor& bins, const Tensor& y, const Tensor& counts, const Tensor& cw) {
  TORCH_CHECK(sim_f64(values) && values.dim() == 2 && values.size(0) >= 1 && values.size(1) >= 2,
              "tree_pack: values must be contiguous float64 [rows >= 1, n_cols >= 2]");
  TORCH_CHECK(values.numel() < (int64_t)INT32_MAX, "tree_pack: a table holds fewer than 2^31 values");
  TORCH_CHECK(sim_i32(kind) && sim_i32(slot) && kind.numel() == values.size(1) && slot.numel() == values.size(1),
              "tree_pack: int32 kind / slot, one entry per column");
  fedtgan::TreePackArgs a{};
  a.t = tree_table("tree_pack", bins, y, counts, cw, values.size(0));
  TORCH_CHECK(bins.size(0) + 1 == values.size(1), "tree_pack: F + 1 must be n_cols");
  TORCH_CHECK(sim_i32(card) && card.numel() == a.t.F && sim_i32(eoff) && eoff.numel() == a.t.F + 1 && sim_f64(edges),
              "tree_pack: card int32 [F], eoff int32 [F + 1], edges float64");
  a.values = values.data_ptr<double>();
  a.n_cols = (int)values.size(1);
  a.kind = kind.data_ptr<int>();
  a.slot = slot.data_ptr<int>();
  a.card = card.data_ptr<int>();
  a.edges = edges.numel() ? edges.data_ptr<double>() : nullptr;
  a.eoff = eoff.data_ptr<int>();
  a.n_edges = (int)edges.numel();
  fedtgan::launch_tree_pack(a, cur_stream());
}

void tree_bootstrap(const Tensor& mult, int64_t n, bool bootstrap, int64_t seed) {
  TORCH_CHECK(sim_i32(mult) && mult.dim() == 2 && mult.size(0) >= 1 && mult.size(0) <= 65535 && n >= 1 &&
                  mult.size(1) >= n && n < (int64_t)INT32_MAX, "tree_bootstrap: mult int32 [T <= 65535, >= n]");
  fedtgan::launch_tree_bootstrap(mult.data_ptr<int>(), (int)mult.size(0), mult.size(1), (int)n, bootstrap ? 1 : 0,
                                 (uint64_t)seed, cur_stream());
}

void tree_grow(const Tensor& bins, const Tensor& y, const Tensor& tcounts, const Tensor& cw, const Tensor& nbins,
               int64_t max_bins, int64_t n, const Tensor& mult, const Tensor& rows, const Tensor& feature,
               const Tensor& bin, const Tensor& left, const Tensor& heap, const Tensor& counts, const Tensor& seg,
               const Tensor& level, const Tensor& lcounts, int64_t max_depth, int64_t min_leaf, int64_t m_feat,
               int64_t seed) {
  fedtgan::TreeGrowArgs a{};
  a.t = tree_table("tree_grow", bins, y, tcounts, cw, n);
  const int64_t K = a.t.K, F = a.t.F;
  tree_check_nodes("tree_grow", feature, bin, left, counts, K);
  const int64_t T = feature.size(0), cap = feature.size(1);
  TORCH_CHECK(sim_i32(heap) && heap.sizes() == feature.sizes() && sim_i32(seg) && seg.numel() == 2 * T * cap &&
                  sim_i32(level) && level.numel() == 4 * T,
              "tree_grow: heap int32 [T, cap], seg int32 [T, cap, 2], level int32 [T, 4]");
  TORCH_CHECK(sim_i32(mult) && mult.dim() == 2 && mult.size(0) == T && mult.size(1) >= n && sim_i32(rows) &&
                  rows.numel() == 2 * mult.numel(), "tree_grow: mult int32 [T, ldr >= n], rows int32 [2, T, ldr]");
  TORCH_CHECK(sim_i32(lcounts) && lcounts.dim() == 3 && lcounts.size(0) == T && lcounts.size(1) >= 1 &&
                  lcounts.size(2) == K, "tree_grow: lcounts int32 [T, lvl_cap, K]");
  TORCH_CHECK(sim_i32(nbins) && nbins.numel() == F && max_bins >= 1 && max_bins <= fedtgan::TREE_MAX_BINS,
              "tree_grow: nbins int32 [F], max_bins <= TREE_MAX_BINS");
  TORCH_CHECK(max_depth >= 0 && max_depth <= fedtgan::TREE_MAX_DEPTH && min_leaf >= 1 && min_leaf < (int64_t)INT32_MAX &&
                  m_feat >= 1, "tree_grow: 0 <= max_depth <= TREE_MAX_DEPTH, min_leaf >= 1, m_feat >= 1");
  a.nbins = nbins.data_ptr<int>();
  a.mult = mult.data_ptr<int>();
  a.rows = rows.data_ptr<int>();
  a.feature = feature.data_ptr<int>();
  a.bin = bin.data_ptr<int>();
  a.left = left.data_ptr<int>();
  a.heap = heap.data_ptr<int>();
  a.counts = counts.data_ptr<int>();
  a.seg = seg.data_ptr<int>();
  a.level = level.data_ptr<int>();
  a.lcounts = lcounts.data_ptr<int>();
  a.ldr = mult.size(1);
  a.T = (int)T;
  a.cap = (int)cap;
  a.lvl_cap = (int)lcounts.size(1);
  a.max_depth = (int)max_depth;
  a.min_leaf = (int)min_leaf;
  a.m_feat = (int)(m_feat < F ? m_feat : F);
  a.hist_bytes = (int)((max_bins * K * 4 + 7) / 8 * 8);
  a.seed = (uint64_t)seed;
  fedtgan::launch_tree_grow(a, cur_stream());
}

void tree_predict(const Tensor& bins, const Tensor& y, const Tensor& tcounts, const Tensor& cw, int64_t n,
                  const Tensor& feature, const Tensor& bin, const Tensor& left, const Tensor& counts, bool soft,
                  const Tensor& conf) {
  fedtgan::TreePredictArgs a{};
  a.t = tree_table("tree_predict", bins, y, tcounts, cw, n);
  tree_check_nodes("tree_predict", feature, bin, left, counts, a.t.K);
  TORCH_CHECK(sim_i32(conf) && conf.numel() == (int64_t)a.t.K * a.t.K, "tree_predict: conf int32 [K, K]");
  TORCH_CHECK(soft || feature.size(0) == 1, "tree_predict: the hard vote is one tree's");
  a.feature = feature.data_ptr<int>();
  a.bin = bin.data_ptr<int>();
  a.left = left.data_ptr<int>();
  a.counts = counts.data_ptr<int>();
  a.T = (int)feature.size(0);
  a.cap = (int)feature.size(1);
  a.soft = soft ? 1 : 0;
  a.conf = conf.data_ptr<int>();
  fedtgan::launch_tree_predict(a, cur_stream());
}

void tree_scores(const Tensor& conf, const Tensor& real, const Tensor& out) {
  TORCH_CHECK(sim_i32(conf) && conf.dim() == 2 && conf.size(0) == conf.size(1) && conf.size(0) >= 1 &&
                  conf.size(0) <= fedtgan::TREE_MAX_CLASSES, "tree_scores: conf int32 [K, K]");
  TORCH_CHECK(sim_f64(real) && real.numel() >= 2 && sim_f64(out) && out.numel() >= 6,
              "tree_scores: real [2], out [6] float64");
  fedtgan::launch_tree_scores(conf.data_ptr<int>(), (int)conf.size(0), real.data_ptr<double>(), out.data_ptr<double>(),
                              cur_stream());
}

int64_t tree_max_bins() { return fedtgan::TREE_MAX_BINS; }
int64_t tree_max_classes() { return fedtgan::TREE_MAX_CLASSES; }
int64_t tree_max_depth() { return fedtgan::TREE_MAX_DEPTH; }
int64_t tree_max_features() { return fedtgan::TREE_MAX_FEATURES; }

// ----------------------------------------------------------------------------- native RCCL plane (csrc/comm)
void rccl_load_op(const std::string& path) { fedtgan::comm::rccl_load(path); }

Tensor rccl_unique_id_op() {
  const std::vector<uint8_t> v = fedtgan::comm::rccl_unique_id();
  Tensor t = at::empty({(int64_t)v.size()}, at::TensorOptions().dtype(at::kByte));
  std::memcpy(t.data_ptr(), v.data(), v.size());
  return t;
}

int64_t rccl_init_op(const Tensor& id, int64_t rank, int64_t nranks) {
  TORCH_CHECK(id.device().is_cpu() && id.scalar_type() == at::kByte && id.numel() == 128 && id.is_contiguous(),
              "rccl_init: id must be the 128-byte CPU uint8 tensor of rccl_unique_id()");
  return fedtgan::comm::rccl_init(id.data_ptr<uint8_t>(), (int)rank, (int)nranks);
}

// in place on the current HIP stream (capturable); premul: this rank's weight, folded into the collective
void rccl_all_reduce_op(int64_t comm, const Tensor& x, double premul) {
  TORCH_CHECK(x.is_cuda() && x.scalar_type() == at::kFloat && x.is_contiguous(),
              "rccl_all_reduce: x must be a contiguous fp32 device tensor");
  fedtgan::comm::rccl_all_reduce_f32(comm, x.data_ptr<float>(), (size_t)x.numel(), (float)premul, cur_stream());
}

void rccl_destroy_op(int64_t comm) { fedtgan::comm::rccl_destroy(comm); }

void write_csv(const std::string& path, const Tensor& values, std::vector<std::string> names, std::vector<int64_t> kinds,
               std::vector<std::string> vocab_flat, std::vector<int64_t> vocab_offsets, int64_t threads,
               std::vector<int64_t> src, std::vector<int64_t> date_desc, std::vector<int64_t> date_lut,
               const optional<Tensor>& aux) {
  // output column j: kinds[j], names[j], vocabulary vocab_flat[vocab_offsets[j], vocab_offsets[j + 1]), source
  // column src[j] of values (default j).  Date columns (kind 3) take their description from date_desc, in
  // output order: [mode, n_parts, (src, elem, lut_off, lut_len) x n_parts], code -> value tables in date_lut.
  TORCH_CHECK(!values.is_cuda() && values.scalar_type() == at::kDouble && values.is_contiguous() && values.dim() == 2,
              "write_csv: values must be a contiguous CPU float64 matrix");
  const int64_t cols = values.size(1);
  const int64_t n_out = (int64_t)kinds.size();
  const bool has_aux = aux.has_value() && aux->defined();
  if (has_aux)
    TORCH_CHECK(!aux->is_cuda() && aux->scalar_type() == at::kDouble && aux->is_contiguous() && aux->dim() == 2 &&
                    aux->size(0) == values.size(0), "write_csv: aux must be a contiguous CPU float64 [rows, n] matrix");
  const int64_t aux_cols = has_aux ? aux->size(1) : 0;
  TORCH_CHECK((int64_t)names.size() == n_out && (int64_t)vocab_offsets.size() == n_out + 1 &&
                  (src.empty() ? n_out == cols : (int64_t)src.size() == n_out),
              "write_csv: descriptors");
  std::vector<fedtgan::CsvColumn> out((size_t)n_out);
  size_t dp = 0;
  for (int64_t j = 0; j < n_out; ++j) {
    auto& c = out[(size_t)j];
    c.kind = (int)kinds[(size_t)j];
    TORCH_CHECK(c.kind >= fedtgan::CSV_FLOAT && c.kind <= fedtgan::CSV_DATE, "write_csv: kind");
    c.src = (int)(src.empty() ? j : src[(size_t)j]);
    TORCH_CHECK(vocab_offsets[(size_t)j] <= vocab_offsets[(size_t)j + 1] &&
                    vocab_offsets[(size_t)j + 1] <= (int64_t)vocab_flat.size(), "write_csv: vocab offsets");
    c.vocab.assign(vocab_flat.begin() + vocab_offsets[(size_t)j], vocab_flat.begin() + vocab_offsets[(size_t)j + 1]);
    if (c.kind != fedtgan::CSV_DATE) {
      TORCH_CHECK(c.src >= 0 && c.src < cols + aux_cols, "write_csv: source column out of range");
      continue;
    }
    TORCH_CHECK(dp + 2 <= date_desc.size(), "write_csv: date_desc too short");
    c.date_mode = (int)date_desc[dp++];
    const int64_t np = date_desc[dp++];
    TORCH_CHECK(np >= 1 && np <= 6 && dp + 4 * (size_t)np <= date_desc.size(), "write_csv: date parts");
    for (int64_t q = 0; q < np; ++q) {
      fedtgan::CsvDatePart part;
      part.src = (int)date_desc[dp++];
      part.elem = (int)date_desc[dp++];
      const int64_t off = date_desc[dp++], len = date_desc[dp++];
      TORCH_CHECK(part.src >= 0 && part.src < cols && part.elem >= 0 && part.elem <= 5 && off >= 0 && len >= 0 &&
                      off + len <= (int64_t)date_lut.size(), "write_csv: date part descriptor");
      part.lut.assign(date_lut.begin() + off, date_lut.begin() + off + len);
      c.parts.push_back(std::move(part));
    }
  }
  TORCH_CHECK(dp == date_desc.size(), "write_csv: unused date_desc entries");
  fedtgan::write_csv_columns(path, values.data_ptr<double>(), values.size(0), cols, names, out, (int)threads,
                             has_aux ? aux->data_ptr<double>() : nullptr, aux_cols);
}

void vgm_encode(const Tensor& x, const Tensor& out, const Tensor& opt, const Tensor& col_kind, const Tensor& col_pos,
                const Tensor& col_aux, const Tensor& col_span, const Tensor& col_lut_n, const Tensor& consts, const Tensor& means,
                const Tensor& prec, const Tensor& stds, const Tensor& vrank, const Tensor& lut, int64_t seed,
                int64_t stream) {
  // row-major, or column-major (a table uploaded as its [cols, rows] transpose: no device transposing copy)
  TORCH_CHECK(x.is_cuda() && x.scalar_type() == at::kDouble && x.dim() == 2 &&
                  (x.stride(1) == 1 || x.stride(0) == 1 || x.size(0) <= 1 || x.size(1) <= 1), "vgm_encode: x");
  check_f32_2d(out, "out");
  TORCH_CHECK(opt.is_cuda() && opt.scalar_type() == at::kInt && opt.is_contiguous() && opt.size(0) == x.size(0),
              "vgm_encode: opt");
  const int64_t n_cols = x.size(1);
  for (const Tensor* t : {&col_kind, &col_pos, &col_aux, &col_span, &col_lut_n})
    TORCH_CHECK(t->is_cuda() && t->scalar_type() == at::kInt && t->numel() == n_cols && t->is_contiguous(),
                "vgm_encode: column tables");
  for (const Tensor* t : {&consts, &means, &prec, &stds})
    TORCH_CHECK(t->is_cuda() && t->scalar_type() == at::kFloat && t->is_contiguous() && t->numel() == vrank.numel(),
                "vgm_encode: bank tables");
  TORCH_CHECK(vrank.scalar_type() == at::kInt && lut.scalar_type() == at::kInt && lut.is_contiguous(), "vgm_encode");
  fedtgan::VgmEncodeArgs a{};
  a.x = x.data_ptr<double>();
  a.ldx = (int)x.stride(0);
  a.ldc = x.stride(1);
  a.n_rows = (int)x.size(0);
  a.n_cols = (int)n_cols;
  a.out = fp(out);
  a.ldo = ld_of(out);
  a.opt = opt.data_ptr<int>();
  a.n_span = (int)opt.size(1);
  a.col_kind = col_kind.data_ptr<int>();
  a.col_pos = col_pos.data_ptr<int>();
  a.col_aux = col_aux.data_ptr<int>();
  a.col_span = col_span.data_ptr<int>();
  a.col_lut_n = col_lut_n.data_ptr<int>();
  a.consts = consts.data_ptr<float>();
  a.means = means.data_ptr<float>();
  a.prec = prec.data_ptr<float>();
  a.stds = stds.data_ptr<float>();
  a.vrank = vrank.data_ptr<int>();
  a.lut = lut.data_ptr<int>();
  a.seed = (uint64_t)seed;
  a.stream = (uint32_t)stream;
  fedtgan::launch_vgm_encode(a, cur_stream());
}

fedtgan::VgmFitArgs fit_args(const Tensor& x, const Tensor& n_rows, const Tensor& means, const Tensor& partial,
                             int64_t rows_per_block, int64_t nv) {
  TORCH_CHECK(x.is_cuda() && x.scalar_type() == at::kDouble && x.dim() == 2 && x.stride(1) == 1, "vgm fit: x");
  TORCH_CHECK(n_rows.is_cuda() && n_rows.scalar_type() == at::kInt && n_rows.numel() == x.size(0), "vgm fit: n_rows");
  TORCH_CHECK(means.scalar_type() == at::kDouble && means.is_contiguous() && means.numel() == x.size(0) * 10,
              "vgm fit: [n_cols, 10] tables");
  TORCH_CHECK(rows_per_block > 0, "vgm fit: rows_per_block");
  const int64_t chunks = (x.size(1) + rows_per_block - 1) / rows_per_block;
  TORCH_CHECK(partial.scalar_type() == at::kDouble && partial.is_contiguous() &&
                  partial.numel() == x.size(0) * chunks * nv, "vgm fit: partial must be [n_cols, chunks, ", nv, "]");
  fedtgan::VgmFitArgs a{};
  a.x = x.data_ptr<double>();
  a.ldx = (int)x.stride(0);
  a.n_cols = (int)x.size(0);
  a.max_rows = (int)x.size(1);
  a.rows_per_block = (int)rows_per_block;
  a.n_rows = n_rows.data_ptr<int>();
  a.means = means.data_ptr<double>();
  a.partial = partial.data_ptr<double>();
  return a;
}

void vgm_estep(const Tensor& x, const Tensor& n_rows, const Tensor& consts, const Tensor& means, const Tensor& prec,
               const Tensor& partial, int64_t rows_per_block) {
  auto a = fit_args(x, n_rows, means, partial, rows_per_block, 31);
  TORCH_CHECK(consts.scalar_type() == at::kDouble && consts.is_contiguous() && consts.numel() == means.numel() &&
                  prec.scalar_type() == at::kDouble && prec.is_contiguous() && prec.numel() == means.numel(),
              "vgm_estep: tables");
  a.consts = consts.data_ptr<double>();
  a.prec = prec.data_ptr<double>();
  fedtgan::launch_vgm_estep(a, cur_stream());
}

void kmeans_step(const Tensor& x, const Tensor& n_rows, const Tensor& centers, const Tensor& partial,
                 int64_t rows_per_block) {
  auto a = fit_args(x, n_rows, centers, partial, rows_per_block, 30);
  fedtgan::launch_kmeans_step(a, cur_stream());
}

void vgm_fit(const Tensor& x, const Tensor& n_rows, const c10::optional<Tensor>& init_centers, int64_t seed,
             double wprior, double tol, double reg_covar, int64_t max_iter, int64_t km_iter, const Tensor& out,
             const Tensor& info, const Tensor& lower_bound) {
  TORCH_CHECK(x.is_cuda() && x.scalar_type() == at::kDouble && x.dim() == 2 && x.stride(1) == 1, "vgm_fit: x");
  const int64_t nc = x.size(0);
  TORCH_CHECK(n_rows.is_cuda() && n_rows.scalar_type() == at::kInt && n_rows.is_contiguous() && n_rows.numel() == nc,
              "vgm_fit: n_rows");
  TORCH_CHECK(out.is_cuda() && out.scalar_type() == at::kDouble && out.is_contiguous() && out.numel() == nc * 60,
              "vgm_fit: out must be [n_cols, 6, 10] fp64");
  TORCH_CHECK(info.is_cuda() && info.scalar_type() == at::kInt && info.is_contiguous() && info.numel() == nc * 2,
              "vgm_fit: info");
  TORCH_CHECK(lower_bound.is_cuda() && lower_bound.scalar_type() == at::kDouble && lower_bound.numel() == nc,
              "vgm_fit: lower_bound");
  fedtgan::VgmFitAllArgs a{};
  a.x = x.data_ptr<double>();
  a.ldx = (int)x.stride(0);
  a.n_cols = (int)nc;
  a.n_rows = n_rows.data_ptr<int>();
  if (init_centers.has_value()) {
    TORCH_CHECK(init_centers->is_cuda() && init_centers->scalar_type() == at::kDouble &&
                    init_centers->is_contiguous() && init_centers->numel() == nc * 10,
                "vgm_fit: init_centers must be [n_cols, 10] fp64");
    a.init_centers = init_centers->data_ptr<double>();
  }
  a.seed = (uint64_t)seed;
  a.wprior = wprior;
  a.tol = tol;
  a.reg_covar = reg_covar;
  a.max_iter = (int)max_iter;
  a.km_iter = (int)km_iter;
  a.out = out.data_ptr<double>();
  a.info = info.data_ptr<int>();
  a.lower_bound = lower_bound.data_ptr<double>();
  // split fit: a cluster of workgroups per column (the record buffer and the zeroed arrival counters live
  // until the launch has run: stream-ordered caching-allocator blocks)
  a.split = fedtgan::vgm_fit_split((int)nc, (int)x.size(1));
  Tensor xpart, sync;
  if (a.split > 1) {
    xpart = at::empty({nc * 2 * a.split * 32}, x.options());
    sync = at::zeros({nc * 32}, x.options().dtype(at::kInt));
    a.xpart = xpart.data_ptr<double>();
    a.sync = reinterpret_cast<unsigned*>(sync.data_ptr<int>());
  }
  fedtgan::launch_vgm_fit(a, cur_stream());
}

// checked build: the check bits raised by every kernel since the last call (cleared); synchronises
int64_t check_status() {
  (void)hipDeviceSynchronize();
  return (int64_t)(fedtgan::check_status_gemm() | fedtgan::check_status_ctgan_ops() | fedtgan::check_status_vgm() |
                   fedtgan::check_status_cond_gen() | fedtgan::check_status_cond_pred() |
                   fedtgan::check_status_known_gen() |
                   fedtgan::check_status_similarity() |
                   fedtgan::check_status_forest());
}

#ifdef FEDTGAN_CHECKED
bool is_checked() { return true; }
#else
bool is_checked() { return false; }
#endif

std::string py_float(double x) { return fedtgan::format_py_float(x); }

// kernel variant knobs for measured sweeps (tools/microbench.py); returns the previous value
int64_t set_tuning(const std::string& key, int64_t value) {
  if (key == "colown_dbg") {   // phase-cost probe of linear_bn_relu_colown (results are wrong while set)
    TORCH_CHECK(value >= 0 && value <= 7, "colown_dbg: bit mask 0..7");
    const int64_t prev = fedtgan::g_colown_dbg;
    fedtgan::g_colown_dbg = (int)value;
    return prev;
  }
  if (key == "bn_cols") {
    TORCH_CHECK(value == 4 || value == 8 || value == 16, "bn_cols must be 4, 8 or 16");
    const int64_t prev = fedtgan::g_bn_cols;
    fedtgan::g_bn_cols = (int)value;
    return prev;
  }
  if (key == "decode_rows") {
    TORCH_CHECK(value >= 0 && value <= 2, "decode_rows: 0 per cell, 1 per row, 2 per row over Philox quads");
    const int prev = fedtgan::g_decode_rows;
    fedtgan::g_decode_rows = (int)value;
    return prev;
  }
  if (key == "chain_pre") {   // chained tail weights prefetched: 0 never, 1 grids of <= 512 workgroups, 2 always
    TORCH_CHECK(value >= 0 && value <= 2, "chain_pre: 0, 1 or 2");
    const int prev = fedtgan::g_chain_pre;
    fedtgan::g_chain_pre = (int)value;
    return prev;
  }
  if (key == "chain_rows") {  // head rows per chain workgroup when the one-row grid is too large to prefetch
    TORCH_CHECK(value == 1 || value == 2, "chain_rows: 1 or 2");
    const int prev = fedtgan::g_chain_rows;
    fedtgan::g_chain_rows = (int)value;
    return prev;
  }
  if (key == "chain_coalesced") {   // chained tail GEMM: lane-contiguous weight rows + wave sums (1)
    const int prev = fedtgan::g_chain_coalesced;
    fedtgan::g_chain_coalesced = value ? 1 : 0;
    return prev;
  }
  if (key == "gp_threads") {
    TORCH_CHECK(value == 256 || value == 1024, "gp_threads: 256 or 1024");
    const int prev = fedtgan::g_gp_threads;
    fedtgan::g_gp_threads = (int)value;
    return prev;
  }
  if (key == "bn_threads") {
    TORCH_CHECK(value == 512 || value == 1024, "bn_threads: 512 or 1024");
    const int prev = fedtgan::g_bn_threads;
    fedtgan::g_bn_threads = (int)value;
    return prev;
  }
  if (key == "bn_slices") {   // paired training BN: 1 one workgroup per column block, 2 / 4 row-storing workgroups per batch
    TORCH_CHECK(value == 1 || value == 2 || value == 4, "bn_slices: 1, 2 or 4");
    const int prev = fedtgan::g_bn_slices;
    fedtgan::g_bn_slices = (int)value;
    return prev;
  }
  if (key == "act_rowreg_narrow") {   // rows <= 512 wide: per-wave kernels (0), row kernels 2-4 waves (1), a block per wave (2)
    TORCH_CHECK(value >= 0 && value <= 2, "act_rowreg_narrow: 0, 1 or 2");
    const int prev = fedtgan::g_act_rowreg_narrow;
    fedtgan::g_act_rowreg_narrow = (int)value;
    return prev;
  }
  if (key == "gp_split") {   // gradient-penalty scale of rows wider than 8,192: chunk-split (1) or one workgroup per row (0)
    const int prev = fedtgan::g_gp_split;
    fedtgan::g_gp_split = value ? 1 : 0;
    return prev;
  }
  if (key == "act_row_mode") {
    TORCH_CHECK(value >= 0 && value <= 2, "act_row_mode: 0 per-wave, 1 row (LDS image), 2 row (registers; forward)");
    const int prev = fedtgan::g_act_row_mode;
    fedtgan::g_act_row_mode = (int)value;
    return prev;
  }
  if (key == "xcd_clients") {   // batched launches: each client on its own XCD(s) (1) or round-robin (0)
    TORCH_CHECK(value == 0 || value == 1, "xcd_clients: 0 or 1");
    const int64_t prev = fedtgan::g_xcd_clients;
    fedtgan::g_xcd_clients = (int)value;
    return prev;
  }
  if (key == "adam_store") {
    TORCH_CHECK(value == 0 || value == 2 || value == 16, "adam_store: 0 plain, 2 nt, 16 sc1");
    const int64_t prev = fedtgan::g_adam_store;
    fedtgan::g_adam_store = (int)value;
    return prev;
  }
  if (key == "adam_u_min") {   // float4 count (x clients) from which the Adam loop loads ADAM_U float4 per thread
    TORCH_CHECK(value >= 0, "adam_u_min: >= 0");
    const int64_t prev = fedtgan::g_adam_u_min;
    fedtgan::g_adam_u_min = value;
    return prev;
  }
  if (key == "bnb_first") {   // gemm_bnbwd_kernel: BN workgroups first (1) or last (0)
    const int64_t prev = fedtgan::g_bnb_first;
    fedtgan::g_bnb_first = value ? 1 : 0;
    return prev;
  }
  if (key == "bnb_cols") {    // gemm_bnbwd_kernel: columns per BN workgroup, 4 or 8
    TORCH_CHECK(value == 4 || value == 8, "bnb_cols: 4 or 8");
    const int64_t prev = fedtgan::g_bnb_cols;
    fedtgan::g_bnb_cols = (int)value;
    return prev;
  }
  if (key == "vgm_split") {   // workgroups per column of the whole-fit VGM kernel: 0 auto, 1 one, n n
    TORCH_CHECK(value >= 0 && value <= 64, "vgm_split: 0..64");
    const int64_t prev = fedtgan::g_vgm_split;
    fedtgan::g_vgm_split = (int)value;
    return prev;
  }
  if (key == "vgm_split_of") {   // read-only probe: the split a fit of `value` columns x 40000 rows would use
    return fedtgan::vgm_fit_split((int)value, 40000);
  }
  if (key == "corr_part_target") {   // fp64 partials corr_moments' row groups may fill (kernels/launch.h); 0 = default
    TORCH_CHECK(value >= 0, "corr_part_target: >= 0");
    const int64_t prev = fedtgan::g_corr_part_target;
    fedtgan::g_corr_part_target = value ? value : fedtgan::CORR_PART_TARGET;
    return prev;
  }
  if (key == "adam_max_blocks") {
    TORCH_CHECK(value >= 1 && value <= 65535, "adam_max_blocks: 1..65535");
    const int64_t prev = fedtgan::g_adam_max_blocks;
    fedtgan::g_adam_max_blocks = (int)value;
    return prev;
  }
  if (key == "gemm_store_wt") {
    const int64_t prev = fedtgan::g_gemm_store_wt;
    fedtgan::g_gemm_store_wt = value ? 1 : 0;
    return prev;
  }
  if (key == "gemm_shortk") {
    const int64_t prev = fedtgan::g_gemm_shortk;
    fedtgan::g_gemm_shortk = value ? 1 : 0;
    return prev;
  }
  if (key == "gemm_shortk_store") {
    TORCH_CHECK(value >= 0 && value <= 2, "gemm_shortk_store: 0 plain, 1 non-temporal, 2 write-through");
    const int64_t prev = fedtgan::g_gemm_shortk_store;
    fedtgan::g_gemm_shortk_store = (int)value;
    return prev;
  }
  if (key == "gemm_shortk_min_n") {
    TORCH_CHECK(value >= 4, "gemm_shortk_min_n: >= 4");
    const int64_t prev = fedtgan::g_gemm_shortk_min_n;
    fedtgan::g_gemm_shortk_min_n = (int)value;
    return prev;
  }
  if (key == "gemm_splitk_inlaunch") {
    const int64_t prev = fedtgan::g_gemm_splitk_inlaunch;
    fedtgan::g_gemm_splitk_inlaunch = value ? 1 : 0;
    return prev;
  }
  if (key == "gemm_pairs") {
    const int64_t prev = fedtgan::g_gemm_pairs;
    fedtgan::g_gemm_pairs = value ? 1 : 0;
    return prev;
  }
  if (key == "gemm_pair_max_wg") {   // pairs with more workgroups than this launch as two GEMMs (0: no limit)
    TORCH_CHECK(value >= 0, "gemm_pair_max_wg: >= 0");
    const int64_t prev = fedtgan::g_gemm_pair_max_wg;
    fedtgan::g_gemm_pair_max_wg = (int)value;
    return prev;
  }
  if (key == "gemm_xcd_nmajor") {
    const int64_t prev = fedtgan::g_gemm_xcd_nmajor;
    fedtgan::g_gemm_xcd_nmajor = value ? 1 : 0;
    return prev;
  }
  if (key == "gemm_xcd_remap") {
    const int64_t prev = fedtgan::g_gemm_xcd_remap;
    TORCH_CHECK(value >= 0 && value <= 2, "gemm_xcd_remap: 0 off, 1 long-K tiles, 2 always");
    fedtgan::g_gemm_xcd_remap = (int)value;
    return prev;
  }
  TORCH_CHECK(false, "unknown tuning key ", key);
}

}  // namespace

TORCH_LIBRARY(fedtgan, m) {
  m.def("gen_weight_prep(Tensor[] w, int[] kd, Tensor(a!)[] w16, Tensor(b!)[] wt) -> ()");
  m.def(
      "gemm(Tensor a, Tensor b, Tensor(a!) c, bool ta, bool tb, float alpha, float beta, Tensor? bias, int epi, "
      "Tensor(b!)? ms, float slope, float p_drop, Tensor(d!)? ws, int splitk, int seed, Tensor? rng_ctr, int stream, "
      "Tensor? bn_gamma, Tensor? bn_beta, Tensor? bn_rm, Tensor? bn_rv, float bn_eps, bool f32, Tensor? head_coef, "
      "Tensor? head_v, Tensor(e!)? head_a, int tile, int group=0, Tensor? oh_w=None, Tensor? oh_col=None, "
      "Tensor? oh_opt=None, Tensor? oh_off=None, bool oh_trans=False, Tensor(f!)? bn_part=None, int bn_rpg=0, "
      "Tensor(g!)? tile_cnt=None, bool chain=False) -> ()");
  m.def(
      "sample(Tensor(a!) h, int zc, int cc, int E, Tensor(b!)? xf, Tensor(c!)? xr, int Dd, Tensor cdf, Tensor cond_off, "
      "Tensor cond_w, Tensor? row_off, Tensor? row_cnt, Tensor? rows, Tensor? data, Tensor(d!)? col, Tensor(e!)? opt, "
      "Tensor(f!)? step_bump, Tensor(h!)? step_bump2, Tensor(g!)? metrics, bool zero_metrics, int seed, Tensor rng_ctr, "
      "int stream, int draws=1, int draw_h=0, int draw_x=0, int draw_col=0) -> ()");
  m.def(
      "activate(Tensor logits, Tensor(a!) out, Tensor start, Tensor width, Tensor kind, Tensor cidx, Tensor elem, "
      "float tau, int seed, Tensor rng_ctr, int stream, Tensor? slerp_real, Tensor(b!)? slerp_out, int slerp_cols, "
      "int slerp_stream) -> ()");
  m.def(
      "act_bwd_ce(Tensor dact, Tensor act, Tensor logits, Tensor start, Tensor width, Tensor kind, Tensor cidx, "
      "Tensor elem, Tensor col, Tensor opt, Tensor(a!) dlogits, Tensor(b!) loss, float tau) -> ()");
  m.def("slerp(Tensor real, Tensor fake, Tensor(a!) out, int seed, Tensor rng_ctr, int stream) -> ()");
  m.def("gp_scale(Tensor g, Tensor(a!) out, float lam, Tensor(b!) loss, Tensor(c!)? ws=None) -> ()");
  m.def("onehot_wgrad(Tensor[] dy, Tensor(a!)[] w, Tensor col, Tensor opt, Tensor cond_off, int zero) -> ()");
  m.def(
      "d_head(Tensor d, Tensor ms, Tensor v, Tensor e, Tensor coef, Tensor wloss, Tensor(a!) y, Tensor(b!) a, "
      "Tensor(c!) loss) -> ()");
  m.def("colsum(Tensor[] srcs, Tensor(a!)[] outs) -> ()");
  m.def(
      "colsum_ex(Tensor[] srcs, Tensor?[] outs, Tensor?[] w, Tensor?[] dot_v, Tensor?[] dot_e, Tensor?[] dot_out, "
      "Tensor?[] dot_w) -> ()");
  m.def(
      "linear_bn_relu_colown(Tensor x, Tensor w, Tensor? bias, Tensor gamma, Tensor beta, Tensor(a!) out, "
      "Tensor(b!) nhat, Tensor(c!) mean, Tensor(d!) invstd, Tensor(e!) rm, Tensor(f!) rv, float momentum, float eps, "
      "int groups, Tensor? oh_w, Tensor? oh_col, Tensor? oh_opt, Tensor? oh_off, bool oh_trans, Tensor(g!) stat, "
      "Tensor(h!) cnt) -> ()");
  m.def(
      "bn_relu_train(Tensor a, Tensor gamma, Tensor beta, Tensor(a!) out, Tensor(b!) nhat, Tensor(c!) mean, "
      "Tensor(d!) invstd, Tensor(e!) rm, Tensor(f!) rv, float momentum, float eps, int groups) -> ()");
  m.def(
      "bn_relu_apply(Tensor a, Tensor part, int n_tiles, Tensor gamma, Tensor beta, Tensor(a!) out, Tensor(b!) nhat, "
      "Tensor(c!) mean, Tensor(d!) invstd, Tensor(e!) rm, Tensor(f!) rv, float momentum, float eps, int groups) -> ()");
  m.def(
      "bn_relu_bwd(Tensor dr, Tensor r, Tensor nhat, Tensor gamma, Tensor invstd, Tensor(a!) da, Tensor(b!) dgamma, "
      "Tensor(c!) dbeta, Tensor(d!)? dbias, bool paired=False) -> ()");
  m.def(
      "adam(Tensor(a!) p, Tensor g, Tensor(b!) m, Tensor(c!) v, Tensor step, float lr, float b1, float b2, float eps, "
      "float wd, Tensor(d!)? rng_bump) -> ()");
  m.def(
      "adam_cs(Tensor(a!) p, Tensor(e!) g, Tensor(b!) m, Tensor(c!) v, Tensor step, float lr, float b1, float b2, "
      "float eps, float wd, Tensor(d!)? rng_bump, Tensor[] srcs, Tensor?[] outs, Tensor?[] w, Tensor?[] dot_v, "
      "Tensor?[] dot_e, Tensor?[] dot_out, Tensor?[] dot_w) -> ()");
  m.def(
      "sample_decode(Tensor logits, Tensor(a!) out, Tensor kind, Tensor start, Tensor width, Tensor cont, "
      "Tensor code_off, Tensor codes, Tensor mu, Tensor sd, int seed, Tensor rng_ctr, int stream, "
      "Tensor? ecol=None, Tensor? quads=None) -> ()");
  m.def("rng_bump(Tensor(a!) ctr) -> ()");
  m.def(
      "cond_request(Tensor drive, Tensor bin_opt, Tensor bin_code, Tensor quota, Tensor filled, Tensor seg_off, "
      "Tensor fixed_j, Tensor fixed_code, Tensor stats, Tensor(a!) col, Tensor(b!) opt, Tensor(c!) tgt, Tensor(d!)? h, "
      "int cc, Tensor cond_off, Tensor cond_w, int seed, Tensor rng_ctr, int stream) -> ()");
  m.def(
      "cond_partition(Tensor drive, Tensor bin_opt, Tensor bin_code, Tensor quota, Tensor(a!) filled, Tensor seg_off, "
      "Tensor fixed_j, Tensor fixed_code, Tensor(b!) stats, Tensor out, Tensor tgt, Tensor(c!) dst, Tensor(d!) keep, "
      "Tensor(e!) counts, bool any_value=False) -> ()");
  m.def("cond_partition_workgroups(int rows) -> int", &cond_partition_workgroups);
  m.def(
      "pred_request(Tensor drv, Tensor drv_opt, Tensor drv_cum, Tensor quota, Tensor filled, Tensor(a!) col, "
      "Tensor(b!) opt, Tensor(c!) tgt, Tensor(d!)? h, int cc, Tensor cond_off, Tensor cond_w, int seed, "
      "Tensor rng_ctr, int stream) -> ()");
  m.def(
      "pred_mark(Tensor pred_j, Tensor pred_kind, Tensor pred_lo, Tensor pred_hi, Tensor pred_lut_off, "
      "Tensor pred_lut_len, Tensor pred_lut, Tensor(a!) pred_stats, Tensor out, Tensor(b!) tgt) -> ()");
  m.def(
      "known_request(Tensor qidx, Tensor drv_span, Tensor drv_opt, int tries, Tensor(a!) col, Tensor(b!) opt, "
      "Tensor(c!)? h, int cc, Tensor cond_off, Tensor cond_w) -> ()");
  m.def(
      "known_match(Tensor known, Tensor mask, Tensor qidx, int tries, Tensor cand, Tensor kind, Tensor scale, "
      "Tensor(a!) best, Tensor(b!) dc, Tensor(c!) miss, Tensor(d!) seen, Tensor(e!) pick, Tensor(f!) dst) -> ()");
  m.def(
      "sim_prepare(Tensor values, Tensor kind, Tensor slot, Tensor vocab, Tensor(a!) keys, Tensor(b!) valid, "
      "Tensor(c!) counts) -> ()");
  m.def("sim_sort(Tensor(a!) keys, Tensor(b!) tmp, int n) -> ()");
  m.def(
      "sim_w1(Tensor real, Tensor n_real, Tensor fake, Tensor n_fake, int max_fake, Tensor(a!) part, "
      "Tensor(b!) out) -> ()");
  m.def("sim_jsd(Tensor real, Tensor fake, Tensor(a!) out) -> ()");
  m.def("sim_mean(Tensor(a!) scores, int n_cat, int n_cont) -> ()");
  m.def("sim_sort_tile() -> int", &sim_sort_tile);
  m.def("sim_w1_chunks(int n) -> int", &sim_w1_chunks);
  m.def(
      "nn_pack(Tensor values, Tensor kind, Tensor slot, Tensor lo, Tensor scale, Tensor(a!) cont, Tensor(b!) cat) -> ()");
  m.def(
      "nn_top2(Tensor q_cont, Tensor q_cat, Tensor r_cont, Tensor r_cat, bool exclude_self, Tensor(a!) d1, "
      "Tensor(b!) d2, Tensor(c!) i1, Tensor(d!) scratch) -> ()");
  m.def(
      "nn_within(Tensor q_cont, Tensor q_cat, Tensor r_cont, Tensor r_cat, Tensor t2, Tensor(a!) near, "
      "Tensor(b!) scratch) -> ()");
  m.def("guard_mark(Tensor near, Tensor(a!) tgt, Tensor(b!) stats) -> ()");
  m.def(
      "nn_merge_shards(Tensor parts, Tensor offsets, Tensor(a!) d1, Tensor(b!) d2, Tensor(c!) i1, Tensor(d!) owner, "
      "Tensor(e!) by_client) -> ()");
  m.def("nn_within_merge_shards(Tensor near, Tensor offsets, Tensor(a!) near_out, Tensor(b!) owner) -> ()");
  m.def("nn_stats(Tensor d1, Tensor d2, int n, Tensor(a!) keys, Tensor(b!) part) -> ()");
  m.def("nn_percentiles(Tensor keys, int n, Tensor part, Tensor(a!) out) -> ()");
  m.def("nn_query_tile() -> int", &nn_query_tile);
  m.def("nn_ref_tile() -> int", &nn_ref_tile);
  m.def("nn_chunk_rows() -> int", &nn_chunk_rows);
  m.def("nn_chunks(int nr) -> int", &nn_chunks);
  m.def("nn_scratch(int nq, int nr) -> int", &nn_scratch);
  m.def("nn_stats_part(int n) -> int", &nn_stats_part);
  m.def(
      "nn_topk(Tensor q_cont, Tensor q_cat, Tensor r_cont, Tensor r_cat, bool exclude_self, int k, Tensor(a!) out, "
      "Tensor(b!) scratch) -> ()");
  m.def(
      "nn_ball(Tensor q_cont, Tensor q_cat, Tensor r_cont, Tensor r_cat, Tensor r_rad2, Tensor(a!) cnt, "
      "Tensor(b!) dmin, Tensor(c!) scratch) -> ()");
  m.def(
      "prdc_reduce(Tensor cnt_a, Tensor cnt_b, Tensor dmin_b, Tensor rr, int n, int m, int k, Tensor(a!) scores) "
      "-> ()");
  m.def("fid_max_k() -> int", &fid_max_k);
  m.def("nn_topk_scratch(int nq, int nr, int k) -> int", &nn_topk_scratch);
  m.def("nn_ball_scratch(int nq, int nr) -> int", &nn_ball_scratch);
  m.def(
      "corr_pack(Tensor values, Tensor kind, Tensor slot, Tensor card, Tensor(a!) cont, Tensor(b!) cat_t, "
      "Tensor(c!) mean, Tensor(d!) part) -> ()");
  m.def(
      "corr_moments(Tensor cont, Tensor cat_t, int n, Tensor mean, Tensor card, Tensor offs, Tensor(a!) G, "
      "Tensor(b!) part) -> ()");
  m.def("corr_counts(Tensor cat_t, int n, Tensor pairs, Tensor poff, Tensor(a!) counts, int lds_bins) -> ()");
  m.def(
      "corr_matrix(Tensor G, Tensor counts, Tensor poff, Tensor kind, Tensor slot, Tensor card, Tensor offs, int n, "
      "Tensor(a!) A) -> ()");
  m.def("corr_diff(Tensor A, Tensor B, Tensor(a!) out) -> ()");
  m.def("corr_chunk() -> int", &corr_chunk);
  m.def("corr_lds_bins() -> int", &corr_lds_bins);
  m.def("corr_part(int n_max, int W, int n_cont) -> int", &corr_part);
  m.def("corr_groups(int n, int W, int n_cont) -> int", &corr_groups);
  m.def(
      "util_pack(Tensor values, Tensor kind, Tensor slot, Tensor card, Tensor offs, Tensor mean, Tensor sd, int D, "
      "Tensor(a!) cont, Tensor(b!) cat_t, Tensor(c!) y, Tensor(d!) s, Tensor(e!) counts, Tensor(f!) info) -> ()");
  m.def("util_gram(Tensor cont, Tensor cat_t, Tensor y, Tensor s, Tensor counts, Tensor info, Tensor card, Tensor offs, int n, Tensor(a!) M, Tensor(b!) part) -> ()");
  m.def("util_factor(Tensor M, Tensor(a!) Lt, Tensor(b!) X, Tensor(c!) Minv) -> ()");
  m.def("util_grad(Tensor cont, Tensor cat_t, Tensor y, Tensor s, Tensor counts, Tensor info, Tensor card, Tensor offs, int n, Tensor P, Tensor(a!) G, Tensor(b!) loss, Tensor(c!) part, Tensor(d!) lossp) -> ()");
  m.def(
      "util_step(Tensor cont, Tensor cat_t, Tensor y, Tensor s, Tensor counts, Tensor info, Tensor card, Tensor offs, int n, Tensor(a!) V, Tensor(b!) W, Tensor Minv, Tensor(c!) G, Tensor(d!) loss, Tensor(e!) part, "
      "Tensor(f!) lossp, float beta) -> ()");
  m.def(
      "util_predict(Tensor cont, Tensor cat_t, Tensor y, Tensor s, Tensor counts, Tensor info, Tensor card, Tensor offs, int n, Tensor train_counts, Tensor W, Tensor(a!) conf, Tensor G, Tensor loss, Tensor real, "
      "Tensor(b!) out) -> ()");
  m.def("util_max_features() -> int", &util_max_features);
  m.def("util_max_classes() -> int", &util_max_classes);
  m.def("util_chunk() -> int", &util_chunk);
  m.def("util_part(int n_max, int D, int K) -> int", &util_part);
  m.def("util_groups(int n, int cells) -> int", &util_groups);
  m.def(
      "mlp_step(Tensor cont, Tensor cat_t, Tensor y, Tensor s, Tensor counts, Tensor info, Tensor card, Tensor offs, int n, int D, int b, int nb, Tensor(a!) theta, Tensor(b!) m, Tensor(c!) v, Tensor(d!) h, Tensor(e!) dz, "
      "Tensor(f!) dh, Tensor(g!) cnt, int H, float alpha, float lr_t) -> ()");
  m.def("mlp_loss(Tensor cont, Tensor cat_t, Tensor y, Tensor s, Tensor counts, Tensor info, Tensor card, Tensor offs, int n, int D, Tensor theta, int H, float alpha, Tensor(a!) loss) -> ()");
  m.def(
      "mlp_predict(Tensor cont, Tensor cat_t, Tensor y, Tensor s, Tensor counts, Tensor info, Tensor card, Tensor offs, int n, int D, Tensor train_counts, Tensor theta, int H, Tensor(a!) conf, Tensor loss, Tensor real, "
      "Tensor(b!) out) -> ()");
  m.def("mlp_max_hidden() -> int", &mlp_max_hidden);
  m.def("mlp_max_batch() -> int", &mlp_max_batch);
  m.def("mlp_max_steps() -> int", &mlp_max_steps);
  m.def("mlp_rows() -> int", &mlp_rows);
  m.def("tree_pack(Tensor values, Tensor kind, Tensor slot, Tensor card, Tensor edges, Tensor eoff, Tensor(a!) bins, Tensor(b!) y, Tensor(c!) counts, Tensor(d!) cw) -> ()");
  m.def("tree_bootstrap(Tensor(a!) mult, int n, bool bootstrap, int seed) -> ()");
  m.def(
      "tree_grow(Tensor bins, Tensor y, Tensor tcounts, Tensor cw, Tensor nbins, int max_bins, int n, Tensor mult, Tensor(a!) rows, Tensor(b!) feature, Tensor(c!) bin, Tensor(d!) left, Tensor(e!) heap, Tensor(f!) counts, "
      "Tensor(g!) seg, Tensor(h!) level, Tensor(i!) lcounts, int max_depth, int min_leaf, int m_feat, int seed) -> ()");
  m.def("tree_predict(Tensor bins, Tensor y, Tensor tcounts, Tensor cw, int n, Tensor feature, Tensor bin, Tensor left, Tensor counts, bool soft, Tensor(a!) conf) -> ()");
  m.def("tree_scores(Tensor conf, Tensor real, Tensor(a!) out) -> ()");
  m.def("tree_max_bins() -> int", &tree_max_bins);
  m.def("tree_max_classes() -> int", &tree_max_classes);
  m.def("tree_max_depth() -> int", &tree_max_depth);
  m.def("tree_max_features() -> int", &tree_max_features);
  m.def(
      "vgm_estep(Tensor x, Tensor n_rows, Tensor consts, Tensor means, Tensor prec, Tensor(a!) partial, "
      "int rows_per_block) -> ()");
  m.def("kmeans_step(Tensor x, Tensor n_rows, Tensor centers, Tensor(a!) partial, int rows_per_block) -> ()");
  m.def(
      "vgm_fit(Tensor x, Tensor n_rows, Tensor? init_centers, int seed, float wprior, float tol, float reg_covar, "
      "int max_iter, int km_iter, Tensor(a!) out, Tensor(b!) info, Tensor(c!) lower_bound) -> ()");
  m.def(
      "vgm_encode(Tensor x, Tensor(a!) out, Tensor(b!) opt, Tensor col_kind, Tensor col_pos, Tensor col_aux, "
      "Tensor col_span, Tensor col_lut_n, Tensor consts, Tensor means, Tensor prec, Tensor stds, Tensor vrank, Tensor lut, int seed, "
      "int stream) -> ()");
  m.def(
      "write_csv(str path, Tensor values, str[] names, int[] kinds, str[] vocab_flat, int[] vocab_offsets, "
      "int threads, int[] src=[], int[] date_desc=[], int[] date_lut=[], Tensor? aux=None) -> ()");
  m.def("py_float(float x) -> str", &py_float);
  m.def("rccl_load(str path) -> ()", &rccl_load_op);
  m.def("rccl_unique_id() -> Tensor", &rccl_unique_id_op);
  m.def("rccl_init(Tensor id, int rank, int nranks) -> int", &rccl_init_op);
  m.def("rccl_all_reduce(int comm, Tensor(a!) x, float premul) -> ()", &rccl_all_reduce_op);
  m.def("rccl_destroy(int comm) -> ()", &rccl_destroy_op);
  m.def("set_tuning(str key, int value) -> int", &set_tuning);
  m.def("reset_held() -> int", &reset_held);
  m.def("device_reset() -> int", &device_reset);
  m.def("pool_sample(Tensor(a!) pool, Tensor seg_off, Tensor mean, Tensor sd, int seed) -> ()");
  m.def("row_center(Tensor(a!) x, Tensor(b!) shift) -> ()");
  m.def("csr_rows(Tensor opt, Tensor width, int maxw, Tensor(a!) part, Tensor(b!) count, Tensor(c!) offset, "
        "Tensor(d!) rows, int chunk) -> ()");
  m.def("gemm_achain_next(Tensor out, Tensor ws, Tensor cnt) -> ()", &gemm_achain_next);
  m.def("set_client_batch(int k, int stride, int seed_step, int base) -> int", &set_client_batch);
  m.def("check_status() -> int", &check_status);
  m.def("is_checked() -> bool", &is_checked);
}

TORCH_LIBRARY_IMPL(fedtgan, CUDA, m) {
  m.impl("gemm", &gemm);
  m.impl("gen_weight_prep", &gen_weight_prep);
  m.impl("sample", &sample);
  m.impl("activate", &activate);
  m.impl("act_bwd_ce", &act_bwd_ce);
  m.impl("slerp", &slerp);
  m.impl("gp_scale", &gp_scale);
  m.impl("onehot_wgrad", &onehot_wgrad);
  m.impl("d_head", &d_head);
  m.impl("colsum", &colsum);
  m.impl("colsum_ex", &colsum_ex);
  m.impl("bn_relu_train", &bn_relu_train);
  m.impl("bn_relu_bwd", &bn_relu_bwd);
  m.impl("bn_relu_apply", &bn_relu_apply);
  m.impl("linear_bn_relu_colown", &linear_bn_relu_colown);
  m.impl("adam", &adam);
  m.impl("adam_cs", &adam_cs);
  m.impl("sample_decode", &sample_decode);
  m.impl("rng_bump", &rng_bump);
  m.impl("known_request", &known_request);
  m.impl("known_match", &known_match);
  m.impl("cond_request", &cond_request);
  m.impl("cond_partition", &cond_partition);
  m.impl("pred_request", &pred_request);
  m.impl("pred_mark", &pred_mark);
  m.impl("sim_prepare", &sim_prepare);
  m.impl("sim_sort", &sim_sort);
  m.impl("sim_w1", &sim_w1);
  m.impl("sim_jsd", &sim_jsd);
  m.impl("sim_mean", &sim_mean);
  m.impl("nn_pack", &nn_pack);
  m.impl("nn_top2", &nn_top2);
  m.impl("nn_within", &nn_within);
  m.impl("guard_mark", &guard_mark);
  m.impl("nn_merge_shards", &nn_merge_shards);
  m.impl("nn_within_merge_shards", &nn_within_merge_shards);
  m.impl("nn_stats", &nn_stats);
  m.impl("nn_percentiles", &nn_percentiles);
  m.impl("nn_topk", &nn_topk);
  m.impl("nn_ball", &nn_ball);
  m.impl("prdc_reduce", &prdc_reduce);
  m.impl("corr_pack", &corr_pack);
  m.impl("corr_moments", &corr_moments);
  m.impl("corr_counts", &corr_counts);
  m.impl("corr_matrix", &corr_matrix);
  m.impl("corr_diff", &corr_diff);
  m.impl("util_pack", &util_pack);
  m.impl("util_gram", &util_gram);
  m.impl("util_factor", &util_factor);
  m.impl("util_grad", &util_grad);
  m.impl("util_step", &util_step);
  m.impl("util_predict", &util_predict);
  m.impl("mlp_step", &mlp_step);
  m.impl("mlp_loss", &mlp_loss);
  m.impl("mlp_predict", &mlp_predict);
  m.impl("tree_pack", &tree_pack);
  m.impl("tree_bootstrap", &tree_bootstrap);
  m.impl("tree_grow", &tree_grow);
  m.impl("tree_predict", &tree_predict);
  m.impl("tree_scores", &tree_scores);
  m.impl("vgm_encode", &vgm_encode);
  m.impl("vgm_estep", &vgm_estep);
  m.impl("kmeans_step", &kmeans_step);
  m.impl("vgm_fit", &vgm_fit);
  m.impl("pool_sample", &pool_sample);
  m.impl("row_center", &row_center);
  m.impl("csr_rows", &csr_rows);
}

TORCH_LIBRARY_IMPL(fedtgan, CPU, m) { m.impl("write_csv", &write_csv); }
