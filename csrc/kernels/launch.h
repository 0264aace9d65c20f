// Host-side launch interface of the fed_tgan_amd HIP kernels (raw pointers + hipStream_t).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace fedtgan {

enum Epilogue : int { EPI_NONE = 0, EPI_LRELU_DROPOUT = 1, EPI_MASK = 2, EPI_RELU = 3, EPI_BN_EVAL_RELU = 4 };

struct RngArgs;

// Batched clients (fed_tgan_amd/models/batched.py): K federated clients' training steps in ONE launch
// per kernel.  Every buffer a kernel touches lives in one device arena, client c's copy exactly `stride`
// bytes after client c-1's (identical layouts), so client c = blockIdx.z (the GEMM folds it with its
// split-K index) offsets every pointer by c * stride and its Philox seed by c * seed_step.  k = 1 (the
// default) is the plain single-client launch.  The host context is per thread (set by the bindings
// around a batched engine's launches); in a batched launch every pointer must lie in client 0's slab
// [base, base + stride), which the launchers verify (check_slab).
struct ClientBatch {
  int k;
  int64_t stride;
  uint64_t seed_step;
  const char* base;
  int xcd;     // 1: place each client's workgroups on its own XCD(s) (common.h xcd_client_map)
};
extern int g_xcd_clients;   // set_tuning("xcd_clients"): the ClientBatch::xcd of new batched contexts
ClientBatch& client_batch();
// host: throws std::runtime_error when a batched launch is handed a pointer outside client 0's slab
void check_slab(const void* p, const char* what);
// host: throws when the launch has no batched form
void require_unbatched(const char* what);
template <class... P>
inline void check_slabs(const char* what, P... ps) {
  (check_slab((const void*)ps, what), ...);
}

struct GemmArgs {
  const float* a;
  const float* b;
  float* c;
  const float* bias;
  float* ms;   // EPI_MASK: read; EPI_LRELU_DROPOUT: written (slope * keep / (1 - p))
  // EPI_LRELU_DROPOUT on D's last hidden layer (nullable): also write the backward seed of that
  // layer, head_a[m, n] = head_coef[m] * head_v[n] * (slope * keep / (1 - p))  (the D head's
  // A_{L-1} = coef * v * MS_{L-1}, which needs no reduction)
  const float* head_coef;
  const float* head_v;
  float* head_a;
  int ldha;
  float* ws;   // split-K partial slabs [splitk][M][N]
  int M, N, K;
  int lda, ldb, ldc, ldms;
  int ta, tb;
  float alpha, beta;
  int epi;
  float slope, p_drop;
  // EPI_BN_EVAL_RELU: out = relu((v - rm) * rsqrt(rv + eps) * gamma + beta)
  const float* bn_gamma;
  const float* bn_beta;
  const float* bn_rm;
  const float* bn_rv;
  float bn_eps;
  uint64_t seed;
  const uint64_t* rng_ctr;
  uint32_t rng_stream;
  int splitk, kchunk;
  int vec;     // 1: both operands may be read with 16-B loads (see gemm.hip Chunk::load)
  int tile;    // output tile edge: 64 (default) or 32 (4x the workgroups, for short-K GEMMs)
  int f32;     // 1: exact-fp32 MFMA (v_mfma_f32_16x16x4_f32); 0: bf16 operands, fp32 accumulate
  int xcd_remap;   // XCD-contiguous tile order (set by launch_gemm): 1 N-fastest, 2 M-fastest
  int wt;          // 1: write-through (sc1) output stores (set by launch_gemm)
  // One-hot conditional block (nullable): the K columns of op(A) are only the DENSE part of the
  // input; its trailing one-hot block (the conditional vector c, exactly one 1 per row at
  // oh_off[oh_col[m]] + oh_opt[m]) is applied as a gather of one weight column per row in the
  // epilogue: v += oh_w[n * oh_ld + oh_off[oh_col[m]] + oh_opt[m]]   (op(B) = B^T row-major weight)
  const float* oh_w;
  int oh_ld;
  int oh_trans;   // 1: oh_w is the transposed block [C, N] (coalesced gathers: lanes of a row read
                  //    consecutive n) -- v += oh_w[(oh_off[oh_col[m]] + oh_opt[m]) * oh_ld + n]
  const int* oh_col;
  const int* oh_opt;
  const int* oh_off;
  // BatchNorm partial statistics (nullable; 32/64 tiles, no split-K, plain C = A B^T + bias): every
  // tile writes, per output column and batch (rows [0, bn_rpg) / [bn_rpg, M)), its row count, mean
  // and sum of squared deviations: bn_part[((m_tile * 2 + batch) * 3 + {0,1,2}) * N + n]
  float* bn_part;
  int bn_rpg;
  int oh_c;       // width of the one-hot block (checked build: gather index bound)
  // Split-K reduced inside the GEMM launch (nullable): one arrival counter per output tile, zero
  // between launches.  Every K-slice workgroup publishes its slab write-through and takes a ticket;
  // the one that completes a tile sums the tile's slabs and applies the epilogue (no
  // gemm_splitk_epilogue launch).  red_inl is set by the launcher where the shape allows it.
  unsigned* tile_cnt;
  int red_inl;
  // bf16 storage (generation): bin = 1 -> both operands are bf16 rows (a16 [M, K] / b16 [N, K], k
  // contiguous, 16-B aligned, ld % 8 == 0), staged into LDS without conversion; c16 (nullable) ->
  // the epilogue writes bf16 (no split-K, no beta).  The values are the ones the fp32 path rounds
  // to bf16 at staging, so a bf16 activation buffer gives bit-identical products.
  const uint16_t* a16;
  const uint16_t* b16;
  uint16_t* c16;
  int bin;
  // Adam applied in the epilogue (gemm_adam_kernel only; nullable): the output is a weight gradient
  // inside an optimizer's flat gradient buffer; adam_p / adam_m / adam_v point at the same offset of
  // the parameter / moment buffers, so output (m, n) updates element m * ldc + n of each.  The
  // gradient itself is still written to c.
  float* adam_p;
  float* adam_m;
  float* adam_v;
  const float* adam_step;
  float adam_lr, adam_b1, adam_b2, adam_eps, adam_wd;
  int adam_grad;   // gemm_shortk_kernel<ADAM>: also store the gradient (gemm_adam_kernel always does)
  // chained GEMM (host-side pointer, nullable; chain_epilogue_kernel): once this GEMM's output C [M, N]
  // is final, the tail C2 = epi2(C B2^T + bias2) (the tail's own GemmArgs: op(A2) = this C, row-local,
  // K2 = N <= 1024) is computed in this GEMM's reduction launch, as fp32 dot products
  const struct GemmArgs* chain;
  // batched clients (ClientBatch; set by the launchers): nclient = grid.z / splitk
  int64_t cstride;
  uint64_t seed_step;
  int nclient;
  int xcd_cl;   // ClientBatch::xcd
  int chain_co;   // chained tail (chain_epilogue_kernel): lane-contiguous weight rows + wave sums (g_chain_coalesced)
  // chained tail with a head seed (head_a = A1) only, nullable: the backward link A0 = (A1 W1) . MS0 formed in the
  // same launch (gemm_achain_next): each (row group, 64-column slab) workgroup stores its slab's partial product
  // A1[:, slab] W1[slab, :] into ach_ws [slabs, M, K] write-through and takes a ticket on ach_cnt[row group] (zero
  // between launches); the row group's last workgroup sums the slabs in order and applies the head's mask MS0
  float* ach_out;
  float* ach_ws;
  unsigned* ach_cnt;
  int ld_ach;
};

void launch_gemm(GemmArgs g, hipStream_t stream);
// checked build: the OR of the check bits raised since the last call in each kernel TU (cleared)
unsigned check_status_gemm();
unsigned check_status_ctgan_ops();
unsigned check_status_vgm();
// two independent GEMMs in one launch where the pair is instantiated, else two launches
void launch_gemm_pair(GemmArgs g1, GemmArgs g2, hipStream_t stream);
extern int g_gemm_pairs;
extern int g_gemm_pair_max_wg;

struct SampleArgs {
  int B, E, C, Dd, n_col, maxw, n_rows;
  float* h;            // generator input rows: z at h[r*ldh + zc], cond at h[r*ldh + cc]
  int ldh, zc, cc;
  // generation into a bf16 activation buffer (nullable): z as bf16 at h16[r*ldh16 + zc16]; h and
  // the one-hot block are then not written (the GEMMs gather the condition from col / opt)
  uint16_t* h16;
  int ldh16, zc16;
  float* xf;           // fake block of the D input (cond copy at xf[r*ldx + Dd]); nullable
  float* xr;           // real block [data row | cond of the permuted fake row]; nullable
  int ldx;
  const float* cdf;    // [n_col, maxw]
  const int* cond_off;
  const int* cond_w;
  const int64_t* row_off;   // [n_col, maxw]
  const int64_t* row_cnt;   // [n_col, maxw]
  const int64_t* rows;      // CSR row lists
  int64_t n_entries;        // length of `rows` (checked build: CSR pick bound)
  const float* data;        // encoded training matrix [n_rows, Dd]
  int* col;
  int* opt;
  int n_real;               // rows [0, n_real) also draw a real row into xr (xr has n_real rows)
  float* step_bump;         // optimizer step counter bumped by this launch (nullable)
  float* step_bump2;        // a second one (both phases of a step drawn by one launch; nullable)
  float* metrics;           // zeroed by this launch when zero_metrics
  int zero_metrics;
  uint64_t seed;
  const uint64_t* rng_ctr;
  uint32_t rng_stream;
  // draws > 1: the batches of `draws` consecutive training steps in ONE launch (blockIdx.y = draw k, keyed on
  // RNG step *rng_ctr + k, its outputs at the pointers above + k x draw_*).  step_bump / step_bump2 then point at
  // [draws] per-step counter arrays whose last entry is the canonical counter: entry q becomes last + q + 1 (the
  // value the q-th per-step launch would have bumped it to), and metrics at [draws, 4] zeroed.
  int draws;
  int64_t draw_h, draw_x, draw_col;
  ClientBatch cb;           // set by launch_sample
};

void launch_sample(const SampleArgs& a, hipStream_t stream);

struct SpanTables {
  const int* start;
  const int* width;
  const int* kind;      // 0 tanh, 1 softmax
  const int* cond_idx;  // softmax span -> conditional column index (or -1)
  // host-packed copy of every table the activation kernels stage in LDS, in LDS order:
  // [elem_span | SOFTMAX bit (D) | kind (S) | start (S) | width (S) | cond_idx (S)], zero-padded to a
  // multiple of 4 ints (one 16-B-load copy per workgroup instead of per-table loops)
  const int* packed;
  int n_span;
  int dim;              // data_dim (sum of widths)
};
inline int span_packed_len(int dim, int n_span) { return (dim + 4 * n_span + 3) & ~3; }

size_t activation_smem_bytes(const SpanTables& sp);   // dynamic LDS of the activation kernels

// optional slerp(real, fake) fused onto the activation of the fake rows (real == nullptr: off)
struct SlerpFuse {
  const float* real;   // [rows, ld] real rows
  float* out;          // [rows, ld] interpolates
  int ld, cols;        // cols = data_dim + n_opt (the fake row continues past the activation)
  int rows;            // only activation rows r < rows are interpolated
  uint32_t stream;
};
void launch_activate(const float* logits, int ldl, float* out, int ldo, int rows, SpanTables sp, float tau,
                     uint64_t seed, const uint64_t* ctr, uint32_t stream_id, SlerpFuse sl, hipStream_t stream);

void launch_act_bwd_ce(const float* dact, int ldd, const float* act, int lda, const float* logits, int ldl, SpanTables sp,
                       const int* col, const int* opt, float* dlogits, int ldg, int rows, float tau, float* loss,
                       int loss_per_row, hipStream_t stream);

void launch_slerp(const float* real, const float* fake, float* out, int rows, int cols, int ld, uint64_t seed,
                  const uint64_t* ctr, uint32_t stream_id, hipStream_t stream);

// ws (nullable, >= rows * ceil(cols / 8192) floats): rows wider than 8,192 run as a chunk-split partial-sum
// launch + a scale launch (g_gp_split) instead of one workgroup per row
void launch_gp_scale(const float* g, int ldg, float* out, int ldo, int rows, int cols, float lam, float* loss,
                     int loss_per_row, float* ws, int64_t ws_n, hipStream_t stream);
extern int g_gp_split;
extern int g_chain_coalesced;   // set_tuning("chain_coalesced")
extern int g_chain_pre;         // set_tuning("chain_pre")
extern int g_chain_rows;        // set_tuning("chain_rows")
extern int g_gp_threads;   // register-resident gp_scale workgroup size (set_tuning("gp_threads"))
extern int g_bn_threads;   // BN workgroup size (set_tuning("bn_threads"))
extern int g_bn_slices;    // paired training BN: workgroups per batch that store rows (set_tuning("bn_slices"))
extern int g_act_rowreg_narrow;   // narrow rows on the register-resident row kernels (set_tuning("act_rowreg_narrow"))

// Weight gradient of a one-hot conditional input block (generator layers, input-major weights): row k of the
// block's gradient is the sum of the upstream-gradient rows whose condition index is k (rows in batch order, so
// the result is deterministic); every other row stays zero.  zero != 0 clears the rows the batch touched (after
// the optimizer has read them), restoring the all-zero block for the next step.
struct OnehotWJob {
  const float* dy;   // [B, n] upstream gradient rows
  float* w;          // row k of the block's gradient at w + k * ldw
  int ldy, ldw, n;
};
struct OnehotWBatch {
  OnehotWJob jobs[4];
  int n_jobs, B;
  const int* col;        // [B] conditioned column
  const int* opt;        // [B] its option
  const int* cond_off;   // [n_col] first block row of each column
};
void launch_onehot_wgrad(const OnehotWBatch& bt, int zero, hipStream_t stream);

void launch_d_head(const float* d, int ldd, const float* ms, int ldms, const float* v, const float* e,
                   const float* coef, const float* wloss, float* y, float* a, int lda, int rows, int cols, float* loss,
                   hipStream_t stream);

// out[c] = sum_r w[r] a[r, c] (w nullable = 1; out nullable); with dot_v, additionally
// *dot_out += sum_c dot_v[c] * (sum_r u[r] a[r, c]) + dot_e[0] * sum_r u[r], u = dot_w (or w
// when dot_w is null): the WGAN loss sum_r u[r] (d_r . v + e) of the D head, folded into the
// bias-gradient launch.  With dot_w, one job gives the head's weight gradient (weights w) and
// the loss (weights dot_w) from one pass over the rows.
struct ColsumJob {
  const float* a;
  int lda, rows, cols;
  float* out;
  const float* w;
  const float* dot_v;
  const float* dot_e;
  float* dot_out;
  const float* dot_w;
};
void launch_colsum(const ColsumJob* jobs, int n_jobs, hipStream_t stream);

// Adam over a flat buffer with up to 8 column-sum jobs folded into the same launch; a job whose
// output lies in the gradient buffer owns [own_lo, own_hi) (elements, 4-aligned) and the Adam
// update of those elements is applied from the freshly reduced sums.
constexpr int ACS_COLS = 16, ACS_GROUPS = 64;
struct AdamColsum {
  ColsumJob jobs[8];
  int n_jobs;
  int vec[8];         // rows 16-B aligned and padded to >= ceil4(cols): float4 loads
  int blk_start[9];   // filled by the launcher
  int64_t own_lo[8], own_hi[8];
  int dot_self[8];    // dot_v is this job's own output's parameters: use the pre-update values
  int64_t skip_lo, skip_hi;   // elements updated by a fused GEMM's Adam epilogue (gemm_adam_kernel)
  int64_t skip2_lo, skip2_hi; // and by a short-K weight gradient that applied Adam ahead of this launch
                              // (launch_gemm_shortk_adam); both ranges 4-aligned, disjoint, skip_lo <= skip2_lo
};
// C = A^T B by gemm_shortk_kernel with Adam applied to the outputs in its epilogue (g.adam_* set as for
// gemm_adam_kernel; the gradient itself is stored only with g.adam_grad); false: shape not taken
bool launch_gemm_shortk_adam(GemmArgs g, hipStream_t stream);
void launch_adam_colsum(float* p, const float* g, float* m, float* v, const float* step, int64_t n, float lr, float b1,
                        float b2, float eps, float wd, uint64_t* rng_ctr_bump, const AdamColsum& cs,
                        hipStream_t stream);
// a weight-gradient GEMM (g.adam_* set, unsplit) and the Adam + column-sum launch of the same
// optimizer (its flat range [cs.skip_lo, cs.skip_hi) left to the GEMM) in ONE launch; returns false
// (nothing launched) where that GEMM shape is not instantiated
bool launch_gemm_adam(GemmArgs g, float* p, const float* gr, float* m, float* v, const float* step, int64_t n,
                      float lr, float b1, float b2, float eps, float wd, uint64_t* rng_ctr_bump, const AdamColsum& cs,
                      hipStream_t stream);

extern int g_gemm_xcd_remap;   // GEMM XCD-contiguous tile order: 0 off, 1 long-K tiles, 2 always
extern int g_gemm_xcd_nmajor;  // let a GEMM take the M-fastest XCD tile order when it touches fewer bytes
extern int g_adam_store;       // Adam p/m/v store policy: 0 plain, 2 nt, 16 sc1 write-through
extern int g_adam_max_blocks;  // Adam grid cap (grid-stride beyond it)
extern int64_t g_adam_u_min;   // Adam launches over >= this many float4 (x clients) load ADAM_U float4 per thread
extern int g_gemm_store_wt;   // GEMM outputs / split-K slabs: plain (0) or write-through sc1 (1)
extern int g_gemm_shortk;          // 1: C = A^T B with K <= 160, M <= 256 and wide N by gemm_shortk_kernel
extern int g_gemm_shortk_min_n;    // narrowest N that takes it
extern int g_gemm_shortk_store;    // its output stores: 0 plain, 1 non-temporal, 2 write-through (sc1)
extern int g_gemm_splitk_inlaunch;   // split-K reduced inside the GEMM launch where a tile counter is given (1)
extern int g_act_row_mode;   // activation kernels on rows wider than 512: one workgroup per row (1) or per 1-4 rows
extern int g_decode_rows;   // generation decode: one wave per row (1) or one thread per (row, column) (0)
extern int g_bn_cols;   // BatchNorm kernels: columns per workgroup (4 / 8 / 16); set_tuning("bn_cols")
void launch_bn_relu_train(const float* a, int lda, const float* gamma, const float* beta, float* out, int ldo,
                          float* nhat, int ldn, float* mean, float* invstd, float* rm, float* rv, int rows, int cols,
                          int groups, float momentum, float eps, hipStream_t stream);

// Linear -> BatchNorm(train) -> ReLU in one launch by column ownership (kernels/bn_fused.hip): a
// workgroup owns 16 output columns of one batch.  x [groups * rpg, K] (unit column stride),
// W(n, k) = w[n * w_sn + k * w_sk]; the optional one-hot block adds oh_w[n * oh_sn + j * oh_sc] with
// j = oh_off[oh_col[r]] + oh_opt[r]; stat [groups][2][N] and cnt [ceil(N / 16)] (zero between launches)
// carry the batch statistics to the running-stat update when groups == 2.
struct ColOwnArgs {
  const float* x;
  int ldx;
  const float* w;
  int64_t w_sn, w_sk;
  const float* bias;
  const float* oh_w;
  int64_t oh_sn, oh_sc;
  const int* oh_col;
  const int* oh_opt;
  const int* oh_off;
  const float* gamma;
  const float* beta;
  float* out;
  int ldo;
  float* nhat;
  int ldn;
  float* mean;
  float* invstd;
  float* rm;
  float* rv;
  float* stat;
  unsigned* cnt;
  int rpg, groups, K, N;
  float momentum, eps;
  int64_t cstride;   // set by the launcher (batched clients)
  int dbg;           // phase-cost probe (set_tuning("colown_dbg")): 1 no GEMM, 2 no staging, 4 no stores
};
extern int g_colown_dbg;
size_t colown_smem_bytes(int K, int rpg);
void launch_linear_bn_relu_colown(ColOwnArgs g, bool vec, hipStream_t stream);

// BatchNorm(train) + ReLU from the GEMM's per-tile partial statistics (kernels/ctgan_ops.hip)
void launch_bn_relu_apply(const float* a, int lda, const float* part, int n_tiles, const float* gamma,
                          const float* beta, float* out, int ldo, float* nhat, int ldn, float* mean, float* invstd,
                          float* rm, float* rv, int rows, int cols, int groups, float momentum, float eps,
                          hipStream_t stream);
void launch_bn_relu_bwd(const float* dr, int lddr, const float* r, int ldr, const float* nhat, int ldn,
                        const float* gamma, const float* invstd, float* da, int ldda, float* dgamma, float* dbeta,
                        float* dbias, int rows, int cols, hipStream_t stream);
// operands of one BatchNorm(train) + ReLU backward (bn_bwd.h)
struct BnBwdArgs {
  const float* dr;
  int lddr;
  const float* r;
  int ldr;
  const float* nhat;
  int ldn;
  const float* gamma;
  const float* invstd;
  float* da;
  int ldda;
  float* dgamma;
  float* dbeta;
  float* dbias;   // nullable
  int rows, cols;
};
// the BN backward's column workgroups and an INDEPENDENT weight-gradient GEMM (op(A) = A^T, bf16 MFMA, 32/64
// tile) in ONE launch (horizontal fusion: the 32-64 narrow, latency-bound BN workgroups no longer run alone on the
// chip).  Returns false (nothing launched) where that combination is not instantiated.
bool launch_gemm_bnbwd(GemmArgs g, const BnBwdArgs& b, hipStream_t stream);
extern int g_bnb_first;   // gemm_bnbwd_kernel: BN workgroups before (1) or after (0) the GEMM tiles
extern int g_bnb_cols;    // gemm_bnbwd_kernel: columns per BN workgroup (4 or 8)

void launch_adam(float* p, const float* g, float* m, float* v, const float* step, int64_t n, float lr, float b1,
                 float b2, float eps, float wd, uint64_t* rng_ctr_bump, hipStream_t stream);

struct DecodeArgs {
  const float* logits;
  int ldl, rows, n_cols;
  const int* kind;      // per output column: 0 continuous, 1 categorical
  const int* start;     // span start (continuous: the tanh unit; modes follow)
  const int* width;     // #valid modes / #categories
  const int* cont;      // continuous column index into mu/sd
  const int* code_off;  // categorical: offset into codes
  const double* codes;
  int n_codes;          // length of `codes` (checked build)
  const double* mu;     // [n_cont, K]
  const double* sd;
  int K;
  double* out;          // [rows, n_cols]
  uint64_t seed;
  const uint64_t* rng_ctr;
  uint32_t rng_stream;
  int dim;              // logits per row
  const int* ecol;      // [dim] element -> output column whose argmax it enters (-1: none, e.g. alpha)
  // [n_quads][2] (nullable): every run of up to 4 logits of one column that share a Philox word:
  // {column | count << 24, offset-in-span << 16 | position}
  const int* quads;
  int n_quads;
};
void launch_sample_decode(const DecodeArgs& a, hipStream_t stream);

void launch_rng_bump(uint64_t* ctr, hipStream_t stream);

// Conditional generation (kernels/cond_gen.hip): a request for rows with given category values, entirely in
// device buffers, so one captured pass serves every request with the same numbers of bins and fixed columns.
constexpr int COND_MAX_BINS = 64;   // requested values of the driving column
struct CondReq {
  const int* drive;          // [2]: the driving column's cond-span index, its output column
  int n_bins;
  const int* bin_opt;        // [n_bins] option index in the driving span
  const double* bin_code;    // [n_bins] label code the decoded row must carry
  const int64_t* quota;      // [n_bins] rows wanted
  int64_t* filled;           // [n_bins] rows delivered so far
  const int64_t* seg_off;    // [n_bins] exclusive prefix of the quotas: first dst row of the bin's segment
  int n_fixed;
  const int* fixed_j;        // [n_fixed] output columns of the other requested columns
  const double* fixed_code;  // [n_fixed] their label codes
  int64_t* stats;            // [2]: rows generated, rows that passed the predicate
};
struct CondRequestArgs {
  CondReq req;
  int rows;
  int* col;                  // [rows] the sampler's draw, overwritten with the driving span
  int* opt;                  // [rows] ... and the drawn bin's option
  int* tgt;                  // [rows] the drawn bin (-1: every quota is full)
  float* h;                  // nullable: fp32 activation buffer whose one-hot block [cc, cc + C) follows the draw
  int ldh, cc, C;
  const int* cond_off;       // [n_span]
  const int* cond_w;         // [n_span]
  int n_span;
  uint64_t seed;
  const uint64_t* rng_ctr;
  uint32_t rng_stream;
};
void launch_cond_request(const CondRequestArgs& a, hipStream_t stream);
struct CondPartitionArgs {
  CondReq req;
  const double* out;         // [rows, n_cols] decoded pass
  int rows, n_cols;
  const int* tgt;            // [rows]
  int* keep;                 // [rows] scratch: the row's bin if it is kept, else -1
  int* counts;               // [cond_partition_workgroups(rows), n_bins] scratch: kept rows per workgroup and bin
  double* dst;               // [n_dst, n_cols] the quota segments
  int64_t n_dst;
  int any_value;             // off by default; on: no value predicate, a row with a target is kept (the privacy guard
                             // without a request: one bin, drive / bin_code / fixed_* unread)
};
int cond_partition_workgroups(int rows);
void launch_cond_partition(const CondPartitionArgs& a, hipStream_t stream);
unsigned check_status_cond_gen();

// Range and set predicates of a conditional request (kernels/cond_pred.hip), in device buffers like the request
// itself: a range on a continuous column (lo <= x <= hi in the decoded space), a set on a categorical column (a
// byte per label code).  A predicate may also drive: its span's options are then drawn by weight.
constexpr int PRED_MAX = 16;        // predicates per request
struct PredReq {
  int n_pred;
  const int* j;              // [n_pred] output column
  const int* kind;           // [n_pred] 0: range, 1: set
  const double* lo;          // [n_pred] inclusive bounds of a range (-inf / +inf: open)
  const double* hi;
  const int* lut_off;        // [n_pred] a set's first byte in lut
  const int* lut_len;        // [n_pred] ... and its bytes: one per label code, 1 = allowed
  const uint8_t* lut;        // [lut_total]
  int lut_total;
  int64_t* stats;            // [2 + PRED_MAX]: rows tested, rows rejected, first failures per predicate
};
struct PredRequestArgs {
  const int* drv;            // [2]: the driving span, its output column
  const int* drv_opt;        // [M] the span's options with positive weight, in option order
  const double* drv_cum;     // [M] their cumulative normalised weights, drv_cum[M - 1] == 1.0
  int M;
  const int64_t* quota;      // [1]
  const int64_t* filled;     // [1]
  int rows;
  int* col;                  // as CondRequestArgs
  int* opt;
  int* tgt;                  // [rows] 0 (-1: the quota is full)
  float* h;
  int ldh, cc, C;
  const int* cond_off;
  const int* cond_w;
  int n_span;
  uint64_t seed;
  const uint64_t* rng_ctr;
  uint32_t rng_stream;
};
void launch_pred_request(const PredRequestArgs& a, hipStream_t stream);
struct PredMarkArgs {
  PredReq p;
  const double* out;         // [rows, n_cols] decoded pass
  int rows, n_cols;
  int* tgt;                  // [rows] -1 where a predicate fails
};
void launch_pred_mark(const PredMarkArgs& a, hipStream_t stream);
unsigned check_status_cond_pred();

// Completion of partial rows (kernels/known_gen.hip): every known row (query) has its own condition, its own block
// of `tries` consecutive candidate rows of a pass (a slot) and its own best candidate so far.  The table, its
// per-row drivers and the per-query state live in device buffers; a pass names its queries in qidx, so one captured
// pass serves every pass of the same size.
constexpr int KNOWN_MAX_TRIES = 1024;   // candidate rows per query and pass
struct KnownRequestArgs {
  const int* qidx;           // [n_slots] the slot's query, -1: idle
  int n_slots, tries;        // rows of the pass = n_slots * tries
  int64_t n_query;           // rows of drv_span / drv_opt
  const int* drv_span;       // [n_query] cond-span that drives the query's rows, -1: none (the sampler's draw stays)
  const int* drv_opt;        // [n_query] ... and its option
  int* col;                  // [rows] as CondRequestArgs
  int* opt;
  float* h;
  int ldh, cc, C;
  const int* cond_off;
  const int* cond_w;
  int n_span;
};
void launch_known_request(const KnownRequestArgs& a, hipStream_t stream);
struct KnownMatchArgs {
  const double* known;       // [n_query, n_cols] the partial table (an unknown cell's value is never read)
  const uint8_t* mask;       // [n_query, n_cols] != 0: the cell is known
  int64_t n_query;
  int n_cols;
  const int* qidx;           // [n_slots]
  int n_slots, tries;
  const double* cand;        // [n_slots * tries, n_cols] decoded pass; slot s owns rows s * tries ...
  const int* kind;           // [n_cols] 0: continuous, 1: categorical (codes compared, never used as an index)
  const double* scale;       // [n_cols] continuous columns: 1 / (max - min)
  double* best;              // [n_query] smallest d2 so far (+inf before the first pass)
  double* dc;                // [n_query] its continuous part
  int* miss;                 // [n_query] its categorical mismatches
  int64_t* seen;             // [n_query] candidates judged so far
  int64_t* pick;             // [n_query] the best candidate's number among them
  double* dst;               // [n_query, n_cols] completed rows
};
void launch_known_match(const KnownMatchArgs& a, hipStream_t stream);
unsigned check_status_known_gen();

// Similarity evaluator (kernels/similarity.hip): Avg_JSD / Avg_WD of a decoded table against a real one, on the
// device.  Counting is in integers and every fp64 sum has a fixed order, so a table scores bit-identically on every
// run; no launch allocates or waits on the host.
constexpr int SIM_SORT_TILE = 2048;   // doubles per sorted LDS tile / merged output tile
enum SimKind : int { SIM_PLAIN = 0, SIM_NONNEG = 1, SIM_CAT = 2 };
struct SimPrepareArgs {
  const double* values;   // [rows, n_cols] decoded table, row-major
  int rows, n_cols;
  const int* kind;        // [n_cols] SimKind
  const int* slot;        // [n_cols] row of keys (continuous) / counts (categorical)
  const int* vocab;       // [n_cat] codes of column slot s lie in [0, vocab[s])
  double* keys;           // [n_cont, ldk] column-major keys; +inf where the CSV would carry no number
  int64_t ldk;
  int* valid;             // [n_cont] finite keys per column
  int* counts;            // [n_cat, ldc] occurrences of each code
  int ldc, n_cont, n_cat;
};
void launch_sim_prepare(const SimPrepareArgs& a, hipStream_t stream);
// rows [0, n) of every segment keys[s * ld ...] ascending, in place; tmp: scratch of the same shape
void launch_sim_sort(double* keys, double* tmp, int n_seg, int64_t ld, int n, hipStream_t stream);
struct SimW1Args {
  const double* real;     // [n_cont, ldr] ascending
  int64_t ldr;
  const int* n_real;      // [n_cont]
  const double* fake;     // [n_cont, ldf] ascending, the valid values first
  int64_t ldf;
  const int* n_fake;      // [n_cont] valid fake values
  int n_cont, max_real, max_fake;
  double* part;           // [n_cont, sim_w1_chunks(max_real + max_fake)] scratch
  double* out;            // [n_cont]
};
int sim_w1_chunks(int64_t n);
void launch_sim_w1(const SimW1Args& a, hipStream_t stream);
struct SimJsdArgs {
  const int* real;        // [n_cat, ldc] counts of the real categories (slots past the vocabulary: real-only values)
  const int* fake;        // [n_cat, ldc]
  int ldc, n_cat;
  double* out;            // [n_cat]
};
void launch_sim_jsd(const SimJsdArgs& a, hipStream_t stream);
// scores = [avg_jsd, avg_wd, jsd x n_cat, wd x n_cont]: the two means from the per-column values behind them
void launch_sim_mean(double* scores, int n_cat, int n_cont, hipStream_t stream);
unsigned check_status_similarity();

// Privacy evaluator (kernels/privacy.hip): distance to the closest record and nearest-neighbour distance ratio of a
// decoded table against a real one.  d2(q, r) = sum over continuous columns of (q_c - r_c)^2 after the real table's
// min-max scaling + the number of categorical columns whose codes differ, in fp64 from direct differences.
constexpr int NN_QUERY_TILE = 256;    // query rows per workgroup (one per thread)
constexpr int NN_REF_TILE = 16;       // reference rows staged in LDS at a time
constexpr int NN_CHUNK_ROWS = 2048;   // reference rows per chunk (grid y); a (query, chunk) pair leaves one partial
enum NnKind : int { NN_CONT = 0, NN_CAT = 1 };
struct NnPackArgs {
  const double* values;   // [rows, n_cols] decoded table, row-major
  int rows, n_cols;
  const int* kind;        // [n_cols] NnKind
  const int* slot;        // [n_cols] column of cont / cat
  const double* lo;       // [n_cont] the real column's minimum
  const double* scale;    // [n_cont] 1 / (max - min), 1 for a constant column
  double* cont;           // [rows, n_cont] (v - lo) * scale
  int* cat;               // [rows, n_cat] codes (a value that is no code in [0, 2^31 - 1): -1)
  int n_cont, n_cat;
};
void launch_nn_pack(const NnPackArgs& a, hipStream_t stream);
struct NnTop2Args {
  const double* q_cont;   // [nq, n_cont]
  const int* q_cat;       // [nq, n_cat]
  const double* r_cont;   // [nr, n_cont]
  const int* r_cat;       // [nr, n_cat]
  int nq, nr, n_cont, n_cat;
  int exclude_self;       // reference row j == query row i is no candidate
  int chunks;             // set by the launcher, as the partials are: [chunks, nq] each, carved from scratch
  double* part_d1;
  double* part_d2;
  int* part_i1;
};
int nn_chunks(int64_t nr);
int64_t nn_scratch_doubles(int64_t nq, int64_t nr);   // fp64 elements of scratch launch_nn_top2 needs
// per query: d1 <= d2 the two smallest d2 over the candidates (with multiplicity; +inf where there are fewer) and
// i1 the lowest index at distance d1 (-1: no candidate)
void launch_nn_top2(NnTop2Args a, double* d1, double* d2, int* i1, double* scratch, hipStream_t stream);
struct NnWithinArgs {
  const double* q_cont;   // [nq, n_cont]
  const int* q_cat;       // [nq, n_cat]
  const double* r_cont;   // [nr, n_cont]
  const int* r_cat;       // [nr, n_cat]
  int nq, nr, n_cont, n_cat;
  const double* t2;       // [1] on the device: the squared radius (one captured launch serves every threshold)
  int* near;              // [nq] lowest index of a reference row with d2 <= t2, or -1
  int* part;              // [nn_chunks(nr), nq] scratch: the per-chunk answers
  int chunks;             // set by the launcher
};
// the radius test of the privacy guard: d2 as launch_nn_top2 computes it, candidates abandoned once out of range
void launch_nn_within(NnWithinArgs a, hipStream_t stream);
// tgt[i] = -1 where near[i] >= 0; stats[0] += n, stats[1] += rows with near >= 0
void launch_guard_mark(const int* near, int* tgt, int n, int64_t* stats, hipStream_t stream);
// Federated audit / guard (eval/fed_privacy.py): the answers of K shards folded into the answer over their union.
constexpr int NN_MAX_SHARDS = 64;     // shards one merge folds (a thread walks them in order)
struct NnMergeShardsArgs {
  const double* parts;    // [k, n, 3]: shard s's (d1, d2, i1 as fp64; -1: no candidate) per query row
  const int64_t* offsets; // [k] exclusive prefix sums of the shard row counts
  int k, n;
  double* d1;             // [n] the two smallest distances over the union, with multiplicity
  double* d2;
  int* i1;                // [n] offsets[s] + local of the lowest global index at d1, -1: none
  int* owner;             // [n] that s, -1: none
  unsigned long long* by_client;   // [2, k], overwritten: rows nearest to shard s; rows shard s holds a copy of
};
void launch_nn_merge_shards(const NnMergeShardsArgs& a, hipStream_t stream);
// near [k, n]: shard s's lowest local hit or -1 -> near_out[n] = offsets[s] + near[s] of the first shard with a hit
void launch_nn_within_merge_shards(const int* near, const int64_t* offsets, int k, int n, int* near_out, int* owner,
                                   hipStream_t stream);
int nn_stats_blocks(int64_t n);
// keys [2, ld]: sqrt(d1) and the ratio sqrt(d1 / d2) of rows [0, n); part [2 * nn_stats_blocks(n)]
void launch_nn_stats(const double* d1, const double* d2, int n, double* keys, int64_t ld, double* part,
                     hipStream_t stream);
// out[0..3] = 5th percentile of each (ascending) key row, smallest sqrt(d1), share of rows with d1 == 0
void launch_nn_percentiles(const double* keys, int64_t ld, int n, const double* part, double* out, hipStream_t stream);

// Fidelity evaluator (kernels/fidelity.hip): precision / recall / density / coverage of a decoded table against a real
// one (Naeem et al. 2020), in the privacy evaluator's row space and metric, on its grid (NN_QUERY_TILE, NN_REF_TILE,
// NN_CHUNK_ROWS).  Every distance of these kernels comes from one device function, so a distance of one pass and a
// radius of another compare exactly.
constexpr int FID_MAX_K = 8;          // the largest k: a (query, chunk) pair keeps its k smallest d2 in registers
struct NnPairs {
  const double* q_cont;   // [nq, n_cont]
  const int* q_cat;       // [nq, n_cat]
  const double* r_cont;   // [nr, n_cont]
  const int* r_cat;       // [nr, n_cat]
  int nq, nr, n_cont, n_cat;
  int chunks;             // set by the launcher
};
struct NnTopkArgs {
  NnPairs p;
  int exclude_self;       // reference row j == query row i is no candidate
  int k;                  // 1..FID_MAX_K
  double* part;           // [chunks, k, nq] scratch: the k smallest d2 of a (query, chunk), ascending
  double* out;            // [nq] the k-th smallest d2 over the candidates, with multiplicity (+inf: fewer than k)
};
int64_t nn_topk_scratch_doubles(int64_t nq, int64_t nr, int k);
void launch_nn_topk(NnTopkArgs a, double* scratch, hipStream_t stream);
struct NnBallArgs {
  NnPairs p;
  const double* r_rad2;   // [nr] squared radius of a reference row's ball (+inf: everything but NaN is inside)
  int* part_cnt;          // [chunks, nq] scratch, carved by the launcher
  double* part_min;       // [chunks, nq]
  int* cnt;               // [nq] number of reference rows r with d2(q, r) <= r_rad2[r]
  double* dmin;           // [nq] smallest d2(q, r) (+inf: every distance is NaN)
};
int64_t nn_ball_scratch_doubles(int64_t nq, int64_t nr);
void launch_nn_ball(NnBallArgs a, double* scratch, hipStream_t stream);
struct PrdcArgs {
  const int* cnt_a;       // [n] real balls a generated row is inside
  const int* cnt_b;       // [m] generated balls a real row is inside
  const double* dmin_b;   // [m] a real row's distance to its nearest generated row
  const double* rr;       // [m] a real row's squared radius
  int n, m, k;
  double* scores;         // [>= 4] precision, recall, density, coverage
};
void launch_prdc_reduce(const PrdcArgs& a, hipStream_t stream);

// Correlation evaluator (kernels/correlation.hip): the [C, C] association matrix of a decoded table (Pearson r,
// Theil's U, correlation ratio) and its distance to the real table's.  Every fp64 sum has a fixed order, counting
// is in integers; no floating-point atomics, no allocation, no host round trip.
constexpr int CORR_CHUNK = 1024;            // rows per chunk; a workgroup sums a whole number of consecutive chunks
constexpr int CORR_COL_TILE = 64;           // continuous columns per workgroup of the column sums
constexpr int CORR_COUNT_ROWS = 8192;       // rows per workgroup of the contingency count
// int32 bins of a contingency table counted in LDS: 64 KiB, so two workgroups share a CU's 160 KiB with room to
// spare; a pair with more bins counts in its global table directly
constexpr int CORR_LDS_BINS = 16384;
constexpr int64_t CORR_PART_TARGET = 8ll << 20;   // fp64 partials (64 MiB) the row groups of corr_moments may fill
extern int64_t g_corr_part_target;                // set_tuning("corr_part_target"): the same, adjustable (tests)
enum CorrKind : int { CORR_CONT = 0, CORR_CAT = 1 };
struct CorrGroups {
  int groups;            // row groups: one partial each
  int rows;              // rows per group, a multiple of CORR_CHUNK
};
// the row split of a table of n rows with one-hot width W and n_cont continuous columns (a function of the shape
// alone, so a shape always sums in the same order)
CorrGroups corr_groups(int64_t n, int64_t W, int64_t n_cont);
int64_t corr_part_doubles(int64_t n_max, int64_t W, int64_t n_cont);   // what any n <= n_max needs
struct CorrPackArgs {
  const double* values;   // [rows, n_cols] decoded table, row-major
  int rows, n_cols;
  const int* kind;        // [n_cols] CorrKind
  const int* slot;        // [n_cols] column of cont / row of cat_t
  const int* card;        // [n_cat] K_c: codes lie in [0, K_c), anything else lands in the overflow bin K_c
  double* cont;           // [>= rows, n_cont] the continuous columns, row-major
  int* cat_t;             // [n_cat, ldk] codes, one row per column
  int64_t ldk;
  double* mean;           // [n_cont]
  double* part;           // scratch: one sum per (CORR_CHUNK rows, continuous column)
  int n_cont, n_cat;
};
void launch_corr_pack(const CorrPackArgs& a, hipStream_t stream);
struct CorrMomentsArgs {
  const double* cont;     // [>= n, n_cont]
  const int* cat_t;       // [n_cat, ldk]
  int64_t ldk;
  int n, n_cont, n_cat, W;
  const double* mean;     // [n_cont]
  const int* card;        // [n_cat]
  const int* offs;        // [n_cat + 1] first one-hot row of a column, less n_cont; offs[n_cat] = W - n_cont
  double* G;              // [W, n_cont] = F^T Xc with F = [Xc | one-hot(codes)]
  double* part;           // [groups, W, n_cont]
};
void launch_corr_moments(const CorrMomentsArgs& a, hipStream_t stream);
struct CorrCountsArgs {
  const int* cat_t;       // [n_cat, ldk]
  int64_t ldk;
  int n, n_cat, n_pairs;
  const int* pairs;       // [n_pairs, 4]: column a, column b (-1: the margin of a), bins of a, bins of b
  const int64_t* poff;    // [n_pairs + 1] first bin of a pair's table in counts
  int* counts;            // [total] int32 tables, row-major [bins of a][bins of b]
  int64_t total;
  int lds_bins;           // the largest table counted in LDS (<= CORR_LDS_BINS)
};
void launch_corr_counts(const CorrCountsArgs& a, hipStream_t stream);
struct CorrMatrixArgs {
  const double* G;        // [W, n_cont]
  const int* counts;
  const int64_t* poff;    // [n_pairs + 1]: margins of the n_cat columns first, then the pairs a < b in row-major order
  int64_t total;
  int n_pairs;
  const int* kind;        // [C]
  const int* slot;        // [C]
  const int* card;        // [n_cat]
  const int* offs;        // [n_cat + 1]
  int n, C, n_cont, n_cat, W;
  double* A;              // [C, C]
};
void launch_corr_matrix(const CorrMatrixArgs& a, hipStream_t stream);
// out[0] = ||A - B||_F, out[1] = mean |A - B| over the off-diagonal entries (0 for C == 1), out[2] = their maximum
void launch_corr_diff(const double* A, const double* B, int C, double* out, hipStream_t stream);

// ML-utility evaluator (kernels/utility.hip): a class-balanced, L2-regularised multinomial logistic regression fitted
// on a decoded table by a fixed number of bound-preconditioned accelerated gradient steps, and its confusion matrix on
// held-out rows (eval/utility_device.py has the definition).  All fp64; every sum has an order fixed by the shapes
// alone, counting is in integers; no floating-point atomics, no allocation, no host round trip.
// The limits: a lane of the one-workgroup factorisation owns one column of the [D, D] matrix (1024 threads), and a
// 64-row block of logits [64, K] lives in 33 KiB of LDS, so four workgroups share a CU's 160 KiB.
constexpr int UTIL_MAX_FEATURES = 1024;     // D: continuous columns + one-hot bins (with overflow bins) + intercept
constexpr int UTIL_MAX_CLASSES = 64;        // K: categories of the target column
constexpr int UTIL_ROWS = 64;               // rows of a block of logits / residuals in LDS
constexpr int UTIL_CHUNK = 128;             // rows per chunk; a row group is a whole number of consecutive chunks
constexpr int UTIL_SLAB = 256;              // features (rows of F^T R) per workgroup of the gradient
constexpr int64_t UTIL_PART_TARGET = 8ll << 20;   // fp64 partials (64 MiB) the row groups of one product may fill
enum UtilKind : int { UTIL_CONT = 0, UTIL_CAT = 1, UTIL_TARGET = 2 };
// the row split of n rows whose partials hold `cells` doubles each (a function of the shape alone)
CorrGroups util_groups(int64_t n, int64_t cells);
int64_t util_part_doubles(int64_t n_max, int64_t D, int64_t K);   // what gram and step need for any n <= n_max
// a packed table: standardised continuous features, clamped feature codes, target codes and sample weights
struct UtilTable {
  double* cont;           // [>= n, n_cont] (v - mean) / sd, row-major
  int* cat_t;             // [n_cat, ldk] codes of the categorical features, overflow bin card[c] included
  int* y;                 // [>= n] target code, K where the value is no code of [0, K)
  double* s;              // [>= n] sample weight, 0 where y == K
  int* counts;            // [K] rows per class
  double* info;           // [4]: n_valid, classes present, S = sum of s, unused
  int64_t ldk;
  int n, n_cont, n_cat, D, K;
  const int* card;        // [n_cat]
  const int* offs;        // [n_cat + 1] first one-hot feature of a column, less n_cont; offs[n_cat] = D - 1 - n_cont
};
struct UtilPackArgs {
  const double* values;   // [rows, n_cols] decoded table, row-major
  int n_cols;
  const int* kind;        // [n_cols] UtilKind
  const int* slot;        // [n_cols] column of cont / row of cat_t
  const double* mean;     // [n_cont]
  const double* sd;       // [n_cont] (> 0)
  UtilTable t;
};
void launch_util_pack(const UtilPackArgs& a, hipStream_t stream);
// M [D, D] = (F^T diag(s) F / 2 + diag(reg)) / S, reg = 1 but for the intercept's 0; part: [groups, D, D]
void launch_util_gram(const UtilTable& t, double* M, double* part, hipStream_t stream);
// Minv = (M + 1e-10 trace(M) / D I)^-1 through the Cholesky factor; Lt, X: [D, D] scratch
void launch_util_factor(const double* M, int D, double* Lt, double* X, double* Minv, hipStream_t stream);
// G [D, K] = grad f(P), loss[0] = f(P); part: [groups, D, K], lossp: [groups]
void launch_util_grad(const UtilTable& t, const double* P, double* G, double* loss, double* part, double* lossp,
                      hipStream_t stream);
// W' = V - Minv G; V' = W' + beta (W' - W)
void launch_util_update(double* V, double* W, const double* Minv, const double* G, int D, int K, double beta,
                        hipStream_t stream);
// conf [K, K] int32 of the rows of t under weights W (classes with train_counts == 0 are never predicted);
// out[0..7] = f1, acc, real[0], real[1], real[0] - f1, real[1] - acc, loss[0], max |G|
void launch_util_predict(const UtilTable& t, const int* train_counts, const double* W, int* conf, const double* G,
                         const double* loss, const double* real, double* out, hipStream_t stream);

// MLP-utility evaluator (kernels/mlp.hip): a one-hidden-layer network h = relu(F W1), z = [h | 1] W2 trained on a packed
// table (UtilTable, unweighted: only y and counts are read) by a fixed number of Adam steps over strided batches, its
// loss and its confusion matrix on held-out rows (eval/mlp_device.py has the definition).  All fp64; every sum has an
// order fixed by the shapes alone, counting is in integers; no floating-point atomics, no allocation, no host round
// trip.  The limits: a block of 64 rows keeps its h [64, H] (65 KiB at the limit) and its logits [64, K] (33 KiB) in
// LDS, one workgroup per CU; a batch is at most 16 such blocks.
constexpr int MLP_MAX_HIDDEN = 128;         // H
constexpr int MLP_MAX_BATCH = 1024;         // rows of a batch
constexpr int MLP_MAX_STEPS = 10000;        // steps of a fit (the evaluator's limit: two graph nodes each)
constexpr int MLP_ROWS = 64;                // rows of a block
// theta = [W1 [D, H] | W2 [H + 1, K]] flat, the last rows the biases; mom / var: Adam's moments, the same shape
struct MlpStepArgs {
  UtilTable t;
  int b, nb;              // the batch: rows b, b + nb, b + 2 nb, ... < t.n
  int H;
  double* theta;
  double* mom;
  double* var;
  double* h;              // [rows of the batch, H]
  double* dz;             // [rows of the batch, K]
  double* dh;             // [rows of the batch, H]
  int* cnt;               // [row blocks of the batch] valid rows
  double alpha, lr_t;     // L2 penalty; lr sqrt(1 - 0.999^t) / (1 - 0.9^t)
};
inline int mlp_batch_rows(int64_t n, int64_t b, int64_t nb) { return (int)((n - b + nb - 1) / nb); }
// one Adam step on the batch: forward / backward over its row blocks, then one gradient tile + Adam per wave
void launch_mlp_step(const MlpStepArgs& a, hipStream_t stream);
// loss[0] = (sum over the valid rows of CE + alpha / 2 |W1, W2 without their bias rows|^2) / max(valid rows, 1);
// loss[1 ..] : the row blocks' partial sums (scratch, ceil(n / 64) of them)
void launch_mlp_loss(const UtilTable& t, const double* theta, int H, double alpha, double* loss, hipStream_t stream);
// conf [K, K] int32 of the rows of t (classes with train_counts == 0 are never predicted);
// out[0..6] = f1, acc, real[0], real[1], real[0] - f1, real[1] - acc, loss[0]
void launch_mlp_predict(const UtilTable& t, const int* train_counts, const double* theta, int H, int* conf,
                        const double* loss, const double* real, double* out, hipStream_t stream);

// Tree-utility evaluator (kernels/forest.hip): a histogram decision tree and a random forest fitted on the binned
// decoded table, and their confusion matrices on held-out rows (eval/forest_device.py has the definition).  Counting
// is in integers, the criterion is fp64 in a fixed order without contraction, so a fit is bit-identical on every run.
// The limits: a bin is one byte; the [bins, K] uint32 histogram of one (node, feature) lives in LDS (64 KiB at both
// limits, against 160 KiB per CU); heap indices below 2^21 fit the Philox counter word they key.
constexpr int TREE_MAX_BINS = 256;          // bins of a feature, the overflow / NaN bin of a categorical one included
constexpr int TREE_MAX_CLASSES = 64;        // K: categories of the target column
constexpr int TREE_MAX_DEPTH = 20;
constexpr int TREE_MAX_FEATURES = 1024;     // per-feature candidates of a node in LDS (20 B each)
enum TreeKind : int { TREE_CONT = 0, TREE_CAT = 1, TREE_TARGET = 2 };
unsigned check_status_forest();
// a binned table
struct TreeTable {
  uint8_t* bins;          // [F, ld] feature-major
  int* y;                 // [>= n] target code, K where the value is no code of [0, K)
  int* counts;            // [K] valid rows per class
  double* cw;             // [K] balanced class weights, 0 for an absent class
  int64_t ld;
  int n, F, K;
};
struct TreePackArgs {
  const double* values;   // [n, n_cols] decoded table, row-major
  int n_cols;
  const int* kind;        // [n_cols] TreeKind
  const int* slot;        // [n_cols] feature index
  const int* card;        // [F] categories of a categorical feature (0 for a continuous one)
  const double* edges;    // ascending distinct edges of the continuous features
  const int* eoff;        // [F + 1] a feature's edges are edges[eoff[f] .. eoff[f + 1])
  int n_edges;
  TreeTable t;
};
void launch_tree_pack(const TreePackArgs& a, hipStream_t stream);
// mult [T, ldr]: 1 per row, or (bootstrap) how often tree t drew the row among its n draws
void launch_tree_bootstrap(int* mult, int T, int64_t ldr, int n, int bootstrap, uint64_t seed, hipStream_t stream);
// the trees of one model and the scratch of their growth
struct TreeGrowArgs {
  TreeTable t;
  const int* nbins;       // [F] bins of a feature (< 2: never a candidate)
  const int* mult;        // [T, ldr]
  int* rows;              // [2, T, ldr] ping-pong row lists: a node's rows are a segment, in ascending row order
  int* feature;           // [T, cap] -1 for a leaf
  int* bin;               // [T, cap]
  int* left;              // [T, cap] the right child is left + 1
  int* heap;              // [T, cap] root 1, children 2 g and 2 g + 1; 0 for an unused slot
  int* counts;            // [T, cap, K] class counts, multiplicities included
  int* seg;               // [T, cap, 2] first entry and length of a node's segment
  int* level;             // [T, 4] first node and nodes of the current level, nodes of the tree
  int* lcounts;           // [T, lvl_cap, K] class counts of the left child of a level's split nodes
  int64_t ldr;
  int T, cap, lvl_cap, max_depth, min_leaf, m_feat, hist_bytes;
  uint64_t seed;
};
void launch_tree_grow(const TreeGrowArgs& a, hipStream_t stream);
struct TreePredictArgs {
  TreeTable t;            // the held-out rows (cw: the training table's)
  const int* feature;
  const int* bin;
  const int* left;
  const int* counts;
  int T, cap, soft;
  int* conf;              // [K, K]
};
void launch_tree_predict(const TreePredictArgs& a, hipStream_t stream);
// out[0..5] = f1, acc, real[0], real[1], real[0] - f1, real[1] - acc
void launch_tree_scores(const int* conf, int K, const double* real, double* out, hipStream_t stream);

struct GenWeightJob {
  const float* w;   // fp32 weight, element (n, k) at w[n * ldw + k * skw] (skw = 1: [N, K] rows; ldw = 1: input-major storage)
  int N, ldw, skw, kd, C;
  uint16_t* w16;    // [N, ld16] bf16: columns [0, kd)
  int ld16;
  float* wt;        // [C, N] fp32: columns [kd, kd + C) transposed
};
struct GenWeightPrep {
  GenWeightJob jobs[4];
  int n_jobs;
};
void launch_gen_weight_prep(const GenWeightPrep& a, hipStream_t stream);

// VGM encode (kernels/vgm.hip): one thread per (row, column) cell of the label-encoded table
struct VgmEncodeArgs {
  const double* x;      // label codes / continuous values: x[r * ldx + j * ldc] (row- or column-major)
  int ldx, n_rows, n_cols;
  int64_t ldc;
  float* out;           // [n_rows, ldo] encoded matrix (zero-filled by the caller)
  int ldo;
  int* opt;             // [n_rows, n_span] option index per conditional span
  int n_span;
  const int* col_kind;  // 0 continuous, 1 categorical
  const int* col_pos;   // output column of the alpha / first one-hot slot
  const int* col_aux;   // continuous: bank row; categorical: LUT offset
  const int* col_span;  // conditional span of the column's one-hot
  const int* col_lut_n; // categorical: LUT length (codes are clamped into it)
  const float* consts;  // [n_cont, 10] constant part of the weighted log prob
  const float* means;   // [n_cont, 10]
  const float* prec;    // [n_cont, 10] precision Cholesky (1 / sigma)
  const float* stds;    // [n_cont, 10]
  const int* vrank;     // [n_cont, 10] position among the valid modes, -1 if invalid
  const int* lut;       // categorical code -> option position
  uint64_t seed;
  uint32_t stream;
};
void launch_vgm_encode(const VgmEncodeArgs& a, hipStream_t stream);

// init_ops.hip: the federator's pooled GMM sample (segment s = (column, client, component) covers pool elements
// [seg_off[s], seg_off[s + 1]); element e = mean[s] + sd[s] * N(0, 1) keyed on (seed, e))
struct PoolSampleArgs {
  double* pool;
  const int64_t* seg_off;   // [nseg + 1]
  const double* mean;       // [nseg]
  const double* sd;         // [nseg]
  int nseg;
  int64_t n;
  uint64_t seed;
};
void launch_pool_sample(const PoolSampleArgs& a, hipStream_t stream);
// init_ops.hip: rows of a contiguous fp64 x [rows, n] centred in place; shift[row] = the row's mean
void launch_row_center(double* x, double* shift, int rows, int64_t n, hipStream_t stream);
// init_ops.hip: CSR real-row lists of an option matrix opt [n, n_col] (row-major, ldo): rows[s * n + ...] holds,
// for every span s and option o < width[s], the rows with that option in ascending order starting at offset[s, o];
// count[s, o] their number (offset / count 0 on padding slots o >= width[s]).  part: [n_col, chunks, maxw] scratch.
struct CsrArgs {
  const int* opt;
  int ldo;
  const int* width;
  int n, n_col, maxw, chunk, chunks;
  int* part;
  int64_t* count;
  int64_t* offset;
  int64_t* rows;
};
void launch_csr_rows(const CsrArgs& a, hipStream_t stream);

// Batched 1-D DP-GMM fit passes (kernels/vgm_fit.hip)
struct VgmFitArgs {
  const double* x;       // [n_cols, ldx] centred column data (row r valid for r < n_rows[col])
  int ldx, n_cols, max_rows, rows_per_block;
  const int* n_rows;     // [n_cols]
  const double* consts;  // [n_cols, 10] E-step: constant part of the weighted log prob
  const double* means;   // [n_cols, 10] E-step: posterior means; k-means: centres
  const double* prec;    // [n_cols, 10] E-step: precision Cholesky
  double* partial;       // [n_cols, chunks, 31] (E-step) or [n_cols, chunks, 30] (k-means)
};
void launch_vgm_estep(const VgmFitArgs& a, hipStream_t stream);
void launch_kmeans_step(const VgmFitArgs& a, hipStream_t stream);

// The whole fit of every column, one workgroup per column (kernels/vgm_fit.hip)
struct VgmFitAllArgs {
  const double* x;            // [n_cols, ldx] centred column data
  int ldx, n_cols;
  const int* n_rows;          // [n_cols]
  const double* init_centers; // [n_cols, 10] k-means centres to start from, or null (k-means++ + Lloyd)
  uint64_t seed;
  double wprior, tol, reg_covar;
  int max_iter, km_iter;
  double* out;                // [n_cols, 6, 10]: stick a, stick b, beta, means, dof, covariances
  int* info;                  // [n_cols, 2]: EM iterations, converged (-1: a cluster barrier timed out)
  double* lower_bound;        // [n_cols]
  // Split fit (split = G > 1 workgroups per column): every workgroup of a column seeds, runs Lloyd and the
  // M-steps on the whole column as before, but each E-step pass covers 1/G of the rows and the G partial records
  // meet through xpart [n_cols, 2, G, 32] (double-buffered by iteration) behind an arrival counter per column
  // (sync [n_cols * 32], zeroed by the caller).  split <= 1: one workgroup per column.
  int split;
  double* xpart;
  unsigned* sync;
};
// workgroups per column for a fit of n_cols columns of <= max_rows rows (set_tuning("vgm_split"): 0 = auto,
// 1 = one workgroup per column, n = n, capped by what the device holds at once)
int vgm_fit_split(int n_cols, int max_rows);
extern int g_vgm_split;
void launch_vgm_fit(const VgmFitAllArgs& a, hipStream_t stream);

}  // namespace fedtgan
