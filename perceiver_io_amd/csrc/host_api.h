// The interface between the host binding (binding.cpp, compiled by g++ with the torch headers)
// and the kernel translation units (*.hip, compiled by hipcc without them): every struct and
// constant that crosses that boundary and the prototype of every function the binding calls,
// one definition each, seen verbatim by both compilers (common.h includes this file).
// Plain C++17: no __device__ code, no builtins.
#pragma once
#include <stdint.h>

#include <hip/hip_runtime_api.h>

namespace pio {

// ---- structs passed by value to kernels ---------------------------------------------------
// (their names, field order and field types are part of the kernels' mangled names and kernarg
// layouts)

struct AttnArgs {
  const uint16_t* q; long long q_bs; int q_rs;
  const uint16_t* k; long long k_bs; int k_rs;
  const uint16_t* v; long long v_bs; int v_rs;
  const uint8_t* kmask;  // (B, Nk), nonzero = padding key; may be null
  int B, H, Nq, Nk;
  float scale_log2;      // softmax scale * log2(e)
  float scale;           // softmax scale (backward)
  uint32_t drop_thresh;  // dropout probability * 2^32 (0 = off)
  float drop_scale;      // 1 / (1 - p)
  const int64_t* seedp;  // device seed of the call (DropCfg); read only when drop_thresh
  uint32_t site;
};

// Dropout configuration of one fused call.  The 64-bit seed lives in DEVICE memory: it is
// drawn per forward call by torch's graph-safe generator (a 1-element randint on the step's
// stream), so a replayed hipGraph reads a fresh seed every step instead of a value frozen at
// capture time, and the backward regenerates the forward's masks from the same tensor.
// ``site`` separates the masks of one call: sub-stream 0 = residual after attention,
// 1 = residual after the MLP, 2 = attention probabilities (reference model.py:47-56, 66-71).
struct DropCfg {
  const int64_t* seed;  // nullptr or thresh == 0: dropout off
  uint32_t site;
  uint32_t thresh;      // p · 2^32
  float scale;          // 1 / (1 - p)
};

// A parameter-gradient slab reduction (common.h slab_reduce_block): dst_j[k] += Σ_s
// slab[s][off_j + k] over the rows of an (S, P) fp32 slab, P and every off_j multiples of 4.
constexpr int kMaxSlabSegs = 16;
// columns per workgroup of a non-deterministic SlabJob (256 threads × 4)
constexpr int kSlabColsPerBlock = 1024;
struct SlabJob {
  const float* slab;  // nullptr: no job
  int S, P, nbx, nblk;
  int det;            // deterministic mode: one block per column range sums ALL rows, plain add
  int n;
  float* dst[kMaxSlabSegs];
  int off[kMaxSlabSegs];
  int len[kMaxSlabSegs];
  // side job of the kernel that carries this struct: clear zero_n4 float4s at zero_p (the
  // accumulator of the NEXT kernel, e.g. the attention backward's atomic dQ), one slice per
  // workgroup — no separate fill launch on the chain
  float* zero_p;
  long long zero_n4;
};
// blocks of the gradient sum-of-squares pass: one fp32 partial each (optim.hip sumsq_kernel)
constexpr int kSumsqBlocks = 512;

// fp32 gradient targets of the post-attention block (views of the flat gradient buffer).
// Two sinks for a workgroup's parameter-gradient partials:
//  * atomic (slab = 0): targets may be replicated: workgroup i adds into replica
//    i % kGradReplicas, vrs floats apart (vrs = 0: one copy), folded once per step;
//  * slab (slab = 1): workgroup i STORES its partials into row i of a (tiles, P) fp32 slab
//    (vrs = P floats per row).  Float atomics execute at the memory side at ≈1.3 TB/s
//    chip-wide, so 256 tiles × 50 KB of partials per kernel cost ≈10 µs of a ≈25 µs kernel;
//    plain stores cost ≈0.3 µs per CU, and the slab rows are summed by a SlabJob.
constexpr int kGradReplicas = 8;
struct PostAttnGrads {
  float *dWo, *dbo, *dg2, *dbe2, *dW1, *db1, *dW2, *db2;
  int vrs;
  int slab;
};

// Fourier-PE split input (SURVEY K-03): logical row r = pe[r mod M] (row stride pe_rs, a
// multiple of 8, with npix leading zero columns and zero padding past Kin) + the npix pixel
// values of row r in those leading columns.  The (B, M, npix + C_pe) concatenation is never
// materialised; the PE table stays L2/MALL-resident across the batch.  With idx given (sparse
// images: the LArTPC events' non-zero pixels, models/lartpc.py) row r reads pe[idx[r]] instead
// (clamped into the table), so the gathered [pixel ‖ PE] rows are not materialised either.
struct PeSplit {
  const float* pe;  // nullptr: a plain input
  int pe_rs, M, npix;
  const long long* idx;
};

struct PeGradTargets {
  float *dWa, *dWb, *db, *dg, *dbeta;  // dW rows [0, Ch) / [Ch, O) (kin columns each); any may be null
};

}  // namespace pio

#include "pe_args.h"
#include "persist_args.h"
#include "sb_args.h"

namespace pio {

// ---- arguments of the row-tile (rowgemm.hip) and chain (chain.hip) launchers ----------------
// Host side only: the launchers unpack them into the kernels' own parameter lists.

// rows of a 2-D operand: fp32 or bf16 elements, rs elements from one row to the next
template <typename V>
struct RowsT {
  V* p;
  bool bf16;
  int rs;
};
using RowsIn = RowsT<const void>;
using RowsOut = RowsT<void>;

// the post-attention block's parameters (reference model.py:36-44): y = Wo·O + bo + x,
// z = y + W2·GELU(W1·LN2(y) + b1) + b2; weights bf16 (nn.Linear layout), the rest fp32.
// The backward launchers read Wo, W1, W2, g2 and be2 only.
struct PostAttnParams {
  const uint16_t* Wo; const float* bo;
  const float *g2, *be2; float eps;
  const uint16_t* W1; const float* b1;
  const uint16_t* W2; const float* b2;
};
// what the post-attention forward saves (written) and its backward reads: y, LN2's row
// statistics and the MLP pre-activation
struct PostAttnSaved {
  float *Ysave, *mean2, *rstd2;
  uint16_t* Usave;
};
// LN1 + projection of the NEXT layer, formed from the same row tile: QKVn = LN(z)·Wqᵀ + bq.
// Forward: QKVn (bf16 rows), mean1, rstd1 are written.  Backward (the gradient of QKVn comes
// in): lnw, lnb, Wq, mean1, rstd1 and nq are read, bq and QKVn unused.
struct NextProj {
  const float *lnw, *lnb;
  const uint16_t* Wq;  // bf16 [nq][C]; forward: nullptr = none
  const float* bq;
  uint16_t* QKVn;
  float *mean1, *rstd1;
  int nq;              // rows of Wq: C (a query projection), 2C (packed K | V) or 3C (packed QKV)
};
// the self-attention backward of the layer below, fused into the chain boundary kernel (N = 64
// latents per sample, the tile is the sample): its packed QKV rows (R, 3C) bf16 and LSE (R, H)
// in, its dQKV (R, 3C) bf16 out.  out = nullptr: not fused.
struct FusedAttnBwd {
  const uint16_t* qkv;
  const float* lse;
  uint16_t* out;
  float scale;
};
// a (B, N, ≥ H·D) fp32 view with unit inner stride
struct Rows3 {
  float* p;
  long long bs;
  int rs;
};

// Y = act(LN(X)·Wᵀ + bias) (+ res); lnw = nullptr: no LayerNorm
struct LnLinearFwdArgs {
  RowsIn X;                     // (R, Kin); with ps.pe: the (R, npix) pixel channels
  int R, Kin;
  const float *lnw, *lnb;
  float eps;
  const uint16_t* W; int w_rs;  // bf16 (N, w_rs ≥ Kin)
  const float* bias;
  int N, act;
  const float* res; int res_rs;
  RowsOut Y;
  float *mean, *rstd;           // LN row statistics out (nullptr: not saved)
  PeSplit ps;
};
// dX = LN_bwd(G·W) (+ dres); dlnw / dlnb / dW / db partials into replicas or a slab (see
// PostAttnGrads: vrs for the vectors, wrs for dW); any target may be null
struct LnLinearBwdArgs {
  RowsIn G; int N;              // (R, N)
  const uint16_t* W; int w_rs, Kin;
  RowsIn X;
  const float *mean, *rstd, *lnw, *lnb;
  const float* dres; int dres_rs;
  float* dX; int dx_rs;         // may alias dres (same row stride)
  float *dlnw, *dlnb, *dW, *db;
  int vrs, wrs, slab;
  int R;
  PeSplit ps;
  SlabJob job;                  // the previous kernel's slab reduction, in appended workgroups
};
// The text encoder's input pass (rowgemm.hip text_kv_fwd / text_kv_bwd): both cross layers'
// LayerNorm + K|V projection of the embedded token rows, 64 channels → 2·64 columns per layer.
// one layer's LN affine (fp32), bf16 K|V weight (128, 64), bias (128) and its bf16 (R, 128) output
struct TextKvProj {
  const float *lnw, *lnb;
  const uint16_t* W;
  const float* bias;
  uint16_t* KV;
};
// x = E[ids]·scale + P[r mod L] (fp32 (R, 64), V table rows), its LN row statistics, both K|V
struct TextKvFwdArgs {
  const int64_t* ids;
  const float *E, *P;
  float scale;
  long long V;
  int L, R;
  float eps;
  TextKvProj a, b;
  float *X, *mean, *rstd;
};
// one layer's accumulated dK|dV (fp32 (R, 128)), LN affine, weight and gradient targets
struct TextKvGrad {
  const float* G;
  const float *lnw, *lnb;
  const uint16_t* W;
  float *dlnw, *dlnb, *dW, *db;
};
// dX = LN_bwd(G_a·W_a∘γ_a + G_b·W_b∘γ_b); the parameter-gradient partials of both layers into
// replicas or one slab (vrs: the shared replica / slab row stride)
struct TextKvBwdArgs {
  TextKvGrad a, b;
  const float *X, *mean, *rstd;
  float* dX;
  int vrs, slab, R;
  SlabJob job;                  // the previous kernel's slab reduction, in appended workgroups
};
// dW (+)= Gᵀ·A', db (+)= Σ rows G; amode: A' = A (0) | LN(A) (1) | GELU(A) (2)
struct WgradArgs {
  RowsIn G; int N;
  RowsIn A; int Kin, amode;
  const float *mean, *rstd, *lnw, *lnb;
  int R;
  int rows_per_wg;              // ≤ 0: pick the split so that the launch has ≈ 512 workgroups
  float *dW, *db;
  int vrs, wrs;
  PeSplit ps;
};
// the post-attention block over R rows: O (R, C) bf16 the attention output, X (Rx, C) the
// residual rows (row r adds X[r % Rx]), Z (R, C) out.  next: post_attn_ln_linear_fwd_launch only.
struct PostAttnFwdArgs {
  const uint16_t* O;
  const float* X;
  PostAttnParams p;
  float* Z;
  PostAttnSaved s;
  int R, Rx;
  NextProj next;
  DropCfg dr;
};
// one latent self-attention layer (C = 64, H = 4) over R = B·N rows: attention over the packed
// QKV (R, 3C) bf16 (O, LSE out), the post-attention block, then the next layer's projection
struct SaLayerFwdArgs {
  const uint16_t* QKV;
  int N;
  float scale_log2;
  uint16_t* O;
  float* LSE;
  const float* X;
  PostAttnParams p;
  float* Z;
  PostAttnSaved s;
  int R;
  NextProj next;
  DropCfg dr;
};
// post-attention backward: dZ (R, C) in; dY (R, C), dO (R, C) bf16 and delta (R, H) =
// per-head rowsum(dO∘O) out
struct PostAttnBwdArgs {
  const float* dZ;              // the fused form (LnLinearPostAttnBwdArgs) forms it in registers: unused
  PostAttnSaved s;
  const uint16_t* O;
  PostAttnParams p;
  float* dY;
  uint16_t* dO;
  float* delta;
  int H;
  PostAttnGrads grads;
  int R;
  SlabJob job;
  DropCfg dr;
};
// layer boundary l+1 → l, backward: the LN1 + projection backward of layer l+1 (G the gradient
// of next.QKVn, dres the other gradient of z_l) feeds the post-attention backward of layer l
struct LnLinearPostAttnBwdArgs {
  const void* G; bool g_bf16;   // (R, next.nq) fp32, or bf16 (the chain kernel only)
  NextProj next;
  const float* X;               // z_l (R, C): the LN1 input
  const float* dres;
  float *dlnw, *dlnb, *dWq, *dbq;
  PostAttnBwdArgs pa;
  FusedAttnBwd att;             // with att.out, pa.dO / pa.delta are not written
};
struct AttnBwdArgs {
  AttnArgs a;
  const uint16_t *O, *dO;       // (B, Nq, H·D) bf16 contiguous
  const float* LSE;
  float* delta;                 // (B, Nq, H) rowsum(dO∘O): written when compute_delta, else read
  Rows3 dq, dk, dv;             // dq needs no zero fill from the caller
  bool compute_delta, kv_acc;
  long long dq_kbs;             // > 0 (deterministic mode): dq slice per key block, plain stores
  int qsplit_ok;
  int dq_zeroed;                // attn_bwd_zero_plan bits the caller has already cleared
};

// ---- arguments of the vocabulary heads (ce_head.hip, mlm_head.hip, soft_ce_head.hip, topk_head.hip)
// W (V, C) bf16 and bias (V) fp32 throughout.
// mean CE over the M rows with a label >= 0; row r = H[hidx[r]] (hidx null: H[r]) of the fp32 H
struct CeFwdArgs {
  int C, M, V;
  const float* H; const int64_t* hidx;
  const int64_t* labels;
  const uint16_t* W; const float* bias;
  float *loss, *lse;            // the mean loss (1) and the rows' log-sum-exp (M)
  uint16_t* hs;                 // the compact bf16 rows (M, C) the backward reads
  float* count; int count_labels;  // the mean's denominator: read, or (count_labels) counted and written
  // workspace, sized by ce_fwd_plan
  int nsplit;
  float* part_ml;               // (nsplit, M, 2) the splits' (max, sum)
  float* part_acc;              // (nsplit, M, C) the splits' Σ p·W (plan.acc), kept for the backward
  float *picked, *blk;          // (M), (2·plan.nblk)
  unsigned *ticket, *rb_tickets;  // one zeroed word, plan.rb_tickets zeroed words: re-armed by the kernels
  float* zero_out; long long zero_n;  // cleared on the way (null: nothing); 16-byte aligned, zero_n % 4 == 0
};
struct CeFwdPlan {
  int nsplit;      // vocab splits
  bool acc;        // the two-pass head (C = 64): part_acc exists and goes to the backward with part_ml
  int nblk;        // block partials of the loss
  int rb_tickets;  // row-block arrival counters needed (0: none)
};
// dH[rowmap[r]] (rowmap null: dH[r]) += the row gradients, dW / db (+)= the parameter gradients of
// the mean loss's gradient gout; hs, lse, count (and part_acc / part_ml, nsplit at C = 64) from the forward
struct CeBwdArgs {
  int C, M, V;
  const uint16_t* hs;
  const int64_t* labels;
  const uint16_t* W; const float* bias;
  const float *lse, *gout, *count;
  const float *part_acc, *part_ml; int nsplit;
  float* dH; long long dh_rows; const int64_t* rowmap;
  float *dW, *db; int accumulate;
  float* slab;                  // (ce_bwd_slab_rows, V·C + V₄) dW | db partials stored, not added; or null
  int det;                      // deterministic mode: the generic head's dH pass runs one vocab split
};
// the soft-target head, both directions.  Forward: H (M, C) fp32 in; lse, pred, hs, loss, count out,
// blk (2·soft_ce_row_tiles) scratch.  Backward: hs, lse, count, gout in; dH overwritten, dW / db
// overwritten or (accumulate) added to.
struct SoftCeArgs {
  int C, M, V;
  const uint16_t* W; const float* bias;
  const int64_t *la, *lb; const float* lam; float eps;
  const float* H;
  uint16_t* hs; float *lse, *count;
  int* pred; float *blk, *loss;
  const float* gout; float *dH, *dW, *db; int accumulate;
};
// the k largest logits of M rows (row r = H[hidx[r]], hidx null: H[r]; H has R rows): C ∈ {64, 128},
// 1 ≤ k ≤ 8, k ≤ V, M ≥ 1; nsplit = vocab_topk_splits, cand_v / cand_i hold nsplit·M·vocab_topk_kt(k)
// entries, part_ml nsplit·M·2
struct VocabTopkArgs {
  int C, M, V, k;
  const float* H; const int64_t* hidx; long long R;
  const uint16_t* W; const float* bias;
  int nsplit; float* cand_v; int* cand_i; float* part_ml;
  float* values; int64_t* indices; float* lse;
};

// ---- attention.hip ----
void attn_fwd_launch(const AttnArgs& a, int D, uint16_t* O, float* LSE, float* Opart, float* MLpart, int nsplit,
                     hipStream_t st);
void attn_combine_launch(const float* Opart, const float* MLpart, uint16_t* O, float* LSE, int nsplit, long long rows,
                         int D, hipStream_t st);
// which accumulators a (non-deterministic, non-accumulating) backward launch clears itself:
// bit 0 dQ (several key blocks add into it), bit 1 dK / dV (query splits add into them) — a
// caller that clears them on the way (a SlabJob zero span of the previous kernel) passes the
// same bits back as dq_zeroed
int attn_bwd_zero_plan(int B, int H, int Nq, int Nk, int D);
// key blocks of the backward grid (dQ partial slices in deterministic mode)
int attn_bwd_key_blocks(int Nk, int D);
void attn_bwd_launch(const AttnBwdArgs& b, int D, hipStream_t st);
// bf16 dQ / dK / dV (attn_bwd_kernel OBF): head width 16, one key block (Nk ≤ 256), no query
// split, more than 64 queries (the full-LDS variant), nothing to accumulate onto; false (nothing
// launched) when the shape does not qualify
bool attn_bwd_bf16_ok(const AttnArgs& a, int D);
// job: the previous kernel's slab reduction in z-slices appended past the batch.  Carrying one,
// the two-query-tile variant runs (≈ 70 KB of LDS: two workgroups per CU), so the reduction
// shares the CUs with the attention tiles instead of queueing behind a one-per-CU carrier's tiles.
bool attn_bwd_bf16_launch(const AttnArgs& a, int D, const uint16_t* dO, const float* LSE, const float* delta,
                          uint16_t* dq, long long dq_bs, int dq_rs, uint16_t* dk, long long dk_bs, int dk_rs,
                          uint16_t* dv, long long dv_bs, int dv_rs, const SlabJob& job, hipStream_t st);
// ---- attention_pe.hip ----
void attn_bwd_pe_launch(const PeBwdArgs& a0, int nkb, int bsplit, hipStream_t st);
// key splits of one launch: about one round of workgroups (2 per CU) of the factored kernel.  (A
// floor of 6 key chunks per split ran MNIST's forward 22.5 → 19.5 µs but moved the 4-sample
// 28×28 classifier test's decoder query-LN gradient — an ill-conditioned tensor — past its
// bf16 floor: not kept, profiles/r6_ab/README.md)
int attn_fwd_pe_auto_splits(int B, int H, int ncu);
// splits × 32-key chunks covering M keys; grid (batch groups, splits, heads), 4 waves each
void attn_fwd_pe_launch(const PeFwdArgs& a0, hipStream_t st);
// ---- attn_weights.hip ----
// query chunks of one launch (its grid.y) for this shape.  One chunk: the kernel stores the mass
// itself; several: per-chunk partials go to part (B, chunks, Nk) fp32 and a second launch adds them
// in chunk order.
int attn_weights_chunks(int B, int Nq, int Nk);
// head-averaged attention weights of a forward: a (q, k, kmask, B, H, Nq, Nk, scale_log2 read; v and
// the dropout fields unused), LSE (B, Nq, H) fp32 as attn_fwd wrote it.  avg (B, Nq, Nk) and / or mass
// (B, Nk) fp32, each may be null (both null: nothing is launched); part: see above, unused when
// nchunks == 1 or mass is null.  nchunks = attn_weights_chunks(B, Nq, Nk).
void attn_weights_launch(const AttnArgs& a, int D, const float* LSE, float* avg, float* mass, float* part, int nchunks,
                         hipStream_t st);
// ---- augment.hip ----
void batch_augment_launch(const uint8_t* src, const float* params, float* out, int B, int Hs, int Ws, int C, int oh,
                          int ow, const float* mean, const float* std, hipStream_t st);
unsigned check_errors_augment(bool reset);
// ---- ce_head.hip (the two-pass head, C = 64; called by mlm_head.hip's launchers) ----
// vocab splits of a (row blocks × vocab splits) grid: ≈ 512 workgroups (2 per CU), every split ≥ 4
// chunks, at most max_splits; rounded so that no split is left without a chunk
int vocab_splits(int M, int V, int rows_per_wg, int chunk, int max_splits);
CeFwdPlan ce2_fwd_plan(int M, int V);
int ce2_bwd_splits(int M, int V);
void ce2_fwd_launch(const CeFwdArgs& a, hipStream_t st);
void ce2_bwd_launch(const CeBwdArgs& a, hipStream_t st);
unsigned check_errors_ce_head(bool reset);
// ---- chain.hip (called by rowgemm.hip's launchers once the operands qualify: C = 64, H = 4,
// every pointer 16-byte aligned, R % 64 == 0) ----
bool sa_layer_fwd_chain_launch(const SaLayerFwdArgs& a, hipStream_t st);
bool ln_linear_post_attn_bwd_chain_launch(const LnLinearPostAttnBwdArgs& a, hipStream_t st);
// ---- elementwise.hip ----
void embed_fwd_launch(const int64_t* ids, const float* E, const float* P, float* out, long long rows, int L, int C,
                      float scale, long long V, hipStream_t st);
void embed_bwd_launch(const int64_t* ids, const float* g, float* dE, float* dP, int B, int L, int C, float scale,
                      hipStream_t st);
// C a multiple of 64 (≤ 256); dE and/or dP
// + the previous backward kernel's slab job in appended workgroups (small LDS: they share the CUs
// with the embedding blocks instead of running after them)
bool embed_bwd_local_launch(const int64_t* ids, const float* g, float* dE, float* dP, int B, int L, int C, float scale,
                            const SlabJob& job, hipStream_t st);
void embed_bwd_sorted_launch(const int64_t* sorted_ids, const int64_t* perm, const float* g, float* dE, long long n,
                             int C, float scale, hipStream_t st);
void text_mask_launch(const int64_t* x, const bool* pad, int64_t* state, int64_t* xm, int64_t* labels, long long n,
                      int unk_id, int mask_id, float p, int lo, uint32_t range, int advance, hipStream_t st);
// whole-word masking looks for a word's first token among this many positions (the token's own
// included); ops/emulation.py WORD_WINDOW is the same number
constexpr int kWordWindow = 16;
// x: (n / L, L) rows; cont: bit-packed continuation table over V ids, ⌈V / 32⌉ words
void text_mask_words_launch(const int64_t* x, const bool* pad, int64_t* state, const int32_t* cont, int64_t* xm,
                            int64_t* labels, long long n, int L, int V, int unk_id, int mask_id, float p, int lo,
                            uint32_t range, int advance, hipStream_t st);
void index_add_rows_launch(float* dst, long long nrows, const int64_t* idx, const float* src, long long R, int C,
                           hipStream_t st);
void gather_rows_launch(float* out, const float* src, long long nrows, const int64_t* idx, long long R, int C,
                        hipStream_t st);
void batch_sum2_launch(const float* a, const float* b, float* oa, float* ob, int B, long long na, long long nb, int acc_b,
                       hipStream_t st);
void slab_reduce_launch(const SlabJob& job, hipStream_t st);
void reduce_probe_launch(const float* x, float* out, hipStream_t st);
void cast_bf16_launch(const float* x, uint16_t* y, long long n, hipStream_t st);
int stage_step_launch(void* const* dst, const void* const* src, const long long* bytes, int nseg, float* hyper_dst,
                      const float* hyper, int nhyper, long long* seed_dst, const long long* seeds, int nseeds,
                      hipStream_t st);
unsigned check_errors_elementwise(bool reset);
// ---- ema.hip ----
// elements one pass of the capped grid covers (larger buffers take the grid-stride loop)
long long ema_pass_elems();
// e ← e + hyper[5]·(w − e) over n fp32 elements (nothing touched when hyper[5] == 0); ema, w
// 16-byte aligned and n % 4 == 0 (checked by the binding)
void ema_update_launch(float* ema, const float* w, long long n, const float* hyper, hipStream_t st);
// w ↔ ema in place, shadow (may be null) ← bf16(new w); 16-byte aligned (shadow 8), n % 4 == 0
void ema_swap_launch(float* w, float* ema, uint16_t* shadow, long long n, hipStream_t st);
// ---- health.hip ----
// the step guard (optim_common.h: the 8 guard words): judges Σ g² of sumsq's partials, one workgroup.
// guard: kGuardWords fp32, part: kSumsqBlocks fp32
void step_guard_launch(const float* part, const float* hyper, float* guard, float gscale, hipStream_t st);
// per-tensor gradient / weight statistics over the chunk table, when hyper[6] != 0 (→ stats) or the
// guard flags this step (→ skip_stats; guard and skip_stats may be null together): part (C, 4) fp32
// scratch, tensors (T, 2) int32 = (first chunk, chunks), stats / skip_stats (T, 4) fp32 =
// ‖g‖·gscale, ‖w‖, max|g|·gscale, non-finite gradient elements.  g, w 16-byte aligned.
void tensor_stats_launch(const float* g, const float* w, long long n, const float* hyper, const float* guard,
                         const long long* chunks, long long C, const int* tensors, int T, float gscale, float* part,
                         float* stats, float* skip_stats, hipStream_t st);
unsigned check_errors_health(bool reset);
// ---- lamb.hip ----
// elements per chunk of the chunk table (lamb_launch, adamw_grouped_launch): the extension's LAMB_CHUNK
int lamb_chunk_elems();
// p, g, m, v 16-byte aligned, shadow 8-byte aligned (checked by the binding); C chunks, T tensors;
// tgroup (T,) tensor → group with hyper of 8 + 4 G floats, or null: every tensor in group 0;
// guard: the step guard's words or null
void lamb_launch(float* p, float* g, float* m, float* v, uint16_t* shadow, long long n, const float* hyper,
                 const long long* chunks, long long C, const int* tensors, const float* topt, int T, float* partials,
                 float* trust, float eps, float clip, float gscale, int zero_g, const float* loss_src,
                 float* loss_ring, int ring_n, const float* norm_part, const int* tgroup, int G, const float* guard,
                 hipStream_t st);
// ---- lartpc_prep.hip ----
// event_compact: img (B, H, W) fp32, lab (B, H·W) uint8 and one dihedral code per sample in words
// (B) int32, all on the device → keys (values / index / kmask, kcap slots per sample), queries
// (qidx / qlab, qcap slots) and counts (B, 2) in the flat order of the transformed event.  wmask:
// bit c set when class c < ncls <= 8 is weighted.  H == W, H·W < 2^31; S in [1, 256] segments per
// sample, V in {4, 8} loads per thread and tile; segcount: (B, S, 2) int32 scratch (unused when
// S == 1)
struct EventCompactArgs {
  const float* img;
  const uint8_t* lab;
  const int* words;
  int B, H, W;
  long long kcap, qcap;
  unsigned wmask;
  int ncls;
  int S, V;
  int* segcount;
  float* values;
  int64_t* index;
  bool* kmask;
  int64_t* qidx;
  int64_t* qlab;
  int* counts;
};
void event_compact_launch(const EventCompactArgs& a, hipStream_t st);
unsigned check_errors_lartpc_prep(bool reset);
// ---- mlm_head.hip (the CE head's entry points; its own kernels are the generic head, C = 32 / 128;
// C = 64 goes to ce_head.hip) ----
CeFwdPlan ce_fwd_plan(int C, int M, int V);
// rows of the backward's slab (the row splits of its dW pass)
int ce_bwd_slab_rows(int C, int M, int V);
void ce_fwd_launch(const CeFwdArgs& a, hipStream_t st);
void ce_bwd_launch(const CeBwdArgs& a, hipStream_t st);
unsigned check_errors_mlm_head(bool reset);
// ---- mlm_select.hip ----
void mlm_select_launch(const int64_t* labels, int B, int L, int cap, int gcap, int64_t* idx_b, int64_t* lab_b,
                       int* count, int64_t* gidx, int64_t* glab, float* total, bool* overflow, bool* sticky,
                       const float* P, int C, float* q, hipStream_t st);
unsigned check_errors_mlm_select(bool reset);
// ---- optim.hip ----
void sumsq_launch(const float* g, long long n, float* part, hipStream_t st);
void adamw_launch(float* p, float* g, float* m, float* v, uint16_t* shadow, long long n, const float* hyper,
                  float eps, float wd, float clip, float gscale, int l2, int zero_g, const float* loss_src,
                  float* loss_ring, int ring_n, const float* norm_part, const float* guard, hipStream_t st);
// AdamW with per-group lr / weight decay / eps over the LAMB chunk table (chunks (C, 3) int64,
// tgroup (T,) int32 = tensor → group, hyper of 8 + 4 G floats); -1 for G outside [1, 8]
int adamw_grouped_launch(float* p, float* g, float* m, float* v, uint16_t* shadow, long long n, const float* hyper,
                         const long long* chunks, long long C, const int* tgroup, int T, int G, float clip, float gscale,
                         int l2, int zero_g, const float* loss_src, float* loss_ring, int ring_n,
                         const float* norm_part, const float* guard, hipStream_t st);
void fold_replicas_launch(float* grad, float* rep, long long n, int nrep, hipStream_t st);
unsigned check_errors_optim(bool reset);
// ---- pe_proj.hip ----
int pe_grad_splits(int M);
void pe_grads_launch(const uint16_t* E, const float* D, int M, int Kp, int O, const float* part, int nblk, float* slab,
                     float* Graw, float* tot, const float* Wa, const float* Wb, const float* g, const float* b, int Ch,
                     int kin, int nc, PeGradTargets t, hipStream_t st);
// C has Mst ≥ M rows; rows past M are written as zeros by the same launch
void pe_gemm_launch(const uint16_t* A, const uint16_t* Bw, void* C, bool bf16_out, int M, int N, int K, int Mst,
                    hipStream_t st);
void pe_weight_prep_launch(const float* W, const float* W2, int O1, const float* g, const float* b, const float* bias,
                           int O, int nc, int kin, int Kp, uint16_t* Wg, float* wpg, float* gw, float* bw, float* wt,
                           hipStream_t st);
void pe_proj_fwd_launch(const float* pix, int nc, const float* P, const float* pes, const float* pesq,
                        const float* wpg, const float* gw, const float* bw, long long R, int M, int O, int kin,
                        float eps, uint16_t* y, float* mean, float* rstd, hipStream_t st);
int pe_proj_bwd_blocks(int M);
void pe_proj_bwd_launch(const float* dy, const float* pix, int nc, const float* mean, const float* rstd, int B, int M,
                        int O, float* D, float* part, hipStream_t st);
// ---- persist.hip ----
void persist_set_spin_limit(unsigned n);
unsigned persist_errors(bool reset);
int persist_sync_words(int B);
bool sa_block_fwd_launch(const SABlockFwdArgs& a, hipStream_t st);
// ---- pixel_head.hip ----
int pixel_ce_blocks(long long R);
void pixel_ce_fwd_launch(int C, int K, const float* H, const float* W, const float* bias, const int64_t* labels,
                         const float* wts, long long R, float* part, float* stats, float* loss, hipStream_t st);
void pixel_ce_bwd_launch(int C, int K, const float* H, const float* W, const float* bias, const int64_t* labels,
                         const float* wts, const float* gout, const float* stats, long long R, float* dH, float* part,
                         float* dW, float* db, hipStream_t st);
// focal cross-entropy + soft Dice on the same row pass.  part: (pixel_ce_blocks(R), 4 + 5K) forward,
// (pixel_ce_blocks(R), K·C + K) backward, zero-filled by the caller when R == 0; stats: 6 + 7K floats
void pixel_seg_fwd_launch(int C, int K, const float* H, const float* W, const float* bias, const int64_t* labels,
                          const float* wts, float gamma, float ce_weight, float dice_weight, float eps, long long R,
                          float* part, float* stats, float* loss, hipStream_t st);
void pixel_seg_bwd_launch(int C, int K, const float* H, const float* W, const float* bias, const int64_t* labels,
                          const float* wts, float gamma, float ce_weight, float dice_weight, float eps,
                          const float* gout, const float* stats, long long R, float* dH, float* part, float* dW,
                          float* db, hipStream_t st);
// cpart: (pixel_ce_blocks(R), K·K) int32 when labels are given, else nullptr; cmap (R / Q, npix) is
// zero-filled by the caller before this launch
void pixel_predict_launch(int C, int K, const float* H, const float* W, const float* bias, const int64_t* qidx,
                          const bool* qvalid, const int64_t* labels, long long R, long long Q, long long npix,
                          uint8_t* classes, float* conf, uint8_t* cmap, int* cpart, hipStream_t st);
// S in [1, 256] segments per sample, V in {4, 8} loads per thread and tile; segcount: (B, S) int32
// scratch (unused when S == 1)
void nonzero_compact_launch(const float* img, int B, long long npix, long long cap, int S, int V, int* segcount,
                            float* values, int64_t* index, bool* kmask, int* count, hipStream_t st);
unsigned check_errors_pixel_head(bool reset);
// ---- randaugment.hip ----
// N layers of words (B, N, 8) over src (B, H, W, C), C ∈ {1, 3}; the result is written to out.
// tmp: a second image of src's size (unused when N == 1); hist: N·B·(C + 1)·256 int32, cleared on st
// by the caller before this call
void rand_augment_launch(const uint8_t* src, const float* words, uint8_t* out, uint8_t* tmp, int* hist, int B, int H,
                         int W, int C, int N, int fill, hipStream_t st);
unsigned check_errors_randaugment(bool reset);
// ---- rowgemm.hip ----
void ln_linear_fwd_launch(const LnLinearFwdArgs& a, hipStream_t st);
void post_attn_fwd_launch(const PostAttnFwdArgs& a, int C, hipStream_t st);
void post_attn_ln_linear_fwd_launch(const PostAttnFwdArgs& a, int C, hipStream_t st);
// fused self-attention layer forward (C = 64, H = 4): the chain kernel (chain.hip
// sa_layer_fwd_chain8_kernel); false (nothing launched) when the operands do not qualify (every
// pointer 16-byte aligned, N <= 512) — the binding turns that into an error
bool sa_layer_fwd_launch(const SaLayerFwdArgs& a, hipStream_t st);
void post_attn_bwd_launch(const PostAttnBwdArgs& a, int C, hipStream_t st);
// G: fp32, or (g_bf16) bf16 — taken by the chain-layout kernel only; returns false (nothing
// launched) for a bf16 G the chain kernel cannot take (the caller converts it to fp32)
bool ln_linear_post_attn_bwd_launch(const LnLinearPostAttnBwdArgs& a, int C, hipStream_t st);
void ln_linear_bwd_launch(const LnLinearBwdArgs& a, hipStream_t st);
void wgrad_launch(const WgradArgs& a, hipStream_t st);
// false (nothing launched) when an operand is not 16-byte aligned
bool text_kv_fwd_launch(const TextKvFwdArgs& a, hipStream_t st);
bool text_kv_bwd_launch(const TextKvBwdArgs& a, hipStream_t st);
unsigned check_errors_rowgemm(bool reset);
// ---- sample_block.hip ----
bool sb_fwd_launch(const SBFwdArgs& a, int C, hipStream_t st);
bool sb_bwd_launch(const SBBwdArgs& a, int C, hipStream_t st);
// rows per split: about 512 rows per workgroup (≥ 1 split; a multiple of 32)
// sj: a slab reduction (the sample-block backward's LayerNorm partials) run by appended workgroups
bool sb_wgrad_launch(SBWgradArgs a, int C, const SlabJob& sj, hipStream_t st);
// ---- soft_ce_head.hip ----
int soft_ce_row_tiles(int M);
void soft_ce_fwd_launch(const SoftCeArgs& a, hipStream_t st);
void soft_ce_bwd_launch(const SoftCeArgs& a, hipStream_t st);
void batch_mix_launch(const float* x, const int64_t* y, const float* mix, float* out, int64_t* yb, float* lam_out, int B,
                      int H, int W, int Ch, hipStream_t st);
unsigned check_errors_soft_ce_head(bool reset);
// ---- topk_head.hip ----
int vocab_topk_splits(int M, int V);
int vocab_topk_kt(int k);
void vocab_topk_launch(const VocabTopkArgs& a, hipStream_t st);
unsigned check_errors_topk_head(bool reset);

}  // namespace pio
