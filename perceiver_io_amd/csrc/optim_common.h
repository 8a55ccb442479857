// What the flat-space optimizer kernels share (optim.hip: AdamW; lamb.hip: LAMB): the chunk table,
// the step prologue, the clip factor and the per-element updates, one definition each.  Device code
// only.  Every function here is compiled under the flags of the translation unit that includes it:
// optim.hip takes the default -ffp-contract=fast, lamb.hip -ffp-contract=off (csrc/build.py
// PER_FILE_FLAGS), so an expression such as `norm + 1e-6f` below may round differently in the two.
// That is each family's own, fixed arithmetic; do not merge the translation units or force one mode.
#pragma once
#include "common.h"

namespace pio {

// ---- the chunk table -----------------------------------------------------------------------
// The flat buffers carry no tensor boundaries, so the host (ops/optim.py _cut_chunks) cuts every
// tensor range into chunks of at most kOptChunk elements, never across a tensor boundary, the
// padding between tensors in no chunk: chunks (C, 3) int64 = start element, length, tensor id.
// 256 threads × float4 walk a chunk.
constexpr int kOptChunk = 4096;                  // elements; the extension's LAMB_CHUNK = ops/optim.py LAMB_CHUNK
constexpr int kOptIter = kOptChunk / (4 * 256);  // float4 per thread of a full chunk
// words of `hyper`: 8 global ones, then 4 per parameter group (lr, weight decay, eps, reserved)
constexpr int kOptGroupBase = 8, kOptGroupWords = 4, kOptMaxGroups = 8;

struct OptChunk {
  long long start;
  int len, tid;
  bool ok;
};
// entry c of the table, validated against the buffers (the tables are built by the host once, but
// nothing here may write out of bounds: an entry that does not fit has ok = false and length 0)
__device__ __forceinline__ OptChunk opt_chunk(const long long* __restrict__ chunks, long long c, long long n, int T) {
  const long long* e = chunks + 3 * c;
  OptChunk k;
  k.start = e[0];
  const long long len = e[1], tid = e[2];
  k.ok = k.start >= 0 && (k.start & 3) == 0 && len >= 0 && len <= kOptChunk && k.start + len <= n && tid >= 0 &&
         tid < T;
  k.len = k.ok ? (int)len : 0;
  k.tid = k.ok ? (int)tid : 0;
  return k;
}

// ---- the step prologue ----------------------------------------------------------------------
// Σ g² of a step from sumsq_kernel's partials, in a fixed order (every block of every launch the same
// value): wave 0 sums the kSumsqBlocks partials, LDS broadcast.  At least 64 threads per block.
__device__ __forceinline__ float opt_sumsq_total(const float* __restrict__ part) {
  __shared__ float s_norm2;
  if (threadIdx.x < 64) {
    float t = 0.f;
#pragma unroll
    for (int k = 0; k < kSumsqBlocks / 64; ++k) t += part[threadIdx.x + 64 * k];
    t = wave_sum(t);
    if (threadIdx.x == 0) s_norm2 = t;
  }
  __syncthreads();
  return s_norm2;
}
// the clip factor of a step from that sum
__device__ __forceinline__ float opt_clip_scale(const float* __restrict__ part, float clip, float gscale) {
  const float norm = sqrtf(opt_sumsq_total(part)) * gscale;
  const float f = clip / (norm + 1e-6f);
  return f < 1.f ? f : 1.f;
}

// hyper[0] = lr, [1] = step (already incremented), [3] = beta1, [4] = beta2, [5] = 1 − EMA decay,
// [6] = "per-tensor statistics due this step" (non-zero: health.hip tensor_stats runs), [7] =
// loss-ring slot — read from device memory so schedulers can change them between replays of
// a captured step.
//
// guard (optional, null = off): the step guard's 8 fp32 words, owned by the optimizer and written by
// health.hip step_guard_kernel between sumsq and the update:
//   [0] skip flag of this step (1: Σ g² is not finite, the update must not happen)
//   [1] steps skipped so far, this one included        [2] consecutive skipped steps, ending here
//   [3] effective step = hyper[1] − steps skipped BEFORE this one: what the bias corrections take,
//       so a skipped step does not advance them (GradScaler's meaning of a skip)
//   [4] this step's gradient norm sqrt(Σ g²)·gscale (the mean gradient's, before clipping; inf / NaN
//       as it comes)                                    [5] the last finite such norm
//   [6] hyper[1] of the last skipped step (0: none)     [7] reserved
// The flag is one word that every block of every launch of the step reads: the decision is uniform.
constexpr int kGuardWords = 8;
__device__ __forceinline__ bool opt_guard_skip(const float* __restrict__ guard) {
  return guard != nullptr && guard[0] != 0.f;
}
__device__ __forceinline__ float opt_guard_step(const float* __restrict__ hyper, const float* __restrict__ guard) {
  return guard != nullptr ? guard[3] : hyper[1];
}
// a float that is inf or NaN, by its exponent bits (no fast-math flag can fold this away)
__device__ __forceinline__ bool opt_nonfinite(float x) { return (__float_as_uint(x) & 0x7f800000u) == 0x7f800000u; }

// loss_src (optional): the step's scalar loss, copied by thread 0 of block 0 into
// loss_ring[hyper[7] % ring_n] (the step engine hands that slot back as the step's loss: no
// separate copy launch per step) — on a skipped step too.
// gs: what a gradient element is multiplied by.  g holds the all-reduced SUM over ranks (gscale =
// 1 / world makes it the mean); with clip > 0 the threshold applies to the norm of the MEAN
// gradient, as in single-process training, from sumsq_kernel's per-block partials (norm_part).
// The bias corrections are each family's own (AdamW: 1 − powf, LAMB: lamb_bias_correction).
// skip (a guard that flags this step): the caller clears the gradient it would have consumed (if it
// clears gradients) and touches nothing else; step and gs are then meaningless.
struct OptStep {
  float step, beta1, beta2, gs;
  bool skip;
};
__device__ __forceinline__ OptStep opt_step(const float* __restrict__ hyper, float clip, float gscale,
                                            const float* __restrict__ loss_src, float* __restrict__ loss_ring,
                                            int ring_n, const float* __restrict__ norm_part,
                                            const float* __restrict__ guard) {
  OptStep s;
  s.step = opt_guard_step(hyper, guard);
  s.skip = opt_guard_skip(guard);
  s.beta1 = hyper[3];
  s.beta2 = hyper[4];
  if (loss_src != nullptr && blockIdx.x == 0 && threadIdx.x == 0) loss_ring[(int)hyper[7] % ring_n] = *loss_src;
  s.gs = gscale;
  if (clip > 0.f && !s.skip) s.gs *= opt_clip_scale(norm_part, clip, gscale);  // uniform over the launch
  return s;
}

// ---- per-element updates --------------------------------------------------------------------
// The AdamW update of one element — the definition every AdamW kernel calls (scalar, float4,
// grouped body and tail), so range, grouped and whole-buffer launches agree bit for bit.
// decay = fma(−wd, lr, 1), omb = 1 − β, step_size = lr / (1 − β1^t), bc2s = sqrt(1 − β2^t).
// l2 (torch.optim.Adam weight_decay): the decay joins the (clipped) gradient; else AdamW's
// decoupled decay of the weights.  Contraction is off inside: the fused multiply-adds are the
// explicit ones, whatever the translation unit's mode.
__device__ __forceinline__ void adamw_elem(float pi, float g0, float mi, float vi, float gs, float wd, float decay,
                                           float beta1, float omb1, float beta2, float omb2, float step_size, float bc2s,
                                           float eps, int l2, float& po, float& mo, float& vo) {
#pragma clang fp contract(off)
  const float gi = l2 ? fmaf(wd, pi, g0 * gs) : g0 * gs;
  if (!l2) pi *= decay;
  mo = fmaf(beta1, mi, omb1 * gi);
  vo = fmaf(beta2, vi, (omb2 * gi) * gi);
  po = pi - step_size * mo / (sqrtf(vo) / bc2s + eps);
}

// LAMB's moments of one element (lamb.hip, no contraction: every product and sum rounded on its own)
__device__ __forceinline__ void lamb_moments(float g0, float mi, float vi, float gs, float beta1, float beta2, float& mo,
                                             float& vo) {
  const float gi = g0 * gs;
  mo = beta1 * mi + (1.f - beta1) * gi;
  vo = beta2 * vi + (1.f - beta2) * gi * gi;
}

// LAMB's u of one element from the NEW moments and the OLD weight (both passes call exactly this)
__device__ __forceinline__ float lamb_u(float w, float m, float v, float bc1, float bc2s, float eps, float wd) {
  const float r = (m / bc1) / (sqrtf(v) / bc2s + eps);
  return fmaf(wd, w, r);
}

}  // namespace pio
