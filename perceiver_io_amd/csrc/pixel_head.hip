// Fused per-pixel classification head + class-weighted cross-entropy (SURVEY K-17).
//
// Reference: the LArTPC decoder output (B, H·W, C) → ClassificationOutputAdapter linear
// (C → K) → F.cross_entropy(weight = class weights, background 0) (run.py:105-112, 234-241),
// plus the per-class accuracies logged every step (run.py:190-206).  PyTorch runs that as a
// K = 3-column library GEMM (a pathological N for MFMA tiles), softmax, nll_loss and half a dozen
// reductions.  Here one pass reads each row once:
//   fwd: logits (16 lanes per row, C/16 channels per lane, DPP row sums), log-sum-exp, weighted
//        CE, argmax; per-block partial sums [Σw·ce, Σw, n(lab>0), hit(lab>0), (n_k, hit_k)…]
//   bwd: logits again, coef_k = w_lab · g/Σw · (softmax_k − [k = lab]),
//        dH = coefᵀ·W (written once), dW = Σ coef ⊗ h, db = Σ coef (per-block partials)
// Two one-block finalize kernels sum the partials in a fixed order (deterministic; no
// atomics): the loss / accuracies, and dW / db added into the parameter gradients.
//
// Inference (further down): pixel_predict — the same row pass writing class, confidence, the
// per-sample class map and an optional confusion count, and nonzero_compact — the device-side
// sparsifier that turns a dense image into the encoder's (values, index, kmask) operands.
#include "common.h"
#include "compact.h"

namespace pio {

__device__ __forceinline__ float row16_sum(float v) {
  v += dpp<0xB1>(v);   // quad_perm [1,0,3,2]
  v += dpp<0x4E>(v);   // quad_perm [2,3,0,1]
  v += dpp<0x124>(v);  // row_ror:4
  v += dpp<0x128>(v);  // row_ror:8
  return v;
}

constexpr int PH_ROWS = 16;  // rows per block iteration: 4 waves × 4 rows (16 lanes per row)

template <int CPL>
__device__ __forceinline__ void load_row(const float* p, float (&h)[CPL]) {
  if constexpr (CPL % 4 == 0) {
#pragma unroll
    for (int j = 0; j < CPL; j += 4) {
      const float4 v = *reinterpret_cast<const float4*>(p + j);
      h[j] = v.x; h[j + 1] = v.y; h[j + 2] = v.z; h[j + 3] = v.w;
    }
  } else {
#pragma unroll
    for (int j = 0; j < CPL; j += 2) {
      const float2 v = *reinterpret_cast<const float2*>(p + j);
      h[j] = v.x; h[j + 1] = v.y;
    }
  }
}

template <int C, int K>
__device__ __forceinline__ void row_logits(const float (&h)[C / 16], const float (&wk)[K][C / 16], const float (&bk)[K],
                                           float (&z)[K]) {
#pragma unroll
  for (int k = 0; k < K; ++k) {
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < C / 16; ++j) s = fmaf(h[j], wk[k][j], s);
    z[k] = row16_sum(s) + bk[k];
  }
}

template <int C, int K>
__global__ __launch_bounds__(256) void pixel_ce_fwd_kernel(const float* __restrict__ H, const float* __restrict__ W,
                                                           const float* __restrict__ bias,
                                                           const int64_t* __restrict__ labels,
                                                           const float* __restrict__ wts, long long R,
                                                           float* __restrict__ part) {
  constexpr int CPL = C / 16, NS = 4 + 2 * K;
  const int l = lane_id(), w = wave_id(), sub = l & 15, grp = l >> 4;
  float wk[K][CPL], bk[K];
#pragma unroll
  for (int k = 0; k < K; ++k) {
    load_row<CPL>(W + k * C + sub * CPL, wk[k]);
    bk[k] = bias[k];
  }
  float acc[NS];
#pragma unroll
  for (int s = 0; s < NS; ++s) acc[s] = 0.f;
  for (long long r = (long long)blockIdx.x * PH_ROWS + w * 4 + grp; r < R; r += (long long)gridDim.x * PH_ROWS) {
    float h[CPL], z[K];
    load_row<CPL>(H + r * C + sub * CPL, h);
    const long long lab64 = labels[r];
    row_logits<C, K>(h, wk, bk, z);
    const int lab = (lab64 >= 0 && lab64 < K) ? (int)lab64 : -1;
    float m = z[0];
    int pred = 0;
#pragma unroll
    for (int k = 1; k < K; ++k) {
      pred = z[k] > m ? k : pred;
      m = fmaxf(m, z[k]);
    }
    float se = 0.f, zl = 0.f, wl = 0.f;
#pragma unroll
    for (int k = 0; k < K; ++k) {
      se += __expf(z[k] - m);
      zl = k == lab ? z[k] : zl;
    }
    if (lab >= 0) wl = wts[lab];
    if (sub == 0 && lab >= 0) {
      const float ce = m + __logf(se) - zl;
      const float hit = pred == lab ? 1.f : 0.f;
      acc[0] += wl * ce;
      acc[1] += wl;
      if (lab > 0) {
        acc[2] += 1.f;
        acc[3] += hit;
      }
#pragma unroll
      for (int k = 0; k < K; ++k) {
        acc[4 + 2 * k] += k == lab ? 1.f : 0.f;
        acc[5 + 2 * k] += k == lab ? hit : 0.f;
      }
    }
  }
  __shared__ float sred[4][NS];
#pragma unroll
  for (int s = 0; s < NS; ++s) {
    const float v = wave_sum(acc[s]);
    if (l == 0) sred[w][s] = v;
  }
  __syncthreads();
  if (threadIdx.x < NS)
    part[(long long)blockIdx.x * NS + threadIdx.x] =
        sred[0][threadIdx.x] + sred[1][threadIdx.x] + sred[2][threadIdx.x] + sred[3][threadIdx.x];
}

template <int C, int K>
__global__ __launch_bounds__(256) void pixel_ce_bwd_kernel(const float* __restrict__ H, const float* __restrict__ W,
                                                           const float* __restrict__ bias,
                                                           const int64_t* __restrict__ labels,
                                                           const float* __restrict__ wts,
                                                           const float* __restrict__ gout,
                                                           const float* __restrict__ stats, long long R,
                                                           float* __restrict__ dH, float* __restrict__ part) {
  constexpr int CPL = C / 16, NP = K * C + K;
  const int l = lane_id(), w = wave_id(), sub = l & 15, grp = l >> 4;
  float wk[K][CPL], bk[K];
#pragma unroll
  for (int k = 0; k < K; ++k) {
    load_row<CPL>(W + k * C + sub * CPL, wk[k]);
    bk[k] = bias[k];
  }
  const float gs = gout[0] / stats[1];  // d(Σw·ce / Σw): the loss gradient over Σw
  float gw[K][CPL], gb[K];
#pragma unroll
  for (int k = 0; k < K; ++k) {
    gb[k] = 0.f;
#pragma unroll
    for (int j = 0; j < CPL; ++j) gw[k][j] = 0.f;
  }
  for (long long r = (long long)blockIdx.x * PH_ROWS + w * 4 + grp; r < R; r += (long long)gridDim.x * PH_ROWS) {
    float h[CPL], z[K];
    load_row<CPL>(H + r * C + sub * CPL, h);
    const long long lab64 = labels[r];
    row_logits<C, K>(h, wk, bk, z);
    const int lab = (lab64 >= 0 && lab64 < K) ? (int)lab64 : -1;
    float m = z[0];
#pragma unroll
    for (int k = 1; k < K; ++k) m = fmaxf(m, z[k]);
    float se = 0.f;
#pragma unroll
    for (int k = 0; k < K; ++k) {
      z[k] = __expf(z[k] - m);
      se += z[k];
    }
    const float scale = lab >= 0 ? wts[lab] * gs / se : 0.f;
    const float g1 = lab >= 0 ? wts[lab] * gs : 0.f;
    float coef[K];
#pragma unroll
    for (int k = 0; k < K; ++k) coef[k] = z[k] * scale - (k == lab ? g1 : 0.f);
    float dh[CPL];
#pragma unroll
    for (int j = 0; j < CPL; ++j) {
      float s = 0.f;
#pragma unroll
      for (int k = 0; k < K; ++k) s = fmaf(coef[k], wk[k][j], s);
      dh[j] = s;
    }
    float* dp = dH + r * C + sub * CPL;
    if constexpr (CPL % 4 == 0) {
#pragma unroll
      for (int j = 0; j < CPL; j += 4) *reinterpret_cast<float4*>(dp + j) = make_float4(dh[j], dh[j + 1], dh[j + 2], dh[j + 3]);
    } else {
#pragma unroll
      for (int j = 0; j < CPL; j += 2) *reinterpret_cast<float2*>(dp + j) = make_float2(dh[j], dh[j + 1]);
    }
#pragma unroll
    for (int k = 0; k < K; ++k) {
#pragma unroll
      for (int j = 0; j < CPL; ++j) gw[k][j] = fmaf(coef[k], h[j], gw[k][j]);
      gb[k] += sub == 0 ? coef[k] : 0.f;
    }
  }
  // the 4 row groups of a wave hold the same channels (lanes l, l ^ 16, l ^ 32, l ^ 48)
  __shared__ float sred[4][NP];
#pragma unroll
  for (int k = 0; k < K; ++k) {
#pragma unroll
    for (int j = 0; j < CPL; ++j) {
      const float v = xor32_sum(xor16_sum(gw[k][j]));
      if (grp == 0) sred[w][k * C + sub * CPL + j] = v;
    }
    const float vb = wave_sum(gb[k]);
    if (l == 0) sred[w][K * C + k] = vb;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < NP; i += blockDim.x)
    part[(long long)blockIdx.x * NP + i] = sred[0][i] + sred[1][i] + sred[2][i] + sred[3][i];
}

// stats = [column sums of the partials (NS) | acc(lab > 0), acc_1 … acc_{K-1}], loss = Σw·ce / Σw.
// One block of NS waves: wave s sums column s.
__global__ void pixel_ce_finalize_kernel(const float* __restrict__ part, int nblk, int NS, int K,
                                         float* __restrict__ stats, float* __restrict__ loss) {
  const int w = wave_id(), l = lane_id();
  float s = 0.f;
  for (int i = l; i < nblk; i += 64) s += part[(long long)i * NS + w];
  s = wave_sum(s);
  __shared__ float tot[16];
  if (l == 0) tot[w] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int j = 0; j < NS; ++j) stats[j] = tot[j];
    loss[0] = tot[0] / tot[1];
    stats[NS] = tot[2] > 0.f ? tot[3] / tot[2] : 0.f;
    for (int k = 1; k < K; ++k) stats[NS + k] = tot[4 + 2 * k] > 0.f ? tot[5 + 2 * k] / tot[4 + 2 * k] : 0.f;
  }
}

// dW (K·C) and db (K) += column sums of the (nblk, K·C + K) partials; 64 columns × 16 row
// phases per block, two independent chains per thread, a fixed-order LDS tree at the end
__global__ __launch_bounds__(1024) void pixel_ce_wgrad_kernel(const float* __restrict__ part, int nblk, int NP, int KC,
                                                              float* __restrict__ dW, float* __restrict__ db) {
  const int c = threadIdx.x & 63, ph = threadIdx.x >> 6, col = blockIdx.x * 64 + c;
  float s0 = 0.f, s1 = 0.f;
  if (col < NP) {
    int i = ph;
    for (; i + 16 < nblk; i += 32) {
      s0 += part[(long long)i * NP + col];
      s1 += part[(long long)(i + 16) * NP + col];
    }
    if (i < nblk) s0 += part[(long long)i * NP + col];
  }
  __shared__ float red[16][64];
  red[ph][c] = s0 + s1;
  __syncthreads();
  for (int h = 8; h > 0; h >>= 1) {
    if (ph < h) red[ph][c] += red[ph + h][c];
    __syncthreads();
  }
  if (ph == 0 && col < NP) {
    if (col < KC) dW[col] += red[0][c];
    else db[col - KC] += red[0][c];
  }
}

int pixel_ce_blocks(long long R) {
  long long b = (R + PH_ROWS - 1) / PH_ROWS;
  if (b > 512) b = 512;
  return b < 1 ? 1 : (int)b;
}

#define PH_DISPATCH(KERNEL, ...)                                                            \
  do {                                                                                      \
    const dim3 g(pixel_ce_blocks(R)), t(256);                                               \
    if (C == 32 && K == 2) hipLaunchKernelGGL((KERNEL<32, 2>), g, t, 0, st, __VA_ARGS__);   \
    else if (C == 32 && K == 3) hipLaunchKernelGGL((KERNEL<32, 3>), g, t, 0, st, __VA_ARGS__); \
    else if (C == 32 && K == 4) hipLaunchKernelGGL((KERNEL<32, 4>), g, t, 0, st, __VA_ARGS__); \
    else if (C == 64 && K == 2) hipLaunchKernelGGL((KERNEL<64, 2>), g, t, 0, st, __VA_ARGS__); \
    else if (C == 64 && K == 3) hipLaunchKernelGGL((KERNEL<64, 3>), g, t, 0, st, __VA_ARGS__); \
    else if (C == 64 && K == 4) hipLaunchKernelGGL((KERNEL<64, 4>), g, t, 0, st, __VA_ARGS__); \
    else if (C == 128 && K == 2) hipLaunchKernelGGL((KERNEL<128, 2>), g, t, 0, st, __VA_ARGS__); \
    else if (C == 128 && K == 3) hipLaunchKernelGGL((KERNEL<128, 3>), g, t, 0, st, __VA_ARGS__); \
    else if (C == 128 && K == 4) hipLaunchKernelGGL((KERNEL<128, 4>), g, t, 0, st, __VA_ARGS__); \
  } while (0)

void pixel_ce_fwd_launch(int C, int K, const float* H, const float* W, const float* bias, const int64_t* labels,
                         const float* wts, long long R, float* part, float* stats, float* loss, hipStream_t st) {
  if (R > 0) PH_DISPATCH(pixel_ce_fwd_kernel, H, W, bias, labels, wts, R, part);
  const int NS = 4 + 2 * K;
  hipLaunchKernelGGL(pixel_ce_finalize_kernel, dim3(1), dim3(64 * NS), 0, st, part, pixel_ce_blocks(R), NS, K, stats,
                     loss);
}

void pixel_ce_bwd_launch(int C, int K, const float* H, const float* W, const float* bias, const int64_t* labels,
                         const float* wts, const float* gout, const float* stats, long long R, float* dH, float* part,
                         float* dW, float* db, hipStream_t st) {
  if (R > 0) PH_DISPATCH(pixel_ce_bwd_kernel, H, W, bias, labels, wts, gout, stats, R, dH, part);
  const int NP = K * C + K;
  hipLaunchKernelGGL(pixel_ce_wgrad_kernel, dim3((NP + 63) / 64), dim3(1024), 0, st, part, pixel_ce_blocks(R), NP,
                     K * C, dW, db);
}

// ---- inference: class / confidence per row, the class map and a confusion count --------------
// The forward kernel's row layout and logits; nothing is reduced but the optional K×K confusion
// count (rows = label, columns = prediction), kept per thread in registers and stored as one int32
// partial row per block (no atomics; the caller sums the rows).  Lane sub == 0 of a row stores
// classes[r] / conf[r] (0 / 0 on an invalid row) and, on a valid row, the byte
// cmap[(r / Q)·npix + qidx[r]]: every build skips an index outside [0, npix), the checked build
// also flags it.  Valid indices of one sample must be distinct (two rows at one pixel race).
template <int C, int K>
__global__ __launch_bounds__(256) void pixel_predict_kernel(const float* __restrict__ H, const float* __restrict__ W,
                                                            const float* __restrict__ bias,
                                                            const int64_t* __restrict__ qidx,
                                                            const bool* __restrict__ qvalid,
                                                            const int64_t* __restrict__ labels, long long R,
                                                            long long Q, long long npix,
                                                            uint8_t* __restrict__ classes, float* __restrict__ conf,
                                                            uint8_t* __restrict__ cmap, int* __restrict__ cpart) {
  constexpr int CPL = C / 16, KK = K * K;
  const int l = lane_id(), w = wave_id(), sub = l & 15, grp = l >> 4;
  float wk[K][CPL], bk[K];
#pragma unroll
  for (int k = 0; k < K; ++k) {
    load_row<CPL>(W + k * C + sub * CPL, wk[k]);
    bk[k] = bias[k];
  }
  int cnt[KK];
#pragma unroll
  for (int s = 0; s < KK; ++s) cnt[s] = 0;
  for (long long r = (long long)blockIdx.x * PH_ROWS + w * 4 + grp; r < R; r += (long long)gridDim.x * PH_ROWS) {
    float h[CPL], z[K];
    load_row<CPL>(H + r * C + sub * CPL, h);
    const bool valid = qvalid[r];
    const long long pix = qidx[r];
    const long long lab64 = labels != nullptr ? labels[r] : -1;
    row_logits<C, K>(h, wk, bk, z);
    float m = z[0];
    int pred = 0;
#pragma unroll
    for (int k = 1; k < K; ++k) {
      pred = z[k] > m ? k : pred;
      m = fmaxf(m, z[k]);
    }
    float se = 0.f;
#pragma unroll
    for (int k = 0; k < K; ++k) se += __expf(z[k] - m);
    if (sub == 0) {
      classes[r] = valid ? (uint8_t)pred : (uint8_t)0;
      conf[r] = valid ? 1.f / se : 0.f;
      if (valid) {
        const bool inside = pix >= 0 && pix < npix;
        if (inside) cmap[(r / Q) * npix + pix] = (uint8_t)pred;
        else pio_flag(kErrGatherRow);
        if (lab64 >= 0 && lab64 < K) {
          const int cell = (int)lab64 * K + pred;
#pragma unroll
          for (int s = 0; s < KK; ++s) cnt[s] += s == cell ? 1 : 0;
        }
      }
    }
  }
  if (cpart == nullptr) return;
  // only lanes 0, 16, 32, 48 of a wave counted
  __shared__ int sred[4][KK];
#pragma unroll
  for (int s = 0; s < KK; ++s) {
    int v = cnt[s];
    v += __shfl_xor(v, 16, 64);
    v += __shfl_xor(v, 32, 64);
    if (l == 0) sred[w][s] = v;
  }
  __syncthreads();
  if (threadIdx.x < KK)
    cpart[(long long)blockIdx.x * KK + threadIdx.x] =
        sred[0][threadIdx.x] + sred[1][threadIdx.x] + sred[2][threadIdx.x] + sred[3][threadIdx.x];
}

// cpart: (pixel_ce_blocks(R), K·K) int32 when labels are given, else nullptr; cmap (R / Q, npix) is
// zero-filled by the caller before this launch
void pixel_predict_launch(int C, int K, const float* H, const float* W, const float* bias, const int64_t* qidx,
                          const bool* qvalid, const int64_t* labels, long long R, long long Q, long long npix,
                          uint8_t* classes, float* conf, uint8_t* cmap, int* cpart, hipStream_t st) {
  if (R > 0) PH_DISPATCH(pixel_predict_kernel, H, W, bias, qidx, qvalid, labels, R, Q, npix, classes, conf, cmap, cpart);
}

// ---- segmentation loss: focal cross-entropy + soft Dice on the same row pass -------------------
// With p = softmax(z), pt = p[lab], q = 1 − pt = Σ_{k≠lab} e_k / Σ_k e_k (no cancellation) and
// w = wts[lab], a row takes part iff 0 <= lab < K and w > 0 (a weight-0 row present in a dense batch
// and the same row left out of a sparse one give the same sums):
//   F   = Σ w·q^γ·(−log pt) / Σ w                                      (γ = 0: the weighted CE above)
//   I_c = Σ p_c·[lab = c]   P_c = Σ p_c   T_c = Σ [lab = c]            (rows that take part)
//   D   = 1 − (1/|S|) Σ_{c∈S} (2·I_c + ε) / (P_c + T_c + ε),  S = {c : wts[c] > 0}
//   loss = ce_weight·F + dice_weight·D     (a term whose weight is 0 is not evaluated: its columns stay 0)
// fwd: the partial columns of pixel_ce_fwd_kernel (Σ w·q^γ·ce in column 0; counts and hits over every
//      labelled row, as there), then I_c, P_c, T_c: 4 + 5K columns.
// bwd: coef_k = g·[ce_weight·w·f/Σw·(p_k − [k = lab]) + dice_weight·p_k·(g_k − Σ_c p_c·g_c)] with
//      f = q^γ + γ·pt·q^(γ−1)·ce (ce = −log pt; exactly 1 at γ = 0, 0 at q = 0 with γ > 0) and
//      g_c = a_c·[lab = c] + b_c, a_c = −2/(|S|·U_c), b_c = (2·I_c + ε)/(|S|·U_c²) on S, else 0;
//      dH, dW | db partials exactly as pixel_ce_bwd_kernel, summed by pixel_ce_wgrad_kernel.
// γ, the two weights and ε are kernel arguments: constants of a run, baked into a captured graph.

// q^γ on q in [0, 1]: γ = 0 does not touch q, γ = 2 is a multiply, else 2^(γ·log2 q), 0 at q = 0
__device__ __forceinline__ float focal_pow(float q, float gamma) {
  if (gamma == 0.f) return 1.f;
  if (gamma == 2.f) return q * q;
  return q > 0.f ? fast_exp2(gamma * __log2f(q)) : 0.f;
}

// f = q^γ − γ·pt·q^(γ−1)·log pt = q^γ·(1 + γ·pt·ce/q): no q^(γ−1), so nothing grows as q → 0
__device__ __forceinline__ float focal_factor(float q, float pt, float ce, float gamma) {
  if (gamma == 0.f) return 1.f;
  if (gamma == 2.f) return q * (q + 2.f * pt * ce);
  return q > 0.f ? focal_pow(q, gamma) * (1.f + gamma * pt * ce / q) : 0.f;
}

template <int C, int K>
__global__ __launch_bounds__(256) void pixel_seg_fwd_kernel(const float* __restrict__ H, const float* __restrict__ W,
                                                            const float* __restrict__ bias,
                                                            const int64_t* __restrict__ labels,
                                                            const float* __restrict__ wts, float gamma, float cew,
                                                            float dcw, long long R, float* __restrict__ part) {
  constexpr int CPL = C / 16, NS = 4 + 5 * K, OI = 4 + 2 * K, OP = OI + K, OT = OP + K;
  const int l = lane_id(), w = wave_id(), sub = l & 15, grp = l >> 4;
  float wk[K][CPL], bk[K];
#pragma unroll
  for (int k = 0; k < K; ++k) {
    load_row<CPL>(W + k * C + sub * CPL, wk[k]);
    bk[k] = bias[k];
  }
  float acc[NS];
#pragma unroll
  for (int s = 0; s < NS; ++s) acc[s] = 0.f;
  for (long long r = (long long)blockIdx.x * PH_ROWS + w * 4 + grp; r < R; r += (long long)gridDim.x * PH_ROWS) {
    float h[CPL], z[K];
    load_row<CPL>(H + r * C + sub * CPL, h);
    const long long lab64 = labels[r];
    row_logits<C, K>(h, wk, bk, z);
    const int lab = (lab64 >= 0 && lab64 < K) ? (int)lab64 : -1;
    float m = z[0];
    int pred = 0;
#pragma unroll
    for (int k = 1; k < K; ++k) {
      pred = z[k] > m ? k : pred;
      m = fmaxf(m, z[k]);
    }
    float e[K], se = 0.f, zl = 0.f, eo = 0.f, wl = 0.f;
#pragma unroll
    for (int k = 0; k < K; ++k) {
      e[k] = __expf(z[k] - m);
      se += e[k];
      zl = k == lab ? z[k] : zl;
      eo += k == lab ? 0.f : e[k];
    }
    if (lab >= 0) wl = wts[lab];
    if (sub == 0 && lab >= 0) {
      const float hit = pred == lab ? 1.f : 0.f;
      if (lab > 0) {
        acc[2] += 1.f;
        acc[3] += hit;
      }
#pragma unroll
      for (int k = 0; k < K; ++k) {
        acc[4 + 2 * k] += k == lab ? 1.f : 0.f;
        acc[5 + 2 * k] += k == lab ? hit : 0.f;
      }
      if (wl > 0.f) {
        acc[1] += wl;
        const float inv = 1.f / se;
        if (cew > 0.f) {
          const float ce = m + __logf(se) - zl;
          acc[0] += wl * focal_pow(eo * inv, gamma) * ce;
        }
        if (dcw > 0.f) {
#pragma unroll
          for (int k = 0; k < K; ++k) {
            const float p = e[k] * inv;
            acc[OI + k] += k == lab ? p : 0.f;
            acc[OP + k] += p;
            acc[OT + k] += k == lab ? 1.f : 0.f;
          }
        }
      }
    }
  }
  __shared__ float sred[4][NS];
#pragma unroll
  for (int s = 0; s < NS; ++s) {
    const float v = wave_sum(acc[s]);
    if (l == 0) sred[w][s] = v;
  }
  __syncthreads();
  if (threadIdx.x < NS)
    part[(long long)blockIdx.x * NS + threadIdx.x] =
        sred[0][threadIdx.x] + sred[1][threadIdx.x] + sred[2][threadIdx.x] + sred[3][threadIdx.x];
}

// stats = [column sums of the partials (NS = 4 + 5K) | acc(lab > 0), acc_1 … acc_{K-1} | F, D |
// (2·I_c + ε)/U_c for every class c], loss = ce_weight·F + dice_weight·D; a term whose weight is 0
// reads 0 (so do its per-class coefficients).  One block of 16 waves: wave w sums the columns w and
// w + 16 in the order of pixel_ce_finalize_kernel (up to 24 columns do not fit one wave each).
__global__ __launch_bounds__(1024) void pixel_seg_finalize_kernel(const float* __restrict__ part, int nblk, int K,
                                                                 const float* __restrict__ wts, float cew, float dcw,
                                                                 float eps, float* __restrict__ stats,
                                                                 float* __restrict__ loss) {
  const int w = wave_id(), l = lane_id(), NS = 4 + 5 * K;
  __shared__ float tot[24];  // NS <= 24 (K <= 4)
  for (int c = w; c < NS; c += 16) {
    float s = 0.f;
    for (int i = l; i < nblk; i += 64) s += part[(long long)i * NS + c];
    s = wave_sum(s);
    if (l == 0) tot[c] = s;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int j = 0; j < NS; ++j) stats[j] = tot[j];
    stats[NS] = tot[2] > 0.f ? tot[3] / tot[2] : 0.f;
    for (int k = 1; k < K; ++k) stats[NS + k] = tot[4 + 2 * k] > 0.f ? tot[5 + 2 * k] / tot[4 + 2 * k] : 0.f;
    const float F = cew > 0.f ? tot[0] / tot[1] : 0.f;
    float D = 0.f;
    if (dcw > 0.f) {
      float ns = 0.f, ds = 0.f;
      for (int c = 0; c < K; ++c) {
        const float d = (2.f * tot[4 + 2 * K + c] + eps) / (tot[4 + 3 * K + c] + tot[4 + 4 * K + c] + eps);
        stats[NS + K + 2 + c] = d;
        if (wts[c] > 0.f) {
          ns += 1.f;
          ds += d;
        }
      }
      D = 1.f - ds / ns;
    } else {
      for (int c = 0; c < K; ++c) stats[NS + K + 2 + c] = 0.f;
    }
    stats[NS + K] = F;
    stats[NS + K + 1] = D;
    loss[0] = (cew > 0.f ? cew * F : 0.f) + (dcw > 0.f ? dcw * D : 0.f);
  }
}

template <int C, int K>
__global__ __launch_bounds__(256) void pixel_seg_bwd_kernel(const float* __restrict__ H, const float* __restrict__ W,
                                                            const float* __restrict__ bias,
                                                            const int64_t* __restrict__ labels,
                                                            const float* __restrict__ wts, float gamma, float cew,
                                                            float dcw, float eps, const float* __restrict__ gout,
                                                            const float* __restrict__ stats, long long R,
                                                            float* __restrict__ dH, float* __restrict__ part) {
  constexpr int CPL = C / 16, NP = K * C + K, OI = 4 + 2 * K, OP = OI + K, OT = OP + K;
  const int l = lane_id(), w = wave_id(), sub = l & 15, grp = l >> 4;
  float wk[K][CPL], bk[K];
#pragma unroll
  for (int k = 0; k < K; ++k) {
    load_row<CPL>(W + k * C + sub * CPL, wk[k]);
    bk[k] = bias[k];
  }
  const float gs = cew > 0.f ? gout[0] * cew / stats[1] : 0.f;  // the focal term's gradient over Σw
  float ca[K], cb[K];  // g·dice_weight·(a_c, b_c)
  {
    float ns = 0.f;
#pragma unroll
    for (int k = 0; k < K; ++k) ns += wts[k] > 0.f ? 1.f : 0.f;
    const float gd = dcw > 0.f ? gout[0] * dcw / ns : 0.f;
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const float u = stats[OP + k] + stats[OT + k] + eps;
      const bool in = dcw > 0.f && wts[k] > 0.f;
      ca[k] = in ? -2.f * gd / u : 0.f;
      cb[k] = in ? gd * (2.f * stats[OI + k] + eps) / (u * u) : 0.f;
    }
  }
  float gw[K][CPL], gb[K];
#pragma unroll
  for (int k = 0; k < K; ++k) {
    gb[k] = 0.f;
#pragma unroll
    for (int j = 0; j < CPL; ++j) gw[k][j] = 0.f;
  }
  for (long long r = (long long)blockIdx.x * PH_ROWS + w * 4 + grp; r < R; r += (long long)gridDim.x * PH_ROWS) {
    float h[CPL], z[K];
    load_row<CPL>(H + r * C + sub * CPL, h);
    const long long lab64 = labels[r];
    row_logits<C, K>(h, wk, bk, z);
    const int lab = (lab64 >= 0 && lab64 < K) ? (int)lab64 : -1;
    float m = z[0];
#pragma unroll
    for (int k = 1; k < K; ++k) m = fmaxf(m, z[k]);
    float se = 0.f, zl = 0.f, el = 0.f, eo = 0.f;
#pragma unroll
    for (int k = 0; k < K; ++k) {
      zl = k == lab ? z[k] : zl;
      z[k] = __expf(z[k] - m);
      se += z[k];
      el = k == lab ? z[k] : el;
      eo += k == lab ? 0.f : z[k];
    }
    const float wl = lab >= 0 ? wts[lab] : 0.f;
    const bool take = wl > 0.f;
    const float inv = 1.f / se;
    float coef[K];
#pragma unroll
    for (int k = 0; k < K; ++k) {
      z[k] *= inv;  // softmax
      coef[k] = 0.f;
    }
    if (cew > 0.f) {
      float f = 1.f;
      if (gamma != 0.f) f = focal_factor(eo * inv, el * inv, m + __logf(se) - zl, gamma);
      const float fs = take ? wl * gs * f : 0.f;
#pragma unroll
      for (int k = 0; k < K; ++k) coef[k] = fs * (z[k] - (k == lab ? 1.f : 0.f));
    }
    if (dcw > 0.f) {
      float g[K], s = 0.f;
#pragma unroll
      for (int k = 0; k < K; ++k) {
        g[k] = cb[k] + (k == lab ? ca[k] : 0.f);
        s = fmaf(z[k], g[k], s);
      }
#pragma unroll
      for (int k = 0; k < K; ++k) coef[k] += take ? z[k] * (g[k] - s) : 0.f;
    }
    float dh[CPL];
#pragma unroll
    for (int j = 0; j < CPL; ++j) {
      float s = 0.f;
#pragma unroll
      for (int k = 0; k < K; ++k) s = fmaf(coef[k], wk[k][j], s);
      dh[j] = s;
    }
    float* dp = dH + r * C + sub * CPL;
    if constexpr (CPL % 4 == 0) {
#pragma unroll
      for (int j = 0; j < CPL; j += 4) *reinterpret_cast<float4*>(dp + j) = make_float4(dh[j], dh[j + 1], dh[j + 2], dh[j + 3]);
    } else {
#pragma unroll
      for (int j = 0; j < CPL; j += 2) *reinterpret_cast<float2*>(dp + j) = make_float2(dh[j], dh[j + 1]);
    }
#pragma unroll
    for (int k = 0; k < K; ++k) {
#pragma unroll
      for (int j = 0; j < CPL; ++j) gw[k][j] = fmaf(coef[k], h[j], gw[k][j]);
      gb[k] += sub == 0 ? coef[k] : 0.f;
    }
  }
  // the 4 row groups of a wave hold the same channels (lanes l, l ^ 16, l ^ 32, l ^ 48)
  __shared__ float sred[4][NP];
#pragma unroll
  for (int k = 0; k < K; ++k) {
#pragma unroll
    for (int j = 0; j < CPL; ++j) {
      const float v = xor32_sum(xor16_sum(gw[k][j]));
      if (grp == 0) sred[w][k * C + sub * CPL + j] = v;
    }
    const float vb = wave_sum(gb[k]);
    if (l == 0) sred[w][K * C + k] = vb;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < NP; i += blockDim.x)
    part[(long long)blockIdx.x * NP + i] = sred[0][i] + sred[1][i] + sred[2][i] + sred[3][i];
}

// part: (pixel_ce_blocks(R), 4 + 5K), zero-filled by the caller when R == 0 (no row launch then);
// stats: 6 + 7K floats (layout above pixel_seg_finalize_kernel)
void pixel_seg_fwd_launch(int C, int K, const float* H, const float* W, const float* bias, const int64_t* labels,
                          const float* wts, float gamma, float ce_weight, float dice_weight, float eps, long long R,
                          float* part, float* stats, float* loss, hipStream_t st) {
  if (R > 0) PH_DISPATCH(pixel_seg_fwd_kernel, H, W, bias, labels, wts, gamma, ce_weight, dice_weight, R, part);
  hipLaunchKernelGGL(pixel_seg_finalize_kernel, dim3(1), dim3(1024), 0, st, part, pixel_ce_blocks(R), K, wts, ce_weight,
                     dice_weight, eps, stats, loss);
}

// part: (pixel_ce_blocks(R), K·C + K), zero-filled by the caller when R == 0; dW / db accumulated
void pixel_seg_bwd_launch(int C, int K, const float* H, const float* W, const float* bias, const int64_t* labels,
                          const float* wts, float gamma, float ce_weight, float dice_weight, float eps,
                          const float* gout, const float* stats, long long R, float* dH, float* part, float* dW,
                          float* db, hipStream_t st) {
  if (R > 0)
    PH_DISPATCH(pixel_seg_bwd_kernel, H, W, bias, labels, wts, gamma, ce_weight, dice_weight, eps, gout, stats, R, dH,
                part);
  const int NP = K * C + K;
  hipLaunchKernelGGL(pixel_ce_wgrad_kernel, dim3((NP + 63) / 64), dim3(1024), 0, st, part, pixel_ce_blocks(R), NP,
                     K * C, dW, db);
}
#undef PH_DISPATCH

// ---- nonzero_compact: dense image (B, npix) → the sparse operands of the encoder ----------------
// Ordered stream compaction of the pixels with img != 0 (-0.0 is zero, NaN is not), per sample:
// slot j < min(count, cap) of values / index / kmask holds the j-th such pixel in flat order
// (kmask False), every later slot (0, 0, True): what data/lartpc.py sparse_collate builds on the
// CPU.  count is the true number of non-zero pixels, also beyond cap.
//
// A sample is cut into S segments of whole tiles.  With S > 1 a first launch counts each
// segment; the scatter launch (S × B blocks) turns the segment counts into its base slot and the
// sample total, then walks its segment in tiles of 256·V pixels: V coalesced loads per thread
// (element j·256 + t of the tile; no alignment assumed), one ballot per load, wave totals through
// a ping-pong LDS buffer (one barrier per tile), the running base in a register of every thread.
// The order comes from the scan alone (no atomics).  With S = 1 the count launch is skipped; a
// counting call (cap = 0) with S > 1 skips the walk instead (its total is the sum of the counts).
__global__ __launch_bounds__(NZ_THREADS) void nonzero_count_kernel(const float* __restrict__ img, long long npix,
                                                                   long long seg, int* __restrict__ segcount) {
  const int s = blockIdx.x, b = blockIdx.y, S = gridDim.x;
  const long long start = (long long)s * seg, end = start + seg < npix ? start + seg : npix;
  const float* p = img + (long long)b * npix;
  int n = 0;
  for (long long i = start + threadIdx.x; i < end; i += NZ_THREADS) n += p[i] != 0.f ? 1 : 0;
  __shared__ int sW[NZ_WAVES];
  n = block_isum(n, sW);
  if (threadIdx.x == 0) segcount[(long long)b * S + s] = n;
}

template <int V>
__global__ __launch_bounds__(NZ_THREADS) void nonzero_scatter_kernel(const float* __restrict__ img, long long npix,
                                                                     long long seg, long long cap,
                                                                     const int* __restrict__ segcount,
                                                                     float* __restrict__ values,
                                                                     int64_t* __restrict__ index,
                                                                     bool* __restrict__ kmask, int* __restrict__ count) {
  constexpr int TILE = NZ_THREADS * V;
  const int s = blockIdx.x, b = blockIdx.y, S = gridDim.x;
  __shared__ int sW[2][V][NZ_WAVES];
  __shared__ int sR[2][NZ_WAVES];
  long long run = 0, total = 0;  // slots of the sample before this block's next tile; the sample's count
  if (S > 1) seg_prefix(segcount + (long long)b * S, 1, s, S, sR, run, total);  // S <= NZ_THREADS
  const long long start = (long long)s * seg, end = start + seg < npix ? start + seg : npix;
  const float* p = img + (long long)b * npix;
  float* vo = values + (long long)b * cap;
  int64_t* io = index + (long long)b * cap;
  bool* mo = kmask + (long long)b * cap;
  int buf = 0;
  // a counting call (cap == 0) with S > 1 already has its total: no second read of the image
  const bool walk = S == 1 || cap > 0;
  for (long long t0 = start; walk && t0 < end; t0 += TILE, buf ^= 1) {
    float v[V];
    bool hit[V];
    int pre[V];
#pragma unroll
    for (int j = 0; j < V; ++j) {
      const long long i = t0 + j * NZ_THREADS + threadIdx.x;
      v[j] = i < end ? p[i] : 0.f;
      hit[j] = v[j] != 0.f;
    }
    tile_ballot<V>(hit, pre, sW[buf]);
    lds_sync();
#pragma unroll
    for (int j = 0; j < V; ++j) {
      const long long pos = tile_slot(sW[buf][j], pre[j], run);
      if (hit[j] && pos < cap) {
        vo[pos] = v[j];
        io[pos] = t0 + j * NZ_THREADS + threadIdx.x;
        mo[pos] = false;
      }
    }
  }
  if (S == 1) total = run;
  // padding slots [min(total, cap), cap) of the sample, dealt over its S blocks
  for (long long j = (total < cap ? total : cap) + (long long)s * NZ_THREADS + threadIdx.x; j < cap;
       j += (long long)S * NZ_THREADS) {
    vo[j] = 0.f;
    io[j] = 0;
    mo[j] = true;
  }
  if (s == 0 && threadIdx.x == 0) count[b] = (int)total;
}

// S in [1, 256] segments per sample, V in {4, 8} loads per thread and tile; segcount: (B, S) int32
// scratch (unused when S == 1)
void nonzero_compact_launch(const float* img, int B, long long npix, long long cap, int S, int V, int* segcount,
                            float* values, int64_t* index, bool* kmask, int* count, hipStream_t st) {
  const long long seg = compact_seg_len(npix, S, V);
  const dim3 g(S, B), t(NZ_THREADS);
  if (S > 1) hipLaunchKernelGGL(nonzero_count_kernel, g, t, 0, st, img, npix, seg, segcount);
  if (V == 8)
    hipLaunchKernelGGL(nonzero_scatter_kernel<8>, g, t, 0, st, img, npix, seg, cap, segcount, values, index, kmask, count);
  else
    hipLaunchKernelGGL(nonzero_scatter_kernel<4>, g, t, 0, st, img, npix, seg, cap, segcount, values, index, kmask, count);
}

unsigned check_errors_pixel_head(bool reset) { return pio_read_errors(reset); }

}  // namespace pio
