// Device code the vocabulary heads share (ce_head.hip, topk_head.hip, mlm_head.hip,
// soft_ce_head.hip): the pieces of a transposed logit tile Sᵀ = W·Hᵀ whose accumulator starts at
// the bias, and the log2-domain softmax statistics.  Include after common.h.
#pragma once

namespace pio {

constexpr float kL2E = 1.4426950408889634f;
constexpr float kLN2 = 0.6931471805599453f;

// a lane's half row (c = 16s + 8h .. + 7, s < KS, hp = the row + 8h) of an fp32 matrix as the bf16
// B operand of Sᵀ = W·Hᵀ, cast on load; zeros for a row outside the matrix (!rin)
template <int KS>
__device__ __forceinline__ void load_row_operand(bf16x8 (&hb)[KS], const float* hp, bool rin) {
  float4 a[KS], b[KS];
#pragma unroll
  for (int s = 0; s < KS; ++s) {
    a[s] = *reinterpret_cast<const float4*>(rin ? hp + 16 * s : kZero32B);
    b[s] = *reinterpret_cast<const float4*>(rin ? hp + 16 * s + 4 : kZero32B);
  }
#pragma unroll
  for (int s = 0; s < KS; ++s) {
    hb[s][0] = (short)f2bf(a[s].x); hb[s][1] = (short)f2bf(a[s].y); hb[s][2] = (short)f2bf(a[s].z);
    hb[s][3] = (short)f2bf(a[s].w); hb[s][4] = (short)f2bf(b[s].x); hb[s][5] = (short)f2bf(b[s].y);
    hb[s][6] = (short)f2bf(b[s].z); hb[s][7] = (short)f2bf(b[s].w);
  }
}

// a logit accumulator started at the bias: register i = bp[(i & 3) + 8(i >> 2)], four 16-byte LDS
// reads (bp = the 32-entry vocab block's bias + 4h), so the MFMAs add the bias
__device__ __forceinline__ f32x16 bias_acc(const float* bp) {
  f32x16 st;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const float4 bb = *reinterpret_cast<const float4*>(bp + 8 * q);
    st[4 * q] = bb.x; st[4 * q + 1] = bb.y; st[4 * q + 2] = bb.z; st[4 * q + 3] = bb.w;
  }
  return st;
}

// (m, l) ← the log2-domain (max, Σ 2^(t − max)) pairs (m, l) and (om, ol) merged; an empty side
// has m = −inf, l = 0
__device__ __forceinline__ void merge_ml(float& m, float& l, float om, float ol) {
  const float mn = fmaxf(m, om);
  const float ms = mn == -__builtin_inff() ? 0.f : mn;
  l = l * fast_exp2(m - ms) + ol * fast_exp2(om - ms);
  m = mn;
}

}  // namespace pio
