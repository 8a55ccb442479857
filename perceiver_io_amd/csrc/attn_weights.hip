// Head-averaged attention weights from the flash forward's operands (CDNA4 / gfx950), inference only.
//
// attn_fwd keeps O and the row LSE; with Q, K and that LSE the probabilities are
// P[b,h,n,k] = 2^(s·scale·log2e − LSE[b,n,h]) exactly, tile by tile.  This unit makes that one
// extra pass and reduces over the heads (and optionally over the queries) in registers:
//   avg  (B, Nq, Nk) fp32 = (1/H) Σ_h P        nn.MultiheadAttention's need_weights=True result
//   mass (B, Nk)     fp32 = Σ_n avg[b,n,k]     the attention each input receives
// No per-head tile is written anywhere: there is no (B, H, Nq, Nk) buffer, and with only the mass
// requested nothing of size Nq·Nk is written.
//
// A wave owns 32 keys, a workgroup (4 waves) 128 keys of one sample, and walks a chunk of 32-query
// tiles.  Per tile and head S = Q·Kᵀ is one chain of v_mfma_f32_32x32x16_bf16 with the query rows on
// the accumulator registers and the key on the lane; both operand fragments are k-contiguous, so
// they are read straight from global memory (16 B per lane) and no operand passes through LDS.
// "Once per head" holds for one query tile (Nq <= 32: the encoder shapes): the head count is a
// run-time value, so a wave does not keep its K fragments of every head in registers and loads them
// again for each further query tile of its chunk (from L1 / L2; 8 query tiles in 2 chunks re-read K
// 4 times per chunk), as every tile loads its Q fragments.  The head sum stays in 16 fp32 registers in head order and is scaled by 1/H once.
// Key on the lane makes an avg row store 128 contiguous bytes per register and the column (query)
// sum an in-lane sum plus one lane^32 exchange; a wave owns its keys for the whole chunk, so the mass
// needs no cross-wave step and the kernel no LDS at all.
//
// mass order (bitwise reproducible, no atomics): the 16 registers of a lane in register order, the
// two lane halves, then the query tiles of the chunk in order; several chunks (few keys, many
// queries: the decoder) store per-chunk partials that a second launch adds in chunk order.
//
// A padded key gives exactly 0 (a select, not an exponential), so a query row whose keys are all
// padded gives all zeros whatever its LSE holds; a non-finite LSE (attn_fwd's +inf sentinel for such
// a row) and query rows past Nq read as +inf, i.e. 2^−inf = 0.  Ragged Nq / Nk are guards on the
// addresses and stores; the operands are not padded.  q_bs = 0 broadcasts one query stream over the
// batch, K may be a strided view of packed K|V rows.
#include "common.h"

// the MFMA shape and operand lane maps used here are gfx950's
#if defined(__HIP_DEVICE_COMPILE__) && !defined(__gfx950__)
#error "this translation unit is written for gfx950 (MI355X) only"
#endif

namespace pio {

constexpr int kAwWaves = 4;               // waves per workgroup, 32 keys each
constexpr int kAwKeys = 32 * kAwWaves;    // keys per workgroup
constexpr int kAwMinTiles = 4;            // query tiles a workgroup walks before the queries are chunked
constexpr int kAwWantBlocks = 1024;       // ≈ 4 workgroups per CU
constexpr int kAwMaxKeys = 1 << 26;       // keys per sample (the binding checks it): 32-bit offsets inside a tile

template <int D, bool AVG, bool MASS>
// workgroups per CU the register budget is held to: 4 (128 VGPRs) for the mass alone, 3 with the avg
// stores (their addresses live beside the operand fragments; 128 spills), 2 at head width 128
__global__ __launch_bounds__(64 * kAwWaves, D > 64 ? 2 : (AVG ? 3 : 4)) void attn_weights_kernel(
    AttnArgs a, const float* __restrict__ LSE, float* __restrict__ avg, float* __restrict__ mass, long long mass_bs,
    int tiles_per_chunk) {
  constexpr int KS = D / 16;
  const int w = wave_id(), l = lane_id(), r = l & 31, hh = l >> 5;
  const int b = blockIdx.z, chunk = blockIdx.y;
  const int kw0 = (blockIdx.x * kAwWaves + w) * 32;
  if (kw0 >= a.Nk) return;  // wave-uniform; the kernel has no barrier
  const int key = kw0 + r;  // accumulator column of this lane
  const bool kin = key < a.Nk;
  const int kc = kin ? key : a.Nk - 1;
  bool pad = !kin;
  if (a.kmask != nullptr) pad |= a.kmask[(long long)b * a.Nk + kc] != 0;
  // B operand: B[k = 8hh + j][col = key] = K[key][h·D + 16s + 8hh + j]
  const uint16_t* kp = a.k + (long long)b * a.k_bs + (long long)kc * a.k_rs + 8 * hh;
  const float* lp = LSE + (long long)b * a.Nq * a.H;
  const float inv_h = 1.f / (float)a.H;
  const int nqt = (a.Nq + 31) / 32;
  const int t0 = chunk * tiles_per_chunk, t1 = min(nqt, t0 + tiles_per_chunk);
  float msum = 0.f;
  for (int t = t0; t < t1; ++t) {
    const int q0 = 32 * t;
    // A operand: A[row = query][k = 8hh + j]; rows past Nq read the last query (their LSE is +inf)
    const int qa = min(q0 + r, a.Nq - 1);
    const uint16_t* qp = a.q + (long long)b * a.q_bs + (long long)qa * a.q_rs + 8 * hh;
    f32x16 acc = f32x16{};
    for (int h = 0; h < a.H; ++h) {
      bf16x8 qf[KS], kf[KS];
#pragma unroll
      for (int s = 0; s < KS; ++s) {
        qf[s] = *reinterpret_cast<const bf16x8*>(qp + h * D + 16 * s);
        kf[s] = *reinterpret_cast<const bf16x8*>(kp + h * D + 16 * s);
      }
      // LSE of this lane's 16 accumulator rows: unconditional loads at clamped rows (one base and
      // 32-bit offsets: Nq·H < 2^31 is checked by the binding), rows past Nq overridden
      float ls[16];
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int qi = q0 + acc_row(i, hh);
        const float v = lp[min(qi, a.Nq - 1) * a.H + h];
        ls[i] = (qi < a.Nq && fabsf(v) < INFINITY) ? v : INFINITY;
      }
      f32x16 s = f32x16{};
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) s = mfma32(qf[ks], kf[ks], s);
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[i] += pad ? 0.f : fast_exp2(fmaf(s[i], a.scale_log2, -ls[i]));
    }
    // explicitly rounded product and sums: the avg + mass and the mass-only instantiation give the
    // same bits whatever the compiler contracts elsewhere
    float cs = 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      acc[i] = __fmul_rn(acc[i], inv_h);
      cs = __fadd_rn(cs, acc[i]);
    }
    if constexpr (AVG) {
      if (kin) {
        // a uniform tile base and 32-bit lane offsets (32·Nk < 2^32: checked by the launcher)
        float* ap = avg + ((long long)b * a.Nq + q0) * a.Nk;
        const unsigned o0 = (unsigned)key + (unsigned)(4 * hh) * (unsigned)a.Nk;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          const int row = acc_row(i, hh);
          if (q0 + row < a.Nq) ap[o0 + (unsigned)acc_row(i, 0) * (unsigned)a.Nk] = acc[i];
        }
      }
    }
    if constexpr (MASS) msum = __fadd_rn(msum, xor32_sum(cs));
  }
  if constexpr (MASS) {
    if (hh == 0 && kin) mass[(long long)b * mass_bs + (long long)chunk * a.Nk + key] = msum;
  }
}

// mass[b][k] = Σ_c part[b][c][k] in chunk order
__global__ void attn_mass_reduce_kernel(const float* __restrict__ part, float* __restrict__ mass, int nchunks, int Nk,
                                        long long total) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const long long b = i / Nk;
  const int k = (int)(i - b * Nk);
  const float* p = part + b * nchunks * Nk + k;
  float s = 0.f;
  for (int c = 0; c < nchunks; ++c) s = __fadd_rn(s, p[(long long)c * Nk]);
  mass[i] = s;
}

int attn_weights_chunks(int B, int Nq, int Nk) {
  const long long base = (long long)B * ((Nk + kAwKeys - 1) / kAwKeys);
  const int nqt = (Nq + 31) / 32;
  const long long want = (kAwWantBlocks + base - 1) / base;
  const long long tpc0 = (nqt + want - 1) / want;
  const int tpc = (int)(tpc0 > kAwMinTiles ? tpc0 : kAwMinTiles);
  return (nqt + tpc - 1) / tpc;
}

template <int D>
static void aw_dispatch(const AttnArgs& a, const float* LSE, float* avg, float* mdst, long long mass_bs, int tpc,
                        dim3 grid, hipStream_t st) {
  const dim3 blk(64 * kAwWaves);
  if (avg != nullptr && mdst != nullptr)
    hipLaunchKernelGGL((attn_weights_kernel<D, true, true>), grid, blk, 0, st, a, LSE, avg, mdst, mass_bs, tpc);
  else if (avg != nullptr)
    hipLaunchKernelGGL((attn_weights_kernel<D, true, false>), grid, blk, 0, st, a, LSE, avg, mdst, mass_bs, tpc);
  else
    hipLaunchKernelGGL((attn_weights_kernel<D, false, true>), grid, blk, 0, st, a, LSE, avg, mdst, mass_bs, tpc);
}

void attn_weights_launch(const AttnArgs& a, int D, const float* LSE, float* avg, float* mass, float* part, int nchunks,
                         hipStream_t st) {
  if (a.B < 1 || a.Nq < 1 || a.Nk < 1 || a.Nk > kAwMaxKeys || nchunks < 1 || (avg == nullptr && mass == nullptr)) return;
  const int nqt = (a.Nq + 31) / 32;
  const int tpc = (nqt + nchunks - 1) / nchunks;
  const dim3 grid((unsigned)((a.Nk + kAwKeys - 1) / kAwKeys), (unsigned)nchunks, (unsigned)a.B);
  const bool two = mass != nullptr && nchunks > 1;
  float* mdst = two ? part : mass;
  const long long mass_bs = (long long)(two ? nchunks : 1) * a.Nk;
  switch (D) {
    case 16: aw_dispatch<16>(a, LSE, avg, mdst, mass_bs, tpc, grid, st); break;
    case 32: aw_dispatch<32>(a, LSE, avg, mdst, mass_bs, tpc, grid, st); break;
    case 64: aw_dispatch<64>(a, LSE, avg, mdst, mass_bs, tpc, grid, st); break;
    case 128: aw_dispatch<128>(a, LSE, avg, mdst, mass_bs, tpc, grid, st); break;
    default: return;
  }
  if (two) {
    const long long total = (long long)a.B * a.Nk;
    hipLaunchKernelGGL(attn_mass_reduce_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, part, mass,
                       nchunks, a.Nk, total);
  }
}

}  // namespace pio
