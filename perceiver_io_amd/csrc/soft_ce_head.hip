// Soft-target classifier head (MixUp / CutMix / label smoothing) and the batch mixing kernel.
//
// Target of row i: t_i = (1 − ε)·(λ_i·e_a + (1 − λ_i)·e_b) + ε/V; row loss
//   lse_i − (1 − ε)·(λ_i·z_ia + (1 − λ_i)·z_ib) − (ε/V)·Σ_v z_iv,  z = h·wᵀ + bias
// = F.cross_entropy(z, t_i) with probability targets.  The logits exist only as bf16 MFMA tiles
// accumulated in fp32; a classifier's M is a batch and V ≤ 1024, so the backward recomputes them.
//
//   forward   one workgroup per 32-row tile; wave w takes the class tiles w, w + 4, … as
//             Sᵀ = W·Hᵀ (classes on the accumulator rows, one row of h per lane) with an online
//             log-sum-exp, the running argmax (lower class on a tie), Σ_v z and the two label
//             logits; the four waves merge through LDS in wave order.  A second one-workgroup
//             launch sums the tiles' loss partials in a fixed order when there are several tiles.
//   backward  workgroups [0, row tiles): dH = dz·W of one 32-row tile, wave w over the class
//             tiles w, w + 4, … (dzᵀ is the accumulator of Sᵀ, used as the next product's B
//             operand), the waves' partials summed through LDS in wave order;
//             workgroups [row tiles, + class tiles): dW = dzᵀ·H and db = Σ dz of one 32-class
//             tile over all rows, wave w over the row tiles w, w + 4, …, merged the same way.
//             dz = g / max(count, 1)·(softmax(z) − t), zero on rows without a label; it enters
//             both products as a bf16 pair hi + lo (two MFMAs), so the gradients carry the
//             rounding of the bf16 operands h and w only.
// No atomics, no slab: every output element has one writer and one summation order, so every
// launch gives the same bits.
#include <algorithm>

#include "common.h"
#include "head_common.h"

namespace pio {

namespace sce {

constexpr int RT = 32;  // rows per tile
constexpr int NW = 4;   // waves per workgroup

// a row's label pair is usable: both inside [0, V) (label_a = -100: the row carries no loss)
__device__ __forceinline__ bool labels_ok(int a, int b, int V) { return a >= 0 && a < V && b >= 0 && b < V; }

// accumulator registers 8s .. 8s+7 as two bf16 operand fragments, x ≈ hi + lo (hi = bf16(x),
// lo = bf16(x − hi)): dz enters its two products with ≈16 mantissa bits instead of 8
__device__ __forceinline__ void pack_hi_lo(const f32x16& a, int s, bf16x8& hi, bf16x8& lo) {
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const uint16_t h = f2bf(a[8 * s + j]);
    hi[j] = (short)h;
    lo[j] = (short)f2bf(a[8 * s + j] - bf2f(h));
  }
}

}  // namespace sce

// ---- forward ------------------------------------------------------------------------------
template <int C>
__global__ __launch_bounds__(256) void soft_ce_fwd_kernel(const float* __restrict__ Hm, const uint16_t* __restrict__ W,
                                                          const float* __restrict__ bias, const int64_t* __restrict__ la,
                                                          const int64_t* __restrict__ lb, const float* __restrict__ lam,
                                                          float eps, int M, int V, float* __restrict__ lse,
                                                          int* __restrict__ pred, uint16_t* __restrict__ hs,
                                                          float* __restrict__ blk, float* __restrict__ loss,
                                                          float* __restrict__ count) {
  using namespace sce;
  constexpr int KS = C / 16;
  __shared__ float sm[NW][6][RT];
  __shared__ int smi[NW][RT];
  __shared__ float srow[2][RT];
  const int w = wave_id(), l = lane_id(), hh = l >> 5, rl = l & 31;
  const int gr = blockIdx.x * RT + rl;
  const bool rin = gr < M;
  // this lane's half row (c = 16s + 8hh .. + 7) as the B operand of Sᵀ = W·Hᵀ, cast on load
  bf16x8 hb[KS];
  {
    const float* hp = Hm + (long long)(rin ? gr : 0) * C + 8 * hh;
#pragma unroll
    for (int s = 0; s < KS; ++s) {
      const float4 a = *reinterpret_cast<const float4*>(hp + 16 * s);
      const float4 b = *reinterpret_cast<const float4*>(hp + 16 * s + 4);
      const float v[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
#pragma unroll
      for (int j = 0; j < 8; ++j) hb[s][j] = (short)f2bf(rin ? v[j] : 0.f);
    }
    if (w == 0 && rin)
#pragma unroll
      for (int s = 0; s < KS; ++s) *reinterpret_cast<bf16x8*>(hs + (long long)gr * C + 16 * s + 8 * hh) = hb[s];
  }
  const int a = rin ? (int)la[gr] : -100, b = rin ? (int)lb[gr] : 0;
  const bool ok = labels_ok(a, b, V);
#if PIO_CHECKS
  if (w == 0 && hh == 0 && rin && a != -100 && !ok) pio_flag(kErrLabel);
#endif
  const int ntiles = (V + 31) / 32, iters = (ntiles + NW - 1) / NW;
  const float ninf = -__builtin_inff();
  float m = ninf, s = 0.f, av = ninf, sz = 0.f, za = 0.f, zb = 0.f;
  int ai = 0x7fffffff;
  for (int t = 0; t < iters; ++t) {
    const int v0 = (t * NW + w) * 32;  // past V: every class of the tile is masked
    f32x16 st;
#pragma unroll
    for (int i = 0; i < 16; ++i) {  // the accumulator starts at the bias (−inf past V)
      const int c = v0 + acc_row(i, hh);
      const float bv = bias[c < V ? c : 0];
      st[i] = c < V ? bv : ninf;
    }
    const int vr = min(v0 + rl, V - 1);  // clamped: a class past V reads a real row, its logit stays −inf
    const uint16_t* wp = W + (long long)vr * C + 8 * hh;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) st = mfma32(*reinterpret_cast<const bf16x8*>(wp + 16 * ks), hb[ks], st);
    float tm = st[0];
#pragma unroll
    for (int i = 1; i < 16; ++i) tm = fmaxf(tm, st[i]);
    const float mn = fmaxf(m, tm);
    if (mn > ninf) {
      float ps = 0.f;
#pragma unroll
      for (int i = 0; i < 16; ++i) ps += fast_exp2((st[i] - mn) * kL2E);
      s = s * fast_exp2((m - mn) * kL2E) + ps;
      m = mn;
    }
#pragma unroll
    for (int i = 0; i < 16; ++i) {  // classes ascend with i: a strict compare keeps the lower one
      const int c = v0 + acc_row(i, hh);
      if (st[i] > av) { av = st[i]; ai = c; }
      sz += c < V ? st[i] : 0.f;
      za = c == a ? st[i] : za;
      zb = c == b ? st[i] : zb;
    }
  }
  // the row's other 16 classes of every tile sit on lane l ^ 32
  auto merge = [&](float m2, float s2, float av2, int ai2, float sz2, float za2, float zb2) {
    const float mn = fmaxf(m, m2);
    const float e1 = m > ninf ? s * fast_exp2((m - mn) * kL2E) : 0.f;
    const float e2 = m2 > ninf ? s2 * fast_exp2((m2 - mn) * kL2E) : 0.f;
    s = e1 + e2;
    m = mn;
    if (av2 > av || (av2 == av && ai2 < ai)) { av = av2; ai = ai2; }
    sz += sz2;
    za += za2;
    zb += zb2;
  };
  merge(__shfl_xor(m, 32), __shfl_xor(s, 32), __shfl_xor(av, 32), __shfl_xor(ai, 32), __shfl_xor(sz, 32),
        __shfl_xor(za, 32), __shfl_xor(zb, 32));
  if (hh == 0) {
    sm[w][0][rl] = m; sm[w][1][rl] = s; sm[w][2][rl] = av; sm[w][3][rl] = sz; sm[w][4][rl] = za; sm[w][5][rl] = zb;
    smi[w][rl] = ai;
  }
  __syncthreads();
  if (threadIdx.x < RT) {  // wave 0, lanes 0..31: the waves in order
#pragma unroll
    for (int k = 1; k < NW; ++k)
      merge(sm[k][0][rl], sm[k][1][rl], sm[k][2][rl], smi[k][rl], sm[k][3][rl], sm[k][4][rl], sm[k][5][rl]);
    const float L = m + __log2f(s) * kLN2;
    const float lm = rin ? lam[gr] : 1.f;
    const bool lab = rin && ok;
    const float row = L - (1.f - eps) * (lm * za + (1.f - lm) * zb) - (eps / (float)V) * sz;
    if (rin) {
      lse[gr] = L;
      pred[gr] = min(ai, V - 1);
    }
    srow[0][rl] = lab ? row : 0.f;
    srow[1][rl] = lab ? 1.f : 0.f;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    float t = 0.f, n = 0.f;
    for (int i = 0; i < RT; ++i) { t += srow[0][i]; n += srow[1][i]; }
    if (gridDim.x == 1) {
      count[0] = n;
      loss[0] = t / fmaxf(n, 1.f);
    } else {
      blk[blockIdx.x] = t;
      blk[gridDim.x + blockIdx.x] = n;
    }
  }
}

// the mean over the labelled rows from the row tiles' (Σ loss, count) partials, fixed order
__global__ __launch_bounds__(64) void soft_ce_finish_kernel(const float* __restrict__ blk, int nblk,
                                                            float* __restrict__ loss, float* __restrict__ count) {
  __shared__ float red[2][64];
  float t = 0.f, n = 0.f;
  for (int i = threadIdx.x; i < nblk; i += 64) { t += blk[i]; n += blk[nblk + i]; }
  red[0][threadIdx.x] = t;
  red[1][threadIdx.x] = n;
  __syncthreads();
  if (threadIdx.x == 0) {
    float tt = 0.f, nn = 0.f;
    for (int i = 0; i < 64; ++i) { tt += red[0][i]; nn += red[1][i]; }
    count[0] = nn;
    loss[0] = tt / fmaxf(nn, 1.f);
  }
}

// ---- backward -----------------------------------------------------------------------------
template <int C>
__global__ __launch_bounds__(256) void soft_ce_bwd_kernel(const uint16_t* __restrict__ Hs, const uint16_t* __restrict__ W,
                                                          const float* __restrict__ bias, const int64_t* __restrict__ la,
                                                          const int64_t* __restrict__ lb, const float* __restrict__ lam,
                                                          float eps, const float* __restrict__ lse,
                                                          const float* __restrict__ gout, const float* __restrict__ count,
                                                          int M, int V, int nrt, float* __restrict__ dH,
                                                          float* __restrict__ dW, float* __restrict__ db, int accumulate) {
  using namespace sce;
  constexpr int KS = C / 16, CT = C / 32, LD = C + 8;
  // the waves' staged operand tiles ([32][LD] bf16 each) in the loop, then the partial
  // accumulators of waves 1..3 ([3][32·C] fp32) for the merge
  __shared__ __attribute__((aligned(16))) float smem[3 * 32 * C];
  static_assert(NW * 32 * LD * 2 <= 3 * 32 * C * 4, "operand tiles fit the merge buffer");
  __shared__ float srv[NW][5][RT];
  __shared__ int sla[NW][2][RT];
  __shared__ float sdb[NW][RT];
  const int w = wave_id(), l = lane_id(), hh = l >> 5, rl = l & 31;
  uint16_t* img = reinterpret_cast<uint16_t*>(smem) + w * 32 * LD;
  const float g = gout[0] / fmaxf(count[0], 1.f);
  const float ninf = -__builtin_inff(), pinf = __builtin_inff();
  f32x16 acc[CT];
#pragma unroll
  for (int ct = 0; ct < CT; ++ct) acc[ct] = f32x16{};
  // one 32 × C bf16 tile, rows clamped to nrows − 1, into this wave's image
  auto stage = [&](const uint16_t* src, int r0, int nrows) {
#pragma unroll
    for (int i = 0; i < C / 16; ++i) {
      const int e = l + 64 * i, row = e / (C / 8), slot = e % (C / 8);
      const int r = min(r0 + row, nrows - 1);
      *reinterpret_cast<bf16x8*>(img + row * LD + 8 * slot) =
          *reinterpret_cast<const bf16x8*>(src + (long long)r * C + 8 * slot);
    }
  };
  if ((int)blockIdx.x < nrt) {
    // ---- dH of rows m0 .. m0 + 31 ----
    const int gr = blockIdx.x * RT + rl;
    const bool rin = gr < M;
    bf16x8 hb[KS];
#pragma unroll
    for (int s = 0; s < KS; ++s)
      hb[s] = *reinterpret_cast<const bf16x8*>(Hs + (long long)(rin ? gr : 0) * C + 16 * s + 8 * hh);
    const int a = rin ? (int)la[gr] : -100, b = rin ? (int)lb[gr] : 0;
    const bool ok = labels_ok(a, b, V);
    const float lm = rin ? lam[gr] : 1.f;
    const float lsl = ok ? lse[rin ? gr : 0] * kL2E : pinf;  // a row without a label: p = 2^−inf = 0
    const float gs = ok ? g : 0.f;
    const float cA = gs * (1.f - eps) * lm, cB = gs * (1.f - eps) * (1.f - lm), base = gs * eps / (float)V;
    const int ntiles = (V + 31) / 32, iters = (ntiles + NW - 1) / NW;
    for (int t = 0; t < iters; ++t) {
      const int v0 = (t * NW + w) * 32;
      stage(W, v0, V);
      __syncthreads();
      f32x16 st;
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int c = v0 + acc_row(i, hh);
        const float bv = bias[c < V ? c : 0];
        st[i] = c < V ? bv : ninf;
      }
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) st = mfma32(frag_kc(img, LD, 0, 16 * ks), hb[ks], st);
      f32x16 dz;
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int c = v0 + acc_row(i, hh);
        const float p = fast_exp2(fmaf(st[i], kL2E, -lsl));
        const float d = gs * p - (c == a ? cA : 0.f) - (c == b ? cB : 0.f) - base;
        dz[i] = c < V ? d : 0.f;
      }
      // dHᵀ[c][row] += Wᵀ[c][v]·dzᵀ[v][row]: the logits accumulator as the B operand
#pragma unroll
      for (int ss = 0; ss < 2; ++ss) {
        bf16x8 pb, pl;
        pack_hi_lo(dz, ss, pb, pl);
#pragma unroll
        for (int ct = 0; ct < CT; ++ct) {
          const bf16x8 wa = frag_ks_perm(img, LD, 32 * ct, 16 * ss);
          acc[ct] = mfma32(wa, pl, mfma32(wa, pb, acc[ct]));
        }
      }
      __syncthreads();
    }
    if (w > 0)
#pragma unroll
      for (int ct = 0; ct < CT; ++ct)
#pragma unroll
        for (int i = 0; i < 16; ++i) smem[((w - 1) * C + 32 * ct + acc_row(i, hh)) * 32 + rl] = acc[ct][i];
    __syncthreads();
    if (w == 0 && rin) {
#pragma unroll
      for (int ct = 0; ct < CT; ++ct)
#pragma unroll
        for (int q = 0; q < 4; ++q) {  // registers 4q .. 4q+3 = c 32ct + 8q + 4hh + 0..3
          float o[4];
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const int c = 32 * ct + 8 * q + 4 * hh + j;
            o[j] = ((acc[ct][4 * q + j] + smem[c * 32 + rl]) + smem[(C + c) * 32 + rl]) + smem[(2 * C + c) * 32 + rl];
          }
          *reinterpret_cast<float4*>(dH + (long long)gr * C + 32 * ct + 8 * q + 4 * hh) =
              make_float4(o[0], o[1], o[2], o[3]);
        }
    }
    return;
  }
  // ---- dW / db of classes v0 .. v0 + 31 over all rows ----
  const int v0 = ((int)blockIdx.x - nrt) * 32, vg = v0 + rl;
  const bool vin = vg < V;
  bf16x8 wb[KS];
#pragma unroll
  for (int s = 0; s < KS; ++s)
    wb[s] = *reinterpret_cast<const bf16x8*>(W + (long long)min(vg, V - 1) * C + 16 * s + 8 * hh);
  const float bnat = vin ? bias[vg] : ninf;
  float bsum = 0.f;
  const int iters = (nrt + NW - 1) / NW;
  for (int t = 0; t < iters; ++t) {
    const int r0 = (t * NW + w) * RT;  // past M: every row of the tile is masked
    stage(Hs, r0, M);
    if (l < RT) {
      const int r = r0 + l;
      const bool rin = r < M;
      const int a = rin ? (int)la[r] : -100, b = rin ? (int)lb[r] : 0;
      const bool ok = labels_ok(a, b, V);
      const float lm = rin ? lam[r] : 1.f;
      const float gs = ok ? g : 0.f;
      srv[w][0][l] = ok ? lse[rin ? r : 0] * kL2E : pinf;
      srv[w][1][l] = gs;
      srv[w][2][l] = gs * (1.f - eps) * lm;
      srv[w][3][l] = gs * (1.f - eps) * (1.f - lm);
      srv[w][4][l] = gs * eps / (float)V;
      sla[w][0][l] = ok ? a : -1;
      sla[w][1][l] = ok ? b : -1;
    }
    __syncthreads();
    f32x16 st;
#pragma unroll
    for (int i = 0; i < 16; ++i) st[i] = bnat;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) st = mfma32(frag_kc(img, LD, 0, 16 * ks), wb[ks], st);
    f32x16 dz;
#pragma unroll
    for (int i = 0; i < 16; ++i) {  // register i: row r0 + acc_row(i, hh); lane: class vg
      const int rr = acc_row(i, hh);
      const float p = fast_exp2(fmaf(st[i], kL2E, -srv[w][0][rr]));
      const float d = srv[w][1][rr] * p - (sla[w][0][rr] == vg ? srv[w][2][rr] : 0.f) -
                      (sla[w][1][rr] == vg ? srv[w][3][rr] : 0.f) - srv[w][4][rr];
      dz[i] = vin ? d : 0.f;
      bsum += dz[i];
    }
    // dW[v][c] += Σ_r dz[r][v]·H[r][c]: the dz accumulator as the A operand (Xᵀ·B)
#pragma unroll
    for (int ss = 0; ss < 2; ++ss) {
      bf16x8 pa, pl;
      pack_hi_lo(dz, ss, pa, pl);
#pragma unroll
      for (int ct = 0; ct < CT; ++ct) {
        const bf16x8 hf = frag_ks_perm(img, LD, 32 * ct, 16 * ss);
        acc[ct] = mfma32(pl, hf, mfma32(pa, hf, acc[ct]));
      }
    }
    __syncthreads();
  }
  bsum += __shfl_xor(bsum, 32);
  if (hh == 0) sdb[w][rl] = bsum;
  if (w > 0)
#pragma unroll
    for (int ct = 0; ct < CT; ++ct)
#pragma unroll
      for (int i = 0; i < 16; ++i) smem[((w - 1) * 32 + acc_row(i, hh)) * C + 32 * ct + rl] = acc[ct][i];
  __syncthreads();
  if (w != 0) return;
  // accumulator: row = class within the tile, col = lane & 31 = c within tile ct
#pragma unroll
  for (int ct = 0; ct < CT; ++ct)
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int vr = acc_row(i, hh), vv = v0 + vr;
      if (vv < V) {
        const int o = vr * C + 32 * ct + rl;
        const float val = ((acc[ct][i] + smem[o]) + smem[32 * C + o]) + smem[2 * 32 * C + o];
        float* p = dW + (long long)vv * C + 32 * ct + rl;
        *p = accumulate ? *p + val : val;
      }
    }
  if (hh == 0 && vin) {
    const float val = ((sdb[0][rl] + sdb[1][rl]) + sdb[2][rl]) + sdb[3][rl];
    db[vg] = accumulate ? db[vg] + val : val;
  }
}

// ---- batch mixing ---------------------------------------------------------------------------
// x (B, H, W, Ch) fp32 channels-last; mix = {mode, λ, y0, y1, x0, x1} as fp32 words in device
// memory (mode 0 off, 1 MixUp, 2 CutMix), read by the kernel: a replayed graph sees the staged
// words.  Workgroup row p handles the pair (p, B − 1 − p): both samples read once, both outputs
// written.  VEC consecutive elements per thread (VEC = 4 needs H·W·Ch a multiple of 4).
template <int VEC>
__global__ __launch_bounds__(256) void batch_mix_kernel(const float* __restrict__ x, const int64_t* __restrict__ y,
                                                        const float* __restrict__ mix, float* __restrict__ out,
                                                        int64_t* __restrict__ yb, float* __restrict__ lam_out, int B,
                                                        int Hh, int Wd, int Ch) {
  int mode = (int)mix[0];
  if (mode != 1 && mode != 2) mode = 0;
  const float lam = mix[1];
  const int y0 = (int)mix[2], y1 = (int)mix[3], x0 = (int)mix[4], x1 = (int)mix[5];
  if (blockIdx.x == 0 && blockIdx.y == 0)
    for (int k = threadIdx.x; k < B; k += blockDim.x) {
      yb[k] = mode ? y[B - 1 - k] : y[k];
      lam_out[k] = mode ? lam : 1.f;
    }
  const int n = Hh * Wd * Ch;
  const int i = blockIdx.y, j = B - 1 - i;
  const bool self = i == j || mode == 0;  // the middle sample of an odd batch pairs with itself
  const float* xi = x + (long long)i * n;
  const float* xj = x + (long long)j * n;
  float* oi = out + (long long)i * n;
  float* oj = out + (long long)j * n;
  const float om = 1.f - lam;
  for (int e = (blockIdx.x * blockDim.x + threadIdx.x) * VEC; e < n; e += gridDim.x * blockDim.x * VEC) {
    float a[VEC], b[VEC], ra[VEC], rb[VEC];
    if constexpr (VEC == 4) {
      const float4 va = *reinterpret_cast<const float4*>(xi + e), vb = *reinterpret_cast<const float4*>(xj + e);
      a[0] = va.x; a[1] = va.y; a[2] = va.z; a[3] = va.w;
      b[0] = vb.x; b[1] = vb.y; b[2] = vb.z; b[3] = vb.w;
    } else {
      a[0] = xi[e];
      b[0] = xj[e];
    }
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
      if (self) {
        ra[k] = a[k];
        rb[k] = b[k];
      } else if (mode == 1) {
        ra[k] = lam * a[k] + om * b[k];
        rb[k] = lam * b[k] + om * a[k];
      } else {
        const int pix = (e + k) / Ch, py = pix / Wd, px = pix - py * Wd;
        const bool in = py >= y0 && py < y1 && px >= x0 && px < x1;
        ra[k] = in ? b[k] : a[k];
        rb[k] = in ? a[k] : b[k];
      }
    }
    if constexpr (VEC == 4) {
      *reinterpret_cast<float4*>(oi + e) = make_float4(ra[0], ra[1], ra[2], ra[3]);
      if (i != j) *reinterpret_cast<float4*>(oj + e) = make_float4(rb[0], rb[1], rb[2], rb[3]);
    } else {
      oi[e] = ra[0];
      if (i != j) oj[e] = rb[0];
    }
  }
}

// ---- host side ----------------------------------------------------------------------------
int soft_ce_row_tiles(int M) { return (M + sce::RT - 1) / sce::RT; }

void soft_ce_fwd_launch(const SoftCeArgs& a, hipStream_t st) {
  const int nrt = soft_ce_row_tiles(a.M);
  const auto kernel = a.C == 64 ? soft_ce_fwd_kernel<64> : soft_ce_fwd_kernel<128>;
  hipLaunchKernelGGL(kernel, dim3(nrt), dim3(256), 0, st, a.H, a.W, a.bias, a.la, a.lb, a.lam, a.eps, a.M, a.V, a.lse,
                     a.pred, a.hs, a.blk, a.loss, a.count);
  if (nrt > 1) hipLaunchKernelGGL(soft_ce_finish_kernel, dim3(1), dim3(64), 0, st, a.blk, nrt, a.loss, a.count);
}

void soft_ce_bwd_launch(const SoftCeArgs& a, hipStream_t st) {
  const int nrt = soft_ce_row_tiles(a.M), nvt = (a.V + 31) / 32;
  const auto kernel = a.C == 64 ? soft_ce_bwd_kernel<64> : soft_ce_bwd_kernel<128>;
  hipLaunchKernelGGL(kernel, dim3(nrt + nvt), dim3(256), 0, st, a.hs, a.W, a.bias, a.la, a.lb, a.lam, a.eps, a.lse,
                     a.gout, a.count, a.M, a.V, nrt, a.dH, a.dW, a.db, a.accumulate);
}

void batch_mix_launch(const float* x, const int64_t* y, const float* mix, float* out, int64_t* yb, float* lam_out, int B,
                      int H, int W, int Ch, hipStream_t st) {
  const int n = H * W * Ch, pairs = (B + 1) / 2;
  if (n % 4 == 0) {
    const int bx = std::min(64, (n / 4 + 255) / 256);
    hipLaunchKernelGGL(batch_mix_kernel<4>, dim3(bx, pairs), dim3(256), 0, st, x, y, mix, out, yb, lam_out, B, H, W, Ch);
  } else {
    const int bx = std::min(64, (n + 255) / 256);
    hipLaunchKernelGGL(batch_mix_kernel<1>, dim3(bx, pairs), dim3(256), 0, st, x, y, mix, out, yb, lam_out, B, H, W, Ch);
  }
}

unsigned check_errors_soft_ce_head(bool reset) { return pio_read_errors(reset); }

}  // namespace pio
