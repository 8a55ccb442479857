// Vocabulary top-k head: the k largest logits of each row, their vocabulary indices and the row's
// log-sum-exp over the whole vocabulary, without writing a logit to memory (SURVEY K-16).
//
// Reference: the fill-mask utility (perceiver/utils.py:22-43) materialises the (n, L, V) logits of
// TextOutputAdapter (perceiver/adapter.py:166-173) and runs topk on the few [MASK] rows; the
// classifiers take an argmax of their logits.  Here only the requested rows are passed in.
//
//   vocab_topk_kernel    rows × vocab split, the geometry of the CE head's pass 1 (ce_head.hip):
//                        transposed logit tiles Sᵀ = W·Hᵀ (vocab on the accumulator rows, one query
//                        row per lane, the accumulator started at the bias, −inf past V) over
//                        double-buffered 64-entry W chunks.  Each lane keeps the KT best
//                        (value, index) pairs of its half of the row's logits in registers (a
//                        fully unrolled compare-and-shift insertion behind a wave-uniform ballot
//                        "some logit of this tile beats my KT-th") and a plain online (max, sum)
//                        for the lse; at the end of the split the two halves of a row are merged
//                        across lanes l and l ^ 32 and the split's candidates are stored.
//   vocab_topk_combine   one thread per row merges splits × KT sorted candidates into the final
//                        k and the splits' (max, sum) into the lse.
// Two launches, no tickets, no atomics: results are bitwise repeatable.
//
// Order: value descending, the lower vocabulary index first on exact ties.  A lane meets its
// logits in ascending vocabulary order (accumulator register i → row (i & 3) + 8(i >> 2) + 4h,
// tiles and chunks ascending), so its insertion needs only the strict value compare; the half
// merge and the split merge compare (value, index) pairs.
//
// LDS images are [64][C + 8] bf16 (a 16-byte pad per row): the k-contiguous ds_read_b128
// fragments of 16 consecutive rows then start 36 (C = 64) or 68 (C = 128) banks apart and cover
// all 64 banks once.
#include "common.h"
#include "head_common.h"

namespace pio {

namespace vtk {

constexpr int RB = 128;        // rows per workgroup (4 waves × 32)
constexpr int VC = 64;         // vocab entries per staged chunk
constexpr int kMaxSplits = 16; // vocab splits (grid.y) at most
constexpr int kMaxK = 8;
constexpr int kNoIndex = 0x7fffffff;  // index of an empty candidate slot (value −inf): loses every tie

__device__ __forceinline__ bool beats(float a, int ai, float b, int bi) { return a > b || (a == b && ai < bi); }

// (x, xi) into the descending list (tv, ti), the last entry dropped.  TIE = false: x enters
// behind equal values (the caller presents ascending indices).  Every index is a compile-time
// constant after unrolling: the lists stay in registers.
template <int KT, bool TIE>
__device__ __forceinline__ void insert(float (&tv)[KT], int (&ti)[KT], float x, int xi) {
#pragma unroll
  for (int j = KT - 1; j >= 0; --j) {
    const int jm = j > 0 ? j - 1 : 0;
    const bool b0 = TIE ? beats(x, xi, tv[j], ti[j]) : x > tv[j];
    const bool b1 = j > 0 && (TIE ? beats(x, xi, tv[jm], ti[jm]) : x > tv[jm]);
    tv[j] = b1 ? tv[jm] : (b0 ? x : tv[j]);
    ti[j] = b1 ? ti[jm] : (b0 ? xi : ti[j]);
  }
}

}  // namespace vtk

// grid (⌈M / 128⌉, splits); wave w: rows m0 + 32w + (l & 31), lane half h = l >> 5.  Per split:
// cand_v / cand_i [split][row][KT] = the split's best logits (natural units) and their vocabulary
// indices, part_ml[split][row] = (max, sum) in log2 units.
template <int C, int KT>
__global__ __launch_bounds__(256) void vocab_topk_kernel(const float* __restrict__ Hm, const int64_t* __restrict__ hidx,
                                                         long long R, const uint16_t* __restrict__ W,
                                                         const float* __restrict__ bias, int M, int V,
                                                         int chunks_per_split, float* __restrict__ cand_v,
                                                         int* __restrict__ cand_i, float2* __restrict__ part_ml) {
  using namespace vtk;
  constexpr int LD = C + 8;       // LDS row pitch (bf16 elements)
  constexpr int KS = C / 16;      // MFMA steps of the K-loop
  constexpr int SL = C / 8;       // 16-byte slots per vocab row
  constexpr int NP = VC * SL / 256;  // staged 16-byte pieces per thread
  __shared__ __attribute__((aligned(16))) uint16_t sW[2][VC * LD];
  __shared__ __attribute__((aligned(16))) float sB[2][VC];  // bias (−inf past V): the logit accumulators' initial value
  const int w = wave_id(), l = lane_id(), hh = l >> 5;
  const int m0 = blockIdx.x * RB, split = blockIdx.y;
  const int nchunks = (V + VC - 1) / VC;
  const int c_begin = split * chunks_per_split, c_end = min(nchunks, c_begin + chunks_per_split);
  const int gr = m0 + 32 * w + (l & 31);
  const bool rin = gr < M;
  // this lane's half row (c = 16s + 8hh .. + 7) as the B operand of Sᵀ = W·Hᵀ, gathered from the
  // fp32 hidden state and cast on load
  bf16x8 hb[KS];
  {
    long long src = hidx ? hidx[rin ? gr : 0] : (long long)(rin ? gr : 0);
#if PIO_CHECKS
    if (src < 0 || src >= R) {
      if (rin && split == 0 && hh == 0) pio_flag(kErrGatherRow);
      src = src < 0 ? 0 : R - 1;
    }
#else
    (void)R;
#endif
    load_row_operand(hb, Hm + src * C + 8 * hh, rin);
  }
  // chunk staging: 64 vocab rows × SL slots of 16 bytes, NP per thread (+ the bias)
  bf16x8 wr[NP];
  float bnext = 0.f;
  auto fetch = [&](int c) {
#pragma unroll
    for (int i = 0; i < NP; ++i) {
      const int e = threadIdx.x + 256 * i, v = c * VC + e / SL;
      wr[i] = *reinterpret_cast<const bf16x8*>(v < V ? W + (long long)v * C + 8 * (e % SL)
                                                     : reinterpret_cast<const uint16_t*>(kZero32B));
    }
    const int v = c * VC + (threadIdx.x & (VC - 1));
    const float bv = bias[v < V ? v : 0];  // unconditional load (address select)
    bnext = v < V ? bv : -__builtin_inff();
  };
  auto stage = [&](int buf) {
#pragma unroll
    for (int i = 0; i < NP; ++i) {
      const int e = threadIdx.x + 256 * i;
      *reinterpret_cast<bf16x8*>(&sW[buf][(e / SL) * LD + 8 * (e % SL)]) = wr[i];
    }
    if (threadIdx.x < VC) sB[buf][threadIdx.x] = bnext;
  };
  float tv[KT];
  int ti[KT];
#pragma unroll
  for (int j = 0; j < KT; ++j) { tv[j] = -__builtin_inff(); ti[j] = kNoIndex; }
  float m_run = -__builtin_inff(), l_run = 0.f;  // log2 units
  if (c_begin < c_end) {
    fetch(c_begin);
    stage(0);
  }
  lds_sync();
  for (int c = c_begin; c < c_end; ++c) {
    const int buf = (c - c_begin) & 1;
    if (c + 1 < c_end) fetch(c + 1);  // in flight under this chunk's MFMAs
    const uint16_t* img = sW[buf];
#pragma unroll
    for (int vb = 0; vb < 2; ++vb) {  // two 32-vocab blocks per chunk
      // register i: vocab c·64 + 32vb + acc_row(i, hh); the accumulator starts at the bias
      f32x16 st = bias_acc(sB[buf] + 32 * vb + 4 * hh);
#pragma unroll
      for (int s = 0; s < KS; ++s) st = mfma32(frag_kc(img, LD, 32 * vb, 16 * s), hb[s], st);
      float mx = st[0];
#pragma unroll
      for (int i = 1; i < 16; ++i) mx = fmaxf(mx, st[i]);
      // running top-KT: only a tile holding a logit above some lane's KT-th enters the insertion
      if (__ballot(mx > tv[KT - 1])) {
        const int v0 = c * VC + 32 * vb + 4 * hh;
#pragma unroll
        for (int i = 0; i < 16; ++i) insert<KT, false>(tv, ti, st[i], v0 + (i & 3) + 8 * (i >> 2));
      }
      // online (max, sum); a half tile of padding only (mx = −inf) adds nothing
      const float mn = fmaxf(m_run, mx * kL2E);
      const float ms = mn == -__builtin_inff() ? 0.f : mn;
      float ps = 0.f;
#pragma unroll
      for (int i = 0; i < 16; ++i) ps += fast_exp2(fmaf(st[i], kL2E, -ms));
      l_run = fmaf(l_run, fast_exp2(m_run - ms), ps);
      m_run = mn;
    }
    if (c + 1 < c_end) stage(buf ^ 1);
    lds_sync();
  }
  // the two halves of a row (lanes l and l ^ 32) merged: both lanes end with the row's list
  {
    float ov[KT];
    int oi[KT];
#pragma unroll
    for (int j = 0; j < KT; ++j) { ov[j] = __shfl_xor(tv[j], 32); oi[j] = __shfl_xor(ti[j], 32); }
#pragma unroll
    for (int j = 0; j < KT; ++j) insert<KT, true>(tv, ti, ov[j], oi[j]);
    const float om = __shfl_xor(m_run, 32), ol = __shfl_xor(l_run, 32);
    merge_ml(m_run, l_run, om, ol);
  }
  if (rin && hh == 0) {
    const long long o = (long long)split * M + gr;
#pragma unroll
    for (int j = 0; j < KT; ++j) { cand_v[o * KT + j] = tv[j]; cand_i[o * KT + j] = ti[j]; }
    part_ml[o] = make_float2(m_run, l_run);
  }
}

// one thread per row: the splits' sorted candidates merged into the final k, the (max, sum)
// pairs into the lse (natural units)
template <int KT>
__global__ __launch_bounds__(256) void vocab_topk_combine_kernel(const float* __restrict__ cand_v,
                                                                 const int* __restrict__ cand_i,
                                                                 const float2* __restrict__ part_ml, int nsplit, int M,
                                                                 int V, int k, float* __restrict__ values,
                                                                 int64_t* __restrict__ indices, float* __restrict__ lse) {
  using namespace vtk;
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= M) return;
  float tv[KT];
  int ti[KT];
#pragma unroll
  for (int j = 0; j < KT; ++j) { tv[j] = -__builtin_inff(); ti[j] = kNoIndex; }
  float m = -__builtin_inff(), ls = 0.f;
  for (int s = 0; s < nsplit; ++s) {
    const long long o = (long long)s * M + r;
    float cv[KT];
    int ci[KT];
#pragma unroll
    for (int j = 0; j < KT; ++j) { cv[j] = cand_v[o * KT + j]; ci[j] = cand_i[o * KT + j]; }
    const float2 ml = part_ml[o];
#pragma unroll
    for (int j = 0; j < KT; ++j) insert<KT, true>(tv, ti, cv[j], ci[j]);
    merge_ml(m, ls, ml.x, ml.y);
  }
#pragma unroll
  for (int j = 0; j < KT; ++j)
    if (j < k) {
      values[(long long)r * k + j] = tv[j];
      indices[(long long)r * k + j] = (int64_t)min(ti[j], V - 1);  // an empty slot (k ≤ V: NaN logits only)
    }
  lse[r] = (m + __log2f(ls)) * kLN2;
}

// ---- host side --------------------------------------------------------------------------
int vocab_topk_splits(int M, int V) { return vocab_splits(M, V, vtk::RB, vtk::VC, vtk::kMaxSplits); }
int vocab_topk_kt(int k) { return k <= 1 ? 1 : (k <= 4 ? 4 : vtk::kMaxK); }

template <int C, int KT>
static void vocab_topk_run(const VocabTopkArgs& a, hipStream_t st) {
  const int nchunks = (a.V + vtk::VC - 1) / vtk::VC;
  const int cps = (nchunks + a.nsplit - 1) / a.nsplit;
  float2* part_ml = reinterpret_cast<float2*>(a.part_ml);
  hipLaunchKernelGGL((vocab_topk_kernel<C, KT>), dim3((a.M + vtk::RB - 1) / vtk::RB, a.nsplit), dim3(256), 0, st, a.H,
                     a.hidx, a.R, a.W, a.bias, a.M, a.V, cps, a.cand_v, a.cand_i, part_ml);
  hipLaunchKernelGGL((vocab_topk_combine_kernel<KT>), dim3((a.M + 255) / 256), dim3(256), 0, st, a.cand_v, a.cand_i,
                     part_ml, a.nsplit, a.M, a.V, a.k, a.values, a.indices, a.lse);
}

void vocab_topk_launch(const VocabTopkArgs& a, hipStream_t st) {
  const int kt = vocab_topk_kt(a.k);
#define PIO_VTK(CC, KK) \
  if (a.C == CC && kt == KK) return vocab_topk_run<CC, KK>(a, st)
  PIO_VTK(64, 1);
  PIO_VTK(64, 4);
  PIO_VTK(64, 8);
  PIO_VTK(128, 1);
  PIO_VTK(128, 4);
  PIO_VTK(128, 8);
#undef PIO_VTK
}

unsigned check_errors_topk_head(bool reset) { return pio_read_errors(reset); }

}  // namespace pio
