// Selected-position bookkeeping for the MLM loss (replaces ~15 small framework kernels)
//   rows  : per sequence b, slots [0, cap): positions of labels != -100 in order (unused
//           slots → slot mod L, label −100), count[b]
//   global: the valid slots of all sequences compacted into gcap rows for the vocab GEMMs
//           (unused → slot 0 with label −100), total = Σ count (the mean's denominator)
//
// select_rows: workgroup b compacts sequence b.  select_global, workgroup (b, 0): finds sequence
// b's offset in the global rows from all the per-sequence counts (each workgroup scans them
// itself: no grid-wide hand-off) and writes its valid slots; workgroup (0, 0) also writes the
// totals, the last one the unused tail.  Every workgroup (b, y) also copies the output-query rows
// q[b, j] = P[idx_b[b, j]] of its kSelSlots slots (the gather of the decoder's query array,
// spread over the whole grid).
#include "common.h"

namespace pio {

constexpr int kSelThreads = 1024;
constexpr int kSelSlots = 128;  // query-gather slots per select_global workgroup
__global__ __launch_bounds__(kSelThreads) void select_rows_kernel(const int64_t* __restrict__ labels, int L, int cap,
                                                                  int64_t* __restrict__ idx_b, int64_t* __restrict__ lab_b,
                                                                  int* __restrict__ count) {
  __shared__ int sW[kSelThreads / 64], sOff;
  const int b = blockIdx.x, w = wave_id(), l = lane_id(), nw = blockDim.x >> 6;
  if (threadIdx.x == 0) sOff = 0;
  lds_sync();
  for (int c0 = 0; c0 < L; c0 += blockDim.x) {
    const int i = c0 + threadIdx.x;
    const int64_t lab = i < L ? labels[(long long)b * L + i] : -100;
    const bool sel = lab != -100;
    const uint64_t m = __ballot(sel);
    const int pre = __popcll(m & ((1ull << l) - 1ull));
    if (l == 0) sW[w] = __popcll(m);
    lds_sync();
    int woff = 0, tot = 0;
    for (int k = 0; k < nw; ++k) {
      woff += k < w ? sW[k] : 0;
      tot += sW[k];
    }
    const int pos = sOff + woff + pre;
    if (sel && pos < cap) {
      idx_b[(long long)b * cap + pos] = i;
      lab_b[(long long)b * cap + pos] = lab;
    }
    lds_sync();
    if (threadIdx.x == 0) sOff += tot;
    lds_sync();
  }
  const int cnt = sOff;
  for (int j = (cnt < cap ? cnt : cap) + threadIdx.x; j < cap; j += blockDim.x) {
    idx_b[(long long)b * cap + j] = j % L;
    lab_b[(long long)b * cap + j] = -100;
  }
  if (threadIdx.x == 0) count[b] = cnt;
}

__device__ __forceinline__ int wave_isum(int v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
  return v;
}

__global__ __launch_bounds__(256) void select_global_kernel(const int* __restrict__ count, int B, int cap,
                                                            const int64_t* __restrict__ lab_b, int gcap,
                                                            int64_t* __restrict__ gidx, int64_t* __restrict__ glab,
                                                            float* __restrict__ total, bool* __restrict__ overflow,
                                                            bool* __restrict__ sticky, const int64_t* __restrict__ idx_b,
                                                            const float* __restrict__ P, int C, float* __restrict__ q) {
  __shared__ int sRed[4][4];
  __shared__ long long sI[kSelSlots];
  const int b = blockIdx.x, w = wave_id(), l = lane_id();
  if (q != nullptr) {  // slots [kSelSlots·y, +kSelSlots) of sequence b: q[b, j] = P[idx_b[b, j]]
    const int C4 = C >> 2, j0 = blockIdx.y * kSelSlots, nj = min(cap - j0, kSelSlots);
    const float4* P4 = reinterpret_cast<const float4*>(P);
    float4* q4 = reinterpret_cast<float4*>(q) + ((long long)b * cap + j0) * C4;
    for (int j = threadIdx.x; j < nj; j += blockDim.x) sI[j] = idx_b[(long long)b * cap + j0 + j];
    __syncthreads();
    for (int e0 = 0; e0 < nj * C4; e0 += 8 * 256) {  // eight independent row loads in flight per thread
      float4 v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int e = e0 + u * 256 + threadIdx.x;
        if (e < nj * C4) {
          const int j = e / C4;
          v[u] = P4[sI[j] * C4 + (e - j * C4)];
        }
      }
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int e = e0 + u * 256 + threadIdx.x;
        if (e < nj * C4) q4[e] = v[u];
      }
    }
  }
  if (blockIdx.y != 0) return;
  int pre = 0, used = 0, all = 0, ovf = 0;
  for (int i = threadIdx.x; i < B; i += blockDim.x) {
    const int c = count[i], n = c < cap ? c : cap;
    pre += i < b ? n : 0;
    used += n;
    all += c;
    ovf += c > cap ? 1 : 0;
  }
  pre = wave_isum(pre); used = wave_isum(used); all = wave_isum(all); ovf = wave_isum(ovf);
  if (l == 0) { sRed[0][w] = pre; sRed[1][w] = used; sRed[2][w] = all; sRed[3][w] = ovf; }
  __syncthreads();
  pre = sRed[0][0] + sRed[0][1] + sRed[0][2] + sRed[0][3];
  used = sRed[1][0] + sRed[1][1] + sRed[1][2] + sRed[1][3];
  const int c = count[b], n = c < cap ? c : cap;
  for (int j = threadIdx.x; j < n; j += blockDim.x) {
    const int g = pre + j;
    if (g < gcap) {
      const long long s = (long long)b * cap + j;
      gidx[g] = s;
      glab[g] = lab_b[s];
    }
  }
  if (b == B - 1)
    for (int g = (used < gcap ? used : gcap) + threadIdx.x; g < gcap; g += blockDim.x) {
      gidx[g] = 0;
      glab[g] = -100;
    }
  if (b == 0 && threadIdx.x == 0) {
    const bool o = (sRed[3][0] + sRed[3][1] + sRed[3][2] + sRed[3][3]) > 0 || used > gcap;
    total[0] = (float)(sRed[2][0] + sRed[2][1] + sRed[2][2] + sRed[2][3]);
    overflow[0] = o;
    if (sticky != nullptr && o) sticky[0] = true;  // the persistent per-device flag (never cleared here)
  }
}

void mlm_select_launch(const int64_t* labels, int B, int L, int cap, int gcap, int64_t* idx_b, int64_t* lab_b,
                       int* count, int64_t* gidx, int64_t* glab, float* total, bool* overflow, bool* sticky,
                       const float* P, int C, float* q, hipStream_t st) {
  hipLaunchKernelGGL(select_rows_kernel, dim3(B), dim3(kSelThreads), 0, st, labels, L, cap, idx_b, lab_b, count);
  const int gy = q ? (cap + kSelSlots - 1) / kSelSlots : 1;
  hipLaunchKernelGGL(select_global_kernel, dim3(B, gy), dim3(256), 0, st, count, B, cap, lab_b, gcap, gidx, glab, total,
                     overflow, sticky, idx_b, P, C, q);
}

unsigned check_errors_mlm_select(bool reset) { return pio_read_errors(reset); }

}  // namespace pio
