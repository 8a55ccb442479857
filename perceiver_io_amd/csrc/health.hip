// Training health on the flat parameter space (ops/optim.py FusedAdamW skip_nonfinite / tensor_stats):
// the step guard that keeps a non-finite gradient out of the weights of a replayed step, and
// per-tensor gradient / weight statistics (the trainer's track_grad_norm).
//
//   step_guard_kernel          one workgroup, between sumsq and the update: sums sumsq's partials in
//                              opt_clip_scale's order (optim_common.h opt_sumsq_total), decides "skip"
//                              and writes the optimizer's 8 guard words (layout: optim_common.h)
//   tensor_stats_kernel        at most 2048 workgroups walk the chunk table grid-stride and write four
//                              partials per chunk: Σg², Σw², max|g|, non-finite gradient elements
//   tensor_stats_reduce_kernel one workgroup per tensor sums its chunks' partials (fp64, fixed order)
//                              → (T, 4) fp32 = ‖g‖·gscale, ‖w‖, max|g|·gscale, non-finite count
// The two statistics kernels return before any load unless hyper[6] ("statistics due") is set or the
// guard flags this step; a flagged step's rows go to a second buffer, so the tensors that carried the
// non-finite values stay readable until the next skipped step.  They run between step_guard and the
// update, while g and w are still this step's.  No atomics, fixed summation orders: bitwise repeatable.
//
// Reference parity: track_grad_norm                                  scripts/trainer.yaml:30
// (the skip has no counterpart in the reference: eager recipes get it from torch.cuda.amp.GradScaler)
#include "optim_common.h"

// wave_sum / wave_max (common.h) use the gfx950 lane swaps: no other target.
#if defined(__HIP_DEVICE_COMPILE__) && !defined(__gfx950__)
#error "this translation unit's cross-lane reductions are written for gfx950 (MI355X) only"
#endif

namespace pio {

// "Not finite" is read off the exponent bits of Σ g² (opt_nonfinite), not isfinite().  A gradient
// whose elements are all finite but whose Σ g² overflows fp32 (‖g‖ ≳ 1.8e19) gives Σ = inf and counts
// as non-finite too: its norm, and with it the clip factor, could not be formed either.
// One wave; thread 0 reads the previous words and writes the new ones (two 16-byte vector stores).
__global__ __launch_bounds__(64) void step_guard_kernel(const float* __restrict__ part, const float* __restrict__ hyper,
                                                        float* __restrict__ guard, float gscale) {
  const float sum = opt_sumsq_total(part);
  if (threadIdx.x != 0) return;
  const float4 a = reinterpret_cast<const float4*>(guard)[0], b = reinterpret_cast<const float4*>(guard)[1];
  const float step = hyper[1], total = a.y, consecutive = a.z, last_finite = b.y, last_skipped = b.z;
  const bool skip = opt_nonfinite(sum);
  const float norm = sqrtf(sum) * gscale;
  const float4 na = make_float4(skip ? 1.f : 0.f, skip ? total + 1.f : total, skip ? consecutive + 1.f : 0.f, step - total);
  const float4 nb = make_float4(norm, skip ? last_finite : norm, skip ? step : last_skipped, 0.f);
  reinterpret_cast<float4*>(guard)[0] = na;
  reinterpret_cast<float4*>(guard)[1] = nb;
}

// run this step?  due: hyper[6]; skip: the guard's flag.  Uniform over both launches.
struct StatsGate {
  bool due, skip;
};
__device__ __forceinline__ StatsGate stats_gate(const float* __restrict__ hyper, const float* __restrict__ guard) {
  return StatsGate{hyper[6] != 0.f, opt_guard_skip(guard)};
}

// 256 threads × float4, every load of a chunk in flight before the arithmetic (adamw_grouped_kernel's
// walk): an HBM-bound read of g and w.  The scalar tail covers len % 4; padding belongs to no chunk
// and is never read.  A chunk that fails opt_chunk's validation is skipped (its partials are zeros)
// and flags kErrOptTable.  max|g| ignores NaN elements (fmaxf); the count tells of them.
__global__ __launch_bounds__(256) void tensor_stats_kernel(const float* __restrict__ g, const float* __restrict__ w,
                                                           long long n, const float* __restrict__ hyper,
                                                           const float* __restrict__ guard,
                                                           const long long* __restrict__ chunks, long long C, int T,
                                                           float* __restrict__ part) {
  const StatsGate gate = stats_gate(hyper, guard);
  if (!gate.due && !gate.skip) return;
  __shared__ float red[4][4];
  for (long long c = blockIdx.x; c < C; c += gridDim.x) {  // uniform over the block
    const OptChunk k = opt_chunk(chunks, c, n, T);
    if (!k.ok && threadIdx.x == 0) pio_flag(kErrOptTable);
    float sg = 0.f, sw = 0.f, mx = 0.f, bad = 0.f;
    const int len4 = k.len >> 2;  // 0 for an entry that does not fit
    const float4* g4 = reinterpret_cast<const float4*>(g + (k.ok ? k.start : 0));
    const float4* w4 = reinterpret_cast<const float4*>(w + (k.ok ? k.start : 0));
    float4 G[kOptIter], W[kOptIter];
#pragma unroll
    for (int j = 0; j < kOptIter; ++j) {
      const int i = threadIdx.x + 256 * j;
      if (i < len4) {
        G[j] = g4[i];
        W[j] = w4[i];
      }
    }
#pragma unroll
    for (int j = 0; j < kOptIter; ++j) {
      const int i = threadIdx.x + 256 * j;
      if (i < len4) {
        const float ga[4] = {G[j].x, G[j].y, G[j].z, G[j].w}, wa[4] = {W[j].x, W[j].y, W[j].z, W[j].w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          sg = fmaf(ga[e], ga[e], sg);
          sw = fmaf(wa[e], wa[e], sw);
          mx = fmaxf(mx, fabsf(ga[e]));
          bad += opt_nonfinite(ga[e]) ? 1.f : 0.f;
        }
      }
    }
    const int t = (len4 << 2) + threadIdx.x;
    if (t < k.len) {
      const float g0 = g[k.start + t], w0 = w[k.start + t];
      sg = fmaf(g0, g0, sg);
      sw = fmaf(w0, w0, sw);
      mx = fmaxf(mx, fabsf(g0));
      bad += opt_nonfinite(g0) ? 1.f : 0.f;
    }
    sg = wave_sum(sg);
    sw = wave_sum(sw);
    mx = wave_max(mx);
    bad = wave_sum(bad);  // ≤ 4096 per chunk: exact in fp32
    if (lane_id() == 0) {
      red[0][wave_id()] = sg;
      red[1][wave_id()] = sw;
      red[2][wave_id()] = mx;
      red[3][wave_id()] = bad;
    }
    __syncthreads();
    if (threadIdx.x == 0)
      reinterpret_cast<float4*>(part)[c] =
          make_float4((red[0][0] + red[0][1]) + (red[0][2] + red[0][3]), (red[1][0] + red[1][1]) + (red[1][2] + red[1][3]),
                      fmaxf(fmaxf(red[2][0], red[2][1]), fmaxf(red[2][2], red[2][3])),
                      (red[3][0] + red[3][1]) + (red[3][2] + red[3][3]));
    __syncthreads();  // red is reused by the block's next chunk
  }
}

// thread-strided fp64 sums and a fixed LDS tree, as lamb_trust_kernel's.  The row goes to `stats`
// when the statistics are due and to `skip_stats` when the guard flags the step (both when both).
// The count is exact up to 2^24 non-finite elements per tensor.
__global__ __launch_bounds__(256) void tensor_stats_reduce_kernel(const float* __restrict__ part,
                                                                  const int* __restrict__ tensors, long long C,
                                                                  const float* __restrict__ hyper,
                                                                  const float* __restrict__ guard, float gscale,
                                                                  float* __restrict__ stats,
                                                                  float* __restrict__ skip_stats) {
  const StatsGate gate = stats_gate(hyper, guard);
  if (!gate.due && !gate.skip) return;
  __shared__ double red[3][256];
  __shared__ float redm[256];
  const int t = blockIdx.x;
  const long long first = tensors[2 * t], cnt = tensors[2 * t + 1];
  if (first < 0 || cnt < 0 || first + cnt > C) {  // uniform over the block
    if (threadIdx.x == 0) pio_flag(kErrOptTable);
    return;
  }
  double sg = 0.0, sw = 0.0, bad = 0.0;
  float mx = 0.f;
  for (long long i = threadIdx.x; i < cnt; i += 256) {
    const float4 q = reinterpret_cast<const float4*>(part)[first + i];
    sg += (double)q.x;
    sw += (double)q.y;
    mx = fmaxf(mx, q.z);
    bad += (double)q.w;
  }
  red[0][threadIdx.x] = sg;
  red[1][threadIdx.x] = sw;
  red[2][threadIdx.x] = bad;
  redm[threadIdx.x] = mx;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) {
      red[0][threadIdx.x] += red[0][threadIdx.x + s];
      red[1][threadIdx.x] += red[1][threadIdx.x + s];
      red[2][threadIdx.x] += red[2][threadIdx.x + s];
      redm[threadIdx.x] = fmaxf(redm[threadIdx.x], redm[threadIdx.x + s]);
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const float4 row = make_float4(sqrtf((float)red[0][0]) * gscale, sqrtf((float)red[1][0]), redm[0] * gscale,
                                   (float)red[2][0]);
    if (gate.due) reinterpret_cast<float4*>(stats)[t] = row;
    if (gate.skip && skip_stats != nullptr) reinterpret_cast<float4*>(skip_stats)[t] = row;
  }
}

// part: kSumsqBlocks fp32, hyper: ≥ 8 fp32, guard: kGuardWords fp32, 16-byte aligned (checked by the binding)
void step_guard_launch(const float* part, const float* hyper, float* guard, float gscale, hipStream_t st) {
  hipLaunchKernelGGL(step_guard_kernel, dim3(1), dim3(64), 0, st, part, hyper, guard, gscale);
}

// g, w, part, stats, skip_stats 16-byte aligned (checked by the binding); C chunks, T tensors.  At most
// 2048 workgroups (8 per CU) walk the chunks.
void tensor_stats_launch(const float* g, const float* w, long long n, const float* hyper, const float* guard,
                         const long long* chunks, long long C, const int* tensors, int T, float gscale, float* part,
                         float* stats, float* skip_stats, hipStream_t st) {
  if (C <= 0 || T <= 0) return;
  const unsigned blocks = (unsigned)(C < 2048 ? C : 2048);
  hipLaunchKernelGGL(tensor_stats_kernel, dim3(blocks), dim3(256), 0, st, g, w, n, hyper, guard, chunks, C, T, part);
  hipLaunchKernelGGL(tensor_stats_reduce_kernel, dim3((unsigned)T), dim3(256), 0, st, part, tensors, C, hyper, guard,
                     gscale, stats, skip_stats);
}

unsigned check_errors_health(bool reset) { return pio_read_errors(reset); }

}  // namespace pio
