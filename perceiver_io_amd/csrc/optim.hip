// The optimizer step over the flat parameter space (ops/optim.py FlatParameterSpace, FusedAdamW):
// replica fold, gradient sum of squares, fused AdamW — single group (scalar and float4) and
// per-group over the chunk table.
//
// Reference parity:
//   AdamW (torch.optim defaults, decoupled wd)           scripts/cli.py:43, lightning.py:44-55 (SURVEY K-15)
// MI355X notes: one launch each, 16-byte accesses on the streaming paths.  AdamW reads its
// hyper-parameters (lr, step, grad-norm clip factor) from device memory so the whole optimizer step
// can be captured in a hipGraph, and writes the bf16 weight shadow that the GEMM kernels consume in
// the same pass.  The step prologue, the chunk table and the per-element update are shared with
// lamb.hip (optim_common.h); this translation unit keeps the default -ffp-contract=fast.
#include "optim_common.h"

namespace pio {

// sum of squares of the flat gradient (clip_grad_norm): Σ g² in fixed order, no atomics: block b writes its partial to part[b] (kSumsqBlocks blocks,
// grid-stride, 8 independent 16-byte loads in flight per thread); the update kernels sum the
// partials themselves (opt_clip_scale).  The previous single-address atomic per block put
// 2048 serialised adds at the end of an HBM-bound pass (36 µs for the 68 MB LArTPC gradient).
__global__ __launch_bounds__(256) void sumsq_kernel(const float* __restrict__ g, long long n, float* __restrict__ part) {
  float s[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  const long long n4 = ((reinterpret_cast<uintptr_t>(g) & 15) == 0) ? n >> 2 : 0;
  const long long stride = (long long)gridDim.x * blockDim.x;
  const float4* g4 = reinterpret_cast<const float4*>(g);
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  for (; i + 7 * stride < n4; i += 8 * stride) {
    float4 a[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) a[k] = g4[i + k * stride];
#pragma unroll
    for (int k = 0; k < 8; ++k)
      s[k] = fmaf(a[k].x, a[k].x, fmaf(a[k].y, a[k].y, fmaf(a[k].z, a[k].z, fmaf(a[k].w, a[k].w, s[k]))));
  }
  for (; i < n4; i += stride) {
    const float4 a = g4[i];
    s[0] = fmaf(a.x, a.x, fmaf(a.y, a.y, fmaf(a.z, a.z, fmaf(a.w, a.w, s[0]))));
  }
  for (long long j = (n4 << 2) + (long long)blockIdx.x * blockDim.x + threadIdx.x; j < n; j += stride) {
    const float v = g[j];
    s[1] = fmaf(v, v, s[1]);
  }
  float t = ((s[0] + s[1]) + (s[2] + s[3])) + ((s[4] + s[5]) + (s[6] + s[7]));
  t = wave_sum(t);
  __shared__ float red[4];
  if (lane_id() == 0) red[wave_id()] = t;
  __syncthreads();
  if (threadIdx.x == 0) part[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

// what AdamW derives from a step's global words (optim_common.h opt_step): the arguments of
// adamw_elem that do not depend on the parameter group
struct AdamStep {
  float gs, beta1, omb1, beta2, omb2, bc1, bc2s;
  bool skip;  // the step guard flags this step: clear the gradient (zero_g), touch nothing else
};
__device__ __forceinline__ AdamStep adam_step(const float* __restrict__ hyper, float clip, float gscale,
                                              const float* __restrict__ loss_src, float* __restrict__ loss_ring,
                                              int ring_n, const float* __restrict__ norm_part,
                                              const float* __restrict__ guard) {
  const OptStep s = opt_step(hyper, clip, gscale, loss_src, loss_ring, ring_n, norm_part, guard);
  return AdamStep{s.gs, s.beta1, 1.f - s.beta1, s.beta2, 1.f - s.beta2, 1.f - powf(s.beta1, s.step),
                  sqrtf(1.f - powf(s.beta2, s.step)), s.skip};
}

// zero_g: the gradient is cleared as it is consumed (a replayed step then needs no separate
// zero fill of the flat gradient buffer before its backward)
// guard (null = off): the step guard's words (optim_common.h).  On a step it flags, the loss still
// reaches the ring and the gradient is still cleared (zero_g) — the poison must not stay in the
// accumulator for the next backward — while p, m, v and the shadow are left as they are; on the other
// steps the bias corrections take the guard's effective step.
__global__ void adamw_kernel(float* __restrict__ p, float* __restrict__ g, float* __restrict__ m,
                             float* __restrict__ v, uint16_t* __restrict__ shadow, long long n,
                             const float* __restrict__ hyper, float eps, float wd, float clip, float gscale,
                             int l2, int zero_g, const float* __restrict__ loss_src, float* __restrict__ loss_ring,
                             int ring_n, const float* __restrict__ norm_part, const float* __restrict__ guard) {
  const AdamStep s = adam_step(hyper, clip, gscale, loss_src, loss_ring, ring_n, norm_part, guard);
  if (s.skip) {  // uniform over the launch
    if (zero_g)
      for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x)
        g[i] = 0.f;
    return;
  }
  const float lr = hyper[0], step_size = lr / s.bc1, decay = fmaf(-wd, lr, 1.f);
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
    const float g0 = g[i];
    if (zero_g) g[i] = 0.f;
    float pi, mi, vi;
    adamw_elem(p[i], g0, m[i], v[i], s.gs, wd, decay, s.beta1, s.omb1, s.beta2, s.omb2, step_size, s.bc2s, eps, l2, pi, mi,
               vi);
    m[i] = mi;
    v[i] = vi;
    p[i] = pi;
    if (shadow) shadow[i] = f2bf(pi);
  }
}

// the same update on 4 elements per thread (16-byte loads / stores; every pointer 16-byte
// aligned, the shadow 8-byte aligned, n % 4 == 0 — checked by the launcher): a quarter of the
// memory instructions of the scalar loop, which is issue-bound at ≈40 % of HBM bandwidth
__global__ __launch_bounds__(256) void adamw4_kernel(float4* __restrict__ p, float4* __restrict__ g,
                                                     float4* __restrict__ m, float4* __restrict__ v,
                                                     uint2* __restrict__ shadow, long long n4,
                                                     const float* __restrict__ hyper, float eps, float wd, float clip,
                                                     float gscale, int l2, int zero_g, const float* __restrict__ loss_src,
                                                     float* __restrict__ loss_ring, int ring_n,
                                                     const float* __restrict__ norm_part,
                                                     const float* __restrict__ guard) {
  const AdamStep s = adam_step(hyper, clip, gscale, loss_src, loss_ring, ring_n, norm_part, guard);
  if (s.skip) {  // uniform over the launch
    if (zero_g)
      for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long long)gridDim.x * blockDim.x)
        g[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    return;
  }
  const float lr = hyper[0], step_size = lr / s.bc1, decay = fmaf(-wd, lr, 1.f);
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long long)gridDim.x * blockDim.x) {
    const float4 p4 = p[i], g4 = g[i], m4 = m[i], v4 = v[i];
    if (zero_g) g[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    const float pa[4] = {p4.x, p4.y, p4.z, p4.w}, ga[4] = {g4.x, g4.y, g4.z, g4.w};
    const float ma[4] = {m4.x, m4.y, m4.z, m4.w}, va[4] = {v4.x, v4.y, v4.z, v4.w};
    float po[4], mo[4], vo[4];
#pragma unroll
    for (int e = 0; e < 4; ++e)
      adamw_elem(pa[e], ga[e], ma[e], va[e], s.gs, wd, decay, s.beta1, s.omb1, s.beta2, s.omb2, step_size, s.bc2s, eps, l2,
                 po[e], mo[e], vo[e]);
    m[i] = make_float4(mo[0], mo[1], mo[2], mo[3]);
    v[i] = make_float4(vo[0], vo[1], vo[2], vo[3]);
    p[i] = make_float4(po[0], po[1], po[2], po[3]);
    if (shadow) shadow[i] = make_uint2(pack2(po[0], po[1]), pack2(po[2], po[3]));
  }
}

// AdamW with per-group lr / weight decay / eps (ops/optim.py FusedAdamW with several parameter
// groups) over the chunk table (optim_common.h) and tgroup (T,) int32 = tensor → group.  Group j's
// words sit behind the 8 global ones: hyper[8 + 4j .. ] = lr, weight decay, eps, reserved.  step /
// betas / clip factor / gscale / l2 / zero_g / loss ring are global.  A workgroup walks chunks
// grid-stride: 256 threads × float4, every load of a chunk in flight before the arithmetic, a scalar
// tail for length % 4.  Padding is neither read nor written; no atomics.  A chunk that does not fit
// the buffers or a group id outside [0, G) is skipped (checked builds flag kErrOptTable).
__global__ __launch_bounds__(256) void adamw_grouped_kernel(
    float* __restrict__ p, float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
    uint16_t* __restrict__ shadow, long long n, const float* __restrict__ hyper, const long long* __restrict__ chunks,
    long long C, const int* __restrict__ tgroup, int T, int G, float clip, float gscale, int l2, int zero_g,
    const float* __restrict__ loss_src, float* __restrict__ loss_ring, int ring_n, const float* __restrict__ norm_part,
    const float* __restrict__ guard) {
  const AdamStep s = adam_step(hyper, clip, gscale, loss_src, loss_ring, ring_n, norm_part, guard);
  if (s.skip && !zero_g) return;  // uniform over the launch
  for (long long c = blockIdx.x; c < C; c += gridDim.x) {  // uniform over the block
    const OptChunk k = opt_chunk(chunks, c, n, T);
    const int grp = k.ok ? tgroup[k.tid] : -1;
    if (grp < 0 || grp >= G) {
      if (threadIdx.x == 0) pio_flag(kErrOptTable);
      continue;
    }
    if (s.skip) {  // a skipped step: the chunk's gradient is cleared, nothing else of it is touched
      float4* gz = reinterpret_cast<float4*>(g + k.start);
      for (int i = threadIdx.x; i < (k.len >> 2); i += 256) gz[i] = make_float4(0.f, 0.f, 0.f, 0.f);
      const int t = (k.len & ~3) + threadIdx.x;
      if (t < k.len) g[k.start + t] = 0.f;
      continue;
    }
    const float* hg = hyper + kOptGroupBase + kOptGroupWords * grp;
    const float lr = hg[0], wd = hg[1], eps = hg[2];
    const float step_size = lr / s.bc1, decay = fmaf(-wd, lr, 1.f);
    const long long start = k.start;
    const int len4 = k.len >> 2;
    float4* p4 = reinterpret_cast<float4*>(p + start);
    float4* g4 = reinterpret_cast<float4*>(g + start);
    float4* m4 = reinterpret_cast<float4*>(m + start);
    float4* v4 = reinterpret_cast<float4*>(v + start);
    uint2* s2 = shadow ? reinterpret_cast<uint2*>(shadow + start) : nullptr;
    float4 P[kOptIter], Gr[kOptIter], M[kOptIter], V[kOptIter];
#pragma unroll
    for (int j = 0; j < kOptIter; ++j) {
      const int i = threadIdx.x + 256 * j;
      if (i < len4) {
        P[j] = p4[i];
        Gr[j] = g4[i];
        M[j] = m4[i];
        V[j] = v4[i];
      }
    }
#pragma unroll
    for (int j = 0; j < kOptIter; ++j) {
      const int i = threadIdx.x + 256 * j;
      if (i < len4) {
        if (zero_g) g4[i] = make_float4(0.f, 0.f, 0.f, 0.f);
        const float pa[4] = {P[j].x, P[j].y, P[j].z, P[j].w}, ga[4] = {Gr[j].x, Gr[j].y, Gr[j].z, Gr[j].w};
        const float ma[4] = {M[j].x, M[j].y, M[j].z, M[j].w}, va[4] = {V[j].x, V[j].y, V[j].z, V[j].w};
        float po[4], mo[4], vo[4];
#pragma unroll
        for (int e = 0; e < 4; ++e)
          adamw_elem(pa[e], ga[e], ma[e], va[e], s.gs, wd, decay, s.beta1, s.omb1, s.beta2, s.omb2, step_size, s.bc2s, eps,
                     l2, po[e], mo[e], vo[e]);
        m4[i] = make_float4(mo[0], mo[1], mo[2], mo[3]);
        v4[i] = make_float4(vo[0], vo[1], vo[2], vo[3]);
        p4[i] = make_float4(po[0], po[1], po[2], po[3]);
        if (s2) s2[i] = make_uint2(pack2(po[0], po[1]), pack2(po[2], po[3]));
      }
    }
    // a tensor's last chunk: up to 3 elements past the last whole float4
    const int t = (len4 << 2) + threadIdx.x;
    if (t < k.len) {
      const long long j = start + t;
      const float g0 = g[j];
      if (zero_g) g[j] = 0.f;
      float pi, mi, vi;
      adamw_elem(p[j], g0, m[j], v[j], s.gs, wd, decay, s.beta1, s.omb1, s.beta2, s.omb2, step_size, s.bc2s, eps, l2, pi,
                 mi, vi);
      m[j] = mi;
      v[j] = vi;
      p[j] = pi;
      if (shadow) shadow[j] = f2bf(pi);
    }
  }
}

// grad[i] += Σ_r rep[r][i], rep[r][i] ← 0 (replicated gradient accumulators, see ops/optim.py)
__global__ void fold_replicas_kernel(float* __restrict__ grad, float* __restrict__ rep, long long n, int nrep) {
  const long long n4 = n >> 2;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long long)gridDim.x * blockDim.x) {
    float4 acc = reinterpret_cast<float4*>(grad)[i];
    for (int r = 0; r < nrep; ++r) {
      float4* p = reinterpret_cast<float4*>(rep + r * n) + i;
      const float4 v = *p;
      acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
      *p = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    reinterpret_cast<float4*>(grad)[i] = acc;
  }
  for (long long i = (n4 << 2) + (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (long long)gridDim.x * blockDim.x) {
    float acc = grad[i];
    for (int r = 0; r < nrep; ++r) { acc += rep[r * n + i]; rep[r * n + i] = 0.f; }
    grad[i] = acc;
  }
}

static dim3 grid_for(long long n, int per = 256) {
  long long b = (n + per - 1) / per;
  if (b > 4096) b = 4096;
  if (b < 1) b = 1;
  return dim3((unsigned)b);
}

void sumsq_launch(const float* g, long long n, float* part, hipStream_t st) {
  hipLaunchKernelGGL(sumsq_kernel, dim3(kSumsqBlocks), dim3(256), 0, st, g, n, part);
}
void adamw_launch(float* p, float* g, float* m, float* v, uint16_t* shadow, long long n, const float* hyper,
                  float eps, float wd, float clip, float gscale, int l2, int zero_g, const float* loss_src,
                  float* loss_ring, int ring_n, const float* norm_part, const float* guard, hipStream_t st) {
  const bool vec = n % 4 == 0 && ((reinterpret_cast<uintptr_t>(p) | reinterpret_cast<uintptr_t>(g) |
                                    reinterpret_cast<uintptr_t>(m) | reinterpret_cast<uintptr_t>(v)) & 15) == 0 &&
                   (reinterpret_cast<uintptr_t>(shadow) & 7) == 0;
  if (vec)
    hipLaunchKernelGGL(adamw4_kernel, grid_for(n / 4), dim3(256), 0, st, reinterpret_cast<float4*>(p),
                       reinterpret_cast<float4*>(g), reinterpret_cast<float4*>(m), reinterpret_cast<float4*>(v),
                       reinterpret_cast<uint2*>(shadow), n / 4, hyper, eps, wd, clip, gscale, l2, zero_g, loss_src,
                       loss_ring, ring_n, norm_part, guard);
  else
    hipLaunchKernelGGL(adamw_kernel, grid_for(n), dim3(256), 0, st, p, g, m, v, shadow, n, hyper, eps, wd, clip, gscale,
                       l2, zero_g, loss_src, loss_ring, ring_n, norm_part, guard);
}
// p, g, m, v 16-byte aligned, shadow 8-byte aligned, hyper of 8 + 4 G floats (checked by the
// binding); C chunks, T tensors, 1 ≤ G ≤ 8.  At most 2048 workgroups (8 per CU) walk the chunks.
int adamw_grouped_launch(float* p, float* g, float* m, float* v, uint16_t* shadow, long long n, const float* hyper,
                         const long long* chunks, long long C, const int* tgroup, int T, int G, float clip, float gscale,
                         int l2, int zero_g, const float* loss_src, float* loss_ring, int ring_n,
                         const float* norm_part, const float* guard, hipStream_t st) {
  if (G < 1 || G > kOptMaxGroups) return -1;
  if (C <= 0 || T <= 0) return 0;
  const unsigned blocks = (unsigned)(C < 2048 ? C : 2048);
  hipLaunchKernelGGL(adamw_grouped_kernel, dim3(blocks), dim3(256), 0, st, p, g, m, v, shadow, n, hyper, chunks, C, tgroup,
                     T, G, clip, gscale, l2, zero_g, loss_src, loss_ring, ring_n, norm_part, guard);
  return 0;
}
void fold_replicas_launch(float* grad, float* rep, long long n, int nrep, hipStream_t st) {
  hipLaunchKernelGGL(fold_replicas_kernel, grid_for((n + 3) / 4), dim3(256), 0, st, grad, rep, n, nrep);
}

unsigned check_errors_optim(bool reset) { return pio_read_errors(reset); }

}  // namespace pio
