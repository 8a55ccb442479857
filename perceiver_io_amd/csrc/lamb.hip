// Fused LAMB over the flat parameter space (ops/optim.py FusedLamb): layer-wise trust ratios
// ‖w‖/‖u‖ and per-tensor weight decay on top of the flat fp32 buffers.
//
// The kernels walk the chunk table of the flat buffers (optim_common.h) and two per-tensor tables:
//   chunks (C, 3) int64: start element, length, tensor id
//   tensors (T, 2) int32: first chunk, chunk count;  topt (T, 2) fp32: weight decay, adapt (0 / 1)
// One step is three launches:
//   lamb_moments_kernel  one block per chunk: reads g, m, v, w; writes m, v (clears g); forms
//                        u = m̂ / (sqrt(v̂) + eps) + wd·w in registers and writes the chunk's
//                        (Σw², Σu²) to partials[2c], partials[2c + 1]
//   lamb_trust_kernel    one block per tensor: sums its chunks' partials in a fixed order (fp64)
//                        → trust[t] = ‖w‖ / ‖u‖ (1 for non-adapted tensors and zero norms)
//   lamb_apply_kernel    one block per chunk: recomputes u from the new m, v and the old w (12 B
//                        per element instead of 4 B written + 8 B read for a stored u) and writes
//                        w ← w − lr·trust·u with its bf16 shadow
// No atomics and fixed summation orders everywhere: results are bitwise repeatable.  Both chunk
// kernels form u with lamb_u() (optim_common.h) from the same operands; this translation unit is
// compiled with -ffp-contract=off (csrc/build.py PER_FILE_FLAGS), so the compiler cannot contract
// its multiply-adds differently in the two kernels — the only fused operations are the explicit
// fmaf calls — and the u whose norm set the trust ratio is bit for bit the u that is applied.
// lr / step / betas come from `hyper` in device memory (optim_common.h opt_step), so a
// replayed graph follows the scheduler.
#include "optim_common.h"

namespace pio {

// 1 − β^t without the cancellation of 1.f − powf(β, t) (β2 = 0.999, t = 3: one ulp of β^t is 1e-5
// of the result, and the trust ratio inherits it)
__device__ __forceinline__ float lamb_bias_correction(float beta, float step) {
  return -expm1f(step * logf(beta));
}

// fixed-order block sum of two values (256 threads): lane butterflies, then the 4 wave results
__device__ __forceinline__ void block_sum2(float& a, float& b) {
  __shared__ float red[2][4];
  a = wave_sum(a);
  b = wave_sum(b);
  if (lane_id() == 0) {
    red[0][wave_id()] = a;
    red[1][wave_id()] = b;
  }
  __syncthreads();
  a = (red[0][0] + red[0][1]) + (red[0][2] + red[0][3]);
  b = (red[1][0] + red[1][1]) + (red[1][2] + red[1][3]);
}

// pass 1.  hyper / loss_src / loss_ring / zero_g / clip / guard as in adamw_kernel (optim.hip)
__global__ __launch_bounds__(256) void lamb_moments_kernel(
    const float* __restrict__ p, float* __restrict__ g, float* __restrict__ m, float* __restrict__ v, long long n,
    const float* __restrict__ hyper, const long long* __restrict__ chunks, const float* __restrict__ topt, int T,
    float* __restrict__ partials, float eps, float clip, float gscale, int zero_g, const float* __restrict__ loss_src,
    float* __restrict__ loss_ring, int ring_n, const float* __restrict__ norm_part, const float* __restrict__ guard) {
  const OptStep s = opt_step(hyper, clip, gscale, loss_src, loss_ring, ring_n, norm_part, guard);
  const OptChunk c = opt_chunk(chunks, blockIdx.x, n, T);
  if (s.skip) {  // uniform over the launch: the gradient is cleared, m, v and the partials stay
    if (zero_g && c.ok) {
      float4* gz = reinterpret_cast<float4*>(g + c.start);
      for (int i = threadIdx.x; i < (c.len >> 2); i += 256) gz[i] = make_float4(0.f, 0.f, 0.f, 0.f);
      const int t = (c.len & ~3) + threadIdx.x;
      if (t < c.len) g[c.start + t] = 0.f;
    }
    return;
  }
  const float bc1 = lamb_bias_correction(s.beta1, s.step), bc2s = sqrtf(lamb_bias_correction(s.beta2, s.step));
  float sw = 0.f, su = 0.f;
  if (c.ok) {
    const float wd = topt[2 * c.tid];
    const int len4 = c.len >> 2;
    const float4* p4 = reinterpret_cast<const float4*>(p + c.start);
    float4* g4 = reinterpret_cast<float4*>(g + c.start);
    float4* m4 = reinterpret_cast<float4*>(m + c.start);
    float4* v4 = reinterpret_cast<float4*>(v + c.start);
    float4 P[kOptIter], G[kOptIter], M[kOptIter], V[kOptIter];
#pragma unroll
    for (int k = 0; k < kOptIter; ++k) {  // every load of the chunk in flight before the arithmetic
      const int i = threadIdx.x + 256 * k;
      if (i < len4) {
        P[k] = p4[i];
        G[k] = g4[i];
        M[k] = m4[i];
        V[k] = v4[i];
      }
    }
#pragma unroll
    for (int k = 0; k < kOptIter; ++k) {
      const int i = threadIdx.x + 256 * k;
      if (i < len4) {
        if (zero_g) g4[i] = make_float4(0.f, 0.f, 0.f, 0.f);
        const float pa[4] = {P[k].x, P[k].y, P[k].z, P[k].w}, ga[4] = {G[k].x, G[k].y, G[k].z, G[k].w};
        const float ma[4] = {M[k].x, M[k].y, M[k].z, M[k].w}, va[4] = {V[k].x, V[k].y, V[k].z, V[k].w};
        float mo[4], vo[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          lamb_moments(ga[e], ma[e], va[e], s.gs, s.beta1, s.beta2, mo[e], vo[e]);
          const float u = lamb_u(pa[e], mo[e], vo[e], bc1, bc2s, eps, wd);
          sw = fmaf(pa[e], pa[e], sw);
          su = fmaf(u, u, su);
        }
        m4[i] = make_float4(mo[0], mo[1], mo[2], mo[3]);
        v4[i] = make_float4(vo[0], vo[1], vo[2], vo[3]);
      }
    }
    // a tensor's last chunk: up to 3 elements past the last whole float4
    const int t = (len4 << 2) + threadIdx.x;
    if (t < c.len) {
      const long long j = c.start + t;
      const float w = p[j], g0 = g[j];
      if (zero_g) g[j] = 0.f;
      float mi, vi;
      lamb_moments(g0, m[j], v[j], s.gs, s.beta1, s.beta2, mi, vi);
      m[j] = mi;
      v[j] = vi;
      const float u = lamb_u(w, mi, vi, bc1, bc2s, eps, wd);
      sw = fmaf(w, w, sw);
      su = fmaf(u, u, su);
    }
  }
  block_sum2(sw, su);
  if (threadIdx.x == 0) {
    partials[2 * (long long)blockIdx.x] = sw;
    partials[2 * (long long)blockIdx.x + 1] = su;
  }
}

// trust[t] = ‖w_t‖ / ‖u_t‖ from the tensor's chunk partials: thread-strided fp64 sums, then a
// fixed LDS tree.  A launch of its own: folded into pass 2, every block of a tensor would re-sum
// the tensor's partials (4100 blocks × 4100 pairs for the 16.8 M-element LArTPC query table).
__global__ __launch_bounds__(256) void lamb_trust_kernel(const float* __restrict__ partials,
                                                         const int* __restrict__ tensors,
                                                         const float* __restrict__ topt, long long C,
                                                         float* __restrict__ trust,
                                                         const float* __restrict__ guard) {
  __shared__ double red[2][256];
  if (opt_guard_skip(guard)) return;  // a skipped step keeps the last update's trust ratios
  const int t = blockIdx.x;
  const long long first = tensors[2 * t], cnt = tensors[2 * t + 1];
  const bool adapt = topt[2 * t + 1] != 0.f && first >= 0 && cnt >= 0 && first + cnt <= C;
  if (!adapt) {  // uniform over the block
    if (threadIdx.x == 0) trust[t] = 1.f;
    return;
  }
  double sw = 0.0, su = 0.0;
  for (long long i = threadIdx.x; i < cnt; i += 256) {
    sw += (double)partials[2 * (first + i)];
    su += (double)partials[2 * (first + i) + 1];
  }
  red[0][threadIdx.x] = sw;
  red[1][threadIdx.x] = su;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) {
      red[0][threadIdx.x] += red[0][threadIdx.x + s];
      red[1][threadIdx.x] += red[1][threadIdx.x + s];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const float nw = sqrtf((float)red[0][0]), nu = sqrtf((float)red[1][0]);
    trust[t] = (nw > 0.f && nu > 0.f) ? nw / nu : 1.f;
  }
}

// pass 2
__global__ __launch_bounds__(256) void lamb_apply_kernel(float* __restrict__ p, const float* __restrict__ m,
                                                         const float* __restrict__ v, uint16_t* __restrict__ shadow,
                                                         long long n, const float* __restrict__ hyper,
                                                         const long long* __restrict__ chunks,
                                                         const float* __restrict__ topt, int T,
                                                         const float* __restrict__ trust, float eps,
                                                         const int* __restrict__ tgroup, int G,
                                                         const float* __restrict__ guard) {
  if (opt_guard_skip(guard)) return;  // the same word the other two launches of this step read
  const float step = opt_guard_step(hyper, guard), beta1 = hyper[3], beta2 = hyper[4];
  const float bc1 = lamb_bias_correction(beta1, step), bc2s = sqrtf(lamb_bias_correction(beta2, step));
  const OptChunk c = opt_chunk(chunks, blockIdx.x, n, T);
  if (!c.ok) return;
  // the tensor's lr: its group's word behind the 8 global ones (hyper[8 + 4 j], the layout of
  // optim.hip adamw_grouped_kernel); without a group table every tensor takes group 0's, hyper[0]
  float lr = hyper[0];
  if (tgroup != nullptr) {
    const int grp = tgroup[c.tid];
    if (grp < 0 || grp >= G) {  // uniform over the block
      if (threadIdx.x == 0) pio_flag(kErrOptTable);
      return;
    }
    lr = hyper[kOptGroupBase + kOptGroupWords * grp];
  }
  const float wd = topt[2 * c.tid];
  const float a = -(lr * trust[c.tid]);
  const int len4 = c.len >> 2;
  float4* p4 = reinterpret_cast<float4*>(p + c.start);
  const float4* m4 = reinterpret_cast<const float4*>(m + c.start);
  const float4* v4 = reinterpret_cast<const float4*>(v + c.start);
  uint2* s2 = shadow ? reinterpret_cast<uint2*>(shadow + c.start) : nullptr;
  float4 P[kOptIter], M[kOptIter], V[kOptIter];
#pragma unroll
  for (int k = 0; k < kOptIter; ++k) {
    const int i = threadIdx.x + 256 * k;
    if (i < len4) {
      P[k] = p4[i];
      M[k] = m4[i];
      V[k] = v4[i];
    }
  }
#pragma unroll
  for (int k = 0; k < kOptIter; ++k) {
    const int i = threadIdx.x + 256 * k;
    if (i < len4) {
      const float pa[4] = {P[k].x, P[k].y, P[k].z, P[k].w}, ma[4] = {M[k].x, M[k].y, M[k].z, M[k].w};
      const float va[4] = {V[k].x, V[k].y, V[k].z, V[k].w};
      float po[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) po[e] = fmaf(a, lamb_u(pa[e], ma[e], va[e], bc1, bc2s, eps, wd), pa[e]);
      p4[i] = make_float4(po[0], po[1], po[2], po[3]);
      if (s2) s2[i] = make_uint2(pack2(po[0], po[1]), pack2(po[2], po[3]));
    }
  }
  const int t = (len4 << 2) + threadIdx.x;
  if (t < c.len) {
    const long long j = c.start + t;
    const float w = p[j];
    const float pn = fmaf(a, lamb_u(w, m[j], v[j], bc1, bc2s, eps, wd), w);
    p[j] = pn;
    if (shadow) shadow[j] = f2bf(pn);
  }
}

int lamb_chunk_elems() { return kOptChunk; }

// p, g, m, v 16-byte aligned, shadow 8-byte aligned (checked by the binding); C chunks, T tensors;
// tgroup (T,) tensor → group with hyper of 8 + 4 G floats, or null: every tensor in group 0
void lamb_launch(float* p, float* g, float* m, float* v, uint16_t* shadow, long long n, const float* hyper,
                 const long long* chunks, long long C, const int* tensors, const float* topt, int T, float* partials,
                 float* trust, float eps, float clip, float gscale, int zero_g, const float* loss_src,
                 float* loss_ring, int ring_n, const float* norm_part, const int* tgroup, int G, const float* guard,
                 hipStream_t st) {
  if (C <= 0 || T <= 0) return;
  hipLaunchKernelGGL(lamb_moments_kernel, dim3((unsigned)C), dim3(256), 0, st, p, g, m, v, n, hyper, chunks, topt, T,
                     partials, eps, clip, gscale, zero_g, loss_src, loss_ring, ring_n, norm_part, guard);
  hipLaunchKernelGGL(lamb_trust_kernel, dim3((unsigned)T), dim3(256), 0, st, partials, tensors, topt, C, trust, guard);
  hipLaunchKernelGGL(lamb_apply_kernel, dim3((unsigned)C), dim3(256), 0, st, p, m, v, shadow, n, hyper, chunks, topt, T,
                     trust, eps, tgroup, G, guard);
}

}  // namespace pio
