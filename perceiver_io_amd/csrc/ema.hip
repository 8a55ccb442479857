// Weight EMA over the flat parameter space (ops/optim.py WeightEMA): the averaged weights are one
// more flat fp32 buffer next to FlatParameterSpace.data.
//   ema_update_kernel  e ← e + omd·(w − e) with omd = 1 − decay read from hyper[5] in device
//                      memory (the optimizer's hyper block, staged before every replay), so a
//                      captured step follows the schedule; omd == 0 (a step that does not update,
//                      decay = 1) returns before any load; omd == 1 (decay = 0) stores w itself.
//                      12 B per element.
//   ema_swap_kernel    w ↔ e in place and shadow ← bf16(new w): evaluation with the averaged
//                      weights and the way back.  The shadow conversion is adamw4_kernel's
//                      (pack2), so a second swap restores all three buffers bit for bit.
// Streaming only: no atomics, no LDS, 16-byte loads and stores, grid-stride loops.  This
// translation unit is compiled with -ffp-contract=off (csrc/build.py PER_FILE_FLAGS): the update
// is a subtraction, a product and a sum, each rounded on its own, which fp32 elementwise ops on
// the host reproduce bit for bit (ops/emulation.py ema_update).
#include "common.h"

namespace pio {

constexpr int kEmaBlocks = 2048;  // grid cap: 8 workgroups of 4 waves per CU (256 CUs)

static dim3 ema_grid(long long n4) {
  long long b = (n4 + 255) / 256;
  if (b > kEmaBlocks) b = kEmaBlocks;
  if (b < 1) b = 1;
  return dim3((unsigned)b);
}

__global__ __launch_bounds__(256) void ema_update_kernel(float4* __restrict__ e, const float4* __restrict__ w,
                                                         long long n4, const float* __restrict__ hyper) {
  const float omd = hyper[5];
  if (omd == 0.f) return;  // uniform over the grid
  // decay = 0: the average IS the weights.  e + (w − e) would miss w by a rounding of the
  // difference wherever w and e are more than a factor of two apart, so that case copies.
  const bool copy = omd == 1.f;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long long)gridDim.x * blockDim.x) {
    const float4 e4 = e[i], w4 = w[i];
    const float ea[4] = {e4.x, e4.y, e4.z, e4.w}, wa[4] = {w4.x, w4.y, w4.z, w4.w};
    float eo[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float d = wa[k] - ea[k];
      const float p = omd * d;
      eo[k] = copy ? wa[k] : ea[k] + p;
    }
    e[i] = make_float4(eo[0], eo[1], eo[2], eo[3]);
  }
}

__global__ __launch_bounds__(256) void ema_swap_kernel(float4* __restrict__ w, float4* __restrict__ e,
                                                       uint2* __restrict__ shadow, long long n4) {
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long long)gridDim.x * blockDim.x) {
    const float4 w4 = w[i], e4 = e[i];
    w[i] = e4;
    e[i] = w4;
    if (shadow) shadow[i] = make_uint2(pack2(e4.x, e4.y), pack2(e4.z, e4.w));
  }
}

long long ema_pass_elems() { return 4LL * 256 * kEmaBlocks; }

// ema, w 16-byte aligned and n % 4 == 0 (checked by the binding)
void ema_update_launch(float* ema, const float* w, long long n, const float* hyper, hipStream_t st) {
  if (n <= 0) return;
  hipLaunchKernelGGL(ema_update_kernel, ema_grid(n / 4), dim3(256), 0, st, reinterpret_cast<float4*>(ema),
                     reinterpret_cast<const float4*>(w), n / 4, hyper);
}

// w, ema 16-byte aligned, shadow (may be null) 8-byte aligned, n % 4 == 0 (checked by the binding)
void ema_swap_launch(float* w, float* ema, uint16_t* shadow, long long n, hipStream_t st) {
  if (n <= 0) return;
  hipLaunchKernelGGL(ema_swap_kernel, ema_grid(n / 4), dim3(256), 0, st, reinterpret_cast<float4*>(w),
                     reinterpret_cast<float4*>(ema), reinterpret_cast<uint2*>(shadow), n / 4);
}

}  // namespace pio
