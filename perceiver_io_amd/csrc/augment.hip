// Device-side image augmentation: crop box → bilinear resize → horizontal flip → normalize, one
// pass from the raw uint8 batch to the fp32 channels-last model input.
//
// src (B, Hs, Ws, C) uint8; params (B, 8) fp32 words in device memory, per sample
// {y0, x0, h, w, flip, 0, 0, 0}: the crop box in source pixels (integers stored as floats) and
// the flip flag (flip if ≥ 0.5).  The kernel reads the words itself, so a replayed hipGraph
// augments with whatever was staged for that step (the contract of batch_mix_kernel).
//
// Semantics = F.interpolate(box, (oh, ow), "bilinear", align_corners=False, antialias=False),
// then the flip, then (v / 255 − mean_c) / std_c on the interpolated 0..255 value:
//   output (i, j), j → ow − 1 − j when flipped;  sy = max((i + 0.5)·(h / oh) − 0.5, 0),
//   i0 = ⌊sy⌋, i1 = min(i0 + 1, h − 1), λ = sy − i0 (columns alike), all inside the box.
// A box of exactly the output size takes the copy path: no interpolation arithmetic, the result
// is bit for bit the host pipeline's (u8.float() / 255 − mean) / std.  This file is compiled
// with -ffp-contract=off (build.py): every product, sum and quotient below is rounded on its
// own, as ATen rounds them, so the kernel and its PyTorch emulation agree bitwise.
//
// Every build clamps the box into the source before an address is formed (NaN or negative
// offsets count as 0, NaN / zero / negative sizes as 1): no word can cause a read outside src.
// The checked build also raises kErrAugmentBox when it had to clamp.
//
// Bandwidth-bound gather: VEC consecutive output floats of one row per thread (VEC = 4: one
// 16-byte store, needs ow·C % 4 == 0), row coefficients computed once per thread, column
// coefficients once per pixel.  Grid (x-blocks, B), no atomics: bitwise repeatable.
#include "common.h"

#include <algorithm>

namespace pio {

struct AugNorm {
  float mean[4];
  float std[4];
};

// element c of a 4-word kernel-argument array by selects (a lane-varying index into the
// argument struct would move it to scratch)
__device__ __forceinline__ float aug_sel(const float (&a)[4], int c) {
  return c == 0 ? a[0] : (c == 1 ? a[1] : (c == 2 ? a[2] : a[3]));
}

// a box word as an integer in [lo, hi]; NaN and anything below lo → lo, anything above hi → hi
__device__ __forceinline__ int aug_word(float v, int lo, int hi) {
  return v >= (float)lo ? (v <= (float)hi ? (int)v : hi) : lo;
}

template <int VEC>
__global__ __launch_bounds__(256) void batch_augment_kernel(const uint8_t* __restrict__ src,
                                                            const float* __restrict__ params,
                                                            float* __restrict__ out, int Hs, int Ws, int C, int oh,
                                                            int ow, AugNorm nm) {
  const int b = blockIdx.y;
  const float* p = params + (long long)b * 8;
  const float p0 = p[0], p1 = p[1], p2 = p[2], p3 = p[3];
  const int y0 = aug_word(p0, 0, Hs - 1), x0 = aug_word(p1, 0, Ws - 1);
  const int h = aug_word(p2, 1, Hs - y0), w = aug_word(p3, 1, Ws - x0);
  const bool flip = p[4] >= 0.5f;
#if PIO_CHECKS
  if (blockIdx.x == 0 && threadIdx.x == 0 &&
      !((float)y0 == p0 && (float)x0 == p1 && (float)h == p2 && (float)w == p3))
    pio_flag(kErrAugmentBox);
#endif
  const bool copy = h == oh && w == ow;
  const float sch = (float)h / (float)oh, scw = (float)w / (float)ow;
  const int rowlen = ow * C, n = oh * rowlen;
  const uint8_t* sb = src + ((long long)b * Hs + y0) * ((long long)Ws * C) + (long long)x0 * C;
  float* ob = out + (long long)b * n;
  const int srow = Ws * C;
  for (int e = (blockIdx.x * blockDim.x + threadIdx.x) * VEC; e < n; e += gridDim.x * blockDim.x * VEC) {
    // the VEC elements share output row i (rowlen % VEC == 0); they walk pixels j, channels c
    const int i = e / rowlen, q = e - i * rowlen;
    int j = q / C, c = q - j * C;
    int i0 = i, i1 = i;
    float ly = 0.f;
    if (!copy) {
      const float sy = fmaxf(((float)i + 0.5f) * sch - 0.5f, 0.f);
      i0 = min((int)sy, h - 1);
      i1 = min(i0 + 1, h - 1);
      ly = sy - (float)i0;
    }
    const uint8_t* r0 = sb + (long long)i0 * srow;
    const uint8_t* r1 = sb + (long long)i1 * srow;
    float res[VEC];
    int jc = -1, c0 = 0, c1 = 0;  // pixel the column coefficients below belong to
    float lx = 0.f;
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
      if (j != jc) {
        jc = j;
        const int jj = flip ? ow - 1 - j : j;
        if (copy) {
          c0 = jj * C;
        } else {
          const float sx = fmaxf(((float)jj + 0.5f) * scw - 0.5f, 0.f);
          const int j0 = min((int)sx, w - 1);
          lx = sx - (float)j0;
          c0 = j0 * C;
          c1 = min(j0 + 1, w - 1) * C;
        }
      }
      float v;
      if (copy) {
        v = (float)r0[c0 + c];
      } else {
        const float v00 = (float)r0[c0 + c], v01 = (float)r0[c1 + c];
        const float v10 = (float)r1[c0 + c], v11 = (float)r1[c1 + c];
        const float mx = 1.f - lx, my = 1.f - ly;
        v = my * (mx * v00 + lx * v01) + ly * (mx * v10 + lx * v11);
      }
      res[k] = (v / 255.f - aug_sel(nm.mean, c)) / aug_sel(nm.std, c);
      if (++c == C) {
        c = 0;
        ++j;
      }
    }
    if constexpr (VEC == 4) {
      *reinterpret_cast<float4*>(ob + e) = make_float4(res[0], res[1], res[2], res[3]);
    } else {
      ob[e] = res[0];
    }
  }
}

void batch_augment_launch(const uint8_t* src, const float* params, float* out, int B, int Hs, int Ws, int C, int oh,
                          int ow, const float* mean, const float* std, hipStream_t st) {
  AugNorm nm;
  for (int c = 0; c < 4; ++c) {
    nm.mean[c] = c < C ? mean[c] : 0.f;
    nm.std[c] = c < C ? std[c] : 1.f;
  }
  const int rowlen = ow * C, n = oh * rowlen;
  if (rowlen % 4 == 0) {
    const int bx = std::min(256, (n / 4 + 255) / 256);
    hipLaunchKernelGGL(batch_augment_kernel<4>, dim3(bx, B), dim3(256), 0, st, src, params, out, Hs, Ws, C, oh, ow, nm);
  } else {
    const int bx = std::min(256, (n + 255) / 256);
    hipLaunchKernelGGL(batch_augment_kernel<1>, dim3(bx, B), dim3(256), 0, st, src, params, out, Hs, Ws, C, oh, ow, nm);
  }
}

unsigned check_errors_augment(bool reset) { return pio_read_errors(reset); }

}  // namespace pio
