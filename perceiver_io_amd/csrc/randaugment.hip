// Device-side RandAugment on raw uint8 batches: N layers per sample, each one of ten operations
// chosen by a word block the host drew (data/augment.py RandAugment) and staged into device
// memory.  The kernels read the words themselves, so a replayed hipGraph augments with whatever
// was staged for that step (the contract of batch_augment_kernel / batch_mix_kernel).
//
// src (B, H, W, C) uint8, C ∈ {1, 3}; words (B, N, 8) fp32, layer l of sample b is
// {op, v, m00, m01, m02, m10, m11, m12}.  Layers run in order, each on the uint8 result of the
// previous one.  All values below are uint8 values x, per channel unless said:
//   0 identity      copy
//   1 affine        output (i, j) reads source pixel (⌊sy⌋, ⌊sx⌋), sx = m00·(j+0.5) + m01·(i+0.5) + m02,
//                   sy = m10·(j+0.5) + m11·(i+0.5) + m12, summed left to right in fp32; outside the
//                   image (NaN and ±inf included): fill.  PIL's Image.transform(AFFINE, NEAREST).
//   2 brightness    blend(x, 0, v)
//   3 color         blend(x, g, v), g = (19595·r + 38470·g + 7471·b + 32768) >> 16 of the pixel;
//                   C = 1: copy
//   4 contrast      blend(x, m, v), m = (2·Σg + n) / (2n) over the n = H·W pixels (integer division)
//   5 sharpness     blend(x, s, v), s = (Σ₃ₓ₃ w·x + 6) / 13, w = {1,1,1; 1,5,1; 1,1,1}; s = x on
//                   the one-pixel border
//   6 posterize     x & ~(2^(8−v) − 1), v bits kept (clamped into 0..8)
//   7 solarize      x ≥ v ? 255 − x : x
//   8 autocontrast  lo, hi = min, max of the channel; hi ≤ lo: copy; else ((x − lo)·255) / (hi − lo)
//   9 equalize      PIL ImageOps.equalize: channel histogram h; at most one non-zero bin: copy;
//                   step = (n − h[last non-zero bin]) / 255; step = 0: copy; else
//                   lut[k] = min(255, (step/2 + Σ_{t<k} h[t]) / step)
// blend(x, d, f) = trunc(clamp(d + f·(x − d), 0, 255)) in fp32, NaN → 0; the difference, the
// product and the sum are rounded one by one (this file is compiled with -ffp-contract=off,
// build.py), as ATen rounds them: the kernels and ops/emulation.py rand_augment agree bitwise.
// An op word that is NaN, negative, above 9 or not an integer is identity in every build; the
// checked build also raises kErrRandAugOp.  No word can cause an access outside the image:
// affine coordinates are range-checked as floats after the floor, before an index is formed.
//
// Two launches per layer over ping-pong images (ops 1 and 5 read neighbours: input ≠ output):
//   ra_stats_kernel  grid (blocks, B): returns at once unless op ∈ {4, 8, 9}; otherwise LDS
//                    histograms (integer atomics) of its pixels — the grey one for op 4, one per
//                    channel for 8 and 9 — added into the layer's int32 (B, C+1, 256) block.
//                    Integer sums: bitwise repeatable whatever the grid.
//   ra_apply_kernel  grid (blocks, B): every workgroup turns the histograms into a 256-entry
//                    table per channel in LDS (ops 2, 4, 6, 7, 8, 9 are all point operations),
//                    then streams whole pixels: 4 pixels = C dwords per thread when H·W % 4 == 0
//                    and the images are 4-byte aligned, else one pixel per thread.  op is
//                    uniform per workgroup: one branch outside the pixel loop.
// Histogram reset: each layer has its own block, and the caller clears all of them with one fill
// launch on the stream before the first layer (the binding's torch::zeros: a kernel node of the
// captured graph, so every replay starts from zeros; a hipMemsetAsync issued during stream
// capture is not replayed on this stack, see persist.hip).  No floating-point atomics anywhere.
#include "common.h"

#include <algorithm>

namespace pio {

// the op code of a word; anything that is not an integer in [0, 9] → −1 (identity)
__device__ __forceinline__ int ra_op(float w) { return (w >= 0.f && w <= 9.f && w == floorf(w)) ? (int)w : -1; }

__device__ __forceinline__ int ra_blend(int x, int d, float f) {
  const float t = (float)d + f * ((float)x - (float)d);
  return (int)(t >= 0.f ? (t <= 255.f ? t : 255.f) : 0.f);  // NaN → 0
}

__device__ __forceinline__ int ra_grey(int r, int g, int b) { return (19595 * r + 38470 * g + 7471 * b + 32768) >> 16; }

// PP·C consecutive bytes (PP pixels) at byte offset e: PP = 4 as C aligned dwords, PP = 1 as bytes
template <int C, int PP>
__device__ __forceinline__ void ra_load(const uint8_t* p, long long e, int (&x)[PP * C]) {
  if constexpr (PP == 4) {
    const uint32_t* q = reinterpret_cast<const uint32_t*>(p + e);
#pragma unroll
    for (int d = 0; d < C; ++d) {
      const uint32_t w = q[d];
#pragma unroll
      for (int k = 0; k < 4; ++k) x[4 * d + k] = (int)((w >> (8 * k)) & 255u);
    }
  } else {
#pragma unroll
    for (int k = 0; k < C; ++k) x[k] = p[e + k];
  }
}
template <int C, int PP>
__device__ __forceinline__ void ra_store(uint8_t* p, long long e, const int (&x)[PP * C]) {
  if constexpr (PP == 4) {
    uint32_t* q = reinterpret_cast<uint32_t*>(p + e);
#pragma unroll
    for (int d = 0; d < C; ++d)
      q[d] = (uint32_t)x[4 * d] | ((uint32_t)x[4 * d + 1] << 8) | ((uint32_t)x[4 * d + 2] << 16) |
             ((uint32_t)x[4 * d + 3] << 24);
  } else {
#pragma unroll
    for (int k = 0; k < C; ++k) p[e + k] = (uint8_t)x[k];
  }
}

// hist: this layer's (B, C+1, 256) block — channels 0..C−1, then grey
template <int C, int PP>
__global__ __launch_bounds__(256) void ra_stats_kernel(const uint8_t* __restrict__ in, const float* __restrict__ words,
                                                       int N, int layer, int* __restrict__ hist, int npix) {
  const int b = blockIdx.y;
  const int op = ra_op(words[((long long)b * N + layer) * 8]);
  if (op != 4 && op != 8 && op != 9) return;
  __shared__ int h[(C + 1) * 256];
  for (int k = threadIdx.x; k < (C + 1) * 256; k += blockDim.x) h[k] = 0;
  __syncthreads();
  const uint8_t* ib = in + (long long)b * npix * C;
  const int nunits = npix / PP;
  for (int u = blockIdx.x * blockDim.x + threadIdx.x; u < nunits; u += gridDim.x * blockDim.x) {
    int x[PP * C];
    ra_load<C, PP>(ib, (long long)u * (PP * C), x);
#pragma unroll
    for (int q = 0; q < PP; ++q) {
      if (op == 4) {
        int g = x[q * C];
        if constexpr (C == 3) g = ra_grey(x[q * C], x[q * C + 1], x[q * C + 2]);
        atomicAdd(&h[C * 256 + g], 1);
      } else {
#pragma unroll
        for (int c = 0; c < C; ++c) atomicAdd(&h[c * 256 + x[q * C + c]], 1);
      }
    }
  }
  __syncthreads();
  int* hb = hist + (long long)b * ((C + 1) * 256);
  for (int k = threadIdx.x; k < (C + 1) * 256; k += blockDim.x)
    if (h[k] != 0) atomicAdd(hb + k, h[k]);
}

// the pixel loop: f(p, x, o) forms the C output bytes o of pixel p from its own input bytes x
template <int C, int PP, typename F>
__device__ __forceinline__ void ra_stream(const uint8_t* ib, uint8_t* ob, int npix, F f) {
  const int nunits = npix / PP;
  for (int u = blockIdx.x * blockDim.x + threadIdx.x; u < nunits; u += gridDim.x * blockDim.x) {
    int x[PP * C], o[PP * C];
    ra_load<C, PP>(ib, (long long)u * (PP * C), x);
#pragma unroll
    for (int q = 0; q < PP; ++q) f(u * PP + q, &x[q * C], &o[q * C]);
    ra_store<C, PP>(ob, (long long)u * (PP * C), o);
  }
}

template <int C, int PP>
__global__ __launch_bounds__(256) void ra_apply_kernel(const uint8_t* __restrict__ in, uint8_t* __restrict__ out,
                                                       const float* __restrict__ words, int N, int layer,
                                                       const int* __restrict__ hist, int H, int W, int fill) {
  const int b = blockIdx.y, t = threadIdx.x;  // 256 threads: thread t owns table entry t
  const float* wd = words + ((long long)b * N + layer) * 8;
  const int op = ra_op(wd[0]);
  const float v = wd[1];
#if PIO_CHECKS
  if (op < 0 && blockIdx.x == 0 && t == 0) pio_flag(kErrRandAugOp);
#endif
  const int npix = H * W;
  const uint8_t* ib = in + (long long)b * npix * C;
  uint8_t* ob = out + (long long)b * npix * C;
  const int* hb = hist + (long long)b * ((C + 1) * 256);

  __shared__ uint8_t lut[C * 256];
  __shared__ int raw[C * 256], cum[C * 256];
  __shared__ int lo[C], hi[C], nnz[C];
  __shared__ unsigned long long sumg;

  if (op == 2 || op == 4 || op == 6 || op == 7 || op == 8 || op == 9) {
    // ---- the table of a point operation ----
    if (op == 2) {
      const int r = ra_blend(t, 0, v);
#pragma unroll
      for (int c = 0; c < C; ++c) lut[c * 256 + t] = (uint8_t)r;
    } else if (op == 6) {
      const int bits = v >= 0.f ? (v <= 8.f ? (int)v : 8) : 0;
      const int r = t & ~((1 << (8 - bits)) - 1) & 255;
#pragma unroll
      for (int c = 0; c < C; ++c) lut[c * 256 + t] = (uint8_t)r;
    } else if (op == 7) {
      const int r = (float)t >= v ? 255 - t : t;
#pragma unroll
      for (int c = 0; c < C; ++c) lut[c * 256 + t] = (uint8_t)r;
    } else if (op == 4) {
      if (t == 0) sumg = 0ull;
      __syncthreads();
      const unsigned long long mine = (unsigned long long)hb[C * 256 + t] * (unsigned long long)t;
      if (mine) atomicAdd(&sumg, mine);
      __syncthreads();
      const long long n = npix;
      const int m = (int)((2ll * (long long)sumg + n) / (2ll * n));
      const int r = ra_blend(t, m, v);
#pragma unroll
      for (int c = 0; c < C; ++c) lut[c * 256 + t] = (uint8_t)r;
    } else {  // 8, 9: per-channel histograms
      if (t < C) {
        lo[t] = 256;
        hi[t] = -1;
        nnz[t] = 0;
      }
#pragma unroll
      for (int c = 0; c < C; ++c) {
        const int hv = hb[c * 256 + t];
        raw[c * 256 + t] = hv;
        cum[c * 256 + t] = hv;
      }
      __syncthreads();
#pragma unroll
      for (int c = 0; c < C; ++c)
        if (raw[c * 256 + t] > 0) {
          atomicMin(&lo[c], t);
          atomicMax(&hi[c], t);
          atomicAdd(&nnz[c], 1);
        }
      if (op == 9) {  // inclusive prefix sums of the 256 bins, all channels in step
        for (int off = 1; off < 256; off <<= 1) {
          int add[C];
          __syncthreads();
#pragma unroll
          for (int c = 0; c < C; ++c) add[c] = t >= off ? cum[c * 256 + t - off] : 0;
          __syncthreads();
#pragma unroll
          for (int c = 0; c < C; ++c) cum[c * 256 + t] += add[c];
        }
      }
      __syncthreads();
#pragma unroll
      for (int c = 0; c < C; ++c) {
        int r = t;
        if (op == 8) {
          const int l = lo[c], h = hi[c];
          if (h > l && t >= l && t <= h) r = ((t - l) * 255) / (h - l);
        } else if (nnz[c] > 1) {
          const int step = (npix - raw[c * 256 + hi[c]]) / 255;
          if (step > 0) r = min(255, (step / 2 + cum[c * 256 + t] - raw[c * 256 + t]) / step);
        }
        lut[c * 256 + t] = (uint8_t)r;
      }
    }
    __syncthreads();
    ra_stream<C, PP>(ib, ob, npix, [&](int, const int* x, int* o) {
#pragma unroll
      for (int c = 0; c < C; ++c) o[c] = lut[c * 256 + x[c]];
    });
  } else if (op == 1) {
    const float m00 = wd[2], m01 = wd[3], m02 = wd[4], m10 = wd[5], m11 = wd[6], m12 = wd[7];
    ra_stream<C, PP>(ib, ob, npix, [&](int p, const int*, int* o) {
      const int i = p / W, j = p - i * W;
      const float xin = (float)j + 0.5f, yin = (float)i + 0.5f;
      const float fx = floorf((m00 * xin + m01 * yin) + m02);
      const float fy = floorf((m10 * xin + m11 * yin) + m12);
      // compared as floats: NaN and ±inf fail, and only a passing value becomes an index
      const bool inside = fx >= 0.f && fx < (float)W && fy >= 0.f && fy < (float)H;
      const uint8_t* s = ib + (inside ? ((long long)(int)fy * W + (int)fx) * C : 0ll);
#pragma unroll
      for (int c = 0; c < C; ++c) o[c] = inside ? (int)s[c] : fill;
    });
  } else if (op == 3 && C == 3) {
    ra_stream<C, PP>(ib, ob, npix, [&](int, const int* x, int* o) {
      const int g = ra_grey(x[0], x[C > 1 ? 1 : 0], x[C > 2 ? 2 : 0]);
#pragma unroll
      for (int c = 0; c < C; ++c) o[c] = ra_blend(x[c], g, v);
    });
  } else if (op == 5) {
    ra_stream<C, PP>(ib, ob, npix, [&](int p, const int* x, int* o) {
      const int i = p / W, j = p - i * W;
      const bool inner = i > 0 && i < H - 1 && j > 0 && j < W - 1;
      // border pixels read their own position nine times (an address select, no branch)
      const uint8_t* s = ib + (long long)p * C;
      const int dr = inner ? W * C : 0, dc = inner ? C : 0;
#pragma unroll
      for (int c = 0; c < C; ++c) {
        const int sum = (int)s[c - dr - dc] + (int)s[c - dr] + (int)s[c - dr + dc] + (int)s[c - dc] + 5 * x[c] +
                        (int)s[c + dc] + (int)s[c + dr - dc] + (int)s[c + dr] + (int)s[c + dr + dc];
        o[c] = ra_blend(x[c], inner ? (sum + 6) / 13 : x[c], v);
      }
    });
  } else {  // identity, color on a grey image, an op word outside the table
    ra_stream<C, PP>(ib, ob, npix, [&](int, const int* x, int* o) {
#pragma unroll
      for (int c = 0; c < C; ++c) o[c] = x[c];
    });
  }
}

template <int C, int PP>
static void ra_layer(const uint8_t* in, uint8_t* out, const float* words, int N, int layer, int* hist, int B, int H,
                     int W, int fill, hipStream_t st) {
  const int nunits = H * W / PP;
  const int bs = std::max(1, std::min(64, (nunits + 256 * 8 - 1) / (256 * 8)));
  const int ba = std::max(1, std::min(64, (nunits + 256 * 4 - 1) / (256 * 4)));
  hipLaunchKernelGGL((ra_stats_kernel<C, PP>), dim3(bs, B), dim3(256), 0, st, in, words, N, layer, hist, H * W);
  hipLaunchKernelGGL((ra_apply_kernel<C, PP>), dim3(ba, B), dim3(256), 0, st, in, out, words, N, layer,
                     (const int*)hist, H, W, fill);
}

// out, tmp: (B, H, W, C) images (tmp unused when N == 1), hist: N·B·(C+1)·256 int32, zero on entry
// (cleared on the stream by the caller); the result is in out.  C ∈ {1, 3}, 1 ≤ N (checked by the
// binding).
void rand_augment_launch(const uint8_t* src, const float* words, uint8_t* out, uint8_t* tmp, int* hist, int B, int H,
                         int W, int C, int N, int fill, hipStream_t st) {
  const long long hl = (long long)B * (C + 1) * 256;
  const uint8_t* in = src;
  for (int l = 0; l < N; ++l) {
    uint8_t* o = (N - 1 - l) % 2 == 0 ? out : tmp;  // the last layer writes out
    const bool vec = (H * W) % 4 == 0 && reinterpret_cast<uintptr_t>(in) % 4 == 0 && reinterpret_cast<uintptr_t>(o) % 4 == 0;
    int* hp = hist + hl * l;
    if (C == 3) {
      if (vec) ra_layer<3, 4>(in, o, words, N, l, hp, B, H, W, fill, st);
      else ra_layer<3, 1>(in, o, words, N, l, hp, B, H, W, fill, st);
    } else {
      if (vec) ra_layer<1, 4>(in, o, words, N, l, hp, B, H, W, fill, st);
      else ra_layer<1, 1>(in, o, words, N, l, hp, B, H, W, fill, st);
    }
    in = o;
  }
}

unsigned check_errors_randaugment(bool reset) { return pio_read_errors(reset); }

}  // namespace pio
