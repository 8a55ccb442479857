// Memory-bound kernels: text embedding (+ scale + learned position table) forward/backward,
// BERT masking, casts, row gather / index-add, batch sums.
//
// Reference parity:
//   TextInputAdapter  emb(x)·sqrt(C) + pos[:L]          perceiver/adapter.py:127-133  (SURVEY K-01)
//   TextMasking       80/10/10 BERT masking, labels      perceiver/model.py:265-293    (SURVEY K-02)
// MI355X notes: one launch each, vectorised 16-B accesses on the streaming paths; the
// masking kernel needs no host sync (the reference's nonzero/sum syncs disappear).  The
// optimizer step over the flat parameter buffer lives in optim.hip.
#include "common.h"

namespace pio {

// out[r, c] = E[ids[r], c] * scale + P[r % L, c]     (fp32), float4 vectorised over c
__global__ void embed_fwd_kernel(const int64_t* __restrict__ ids, const float* __restrict__ E,
                                 const float* __restrict__ P, float* __restrict__ out, long long rows, int L, int C,
                                 float scale, long long V) {
  const int c4 = C / 4;
  const long long n = rows * c4;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
    const long long r = i / c4;
    const int c = (int)(i % c4) * 4;
    int64_t id = ids[r];
#if PIO_CHECKS
    if (id < 0 || id >= V) {
      pio_flag(kErrEmbedId);
      id = id < 0 ? 0 : V - 1;
    }
#else
    (void)V;
#endif
    const float4 e = *reinterpret_cast<const float4*>(E + id * C + c);
    const float4 p = *reinterpret_cast<const float4*>(P + (r % L) * C + c);
    *reinterpret_cast<float4*>(out + r * C + c) =
        make_float4(e.x * scale + p.x, e.y * scale + p.y, e.z * scale + p.z, e.w * scale + p.w);
  }
}

// dE[ids[r]] += g[r] * scale, dP[l] += Σ_b g[b, l]  (both fp32 atomics)
// grid (L, ceil(B / EB)): block (l, j) handles batch rows j·EB .. j·EB+EB-1 of position l, one
// thread per channel; the EB loads per thread are issued together, then the EB scatter-adds
constexpr int EB = 16;
__global__ void embed_bwd_kernel(const int64_t* __restrict__ ids, const float* __restrict__ g, float* __restrict__ dE,
                                 float* __restrict__ dP, int B, int L, int C, float scale) {
  const int l = blockIdx.x, b0 = blockIdx.y * EB;
  for (int c = threadIdx.x; c < C; c += blockDim.x) {
    float v[EB];
    int64_t id[EB];
#pragma unroll
    for (int j = 0; j < EB; ++j) {
      const long long r = (long long)(b0 + j) * L + l;
      const bool ok = b0 + j < B;
      v[j] = ok ? g[r * C + c] : 0.f;
      id[j] = ok ? ids[r] : -1;
    }
    float acc = 0.f;
#pragma unroll
    for (int j = 0; j < EB; ++j) {
      acc += v[j];
      if (dE && id[j] >= 0) atomicAdd(dE + id[j] * C + c, v[j] * scale);
    }
    if (dP) atomicAdd(dP + (long long)l * C + c, acc);
  }
}

// dE[id] += scale · Σ g rows with that id, over token positions SORTED by id (perm = the
// sort permutation): each 64-position chunk folds its runs of equal ids in registers and adds
// one row per run, so a frequent id ([MASK] is ~12 % of an MLM batch, [PAD] of a padded one)
// costs a few atomics per chunk instead of one per occurrence.  One thread per channel.
constexpr int ES = 64;
__global__ void embed_bwd_sorted_kernel(const int64_t* __restrict__ sorted_ids, const int64_t* __restrict__ perm,
                                        const float* __restrict__ g, float* __restrict__ dE, long long n, int C,
                                        float scale) {
  const long long j0 = (long long)blockIdx.x * ES;
  for (int c = threadIdx.x; c < C; c += blockDim.x) {
    float v[ES];
#pragma unroll
    for (int j = 0; j < ES; ++j) v[j] = j0 + j < n ? g[perm[j0 + j] * C + c] : 0.f;
    int64_t cur = sorted_ids[j0];
    float acc = 0.f;
#pragma unroll
    for (int j = 0; j < ES; ++j) {
      if (j0 + j >= n) break;
      const int64_t id = sorted_ids[j0 + j];
      if (id != cur) {
        atomicAdd(dE + cur * C + c, acc * scale);
        cur = id;
        acc = 0.f;
      }
      acc += v[j];
    }
    atomicAdd(dE + cur * C + c, acc * scale);
  }
}

// dE[id] += scale · Σ g rows with that id, with NO global sort: each workgroup takes 256
// consecutive token positions, bitonic-sorts their (id, slot) keys in LDS, and every wave walks
// a quarter of the sorted keys with its g rows' loads all in flight (lane = channel), adding
// one contiguous 256-B row per run of equal ids.  A hot id ([MASK] ≈ 12 % of an MLM batch,
// [PAD], frequent words) then costs ≤ 4 row atomics per 256 tokens instead of one per
// occurrence — the property the earlier sort-by-id pipeline (≈10 launches) paid for.
// Workgroups past the token blocks do the position-table gradient dP (batch sums per
// position, embed_bwd_kernel's layout): one launch for the whole text-embedding backward.
constexpr int ET = 256;
template <int C>
__global__ __launch_bounds__(256) void embed_bwd_local_kernel(const int64_t* __restrict__ ids,
                                                              const float* __restrict__ g, float* __restrict__ dE,
                                                              float* __restrict__ dP, long long n, int nblk_e, int B,
                                                              int L, float scale, int nblk_ep, SlabJob job) {
  __shared__ uint32_t sKey[ET];
  __shared__ __attribute__((aligned(16))) float4 sPart[256];  // a deterministic slab job's partials
  const int t = threadIdx.x;
  if ((int)blockIdx.x >= nblk_ep) {  // appended workgroups: the previous backward kernel's slab job
    slab_reduce_block(job, blockIdx.x - nblk_ep, sPart);
    return;
  }
  if ((int)blockIdx.x >= nblk_e) {  // position-table gradient: block (256 / C positions, batch group)
    constexpr int TPP = C < 256 ? C : 256, PPB = 256 / TPP;
    const int nlb = (L + PPB - 1) / PPB;
    const int pb = blockIdx.x - nblk_e, l = (pb % nlb) * PPB + t / TPP, b0 = (pb / nlb) * EB;
    if (l >= L) return;
    for (int c = t % TPP; c < C; c += TPP) {
      float v[EB];
#pragma unroll
      for (int j = 0; j < EB; ++j) v[j] = b0 + j < B ? g[((long long)(b0 + j) * L + l) * C + c] : 0.f;
      float acc = 0.f;
#pragma unroll
      for (int j = 0; j < EB; ++j) acc += v[j];
      atomicAdd(dP + (long long)l * C + c, acc);
    }
    return;
  }
  const long long j0 = (long long)blockIdx.x * ET;
  sKey[t] = j0 + t < n ? ((uint32_t)ids[j0 + t] << 8) | (uint32_t)t : 0xFFFFFFFFu;  // ids < 2^24
  __syncthreads();
  for (int k = 2; k <= ET; k <<= 1) {
    for (int jj = k >> 1; jj > 0; jj >>= 1) {
      const int ix = t ^ jj;
      if (ix > t) {
        const uint32_t a = sKey[t], b = sKey[ix];
        if ((a > b) == ((t & k) == 0)) { sKey[t] = b; sKey[ix] = a; }
      }
      __syncthreads();
    }
  }
  if (dE == nullptr) return;
  constexpr int NC = C / 64;  // channels per lane (lane l: l, l + 64, ...)
  const int w = wave_id(), l = lane_id();
  const int e0 = 64 * w;
  for (int h = 0; h < 64; h += 32) {  // 32 sorted entries at a time: their loads all in flight
    float v[32][NC];
#pragma unroll
    for (int e = 0; e < 32; ++e) {
      const uint32_t key = sKey[e0 + h + e];
      const long long row = j0 + (key & 255u);
#pragma unroll
      for (int q = 0; q < NC; ++q) v[e][q] = key != 0xFFFFFFFFu ? g[row * C + l + 64 * q] : 0.f;
    }
    uint32_t cur = sKey[e0 + h] >> 8;
    float acc[NC];
#pragma unroll
    for (int q = 0; q < NC; ++q) acc[q] = 0.f;
#pragma unroll
    for (int e = 0; e < 32; ++e) {
      const uint32_t key = sKey[e0 + h + e];
      if (key == 0xFFFFFFFFu) break;  // padding past n sorts last (wave-uniform)
      if ((key >> 8) != cur) {
#pragma unroll
        for (int q = 0; q < NC; ++q) {
          atomicAdd(dE + (long long)cur * C + l + 64 * q, acc[q] * scale);
          acc[q] = 0.f;
        }
        cur = key >> 8;
      }
#pragma unroll
      for (int q = 0; q < NC; ++q) acc[q] += v[e][q];
    }
    if (cur != (0xFFFFFFFFu >> 8)) {
#pragma unroll
      for (int q = 0; q < NC; ++q) atomicAdd(dE + (long long)cur * C + l + 64 * q, acc[q] * scale);
    }
  }
}

// BERT masking with in-kernel counter-based randomness (no torch RNG kernels, no generator
// bookkeeping in a replayed graph).  Per token i, with key = hash3(seed, counter):
//   u_k = (hash3(key, k, i) >> 8) · 2^-24 (k = 0, 1, 2), rid = lo + mulhi(hash3(key, 3, i), range)
//   sel = ~special & u0 < p ; msk = sel & u1 < 0.9 ; rnd = msk & u2 < 1/9
//   x' = rnd ? rid : (msk ? MASK : x) ; label = sel ? x : -100
// state = {seed, counter, ticket}: with advance != 0 the last workgroup to finish (ticket
// count) increments the counter, so every launch — every replay of a captured step — draws
// fresh masks; every workgroup has read the counter before it takes its ticket.
__device__ __forceinline__ float unit24(uint32_t h) { return (float)(h >> 8) * (1.0f / 16777216.0f); }

// token i's outputs once its selection is known: the 80/10/10 split and the replacement id stay
// keyed by the token's own index (both masking kernels)
__device__ __forceinline__ void mask_token_out(int64_t* __restrict__ xm, int64_t* __restrict__ labels, long long i,
                                               int64_t t, bool sel, uint32_t key, int mask_id, int lo, uint32_t range) {
  const uint32_t ii = (uint32_t)i;
  const bool msk = sel & (unit24(hash3(key, 1u, ii)) < 0.9f);
  const bool rnd = msk & (unit24(hash3(key, 2u, ii)) < (1.0f / 9.0f));
  const int64_t rid = (int64_t)lo + (int64_t)__umulhi(hash3(key, 3u, ii), range);
  xm[i] = rnd ? rid : (msk ? (int64_t)mask_id : t);
  labels[i] = sel ? t : (int64_t)-100;
}
// the last workgroup to finish bumps the counter and clears the ticket (block-uniform call)
__device__ __forceinline__ void mask_advance(int64_t* __restrict__ state, int64_t ctr) {
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned* ticket = reinterpret_cast<unsigned*>(state + 2);
    if (atomicAdd(ticket, 1u) == gridDim.x - 1) {
      state[1] = ctr + 1;
      *ticket = 0u;
    }
  }
}

__global__ void text_mask_kernel(const int64_t* __restrict__ x, const bool* __restrict__ pad, int64_t* __restrict__ state,
                                 int64_t* __restrict__ xm, int64_t* __restrict__ labels, long long n, int unk_id,
                                 int mask_id, float p, int lo, uint32_t range, int advance) {
  const uint64_t seed = (uint64_t)state[0];
  const int64_t ctr = state[1];
  const uint32_t key = hash3((uint32_t)seed, (uint32_t)(seed >> 32), (uint32_t)ctr);
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
    const int64_t t = x[i];
    const bool special = (t == unk_id) | (pad != nullptr && pad[i]);
    const bool sel = !special & (unit24(hash3(key, 0u, (uint32_t)i)) < p);
    mask_token_out(xm, labels, i, t, sel, key, mask_id, lo, range);
  }
  if (advance) mask_advance(state, ctr);
}

// Whole-word BERT masking: text_mask_kernel with the SELECTION hash keyed by the index of the
// first token of the token's word, so a word is selected or left as a whole; the 80/10/10
// split and the replacement id stay per token.  cont: the vocabulary's bit-packed continuation
// table (WordPiece "##" pieces), V ids; an id outside [0, V) has bit 0 and is never an index.
//   special(i) = x[i] == unk | pad[i]
//   begin(i)   = col(i) == 0 | special(i) | special(i − 1) | !cont(x[i])
//   head(i)    = the nearest j in i, i − 1, …, i − (kWordWindow − 1) with begin(j), else i
//   sel(i)     = !special(i) & unit24(hash3(key, 0, head(i))) < p
// A row's column 0 always begins a word, so the look-back over the flat index never leaves the
// row.  The tail of a word longer than kWordWindow tokens finds no beginning in its window and
// is masked token by token.
// One thread per token, 256-token tiles in a block-uniform grid-stride loop.  Per tile every
// wave ballots two bits per token — s = special and b = col == 0 | special | !cont — into LDS
// (wave 0 also those of the kWordWindow tokens before the tile, the halo), so begin = b |
// (s shifted up one token) and head come from two 16-bit windows of the tile's bit image: no
// dependent global loads.  The bit image is double-buffered by tile parity: one barrier a tile.
static_assert(kWordWindow == 16, "the look-back window is read as 16 bits of the tile's bit image");
__global__ __launch_bounds__(256) void text_mask_words_kernel(
    const int64_t* __restrict__ x, const bool* __restrict__ pad, int64_t* __restrict__ state,
    const int32_t* __restrict__ cont, int64_t* __restrict__ xm, int64_t* __restrict__ labels, long long n, int L, int V,
    int unk_id, int mask_id, float p, int lo, uint32_t range, int advance) {
  // word 0: the halo in its top 16 bits (tokens base − 16 … base − 1), words 1–4: the tile's waves
  __shared__ unsigned long long sB[2][5], sS[2][5];
  const uint64_t seed = (uint64_t)state[0];
  const int64_t ctr = state[1];
  const uint32_t key = hash3((uint32_t)seed, (uint32_t)(seed >> 32), (uint32_t)ctr);
  const int tid = threadIdx.x, w = wave_id();
  const long long ntiles = (n + 255) / 256;
  int buf = 0;
  for (long long tile = blockIdx.x; tile < ntiles; tile += gridDim.x, buf ^= 1) {
    const long long base = tile * 256, i = base + tid;
    // this token's two bits
    const bool in = i < n;
    const int64_t t = in ? x[i] : 0;
    const bool s = in && ((t == unk_id) | (pad != nullptr && pad[i]));
    const bool tin = t >= 0 && t < V;
#if PIO_CHECKS
    if (in && !tin) pio_flag(kErrEmbedId);
#endif
    const bool c = in && tin && ((cont[tin ? t >> 5 : 0] >> (t & 31)) & 1);
    const bool b = in && (((uint32_t)i % (uint32_t)L == 0u) | s | !c);  // n < 2^32
    const unsigned long long mb = __ballot(b), ms = __ballot(s);
    if (lane_id() == 0) {
      sB[buf][1 + w] = mb;
      sS[buf][1 + w] = ms;
    }
    if (w == 0) {  // halo: lanes 0–15 of wave 0 take tokens base − 16 … base − 1 (none before token 0)
      const long long j = base - kWordWindow + tid;
      const bool hin = tid < kWordWindow && j >= 0;
      const int64_t ht = hin ? x[j] : 0;
      const bool hs = hin && ((ht == unk_id) | (pad != nullptr && pad[j]));
      const bool htin = ht >= 0 && ht < V;
      const bool hc = hin && htin && ((cont[htin ? ht >> 5 : 0] >> (ht & 31)) & 1);
      const bool hb = hin && (((uint32_t)j % (uint32_t)L == 0u) | hs | !hc);
      const unsigned long long hmb = __ballot(hb), hms = __ballot(hs);
      if (tid == 0) {
        sB[buf][0] = hmb << 48;
        sS[buf][0] = hms << 48;
      }
    }
    __syncthreads();
    if (in) {
      // bit 64 + k of the image is tile token k.  begin bits of tokens i − 15 … i: image bits from
      // q = 49 + tid; the special bits of their predecessors: from q − 1
      const int q = 64 - (kWordWindow - 1) + tid, q1 = q - 1;
      const int wq = q >> 6, sq = q & 63, wq1 = q1 >> 6, sq1 = q1 & 63;
      unsigned long long vb = sB[buf][wq] >> sq, vs = sS[buf][wq1] >> sq1;
      // a window that runs into the next word (never past word 4: q ≤ 304 = 4·64 + 48)
      if (sq > 64 - kWordWindow) vb |= sB[buf][wq + 1] << (64 - sq);
      if (sq1 > 64 - kWordWindow) vs |= sS[buf][wq1 + 1] << (64 - sq1);
      const uint32_t beg = (uint32_t)(vb | vs) & 0xFFFFu;  // bit 15: token i, bit 0: token i − 15
      const uint32_t back = beg ? (uint32_t)__clz((int)beg) - 16u : 0u;
      const bool sel = !s & (unit24(hash3(key, 0u, (uint32_t)i - back)) < p);
      mask_token_out(xm, labels, i, t, sel, key, mask_id, lo, range);
    }
  }
  if (advance) mask_advance(state, ctr);
}

__global__ void cast_bf16_kernel(const float* __restrict__ x, uint16_t* __restrict__ y, long long n) {
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x)
    y[i] = f2bf(x[i]);
}

static dim3 grid_for(long long n, int per = 256) {
  long long b = (n + per - 1) / per;
  if (b > 4096) b = 4096;
  if (b < 1) b = 1;
  return dim3((unsigned)b);
}

void embed_fwd_launch(const int64_t* ids, const float* E, const float* P, float* out, long long rows, int L, int C,
                      float scale, long long V, hipStream_t st) {
  hipLaunchKernelGGL(embed_fwd_kernel, grid_for(rows * C / 4), dim3(256), 0, st, ids, E, P, out, rows, L, C, scale, V);
}
void embed_bwd_launch(const int64_t* ids, const float* g, float* dE, float* dP, int B, int L, int C, float scale,
                      hipStream_t st) {
  hipLaunchKernelGGL(embed_bwd_kernel, dim3(L, (B + EB - 1) / EB), dim3(C < 256 ? C : 256), 0, st, ids, g, dE, dP, B, L,
                     C, scale);
}
// C a multiple of 64 (≤ 256); dE and/or dP
// + the previous backward kernel's slab job in appended workgroups (small LDS: they share the CUs
// with the embedding blocks instead of running after them)
bool embed_bwd_local_launch(const int64_t* ids, const float* g, float* dE, float* dP, int B, int L, int C, float scale,
                            const SlabJob& job, hipStream_t st) {
  if (C != 64 && C != 128 && C != 256) return false;
  const long long n = (long long)B * L;
  const int nblk_e = dE ? (int)((n + ET - 1) / ET) : 0;
  const int ppb = 256 / (C < 256 ? C : 256);
  const int nblk_p = dP ? ((L + ppb - 1) / ppb) * ((B + EB - 1) / EB) : 0;
  const int nblk_ep = nblk_e + nblk_p;
  const dim3 grid(nblk_ep + (job.slab ? job.nblk : 0));
  if (grid.x == 0) return true;
  switch (C) {
    case 64: hipLaunchKernelGGL(embed_bwd_local_kernel<64>, grid, dim3(256), 0, st, ids, g, dE, dP, n, nblk_e, B, L, scale, nblk_ep, job); break;
    case 128: hipLaunchKernelGGL(embed_bwd_local_kernel<128>, grid, dim3(256), 0, st, ids, g, dE, dP, n, nblk_e, B, L, scale, nblk_ep, job); break;
    default: hipLaunchKernelGGL(embed_bwd_local_kernel<256>, grid, dim3(256), 0, st, ids, g, dE, dP, n, nblk_e, B, L, scale, nblk_ep, job); break;
  }
  return true;
}
void embed_bwd_sorted_launch(const int64_t* sorted_ids, const int64_t* perm, const float* g, float* dE, long long n,
                             int C, float scale, hipStream_t st) {
  hipLaunchKernelGGL(embed_bwd_sorted_kernel, dim3((unsigned)((n + ES - 1) / ES)), dim3(C < 256 ? C : 256), 0, st,
                     sorted_ids, perm, g, dE, n, C, scale);
}
void text_mask_launch(const int64_t* x, const bool* pad, int64_t* state, int64_t* xm, int64_t* labels, long long n,
                      int unk_id, int mask_id, float p, int lo, uint32_t range, int advance, hipStream_t st) {
  hipLaunchKernelGGL(text_mask_kernel, grid_for(n), dim3(256), 0, st, x, pad, state, xm, labels, n, unk_id, mask_id, p, lo,
                     range, advance);
}
void text_mask_words_launch(const int64_t* x, const bool* pad, int64_t* state, const int32_t* cont, int64_t* xm,
                            int64_t* labels, long long n, int L, int V, int unk_id, int mask_id, float p, int lo,
                            uint32_t range, int advance, hipStream_t st) {
  hipLaunchKernelGGL(text_mask_words_kernel, grid_for(n), dim3(256), 0, st, x, pad, state, cont, xm, labels, n, L, V,
                     unk_id, mask_id, p, lo, range, advance);
}
// dst[idx[r]][:] += src[r][:] — the backward of a row gather (rows of idx may repeat: fp32
// atomics; an index outside dst is skipped).  One thread per 4 columns.
__global__ void index_add_rows_kernel(float* __restrict__ dst, long long nrows, const int64_t* __restrict__ idx,
                                      const float* __restrict__ src, long long R, int C) {
  const int c4 = C >> 2;
  const long long total = R * c4;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const long long r = i / c4;
    const int c = (int)(i - r * c4) * 4;
    const long long d = idx[r];
#if PIO_CHECKS
    if (d < 0 || d >= nrows) pio_flag(kErrGatherRow);
#endif
    const float4 v = *reinterpret_cast<const float4*>(src + r * C + c);
    // all-zero quads (padding rows of a fixed-capacity gather) skip their atomics: padding
    // slots often share one destination row, whose serialised atomics would dominate
    const bool nz = v.x != 0.f || v.y != 0.f || v.z != 0.f || v.w != 0.f;
    if (nz && d >= 0 && d < nrows) {
      float* p = dst + d * C + c;
      atomicAdd(p, v.x);
      atomicAdd(p + 1, v.y);
      atomicAdd(p + 2, v.z);
      atomicAdd(p + 3, v.w);
    }
  }
}
void index_add_rows_launch(float* dst, long long nrows, const int64_t* idx, const float* src, long long R, int C,
                           hipStream_t st) {
  hipLaunchKernelGGL(index_add_rows_kernel, grid_for(R * (C / 4)), dim3(256), 0, st, dst, nrows, idx, src, R, C);
}
// out (R, C) = src[idx] (the forward of that gather: a decoder's output queries at the pixels of a
// sparse image); an index outside [0, nrows) yields a zero row
__global__ void gather_rows_kernel(float* __restrict__ out, const float* __restrict__ src, long long nrows,
                                   const int64_t* __restrict__ idx, long long R, int C) {
  const int c4 = C >> 2;
  const long long total = R * c4;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const long long r = i / c4;
    const int c = (int)(i - r * c4) * 4;
    const long long d = idx[r];
#if PIO_CHECKS
    if (d < 0 || d >= nrows) pio_flag(kErrGatherRow);
#endif
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (d >= 0 && d < nrows) v = *reinterpret_cast<const float4*>(src + d * C + c);
    *reinterpret_cast<float4*>(out + r * C + c) = v;
  }
}
void gather_rows_launch(float* out, const float* src, long long nrows, const int64_t* idx, long long R, int C,
                        hipStream_t st) {
  hipLaunchKernelGGL(gather_rows_kernel, grid_for(R * (C / 4)), dim3(256), 0, st, out, src, nrows, idx, R, C);
}
// Σ over the batch of two (B, n) fp32 tensors in one launch: oa = Σ_b a[b], ob = Σ_b b[b] (the
// gradients of a batch-broadcast query stream: dQ and the residual dY of the first cross-attention
// over the shared latent array).  Block = 64 float4 columns × 4 batch groups, fixed summation
// order (deterministic).  n a multiple of 4, 16-byte aligned rows.
__global__ __launch_bounds__(256) void batch_sum2_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                         float* __restrict__ oa, float* __restrict__ ob, int B,
                                                         long long na4, long long nb4, int acc_b) {
  __shared__ float4 part[4][64];
  const int l = threadIdx.x & 63, g = threadIdx.x >> 6;
  const long long c = (long long)blockIdx.x * 64 + l;  // float4 column of [a | b]
  const bool second = c >= na4;
  const long long cc = second ? c - na4 : c, n4 = second ? nb4 : na4;
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  if (c < na4 + nb4) {
    const float4* src = reinterpret_cast<const float4*>(second ? b : a) + cc;
#pragma unroll 8
    for (int bb = g; bb < B; bb += 4) {
      const float4 v = src[(long long)bb * n4];
      acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
    }
  }
  part[g][l] = acc;
  __syncthreads();
  if (g == 0 && c < na4 + nb4) {
    float4 r = part[0][l];
#pragma unroll
    for (int k = 1; k < 4; ++k) {
      const float4 v = part[k][l];
      r.x += v.x; r.y += v.y; r.z += v.z; r.w += v.w;
    }
    float4* dst = reinterpret_cast<float4*>(second ? ob : oa) + cc;
    if (second && acc_b) {  // ob += Σ_b b (e.g. straight into a parameter's gradient)
      const float4 o = *dst;
      r.x += o.x; r.y += o.y; r.z += o.z; r.w += o.w;
    }
    *dst = r;
  }
}
void batch_sum2_launch(const float* a, const float* b, float* oa, float* ob, int B, long long na, long long nb, int acc_b,
                       hipStream_t st) {
  const long long na4 = a ? na / 4 : 0, nb4 = nb / 4;
  hipLaunchKernelGGL(batch_sum2_kernel, dim3((unsigned)((na4 + nb4 + 63) / 64)), dim3(256), 0, st, a, b, oa, ob, B, na4,
                     nb4, acc_b);
}

// standalone form of a SlabJob (common.h): the reductions still pending at the end of a
// backward pass
__global__ __launch_bounds__(256) void slab_reduce_kernel(SlabJob job) {
  __shared__ float4 part[256];
  slab_reduce_block(job, blockIdx.x, part);
}
void slab_reduce_launch(const SlabJob& job, hipStream_t st) {
  if (job.slab == nullptr || job.nblk == 0) return;
  hipLaunchKernelGGL(slab_reduce_kernel, dim3(job.nblk), dim3(256), 0, st, job);
}

// one wave: the cross-lane reduction helpers of common.h on x[0..63] (numerics self-test)
__global__ void reduce_probe_kernel(const float* __restrict__ x, float* __restrict__ out) {
  const int l = threadIdx.x;
  const float v = x[l];
  out[l] = wave_sum(v);
  out[64 + l] = wave_max(v);
  out[128 + l] = half_sum(v);
  out[192 + l] = half_max(v);
  out[256 + l] = xor16_sum(v);
  out[320 + l] = xor32_sum(v);
}

void reduce_probe_launch(const float* x, float* out, hipStream_t st) {
  hipLaunchKernelGGL(reduce_probe_kernel, dim3(1), dim3(64), 0, st, x, out);
}

void cast_bf16_launch(const float* x, uint16_t* y, long long n, hipStream_t st) {
  hipLaunchKernelGGL(cast_bf16_kernel, grid_for(n), dim3(256), 0, st, x, y, n);
}

}  // namespace pio

// ------------------------------------------------------------------------------------------
// Per-step staging for a replayed hipGraph in ONE launch: the new batch's tensors are copied
// into the graph's static input buffers and the optimizer's per-step hyper-parameters (lr,
// step, betas, ...) arrive as kernel arguments (captured by value at launch, so no pinned
// staging ring and no host→device copy).  Replaces one copyBuffer per input tensor + one for
// the hyper-parameters.  Segments whose pointers and size are 16-byte multiples are copied in
// 16-byte units, the others byte-wise.
// ------------------------------------------------------------------------------------------
namespace pio {
// kStageHyper: the optimizer's 8 global words + 4 per parameter group, at most 8 groups
constexpr int kStageSegs = 8, kStageHyper = 40, kStageSeeds = 64;
struct StageArgs {
  void* dst[kStageSegs];
  const void* src[kStageSegs];
  long long bytes[kStageSegs];
  int vec[kStageSegs];
  int nseg;
  float* hyper_dst;
  float hyper[kStageHyper];
  int nhyper;
  long long* seed_dst;  // a captured step's dropout seed slots (ops/fused.py static seeds)
  long long seeds[kStageSeeds];
  int nseeds;
};

__global__ __launch_bounds__(256) void stage_step_kernel(StageArgs a) {
  const long long tid = (long long)blockIdx.x * blockDim.x + threadIdx.x, nt = (long long)gridDim.x * blockDim.x;
  if (blockIdx.x == 0 && threadIdx.x < a.nhyper && a.hyper_dst != nullptr) a.hyper_dst[threadIdx.x] = a.hyper[threadIdx.x];
  if (blockIdx.x == 0 && threadIdx.x < a.nseeds) a.seed_dst[threadIdx.x] = a.seeds[threadIdx.x];
  for (int s = 0; s < a.nseg; ++s) {
    if (a.vec[s]) {
      const long long n = a.bytes[s] >> 4;
      uint4* d = reinterpret_cast<uint4*>(a.dst[s]);
      const uint4* x = reinterpret_cast<const uint4*>(a.src[s]);
      for (long long i = tid; i < n; i += nt) d[i] = x[i];
    } else {
      uint8_t* d = reinterpret_cast<uint8_t*>(a.dst[s]);
      const uint8_t* x = reinterpret_cast<const uint8_t*>(a.src[s]);
      for (long long i = tid; i < a.bytes[s]; i += nt) d[i] = x[i];
    }
  }
}

int stage_step_launch(void* const* dst, const void* const* src, const long long* bytes, int nseg, float* hyper_dst,
                      const float* hyper, int nhyper, long long* seed_dst, const long long* seeds, int nseeds,
                      hipStream_t st) {
  if (nseg > kStageSegs || nhyper > kStageHyper || nseeds > kStageSeeds || (nseeds > 0 && seed_dst == nullptr)) return -1;
  StageArgs a{};
  a.seed_dst = seed_dst;
  a.nseeds = nseeds;
  for (int i = 0; i < nseeds; ++i) a.seeds[i] = seeds[i];
  long long units = 0;
  for (int s = 0; s < nseg; ++s) {
    a.dst[s] = dst[s];
    a.src[s] = src[s];
    a.bytes[s] = bytes[s];
    a.vec[s] = ((reinterpret_cast<uintptr_t>(dst[s]) | reinterpret_cast<uintptr_t>(src[s]) | (uintptr_t)bytes[s]) & 15) == 0;
    const long long u = a.vec[s] ? bytes[s] >> 4 : bytes[s];
    units = u > units ? u : units;
  }
  a.nseg = nseg;
  a.hyper_dst = hyper_dst;
  for (int i = 0; i < nhyper; ++i) a.hyper[i] = hyper[i];
  a.nhyper = hyper_dst ? nhyper : 0;
  long long blocks = (units + 255) / 256;
  blocks = blocks < 1 ? 1 : (blocks > 1024 ? 1024 : blocks);
  hipLaunchKernelGGL(stage_step_kernel, dim3((unsigned)blocks), dim3(256), 0, st, a);
  return 0;
}
}  // namespace pio

namespace pio {
unsigned check_errors_elementwise(bool reset) { return pio_read_errors(reset); }
}  // namespace pio

