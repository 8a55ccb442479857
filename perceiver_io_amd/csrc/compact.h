// Ordered stream compaction shared by nonzero_compact (pixel_head.hip) and event_compact
// (lartpc_prep.hip): the segment layout, the per-segment count, the segment prefix and the tile
// scan.  A sample is cut into S segments of whole tiles of 256·V elements; a count launch sums the
// selected elements of each segment, and the scatter launch turns those sums into its segment's
// base slot and walks the segment tile by tile: one ballot per load, wave totals through a
// ping-pong LDS buffer (one barrier per tile), the running base in a register of every thread.
// Order comes from the scans alone (no atomics).
#pragma once
#include "common.h"

namespace pio {

constexpr int NZ_THREADS = 256, NZ_WAVES = NZ_THREADS / 64;

__device__ __forceinline__ int wave_isum(int v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
  return v;
}

// the block's sum of n (one barrier); sW: NZ_WAVES ints of LDS
__device__ __forceinline__ int block_isum(int n, int* sW) {
  n = wave_isum(n);
  if (lane_id() == 0) sW[wave_id()] = n;
  __syncthreads();
  return sW[0] + sW[1] + sW[2] + sW[3];
}

// segment counts seg[i · stride], i < S <= NZ_THREADS, of one sample → the slots before segment s
// (run) and the sample's total; sR: 2 × NZ_WAVES ints of LDS (one barrier)
__device__ __forceinline__ void seg_prefix(const int* __restrict__ seg, int stride, int s, int S, int (*sR)[NZ_WAVES],
                                           long long& run, long long& total) {
  const int l = lane_id(), w = wave_id();
  const int c = (int)threadIdx.x < S ? seg[(long long)threadIdx.x * stride] : 0;
  const int before = wave_isum((int)threadIdx.x < s ? c : 0), all = wave_isum(c);
  if (l == 0) { sR[0][w] = before; sR[1][w] = all; }
  __syncthreads();
  run = sR[0][0] + sR[0][1] + sR[0][2] + sR[0][3];
  total = sR[1][0] + sR[1][1] + sR[1][2] + sR[1][3];
}

// first half of a tile's scan: load j's rank among the selected lanes of its wave below this one
// (pre[j]), the wave totals to sW[j][wave].  An lds_sync() separates it from tile_slot.
template <int V>
__device__ __forceinline__ void tile_ballot(const bool (&hit)[V], int (&pre)[V], int (*sW)[NZ_WAVES]) {
  const int l = lane_id(), w = wave_id();
  const uint64_t below = (1ull << l) - 1ull;
#pragma unroll
  for (int j = 0; j < V; ++j) {
    const uint64_t m = __ballot(hit[j]);
    pre[j] = __popcll(m & below);
    if (l == 0) sW[j][w] = __popcll(m);
  }
}

// second half: the slot of this thread's load j (meaningful where it is selected); run advances by
// the load's block total
__device__ __forceinline__ long long tile_slot(const int* sWj, int pre, long long& run) {
  const int w = wave_id();
  int woff = 0, tot = 0;
#pragma unroll
  for (int k = 0; k < NZ_WAVES; ++k) {
    const int c = sWj[k];
    woff += k < w ? c : 0;
    tot += c;
  }
  const long long pos = run + woff + pre;
  run += tot;
  return pos;
}

// pixels per segment for S segments: whole tiles of 256·V
inline long long compact_seg_len(long long npix, int S, int V) {
  const long long tile = (long long)NZ_THREADS * V, per = (npix + S - 1) / S;
  return (per + tile - 1) / tile * tile;
}

}  // namespace pio
