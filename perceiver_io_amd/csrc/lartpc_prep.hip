// event_compact: a dense LArTPC training event → the sparse batch of data/lartpc.py sparse_collate,
// on the device, read through one of the eight symmetries of the square.
//
// Per sample b the int32 word words[b] (device memory: a replayed graph follows whatever was staged)
// picks the transform.  Output pixel (i, j) of the transformed event takes source pixel (i', j'):
//   bit 2 (first): (i', j') = (j, i), else (i, j);  bit 0: j' = W − 1 − j';  bit 1: i' = H − 1 − i'.
// H == W is required by the launcher (it cannot see the words), so every source index lies inside
// the plane whatever the word holds.  A word outside 0–7 is the identity (the checked build flags
// kErrDihedral).
//
// Two ordered compactions run over the same walk of the transformed event, in its flat order:
//   keys    — img != 0 (−0.0 is zero, NaN is not): values / index / kmask, padding (0, 0, True);
//   queries — label < 8 with its bit set in wmask: qidx / qlab (int64), padding slot j holds
//             (j % npix, −100).  A label at or past ncls is not weighted by any caller; the
//             checked build flags it (kErrLabel).
// counts[b] = {keys, queries} of the sample, also beyond the capacities.
//
// The segment layout, count + scatter split and tile scan are nonzero_compact's (compact.h); both
// predicates are evaluated from one read of the image and the label plane per launch.  The
// transposed codes read the source down its columns: one cache line per lane and load, served by
// L2 (a 512 × 512 plane is 1 MB; profiles/lartpc_prep.md has the measured cost).
#include "common.h"
#include "compact.h"

namespace pio {

struct Dihedral {
  int H, W;
  bool tr, fx, fy;
  // flat source index of flat output index o (o < H·W)
  __device__ __forceinline__ int src(int o) const {
    const int i = (int)((unsigned)o / (unsigned)W), j = o - i * W;
    int si = tr ? j : i, sj = tr ? i : j;
    sj = fx ? W - 1 - sj : sj;
    si = fy ? H - 1 - si : si;
    return si * W + sj;
  }
};

__device__ __forceinline__ Dihedral dihedral_of(const int* __restrict__ words, int b, int H, int W) {
  int code = words[b];
  if ((unsigned)code > 7u) {
    if (blockIdx.x == 0 && threadIdx.x == 0) pio_flag(kErrDihedral);
    code = 0;
  }
  return Dihedral{H, W, (code & 4) != 0, (code & 1) != 0, (code & 2) != 0};
}

__device__ __forceinline__ bool query_hit(unsigned lab, unsigned wmask, int ncls) {
  if (lab >= (unsigned)ncls) pio_flag(kErrLabel);
  return lab < 8u && ((wmask >> lab) & 1u) != 0u;
}

// segcount[(b·S + s)·2 + {0, 1}]: keys and queries of segment s of the transformed sample b
__global__ __launch_bounds__(NZ_THREADS) void event_count_kernel(EventCompactArgs a, long long seg) {
  const int s = blockIdx.x, b = blockIdx.y, S = gridDim.x;
  const long long npix = (long long)a.H * a.W;
  const long long start = (long long)s * seg, end = start + seg < npix ? start + seg : npix;
  const Dihedral d = dihedral_of(a.words, b, a.H, a.W);
  const float* p = a.img + (long long)b * npix;
  const uint8_t* q = a.lab + (long long)b * npix;
  int nk = 0, nq = 0;
  for (long long o = start + threadIdx.x; o < end; o += NZ_THREADS) {
    const int i = d.src((int)o);
    nk += p[i] != 0.f ? 1 : 0;
    nq += query_hit(q[i], a.wmask, a.ncls) ? 1 : 0;
  }
  __shared__ int sK[NZ_WAVES], sQ[NZ_WAVES];
  nk = block_isum(nk, sK);
  nq = block_isum(nq, sQ);
  if (threadIdx.x == 0) {
    a.segcount[((long long)b * S + s) * 2] = nk;
    a.segcount[((long long)b * S + s) * 2 + 1] = nq;
  }
}

template <int V>
__global__ __launch_bounds__(NZ_THREADS) void event_scatter_kernel(EventCompactArgs a, long long seg) {
  constexpr int TILE = NZ_THREADS * V;
  const int s = blockIdx.x, b = blockIdx.y, S = gridDim.x;
  const long long npix = (long long)a.H * a.W, kcap = a.kcap, qcap = a.qcap;
  __shared__ int sWk[2][V][NZ_WAVES], sWq[2][V][NZ_WAVES];
  __shared__ int sRk[2][NZ_WAVES], sRq[2][NZ_WAVES];
  long long runk = 0, totk = 0, runq = 0, totq = 0;
  if (S > 1) {  // S <= NZ_THREADS
    const int* sc = a.segcount + (long long)b * S * 2;
    seg_prefix(sc, 2, s, S, sRk, runk, totk);
    seg_prefix(sc + 1, 2, s, S, sRq, runq, totq);
  }
  const long long start = (long long)s * seg, end = start + seg < npix ? start + seg : npix;
  const Dihedral d = dihedral_of(a.words, b, a.H, a.W);
  const float* p = a.img + (long long)b * npix;
  const uint8_t* q = a.lab + (long long)b * npix;
  float* vo = a.values + (long long)b * kcap;
  int64_t* io = a.index + (long long)b * kcap;
  bool* mo = a.kmask + (long long)b * kcap;
  int64_t* qi = a.qidx + (long long)b * qcap;
  int64_t* ql = a.qlab + (long long)b * qcap;
  int buf = 0;
  // a counting call (both capacities 0) with S > 1 already has its totals: no second read
  const bool walk = S == 1 || kcap > 0 || qcap > 0;
  for (long long t0 = start; walk && t0 < end; t0 += TILE, buf ^= 1) {
    float v[V];
    unsigned lb[V];
    bool hk[V], hq[V];
    int prek[V], preq[V];
#pragma unroll
    for (int j = 0; j < V; ++j) {
      const long long o = t0 + j * NZ_THREADS + threadIdx.x;
      const bool in = o < end;
      const int i = in ? d.src((int)o) : 0;
      v[j] = in ? p[i] : 0.f;
      lb[j] = in ? (unsigned)q[i] : 0u;
      hk[j] = v[j] != 0.f;
      hq[j] = in && query_hit(lb[j], a.wmask, a.ncls);
    }
    tile_ballot<V>(hk, prek, sWk[buf]);
    tile_ballot<V>(hq, preq, sWq[buf]);
    lds_sync();
#pragma unroll
    for (int j = 0; j < V; ++j) {
      const long long o = t0 + j * NZ_THREADS + threadIdx.x;
      const long long pk = tile_slot(sWk[buf][j], prek[j], runk);
      const long long pq = tile_slot(sWq[buf][j], preq[j], runq);
      if (hk[j] && pk < kcap) {
        vo[pk] = v[j];
        io[pk] = o;
        mo[pk] = false;
      }
      if (hq[j] && pq < qcap) {
        qi[pq] = o;
        ql[pq] = (int64_t)lb[j];
      }
    }
  }
  if (S == 1) { totk = runk; totq = runq; }
  // padding slots [min(total, cap), cap) of the sample, dealt over its S blocks
  for (long long j = (totk < kcap ? totk : kcap) + (long long)s * NZ_THREADS + threadIdx.x; j < kcap;
       j += (long long)S * NZ_THREADS) {
    vo[j] = 0.f;
    io[j] = 0;
    mo[j] = true;
  }
  for (long long j = (totq < qcap ? totq : qcap) + (long long)s * NZ_THREADS + threadIdx.x; j < qcap;
       j += (long long)S * NZ_THREADS) {
    qi[j] = j % npix;
    ql[j] = -100;
  }
  if (s == 0 && threadIdx.x == 0) {
    a.counts[b * 2] = (int)totk;
    a.counts[b * 2 + 1] = (int)totq;
  }
}

// a.S in [1, 256] segments per sample, a.V in {4, 8}; a.segcount: (B, S, 2) int32 scratch (unused
// when S == 1); H == W and H·W < 2^31 are the caller's to check
void event_compact_launch(const EventCompactArgs& a, hipStream_t st) {
  const long long seg = compact_seg_len((long long)a.H * a.W, a.S, a.V);
  const dim3 g(a.S, a.B), t(NZ_THREADS);
  if (a.S > 1) hipLaunchKernelGGL(event_count_kernel, g, t, 0, st, a, seg);
  if (a.V == 8) hipLaunchKernelGGL(event_scatter_kernel<8>, g, t, 0, st, a, seg);
  else hipLaunchKernelGGL(event_scatter_kernel<4>, g, t, 0, st, a, seg);
}

unsigned check_errors_lartpc_prep(bool reset) { return pio_read_errors(reset); }

}  // namespace pio
