// drift.hip -- the drift search: sums of rows along straight lines of frequency drift, and the largest sum per bin with its drift
// (glfer_hip.h, "Drift search"; the definition is restated in drift_params.h).
//
// A workgroup owns kDriftBlock bins of one block of one stream, a bin a lane.  It streams the block's T rows through LDS: the
// tile and a halo of max(|dmin|, dmax) bins each side, bins outside the row written as +0.0f (the padding between bins and pitch
// and the next row are never read).  Two tiles: row t + 1 is loaded from global memory into registers before row t's adds and
// written to the other tile after them, one barrier a row.  A lane keeps one accumulator per drift of the current group in
// registers under compile-time indices (the group capacity G is the template argument; T is not); a request for more drifts
// than G is further passes of the same lanes over the block's rows, so best / drift merge in registers.
//
// o(d, t) is wave-uniform.  Lane g of every wavefront carries the offset of the group's drift g forward from row to row (the
// remainder of the division by 2 (T - 1) grows by 2 |d| a row and gives up at most one step: integers only, exact), and a
// (d, t) step is one v_readlane of that offset, one LDS read of consecutive words and one add.
#include "drift_params.h"

namespace glfer {

// the scan order 0, +1, -1, +2, -2, ... as a rank
__device__ __forceinline__ int drift_rank(int d) { return d == 0 ? 0 : d > 0 ? 2 * d - 1 : -2 * d; }

template <int G>
__global__ __launch_bounds__(kDriftBlock) void drift_kernel(const DriftParams q) {
  static_assert(G >= 1 && G <= 64, "a wavefront's lanes hold the group's offsets");
  __shared__ float tile[2][kDriftTileWords];
  const int lane = threadIdx.x, wl = lane & 63;
  const int k0 = (int)blockIdx.x * kDriftBlock, k = k0 + lane;
  const long long b = q.block0 + (long long)blockIdx.y, s = (long long)blockIdx.z;
  const int T = q.frames, D = q.dmax - q.dmin + 1, halo = q.halo, bins = q.bins;
  const int words = kDriftBlock + 2 * halo;            // of a staged tile: <= kDriftTileWords
  const int den = 2 * (T - 1);
  const float *row0 = q.rows + s * q.row_stride + b * q.step * q.pitch;
  const bool want_best = q.best || q.drift;

  float bv = -__builtin_inff(), v0 = 0.0f;
  int bd = 0, br = 0x7fffffff;

  for (int d0 = q.dmin; d0 <= q.dmax; d0 += G) {
    const int ng = min(G, q.dmax - d0 + 1);
    float acc[G];
#pragma unroll
    for (int g = 0; g < G; g++) acc[g] = 0.0f;
    // this lane's drift of the group (lanes past the group keep the first), its offset at row 0 and the remainder
    const int dg = d0 + (wl < ng ? wl : 0), inc = 2 * (dg < 0 ? -dg : dg);
    int off = 0, rem = T - 1;

    float r[3];
#pragma unroll
    for (int i = 0; i < 3; i++) {
      const int idx = lane + i * kDriftBlock, bin = k0 - halo + idx;
      r[i] = (idx < words && bin >= 0 && bin < bins) ? row0[bin] : 0.0f;
    }
#pragma unroll
    for (int i = 0; i < 3; i++) {
      const int idx = lane + i * kDriftBlock;
      if (idx < words) tile[0][idx] = r[i];
    }
    __syncthreads();

    for (int t = 0; t < T; t++) {
      if (t + 1 < T) {
        const float *next = row0 + (long long)(t + 1) * q.pitch;
#pragma unroll
        for (int i = 0; i < 3; i++) {
          const int idx = lane + i * kDriftBlock, bin = k0 - halo + idx;
          r[i] = (idx < words && bin >= 0 && bin < bins) ? next[bin] : 0.0f;
        }
      }
      const float *cur = &tile[t & 1][halo + lane];
      const int signed_off = dg < 0 ? -off : off;
      // eight drifts to a uniform branch (a guard per drift becomes G lane masks in SGPRs the kernel does not have); the up to
      // seven accumulators past the group's last drift add its first drift's line and are never looked at
#pragma unroll
      for (int c = 0; c < G; c += 8) {
        if (c < ng) {
#pragma unroll
          for (int g = c; g < c + 8; g++) acc[g] += cur[__builtin_amdgcn_readlane(signed_off, g)];
        }
      }
      rem += inc;
      if (rem >= den) {
        rem -= den;
        off++;
      }
      if (t + 1 < T) {
#pragma unroll
        for (int i = 0; i < 3; i++) {
          const int idx = lane + i * kDriftBlock;
          if (idx < words) tile[(t + 1) & 1][idx] = r[i];
        }
      }
      __syncthreads();
    }

    if (q.sums && k < bins) {
      float *out = q.sums + s * q.sums_stride + ((b * D + (d0 - q.dmin)) * bins + k);
      // the row stride made opaque here: known to the compiler it becomes G products g * bins held in SGPR pairs through the frame loop
      long long stride = bins;
      asm volatile("" : "+s"(stride));
#pragma unroll
      for (int g = 0; g < G; g++) {
        if (g < ng) {
          *out = acc[g];
          out += stride;
        }
      }
    }
    if (want_best) {
#pragma unroll
      for (int g = 0; g < G; g++) {
        if (g < ng) {
          const int d = d0 + g, rank = drift_rank(d);
          const float v = acc[g];
          if (d == 0) v0 = v;
          if (v > bv || (v == bv && rank < br)) {
            bv = v;
            bd = d;
            br = rank;
          }
        }
      }
    }
  }

  if (want_best && k < bins) {
    if (v0 != v0) {          // the scan starts on the zero-drift line and nothing is > NaN
      bv = v0;
      bd = 0;
    }
    if (q.best) q.best[s * q.best_stride + b * bins + k] = bv;
    if (q.drift) q.drift[s * q.drift_stride + b * bins + k] = (short)bd;
  }
}

template <int G>
static hipError_t launch(const DriftParams &q, hipStream_t st) {
  const dim3 grid((unsigned)((q.bins + kDriftBlock - 1) / kDriftBlock), q.nblocks_here, q.nstreams_here);
  hipLaunchKernelGGL(drift_kernel<G>, grid, dim3(kDriftBlock), 0, st, q);
  return hipGetLastError();
}

}  // namespace glfer

extern "C" hipError_t glfer_launch_drift(const DriftParams *p, hipStream_t st) {
  if (p->halo < 0 || p->halo > kDriftHaloMax || p->frames < 2 || p->nblocks_here == 0 || p->nstreams_here == 0) return hipErrorInvalidValue;
  switch (drift_group(p->dmax - p->dmin + 1)) {
    case 8: return glfer::launch<8>(*p, st);
    case 32: return glfer::launch<32>(*p, st);
    default: return glfer::launch<kDriftMaxGroup>(*p, st);
  }
}
