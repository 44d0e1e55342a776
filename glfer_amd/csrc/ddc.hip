// ddc.hip -- digital down-converter: a frequency-translating, decimating FIR over a device stream (gfx950).
//
//   y[m] = exp(-2 pi i phi(n0)) sum_{t < T} g[t] x[n0 - t],   n0 = (m + 1) D - 1,   phi(n) = (W n mod 2^64) / 2^64 turns,
//
// x real or complex (interleaved I/Q) in f32 / s16 / u8, zero before sample 0; g[t] = h[t] exp(+2 pi i phi(t)) the complex taps made
// on the host; y complex64.  One rotation per OUTPUT instead of a mixer multiply per input sample.
//
// Layout (ddc_params.h).  A tile is 1024 consecutive outputs of one stream, four per lane.  Its samples are staged in LDS by phase,
// converted to float (exact): sample n in row D - 1 - (n mod D), column n div D.  Tap t = j D + r of output m then reads row r at
// column m - j: consecutive outputs read consecutive words whatever D is (read straight from the stream they would be D words
// apart: every lane on one bank at D = 32 or 64), and the tap is wave-uniform -- it comes through the scalar cache, not from LDS.
// The sum runs over the rows r outermost and j = 0, 1, ... inside a row, so along a row the four outputs of a lane and eight
// consecutive j need 11 consecutive words: three 16-byte LDS reads feed 64 FMAs (128 for complex input), against one 4-byte
// read per two FMAs for a lane per output.  That order depends on t (and the handle's D) alone; a tile, a launch, a frame range
// or a batch only decide WHICH outputs a lane owns, never how one is summed, and a sample outside the stream enters as the
// same 0.0f multiply-add a sample inside would be -- so an output's bits do not depend on where it falls.
// Any D <= 1024 and T <= 8192: rows are staged ddc_rows_per_chunk at a time (a row is at most 1024 + 8192 columns: one always
// fits), in the same order.
//
// The rotation: W n0 in 64-bit integers (no drift at any stream length), negated, taken as a signed fraction of a turn in double
// and given to one double sincospi per output, each part rounded once to float.  A table of 1024 angles (floats with their rounding
// remainders) plus a small-angle series for the low 54 bits was built as well and measured at D = 2, T = 9: its 16-byte gather
// per output made the whole kernel 1.22x SLOWER than the double form (profiles/ddc_rate.txt), so it is not kept.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "ddc_params.h"

namespace glfer {

typedef float v4f __attribute__((ext_vector_type(4)));

// one sample, converted as everywhere in this library (x / 32768, (x - 128) / 128); CPLX: the pair at complex index n
template <int FMT, int CPLX>
__device__ __forceinline__ void ddc_load(const char *base, long long n, float &re, float &im) {
  im = 0.0f;
  if constexpr (FMT == GLFER_FMT_F32) {
    if constexpr (CPLX) {
      const float2 v = *reinterpret_cast<const float2 *>(base + n * 8);
      re = v.x;
      im = v.y;
    } else {
      re = *reinterpret_cast<const float *>(base + n * 4);
    }
  } else if constexpr (FMT == GLFER_FMT_S16) {
    if constexpr (CPLX) {
      const unsigned v = *reinterpret_cast<const unsigned *>(base + n * 4);
      re = (float)(short)(v & 0xffffu) / 32768.0f;
      im = (float)(short)(v >> 16) / 32768.0f;
    } else {
      re = (float)*reinterpret_cast<const short *>(base + n * 2) / 32768.0f;
    }
  } else {
    if constexpr (CPLX) {
      const unsigned v = *reinterpret_cast<const unsigned short *>(base + n * 2);
      re = ((float)(v & 0xffu) - 128.0f) / 128.0f;
      im = ((float)(v >> 8) - 128.0f) / 128.0f;
    } else {
      re = ((float)*reinterpret_cast<const unsigned char *>(base + n) - 128.0f) / 128.0f;
    }
  }
}

// taps j0 .. j0 + cnt - 1 (cnt = 8 when FULL) of one row for the lane's four outputs; w: the row at column (lane's first) - j0 - 8
template <bool FULL, int CPLX>
__device__ __forceinline__ void ddc_row_block(const float *w, int plane, const float2 *__restrict__ g, int cnt, float (&ar)[4],
                                              float (&ai)[4]) {
  float xr[12], xi[12];
#pragma unroll
  for (int q = 0; q < 3; q++) {
    const v4f a = *reinterpret_cast<const v4f *>(w + 4 * q);
    xr[4 * q] = a.x, xr[4 * q + 1] = a.y, xr[4 * q + 2] = a.z, xr[4 * q + 3] = a.w;
    if constexpr (CPLX) {
      const v4f b = *reinterpret_cast<const v4f *>(w + plane + 4 * q);
      xi[4 * q] = b.x, xi[4 * q + 1] = b.y, xi[4 * q + 2] = b.z, xi[4 * q + 3] = b.w;
    }
  }
#pragma unroll
  for (int i = 0; i < kDdcJBlock; i++) {
    if (FULL || i < cnt) {
      const float2 c = g[i];
#pragma unroll
      for (int k = 0; k < kDdcPerLane; k++) {
        const int q = kDdcJBlock + k - i;                   // column m - j of output k, tap j0 + i
        ar[k] = __builtin_fmaf(c.x, xr[q], ar[k]);
        if constexpr (CPLX) ar[k] = __builtin_fmaf(-c.y, xi[q], ar[k]);
        if constexpr (CPLX) ai[k] = __builtin_fmaf(c.x, xi[q], ai[k]);
        ai[k] = __builtin_fmaf(c.y, xr[q], ai[k]);
      }
    }
  }
}

template <int FMT, int CPLX>
__global__ __launch_bounds__(kDdcBlock) void ddc_kernel(DdcParams p, const void *__restrict__ in_, const float2 *__restrict__ taps,
                                                        float2 *__restrict__ out_) {
  extern __shared__ __attribute__((aligned(16))) float lds[];   // [planes][p.plane]: p.rc rows of p.cols words
  const char *in = reinterpret_cast<const char *>(in_) + (long long)blockIdx.y * p.in_stride;
  float2 *out = out_ + (long long)blockIdx.y * p.out_stride;
  const int tid = (int)threadIdx.x;
  const int D = p.D, cols = p.cols;

  for (int tile = (int)blockIdx.x; tile < p.ntiles; tile += (int)gridDim.x) {
    const long long m0 = p.first_out + (long long)tile * kDdcTile;
    const long long cbase = m0 - p.jpad;                         // the column staged at word 0 of a row
    const long long live64 = p.end_out - cbase;                  // columns from here on hold no output of the call: not read
    const int live = live64 < (long long)cols ? (int)live64 : cols;
    float ar[4] = {0.0f, 0.0f, 0.0f, 0.0f}, ai[4] = {0.0f, 0.0f, 0.0f, 0.0f};

    for (int r0 = 0; r0 < p.rows; r0 += p.rc) {
      const int rcur = p.rows - r0 < p.rc ? p.rows - r0 : p.rc;
      // ---- stage rows r0 .. r0 + rcur - 1: phases plo .. plo + rcur - 1 of every column, in memory order
      const int plo = D - r0 - rcur;
      const long long nbase = cbase * D + plo;
      const int total = rcur * cols;
      const int qd = kDdcBlock / rcur, qm = kDdcBlock % rcur;
      int ci = tid / rcur, e = tid % rcur;
      __syncthreads();                                           // the previous chunk (or tile) has been read
      for (int idx = tid; idx < total; idx += kDdcBlock) {
        const long long n = nbase + (long long)(ci * D + e);
        float re = 0.0f, im = 0.0f;
        if (n >= p.lo_sample && ci < live) ddc_load<FMT, CPLX>(in, n, re, im);
        const int at = (rcur - 1 - e) * cols + ci;
        lds[at] = re;
        if constexpr (CPLX) lds[p.plane + at] = im;
        ci += qd;
        e += qm;
        if (e >= rcur) {
          e -= rcur;
          ci++;
        }
      }
      __syncthreads();
      // ---- the rows' taps, j ascending, eight at a time
      for (int rr = 0; rr < rcur; rr++) {
        const int r = r0 + rr;
        const int jr = r <= p.rlast ? p.jmax : p.jmax - 1;
        const float *row = lds + rr * cols + (kDdcPerLane * tid + p.jpad - kDdcJBlock);
        const float2 *g = taps + (size_t)r * (size_t)p.jpad;
        int j0 = 0;
        for (; j0 + kDdcJBlock <= jr; j0 += kDdcJBlock) ddc_row_block<true, CPLX>(row - j0, p.plane, g + j0, kDdcJBlock, ar, ai);
        if (j0 < jr) ddc_row_block<false, CPLX>(row - j0, p.plane, g + j0, jr - j0, ar, ai);
      }
    }

    // ---- the rotation exp(-2 pi i phi(n0)), one per output, and the store
#pragma unroll
    for (int k = 0; k < kDdcPerLane; k++) {
      const long long m = m0 + kDdcPerLane * tid + k;
      if (m < p.end_out) {
        const unsigned long long n0 = (unsigned long long)(m + 1) * (unsigned long long)D - 1ull;
        const unsigned long long ph = 0ull - p.W * n0;            // turns * 2^64 of the NEGATED phase
        double sd, cd;                                            // the angle in [-1/2, 1/2) turns, good to 2^-54 of a turn
        sincospi(2.0 * ((double)(long long)ph * 0x1p-64), &sd, &cd);
        const float c = (float)cd, s = (float)sd;
        float2 y;
        y.x = __builtin_fmaf(ar[k], c, -(ai[k] * s));
        y.y = __builtin_fmaf(ar[k], s, ai[k] * c);
        out[m - p.first_out] = y;
      }
    }
  }
}

}  // namespace glfer

using namespace glfer;

template <int FMT, int CPLX>
static hipError_t ddc_launch_fmt(const DdcParams &p, hipStream_t st) {
  if (p.ntiles <= 0 || p.nbatch <= 0) return hipSuccess;
  // a grid-stride loop over the tiles: enough workgroups for every CU at this kernel's occupancy, shared among a batch's streams
  const long long cap = 256LL * 16 / (p.nbatch < 16 ? p.nbatch : 16);   // (at least one workgroup a CU and stream)
  const unsigned grid = (unsigned)((long long)p.ntiles < cap ? (long long)p.ntiles : cap);
  const size_t bytes = (size_t)(CPLX ? 2 : 1) * (size_t)p.plane * sizeof(float);   // what the handle's chunk takes: small tiles, more of them a CU
  hipLaunchKernelGGL((ddc_kernel<FMT, CPLX>), dim3(grid, (unsigned)p.nbatch), dim3(kDdcBlock), bytes, st, p, p.in, p.taps, p.out);
  return hipGetLastError();
}

extern "C" hipError_t glfer_launch_ddc(const DdcParams *p, hipStream_t st) {
  if (p->complex_in) {
    switch (p->fmt) {
      case GLFER_FMT_F32: return ddc_launch_fmt<GLFER_FMT_F32, 1>(*p, st);
      case GLFER_FMT_S16: return ddc_launch_fmt<GLFER_FMT_S16, 1>(*p, st);
      case GLFER_FMT_U8: return ddc_launch_fmt<GLFER_FMT_U8, 1>(*p, st);
    }
  } else {
    switch (p->fmt) {
      case GLFER_FMT_F32: return ddc_launch_fmt<GLFER_FMT_F32, 0>(*p, st);
      case GLFER_FMT_S16: return ddc_launch_fmt<GLFER_FMT_S16, 0>(*p, st);
      case GLFER_FMT_U8: return ddc_launch_fmt<GLFER_FMT_U8, 0>(*p, st);
    }
  }
  return hipErrorInvalidValue;
}

extern "C" hipError_t glfer_ddc_prepare() {
  const int bytes = 2 * kDdcLdsWords * (int)sizeof(float);
  hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(&ddc_kernel<GLFER_FMT_F32, 1>), hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
  if (e == hipSuccess) e = hipFuncSetAttribute(reinterpret_cast<const void *>(&ddc_kernel<GLFER_FMT_S16, 1>), hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
  if (e == hipSuccess) e = hipFuncSetAttribute(reinterpret_cast<const void *>(&ddc_kernel<GLFER_FMT_U8, 1>), hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
  return e;
}
