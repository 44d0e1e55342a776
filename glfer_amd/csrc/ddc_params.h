// ddc_params.h -- the argument block of ddc.hip (the frequency-translating, decimating FIR) and the layout rules its host side
// (glfer_hip.cpp) and the kernel share.  Nothing else reads it.
//
// Output m of a stream, n0 = (m + 1) D - 1:   y[m] = exp(-2 pi i phi(n0)) sum_t g[t] x[n0 - t],   phi(n) = (W n mod 2^64) / 2^64.
// With t = j D + r (0 <= r < D) the sample of tap t is x[(m - j) D + (D - 1 - r)]: the stream laid out by phase, sample n at row
// n mod D and column n div D, has it in row D - 1 - r at column m - j, so lanes with consecutive m read consecutive words and the
// tap is the same for every lane.  The sum runs r = 0 .. min(D, T) - 1 outermost and j = 0, 1, ... inside a row: an order that t
// alone fixes (for the handle's D), whatever tile, launch or batch the output belongs to.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "spectro_params.h"                          // GLFER_FMT_*

constexpr int kDdcBlock = 256;                      // lanes of a workgroup
constexpr int kDdcPerLane = 4;                      // consecutive outputs a lane owns
constexpr int kDdcTile = kDdcBlock * kDdcPerLane;   // outputs of a tile
constexpr int kDdcJBlock = 8;                       // taps j0 .. j0 + 7 of a row share one window of 8 + 3 (read as 12) words
constexpr int kDdcLdsWords = 9216;                  // words of a plane of the staged tile: kDdcTile + 8192 columns of one row fit

// columns of a staged row: the tile's outputs and the kDdcJBlock-padded reach of the taps to their left
static inline int ddc_jmax(int decim, int ntaps) { return (ntaps - 1) / decim + 1; }
static inline int ddc_jpad(int decim, int ntaps) { return (ddc_jmax(decim, ntaps) + kDdcJBlock - 1) / kDdcJBlock * kDdcJBlock; }
static inline int ddc_cols(int decim, int ntaps) { return kDdcTile + ddc_jpad(decim, ntaps); }
// rows staged at a time (at least one: ddc_cols <= kDdcLdsWords for every D >= 1, T <= 8192)
static inline int ddc_rows_per_chunk(int decim, int ntaps) {
  const int rows = decim < ntaps ? decim : ntaps, fit = kDdcLdsWords / ddc_cols(decim, ntaps);
  return fit < rows ? fit : rows;
}

struct DdcParams {
  const void *in;              // sample 0 of stream 0 (virtual base)
  float2 *out;                 // output first_out of stream 0
  const float2 *taps;          // [min(D, T)][jpad]: g[j D + r] at [r][j], zeros where j D + r >= T (never multiplied)
  unsigned long long W;        // the phase word
  long long first_out;         // global index of the first output of the call
  long long end_out;           // first_out + nout
  long long lo_sample;         // max(0, first_out D - (T - 1)): nothing below it is read
  long long in_stride;         // bytes from one stream to the next
  long long out_stride;        // complex samples from one stream's outputs to the next's
  int D, T;
  int jmax, jpad, cols;        // ddc_jmax, ddc_jpad, ddc_cols
  int rows, rc;                // min(D, T); rows staged at a time
  int plane;                   // rc * cols: words of a staged plane (complex input: the imaginary plane follows the real one)
  int rlast;                   // (T - 1) mod D: rows r <= rlast have jmax taps, the others jmax - 1
  int ntiles;                  // ceil(nout / kDdcTile)
  int nbatch;
  int fmt, complex_in;
};

extern "C" hipError_t glfer_launch_ddc(const DdcParams *p, hipStream_t st);
// once per device, before the first launch (a complex tile takes more than the 64 KiB a kernel may use unasked)
extern "C" hipError_t glfer_ddc_prepare();
