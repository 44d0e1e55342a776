// drift_params.h -- the argument block of drift.hip (sums of rows along straight lines of frequency drift) and the constants its
// host side (drift.cpp) and the kernel share.  Nothing else reads it.
//
// Block b of a stream is rows b step .. b step + T - 1.  sums[b][d - dmin][k] = sum over t = 0 .. T - 1, in that order, in float
// from +0.0f, of row (b step + t) at bin k + o(d, t), o(d, t) = sgn(d) ((2 |d| t + (T - 1)) div (2 (T - 1))) (drift_cuts.h); a
// bin outside [0, bins) adds +0.0f.  best / drift: the largest of the D sums at k and its d, by a scan 0, +1, -1, +2, ... that
// replaces on strict >.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

constexpr int kDriftBlock = 256;                     // lanes of a workgroup, and the bins of its tile (a bin a lane)
constexpr int kDriftHaloMax = 254;                   // max(|dmin|, dmax) with 255 drifts that include 0
constexpr int kDriftTileWords = kDriftBlock + 2 * 256;   // words of a staged row tile (two of them in LDS)
constexpr int kDriftMaxGroup = 64;                   // the largest group capacity: drifts a lane accumulates in one pass (a wavefront's lanes hold their offsets)

struct DriftParams {
  const float *rows;           // row 0 of stream 0
  float *sums;                 // [nblocks][D][bins] of stream 0, or null
  float *best;                 // [nblocks][bins], or null
  short *drift;                // [nblocks][bins], or null
  long long pitch;             // floats from one row to the next
  long long step;              // rows from one block to the next
  long long row_stride;        // floats from one stream's rows to the next's
  long long sums_stride, best_stride, drift_stride;   // elements from one stream's output to the next's
  long long block0;            // the block of blockIdx.y == 0 (launches beyond the grid's y limit)
  int bins;
  int frames;                  // T
  int dmin, dmax;
  int halo;                    // max(-dmin, dmax)
  unsigned nblocks_here;       // grid y
  unsigned nstreams_here;      // grid z (rows, sums ... already point at the launch's first stream)
};

// picks the instantiation by the drift count: group capacity 8, 32 or 64 (more than 64 drifts: further passes of the same lanes)
extern "C" hipError_t glfer_launch_drift(const DriftParams *p, hipStream_t st);
// the group capacity glfer_launch_drift takes for D drifts
static inline int drift_group(int D) { return D <= 8 ? 8 : D <= 32 ? 32 : kDriftMaxGroup; }
