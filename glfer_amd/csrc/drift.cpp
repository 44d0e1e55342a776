// drift.cpp -- the drift-search entries of include/glfer_hip.h: sums of rows along straight lines of frequency drift (drift.hip)
// over rows the caller holds, over many streams' rows, and over a plan's rows computed into scratch piece by piece.  The checks
// follow the LMP statistic's entries of glfer_hip.cpp in order; the integer arithmetic is drift_cuts.h's.  The spectrogram-level
// entry calls the public rows entry, so nothing of the estimators' host side is touched.
#include "plan.h"

#include <algorithm>
#include <climits>
#include <cstring>

#include "drift_cuts.h"
#include "drift_params.h"

using glfer::DeviceGuard;
using glfer::hip_fail;

static_assert(GLFER_DRIFT_ROW_ALIGN == GLFER_FRAME_ALIGN, "drift_cuts.h restates the frame grid");
static_assert(GLFER_DRIFT_MAX_DRIFTS - 1 == kDriftHaloMax, "the widest halo: 255 drifts that include 0");

size_t glfer_hip_drift_blocks(size_t nrows, size_t frames, size_t step) {
  if (frames < 2 || frames > GLFER_DRIFT_MAX_FRAMES) return 0;
  return glfer_drift_blocks(nrows, frames, step);
}

int glfer_hip_drift_offsets(size_t frames, int dmin, int dmax, int *offsets) {
  if (!glfer_drift_args_ok(frames, 1, dmin, dmax)) return GLFER_E_ARG;
  if (offsets)
    for (int d = dmin; d <= dmax; d++)
      for (size_t t = 0; t < frames; t++) offsets[(size_t)(d - dmin) * frames + t] = glfer_drift_offset((int)frames, d, (int)t);
  return GLFER_OK;
}

// frames, step, the drift range and the row shape: what every device entry refuses first
static bool drift_shape_ok(int bins, size_t pitch, size_t frames, size_t step, int dmin, int dmax) {
  // (bins: the kernel's tile and halo indices, bins + 255 and k0 - halo + 767 at most, stay inside an int)
  return glfer_drift_args_ok(frames, step, dmin, dmax) && bins >= 1 && bins <= INT_MAX - 1024 && pitch >= (size_t)bins &&
         pitch <= (size_t)LLONG_MAX / sizeof(float);
}

// Checked arguments: nblocks blocks of each of nstreams streams, in launches of at most 65 535 blocks by 65 535 streams (the
// grid's y and z limits).  No allocation, no upload, no synchronisation: legal on a stream that is being captured.
static hipError_t drift_launches(const float *d_rows, size_t nstreams, size_t row_stride, int bins, size_t pitch, size_t frames, size_t step,
                                 size_t nblocks, int dmin, int dmax, float *d_sums, size_t sums_stride, float *d_best, size_t best_stride,
                                 short *d_drift, size_t drift_stride, hipStream_t st) {
  DriftParams q;
  memset(&q, 0, sizeof q);
  q.pitch = (long long)pitch;
  q.step = (long long)step;
  q.row_stride = (long long)row_stride;
  q.sums_stride = (long long)sums_stride;
  q.best_stride = (long long)best_stride;
  q.drift_stride = (long long)drift_stride;
  q.bins = bins;
  q.frames = (int)frames;
  q.dmin = dmin;
  q.dmax = dmax;
  q.halo = std::max(-dmin, dmax);
  const size_t chunk = 65535;
  for (size_t s0 = 0; s0 < nstreams; s0 += chunk) {
    q.nstreams_here = (unsigned)std::min(nstreams - s0, chunk);
    q.rows = d_rows + s0 * row_stride;
    q.sums = d_sums ? d_sums + s0 * sums_stride : nullptr;
    q.best = d_best ? d_best + s0 * best_stride : nullptr;
    q.drift = d_drift ? d_drift + s0 * drift_stride : nullptr;
    for (size_t b0 = 0; b0 < nblocks; b0 += chunk) {
      q.block0 = (long long)b0;
      q.nblocks_here = (unsigned)std::min(nblocks - b0, chunk);
      const hipError_t e = glfer_launch_drift(&q, st);
      if (e != hipSuccess) return e;
    }
  }
  return hipSuccess;
}

// nblocks * D * bins floats (the largest output) within size_t; nblocks >= 1
static bool drift_outputs_fit(size_t nblocks, int D, int bins) {
  const size_t per_block = (size_t)D * (size_t)bins;     // <= 255 * INT_MAX
  return nblocks <= SIZE_MAX / sizeof(float) / per_block;
}

int glfer_hip_drift_batch_device(const float *d_rows, size_t nstreams, size_t row_stride, size_t nrows, int bins, size_t pitch, size_t frames,
                                 size_t step, size_t nblocks, int dmin, int dmax, float *d_sums, size_t sums_stride, float *d_best,
                                 size_t best_stride, short *d_drift, size_t drift_stride, void *hip_stream) {
  if (!drift_shape_ok(bins, pitch, frames, step, dmin, dmax)) return GLFER_E_ARG;
  if (nblocks == 0 || nstreams == 0) return GLFER_OK;
  if (!d_rows || (!d_sums && !d_best && !d_drift)) return GLFER_E_ARG;
  if (nblocks > glfer_hip_drift_blocks(nrows, frames, step)) return GLFER_E_ARG;
  const int D = dmax - dmin + 1;
  if (nrows > SIZE_MAX / sizeof(float) / pitch || !drift_outputs_fit(nblocks, D, bins)) return GLFER_E_ARG;
  // a stream's rows end with the last row's bins; its outputs are dense
  const size_t held = (nrows - 1) * pitch + (size_t)bins, nbest = nblocks * (size_t)bins, nsums = nbest * (size_t)D;
  if (nstreams > 1) {
    if (row_stride < held || (d_sums && sums_stride < nsums) || (d_best && best_stride < nbest) || (d_drift && drift_stride < nbest))
      return GLFER_E_ARG;
    const size_t top = SIZE_MAX / sizeof(float) / nstreams;
    if (row_stride > top || (d_sums && sums_stride > top) || (d_best && best_stride > top) || (d_drift && drift_stride > top)) return GLFER_E_ARG;
  }
  DeviceGuard guard(glfer::data_device(d_rows));
  HIP_TRY(guard.error());
  HIP_TRY(drift_launches(d_rows, nstreams, row_stride, bins, pitch, frames, step, nblocks, dmin, dmax, d_sums, sums_stride, d_best, best_stride,
                         d_drift, drift_stride, (hipStream_t)hip_stream));
  return GLFER_OK;
}

int glfer_hip_drift_device(const float *d_rows, size_t nrows, int bins, size_t pitch, size_t frames, size_t step, size_t nblocks, int dmin,
                           int dmax, float *d_sums, float *d_best, short *d_drift, void *hip_stream) {
  return glfer_hip_drift_batch_device(d_rows, 1, 0, nrows, bins, pitch, frames, step, nblocks, dmin, dmax, d_sums, 0, d_best, 0, d_drift, 0,
                                      hip_stream);
}

int glfer_hip_spectrogram_drift_device(glfer_hip_plan *p, const void *d_stream, size_t nsamples, size_t first, size_t frames, size_t step,
                                       size_t nblocks, int dmin, int dmax, float *d_sums, float *d_best, short *d_drift, void *hip_stream) {
  if (!p) return GLFER_E_ARG;
  const int bins = p->bins;
  const size_t pitch = (size_t)p->pitch;
  if (!drift_shape_ok(bins, pitch, frames, step, dmin, dmax)) return GLFER_E_ARG;
  if (nblocks == 0) return GLFER_OK;
  if (!d_stream || (!d_sums && !d_best && !d_drift)) return GLFER_E_ARG;
  // the call's frames [first, end) lie inside the stream
  const size_t F = glfer_hip_num_frames(p, nsamples), span = glfer_drift_span(nblocks, frames, step);
  if (first > F || span > F - first) return GLFER_E_ARG;
  const int D = dmax - dmin + 1;
  if (!drift_outputs_fit(nblocks, D, bins)) return GLFER_E_ARG;
  hipStream_t st = (hipStream_t)hip_stream;
  if (glfer::stream_is_capturing(st)) return GLFER_E_ARG;     // scratch is taken per piece
  const size_t end = first + span, row_bytes = pitch * sizeof(float);
  DeviceGuard guard(p->cfg.device);
  HIP_TRY(guard.error());
  glfer::Scratch<float> rows(st);
  for (size_t b0 = 0; b0 < nblocks;) {
    const size_t nb = glfer_drift_piece_blocks(nblocks - b0, frames, step, row_bytes, glfer::scratch_cap() / 2);
    const size_t a = first + b0 * step, e = a + glfer_drift_span(nb, frames, step);
    const size_t lo = glfer_drift_piece_lo(a, first), hi = glfer_drift_piece_hi(e, end);
    HIP_TRY(rows.take((hi - lo) * pitch));
    if (const int rc = glfer_hip_spectrogram_device(p, d_stream, nsamples, lo, hi - lo, rows.get(), st); rc != GLFER_OK) return rc;
    HIP_TRY(drift_launches(rows.get() + (a - lo) * pitch, 1, 0, bins, pitch, frames, step, nb, dmin, dmax,
                           d_sums ? d_sums + b0 * (size_t)D * (size_t)bins : nullptr, 0, d_best ? d_best + b0 * (size_t)bins : nullptr, 0,
                           d_drift ? d_drift + b0 * (size_t)bins : nullptr, 0, st));
    b0 += nb;
  }
  return GLFER_OK;
}
