// cross.cpp -- the cross-spectrum entries of include/glfer_hip.h: the auto-spectra, cross-spectrum and coherence of two interleaved
// real channels in one pass (spectro16cx.hip), per frame over a multitaper plan's tapers (glfer_hip_mtm_cross_*) or averaged over
// L consecutive frames of any plan that has an I/Q table (glfer_hip_welch_cross_*).  The checks follow the complex I/Q entries of
// glfer_hip.cpp in order and wording; the kernel reads the plan's I/Q table and twiddles, so the plan holds nothing new.
#include "plan.h"

#include <algorithm>
#include <cstring>

#include "frame_cuts.h"
#include "spectro_cross_params.h"
#include "spectro_params.h"

using glfer::DeviceGuard;
using glfer::hip_fail;

static_assert(GLFER_FMT_F32 == GLFER_SAMPLES_F32 && GLFER_FMT_S16 == GLFER_SAMPLES_S16 && GLFER_FMT_U8 == GLFER_SAMPLES_U8, "CrossParams::fmt");

static hipError_t launch_cross(const CrossParams &q, int n, hipStream_t st) {
  const auto f = launcher16_cx(glfer_logn(n));
  return f ? f(&q, st) : hipErrorInvalidValue;
}

// rows of a stream of F frames: (F - first - L) / step + 1, none where fewer than L frames follow `first` (or first + L wraps)
static size_t welch_rows_of(size_t F, size_t first, size_t L, size_t step) {
  if (L == 0 || step == 0 || first > F || F - first < L) return 0;
  return (F - first - L) / step + 1;
}

// Both forms' device entry.  segments == 0: a row per frame (nrows frames from `first`); else row r averages the `segments` frames
// from first + r * step.  `ok`: the plan is one the calling entry takes.
static int cross_rows(glfer_hip_plan *p, bool ok, const void *d_xy, size_t nstreams, size_t stream_pitch, size_t nsamples, size_t first,
                      size_t segments, size_t step, size_t nrows, float *d_sxx, float *d_syy, float *d_coh, size_t row_pitch, void *d_sxy,
                      size_t sxy_pitch, void *hip_stream) {
  if (!p || !p->d_iqtaps || !ok) return GLFER_E_ARG;
  const size_t bins = (size_t)p->n / 2 + 1, pitch = row_pitch ? row_pitch : bins, xpitch = sxy_pitch ? sxy_pitch : bins;
  if (pitch < bins || xpitch < bins) return GLFER_E_ARG;
  if (nstreams == 0 || nrows == 0) return GLFER_OK;
  if (!d_xy || (!d_sxx && !d_syy && !d_coh && !d_sxy)) return GLFER_E_ARG;
  const size_t csz = 2 * glfer_sample_size(p->cfg.sample_format);       // bytes of a pair
  if (reinterpret_cast<uintptr_t>(d_xy) & (csz - 1)) return GLFER_E_ARG;
  const size_t F = nsamples / (size_t)p->hop;
  if (segments == 0) {
    if (first + nrows < first || (first + nrows) > F) return GLFER_E_ARG;   // wraps, or a frame past the stream
  } else if (nrows > welch_rows_of(F, first, segments, step)) {             // the same of a row's last frame
    return GLFER_E_ARG;
  }
  if (nrows > 0x7fffffffu) return GLFER_E_ARG;
  if (nsamples > SIZE_MAX / csz || stream_pitch > (SIZE_MAX / csz) / nstreams) return GLFER_E_ARG;
  if (xpitch > SIZE_MAX / 2) return GLFER_E_ARG;
  const size_t wide = std::max(pitch, 2 * xpitch);                      // floats of the widest row
  if (wide > SIZE_MAX / sizeof(float) / nrows || nrows * wide > (SIZE_MAX / sizeof(float)) / nstreams) return GLFER_E_ARG;
  hipStream_t st = (hipStream_t)hip_stream;
  DeviceGuard guard(p->cfg.device);
  HIP_TRY(guard.error());
  size_t ymax = 1;
  if (nstreams > 1) {
    int dev = 0, y = 0;
    HIP_TRY(hipGetDevice(&dev));
    HIP_TRY(hipDeviceGetAttribute(&y, hipDeviceAttributeMaxGridDimY, dev));
    ymax = (size_t)std::max(1, std::min(y, 65535));
  }
  CrossParams q;
  memset(&q, 0, sizeof q);
  q.frame0 = (long long)first;
  q.nframes = (int)nrows;
  q.H = p->hop;
  q.R = p->keep;
  q.ntap = p->ntapers;
  q.history_mode = p->cfg.history_mode ? 1 : 0;
  q.fmt = p->cfg.sample_format;
  q.taps = p->d_iqtaps.get();
  q.tw = p->d_tw.as<float2>();
  q.row_pitch = (long long)pitch;
  q.sxy_pitch = (long long)xpitch;
  q.batch_stride = (long long)(stream_pitch * csz);
  q.row_batch_stride = (long long)(nrows * pitch);
  q.sxy_batch_stride = (long long)(nrows * xpitch);
  if (segments != 0) {
    q.segments = (int)segments;
    q.step = (long long)step;
    q.scale = (float)(0.25 / (double)segments);           // rounded once; one segment: the per-frame form's 1/4
  }
  for (size_t c0 = 0; c0 < nstreams; c0 += ymax) {      // batches above the grid's y limit: chunks of it
    const size_t nb = std::min(nstreams - c0, ymax);
    q.stream = static_cast<const char *>(d_xy) + c0 * stream_pitch * csz;
    q.sxx = d_sxx ? d_sxx + c0 * nrows * pitch : nullptr;
    q.syy = d_syy ? d_syy + c0 * nrows * pitch : nullptr;
    q.coh = d_coh ? d_coh + c0 * nrows * pitch : nullptr;
    q.sxy = d_sxy ? static_cast<float2 *>(d_sxy) + c0 * nrows * xpitch : nullptr;
    q.nbatch = (int)nb;
    const hipError_t e = launch_cross(q, p->n, st);
    if (e != hipSuccess) return hip_fail(e, "estimator launch (cross)");
  }
  return GLFER_OK;
}

extern "C" {

int glfer_hip_cross_supported(const glfer_hip_config *cfg) {
  if (!cfg) return GLFER_E_ARG;
  if (cfg->mode != GLFER_MODE_MTM || cfg->mtm_k < 1) return GLFER_E_ARG;      // one window: coherence is identically 1
  if (cfg->n < 256 || cfg->n > 8192 || (cfg->n & (cfg->n - 1))) return GLFER_E_ARG;
  return glfer_hip_iq_supported(cfg);                                          // mean removal, limiter, RA9MB, the sample format
}

int glfer_hip_mtm_cross_batch_device(glfer_hip_plan *p, const void *d_xy, size_t nstreams, size_t stream_pitch, size_t nsamples,
                                     size_t first, size_t nframes, float *d_sxx, float *d_syy, float *d_coh, size_t row_pitch,
                                     void *d_sxy, size_t sxy_pitch, void *hip_stream) {
  return cross_rows(p, p && glfer_hip_cross_supported(&p->cfg) == GLFER_OK, d_xy, nstreams, stream_pitch, nsamples, first, 0, 1, nframes,
                    d_sxx, d_syy, d_coh, row_pitch, d_sxy, sxy_pitch, hip_stream);
}

int glfer_hip_mtm_cross_device(glfer_hip_plan *p, const void *d_xy, size_t nsamples, size_t first, size_t nframes, float *d_sxx,
                               float *d_syy, float *d_coh, size_t row_pitch, void *d_sxy, size_t sxy_pitch, void *hip_stream) {
  return glfer_hip_mtm_cross_batch_device(p, d_xy, 1, 0, nsamples, first, nframes, d_sxx, d_syy, d_coh, row_pitch, d_sxy, sxy_pitch,
                                          hip_stream);
}

int glfer_hip_welch_cross_supported(const glfer_hip_config *cfg, size_t segments, size_t step) {
  if (!cfg) return GLFER_E_ARG;
  if (cfg->n < 256 || cfg->n > 8192 || (cfg->n & (cfg->n - 1))) return GLFER_E_ARG;
  if (glfer_hip_iq_supported(cfg) != GLFER_OK) return GLFER_E_ARG;             // FFT or MTM; mean removal, limiter, RA9MB, the sample format
  if (cfg->mode == GLFER_MODE_MTM ? (cfg->mtm_k < 0 || cfg->mtm_k > 31) : (cfg->window_type < 0 || cfg->window_type > 7)) return GLFER_E_ARG;
  if (!(cfg->overlap >= 0.0f) || !(cfg->overlap < 1.0f)) return GLFER_E_ARG;
  const size_t tapers = cfg->mode == GLFER_MODE_MTM ? (size_t)cfg->mtm_k + 1 : 1;
  if (segments < 1 || segments > 4096 || step < 1) return GLFER_E_ARG;
  if (segments * tapers < 2) return GLFER_E_ARG;                               // one window, one segment: coherence is identically 1
  // the rows one block handles read through one buffer descriptor: (FPB - 1) step H + N pairs within 2^31 - 1 bytes
  const size_t n = (size_t)cfg->n, fpb = n < 4096 ? 4096 / n : 1, hop = (size_t)(int)(cfg->n * (1.0 - cfg->overlap));
  if (hop < 1) return GLFER_E_ARG;
  const size_t pairs = (size_t)0x7fffffff / (2 * glfer_sample_size(cfg->sample_format));
  if (fpb > 1 && step > (pairs - n) / ((fpb - 1) * hop)) return GLFER_E_ARG;
  return GLFER_OK;
}

size_t glfer_hip_welch_rows(glfer_hip_plan *p, size_t nsamples, size_t first, size_t segments, size_t step) {
  return p ? welch_rows_of(nsamples / (size_t)p->hop, first, segments, step) : 0;
}

int glfer_hip_welch_cross_batch_device(glfer_hip_plan *p, const void *d_xy, size_t nstreams, size_t stream_pitch, size_t nsamples,
                                       size_t first, size_t segments, size_t step, size_t nrows, float *d_sxx, float *d_syy,
                                       float *d_coh, size_t row_pitch, void *d_sxy, size_t sxy_pitch, void *hip_stream) {
  return cross_rows(p, p && glfer_hip_welch_cross_supported(&p->cfg, segments, step) == GLFER_OK, d_xy, nstreams, stream_pitch, nsamples,
                    first, segments, step, nrows, d_sxx, d_syy, d_coh, row_pitch, d_sxy, sxy_pitch, hip_stream);
}

int glfer_hip_welch_cross_device(glfer_hip_plan *p, const void *d_xy, size_t nsamples, size_t first, size_t segments, size_t step,
                                 size_t nrows, float *d_sxx, float *d_syy, float *d_coh, size_t row_pitch, void *d_sxy,
                                 size_t sxy_pitch, void *hip_stream) {
  return glfer_hip_welch_cross_batch_device(p, d_xy, 1, 0, nsamples, first, segments, step, nrows, d_sxx, d_syy, d_coh, row_pitch, d_sxy,
                                            sxy_pitch, hip_stream);
}

}  // extern "C"
