// cross.cpp -- the cross-spectrum entries of include/glfer_hip.h: the multitaper auto-spectra, cross-spectrum and coherence of two
// interleaved real channels in one pass (spectro16cx.hip).  The checks follow the complex I/Q entries of glfer_hip.cpp in order
// and wording; the kernel reads the plan's I/Q table and twiddles, so the plan holds nothing new.
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
  if (!p || !p->d_iqtaps || glfer_hip_cross_supported(&p->cfg) != GLFER_OK) return GLFER_E_ARG;
  const size_t bins = (size_t)p->n / 2 + 1, pitch = row_pitch ? row_pitch : bins, xpitch = sxy_pitch ? sxy_pitch : bins;
  if (pitch < bins || xpitch < bins) return GLFER_E_ARG;
  if (nstreams == 0 || nframes == 0) return GLFER_OK;
  if (!d_xy || (!d_sxx && !d_syy && !d_coh && !d_sxy)) return GLFER_E_ARG;
  const size_t csz = 2 * glfer_sample_size(p->cfg.sample_format);       // bytes of a pair
  if (reinterpret_cast<uintptr_t>(d_xy) & (csz - 1)) return GLFER_E_ARG;
  if (first + nframes < first || (first + nframes) > nsamples / (size_t)p->hop) return GLFER_E_ARG;   // wraps, or a frame past the stream
  if (nframes > 0x7fffffffu) return GLFER_E_ARG;
  if (nsamples > SIZE_MAX / csz || stream_pitch > (SIZE_MAX / csz) / nstreams) return GLFER_E_ARG;
  if (xpitch > SIZE_MAX / 2) return GLFER_E_ARG;
  const size_t wide = std::max(pitch, 2 * xpitch);                      // floats of the widest row
  if (wide > SIZE_MAX / sizeof(float) / nframes || nframes * wide > (SIZE_MAX / sizeof(float)) / nstreams) return GLFER_E_ARG;
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
  q.nframes = (int)nframes;
  q.H = p->hop;
  q.R = p->keep;
  q.ntap = p->ntapers;
  q.history_mode = p->cfg.history_mode ? 1 : 0;
  q.fmt = p->cfg.sample_format;
  q.taps = p->d_iqtaps;
  q.tw = p->d_tw;
  q.row_pitch = (long long)pitch;
  q.sxy_pitch = (long long)xpitch;
  q.batch_stride = (long long)(stream_pitch * csz);
  q.row_batch_stride = (long long)(nframes * pitch);
  q.sxy_batch_stride = (long long)(nframes * xpitch);
  for (size_t c0 = 0; c0 < nstreams; c0 += ymax) {      // batches above the grid's y limit: chunks of it
    const size_t nb = std::min(nstreams - c0, ymax);
    q.stream = static_cast<const char *>(d_xy) + c0 * stream_pitch * csz;
    q.sxx = d_sxx ? d_sxx + c0 * nframes * pitch : nullptr;
    q.syy = d_syy ? d_syy + c0 * nframes * pitch : nullptr;
    q.coh = d_coh ? d_coh + c0 * nframes * pitch : nullptr;
    q.sxy = d_sxy ? static_cast<float2 *>(d_sxy) + c0 * nframes * xpitch : nullptr;
    q.nbatch = (int)nb;
    const hipError_t e = launch_cross(q, p->n, st);
    if (e != hipSuccess) return hip_fail(e, "estimator launch (cross)");
  }
  return GLFER_OK;
}

int glfer_hip_mtm_cross_device(glfer_hip_plan *p, const void *d_xy, size_t nsamples, size_t first, size_t nframes, float *d_sxx,
                               float *d_syy, float *d_coh, size_t row_pitch, void *d_sxy, size_t sxy_pitch, void *hip_stream) {
  return glfer_hip_mtm_cross_batch_device(p, d_xy, 1, 0, nsamples, first, nframes, d_sxx, d_syy, d_coh, row_pitch, d_sxy, sxy_pitch,
                                          hip_stream);
}

}  // extern "C"
