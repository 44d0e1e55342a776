// adaptive.cpp -- the adaptive-weight entries of include/glfer_hip.h: Thomson's adaptively weighted multitaper rows of one real
// channel and their degrees of freedom in one pass (spectro16a.hip).  The checks follow cross.cpp's cross_rows in order and
// wording; the kernel reads the plan's unscaled taper table (made with the plan) and twiddles, and the weights ride in its
// argument block.  The jackknife entries (the JK instantiations of the same kernel: a third row, the jackknife variance of
// ln psd) share adaptive_rows' checks; glfer_hip_jackknife_factor is host arithmetic, Student's quantile in closed form.
#include "plan.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "frame_cuts.h"
#include "host_tables.h"
#include "plan_tables.h"
#include "spectro_adaptive_params.h"
#include "spectro_params.h"

using glfer::DeviceGuard;
using glfer::hip_fail;

static_assert(GLFER_FMT_F32 == GLFER_SAMPLES_F32 && GLFER_FMT_S16 == GLFER_SAMPLES_S16 && GLFER_FMT_U8 == GLFER_SAMPLES_U8, "AdaptiveParams::fmt");

// The floats the kernel gets from a plan's sig_j (lambda_j = 1 + sig_j, g-l_dpss.c:343): beta_j = max(-sig_j, 0) formed in double
// and rounded, lambda_j = 1 - beta_j formed in double from the unrounded beta_j and rounded.  false: the lambda are not
// non-increasing in j (u_j <= 1 rests on that), or not in (0, 1].
static bool adaptive_weights_of(const double *sig, int k, float *lam, float *beta) {
  double prev = 1.0;
  for (int j = 0; j < k; j++) {
    const double b = std::max(-sig[j], 0.0), l = 1.0 - b;
    if (!(l > 0.0) || !(l <= prev)) return false;
    prev = l;
    if (lam) lam[j] = (float)l;
    if (beta) beta[j] = (float)b;
  }
  return true;
}

// jk: the jackknife entries -- their own launchers, the third row d_logvar, and iters = 0 allowed (w_j = lambda_j)
static int adaptive_rows(glfer_hip_plan *p, const void *d_stream, size_t nstreams, size_t stream_pitch, size_t nsamples, size_t first,
                         size_t nframes, float *d_psd, float *d_dof, size_t row_pitch, int iters, void *hip_stream, bool jk = false,
                         float *d_logvar = nullptr) {
  if (!p || !p->d_ataps || (jk ? glfer_hip_jackknife_supported(&p->cfg) : glfer_hip_adaptive_supported(&p->cfg)) != GLFER_OK)
    return GLFER_E_ARG;
  const size_t bins = (size_t)p->n / 2 + 1, pitch = row_pitch ? row_pitch : bins;
  if (pitch < bins) return GLFER_E_ARG;
  if (iters < (jk ? 0 : 1) || iters > GLFER_ADAPTIVE_ITERS_MAX) return GLFER_E_ARG;
  AdaptiveParams q;
  memset(&q, 0, sizeof q);
  if (!adaptive_weights_of(p->sig.data(), p->ntapers, q.lam, q.beta)) return GLFER_E_ARG;
  if (nstreams == 0 || nframes == 0) return GLFER_OK;
  if (!d_stream || (!d_psd && !d_dof && !d_logvar)) return GLFER_E_ARG;
  const size_t csz = glfer_sample_size(p->cfg.sample_format);
  if (reinterpret_cast<uintptr_t>(d_stream) & (csz - 1)) return GLFER_E_ARG;
  const size_t F = nsamples / (size_t)p->hop;
  if (first + nframes < first || (first + nframes) > F) return GLFER_E_ARG;   // wraps, or a frame past the stream
  if (nframes > 0x7fffffffu) return GLFER_E_ARG;
  if (nsamples > SIZE_MAX / csz || stream_pitch > (SIZE_MAX / csz) / nstreams) return GLFER_E_ARG;
  if (pitch > SIZE_MAX / sizeof(float) / nframes || nframes * pitch > (SIZE_MAX / sizeof(float)) / nstreams) return GLFER_E_ARG;
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
  q.frame0 = (long long)first;
  q.nframes = (int)nframes;
  q.H = p->hop;
  q.R = p->keep;
  q.ntap = p->ntapers;
  q.history_mode = p->cfg.history_mode ? 1 : 0;
  q.fmt = p->cfg.sample_format;
  q.iters = iters;
  q.inv_n = 1.0f / (float)p->n;
  q.taps = p->d_ataps.get();
  q.tw = p->d_tw.as<float2>();
  q.row_pitch = (long long)pitch;
  q.batch_stride = (long long)(stream_pitch * csz);
  q.row_batch_stride = (long long)(nframes * pitch);
  const auto launcher = jk ? launcher16_jackknife(glfer_logn(p->n)) : launcher16_adaptive(glfer_logn(p->n));
  for (size_t c0 = 0; c0 < nstreams; c0 += ymax) {      // batches above the grid's y limit: chunks of it
    const size_t nb = std::min(nstreams - c0, ymax);
    q.stream = static_cast<const char *>(d_stream) + c0 * stream_pitch * csz;
    q.psd = d_psd ? d_psd + c0 * nframes * pitch : nullptr;
    q.dof = d_dof ? d_dof + c0 * nframes * pitch : nullptr;
    q.logvar = d_logvar ? d_logvar + c0 * nframes * pitch : nullptr;
    q.nbatch = (int)nb;
    const hipError_t e = launcher ? launcher(&q, st) : hipErrorInvalidValue;
    if (e != hipSuccess) return hip_fail(e, jk ? "estimator launch (jackknife)" : "estimator launch (adaptive)");
  }
  return GLFER_OK;
}

// Student's t distribution function for an integer number nu >= 1 of degrees of freedom, in closed form (Abramowitz & Stegun
// 26.7.3 / 26.7.4): with theta = atan(t / sqrt(nu)), c = cos^2 theta,
//   nu odd:   1/2 + (theta + sin theta cos theta (1 + 2/3 c + 2.4/(3.5) c^2 + ... up to c^((nu-3)/2))) / pi     (nu = 1: theta / pi)
//   nu even:  1/2 + sin theta (1 + 1/2 c + 1.3/(2.4) c^2 + ... up to c^((nu-2)/2)) / 2
static double student_cdf(double t, int nu) {
  const double pi = 3.14159265358979323846;
  const double r = t / std::sqrt((double)nu), c = 1.0 / (1.0 + r * r), sn = r / std::sqrt(1.0 + r * r);   // cos^2, sin of theta
  double sum = 1.0, term = 1.0;
  if (nu & 1) {
    for (int m = 1; 2 * m + 1 <= nu - 2; m++) sum += (term *= c * (2.0 * m) / (2.0 * m + 1.0));
    return 0.5 + (std::atan(r) + (nu > 1 ? sn * std::sqrt(c) * sum : 0.0)) / pi;
  }
  for (int m = 1; 2 * m <= nu - 2; m++) sum += (term *= c * (2.0 * m - 1.0) / (2.0 * m));
  return 0.5 + 0.5 * sn * sum;
}

extern "C" {

int glfer_hip_adaptive_supported(const glfer_hip_config *cfg) { return glfer::adaptive_config_ok(cfg); }   // (plan_tables.cpp: the plan asks the same)

int glfer_hip_adaptive_weights(const glfer_hip_config *cfg, float *lambda_out, float *beta_out) {
  if (glfer_hip_adaptive_supported(cfg) != GLFER_OK || !(cfg->mtm_w > 0.0f)) return GLFER_E_ARG;
  const int nt = cfg->mtm_k + 1;
  std::vector<double> tapers((size_t)nt * cfg->n), sig(nt);
  if (!glfer::make_dpss(cfg->n, cfg->mtm_k, (double)cfg->mtm_w, tapers.data(), sig.data())) return GLFER_E_NUMERIC;
  return adaptive_weights_of(sig.data(), nt, lambda_out, beta_out) ? nt : GLFER_E_ARG;
}

int glfer_hip_jackknife_supported(const glfer_hip_config *cfg) {
  if (glfer_hip_adaptive_supported(cfg) != GLFER_OK) return GLFER_E_ARG;
  return launcher16_jackknife(glfer_logn(cfg->n)) ? GLFER_OK : GLFER_E_ARG;      // a size whose JK instantiations are not built
}

int glfer_hip_jackknife_factor(const glfer_hip_config *cfg, double level, double *t_out) {
  if (!t_out || glfer_hip_jackknife_supported(cfg) != GLFER_OK || !(level > 0.0) || !(level < 1.0)) return GLFER_E_ARG;
  const int nu = cfg->mtm_k;                                                    // K - 1 = 1 .. 7
  const double q = 0.5 + 0.5 * level;
  if (!(q < 1.0)) return GLFER_E_ARG;                                            // (a level that rounds to 1)
  // bisection: the distribution function rises from 1/2 at 0; the bracket's upper end doubles until it passes q
  double lo = 0.0, hi = 1.0;
  while (student_cdf(hi, nu) < q && hi < 1e300) lo = hi, hi *= 2.0;
  for (int it = 0; it < 200 && lo < hi; it++) {
    const double mid = 0.5 * (lo + hi);
    if (mid <= lo || mid >= hi) break;
    (student_cdf(mid, nu) < q ? lo : hi) = mid;
  }
  *t_out = 0.5 * (lo + hi);
  return GLFER_OK;
}

int glfer_hip_mtm_jackknife_batch_device(glfer_hip_plan *p, const void *d_stream, size_t nstreams, size_t stream_pitch, size_t nsamples,
                                         size_t first, size_t nframes, float *d_psd, float *d_dof, float *d_logvar, size_t row_pitch,
                                         int iters, void *hip_stream) {
  return adaptive_rows(p, d_stream, nstreams, stream_pitch, nsamples, first, nframes, d_psd, d_dof, row_pitch, iters, hip_stream, true,
                       d_logvar);
}

int glfer_hip_mtm_jackknife_device(glfer_hip_plan *p, const void *d_stream, size_t nsamples, size_t first, size_t nframes, float *d_psd,
                                   float *d_dof, float *d_logvar, size_t row_pitch, int iters, void *hip_stream) {
  return adaptive_rows(p, d_stream, 1, 0, nsamples, first, nframes, d_psd, d_dof, row_pitch, iters, hip_stream, true, d_logvar);
}

int glfer_hip_mtm_adaptive_batch_device(glfer_hip_plan *p, const void *d_stream, size_t nstreams, size_t stream_pitch, size_t nsamples,
                                        size_t first, size_t nframes, float *d_psd, float *d_dof, size_t row_pitch, int iters,
                                        void *hip_stream) {
  return adaptive_rows(p, d_stream, nstreams, stream_pitch, nsamples, first, nframes, d_psd, d_dof, row_pitch, iters, hip_stream);
}

int glfer_hip_mtm_adaptive_device(glfer_hip_plan *p, const void *d_stream, size_t nsamples, size_t first, size_t nframes, float *d_psd,
                                  float *d_dof, size_t row_pitch, int iters, void *hip_stream) {
  return adaptive_rows(p, d_stream, 1, 0, nsamples, first, nframes, d_psd, d_dof, row_pitch, iters, hip_stream);
}

}  // extern "C"
