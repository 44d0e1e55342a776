// glfer_hip.cpp -- the C-ABI of include/glfer_hip.h: the launches of a plan's estimators.
//
// Host side of the drop-in boundary.  The plan itself -- what fft_init()/mtm_init() build in the
// reference (fft.c:168-187, mtm.c:88-151) -- is made by plan.cpp from the tables of plan_tables.cpp;
// the entries here fill a kernel's argument block from it and launch.  No CPU fallback exists:
// every compute entry fails with GLFER_E_HIP when HIP cannot run it.
#include "plan.h"

#include <algorithm>
#include <cassert>
#include <cmath>
#include <cstdlib>
#include <cstdio>
#include <cstring>
#include <map>
#include <mutex>
#include <new>

#include "frame_cuts.h"
#include "channel_cuts.h"
#include "host_tables.h"
#include "ragged_cols.hpp"
#include "spectro_params.h"
#include "spectro_iq_params.h"
#include "ddc_params.h"

static_assert(GLFER_FMT_F32 == GLFER_SAMPLES_F32 && GLFER_FMT_S16 == GLFER_SAMPLES_S16 && GLFER_FMT_U8 == GLFER_SAMPLES_U8, "glfer_sample_size");

extern "C" hipError_t glfer_launch_hparma(const SpectroParams *sp, int n, int t, int ncol, const int *rot_sched, int rot_steps, int rot_width, const uint16_t *lagmap,
                                          const float2 *unit, hipStream_t st);
extern "C" hipError_t glfer_launch_hparma_batch(const SpectroParams *sp, int n, int t, int ncol, const int *rot_sched, int rot_steps, int rot_width,
                                                const uint16_t *lagmap, const float2 *unit, hipStream_t st);
extern "C" hipError_t glfer_launch_hparma_ragged(const SpectroParams *sp, const GlferRaggedEntry *streams, size_t nstreams, int n, int t, int ncol,
                                                 const int *rot_sched, int rot_steps, int rot_width, const uint16_t *lagmap, const float2 *unit,
                                                 hipStream_t st);
extern "C" hipError_t glfer_launch_avg(int mode, const float *psd, size_t nframes, int bins, int n_out,
                                       int depth, int minbin, int maxbin, int max0, double *avg,
                                       double *ret, hipStream_t st);
extern "C" hipError_t glfer_launch_avg_cum(const float *psd, size_t nframes, int bins, int n_out, int depth,
                                           int minbin, int maxbin, double *cum, hipStream_t st);
extern "C" hipError_t glfer_launch_lmp(const float *rows, long long row0, long long first, size_t nframes, int bins,
                                       int nl, float *out, hipStream_t st);
extern "C" hipError_t glfer_launch_lmp_batch(const float *rows, long long row0, long long first, size_t nframes, int bins, int nl,
                                             float *out, unsigned nb, long long row_stride, long long out_stride, hipStream_t st);
extern "C" hipError_t glfer_launch_lmp_ragged(const float *rows, const size_t *row_starts, size_t nstreams, int bins, int nl, float *out,
                                              hipStream_t st);
extern "C" hipError_t glfer_launch_ftest(const float *spec, size_t nframes, int n, int ntap, const double *U0,
                                         float sum_U0_sqr, int mu_live, float *ftest, hipStream_t st);
extern "C" hipError_t glfer_launch_ftest_rows(const float *spec, size_t nframes, int n, int ntap, const double *U0,
                                              float sum_U0_sqr, int mu_live, float *ftest, const float *cj, float *psd, int pitch,
                                              hipStream_t st);
extern "C" hipError_t glfer_launch_submean_tail_ex(const void *raw_last, const float *prev, float *out, int H, int fresh, int exact,
                                                   int fmt, hipStream_t st);
extern "C" hipError_t glfer_launch_hop_means_seq(const void *in, float *means, int H, long long nhops, int fmt, hipStream_t st);
extern "C" hipError_t glfer_launch_hop_means_seq_batch(const void *in, float *means, int H, long long nhops, int fmt, unsigned nb,
                                                       long long in_bstride, long long means_bstride, hipStream_t st);
extern "C" hipError_t glfer_launch_hop_means_tiled(const void *in, float *means, int H, long long nhops, int fmt, int hpw, unsigned blocks,
                                                   hipStream_t st);
extern "C" hipError_t glfer_launch_prepare(const SpectroParams *p, int n, const float *window, float *out,
                                           hipStream_t st);

static thread_local std::string g_hip_err;

namespace glfer {
int hip_fail(hipError_t e, const char *what) {
  char buf[256];
  snprintf(buf, sizeof buf, "%s: %s", what, hipGetErrorString(e));
  g_hip_err = buf;
  return GLFER_E_HIP;
}

std::string error_text() { return g_hip_err; }
void set_error_text(const std::string &text) { g_hip_err = text; }

int device_of(const void *d_ptr) {
  hipPointerAttribute_t at;
  if (!d_ptr || hipPointerGetAttributes(&at, d_ptr) != hipSuccess) {
    (void)hipGetLastError();
    return -1;
  }
  return at.type == hipMemoryTypeDevice || at.type == hipMemoryTypeManaged ? at.device : -1;
}
int data_device(const void *d_ptr) {
  int dev = device_of(d_ptr);
  if (dev < 0 && hipGetDevice(&dev) != hipSuccess) dev = 0;
  return dev;
}
// Dynamic LDS above the default limit has to be allowed per kernel -- and per DEVICE: a process that
// drives several GPUs (glfer_hip_spectrogram_host_multi) launches the same kernel on each.  One call
// per (device, kernel) and size class, not one per launch.
hipError_t allow_dynamic_lds(const void *kernel, size_t bytes) {
  static std::mutex mu;
  static std::map<std::pair<int, const void *>, size_t> allowed;
  int dev = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return e;
  std::lock_guard<std::mutex> lock(mu);
  size_t &have = allowed[{dev, kernel}];
  if (bytes <= have) return hipSuccess;
  e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
  if (e == hipSuccess) have = bytes;
  return e;
}

}  // namespace glfer
using glfer::data_device;
using glfer::DeviceGuard;
using glfer::hip_fail;

extern "C" {

const char *glfer_hip_version(void) { return "glfer_hip 0.9 (gfx950; 16 points/lane Stockham radix-16 with LDS exchange, inter-pass twiddles folded into the butterflies: packed pairs, real-input and wavefront-private forms, shared odd taper, register reuse across overlapped frames, mean removal in the reference's summation order (cfg.sub_mean = 1) or inside the kernels; N = 8..1048576; periodogram, multitaper + F-test, HP-ARMA with column-disjoint Jacobi rotations side by side and frames from a queue, LMP; rows at a caller's pitch; wavefront floor, fused average, display map with the average taken inside it; chunk ring for ingest with uploads and downloads at once, WAV files and waterfalls over several GPUs, read-ahead behind the per-hop shim, kept scratch blocks with a cap, workers bound to their GPU's NUMA node)"; }

int glfer_hip_abi_version(void) { return GLFER_HIP_ABI; }

int glfer_hip_palette(int palette, unsigned char colortab[768]) {
  if (!colortab) return GLFER_E_ARG;
  glfer::make_palette(palette, colortab);
  return GLFER_OK;
}

}  // extern "C"

extern "C" {

size_t glfer_hip_scratch_trim(int device, size_t keep_bytes) {
  size_t ring = 0;
  if (keep_bytes == 0 && device >= 0 && device < 64) {       // "give everything back": the parked ingest ring too
    DeviceGuard guard(device);
    if (guard.error() == hipSuccess) {
      ring = glfer::workers_kept_bytes(device);
      glfer::workers_drop_kept();                              // (their plans park one ring per device on the way out: dropped next)
      ring += glfer::ingest_ring_spare_bytes(device);
      glfer::ingest_ring_drop_spare(device);
    }
  }
  return ring + glfer::scratch_trim(device, keep_bytes);      // (what glfer_hip_scratch_held counted and is gone)
}
size_t glfer_hip_scratch_held(int device) { return glfer::scratch_held(device) + glfer::ingest_ring_spare_bytes(device) + glfer::workers_kept_bytes(device); }
void glfer_hip_scratch_limit(size_t bytes) {
  glfer::scratch_set_cap(bytes);
  if (bytes == 0) glfer::workers_drop_kept();
  // a parked chunk ring larger than the new cap goes back too (it is pinned host + device memory the host did not ask to keep)
  int cur = -1;
  if (hipGetDevice(&cur) != hipSuccess) cur = -1;
  for (int dev = 0; dev < 64; dev++)
    if (glfer::ingest_ring_spare_bytes(dev) > bytes) {
      DeviceGuard guard(dev);
      if (guard.error() == hipSuccess) glfer::ingest_ring_drop_spare(dev);
    }
}

const char *glfer_hip_strerror(int code) {
  switch (code) {
    case GLFER_OK: return "ok";
    case GLFER_E_ARG: return "bad argument or unsupported configuration";
    case GLFER_E_HIP: return "HIP runtime error";
    case GLFER_E_NOMEM: return "out of memory";
    case GLFER_E_NUMERIC: return "DPSS eigen-solve did not converge";
  }
  return "unknown error";
}

const char *glfer_hip_last_hip_error(void) { return g_hip_err.c_str(); }

extern "C" hipError_t glfer_launch_spectro_small(const SpectroParams *p, int n, const float *staps, hipStream_t st);
extern "C" hipError_t glfer_launch_spectro_big(const SpectroParams *p, int n, hipStream_t st);

// a launcher of N = 256 .. 16384 out of the table of built launchers (spectro_params.h), or its ragged twin (the same source
// compiled with GLFER_RAGGED: the stream from sp.ragged); nothing built for this kind and size: hipErrorInvalidValue
static hipError_t launch16(glfer_kind16 kind, const SpectroParams &sp, int n, hipStream_t st) {
  const glfer_launcher16_fn f = launcher16(kind, glfer_logn(n), sp.ragged != nullptr);
  return f ? f(&sp, st) : hipErrorInvalidValue;
}

static hipError_t launch_packed(const SpectroParams &sp, int n, hipStream_t st) {
  if (n < 256) return glfer_launch_spectro_small(&sp, n, sp.taps, st);   // the same role below the 16-points-per-lane range
  return launch16(GLFER_KIND_spectro16, sp, n, st);
}

static hipError_t launch_real_input(const SpectroParams &sp, int n, hipStream_t st) {
  return launch16(GLFER_KIND_spectro16h, sp, n, st);
}

// measured defaults: where spectro16w.hip is the faster form (profiles/r02_form_size_sweep.txt: the
// multitaper at N = 16384, every taper count; spectro16h.hip keeps the periodogram -- its coalesced
// sample loads beat the sub-transforms' strided ones when a frame is transformed only once -- and
// N = 8192)
#define GLFER_W_PERIODOGRAM(n) (false)
#define GLFER_W_MULTITAPER(n, tapers) ((n) >= 16384)

static int form_override();

static hipError_t launch_wave_private(const SpectroParams &sp, int n, hipStream_t st) {
  // N = 32768: the two-kernel form is the faster one (profiles/r02_big_blocks.txt); spectro16w.hip's single-kernel
  // form keeps the halfcomplex spectrum output and GLFER_FORM=w
  if (n == 32768) return (sp.spec || form_override() == 'w') ? glfer_launch_spectro16w_n15(&sp, st) : glfer_launch_spectro_big(&sp, n, st);
  if (n == 65536) return glfer_launch_spectro_big(&sp, n, st);
  if (n >= 131072 && n <= (1 << 20)) return glfer_launch_spectro_big(&sp, n, st);   // two-level combine (round 3)
  return launch16(GLFER_KIND_spectro16w, sp, n, st);
}

// Which form takes a configuration is a measured choice (profiles/r02_*): GLFER_FORM=h|w|x in the
// environment overrides it for A/B runs on one box (h: spectro16h, w: spectro16w, x: the packed /
// shared-odd-taper forms).
static int form_override() {
  const char *e = getenv("GLFER_FORM");          // read per launch: tests and A/B runs switch it in-process
  return e && *e ? (int)*e : 0;
}

// GLFER_Y_TAPERS=full in the environment: spectro16y.hip keeps its full-table form where the plan has half tables (same-box
// A/B runs and the tests that compare the two forms' rows; read per launch like GLFER_FORM)
static bool y_full_tables_forced() {
  const char *e = getenv("GLFER_Y_TAPERS");
  return e && !strcmp(e, "full");
}

// GLFER_Y_QUEUE=0 in the environment: spectro16y.hip keeps the static stride where it would draw its frame pairs from the
// plan's counter (same-box A/B runs and the tests that compare the two launch shapes' rows; read per launch).
// GLFER_Y_CHUNK=<pairs per ticket> overrides GLFER_YQ_CHUNK (the chunk sweep of profiles/y_frame_queue.txt).
static bool y_queue_off() {
  const char *e = getenv("GLFER_Y_QUEUE");
  return e && !strcmp(e, "0");
}
static int y_queue_chunk() {
  const char *e = getenv("GLFER_Y_CHUNK");
  const int c = e && *e ? atoi(e) : 0;
  return c >= 1 && c <= 64 ? c : GLFER_YQ_CHUNK;
}

// spectro16y.hip with its frame pairs from the plan's counter where that applies (see glfer_yqueue in plan.h for the streams
// that get a counter), else with the static stride
static hipError_t launch_y(SpectroParams &q, hipStream_t st) {
  q.yq_counter = nullptr;
  glfer_yqueue *yq = q.yq;
  if (!yq || q.mean_inkernel || q.nbatch > 1 || y_queue_off() || st == hipStreamPerThread) return launch16(GLFER_KIND_spectro16y, q, 4096, st);
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(st, &cs) != hipSuccess) {
    (void)hipGetLastError();
    return launch16(GLFER_KIND_spectro16y, q, 4096, st);
  }
  if (cs != hipStreamCaptureStatusNone) return launch16(GLFER_KIND_spectro16y, q, 4096, st);
  std::lock_guard<std::mutex> lock(yq->mu);
  int slot = 0;
  while (slot < yq->used && yq->owner[slot] != st) slot++;
  if (slot == yq->used) {
    if (slot == glfer_yqueue::SLOTS) return launch16(GLFER_KIND_spectro16y, q, 4096, st);
    yq->owner[yq->used++] = st;
  }
  q.yq_counter = yq->d_counters.get() + (size_t)slot * glfer_yqueue::PITCH;
  q.yq_base = yq->base[slot];
  q.yq_chunk = y_queue_chunk();
  const hipError_t e = glfer_launch_spectro16y_n12(&q, st);
  if (e == hipSuccess) yq->base[slot] += (unsigned)glfer_yq_chunks(q.nframes, q.yq_chunk);   // the tickets the launch draws
  return e;
}

static hipError_t launch_shared_odd(const SpectroParams &sp, int n, hipStream_t st) {
  if (n == 4096) {                     // two frames interleaved per wavefront
    SpectroParams q = sp;
    if (sp.ytaps && y_full_tables_forced()) q.ytaps = nullptr;
    return launch_y(q, st);
  }
  if (sp.ltaps) {                      // taper half tables resident in LDS
    if (const glfer_launcher16_fn f = launcher16(GLFER_KIND_spectro16xl, glfer_logn(n), sp.ragged != nullptr)) return f(&sp, st);
  }
  return launch16(GLFER_KIND_spectro16x, sp, n, st);
}

// Kernel choice.  spectro16.hip (two tapers packed per N-point transform) does everything; two
// specialisations take the frames that lie wholly inside the stream when they apply:
//   * one taper, PSD only      -> spectro16h.hip, real-input N/2-point transform
//   * odd taper count >= 3     -> last taper shared by two frames: spectro16y.hip (N = 4096, the two
//                                 frames interleaved per wavefront), spectro16xl.hip (taper half
//                                 tables in LDS, when they fit), spectro16x.hip otherwise
// The first ceil(R/H) frames of a stream reach back before sample 0 (zero history, fft.c:103-108);
// they stay with spectro16.hip, which has the range-checked gather for that.
enum BodyRoute { ROUTE_PACKED, ROUTE_REAL_INPUT, ROUTE_SHARED_ODD, ROUTE_WAVE_PRIVATE };
static BodyRoute body_route(const SpectroParams &sp, int n) {
  // spectro16h.hip fetches y[2j], y[2j+1] with one load: integer samples must then sit on naturally
  // aligned pairs (even hop, so every frame starts on an even sample, and an aligned stream)
  const unsigned esz = (unsigned)glfer_sample_size(sp.fmt);
  const bool pairs_aligned = sp.fmt == GLFER_FMT_F32 ||
                             ((sp.H & 1) == 0 && (reinterpret_cast<uintptr_t>(sp.stream) & (2u * esz - 1u)) == 0);
  const int force = form_override();
  bool real_input = sp.htaps && (sp.npairs == 1 || sp.htapers > 1) && n >= 512 && pairs_aligned;
  // built where it fits 3 waves/SIMD without spilling (N = 2048 and N >= 8192 do not: they stay packed)
  bool shared_odd = sp.xtaps && sp.npairs >= 2 && (sp.ltaps || n <= 1024 || n == 4096);
  // wavefront-private sub-transforms: the periodogram and the large-block multitaper by default
  // (GLFER_WAVE_PRIVATE_DEFAULT below), any multitaper at N >= 2048 on request
  bool wave_private = sp.wtaps && n >= 2048 && pairs_aligned &&
                      (force == 'w' || (force == 0 && (sp.npairs == 1 ? GLFER_W_PERIODOGRAM(n) : GLFER_W_MULTITAPER(n, sp.wtapers))));
  if (force == 'h') wave_private = false;
  if (force == 'x') wave_private = real_input = false;
  if (wave_private) real_input = true, shared_odd = false;
  if (sp.spec || sp.nonlin || !(real_input || shared_odd)) return ROUTE_PACKED;
  if (wave_private) return ROUTE_WAVE_PRIVATE;
  return real_input ? ROUTE_REAL_INPUT : ROUTE_SHARED_ODD;
}
// the forms that remove the hop means themselves (SpectroParams::mean_inkernel): the packed kernel,
// spectro16h.hip's periodogram form, spectro16y.hip, spectro16w.hip's multitaper form
static bool route_takes_mean(BodyRoute r, const SpectroParams &sp, int n) {
  if (n < 256 || n > 16384 || sp.spec || sp.nonlin || sp.history_mode) return false;
  if ((16 * sp.H) % n) return false;
  const int k16 = 16 * sp.H / n;
  switch (r) {
    case ROUTE_PACKED: return k16 == 4 || k16 == 8 || k16 == 16;
    case ROUTE_REAL_INPUT: return (sp.npairs == 1 && sp.htapers <= 1 && (k16 == 2 || k16 == 4 || k16 == 8 || k16 == 16)) ||
                                  (sp.htapers > 1 && n >= 8192 && k16 == 16);      // spectro16h.hip's multitaper form, hop = frame (its 50 / 75 % forms exist and lose to the copy: two wavefronts per SIMD against three)
    case ROUTE_SHARED_ODD: return (n == 4096 || n <= 1024) && (k16 == 4 || k16 == 8 || k16 == 16);   // y; x / xl while a frame sits in one wavefront
    case ROUTE_WAVE_PRIVATE: return sp.wtapers > 1 && (k16 == 8 || k16 == 16);     // spectro16w.hip's multitaper form (at 75 % overlap the copy is a quarter of a frame and wins: 7.50 against 7.36 M frames/s)
    default: return false;
  }
}

// ... and of those, the forms that subtract GIVEN means (round 3): spectro16h.hip's periodogram form, the packed
// kernel, spectro16y.hip
static bool route_takes_table(BodyRoute r, const SpectroParams &sp, int n) {
  switch (r) {
    // (round 4: every form that removes the means itself also takes them GIVEN -- spectro16w.hip's multitaper form (C4 with the
    // reference's order used to go through the corrected copy: 6.7 against 8.1 M frames/s), spectro16h.hip's multitaper form,
    // spectro16x / xl's frame loader)
    case ROUTE_PACKED: return true;
    case ROUTE_REAL_INPUT: return true;
    case ROUTE_SHARED_ODD: return true;
    case ROUTE_WAVE_PRIVATE: return true;
    default: return false;
  }
}

static hipError_t launch_by_n(const SpectroParams &sp, int n, hipStream_t st) {
  if (n > 16384) return launch_wave_private(sp, n, st);        // its general form takes every case itself
  const BodyRoute route = body_route(sp, n);
  const bool real_input = route == ROUTE_REAL_INPUT || route == ROUTE_WAVE_PRIVATE, wave_private = route == ROUTE_WAVE_PRIVATE;
  if (sp.mean_inkernel && !route_takes_mean(route, sp, n)) return hipErrorInvalidValue;
  if (route == ROUTE_PACKED) return launch_packed(sp, n, st);
  const long long first_inside = (long long)glfer_first_inside((size_t)sp.R, (size_t)sp.H);
  if (sp.mean_inkernel && sp.frame0 < first_inside) return hipErrorInvalidValue;   // (the caller sends the head frames another way)
  // only whole, globally aligned frame groups go to the route's kernel (frame_cuts.h; shard.py and the WAV reader cut streams
  // on multiples of GLFER_FRAME_ALIGN)
  const long long lo = sp.frame0, hi = sp.frame0 + sp.nframes;
  const glfer_frame_cut cut = glfer_cut_frames((size_t)lo, (size_t)hi, (size_t)first_inside, glfer_frame_group(route == ROUTE_SHARED_ODD, n));
  const long long b0 = (long long)cut.b0, b1 = (long long)cut.b1;
  if (sp.mean_inkernel && (b0 != lo || b1 != hi)) return hipErrorInvalidValue;   // (the caller cuts at the frame groups)
  if (b0 == b1) return launch_packed(sp, n, st);
  auto sub = [&](long long from, long long to) {
    SpectroParams q = sp;
    q.frame0 = from;
    q.nframes = (int)(to - from);
    q.psd = sp.psd + (size_t)(from - lo) * (size_t)sp.pitch;
    q.mean_inkernel = 0;                           // (head and tail frames: never with mean_inkernel, see above)
    q.means = nullptr;
    return q;
  };
  if (b0 > lo) {
    const SpectroParams head = sub(lo, b0);
    hipError_t e = launch_packed(head, n, st);
    if (e != hipSuccess) return e;
  }
  if (hi > b1) {
    const SpectroParams tail = sub(b1, hi);
    hipError_t e = launch_packed(tail, n, st);
    if (e != hipSuccess) return e;
  }
  SpectroParams body = sub(b0, b1);
  body.mean_inkernel = sp.mean_inkernel;
  body.means = sp.means;
  if (wave_private) return launch_wave_private(body, n, st);
  return real_input ? launch_real_input(body, n, st) : launch_shared_odd(body, n, st);
}

}  // extern "C"

// Fills the kernel argument block from a plan.
static void fill_params(const glfer_hip_plan *p, SpectroParams &sp) {
  memset(&sp, 0, sizeof sp);
  sp.H = p->hop;
  sp.R = p->keep;
  sp.npairs = p->npairs;
  sp.history_mode = p->cfg.history_mode ? 1 : 0;
  sp.pitch = p->pitch;
  sp.fmt = p->cfg.sample_format;
  sp.nonlin = p->nonlin ? 1 : 0;
  sp.limiter = (p->cfg.enable_limiter == 1);
  sp.a = p->cfg.limiter_a;
  sp.post_scale = p->spec_unscale;
  sp.spec_unscale = p->spec_unscale;
  sp.taps = p->d_taps.get();
  sp.tw = p->d_tw.as<float2>();
  sp.htaps = p->d_htaps.get();
  sp.htapers = p->htapers;
  sp.htw = p->d_htw.as<float2>();
  sp.hrot = p->d_hrot.as<float2>();
  sp.xtaps = p->d_xtaps.get();
  sp.ltaps = p->d_ltaps.get();
  sp.ytaps = p->d_ytaps.get();
  sp.yq = p->yq.get();
  sp.wtaps = p->d_wtaps.get();
  sp.wtapers = p->wtapers;
  sp.wtw = p->d_wtw.as<float2>();
  sp.wcomb = p->d_wcomb.as<float2>();
  sp.bigtw = p->d_bigtw.as<float2>();
}

// cfg.sub_mean: any non-zero value but GLFER_SUBMEAN_FAST asks for the reference's rows, i.e. the hop means in
// the reference's own summation order (1 = GLFER_SUBMEAN_EXACT is what fft_init stores: sub_mean = opt.autoscale)
static size_t plan_first_inside(const glfer_hip_plan *p) { return glfer_first_inside((size_t)p->keep, (size_t)p->hop); }
static bool reference_means(const glfer_hip_plan *p) { return p->cfg.sub_mean != 0 && p->cfg.sub_mean != GLFER_SUBMEAN_FAST; }

// K0 (fft.c:86-96) for the hops that frames [first, first+nframes) touch: the mean of each hop's
// NEW samples is removed before the hop enters the frame history, so every sample is corrected by
// the mean of the hop it arrived in.  ZERO_ALWAYS frames see only their own hop; otherwise a frame
// reaches back ceil(R/H) whole hops -- which is why a shard's or a chunk's halo is whole hops
// (glfer_hip.h, "Cutting a stream").  The corrected float copy lives in stream-ordered scratch
// (hipMallocAsync on `st`: nothing is shared between calls, the call stays asynchronous) and the
// kernels get its VIRTUAL base, so frame indices stay global and the frame groups of the
// shared-odd-taper kernels stay aligned to the stream, not to the launch.
//
// tail_fresh >= 0: the last hop is the file source's trailing partial block.  The caller has laid
// its fresh samples over a copy of the previous hop's RAW samples; what the reference's buffer
// holds there is the previous hop AFTER its mean removal (wav_fmt.c:102-119 over fft.c:93-95), so
// the last hop is rebuilt from the corrected previous hop before its own mean is taken.
// The copy is the caller's to hold until its launches are enqueued: it is left in `copy`, a guard on `st`.
static int submean_scratch(const glfer_hip_plan *p, SpectroParams &sp, size_t first, size_t nframes, hipStream_t st,
                           glfer::Scratch<float> &copy, long tail_fresh = -1) {
  // A batch (sp.nbatch streams, sp.batch_stride bytes apart): one copy per stream, side by side in one scratch block, from
  // launches that cover the whole batch; sp leaves with the copy of stream 0 and the copies' stride.
  const unsigned nb = glfer_batch_y(sp);
  assert(tail_fresh < 0 || nb == 1);   // (a trailing partial block is a file source's: one stream; no batch caller passes one)
  // ZERO_ALWAYS frames use only their own hop, and no kernel loads the history it would zero
  // (round 3: odd_taper.hpp::load_frame16, spectro16h / spectro16w's HIST gathers start their
  // descriptor at the frame's own hop), so the copy starts there too -- a piece cut for that mode
  // carries no history below its first hop (glfer_hip.h, "Cutting a stream", rule 2).
  const size_t hops_back = glfer_hops_back(sp.history_mode, plan_first_inside(p));
  const glfer_hop_span h = glfer_copy_hops(first, nframes, hops_back, tail_fresh >= 0);
  const size_t hop_lo = h.lo, nhops = h.n, per = nhops * (size_t)p->hop;
  HIP_TRY(copy.take((size_t)nb * per));
  float *scratch = copy.get();
  const size_t esz = glfer_sample_size(sp.fmt);
  const char *src = (const char *)sp.stream + hop_lo * (size_t)p->hop * esz;
  // GLFER_SUBMEAN_EXACT: the hop means first, accumulated sample after sample as fft.c:88-92 does
  // (submean_seq.hip: one more read of the stream), then the copy with those means
  const bool exact = reference_means(p);
  glfer::Scratch<float> means(st);
  hipError_t e = hipSuccess;
  if (exact) {
    e = means.take((size_t)nb * nhops);
    if (e == hipSuccess)
      e = glfer_launch_hop_means_seq_batch(src, means.get(), p->hop, (long long)nhops, sp.fmt, nb, sp.batch_stride, (long long)nhops, st);
  }
  if (e == hipSuccess)
    e = glfer_launch_submean_batch(src, scratch, p->hop, (long long)nhops, sp.fmt, st, means.get(), nb, sp.batch_stride, (long long)per,
                                   (long long)nhops);
  if (e == hipSuccess && tail_fresh >= 0)
    e = glfer_launch_submean_tail_ex(src + (nhops - 1) * (size_t)p->hop * esz, nhops > 1 ? scratch + (nhops - 2) * (size_t)p->hop : nullptr,
                                     scratch + (nhops - 1) * (size_t)p->hop, p->hop, (int)tail_fresh, exact ? 1 : 0, sp.fmt, st);
  if (e != hipSuccess) {
    copy.release();
    return hip_fail(e, "glfer_launch_submean");
  }
  sp.stream = reinterpret_cast<const char *>(scratch) - hop_lo * (size_t)p->hop * sizeof(float);
  sp.fmt = GLFER_FMT_F32;
  if (nb > 1) sp.batch_stride = (long long)(per * sizeof(float));
  return GLFER_OK;
}

// Can spectro16h.hip take the hop means out itself for this plan and call?  The periodogram (one
// window, PSD only, no RA9MB/limiter), history from the stream, a hop of 2, 4, 8 or all 16 of a
// lane's 16 sample registers (overlap 87.5 / 75 / 50 / 0 %), samples it can fetch in pairs, no
// trailing partial block, and the form not forced elsewhere (GLFER_FORM).  GLFER_MEAN_PREPASS=1
// keeps the pre-pass (A/B runs, and the tests that compare the two).
static bool mean_inkernel_ok(const glfer_hip_plan *p, const SpectroParams &sp, const float *d_spec, long tail_fresh) {
  if (p->nonlin || d_spec || tail_fresh >= 0 || sp.history_mode) return false;
  if (p->cfg.mode != GLFER_MODE_FFT && p->cfg.mode != GLFER_MODE_LMP && p->cfg.mode != GLFER_MODE_MTM) return false;
  const char *e = getenv("GLFER_MEAN_PREPASS");
  if (e && *e == '1') return false;
  const BodyRoute r = body_route(sp, p->n);
  if (!route_takes_mean(r, sp, p->n)) return false;
  // GLFER_SUBMEAN_EXACT: the kernels sum a hop in another order than fft.c:88-92, so they are handed the means
  // (SpectroParams::means) -- the forms that take a table: the periodogram, the packed kernel, spectro16y
  if (reference_means(p) && !route_takes_table(r, sp, p->n)) return false;
  return true;
}

// The hop means in the reference's own order (fft.c:88-92, submean_seq.hip) for hops [hop_lo, hop_lo + nhops) of the raw
// stream, into means[0 .. nhops): the tiled kernel where the hop and the stream's alignment allow it -- 16 or 4 hops per
// wavefront, whichever still gives the pass a few thousand wavefronts -- else 64 hops per wavefront.
static hipError_t launch_reference_means(const glfer_hip_plan *p, const SpectroParams &sp, size_t hop_lo, size_t nhops, float *means,
                                         unsigned blocks, hipStream_t st) {
  const size_t esz = glfer_sample_size(sp.fmt);
  const char *src = (const char *)sp.stream + hop_lo * (size_t)p->hop * esz;
  const int forced = [] { const char *e = getenv("GLFER_MEANS_HPW"); return e && *e ? atoi(e) : 0; }();
  int hpw = forced;
  // (measured, profiles/r04_piecewise_means.txt: on a whole 2^30-sample stream the tiled form with 16 hops per wavefront and
  // 16-byte loads is the faster one at H = 1024 -- C2 285 against 267 M frames/s --, level at H = 512, behind at H = 4096)
  if (!hpw) hpw = nhops >= 262144 ? (p->hop <= 2048 ? 16 : 64) : (nhops >= 32768 || p->hop % 1024 != 0 ? 16 : 4);
  if (hpw == 4 && p->hop % 1024 != 0) hpw = 16;
  if (hpw == 16 && p->hop % 256 != 0) hpw = 64;
  if ((hpw == 16 || hpw == 4) && (reinterpret_cast<uintptr_t>(src) & (4 * esz - 1)) == 0)
    return glfer_launch_hop_means_tiled(src, means, p->hop, (long long)nhops, sp.fmt, hpw, blocks, st);
  return glfer_launch_hop_means_seq(src, means, p->hop, (long long)nhops, sp.fmt, st);
}

// Frames [b0, b1) of the body (they lie inside the stream and on the kernel's frame groups) with GIVEN hop means
// (cfg.sub_mean = GLFER_SUBMEAN_EXACT: the reference's rows).  Round 3 took the means of the whole range in one launch and
// then ran the estimator: the stream came from HBM twice (C1 772 against 1 108, C2 230 against 277, C3 64 against 75 M
// frames/s).  Round 4: PIECE BY PIECE -- the means of piece c+1 (side stream) run beside the estimator launch of piece c,
// and a piece is small enough (samples + rows of two pieces under the 256 MiB Infinity Cache) that the estimator's read of
// it is served on-die: the stream leaves HBM once.  Pieces end on multiples of GLFER_FRAME_ALIGN frames, so every row is
// the one-launch row bit for bit.  GLFER_EXACT_PIECE_MB (samples per piece; 0 = one piece), GLFER_EXACT_STREAMS (1: means and
// estimator in turn on the caller's stream; 2: means on a side stream; 3: estimator launches alternate between the
// caller's stream and a second side stream as well), GLFER_MEANS_BLOCKS (grid of the tiled means kernel beside an
// estimator launch) are the knobs tools/exact_mean_time.py sweeps.
static int launch_body_with_reference_means(glfer_hip_plan *p, const SpectroParams &bs, size_t b0, size_t b1, hipStream_t st) {
  const long piece_mb = [] { const char *e = getenv("GLFER_EXACT_PIECE_MB"); return e && *e ? atol(e) : 0L; }();   // (read per call: the sweep sets them between calls)
  const int nstreams_env = [] {                                                  // 1..3: the plan has two side streams (aux[2]) and the join below knows three
    const char *e = getenv("GLFER_EXACT_STREAMS");
    const int v = e && *e ? atoi(e) : 2;
    return v < 1 ? 1 : (v > 3 ? 3 : v);
  }();
  const unsigned means_blocks = [] { const char *e = getenv("GLFER_MEANS_BLOCKS"); return e && *e ? (unsigned)atol(e) : 0u; }();
  const glfer_hop_span h = glfer_means_hops(b0, b1, 0, plan_first_inside(p));
  const size_t hop_lo = h.lo, nhops = h.n;
  const size_t esz = glfer_sample_size(bs.fmt);
  // frames per piece: a multiple of 64 frames (the frame groups of every form and GLFER_FRAME_ALIGN)
  size_t piece = b1 - b0;
  if (piece_mb > 0) {
    piece = ((size_t)piece_mb << 20) / ((size_t)p->hop * esz);
    piece = std::max<size_t>(piece / 64 * 64, 64);
  }
  const size_t npieces = (b1 - b0 + piece - 1) / piece;
  int nstreams = npieces > 1 ? nstreams_env : 1;
  // (on the caller's stream: the piecewise form gives it back below, after the join of the side streams and the failure path's waits)
  glfer::Scratch<float> means_buf(st);
  hipError_t e = means_buf.take(nhops);
  if (e != hipSuccess) return hip_fail(e, "scratch (hop means)");
  float *const means = means_buf.get();
  SpectroParams q = bs;
  q.means = means - hop_lo;                                                    // indexed by GLOBAL hop (= frame) index
  // THE FUSED LAUNCH (round 4, the periodogram's table form, N <= 8192; an EXPERIMENT, off by default): the hop means are
  // produced INSIDE the estimator's launch -- its first workgroups run the 64-hops-side-by-side chains of submean_seq.hip, the
  // others transform and wait for the chunks of means their frames need (spectro16h.hip produce_hop_means) -- so that the two
  // kinds of workgroup are co-resident whatever the streams' scheduling does and the means' read of the stream could ride in
  // the HBM bandwidth the periodogram kernel leaves idle.  Measured (profiles/r04_piecewise_means.txt): correct (rows
  // bit-identical), and NOT faster -- C1 753 M frames/s with 512 producer workgroups against 787 with the separate launch: the
  // fused launch moves its 12.9 GB at the same 4.6 TB/s the periodogram kernel reaches alone; the chip's rate for this 2 : 1
  // read : write mix, not idle time, is what the second read of the stream costs.
  // GLFER_MEANS_PRODUCERS: producer workgroups (a multiple of 8; 0 = the separate launch, the default).
  {
    const long producers = [] { const char *e = getenv("GLFER_MEANS_PRODUCERS"); return e && *e ? atol(e) : 0L; }();
    const bool periodogram_table = body_route(bs, p->n) == ROUTE_REAL_INPUT && bs.npairs == 1 && bs.htapers <= 1 && p->n <= 8192;
    // (short launches: the producers' lead over the first consumers is a bubble of nhops / producers' rate -- keep the two launches)
    const long min_frames = [] { const char *e = getenv("GLFER_FUSED_MIN_FRAMES"); return e && *e ? atol(e) : 65536L; }();   // (tests lower it)
    if (producers > 0 && periodogram_table && npieces == 1 && (long)(b1 - b0) >= min_frames) {
      // GLFER_FUSED_BLOCK_FRAMES > 0 (round 5): the lock-stepped form -- consumer workgroups of so many frames walked front by front,
      // a flag per 64-hop group, the producers GLFER_FUSED_LOOK hops (default 1024) beyond what their front's resident consumers span
      const long block_frames = [] { const char *e = getenv("GLFER_FUSED_BLOCK_FRAMES"); return e && *e ? atol(e) : 0L; }();
      const long look = [] { const char *e = getenv("GLFER_FUSED_LOOK"); return e && *e ? atol(e) : 1024L; }();
      const bool lockstep = block_frames > 0;
      const int chunk = lockstep ? 64 : 4096;
      const size_t nchunks = (nhops + chunk - 1) / chunk;
      glfer::Scratch<unsigned> ready_buf(st);
      e = ready_buf.take(nchunks + 8);
      unsigned *const ready = ready_buf.get();
      if (e == hipSuccess) e = hipMemsetAsync(ready, 0, (nchunks + 8) * sizeof(unsigned), st);
      if (e == hipSuccess) {
        q.nprod = (int)(producers / 8 * 8);
        q.prod_chunk = chunk;
        q.means_out = means - hop_lo;
        q.means_ready = ready;
        q.prod_hop0 = (long long)hop_lo;
        q.prod_nhops = (long long)nhops;
        if (lockstep) {
          q.prod_front_frames = -1;                                            // (the launcher sizes the fronts from its grid)
          q.prod_block_frames = (int)block_frames;
          q.prod_look = (int)look;
          q.front_done = ready + nchunks;
        }
        e = launch_by_n(q, p->n, st);
      }
      return e == hipSuccess ? GLFER_OK : hip_fail(e, "estimator launch (hop means produced in the launch)");
    }
  }
  static std::mutex aux_mu;
  bool own_aux = false;
  if (nstreams > 1) {                                                          // the side streams and their events, once per plan
    std::lock_guard<std::mutex> lock(aux_mu);
    if (p->aux_busy) {
      nstreams = 1;                                                            // another call of this plan is on them: stay on the caller's stream
    } else {
      for (int i = 0; i < nstreams - 1 && e == hipSuccess; i++)
        if (!p->aux[i]) e = hipStreamCreateWithFlags(&p->aux[i], hipStreamNonBlocking);
      while (e == hipSuccess && p->aux_events.size() < 2 * npieces + 1) {
        hipEvent_t ev = nullptr;
        e = hipEventCreateWithFlags(&ev, hipEventDisableTiming);
        if (e == hipSuccess) p->aux_events.push_back(ev);
      }
      if (e != hipSuccess) {
        (void)hipGetLastError();
        nstreams = 1;
        e = hipSuccess;
      } else {
        p->aux_busy = own_aux = true;
      }
    }
  }
  if (nstreams <= 1) {
    for (size_t c = 0; c < npieces && e == hipSuccess; c++) {
      const size_t f0 = b0 + c * piece, f1 = std::min(b1, f0 + piece);
      const size_t h0 = c == 0 ? hop_lo : f0;
      e = launch_reference_means(p, bs, h0, f1 - h0, means + (h0 - hop_lo), 0, st);
      q.frame0 = (long long)f0;
      q.nframes = (int)(f1 - f0);
      q.psd = bs.psd + (f0 - b0) * (size_t)p->pitch;
      if (e == hipSuccess) e = launch_by_n(q, p->n, st);
    }
    return e == hipSuccess ? GLFER_OK : hip_fail(e, "estimator launch (given hop means)");
  }
  // means(c) on aux[0]; estimator(c) on the caller's stream (or alternately aux[1]) after means(c); means(c + 2) not before
  // estimator(c) is done, so that at most two pieces are between their two reads at any time.  (An event may be recorded
  // again once every wait on its previous record has been ENQUEUED -- a wait captures the record it follows -- so the
  // plan's events serve call after call.)
  hipStream_t sm = p->aux[0];
  hipEvent_t *ev_m = p->aux_events.data(), *ev_e = ev_m + npieces, ev_fork = p->aux_events[2 * npieces];
  e = hipEventRecord(ev_fork, st);                                             // the samples (and the scratch) are ordered on the caller's stream
  if (e == hipSuccess) e = hipStreamWaitEvent(sm, ev_fork, 0);
  if (e == hipSuccess && nstreams > 2) e = hipStreamWaitEvent(p->aux[1], ev_fork, 0);
  size_t launched = 0;
  for (size_t c = 0; c < npieces && e == hipSuccess; c++) {
    const size_t f0 = b0 + c * piece, f1 = std::min(b1, f0 + piece);
    const size_t h0 = c == 0 ? hop_lo : f0;
    if (c >= 2) e = hipStreamWaitEvent(sm, ev_e[c - 2], 0);
    if (e == hipSuccess) e = launch_reference_means(p, bs, h0, f1 - h0, means + (h0 - hop_lo), c == 0 ? 0 : means_blocks, sm);
    if (e == hipSuccess) e = hipEventRecord(ev_m[c], sm);
    hipStream_t se = (nstreams > 2 && (c & 1)) ? p->aux[1] : st;
    if (e == hipSuccess) e = hipStreamWaitEvent(se, ev_m[c], 0);
    q.frame0 = (long long)f0;
    q.nframes = (int)(f1 - f0);
    q.psd = bs.psd + (f0 - b0) * (size_t)p->pitch;
    if (e == hipSuccess) e = launch_by_n(q, p->n, se);
    if (e == hipSuccess) e = hipEventRecord(ev_e[c], se);
    if (e == hipSuccess) launched = c + 1;
  }
  // join: the caller's stream goes on after everything the side streams were given
  if (nstreams > 2)
    for (size_t c = launched >= 2 ? launched - 2 : 0; c < launched; c++)
      if (c & 1) (void)hipStreamWaitEvent(st, ev_e[c], 0);
  if (e != hipSuccess) {                                                       // a launch failed midway: the side streams may hold work nothing waits for
    (void)hipStreamSynchronize(sm);
    if (nstreams > 2) (void)hipStreamSynchronize(p->aux[1]);
  }
  means_buf.release();
  if (own_aux) {
    std::lock_guard<std::mutex> lock(aux_mu);
    p->aux_busy = false;
  }
  return e == hipSuccess ? GLFER_OK : hip_fail(e, "estimator launch (given hop means, piecewise)");
}

// Periodograms of frames [sp.frame0, sp.frame0 + sp.nframes), to sp.psd, with the mean removal (fft.c:86-96) done inside the
// estimator kernel: the frames that lie inside the stream read the RAW stream and no corrected copy is written for them; the
// first ceil(R/H) frames of a stream (zero history: the packed kernel) and the frames off the route's frame groups keep the
// copy, a few hops long.  sp: fill_params + the raw stream -- or the raw streams of a batch (nbatch and the batch strides):
// every launch then covers the whole batch, and the body's reference-order hop means are one table per stream.
static int launch_mean_inkernel(glfer_hip_plan *p, const SpectroParams &sp, hipStream_t st) {
  const size_t first = (size_t)sp.frame0, end = first + (size_t)sp.nframes;
  const size_t first_inside = plan_first_inside(p);
  const glfer_frame_cut cut = glfer_cut_frames(first, end, first_inside, glfer_frame_group(body_route(sp, p->n) == ROUTE_SHARED_ODD, p->n));
  const size_t b0 = cut.b0, b1 = cut.b1;
  const unsigned nb = glfer_batch_y(sp);
  int rc = GLFER_OK;
  // frames [from, to) through the corrected copy (the stream's first frames, a lone frame off the pair grid)
  auto by_copy = [&](size_t from, size_t to) {
    if (rc != GLFER_OK || from >= to) return;
    SpectroParams hs = sp;
    hs.frame0 = (long long)from;
    hs.nframes = (int)(to - from);
    hs.psd = sp.psd + (from - first) * (size_t)p->pitch;
    glfer::Scratch<float> copy(st);
    rc = submean_scratch(p, hs, from, to - from, st, copy);
    if (rc == GLFER_OK) {
      hipError_t e = launch_by_n(hs, p->n, st);
      if (e != hipSuccess) rc = hip_fail(e, nb > 1 ? "estimator launch (batch, frames through the corrected copies)" : "estimator launch (frames through the corrected copy)");
    }
  };
  by_copy(first, b0);
  if (rc == GLFER_OK && b1 > b0) {
    SpectroParams bs = sp;
    bs.frame0 = (long long)b0;
    bs.nframes = (int)(b1 - b0);
    bs.psd = sp.psd + (b0 - first) * (size_t)p->pitch;
    bs.spec = nullptr;
    bs.mean_inkernel = 1;
    if (!reference_means(p)) {
      hipError_t e = launch_by_n(bs, p->n, st);
      if (e != hipSuccess) rc = hip_fail(e, nb > 1 ? "estimator launch (batch, mean removal in the kernel)" : "estimator launch (mean removal in the kernel)");
    } else if (sp.nbatch == 0) {                                         // the single-stream entry (a batch chunk of one stream keeps the batch's launches)
      rc = launch_body_with_reference_means(p, bs, b0, b1, st);
    } else {                                                             // a batch: one table per stream, nhops apart, from one launch
      const glfer_hop_span h = glfer_means_hops(b0, b1, 0, first_inside);
      glfer::Scratch<float> means(st);
      hipError_t e = means.take((size_t)nb * h.n);
      if (e == hipSuccess)
        e = glfer_launch_hop_means_seq_batch((const char *)sp.stream + h.lo * (size_t)p->hop * glfer_sample_size(sp.fmt), means.get(), p->hop,
                                             (long long)h.n, sp.fmt, nb, sp.batch_stride, (long long)h.n, st);
      bs.means = means.get() - h.lo;                                     // indexed by the stream's own hop (= frame) index
      bs.means_batch_stride = (long long)h.n;
      if (e == hipSuccess) e = launch_by_n(bs, p->n, st);
      if (e != hipSuccess) rc = hip_fail(e, "estimator launch (batch, mean removal in the kernel)");
    }
  }
  by_copy(b1, end);
  return rc;
}

int glfer_run_device(glfer_hip_plan *p, const void *d_stream, size_t nsamples, size_t first, size_t nframes,
                     float *d_psd, float *d_spec, hipStream_t st, long tail_fresh) {
  if (!p || !d_stream || (!d_psd && nframes)) return GLFER_E_ARG;
  if (nframes == 0) return GLFER_OK;
  if ((first + nframes) > nsamples / (size_t)p->hop) return GLFER_E_ARG;   // frame past the stream
  if (nframes > 0x7fffffffu) return GLFER_E_ARG;
  if (d_spec && p->cfg.mode != GLFER_MODE_FFT) return GLFER_E_ARG;
  DeviceGuard guard(p->cfg.device);
  HIP_TRY(guard.error());

  SpectroParams sp;
  fill_params(p, sp);
  sp.stream = d_stream;
  sp.frame0 = (long long)first;
  sp.nframes = (int)nframes;
  sp.psd = d_psd;
  sp.spec = d_spec;

  glfer::Scratch<float> copy(st), rows(st);
  if (tail_fresh >= 0 && (tail_fresh >= (long)p->hop || p->cfg.mode == GLFER_MODE_LMP)) return GLFER_E_ARG;
  const bool inkernel = p->cfg.sub_mean && mean_inkernel_ok(p, sp, d_spec, tail_fresh);
  if (inkernel && p->cfg.mode != GLFER_MODE_LMP) return launch_mean_inkernel(p, sp, st);
  if (p->cfg.sub_mean && !inkernel)
    if (const int rc = submean_scratch(p, sp, first, nframes, st, copy, tail_fresh); rc != GLFER_OK) return rc;
  if (p->cfg.mode != GLFER_MODE_LMP) {
    const hipError_t e = p->cfg.mode == GLFER_MODE_HPARMA
                             ? glfer_launch_hparma(&sp, p->n, p->cfg.hparma_t, p->cfg.hparma_p_e + 1, p->d_rot_sched.get(), p->rot_steps, p->rot_width, p->d_lagmap.get(), p->d_unit.as<float2>(), st)
                             : launch_by_n(sp, p->n, st);
    return e == hipSuccess ? GLFER_OK : hip_fail(e, "estimator launch");
  }
  // lmp.c:101-181: periodograms of the frames the ring holds when frame first+nframes-1 is done
  // (lmp_av - 1 frames before `first`, recomputed rather than carried), then the statistic
  const size_t back = std::min<size_t>((size_t)p->lmp_av - 1, first);
  const size_t nrows = nframes + back;
  hipError_t e = rows.take(nrows * (size_t)p->bins);
  if (e != hipSuccess) return hip_fail(e, "hipMallocAsync(lmp rows)");
  if (!inkernel && back && p->cfg.sub_mean) {
    // the extra frames reach further back than the hops corrected above
    sp.stream = d_stream;
    sp.fmt = p->cfg.sample_format;
    if (const int rc = submean_scratch(p, sp, first - back, nrows, st, copy); rc != GLFER_OK) return rc;
  }
  sp.frame0 = (long long)(first - back);
  sp.nframes = (int)nrows;
  sp.psd = rows.get();
  if (inkernel) {
    if (const int rc = launch_mean_inkernel(p, sp, st); rc != GLFER_OK) return rc;
  } else {
    e = launch_by_n(sp, p->n, st);
    if (e != hipSuccess) return hip_fail(e, "lmp launch");
  }
  e = glfer_launch_lmp(rows.get(), (long long)(first - back), (long long)first, nframes, p->bins, p->lmp_av, d_psd, st);
  return e == hipSuccess ? GLFER_OK : hip_fail(e, "lmp launch");
}

extern "C" {

int glfer_hip_spectrogram_device(glfer_hip_plan *p, const void *d_stream, size_t nsamples, size_t first,
                                 size_t nframes, float *d_psd, void *hip_stream) {
  return glfer_run_device(p, d_stream, nsamples, first, nframes, d_psd, nullptr, (hipStream_t)hip_stream);
}

// Many streams of one plan in one call (glfer_hip.h).  The estimator kernels at N = 256 .. 16384, the hop-means kernel and the
// corrected copy carry a stream dimension (blockIdx.y; SpectroParams::nbatch / batch_stride / psd_batch_stride /
// means_batch_stride): the routing, the cuts into head / body / tail frames and the hops each piece needs are those of ONE
// stream (launch_by_n, launch_mean_inkernel, submean_scratch), and every launch they produce covers the whole batch, so the
// rows are those of the single-stream entry and the launch count does not grow with the batch.

// the streams one launch takes: the current device's grid y limit, at least `floor`
static int grid_y_limit(int floor, size_t *ymax) {
  int dev = 0, y = 0;
  HIP_TRY(hipGetDevice(&dev));
  HIP_TRY(hipDeviceGetAttribute(&y, hipDeviceAttributeMaxGridDimY, dev));
  *ymax = (size_t)std::max(floor, std::min(y, 65535));
  return GLFER_OK;
}

// the plans whose rows a batch computes in the launches of one stream (the others go stream by stream): the estimator kernels'
// stream dimension at N = 256 .. 16384, and HP-ARMA at every N a plan accepts -- its launch runs over the flat list of all
// streams' frames (hparma.hip, HpPlace) -- but for a plan built with GLFER_HPARMA_WIDTH=16 (A/B runs: a single-stream kernel)
static bool batch_one_launch(const glfer_hip_plan *p) {
  if (p->cfg.mode == GLFER_MODE_HPARMA) return p->rot_width != 16;
  return (p->cfg.mode == GLFER_MODE_FFT || p->cfg.mode == GLFER_MODE_MTM || p->cfg.mode == GLFER_MODE_LMP) && p->n >= 256 && p->n <= 16384;
}
// LMP batches keep the periodograms of a chunk of streams in scratch: the streams whose rows (stream_bytes each) take at most
// half the kept-scratch cap (plan.h scratch_cap: glfer_hip_scratch_limit / GLFER_SCRATCH_CAP_MB, 16 GiB by default), one at least
static size_t lmp_chunk_streams(size_t stream_bytes) {
  return std::max<size_t>(1, (glfer::scratch_cap() / 2) / std::max<size_t>(stream_bytes, 1));
}
static int batch_rows(glfer_hip_plan *p, const void *d_streams, size_t nstreams, size_t stream_pitch, size_t nsamples, size_t first,
                      size_t nframes, float *d_psd, size_t psd_bs, hipStream_t st);

int glfer_hip_spectrogram_batch_device(glfer_hip_plan *p, const void *d_streams, size_t nstreams, size_t stream_pitch,
                                       size_t nsamples, size_t first, size_t nframes, float *d_psd, void *hip_stream) {
  if (!p) return GLFER_E_ARG;
  if (nstreams == 0 || nframes == 0) return GLFER_OK;
  if (!d_streams || !d_psd) return GLFER_E_ARG;
  if ((first + nframes) > nsamples / (size_t)p->hop) return GLFER_E_ARG;   // frame past the stream
  if (nframes > 0x7fffffffu) return GLFER_E_ARG;
  const int fmt = p->cfg.sample_format;
  const size_t esz = glfer_sample_size(fmt);
  // body_route (and spectro16w's launcher) read the stream's alignment for integer samples: every stream must see the
  // same kernels, so an odd pitch -- every other stream off the pair alignment -- is refused rather than routed per stream
  if (fmt != GLFER_FMT_F32 && (stream_pitch & 1)) return GLFER_E_ARG;
  const size_t rows = (size_t)p->pitch;
  if (stream_pitch > (SIZE_MAX / esz) / nstreams || nframes > (SIZE_MAX / sizeof(float) / rows) / nstreams) return GLFER_E_ARG;
  return batch_rows(p, d_streams, nstreams, stream_pitch, nsamples, first, nframes, d_psd, nframes * rows, (hipStream_t)hip_stream);
}

// the body of glfer_hip_spectrogram_batch_device, arguments checked: stream b's rows at d_psd + b * psd_bs floats
static int batch_rows(glfer_hip_plan *p, const void *d_streams, size_t nstreams, size_t stream_pitch, size_t nsamples, size_t first,
                      size_t nframes, float *d_psd, size_t psd_bs, hipStream_t st) {
  const int fmt = p->cfg.sample_format;
  const size_t esz = glfer_sample_size(fmt);
  const char *base = static_cast<const char *>(d_streams);
  if (!batch_one_launch(p) || nstreams == 1) {
    for (size_t b = 0; b < nstreams; b++) {
      const int rc = glfer_run_device(p, base + b * stream_pitch * esz, nsamples, first, nframes, d_psd + b * psd_bs, nullptr, st);
      if (rc != GLFER_OK) return rc;
    }
    return GLFER_OK;
  }
  DeviceGuard guard(p->cfg.device);
  HIP_TRY(guard.error());
  size_t ymax = 0;
  if (const int yrc = grid_y_limit(1, &ymax); yrc != GLFER_OK) return yrc;
  // LMP (lmp.c:101-181): the periodograms of frames [first - back, first + nframes) of every stream go to scratch -- back: the
  // frames the ring still holds at `first`, recomputed as glfer_run_device recomputes them, the mean-corrected copy reaching
  // back with them -- and one batched statistic launch set follows (glfer_launch_lmp_batch).  The call is cut into chunks of
  // streams whose periodograms take at most half the kept-scratch cap (glfer_hip_scratch_limit; 8 GiB by default), one stream
  // at least: the launch count grows with the bytes, not with the streams.
  // HP-ARMA: the corrected copies of a chunk's streams (submean_scratch, as for the other plans), then ONE launch over the chunk's
  // nb x nframes frames (glfer_launch_hparma_batch); mean_inkernel_ok refuses the mode.
  const bool lmp = p->cfg.mode == GLFER_MODE_LMP, hparma = p->cfg.mode == GLFER_MODE_HPARMA;
  const size_t back = lmp ? std::min<size_t>((size_t)p->lmp_av - 1, first) : 0;
  const size_t nrows = nframes + back, lmp_bs = nrows * (size_t)p->bins;
  if (lmp) ymax = std::min(ymax, lmp_chunk_streams(lmp_bs * sizeof(float)));
  for (size_t c0 = 0; c0 < nstreams; c0 += ymax) {      // batches above the grid's y limit: chunks of it
    const unsigned nb = (unsigned)std::min(nstreams - c0, ymax);
    if ((lmp || hparma) && nb == 1) {                   // (a chunk of one stream: the single-stream entry)
      const int rc = glfer_run_device(p, base + c0 * stream_pitch * esz, nsamples, first, nframes, d_psd + c0 * psd_bs, nullptr, st);
      if (rc != GLFER_OK) return rc;
      continue;
    }
    glfer::Scratch<float> rows(st);
    if (lmp) {
      const hipError_t e = rows.take((size_t)nb * lmp_bs);
      if (e != hipSuccess) return hip_fail(e, "scratch (lmp rows, batch)");
    }
    SpectroParams sp;
    fill_params(p, sp);
    sp.stream = base + c0 * stream_pitch * esz;
    sp.frame0 = (long long)(first - back);
    sp.nframes = (int)nrows;
    sp.psd = lmp ? rows.get() : d_psd + c0 * psd_bs;
    sp.nbatch = (int)nb;
    sp.batch_stride = (long long)(stream_pitch * esz);
    sp.psd_batch_stride = (long long)(lmp ? lmp_bs : psd_bs);
    if (p->cfg.sub_mean && mean_inkernel_ok(p, sp, nullptr, -1)) {
      if (const int rc = launch_mean_inkernel(p, sp, st); rc != GLFER_OK) return rc;
    } else {
      glfer::Scratch<float> copy(st);
      if (p->cfg.sub_mean)
        if (const int rc = submean_scratch(p, sp, first - back, nrows, st, copy); rc != GLFER_OK) return rc;
      const hipError_t e = hparma ? glfer_launch_hparma_batch(&sp, p->n, p->cfg.hparma_t, p->cfg.hparma_p_e + 1, p->d_rot_sched.get(), p->rot_steps,
                                                              p->rot_width, p->d_lagmap.get(), p->d_unit.as<float2>(), st)
                                  : launch_by_n(sp, p->n, st);
      if (e != hipSuccess) return hip_fail(e, "estimator launch (batch)");
    }
    if (lmp) {
      const hipError_t e = glfer_launch_lmp_batch(rows.get(), (long long)(first - back), (long long)first, nframes, p->bins, p->lmp_av,
                                                  d_psd + c0 * psd_bs, nb, (long long)lmp_bs, (long long)psd_bs, st);
      if (e != hipSuccess) return hip_fail(e, "lmp launch (batch)");
    }
  }
  return GLFER_OK;
}

// ---- complex I/Q input (glfer_hip.h): two-sided rows of N bins, spectro16c.hip ---------------------------------------------------

static hipError_t launch_iq(const IqParams &q, int n, hipStream_t st) {
  const auto f = launcher16_iq(glfer_logn(n));
  return f ? f(&q, st) : hipErrorInvalidValue;
}

int glfer_hip_spectrogram_iq_batch_device(glfer_hip_plan *p, const void *d_iq, size_t nstreams, size_t stream_pitch, size_t nsamples,
                                          size_t first, size_t nframes, float *d_psd, size_t row_pitch, unsigned flags,
                                          void *hip_stream) {
  if (!p || !p->d_iqtaps || glfer_hip_iq_supported(&p->cfg) != GLFER_OK) return GLFER_E_ARG;
  if (flags & ~(GLFER_IQ_CENTERED | GLFER_IQ_SWAP)) return GLFER_E_ARG;
  const size_t n = (size_t)p->n, pitch = row_pitch ? row_pitch : n;
  if (pitch < n) return GLFER_E_ARG;
  if (nstreams == 0 || nframes == 0) return GLFER_OK;
  if (!d_iq || !d_psd) return GLFER_E_ARG;
  const size_t csz = 2 * glfer_sample_size(p->cfg.sample_format);       // bytes of a complex sample
  if (reinterpret_cast<uintptr_t>(d_iq) & (csz - 1)) return GLFER_E_ARG;
  if (first + nframes < first || (first + nframes) > nsamples / (size_t)p->hop) return GLFER_E_ARG;   // wraps, or a frame past the stream
  if (nframes > 0x7fffffffu) return GLFER_E_ARG;
  if (nsamples > SIZE_MAX / csz || stream_pitch > (SIZE_MAX / csz) / nstreams) return GLFER_E_ARG;
  if (pitch > SIZE_MAX / sizeof(float) / nframes || nframes * pitch > (SIZE_MAX / sizeof(float)) / nstreams) return GLFER_E_ARG;
  hipStream_t st = (hipStream_t)hip_stream;
  DeviceGuard guard(p->cfg.device);
  HIP_TRY(guard.error());
  size_t ymax = 1;
  if (nstreams > 1)
    if (const int yrc = grid_y_limit(1, &ymax); yrc != GLFER_OK) return yrc;
  IqParams q;
  memset(&q, 0, sizeof q);
  q.frame0 = (long long)first;
  q.nframes = (int)nframes;
  q.H = p->hop;
  q.R = p->keep;
  q.ntap = p->ntapers;
  q.history_mode = p->cfg.history_mode ? 1 : 0;
  q.fmt = p->cfg.sample_format;
  q.flags = flags;
  q.taps = p->d_iqtaps.get();
  q.tw = p->d_tw.as<float2>();
  q.pitch = (long long)pitch;
  q.batch_stride = (long long)(stream_pitch * csz);
  q.psd_batch_stride = (long long)(nframes * pitch);
  for (size_t c0 = 0; c0 < nstreams; c0 += ymax) {      // batches above the grid's y limit: chunks of it
    const size_t nb = std::min(nstreams - c0, ymax);
    q.stream = static_cast<const char *>(d_iq) + c0 * stream_pitch * csz;
    q.psd = d_psd + c0 * nframes * pitch;
    q.nbatch = (int)nb;
    const hipError_t e = launch_iq(q, p->n, st);
    if (e != hipSuccess) return hip_fail(e, "estimator launch (iq)");
  }
  return GLFER_OK;
}

int glfer_hip_spectrogram_iq_device(glfer_hip_plan *p, const void *d_iq, size_t nsamples, size_t first, size_t nframes, float *d_psd,
                                    size_t row_pitch, unsigned flags, void *hip_stream) {
  return glfer_hip_spectrogram_iq_batch_device(p, d_iq, 1, 0, nsamples, first, nframes, d_psd, row_pitch, flags, hip_stream);
}

// ---- digital down-converter and zoom (glfer_hip.h): ddc.hip, then the I/Q rows of its output ----------------------------------

struct glfer_hip_ddc {
  glfer_hip_ddc_config cfg;
  unsigned long long W = 0;
  float2 *d_taps = nullptr;         // [min(D, T)][jpad]: g[j D + r] at [r][j] (ddc_params.h)
};

unsigned long long glfer_hip_ddc_phase_word(double freq) { return glfer::ddc_phase_word(freq); }

int glfer_hip_ddc_design(int decim, int ntaps, double cutoff, double beta, float *taps) {
  if (decim < 1 || decim > 1024 || ntaps > 8192) return GLFER_E_ARG;
  glfer::ddc_design_defaults(decim, &ntaps, &cutoff, &beta);
  if (!(cutoff <= 0.5) || !(beta < 700.0)) return GLFER_E_ARG;
  if (taps) glfer::ddc_design(ntaps, cutoff, beta, taps);
  return ntaps;
}

int glfer_hip_ddc_supported(const glfer_hip_ddc_config *cfg) {
  if (!cfg) return GLFER_E_ARG;
  if (cfg->decim < 1 || cfg->decim > 1024 || cfg->ntaps < 1 || cfg->ntaps > 8192) return GLFER_E_ARG;
  if (!(cfg->freq >= -0.5 && cfg->freq < 0.5)) return GLFER_E_ARG;
  if (cfg->sample_format < 0 || cfg->sample_format > 2) return GLFER_E_ARG;
  if (cfg->complex_in != 0 && cfg->complex_in != 1) return GLFER_E_ARG;
  return GLFER_OK;
}

int glfer_hip_ddc_tables(const glfer_hip_ddc_config *cfg, const float *taps, float *g) {
  if (glfer_hip_ddc_supported(cfg) != GLFER_OK || !taps || !g) return GLFER_E_ARG;
  glfer::ddc_tables(glfer::ddc_phase_word(cfg->freq), cfg->ntaps, taps, g);
  return GLFER_OK;
}

int glfer_hip_ddc_create(const glfer_hip_ddc_config *cfg, const float *taps, glfer_hip_ddc **out) {
  if (!out) return GLFER_E_ARG;
  *out = nullptr;
  if (glfer_hip_ddc_supported(cfg) != GLFER_OK || !taps) return GLFER_E_ARG;
  const int D = cfg->decim, T = cfg->ntaps, rows = std::min(D, T), jpad = ddc_jpad(D, T);
  std::vector<float> g((size_t)2 * T), perm((size_t)2 * rows * jpad, 0.0f);
  const unsigned long long W = glfer::ddc_phase_word(cfg->freq);
  glfer::ddc_tables(W, T, taps, g.data());
  for (int t = 0; t < T; t++) {
    const size_t at = (size_t)(t % D) * jpad + (size_t)(t / D);
    perm[2 * at] = g[2 * t];
    perm[2 * at + 1] = g[2 * t + 1];
  }
  glfer_hip_ddc *d = new (std::nothrow) glfer_hip_ddc;
  if (!d) return GLFER_E_NOMEM;
  d->cfg = *cfg;
  d->W = W;
  DeviceGuard guard(cfg->device);
  hipError_t e = guard.error();
  if (e == hipSuccess) e = glfer_ddc_prepare();
  if (e == hipSuccess) e = hipMalloc((void **)&d->d_taps, perm.size() * sizeof(float));
  if (e == hipSuccess) e = hipMemcpy(d->d_taps, perm.data(), perm.size() * sizeof(float), hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    const int rc = hip_fail(e, "ddc tables");
    (void)hipGetLastError();
    glfer_hip_ddc_destroy(d);
    return rc;
  }
  *out = d;
  return GLFER_OK;
}

void glfer_hip_ddc_destroy(glfer_hip_ddc *d) {
  if (!d) return;
  DeviceGuard guard(d->cfg.device);
  if (d->d_taps) (void)hipFree(d->d_taps);
  delete d;
}

int glfer_hip_ddc_batch_device(glfer_hip_ddc *d, const void *d_in, size_t nstreams, size_t stream_pitch, size_t nsamples, size_t first,
                               size_t nout, void *d_out, size_t out_pitch, void *hip_stream) {
  if (!d) return GLFER_E_ARG;
  const size_t opitch = out_pitch ? out_pitch : nout;
  if (opitch < nout) return GLFER_E_ARG;
  if (nstreams == 0 || nout == 0) return GLFER_OK;
  if (!d_in || !d_out) return GLFER_E_ARG;
  const size_t D = (size_t)d->cfg.decim, T = (size_t)d->cfg.ntaps;
  const size_t esz = glfer_sample_size(d->cfg.sample_format) * (d->cfg.complex_in ? 2 : 1);   // bytes of one input sample
  if (first + nout < first || first + nout > nsamples / D) return GLFER_E_ARG;                // wraps, or an output past the stream
  if (nout > 0x7fffffffu) return GLFER_E_ARG;
  if (reinterpret_cast<uintptr_t>(d_in) & (esz - 1)) return GLFER_E_ARG;
  if (nsamples > ((size_t)1 << 62) / esz || stream_pitch > (((size_t)1 << 62) / esz) / nstreams) return GLFER_E_ARG;
  if (opitch > (((size_t)1 << 62) / sizeof(float2)) / nstreams) return GLFER_E_ARG;
  hipStream_t st = (hipStream_t)hip_stream;
  DeviceGuard guard(d->cfg.device);
  HIP_TRY(guard.error());
  size_t ymax = 1;
  if (nstreams > 1)
    if (const int yrc = grid_y_limit(1, &ymax); yrc != GLFER_OK) return yrc;
  DdcParams q;
  memset(&q, 0, sizeof q);
  q.taps = d->d_taps;
  q.W = d->W;
  q.first_out = (long long)first;
  q.end_out = (long long)(first + nout);
  q.lo_sample = first * D > T - 1 ? (long long)(first * D - (T - 1)) : 0;
  q.in_stride = (long long)(stream_pitch * esz);
  q.out_stride = (long long)opitch;
  q.D = (int)D;
  q.T = (int)T;
  q.jmax = ddc_jmax((int)D, (int)T);
  q.jpad = ddc_jpad((int)D, (int)T);
  q.cols = ddc_cols((int)D, (int)T);
  q.rows = (int)std::min(D, T);
  q.rc = ddc_rows_per_chunk((int)D, (int)T);
  q.plane = q.rc * q.cols;
  q.rlast = (int)((T - 1) % D);
  q.ntiles = (int)((nout + kDdcTile - 1) / kDdcTile);
  q.fmt = d->cfg.sample_format;
  q.complex_in = d->cfg.complex_in;
  for (size_t c0 = 0; c0 < nstreams; c0 += ymax) {      // batches above the grid's y limit: chunks of it
    q.in = static_cast<const char *>(d_in) + c0 * stream_pitch * esz;
    q.out = static_cast<float2 *>(d_out) + c0 * opitch;
    q.nbatch = (int)std::min(nstreams - c0, ymax);
    const hipError_t e = glfer_launch_ddc(&q, st);
    if (e != hipSuccess) return hip_fail(e, "ddc launch");
  }
  return GLFER_OK;
}

int glfer_hip_ddc_device(glfer_hip_ddc *d, const void *d_in, size_t nsamples, size_t first, size_t nout, void *d_out, void *hip_stream) {
  return glfer_hip_ddc_batch_device(d, d_in, 1, 0, nsamples, first, nout, d_out, 0, hip_stream);
}

int glfer_hip_spectrogram_zoom_device(glfer_hip_plan *p, glfer_hip_ddc *d, const void *d_in, size_t nsamples, size_t first, size_t nframes,
                                      float *d_psd, size_t row_pitch, unsigned flags, void *hip_stream) {
  if (!p || !d || !p->d_iqtaps || glfer_hip_iq_supported(&p->cfg) != GLFER_OK || p->cfg.sample_format != GLFER_SAMPLES_F32) return GLFER_E_ARG;
  if (p->cfg.device != d->cfg.device) return GLFER_E_ARG;
  if (flags & ~GLFER_IQ_CENTERED) return GLFER_E_ARG;
  const size_t n = (size_t)p->n, H = (size_t)p->hop, pitch = row_pitch ? row_pitch : n;
  if (pitch < n) return GLFER_E_ARG;
  if (nframes == 0) return GLFER_OK;
  if (!d_in || !d_psd) return GLFER_E_ARG;
  const size_t nbase = nsamples / (size_t)d->cfg.decim;                  // complex samples of the baseband stream
  if (first + nframes < first || first + nframes > nbase / H) return GLFER_E_ARG;
  if (nframes > 0x7fffffffu) return GLFER_E_ARG;
  const size_t hi = (first + nframes) * H, lo = first * H > n - H ? first * H - (n - H) : 0;
  if (hi - lo > 0x7fffffffu) return GLFER_E_ARG;                         // (one DDC launch: its outputs count in 31 bits)
  hipStream_t st = (hipStream_t)hip_stream;
  DeviceGuard guard(p->cfg.device);
  HIP_TRY(guard.error());
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  if (st != hipStreamPerThread && hipStreamIsCapturing(st, &cs) == hipSuccess && cs != hipStreamCaptureStatusNone) return GLFER_E_ARG;
  (void)hipGetLastError();
  glfer::Scratch<float2> base(st);
  HIP_TRY(base.take(hi - lo));
  const int rc = glfer_hip_ddc_device(d, d_in, nsamples, lo, hi - lo, base.get(), st);
  if (rc != GLFER_OK) return rc;
  // the baseband's virtual base: its sample 0 lies lo samples below the scratch
  return glfer_hip_spectrogram_iq_device(p, base.get() - lo, nbase, first, nframes, d_psd, pitch, flags, st);
}

// ---- multi-channel recordings (glfer_hip.h): every interleaved channel as a stream of its own ---------------------------------

static bool channels_wide() {                       // GLFER_CHANNELS_WIDE=0: the general form everywhere (A/B runs)
  const char *e = getenv("GLFER_CHANNELS_WIDE");
  return !(e && *e == '0');
}

int glfer_hip_deinterleave_device(const void *d_in, size_t nframes, int channels, int sample_format, const int *select, int nselect,
                                  void *d_out, size_t out_pitch, void *hip_stream) {
  unsigned char sel[GLFER_MAX_CHANNELS];
  const int nsel = glfer_channel_selection(channels, select, nselect, sel);
  if (!nsel) return GLFER_E_ARG;
  if (sample_format != GLFER_SAMPLES_F32 && sample_format != GLFER_SAMPLES_S16 && sample_format != GLFER_SAMPLES_U8) return GLFER_E_ARG;
  if (out_pitch < nframes) return GLFER_E_ARG;
  if (nframes == 0) return GLFER_OK;
  if (!d_in || !d_out) return GLFER_E_ARG;
  const size_t esz = glfer_sample_size(sample_format);
  if (nframes > (SIZE_MAX / esz) / (size_t)channels || out_pitch > (SIZE_MAX / esz) / (size_t)nsel) return GLFER_E_ARG;
  DeviceGuard guard(glfer::data_device(d_in));
  HIP_TRY(guard.error());
  const hipError_t e = glfer_launch_deinterleave(d_in, nframes, channels, (int)esz, sel, nsel, d_out, out_pitch, channels_wide() ? 1 : 0,
                                                 (hipStream_t)hip_stream);
  return e == hipSuccess ? GLFER_OK : hip_fail(e, "deinterleave launch");
}

int glfer_hip_spectrogram_channels_device(glfer_hip_plan *p, const void *d_samples, size_t nsamples_per_channel, int channels,
                                          const int *select, int nselect, size_t first, size_t nframes, float *d_psd,
                                          void *hip_stream) {
  if (!p) return GLFER_E_ARG;
  unsigned char sel[GLFER_MAX_CHANNELS];
  const int nsel = glfer_channel_selection(channels, select, nselect, sel);
  if (!nsel) return GLFER_E_ARG;
  if (nframes == 0) return GLFER_OK;
  if (!d_samples || !d_psd) return GLFER_E_ARG;
  if (first > SIZE_MAX - nframes || (first + nframes) > nsamples_per_channel / (size_t)p->hop) return GLFER_E_ARG;   // frame past the recording
  if (nframes > 0x7fffffffu) return GLFER_E_ARG;
  const size_t esz = glfer_sample_size(p->cfg.sample_format), hop = (size_t)p->hop, rows = (size_t)p->pitch;
  if (nsamples_per_channel > (SIZE_MAX / esz) / (size_t)channels || nframes > (SIZE_MAX / sizeof(float) / rows) / (size_t)nsel)
    return GLFER_E_ARG;
  hipStream_t st = (hipStream_t)hip_stream;
  // one channel, the default selection: the recording is the stream
  if (channels == 1 && !select) return glfer_run_device(p, d_samples, nsamples_per_channel, first, nframes, d_psd, nullptr, st);
  DeviceGuard guard(p->cfg.device);
  HIP_TRY(guard.error());
  // The hops frames [at, end) read go to scratch planes and the batch entry's body runs on the planes' virtual base, the frame
  // indices left global.  Planes of more than half the scratch cap: pieces of frames (channel_cuts.h), each with its own halo.
  const size_t halo = glfer_channel_halo((size_t)p->keep, hop, p->cfg.mode == GLFER_MODE_LMP ? (size_t)p->lmp_av : 0);
  const size_t budget = glfer::scratch_cap() / 2, end = first + nframes;
  const char *src = static_cast<const char *>(d_samples);
  for (size_t at = first; at < end;) {
    const size_t to = glfer_channel_piece_end(at, end, halo, hop, esz, (size_t)nsel, budget);
    const glfer_hop_span h = glfer_channel_hops(at, to - at, halo);
    const size_t plane = h.n * hop, pitch = glfer_plane_pitch(plane, esz);
    glfer::Scratch<char> planes(st);
    hipError_t e = planes.take((size_t)nsel * pitch * esz);
    if (e != hipSuccess) return hip_fail(e, "scratch (channel planes)");
    e = glfer_launch_deinterleave(src + h.lo * hop * (size_t)channels * esz, plane, channels, (int)esz, sel, nsel, planes.get(), pitch,
                                  channels_wide() ? 1 : 0, st);
    if (e != hipSuccess) return hip_fail(e, "deinterleave launch");
    const int rc = batch_rows(p, planes.get() - h.lo * hop * esz, (size_t)nsel, pitch, nsamples_per_channel, at, to - at,
                              d_psd + (at - first) * rows, nframes * rows, st);
    if (rc != GLFER_OK) return rc;
    at = to;
  }
  return GLFER_OK;
}

}  // extern "C"

// Streams of unequal length in one call (glfer_hip.h).  Every launch the single-stream entry would make for a stream -- the
// packed kernel for its first frames and for the frames off the frame groups, the route's kernel for its body, the hop means and
// the corrected copies of the mean removal -- is made ONCE for all streams: blockIdx.y indexes a table (GlferRaggedEntry /
// GlferRaggedHops, spectro_params.h) that holds each stream's samples, rows, means and its own frames of that launch, cut stream
// by stream with the functions launch_by_n and launch_mean_inkernel cut with (frame_cuts.h).  The tables are built here and go to
// stream-ordered scratch.
namespace {

struct RaggedStream {
  size_t off;        // first sample, in elements from the call's d_samples
  size_t frames;     // lengths[b] / hop
  size_t row;        // first row of d_psd
};

// one ragged launch set over the streams of a chunk (nb <= the grid's y limit, >= 2)
struct RaggedChunk {
  glfer_hip_plan *p;
  const RaggedStream *s;
  unsigned nb;
  const char *base;    // the call's d_samples
  float *d_psd;
  hipStream_t st;
  size_t esz;
  size_t first_inside;

  // a table to the device (Scratch::upload, on st)
  template <typename T>
  int upload(const std::vector<T> &host, glfer::Scratch<T> &dev) const {
    const hipError_t e = dev.upload(host.data(), host.size());
    return e == hipSuccess ? GLFER_OK : hip_fail(e, "ragged table upload");
  }

  // one launch over a table; sp: everything but frame0 / nframes / nbatch / ragged.  r: the kernel (ROUTE_PACKED: the packed one)
  int launch(SpectroParams sp, const std::vector<GlferRaggedEntry> &tab, BodyRoute r) const {
    long long f0 = -1;
    int longest = 0;
    for (const GlferRaggedEntry &e : tab)
      if (e.nframes > 0) {
        if (f0 < 0 || e.frame0 < f0) f0 = e.frame0;
        longest = std::max(longest, e.nframes);
      }
    if (longest == 0) return GLFER_OK;
    glfer::Scratch<GlferRaggedEntry> d_tab(st);
    const int rc = upload(tab, d_tab);
    if (rc != GLFER_OK) return rc;
    sp.frame0 = f0;                  // (the launchers check the range and size the grid with these; the kernels read the table)
    sp.nframes = longest;
    sp.nbatch = (int)nb;
    sp.ragged = d_tab.get();
    hipError_t e;
    if (r == ROUTE_PACKED) e = launch_packed(sp, p->n, st);
    else if (r == ROUTE_WAVE_PRIVATE) e = launch_wave_private(sp, p->n, st);
    else e = r == ROUTE_REAL_INPUT ? launch_real_input(sp, p->n, st) : launch_shared_odd(sp, p->n, st);
    return e == hipSuccess ? GLFER_OK : hip_fail(e, "estimator launch (ragged)");
  }

  // launch_by_n over the streams: frames [from[b], to[b]) of stream b, whose sample 0 is soff[b] bytes from sp.stream
  int by_n(const SpectroParams &sp, const std::vector<long long> &soff, const std::vector<size_t> &from,
           const std::vector<size_t> &to) const {
    if (p->cfg.mode == GLFER_MODE_HPARMA) {                              // no routes and no frame groups: one launch over all frames
      std::vector<GlferRaggedEntry> all(nb);
      for (unsigned b = 0; b < nb; b++) {
        all[b] = GlferRaggedEntry{};
        if (to[b] <= from[b]) continue;
        all[b].stream_off = soff[b];
        all[b].psd_off = (long long)((s[b].row + from[b]) * (size_t)p->pitch);
        all[b].frame0 = (long long)from[b];
        all[b].nframes = (int)(to[b] - from[b]);
      }
      const hipError_t e = glfer_launch_hparma_ragged(&sp, all.data(), nb, p->n, p->cfg.hparma_t, p->cfg.hparma_p_e + 1, p->d_rot_sched.get(),
                                                      p->rot_steps, p->rot_width, p->d_lagmap.get(), p->d_unit.as<float2>(), st);
      return e == hipSuccess ? GLFER_OK : hip_fail(e, "estimator launch (HP-ARMA, ragged)");
    }
    // the route of THESE samples, as launch_by_n reads it: a corrected copy is f32 whatever the raw format, so its frames may
    // take a real-input kernel where the raw stream's alignment (or an odd hop) keeps the raw samples on the packed one
    SpectroParams r0 = sp;
    r0.stream = reinterpret_cast<const char *>(sp.stream) + soff[0];
    const BodyRoute r = body_route(r0, p->n);
    const size_t G = glfer_frame_group(r == ROUTE_SHARED_ODD, p->n);
    std::vector<GlferRaggedEntry> head(nb), tail(nb), body(nb);
    auto entry = [&](unsigned b, size_t f0, size_t f1) {
      GlferRaggedEntry e = {};
      if (f1 > f0) {
        e.stream_off = soff[b];
        e.psd_off = (long long)((s[b].row + f0) * (size_t)p->pitch);
        e.frame0 = (long long)f0;
        e.nframes = (int)(f1 - f0);
      }
      return e;
    };
    for (unsigned b = 0; b < nb; b++) {
      const size_t lo = from[b], hi = std::max(to[b], from[b]);
      glfer_frame_cut c = glfer_cut_frames(lo, hi, first_inside, G);
      if (r == ROUTE_PACKED) c.b0 = c.b1 = hi;                         // (the packed route: everything is head)
      head[b] = entry(b, lo, c.b0);
      body[b] = entry(b, c.b0, c.b1);
      tail[b] = entry(b, c.b1, hi);
    }
    SpectroParams q = sp;
    q.mean_inkernel = 0;
    q.means = nullptr;
    int rc = launch(q, head, ROUTE_PACKED);
    if (rc == GLFER_OK) rc = launch(q, tail, ROUTE_PACKED);
    if (rc == GLFER_OK) rc = launch(q, body, r);
    return rc;
  }

  // submean_scratch over the streams: the corrected copy of hops [hlo[b], hhi[b]) of stream b, side by side in one block;
  // soff[b] leaves as the copy's virtual sample 0 in bytes from the block, which is left in the caller's `copy` (empty: no hops)
  int submean(int fmt, const std::vector<size_t> &hlo, const std::vector<size_t> &hhi, glfer::Scratch<float> &copy,
              std::vector<long long> &soff) const {
    const size_t H = (size_t)p->hop;
    size_t total = 0, longest = 0;
    for (unsigned b = 0; b < nb; b++) {
      const size_t n = hhi[b] > hlo[b] ? hhi[b] - hlo[b] : 0;
      total += n;
      longest = std::max(longest, n);
    }
    copy.release();
    if (total == 0) return GLFER_OK;
    glfer::Scratch<float> means(st);
    HIP_TRY(copy.take(total * H));
    const bool exact = reference_means(p);
    hipError_t e = exact ? means.take(total) : hipSuccess;
    std::vector<GlferRaggedHops> tab(nb);
    size_t at = 0;
    for (unsigned b = 0; b < nb; b++) {
      const size_t n = hhi[b] > hlo[b] ? hhi[b] - hlo[b] : 0;
      tab[b].in = base + (s[b].off + hlo[b] * H) * esz;
      tab[b].out = copy.get() + at * H;
      tab[b].means = means ? means.get() + at : nullptr;
      tab[b].nhops = (long long)n;
      soff[b] = ((long long)at - (long long)hlo[b]) * (long long)(H * sizeof(float));
      at += n;
    }
    glfer::Scratch<GlferRaggedHops> d_tab(st);
    int rc = e == hipSuccess ? upload(tab, d_tab) : hip_fail(e, "scratch (hop means, ragged)");
    if (rc == GLFER_OK) {
      if (exact) e = glfer_launch_hop_means_seq_ragged(d_tab.get(), nb, p->hop, (long long)longest, fmt, st);
      if (e == hipSuccess) e = glfer_launch_submean_ragged(d_tab.get(), nb, p->hop, (long long)longest, fmt, exact ? 1 : 0, st);
      if (e != hipSuccess) rc = hip_fail(e, "glfer_launch_submean_ragged");
    }
    if (rc != GLFER_OK) copy.release();
    return rc;
  }

  // frames [from[b], to[b]) through corrected copies (launch_mean_inkernel's by_copy, and the plans whose kernels take no means)
  int by_copy(const SpectroParams &sp, const std::vector<size_t> &from, const std::vector<size_t> &to) const {
    const size_t hops_back = glfer_hops_back(sp.history_mode, first_inside);
    std::vector<size_t> hlo(nb), hhi(nb);
    std::vector<long long> soff(nb);
    for (unsigned b = 0; b < nb; b++) {
      const glfer_hop_span h = glfer_copy_hops(from[b], to[b] > from[b] ? to[b] - from[b] : 0, hops_back, 0);
      hlo[b] = h.lo;
      hhi[b] = h.lo + h.n;
    }
    glfer::Scratch<float> copy(st);
    const int rc = submean(sp.fmt, hlo, hhi, copy, soff);
    if (rc != GLFER_OK || !copy) return rc;
    SpectroParams hs = sp;
    hs.stream = copy.get();
    hs.fmt = GLFER_FMT_F32;
    return by_n(hs, soff, from, to);
  }

  int run() {
    SpectroParams sp;
    fill_params(p, sp);
    sp.stream = base;
    sp.psd = d_psd;
    esz = glfer_sample_size(sp.fmt);
    // (every stream sees the route of stream 0: integer samples sit at even offsets -- glfer_hip.h; by_n reads the route of the
    // samples a launch is given, raw or corrected copy, as launch_by_n does)
    SpectroParams s0 = sp;
    s0.stream = base + s[0].off * esz;
    first_inside = plan_first_inside(p);
    std::vector<size_t> zero(nb, 0), end(nb);
    std::vector<long long> raw(nb);
    for (unsigned b = 0; b < nb; b++) {
      end[b] = s[b].frames;
      raw[b] = (long long)(s[b].off * esz);
    }
    if (!p->cfg.sub_mean) return by_n(sp, raw, zero, end);
    if (!mean_inkernel_ok(p, s0, nullptr, -1)) return by_copy(sp, zero, end);
    // launch_mean_inkernel per stream: [0, b0) and [b1, end) through the copies, [b0, b1) from the raw samples (their route)
    const BodyRoute route = body_route(s0, p->n);
    const size_t G = glfer_frame_group(route == ROUTE_SHARED_ODD, p->n);
    std::vector<size_t> b0(nb), b1(nb);
    for (unsigned b = 0; b < nb; b++) {
      const glfer_frame_cut c = glfer_cut_frames(0, end[b], first_inside, G);
      b0[b] = c.b0;
      b1[b] = c.b1;
    }
    int rc = by_copy(sp, zero, b0);
    if (rc != GLFER_OK) return rc;
    {
      SpectroParams bs = sp;
      bs.mean_inkernel = 1;
      std::vector<GlferRaggedEntry> body(nb);
      glfer::Scratch<float> means(st);
      glfer::Scratch<GlferRaggedHops> d_hops(st);
      if (reference_means(p)) {                      // the hop means in the reference's order: hops [b0 - first_inside, b1) of each stream
        std::vector<GlferRaggedHops> hops(nb);
        size_t total = 0, longest = 0;
        for (unsigned b = 0; b < nb; b++) total += glfer_means_hops(b0[b], b1[b], 0, first_inside).n;
        if (total) {
          HIP_TRY(means.take(total));
          size_t at = 0;
          for (unsigned b = 0; b < nb; b++) {
            const glfer_hop_span h = glfer_means_hops(b0[b], b1[b], 0, first_inside);
            const size_t hop_lo = h.lo, n = h.n;
            hops[b].in = base + (s[b].off + hop_lo * (size_t)p->hop) * esz;
            hops[b].out = nullptr;
            hops[b].means = means.get() + at;
            hops[b].nhops = (long long)n;
            body[b].means_off = (long long)at - (long long)hop_lo;       // indexed by the stream's own hop (= frame) index
            longest = std::max(longest, n);
            at += n;
          }
          rc = upload(hops, d_hops);
          if (rc != GLFER_OK) return rc;
          const hipError_t e = glfer_launch_hop_means_seq_ragged(d_hops.get(), nb, p->hop, (long long)longest, sp.fmt, st);
          if (e != hipSuccess) return hip_fail(e, "hop means (ragged)");
          bs.means = means.get();
        }
      }
      for (unsigned b = 0; b < nb; b++) {
        if (b1[b] <= b0[b]) {
          body[b] = GlferRaggedEntry{};
          continue;
        }
        body[b].stream_off = raw[b];
        body[b].psd_off = (long long)((s[b].row + b0[b]) * (size_t)p->pitch);
        body[b].frame0 = (long long)b0[b];
        body[b].nframes = (int)(b1[b] - b0[b]);
      }
      rc = launch(bs, body, route);
      if (rc != GLFER_OK) return rc;
    }
    return by_copy(sp, b1, end);
  }
};

}  // namespace

extern "C" {

size_t glfer_hip_ragged_frames(const glfer_hip_plan *p, size_t nstreams, const size_t *lengths, size_t *row_starts) {
  if (!p || (nstreams && !lengths)) return 0;
  size_t total = 0;
  for (size_t b = 0; b < nstreams; b++) {
    if (row_starts) row_starts[b] = total;
    const size_t f = lengths[b] / (size_t)p->hop;
    if (f > SIZE_MAX - total) return SIZE_MAX;
    total += f;
  }
  if (row_starts) row_starts[nstreams] = total;
  return total;
}

int glfer_hip_spectrogram_ragged_device(glfer_hip_plan *p, const void *d_samples, size_t nstreams, const size_t *offsets,
                                        const size_t *lengths, float *d_psd, size_t *row_starts, void *hip_stream) {
  if (!p) return GLFER_E_ARG;
  if (nstreams == 0) {
    if (row_starts) row_starts[0] = 0;
    return GLFER_OK;
  }
  if (!offsets || !lengths) return GLFER_E_ARG;
  const int fmt = p->cfg.sample_format;
  const size_t esz = glfer_sample_size(fmt);
  // the arguments, before anything is read or written: the host arrays are all this looks at
  std::vector<RaggedStream> s(nstreams);
  size_t total = 0;
  for (size_t b = 0; b < nstreams; b++) {
    const size_t f = lengths[b] / (size_t)p->hop;
    if (f > 0x7fffffffu) return GLFER_E_ARG;
    if (lengths[b] > SIZE_MAX / esz || offsets[b] > SIZE_MAX / esz - lengths[b]) return GLFER_E_ARG;
    // body_route and the launchers read a stream's alignment for integer samples (pairs come with one load): every stream of a
    // launch must see the same kernels, so an odd offset is refused rather than routed per stream (as the batch entry's odd pitch)
    if (fmt != GLFER_FMT_F32 && (offsets[b] & 1)) return GLFER_E_ARG;
    if (f > SIZE_MAX / sizeof(float) / (size_t)p->pitch - total) return GLFER_E_ARG;
    s[b] = RaggedStream{offsets[b], f, total};
    total += f;
  }
  if (row_starts) {
    for (size_t b = 0; b < nstreams; b++) row_starts[b] = s[b].row;
    row_starts[nstreams] = total;
  }
  if (total == 0) return GLFER_OK;
  if (!d_samples || !d_psd) return GLFER_E_ARG;
  hipStream_t st = (hipStream_t)hip_stream;
  // the per-stream tables are uploaded from host memory that is gone when the call returns: a copy node of a captured graph
  // would read it at every replay, so a capturing stream is refused
  if (glfer::stream_is_capturing(st)) return GLFER_E_ARG;
  const char *base = static_cast<const char *>(d_samples);
  auto single = [&](size_t b) {
    if (!s[b].frames) return (int)GLFER_OK;
    return glfer_run_device(p, base + s[b].off * esz, lengths[b], 0, s[b].frames, d_psd + s[b].row * (size_t)p->pitch, nullptr, st);
  };
  if (!batch_one_launch(p) || nstreams == 1) {      // N outside 256 .. 16384 (but HP-ARMA's): stream by stream, as batch_rows
    for (size_t b = 0; b < nstreams; b++) {
      const int rc = single(b);
      if (rc != GLFER_OK) return rc;
    }
    return GLFER_OK;
  }
  DeviceGuard guard(p->cfg.device);
  HIP_TRY(guard.error());
  size_t ymax = 0;
  if (const int yrc = grid_y_limit(2, &ymax); yrc != GLFER_OK) return yrc;
  // LMP: a chunk's packed periodogram rows go to scratch (the ragged launch set, as for an FFT plan) and the ragged statistic runs
  // over the same row starts into d_psd (glfer_launch_lmp_ragged).  A chunk takes the streams whose rows fit half the kept-scratch
  // cap (lmp_chunk_streams), one at least.
  const bool lmp = p->cfg.mode == GLFER_MODE_LMP;
  const size_t bins = (size_t)p->bins, lmp_rows_max = lmp_chunk_streams(bins * sizeof(float));
  for (size_t c0 = 0; c0 < nstreams;) {                 // above the grid's y limit: chunks of it
    unsigned nb = (unsigned)std::min(nstreams - c0, ymax);
    if (lmp) {
      unsigned k = 1;
      while (k < nb && s[c0 + k].row + s[c0 + k].frames - s[c0].row <= lmp_rows_max) k++;
      nb = k;
    }
    int rc = GLFER_OK;
    if (nb == 1) {
      rc = single(c0);
    } else if (!lmp) {
      RaggedChunk c{p, s.data() + c0, nb, base, d_psd, st, esz, 0};
      rc = c.run();
    } else if (const size_t r0 = s[c0].row, nrows = s[c0 + nb - 1].row + s[c0 + nb - 1].frames - r0; nrows != 0) {
      std::vector<RaggedStream> rel(s.begin() + c0, s.begin() + c0 + nb);      // the chunk's streams, rows counted from its scratch
      std::vector<size_t> starts(nb + 1, nrows);
      for (unsigned b = 0; b < nb; b++) starts[b] = rel[b].row -= r0;
      glfer::Scratch<float> rows(st);
      const hipError_t e = rows.take(nrows * bins);
      if (e != hipSuccess) return hip_fail(e, "scratch (lmp rows, ragged)");
      RaggedChunk c{p, rel.data(), nb, base, rows.get(), st, esz, 0};
      rc = c.run();
      if (rc == GLFER_OK) {
        const hipError_t le = glfer_launch_lmp_ragged(rows.get(), starts.data(), nb, p->bins, p->lmp_av, d_psd + r0 * bins, st);
        if (le != hipSuccess) rc = hip_fail(le, "lmp launch (ragged)");
      }
    }
    if (rc != GLFER_OK) return rc;
    c0 += nb;
  }
  return GLFER_OK;
}

int glfer_hip_spectrum_device(glfer_hip_plan *p, const void *d_stream, size_t nsamples, size_t first,
                              size_t nframes, float *d_psd, float *d_spec, void *hip_stream) {
  if (!d_spec) return GLFER_E_ARG;
  return glfer_run_device(p, d_stream, nsamples, first, nframes, d_psd, d_spec, (hipStream_t)hip_stream);
}

// prepare_audio (fft.c:66-165) for a batch of frames: what it leaves in params->inbuf_fft
// (lmp.c:101-120 and g_scope.c:194-197 read it).  d_frames: [nframes][N] floats.
int glfer_hip_prepare_device(glfer_hip_plan *p, const void *d_stream, size_t nsamples, size_t first,
                             size_t nframes, float *d_frames, void *hip_stream) {
  if (!p || !d_stream || (!d_frames && nframes)) return GLFER_E_ARG;
  if (nframes == 0) return GLFER_OK;
  if ((first + nframes) > nsamples / (size_t)p->hop || nframes > 0x7fffffffu) return GLFER_E_ARG;
  hipStream_t st = (hipStream_t)hip_stream;
  DeviceGuard guard(p->cfg.device);
  HIP_TRY(guard.error());
  SpectroParams sp;
  fill_params(p, sp);
  sp.stream = d_stream;
  sp.frame0 = (long long)first;
  sp.nframes = (int)nframes;
  glfer::Scratch<float> copy(st);
  if (p->cfg.sub_mean)
    if (const int rc = submean_scratch(p, sp, first, nframes, st, copy); rc != GLFER_OK) return rc;
  // MTM / HP-ARMA / LMP run prepare_audio with a rectangular window (source.c:344,369,395); a and
  // the limiter still act on inbuf_fft there, but those estimators overwrite it, so the shims ask
  // for this only in FFT mode
  const hipError_t e = glfer_launch_prepare(&sp, p->n, p->d_window.get(), d_frames, st);
  return e == hipSuccess ? GLFER_OK : hip_fail(e, "glfer_launch_prepare");
}

// The argument block both F entries start from: the packed kernel (it is the one with the spectrum output), one table per launch.
static void ftest_params(const glfer_hip_plan *p, SpectroParams &sp) {
  fill_params(p, sp);
  sp.pitch = p->bins;                    // (the statistic and the entries' scratch rows are dense)
  sp.npairs = 1;
  sp.nonlin = 0;
  sp.post_scale = sp.spec_unscale = 1.0f;
  sp.htaps = nullptr;
  sp.xtaps = sp.ltaps = sp.ytaps = nullptr;
}

// N >= 256, one launch: every round of spectro16_kernel's FT form transforms the frame under one taper (or two sequences, the
// paired form) and keeps what the statistic needs in registers (no spectrum goes through HBM).  sp: ftest_params with the stream set.
// d_psd (the rows-and-F entries): the multitaper rows of the same frames at the plan's pitch, from the same rounds (the ROWS forms).
static SpectroParams ftest_in_launch(const glfer_hip_plan *p, const SpectroParams &sp, size_t first, size_t nframes, float *d_ftest,
                                     int mu_live, float *d_psd = nullptr) {
  const int n = p->n, T = p->ntapers;
  SpectroParams q = sp;
  q.frame0 = (long long)first;
  q.nframes = (int)nframes;
  q.psd = d_psd;
  if (d_psd) {
    q.pitch = p->pitch;
    q.ft_cj = p->d_rows_cj;
  }
  q.spec = nullptr;
  q.ftest = d_ftest;
  q.ft_U0 = p->d_U0.get();
  q.ft_sum_U0_sqr = p->sum_U0_sqr;
  q.ft_mu_live = mu_live ? 1 : 0;
  q.npairs = mu_live ? T + 1 : T;                    // rounds: hn first (mu), then the tapers
  q.taps = mu_live ? p->d_ftaps_mu_first.get() : p->d_ftaps;
  // round 5: two sequences per transform, separated through the mirror bins (GLFER_FTEST_PAIRED=0: one per transform, for A/B runs and tests)
  // Measured (gpurun_out/r5/ftest_rate.txt): N = 4096, 5 tapers 39.2 against 33.5 M frames/s; N = 1024, 8 tapers 94.3 against 105.9 -- the
  // mirror exchange (two barriers, 16 LDS writes, 9 reads a round) costs a short transform more than it saves: paired from N = 2048.
  const char *pe = getenv("GLFER_FTEST_PAIRED");
  if (pe && *pe ? *pe != '0' : n >= 2048) {
    q.ft_nseq = mu_live ? T + 1 : T;
    q.npairs = (q.ft_nseq + 1) / 2;
    q.taps = mu_live ? p->d_ftaps2.get() : p->d_ftaps2_nomu;
    q.ft_mu_unscale = 1.0f / p->hn_scale;
  }
  return q;
}

// The harmonic F-test of mtm_do (mtm.c:165-174, 203-233) as an optional output of the multitaper
// path.  The tapered spectra y_j(f) and mu(f) come from the estimator's own spectrum output (one
// single-taper launch of spectro16_kernel per taper and one for hn), the statistic from a per-bin
// epilogue (stats_kernels.hip).  Frames are processed in groups that keep the spectra scratch
// under ~256 MiB.
static int ftest_single(glfer_hip_plan *p, const void *d_stream, size_t first, size_t nframes, float *d_psd, float *d_ftest,
                        int mu_live, hipStream_t st);

int glfer_hip_mtm_ftest_device(glfer_hip_plan *p, const void *d_stream, size_t nsamples, size_t first,
                               size_t nframes, float *d_ftest, int mu_live, void *hip_stream) {
  if (!p || !d_stream || (!d_ftest && nframes) || p->cfg.mode != GLFER_MODE_MTM) return GLFER_E_ARG;
  if (p->n > 16384) return GLFER_E_ARG;              // needs the packed form's spectrum output
  if (nframes == 0) return GLFER_OK;
  if ((first + nframes) > nsamples / (size_t)p->hop || nframes > 0x7fffffffu) return GLFER_E_ARG;
  return ftest_single(p, d_stream, first, nframes, nullptr, d_ftest, mu_live, (hipStream_t)hip_stream);
}

// The body of the single-stream F entries, arguments checked.  d_psd NULL: F alone (glfer_hip_mtm_ftest_device); else the multitaper
// rows of the same frames too, at the plan's pitch (glfer_hip_mtm_rows_ftest_device) -- from the same rounds of the same launch at
// N >= 256, from the same spectra in the per-bin epilogue below that.
static int ftest_single(glfer_hip_plan *p, const void *d_stream, size_t first, size_t nframes, float *d_psd, float *d_ftest,
                        int mu_live, hipStream_t st) {
  DeviceGuard guard(p->cfg.device);
  HIP_TRY(guard.error());
  const int n = p->n, T = p->ntapers;
  {
    const int trc = ftest_tables(p);
    if (trc != GLFER_OK) return trc;
  }
  SpectroParams sp;
  ftest_params(p, sp);
  sp.stream = d_stream;
  glfer::Scratch<float> copy(st);
  if (p->cfg.sub_mean) {
    sp.frame0 = (long long)first;
    if (const int rc = submean_scratch(p, sp, first, nframes, st, copy); rc != GLFER_OK) return rc;
  }
  if (n >= 256) {
    const SpectroParams q = ftest_in_launch(p, sp, first, nframes, d_ftest, mu_live, d_psd);
    const hipError_t e = launch_packed(q, n, st);
    return e == hipSuccess ? GLFER_OK : hip_fail(e, "ftest launch");
  }
  size_t group = ((size_t)256 << 20) / ((size_t)(T + 1) * n * sizeof(float));
  group = std::max<size_t>(1, std::min<size_t>(group, 32768));
  glfer::Scratch<float> spec(st), dummy(st);
  {
    const size_t g = std::min(group, nframes);
    hipError_t e = spec.take((size_t)(T + 1) * g * n);
    if (e == hipSuccess) e = dummy.take(g * (size_t)p->bins);
    if (e != hipSuccess) return hip_fail(e, "hipMallocAsync(ftest spectra)");
  }
  for (size_t done = 0; done < nframes; done += group) {
    const size_t g = std::min(group, nframes - done);
    hipError_t e = hipSuccess;
    for (int j = 0; j <= T && e == hipSuccess; j++) {
      if (j == T && !mu_live) break;     // mu is never written in the reference build (mtm.c:173)
      SpectroParams q = sp;
      q.frame0 = (long long)(first + done);
      q.nframes = (int)g;
      q.taps = p->d_ftaps + (size_t)j * 2 * n;
      q.psd = dummy.get();
      q.spec = spec.get() + (size_t)j * g * n;
      e = launch_packed(q, n, st);
    }
    if (e == hipSuccess && d_psd)
      e = glfer_launch_ftest_rows(spec.get(), g, n, T, p->d_U0.get(), p->sum_U0_sqr, mu_live ? 1 : 0, d_ftest + done * (size_t)p->bins,
                                  p->d_rows_cj, d_psd + done * (size_t)p->pitch, p->pitch, st);
    else if (e == hipSuccess)
      e = glfer_launch_ftest(spec.get(), g, n, T, p->d_U0.get(), p->sum_U0_sqr, mu_live ? 1 : 0, d_ftest + done * (size_t)p->bins, st);
    if (e != hipSuccess) return hip_fail(e, "ftest launch");
  }
  return GLFER_OK;
}

// glfer_hip_mtm_ftest_device over many streams (glfer_hip.h).  N >= 256: the launches of one stream -- the corrected copies under
// mean removal (submean_scratch), then spectro16_kernel's FT form with blockIdx.y as the stream, the form chosen as the
// single entry chooses it -- so the launch count does not grow with the batch; below 256 the single entry, stream by stream.
// (The multitaper rows and F from one pass over the samples: glfer_hip_mtm_rows_ftest_device / _batch_device below, the same bodies.)
static int ftest_batch(glfer_hip_plan *p, const void *d_streams, size_t nstreams, size_t stream_pitch, size_t first, size_t nframes,
                       float *d_psd, float *d_ftest, int mu_live, hipStream_t st);

// The batched F entries' argument checks, in the order glfer_hip.h states.  want_psd: the rows-and-F entry (both outputs required;
// its PSD rows lie at the plan's pitch, the wider of the two row sizes).
static int ftest_batch_args(const glfer_hip_plan *p, const void *d_streams, size_t nstreams, size_t stream_pitch, size_t nsamples,
                            size_t first, size_t nframes, const float *d_psd, bool want_psd, const float *d_ftest, bool *empty) {
  *empty = false;
  if (!p) return GLFER_E_ARG;
  if (p->cfg.mode != GLFER_MODE_MTM || p->n > 16384) return GLFER_E_ARG;
  if (nstreams == 0 || nframes == 0) {
    *empty = true;
    return GLFER_OK;
  }
  if (!d_streams || !d_ftest || (want_psd && !d_psd)) return GLFER_E_ARG;
  if ((first + nframes) > nsamples / (size_t)p->hop) return GLFER_E_ARG;   // frame past the stream
  if (nframes > 0x7fffffffu) return GLFER_E_ARG;
  const int fmt = p->cfg.sample_format;
  const size_t esz = glfer_sample_size(fmt);
  // (as glfer_hip_spectrogram_batch_device: every stream of a batch must see the same alignment)
  if (fmt != GLFER_FMT_F32 && (stream_pitch & 1)) return GLFER_E_ARG;
  const size_t rows = want_psd ? (size_t)p->pitch : (size_t)p->bins;
  if (stream_pitch > (SIZE_MAX / esz) / nstreams || nframes > (SIZE_MAX / sizeof(float) / rows) / nstreams) return GLFER_E_ARG;
  return GLFER_OK;
}

int glfer_hip_mtm_ftest_batch_device(glfer_hip_plan *p, const void *d_streams, size_t nstreams, size_t stream_pitch,
                                     size_t nsamples, size_t first, size_t nframes, float *d_ftest, int mu_live,
                                     void *hip_stream) {
  bool empty = false;
  const int rc = ftest_batch_args(p, d_streams, nstreams, stream_pitch, nsamples, first, nframes, nullptr, false, d_ftest, &empty);
  if (rc != GLFER_OK || empty) return rc;
  return ftest_batch(p, d_streams, nstreams, stream_pitch, first, nframes, nullptr, d_ftest, mu_live, (hipStream_t)hip_stream);
}

// The multitaper rows and the F rows of the same frames from one pass over the samples (glfer_hip.h).
int glfer_hip_mtm_rows_ftest_device(glfer_hip_plan *p, const void *d_stream, size_t nsamples, size_t first, size_t nframes,
                                    float *d_psd, float *d_ftest, int mu_live, void *hip_stream) {
  bool empty = false;
  const int rc = ftest_batch_args(p, d_stream, 1, 0, nsamples, first, nframes, d_psd, true, d_ftest, &empty);
  if (rc != GLFER_OK || empty) return rc;
  return ftest_single(p, d_stream, first, nframes, d_psd, d_ftest, mu_live, (hipStream_t)hip_stream);
}

int glfer_hip_mtm_rows_ftest_batch_device(glfer_hip_plan *p, const void *d_streams, size_t nstreams, size_t stream_pitch,
                                          size_t nsamples, size_t first, size_t nframes, float *d_psd, float *d_ftest, int mu_live,
                                          void *hip_stream) {
  bool empty = false;
  const int rc = ftest_batch_args(p, d_streams, nstreams, stream_pitch, nsamples, first, nframes, d_psd, true, d_ftest, &empty);
  if (rc != GLFER_OK || empty) return rc;
  return ftest_batch(p, d_streams, nstreams, stream_pitch, first, nframes, d_psd, d_ftest, mu_live, (hipStream_t)hip_stream);
}

// The body of the batched F entries, arguments checked.  d_psd NULL: F alone; else stream b's multitaper rows at
// d_psd + b * nframes * pitch beside its F rows, from the same launch (the ROWS forms carry a PSD stride next to the F stride).
static int ftest_batch(glfer_hip_plan *p, const void *d_streams, size_t nstreams, size_t stream_pitch, size_t first, size_t nframes,
                       float *d_psd, float *d_ftest, int mu_live, hipStream_t st) {
  const int fmt = p->cfg.sample_format;
  const size_t esz = glfer_sample_size(fmt);
  const char *base = static_cast<const char *>(d_streams);
  const size_t ft_bs = nframes * (size_t)p->bins;            // floats from one stream's first F row to the next one's
  const size_t psd_bs = nframes * (size_t)p->pitch;          // and from one stream's first PSD row to the next one's
  const int n = p->n;
  if (n < 256 || nstreams == 1) {
    for (size_t b = 0; b < nstreams; b++) {
      const int rc = ftest_single(p, base + b * stream_pitch * esz, first, nframes, d_psd ? d_psd + b * psd_bs : nullptr,
                                  d_ftest + b * ft_bs, mu_live, st);
      if (rc != GLFER_OK) return rc;
    }
    return GLFER_OK;
  }
  DeviceGuard guard(p->cfg.device);
  HIP_TRY(guard.error());
  {
    const int trc = ftest_tables(p);
    if (trc != GLFER_OK) return trc;
  }
  size_t ymax = 0;
  if (const int yrc = grid_y_limit(1, &ymax); yrc != GLFER_OK) return yrc;
  for (size_t c0 = 0; c0 < nstreams; c0 += ymax) {      // batches above the grid's y limit: chunks of it
    const unsigned nb = (unsigned)std::min(nstreams - c0, ymax);
    SpectroParams sp;
    ftest_params(p, sp);
    sp.stream = base + c0 * stream_pitch * esz;
    sp.nbatch = (int)nb;
    sp.batch_stride = (long long)(stream_pitch * esz);
    glfer::Scratch<float> copy(st);
    if (p->cfg.sub_mean) {
      sp.frame0 = (long long)first;
      if (const int rc = submean_scratch(p, sp, first, nframes, st, copy); rc != GLFER_OK) return rc;
    }
    SpectroParams q = ftest_in_launch(p, sp, first, nframes, d_ftest + c0 * ft_bs, mu_live, d_psd ? d_psd + c0 * psd_bs : nullptr);
    q.ftest_batch_stride = (long long)ft_bs;                  // (F alone: psd NULL, psd_batch_stride 0)
    if (d_psd) q.psd_batch_stride = (long long)psd_bs;
    const hipError_t e = launch_packed(q, n, st);
    if (e != hipSuccess) return hip_fail(e, "ftest launch (batch)");
  }
  return GLFER_OK;
}

// The F entries over streams of unequal length (glfer_hip.h): the launches of ftest_batch with a table in place of the strides.
// One chunk (2 <= nb <= the grid's y limit, c.d_psd NULL: F alone): every frame of an F entry goes through corrected copies under
// mean removal, so the copies of hops [0, frames_b) of every stream come from one RaggedChunk::submean -- no head / body / tail --
// and one launch of the FT form follows, the form chosen by ftest_in_launch.  d_ftest: the call's; the plan's F tables are made.
static int ftest_ragged_chunk(const RaggedChunk &c, float *d_ftest, int mu_live) {
  glfer_hip_plan *p = c.p;
  SpectroParams sp;
  ftest_params(p, sp);
  sp.stream = c.base;
  std::vector<long long> soff(c.nb);
  glfer::Scratch<float> copy(c.st);
  if (p->cfg.sub_mean) {
    std::vector<size_t> hlo(c.nb, 0), hhi(c.nb);
    for (unsigned b = 0; b < c.nb; b++) hhi[b] = c.s[b].frames;
    const int rc = c.submean(sp.fmt, hlo, hhi, copy, soff);
    if (rc != GLFER_OK || !copy) return rc;              // (no copy: no stream of the chunk has a frame)
    sp.stream = copy.get();
    sp.fmt = GLFER_FMT_F32;
  } else {
    for (unsigned b = 0; b < c.nb; b++) soff[b] = (long long)(c.s[b].off * c.esz);
  }
  const SpectroParams q = ftest_in_launch(p, sp, 0, 0, d_ftest, mu_live, c.d_psd);
  std::vector<GlferRaggedEntry> tab(c.nb);
  for (unsigned b = 0; b < c.nb; b++) {
    GlferRaggedEntry e = {};
    if (c.s[b].frames) {
      e.stream_off = soff[b];
      e.psd_off = c.d_psd ? (long long)(c.s[b].row * (size_t)p->pitch) : 0;   // (F alone: psd NULL stays NULL in the kernel)
      e.ftest_off = (long long)(c.s[b].row * (size_t)p->bins);
      e.nframes = (int)c.s[b].frames;
    }
    tab[b] = e;
  }
  return c.launch(q, tab, ROUTE_PACKED);
}

// both ragged F entries; want_psd: the rows-and-F one (d_psd required, its rows at the plan's pitch)
static int ftest_ragged(glfer_hip_plan *p, const void *d_samples, size_t nstreams, const size_t *offsets, const size_t *lengths,
                        float *d_psd, bool want_psd, float *d_ftest, int mu_live, size_t *row_starts, hipStream_t st) {
  if (!p) return GLFER_E_ARG;
  if (p->cfg.mode != GLFER_MODE_MTM || p->n > 16384) return GLFER_E_ARG;
  if (nstreams == 0) {
    if (row_starts) row_starts[0] = 0;
    return GLFER_OK;
  }
  if (!offsets || !lengths) return GLFER_E_ARG;
  const int fmt = p->cfg.sample_format;
  const size_t esz = glfer_sample_size(fmt);
  const size_t rowlen = want_psd ? (size_t)p->pitch : (size_t)p->bins;    // (the wider of the two row sizes: pitch >= bins)
  // glfer_hip_spectrogram_ragged_device's per-stream rules, from the host arrays alone
  std::vector<RaggedStream> s(nstreams);
  size_t total = 0;
  for (size_t b = 0; b < nstreams; b++) {
    const size_t f = lengths[b] / (size_t)p->hop;
    if (f > 0x7fffffffu) return GLFER_E_ARG;
    if (lengths[b] > SIZE_MAX / esz || offsets[b] > SIZE_MAX / esz - lengths[b]) return GLFER_E_ARG;
    if (fmt != GLFER_FMT_F32 && (offsets[b] & 1)) return GLFER_E_ARG;   // (every stream of a launch must see the same alignment)
    if (f > SIZE_MAX / sizeof(float) / rowlen - total) return GLFER_E_ARG;
    s[b] = RaggedStream{offsets[b], f, total};
    total += f;
  }
  if (row_starts) {
    for (size_t b = 0; b < nstreams; b++) row_starts[b] = s[b].row;
    row_starts[nstreams] = total;
  }
  if (total == 0) return GLFER_OK;
  if (!d_samples || !d_ftest || (want_psd && !d_psd)) return GLFER_E_ARG;
  // (the tables are uploaded from host memory that is gone when the call returns: glfer_hip_spectrogram_ragged_device)
  if (glfer::stream_is_capturing(st)) return GLFER_E_ARG;
  if (!want_psd) d_psd = nullptr;
  const char *base = static_cast<const char *>(d_samples);
  auto single = [&](size_t b) {
    if (!s[b].frames) return (int)GLFER_OK;
    return ftest_single(p, base + s[b].off * esz, 0, s[b].frames, d_psd ? d_psd + s[b].row * (size_t)p->pitch : nullptr,
                        d_ftest + s[b].row * (size_t)p->bins, mu_live, st);
  };
  if (p->n < 256 || nstreams == 1) {
    for (size_t b = 0; b < nstreams; b++) {
      const int rc = single(b);
      if (rc != GLFER_OK) return rc;
    }
    return GLFER_OK;
  }
  DeviceGuard guard(p->cfg.device);
  HIP_TRY(guard.error());
  {
    const int trc = ftest_tables(p);
    if (trc != GLFER_OK) return trc;
  }
  size_t ymax = 0;
  if (const int yrc = grid_y_limit(2, &ymax); yrc != GLFER_OK) return yrc;
  for (size_t c0 = 0; c0 < nstreams; c0 += ymax) {      // above the grid's y limit: chunks of it
    const unsigned nb = (unsigned)std::min(nstreams - c0, ymax);
    int rc;
    if (nb == 1) {
      rc = single(c0);
    } else {
      const RaggedChunk c{p, s.data() + c0, nb, base, d_psd, st, esz, 0};   // (esz: the raw samples'; first_inside is not used)
      rc = ftest_ragged_chunk(c, d_ftest, mu_live);
    }
    if (rc != GLFER_OK) return rc;
  }
  return GLFER_OK;
}

int glfer_hip_mtm_ftest_ragged_device(glfer_hip_plan *p, const void *d_samples, size_t nstreams, const size_t *offsets,
                                      const size_t *lengths, float *d_ftest, int mu_live, size_t *row_starts, void *hip_stream) {
  return ftest_ragged(p, d_samples, nstreams, offsets, lengths, nullptr, false, d_ftest, mu_live, row_starts, (hipStream_t)hip_stream);
}

int glfer_hip_mtm_rows_ftest_ragged_device(glfer_hip_plan *p, const void *d_samples, size_t nstreams, const size_t *offsets,
                                           const size_t *lengths, float *d_psd, float *d_ftest, int mu_live, size_t *row_starts,
                                           void *hip_stream) {
  return ftest_ragged(p, d_samples, nstreams, offsets, lengths, d_psd, true, d_ftest, mu_live, row_starts, (hipStream_t)hip_stream);
}

int glfer_hip_submean_device(const void *d_in, float *d_out, int hop, size_t nhops, int sample_format,
                             void *hip_stream) {
  if (!d_in || !d_out || hop < 1 || sample_format < 0 || sample_format > 2) return GLFER_E_ARG;
  DeviceGuard guard(data_device(d_out));
  HIP_TRY(guard.error());
  HIP_TRY(glfer_launch_submean(d_in, d_out, hop, (long long)nhops, sample_format, (hipStream_t)hip_stream, nullptr));
  return GLFER_OK;
}

// The same with every hop summed in the reference's own order (fft.c:88-92; submean_seq.hip).
int glfer_hip_submean_exact_device(const void *d_in, float *d_out, int hop, size_t nhops, int sample_format,
                                   void *hip_stream) {
  if (!d_in || !d_out || hop < 1 || sample_format < 0 || sample_format > 2) return GLFER_E_ARG;
  if (nhops == 0) return GLFER_OK;
  hipStream_t st = (hipStream_t)hip_stream;
  DeviceGuard guard(data_device(d_out));
  HIP_TRY(guard.error());
  glfer::Scratch<float> means(st);
  HIP_TRY(means.take(nhops));
  hipError_t e = glfer_launch_hop_means_seq(d_in, means.get(), hop, (long long)nhops, sample_format, st);
  if (e == hipSuccess) e = glfer_launch_submean(d_in, d_out, hop, (long long)nhops, sample_format, st, means.get());
  return e == hipSuccess ? GLFER_OK : hip_fail(e, "glfer_hip_submean_exact_device");
}

int glfer_hip_floor_device_pitched(const float *d_psd, size_t nframes, int bins, int pitch, float *d_stats, void *hip_stream) {
  if (!d_psd || !d_stats || bins < 1 || bins > 32769 || pitch < bins) return GLFER_E_ARG;
  DeviceGuard guard(data_device(d_psd));
  HIP_TRY(guard.error());
  HIP_TRY(glfer::floor_rows(d_psd, nframes, bins, pitch, d_stats, (hipStream_t)hip_stream));
  return GLFER_OK;
}

int glfer_hip_floor_device(const float *d_psd, size_t nframes, int bins, float *d_stats, void *hip_stream) {
  return glfer_hip_floor_device_pitched(d_psd, nframes, bins, bins, d_stats, hip_stream);
}

int glfer_hip_avg_device(int avg_mode, const float *d_psd, size_t nframes, int bins, int n_out, int depth,
                         int minbin, int maxbin, int max0, double *d_avg, double *d_ret, void *hip_stream) {
  if (!d_psd || !d_avg || !d_ret) return GLFER_E_ARG;
  if (!glfer::update_avg_args_ok(avg_mode, depth, minbin, maxbin, bins, n_out)) return GLFER_E_ARG;
  DeviceGuard guard(data_device(d_psd));
  HIP_TRY(guard.error());
  HIP_TRY(glfer_launch_avg(avg_mode, d_psd, nframes, bins, n_out, depth, minbin, maxbin, max0 ? 1 : 0, d_avg,
                           d_ret, (hipStream_t)hip_stream));
  return GLFER_OK;
}

// The route of glfer_hip_spectrogram_avg_device (and of every stream of glfer_hip_spectrogram_avg_batch_device): true where the
// average is taken inside the estimator launch for frames [*b0, first + nframes) -- the frames before *b0 then take the two
// launches --, false where the whole call takes them.  sp: the call's parameters (the stream's alignment picks the form).
static bool avg_in_launch(const glfer_hip_plan *p, const SpectroParams &sp, int avg_mode, int depth, int n_out, size_t first,
                          size_t nframes, size_t *b0) {
  static const bool fused_off = [] { const char *e = getenv("GLFER_AVG_FUSED"); return e && *e == '0'; }();   // (A/B runs and the tests that compare the two)
  // mean removal: off, or the reference's own (cfg.sub_mean = 1: the means are taken first, in its summation order, and given to the kernel)
  // where the hop is 2, 4, 8 or 16 sixteenths of the block; the in-kernel sums (GLFER_SUBMEAN_FAST) take the two launches
  const bool with_means = p->cfg.sub_mean != 0;
  const bool fused = !fused_off && avg_mode == GLFER_AVG_PLAIN && depth <= 4 && p->cfg.mode == GLFER_MODE_FFT && !p->nonlin &&
                     !p->cfg.history_mode && p->n >= 512 && p->n <= 4096 && n_out <= 2 * p->n && body_route(sp, p->n) == ROUTE_REAL_INPUT &&
                     (!with_means || (reference_means(p) && route_takes_mean(ROUTE_REAL_INPUT, sp, p->n) && !getenv("GLFER_MEAN_PREPASS")));
  // the first frame every one of whose depth-1 predecessors lies inside the stream AND inside this call's averaging state
  const size_t end = first + nframes;
  // (G = 1: the cut's b0 is the call's first frame inside the stream -- or `end` when it has none, and the test below fails)
  *b0 = glfer_cut_frames(first, end, plan_first_inside(p), 1).b0 + (size_t)(depth - 1);
  return fused && *b0 + 256 <= end;                       // (short calls: the lead frames of every slot would outweigh the rest)
}

// fft_do + fft_psd + update_avg_* for a batch of frames in ONE call (source.c:141-158 followed by g_main.c:1153-1183).  Where the
// periodogram's real-input kernel applies -- FFT mode, N = 512 .. 4096, no RA9MB / limiter, no mean removal, history from the
// stream, dense rows -- and the average is the plain one over a window of at most four frames (glfer.c:295-296: the default
// depth is 4), the average is taken INSIDE the estimator launch on the PSD values in registers (spectro16h.hip AVG): no PSD row
// goes to memory unless d_psd asks for it.  The frames up to the first one with a full window behind it inside the stream (at
// most ceil((N-H)/H) + depth - 1 of them) and every other configuration take the two launches (rows, then avg_fused_kernel).
int glfer_hip_spectrogram_avg_device(glfer_hip_plan *p, const void *d_stream, size_t nsamples, size_t first, size_t nframes,
                                     int avg_mode, int depth, int minbin, int maxbin, int max0, int n_out, float *d_psd,
                                     double *d_avg, double *d_ret, void *hip_stream) {
  if (!p || !d_stream || (!d_avg && nframes)) return GLFER_E_ARG;
  if (p->cfg.mode == GLFER_MODE_HPARMA || p->pitch != p->bins) return GLFER_E_ARG;       // (HP-ARMA rows are not averaged by the reference's callers; rows dense)
  if (!glfer::update_avg_args_ok(avg_mode, depth, minbin, maxbin, p->bins, n_out) || n_out < p->bins) return GLFER_E_ARG;
  if (nframes == 0) return GLFER_OK;
  if ((first + nframes) > nsamples / (size_t)p->hop || nframes > 0x7fffffffu) return GLFER_E_ARG;
  hipStream_t st = (hipStream_t)hip_stream;
  DeviceGuard guard(p->cfg.device);
  HIP_TRY(guard.error());
  const size_t bins = (size_t)p->bins;
  // frames [from, to): the rows (to d_psd, or scratch), then update_avg over them with the state empty at `from`
  auto two_launches = [&](size_t from, size_t to) -> int {
    if (from >= to) return GLFER_OK;
    const size_t nf = to - from;
    glfer::Scratch<float> rows_buf(st);
    glfer::Scratch<double> ret_buf(st);
    hipError_t e = hipSuccess;
    if (!d_psd) e = rows_buf.take(nf * bins);
    if (e == hipSuccess && !d_ret) e = ret_buf.take(nf * 4);
    if (e != hipSuccess) return hip_fail(e, "scratch (rows to average)");
    float *rows = d_psd ? d_psd + (from - first) * bins : rows_buf.get();
    double *ret = d_ret ? d_ret + (from - first) * 4 : ret_buf.get();
    if (const int rc = glfer_run_device(p, d_stream, nsamples, from, nf, rows, nullptr, st); rc != GLFER_OK) return rc;
    e = glfer_launch_avg(avg_mode, rows, nf, (int)bins, n_out, depth, minbin, maxbin, max0 ? 1 : 0, d_avg + (from - first) * (size_t)n_out, ret, st);
    return e == hipSuccess ? GLFER_OK : hip_fail(e, "update_avg launch");
  };
  SpectroParams sp;
  fill_params(p, sp);
  sp.stream = d_stream;
  sp.frame0 = (long long)first;
  sp.nframes = (int)nframes;
  const bool with_means = p->cfg.sub_mean != 0;
  const size_t end = first + nframes;
  size_t b0 = end;
  if (!avg_in_launch(p, sp, avg_mode, depth, n_out, first, nframes, &b0)) return two_launches(first, end);
  // The head's state starts empty at `first`, like the whole call's.  Its rows are also what the body's first slots would need
  // in front of them -- they recompute them instead (frames >= b0 - (depth-1) >= first_inside are all computable).
  if (const int rc = two_launches(first, b0); rc != GLFER_OK) return rc;
  const size_t piece = (size_t)1 << 24;                     // frames per launch: keeps a workgroup's rows under the 4 GiB of a buffer descriptor
  // (the kernel always forms the return values -- one code path, no branch per bin: without d_ret they land in scratch)
  glfer::Scratch<double> ret_scratch(st);
  if (!d_ret) {
    hipError_t e = ret_scratch.take(std::min(piece, end - b0) * 4);
    if (e != hipSuccess) return hip_fail(e, "scratch (return values)");
  }
  // the hop means of everything the body touches: its frames, the depth-1 frames a slot recomputes in front of them, their history
  glfer::Scratch<float> means(st);
  const glfer_hop_span mh = glfer_means_hops(b0, end, (size_t)(depth - 1), plan_first_inside(p));
  if (with_means) {
    hipError_t e = means.take(mh.n);
    if (e == hipSuccess) e = launch_reference_means(p, sp, mh.lo, mh.n, means.get(), 0, st);
    if (e != hipSuccess) return hip_fail(e, "hop means (average inside the kernel)");
  }
  for (size_t f0 = b0; f0 < end; f0 += piece) {
    const size_t nf = std::min(piece, end - f0);
    SpectroParams q = sp;
    if (with_means) {
      q.mean_inkernel = 1;
      q.means = means.get() - mh.lo;                         // indexed by GLOBAL hop (= frame) index
    }
    q.frame0 = (long long)f0;
    q.nframes = (int)nf;
    q.psd = d_psd ? d_psd + (f0 - first) * bins : nullptr;
    q.avg = d_avg + (f0 - first) * (size_t)n_out;
    q.avg_ret = d_ret ? d_ret + (f0 - first) * 4 : ret_scratch.get();
    q.avg_depth = depth;
    q.avg_minbin = minbin;
    q.avg_maxbin = maxbin;
    q.avg_nout = n_out;
    hipError_t e = launch_real_input(q, p->n, st);
    if (e != hipSuccess) return hip_fail(e, "estimator launch (average inside the kernel)");
  }
  return GLFER_OK;
}

int glfer_hip_avg_batch_device(int avg_mode, const float *d_psd, size_t nstreams, size_t nframes, int bins, int n_out, int depth,
                               int minbin, int maxbin, int max0, double *d_avg, double *d_ret, void *hip_stream) {
  if (!glfer::update_avg_args_ok(avg_mode, depth, minbin, maxbin, bins, n_out)) return GLFER_E_ARG;
  if (nstreams == 0 || nframes == 0) return GLFER_OK;
  if (!d_psd || !d_avg || !d_ret) return GLFER_E_ARG;
  if (nframes > (SIZE_MAX / sizeof(double) / (size_t)std::max(bins, n_out)) / nstreams) return GLFER_E_ARG;
  DeviceGuard guard(data_device(d_psd));
  HIP_TRY(guard.error());
  const size_t chunk = 65535;                                    // streams per launch: the grid's y (z) limit
  for (size_t c0 = 0; c0 < nstreams; c0 += chunk) {
    const unsigned nb = (unsigned)std::min(nstreams - c0, chunk);
    HIP_TRY(glfer_launch_avg_batch(avg_mode, d_psd + c0 * nframes * (size_t)bins, nframes, bins, n_out, depth, minbin, maxbin,
                                   max0 ? 1 : 0, d_avg + c0 * nframes * (size_t)n_out, d_ret + c0 * nframes * 4, nb,
                                   (long long)(nframes * (size_t)bins), (long long)(nframes * (size_t)n_out), (long long)(nframes * 4),
                                   (hipStream_t)hip_stream));
  }
  return GLFER_OK;
}

// glfer_hip_spectrogram_avg_device over many streams (glfer_hip.h).  The route is that entry's for one stream (avg_in_launch: the
// streams differ only by a multiple of an even pitch, so every stream would get the same one); each launch it produces -- the
// rows (batch_rows), the average over them (glfer_launch_avg_batch), the estimator with the average inside it -- covers the
// whole batch (blockIdx.y), with the frames of each stream cut exactly as the single-stream entry cuts them.
int glfer_hip_spectrogram_avg_batch_device(glfer_hip_plan *p, const void *d_streams, size_t nstreams, size_t stream_pitch,
                                           size_t nsamples, size_t first, size_t nframes, int avg_mode, int depth, int minbin,
                                           int maxbin, int max0, int n_out, float *d_psd, double *d_avg, double *d_ret,
                                           void *hip_stream) {
  if (!p) return GLFER_E_ARG;
  if (p->cfg.mode == GLFER_MODE_HPARMA || p->pitch != p->bins) return GLFER_E_ARG;
  if (!glfer::update_avg_args_ok(avg_mode, depth, minbin, maxbin, p->bins, n_out) || n_out < p->bins) return GLFER_E_ARG;
  const int fmt = p->cfg.sample_format;
  if (fmt != GLFER_FMT_F32 && (stream_pitch & 1)) return GLFER_E_ARG;      // (glfer_hip_spectrogram_batch_device's rule)
  if (nstreams == 0 || nframes == 0) return GLFER_OK;
  if (!d_streams || !d_avg) return GLFER_E_ARG;
  if ((first + nframes) > nsamples / (size_t)p->hop || nframes > 0x7fffffffu) return GLFER_E_ARG;
  const size_t esz = glfer_sample_size(fmt);
  const size_t bins = (size_t)p->bins;
  if (stream_pitch > (SIZE_MAX / esz) / nstreams || nframes > (SIZE_MAX / sizeof(double) / (size_t)n_out) / nstreams) return GLFER_E_ARG;
  hipStream_t st = (hipStream_t)hip_stream;
  DeviceGuard guard(p->cfg.device);
  HIP_TRY(guard.error());
  const char *base = static_cast<const char *>(d_streams);
  const size_t end = first + nframes;
  SpectroParams sp;
  fill_params(p, sp);
  sp.stream = base;
  sp.frame0 = (long long)first;
  sp.nframes = (int)nframes;
  size_t b0 = end;
  const bool in_launch = avg_in_launch(p, sp, avg_mode, depth, n_out, first, nframes, &b0);
  const bool with_means = p->cfg.sub_mean != 0;
  // streams per group: the grid's y limit, and rows that go to scratch (no d_psd) kept under 8 GiB a group (4 096 one-second
  // C2 streams take 1.5 GiB: one group)
  const size_t scratch_frames = in_launch ? b0 - first : nframes;
  size_t group = 65535;
  if (!d_psd && scratch_frames > 0)
    group = std::max<size_t>(1, std::min(group, ((size_t)8 << 30) / (scratch_frames * bins * sizeof(float))));
  for (size_t c0 = 0; c0 < nstreams; c0 += group) {
    const unsigned nb = (unsigned)std::min(nstreams - c0, group);
    const char *sbase = base + c0 * stream_pitch * esz;
    float *psd_c = d_psd ? d_psd + c0 * nframes * bins : nullptr;
    double *avg_c = d_avg + c0 * nframes * (size_t)n_out, *ret_c = d_ret ? d_ret + c0 * nframes * 4 : nullptr;
    // frames [from, to) of every stream of the group: the rows (to d_psd, or scratch), then update_avg over them with the state
    // empty at `from`
    auto two_launches = [&](size_t from, size_t to) -> int {
      if (from >= to) return GLFER_OK;
      const size_t nf = to - from;
      const size_t rows_bs = psd_c ? nframes * bins : nf * bins, ret_bs = ret_c ? nframes * 4 : nf * 4;
      glfer::Scratch<float> rows_buf(st);
      glfer::Scratch<double> ret_buf(st);
      hipError_t e = hipSuccess;
      if (!psd_c) e = rows_buf.take((size_t)nb * nf * bins);
      if (e == hipSuccess && !ret_c) e = ret_buf.take((size_t)nb * nf * 4);
      if (e != hipSuccess) return hip_fail(e, "scratch (rows to average, batch)");
      float *rows = psd_c ? psd_c + (from - first) * bins : rows_buf.get();
      double *ret = ret_c ? ret_c + (from - first) * 4 : ret_buf.get();
      if (const int rc = batch_rows(p, sbase, nb, stream_pitch, nsamples, from, nf, rows, rows_bs, st); rc != GLFER_OK) return rc;
      e = glfer_launch_avg_batch(avg_mode, rows, nf, (int)bins, n_out, depth, minbin, maxbin, max0 ? 1 : 0,
                                 avg_c + (from - first) * (size_t)n_out, ret, nb, (long long)rows_bs,
                                 (long long)(nframes * (size_t)n_out), (long long)ret_bs, st);
      return e == hipSuccess ? GLFER_OK : hip_fail(e, "update_avg launch (batch)");
    };
    if (const int rc = two_launches(first, in_launch ? b0 : end); rc != GLFER_OK) return rc;
    if (!in_launch) continue;
    const size_t piece = (size_t)1 << 24;                   // frames per launch, as the single-stream entry cuts them
    const size_t ret_rows = std::min(piece, end - b0);
    glfer::Scratch<double> ret_scratch(st);
    if (!ret_c) {
      hipError_t e = ret_scratch.take((size_t)nb * ret_rows * 4);
      if (e != hipSuccess) return hip_fail(e, "scratch (return values, batch)");
    }
    // the hop means of everything the body touches, one table per stream: its frames, the depth-1 frames a slot recomputes in
    // front of them, their history
    glfer::Scratch<float> means(st);
    const glfer_hop_span mh = glfer_means_hops(b0, end, (size_t)(depth - 1), plan_first_inside(p));
    const size_t hop_lo = mh.lo, nhops = mh.n;
    if (with_means) {
      hipError_t e = means.take((size_t)nb * nhops);
      if (e == hipSuccess)
        e = glfer_launch_hop_means_seq_batch(sbase + hop_lo * (size_t)p->hop * esz, means.get(), p->hop, (long long)nhops, fmt, nb,
                                             (long long)(stream_pitch * esz), (long long)nhops, st);
      if (e != hipSuccess) return hip_fail(e, "hop means (average inside the kernel, batch)");
    }
    for (size_t f0 = b0; f0 < end; f0 += piece) {
      const size_t nf = std::min(piece, end - f0);
      SpectroParams q = sp;
      q.stream = sbase;
      q.nbatch = (int)nb;
      q.batch_stride = (long long)(stream_pitch * esz);
      if (with_means) {
        q.mean_inkernel = 1;
        q.means = means.get() - hop_lo;                        // indexed by the stream's own hop (= frame) index
        q.means_batch_stride = (long long)nhops;
      }
      q.frame0 = (long long)f0;
      q.nframes = (int)nf;
      q.psd = psd_c ? psd_c + (f0 - first) * bins : nullptr;
      q.psd_batch_stride = psd_c ? (long long)(nframes * bins) : 0;    // (0: psd stays NULL in every stream)
      q.avg = avg_c + (f0 - first) * (size_t)n_out;
      q.avg_batch_stride = (long long)(nframes * (size_t)n_out);
      q.avg_ret = ret_c ? ret_c + (f0 - first) * 4 : ret_scratch.get();
      q.avg_ret_batch_stride = (long long)(ret_c ? nframes * 4 : ret_rows * 4);
      q.avg_depth = depth;
      q.avg_minbin = minbin;
      q.avg_maxbin = maxbin;
      q.avg_nout = n_out;
      hipError_t e = launch_real_input(q, p->n, st);
      if (e != hipSuccess) return hip_fail(e, "estimator launch (average inside the kernel, batch)");
    }
  }
  return GLFER_OK;
}

// update_avg_* over packed rows of streams of unequal length (glfer_hip.h): glfer_launch_avg_ragged over the streams that have rows
int glfer_hip_avg_ragged_device(int avg_mode, const float *d_psd, size_t nstreams, const size_t *row_starts, int bins, int n_out,
                                int depth, int minbin, int maxbin, int max0, double *d_avg, double *d_ret, void *hip_stream) {
  if (!glfer::update_avg_args_ok(avg_mode, depth, minbin, maxbin, bins, n_out)) return GLFER_E_ARG;
  if (nstreams == 0) return GLFER_OK;
  if (!row_starts || !glfer::ragged_rows_ok(row_starts, nstreams)) return GLFER_E_ARG;
  const size_t rows_hi = row_starts[nstreams];
  if (rows_hi > SIZE_MAX / sizeof(double) / (size_t)std::max(bins, n_out)) return GLFER_E_ARG;
  if (rows_hi == row_starts[0]) return GLFER_OK;
  if (!d_psd || !d_avg) return GLFER_E_ARG;
  hipStream_t st = (hipStream_t)hip_stream;
  if (glfer::stream_is_capturing(st)) return GLFER_E_ARG;
  DeviceGuard guard(data_device(d_psd));
  HIP_TRY(guard.error());
  const std::vector<glfer::RaggedColsEntry> s = glfer::ragged_streams(row_starts, nstreams);
  glfer::Scratch<double> ret(st);                        // (the kernels always form the return values: without d_ret they land in scratch)
  if (!d_ret) HIP_TRY(ret.take(rows_hi * 4));
  const hipError_t e = glfer_launch_avg_ragged(avg_mode, d_psd, s.data(), s.size(), bins, n_out, depth, minbin, maxbin, max0 ? 1 : 0, d_avg,
                                               d_ret ? d_ret : ret.get(), st);
  return e == hipSuccess ? GLFER_OK : hip_fail(e, "update_avg launch (ragged)");
}

// The ragged rows, then the ragged average over them: the two-launch route of glfer_hip_spectrogram_avg_device, stream by stream
// (glfer_hip.h; the average inside the estimator launch is not built for ragged calls).
int glfer_hip_spectrogram_avg_ragged_device(glfer_hip_plan *p, const void *d_samples, size_t nstreams, const size_t *offsets,
                                            const size_t *lengths, int avg_mode, int depth, int minbin, int maxbin, int max0,
                                            int n_out, float *d_psd, double *d_avg, double *d_ret, size_t *row_starts,
                                            void *hip_stream) {
  if (!p) return GLFER_E_ARG;
  if (p->cfg.mode == GLFER_MODE_HPARMA || p->pitch != p->bins) return GLFER_E_ARG;       // (glfer_hip_spectrogram_avg_device's rules)
  if (!glfer::update_avg_args_ok(avg_mode, depth, minbin, maxbin, p->bins, n_out) || n_out < p->bins) return GLFER_E_ARG;
  if (nstreams == 0) {
    if (row_starts) row_starts[0] = 0;
    return GLFER_OK;
  }
  if (!offsets || !lengths || nstreams > 0x7fffffffu) return GLFER_E_ARG;
  // glfer_hip_spectrogram_ragged_device's rules, before scratch is taken for its rows
  const int fmt = p->cfg.sample_format;
  const size_t esz = glfer_sample_size(fmt), bins = (size_t)p->bins;
  std::vector<size_t> starts(nstreams + 1);
  size_t total = 0;
  for (size_t b = 0; b < nstreams; b++) {
    const size_t f = lengths[b] / (size_t)p->hop;
    if (f > 0x7fffffffu) return GLFER_E_ARG;
    if (lengths[b] > SIZE_MAX / esz || offsets[b] > SIZE_MAX / esz - lengths[b]) return GLFER_E_ARG;
    if (fmt != GLFER_FMT_F32 && (offsets[b] & 1)) return GLFER_E_ARG;
    if (f > SIZE_MAX / sizeof(double) / (size_t)n_out - total) return GLFER_E_ARG;
    starts[b] = total;
    total += f;
  }
  starts[nstreams] = total;
  hipStream_t st = (hipStream_t)hip_stream;
  if (total != 0) {
    if (!d_samples || !d_avg) return GLFER_E_ARG;
    if (glfer::stream_is_capturing(st)) return GLFER_E_ARG;
  }
  if (row_starts) std::copy(starts.begin(), starts.end(), row_starts);   // (past the last refusal: a refused call writes nothing)
  if (total == 0) return GLFER_OK;
  DeviceGuard guard(p->cfg.device);
  HIP_TRY(guard.error());
  glfer::Scratch<float> rows_buf(st);
  if (!d_psd) HIP_TRY(rows_buf.take(total * bins));
  float *rows = d_psd ? d_psd : rows_buf.get();
  if (const int rc = glfer_hip_spectrogram_ragged_device(p, d_samples, nstreams, offsets, lengths, rows, nullptr, st); rc != GLFER_OK) return rc;
  return glfer_hip_avg_ragged_device(avg_mode, rows, nstreams, starts.data(), (int)bins, n_out, depth, minbin, maxbin, max0, d_avg, d_ret, st);
}

// the sliding sums alone (avgdata->cum after each frame, avg.c:114-127); bins outside
// [minbin, maxbin) are left untouched
int glfer_hip_avg_cum_device(const float *d_psd, size_t nframes, int bins, int n_out, int depth, int minbin,
                             int maxbin, double *d_cum, void *hip_stream) {
  if (!d_psd || !d_cum) return GLFER_E_ARG;
  if (!glfer::update_avg_args_ok(GLFER_AVG_PLAIN, depth, minbin, maxbin, bins, n_out)) return GLFER_E_ARG;   // (the sums have no mode)
  DeviceGuard guard(data_device(d_psd));
  HIP_TRY(guard.error());
  HIP_TRY(glfer_launch_avg_cum(d_psd, nframes, bins, n_out, depth, minbin, maxbin, d_cum, (hipStream_t)hip_stream));
  return GLFER_OK;
}

// The LMP statistic (lmp.c:132-160) over rectangular-window periodogram rows the caller holds (glfer_hip.h): what an LMP plan's
// entries run after their transforms.  The ring size and the row length are checked first, then "nothing to do", then the rest.
static bool lmp_args_ok(int bins, int lmp_av) { return bins >= 1 && bins <= 65535 * 256 && lmp_av >= 1 && lmp_av <= 4096; }   // (the bin blocks fit a grid dimension)
// rows from frame row_first on hold everything frames [first, ..) sum over: the ring reaches back min(lmp_av - 1, first) frames
static bool lmp_rows_reach(size_t row_first, size_t first, int lmp_av) {
  return row_first <= first - std::min<size_t>((size_t)lmp_av - 1, first);
}

int glfer_hip_lmp_device(const float *d_rows, size_t row_first, size_t first, size_t nframes, int bins, int lmp_av, float *d_out,
                         void *hip_stream) {
  if (!lmp_args_ok(bins, lmp_av)) return GLFER_E_ARG;
  if (nframes == 0) return GLFER_OK;
  if (!d_rows || !d_out) return GLFER_E_ARG;
  if (nframes > 0x7fffffffu || first > (size_t)LLONG_MAX - nframes || !lmp_rows_reach(row_first, first, lmp_av)) return GLFER_E_ARG;
  DeviceGuard guard(data_device(d_rows));
  HIP_TRY(guard.error());
  HIP_TRY(glfer_launch_lmp(d_rows, (long long)row_first, (long long)first, nframes, bins, lmp_av, d_out, (hipStream_t)hip_stream));
  return GLFER_OK;
}

int glfer_hip_lmp_batch_device(const float *d_rows, size_t nstreams, size_t row_stride, size_t row_first, size_t first, size_t nframes,
                               int bins, int lmp_av, float *d_out, size_t out_stride, void *hip_stream) {
  if (!lmp_args_ok(bins, lmp_av)) return GLFER_E_ARG;
  if (nstreams == 0 || nframes == 0) return GLFER_OK;
  if (!d_rows || !d_out) return GLFER_E_ARG;
  if (nframes > 0x7fffffffu || first > (size_t)LLONG_MAX - nframes || !lmp_rows_reach(row_first, first, lmp_av)) return GLFER_E_ARG;
  // a stream's rows and outputs lie inside its stride; the strides of all streams inside size_t
  const size_t held = first - row_first + nframes;
  if (held > SIZE_MAX / sizeof(float) / (size_t)bins || row_stride < held * (size_t)bins || out_stride < nframes * (size_t)bins)
    return GLFER_E_ARG;
  if (row_stride > (SIZE_MAX / sizeof(float)) / nstreams || out_stride > (SIZE_MAX / sizeof(float)) / nstreams) return GLFER_E_ARG;
  DeviceGuard guard(data_device(d_rows));
  HIP_TRY(guard.error());
  const size_t chunk = 65535;                                    // streams per launch: the grid's z limit
  for (size_t c0 = 0; c0 < nstreams; c0 += chunk) {
    const unsigned nb = (unsigned)std::min(nstreams - c0, chunk);
    HIP_TRY(glfer_launch_lmp_batch(d_rows + c0 * row_stride, (long long)row_first, (long long)first, nframes, bins, lmp_av,
                                   d_out + c0 * out_stride, nb, (long long)row_stride, (long long)out_stride, (hipStream_t)hip_stream));
  }
  return GLFER_OK;
}

int glfer_hip_lmp_ragged_device(const float *d_rows, size_t nstreams, const size_t *row_starts, int bins, int lmp_av, float *d_out,
                                void *hip_stream) {
  if (!lmp_args_ok(bins, lmp_av)) return GLFER_E_ARG;
  if (nstreams == 0) return GLFER_OK;
  if (!row_starts || !glfer::ragged_rows_ok(row_starts, nstreams)) return GLFER_E_ARG;
  const size_t rows_hi = row_starts[nstreams];
  if (rows_hi > SIZE_MAX / sizeof(float) / (size_t)bins) return GLFER_E_ARG;
  if (rows_hi == row_starts[0]) return GLFER_OK;
  if (!d_rows || !d_out) return GLFER_E_ARG;
  hipStream_t st = (hipStream_t)hip_stream;
  if (glfer::stream_is_capturing(st)) return GLFER_E_ARG;
  DeviceGuard guard(data_device(d_rows));
  HIP_TRY(guard.error());
  HIP_TRY(glfer_launch_lmp_ragged(d_rows, row_starts, nstreams, bins, lmp_av, d_out, st));
  return GLFER_OK;
}

}  // extern "C"
