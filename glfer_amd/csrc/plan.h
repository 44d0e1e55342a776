// plan.h -- what the translation units of the C-ABI layer share: the plan (fft_init / mtm_init
// state, fft.c:168-187, mtm.c:88-151), error plumbing and the device guard.  Internal.
#pragma once
#include "../../include/glfer_hip.h"
#include "device_table.hpp"
#include "ragged_cols.hpp"
#include "scratch.hpp"

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <memory>
#include <mutex>
#include <string>
#include <vector>

namespace glfer {

int hip_fail(hipError_t e, const char *what);      // records the text for glfer_hip_last_hip_error(), returns GLFER_E_HIP
std::string error_text();                          // this thread's recorded text
void set_error_text(const std::string &text);      // (worker threads hand theirs to the calling thread)

// Every entry point runs on the device its plan (or its data) lives on and leaves the caller's
// current device as it found it (torch reads it through hipGetDevice).
class DeviceGuard {
 public:
  explicit DeviceGuard(int device) {
    if (hipGetDevice(&prev_) != hipSuccess) prev_ = -1;
    err_ = (device == prev_) ? hipSuccess : hipSetDevice(device);
    changed_ = err_ == hipSuccess && device != prev_;
  }
  ~DeviceGuard() {
    if (changed_ && prev_ >= 0) (void)hipSetDevice(prev_);
  }
  hipError_t error() const { return err_; }
  DeviceGuard(const DeviceGuard &) = delete;
  DeviceGuard &operator=(const DeviceGuard &) = delete;

 private:
  int prev_ = -1;
  bool changed_ = false;
  hipError_t err_ = hipSuccess;
};

// the device a device pointer belongs to (-1: not a device pointer HIP knows)
int device_of(const void *d_ptr);
// the device the data of a plan-less entry lives on: the pointer's, else the current one
int data_device(const void *d_ptr);

// ---- what the per-column entries share: waterfall.cpp (display and waterfall) and the floor / update_avg entries of glfer_hip.cpp
// The averaging-argument rule.  The waterfall's: a mode of update_avg_*, a window of at least one frame, a band inside the row.
inline bool avg_args_ok(int mode, int depth, int minbin, int maxbin, int bins) {
  return mode >= GLFER_AVG_SUMAVG && mode <= GLFER_AVG_SUMEXTREME && depth >= 1 && minbin >= 0 && maxbin > minbin && maxbin <= bins;
}
// update_avg's own: the band also lies inside the n_out values of an averaged row
inline bool update_avg_args_ok(int mode, int depth, int minbin, int maxbin, int bins, int n_out) {
  return avg_args_ok(mode, depth, minbin, maxbin, bins) && maxbin <= n_out && n_out >= 1;
}
// compute_floor of a contiguous run of rows `pitch` floats apart (the top 5 % of a row, fft.c:271), 2^22 rows a launch.  waterfall.cpp
hipError_t floor_rows(const float *d_psd, size_t rows, int bins, int pitch, float *d_stats, hipStream_t st);

// Allow `bytes` of dynamic LDS for `kernel` on the current device (hipFuncSetAttribute, once per
// device, kernel and size class).
hipError_t allow_dynamic_lds(const void *kernel, size_t bytes);

// The host-to-host entries' chunk ring (ingest.cpp run_job): two pinned sample buffers, two device
// sample buffers, two device row buffers, two pinned row buffers (+ the waterfall's), two streams.
// Kept with the plan between calls, freed by glfer_hip_plan_destroy.
struct IngestRing {
  unsigned char *h_in[2] = {nullptr, nullptr}, *d_in[2] = {nullptr, nullptr}, *h_out[2] = {nullptr, nullptr};
  unsigned char *d_rgb[2] = {nullptr, nullptr};
  short *h_lev[2] = {nullptr, nullptr}, *d_lev[2] = {nullptr, nullptr};
  float *d_psd[2] = {nullptr, nullptr}, *d_stats[2] = {nullptr, nullptr};
  unsigned char *d_planes[2] = {nullptr, nullptr};   // the channel entries' de-interleaved chunk (cap_planes bytes); never made by a one-channel job
  size_t cap_planes[2] = {0, 0};
  hipStream_t st[2] = {nullptr, nullptr};
  hipStream_t up = nullptr;                       // every chunk's upload (round 4): uploads queue behind one another, so that chunk c + 1 goes up while chunk c's rows come down
  hipEvent_t ev_up[2] = {nullptr, nullptr};       // chunk b's upload done: its stream's kernels wait for it
  hipEvent_t ev_t[2][4] = {{nullptr, nullptr, nullptr, nullptr}, {nullptr, nullptr, nullptr, nullptr}};   // timing (glfer_hip_phases, made on first use): upload begins / ends, kernels end, download ends
  size_t cap[2][8] = {{0, 0, 0, 0, 0, 0, 0, 0}, {0, 0, 0, 0, 0, 0, 0, 0}};
  bool busy = false;
};
void ingest_ring_free(IngestRing *r);          // parks the ring as the device's spare, or frees it
IngestRing *ingest_ring_take(int dev);         // the device's parked ring (the caller owns it), or null
void ingest_ring_drop_spare(int dev);          // frees the parked ring (glfer_hip_scratch_trim, glfer_hip_scratch_limit)
void workers_drop_kept();                      // the *_workers entries' kept handles (ingest.cpp): all of them
size_t workers_kept_bytes(int dev);            // their rings' bytes on `dev`
size_t ingest_ring_spare_bytes(int dev);       // pinned host + device bytes of the parked ring (counted by glfer_hip_scratch_held)

}  // namespace glfer

// The ticket counters of spectro16y.hip's queue form (SpectroParams::yq_counter), made with the plan and zeroed once.
// A counter is never reset: the host keeps the value it will have when the next launch starts (base) and advances it by
// the launch's chunks after a launch call that succeeded.  That holds while the launches that share a counter run one
// after another, so a counter belongs to ONE stream: the first SLOTS streams a plan is used on get one each (the host
// entries' chunk ring runs one plan on two streams), a launch on any further stream, on hipStreamPerThread (one handle,
// a stream per host thread) or on a stream that is being captured (a graph replays the base it was captured with) keeps
// the static stride.
struct glfer_yqueue {
  static constexpr int SLOTS = 8, PITCH = 32;      // a 128-byte line per counter
  glfer::DeviceTable<unsigned> d_counters;         // [SLOTS][PITCH]
  hipStream_t owner[SLOTS] = {};
  unsigned base[SLOTS] = {};
  int used = 0;
  std::mutex mu;                                   // held from reading a base to advancing it
};

#define HIP_TRY(call)                                          \
  do {                                                         \
    hipError_t e_ = (call);                                    \
    if (e_ != hipSuccess) return glfer::hip_fail(e_, #call);   \
  } while (0)

// The launchers of aux_kernels.hip that both glfer_hip.cpp (the update_avg entries) and waterfall.cpp (the staged waterfalls) call;
// every other launcher is declared where its one caller is, or in spectro_params.h.
extern "C" hipError_t glfer_launch_avg_batch(int mode, const float *psd, size_t nframes, int bins, int n_out, int depth, int minbin,
                                             int maxbin, int max0, double *avg, double *ret, unsigned nb, long long psd_bs,
                                             long long avg_bs, long long ret_bs, hipStream_t st);
extern "C" hipError_t glfer_launch_avg_ragged(int mode, const float *psd, const glfer::RaggedColsEntry *streams, size_t n, int bins,
                                              int n_out, int depth, int minbin, int maxbin, int max0, double *avg, double *ret,
                                              hipStream_t st);

// channels.hip: out[j * out_pitch + i] = in[i * channels + select[j]] over nframes sample frames of esz bytes a sample; select holds
// nselect checked channel indices.  wide = 0 keeps the general form where the stereo form could run (A/B runs).
extern "C" hipError_t glfer_launch_deinterleave(const void *in, size_t nframes, int channels, int esz, const unsigned char *select,
                                                int nselect, void *out, size_t out_pitch, int wide, hipStream_t st);

struct glfer_hip_plan {
  glfer_hip_config cfg;
  int n, hop, keep, bins, ntapers, npairs, lanes;
  int pitch = 0;                    // floats from one PSD row to the next in the device entries (cfg.psd_pitch, or bins)
  int lmp_av = 0;                   // LMP mode: periodograms in the ring (lmp.c:85)
  std::vector<float> window;        // [n] as the reference stores it (unit power)
  std::vector<double> tapers;       // [ntapers][n]
  std::vector<double> sig;          // [ntapers]
  // the device tables (plan_tables.h has a builder for each layout); an empty one: this plan has no such table
  glfer::DeviceTable<float> d_taps;     // [npairs][8][n/16][4] scaled tables (tap_slot)
  glfer::DeviceTable<float> d_window;   // [n] the window itself (FFT mode, not rectangular): prepare_audio's multiply
  glfer::DeviceTable<float> d_tw;       // [slots][lanes] float2
  glfer::DeviceTable<float> d_htaps;    // real-input form (spectro16h.hip): window pairs, [htapers][8][n/32][4]
  int htapers = 0;                      // 1: periodogram window; > 1: the tapers of the multitaper form (n >= 8192)
  glfer::DeviceTable<float> d_htw;      //   twiddles of the n/2-point transform, float2
  glfer::DeviceTable<float> d_hrot;     //   (cos,sin)(2 pi t/n), t < n/32
  glfer::DeviceTable<float> d_wtaps;    // wavefront-private real-input form (spectro16w.hip): [wtapers][W][8][64][4]
  int wtapers = 0;
  glfer::DeviceTable<float> d_wtw;      //   [27][64] twiddles of the 1024-point transform, float2
  glfer::DeviceTable<float> d_wcomb;    //   combine / split twiddles per lane, float2
  glfer::DeviceTable<float> d_bigtw;    // spectro_big.hip (N >= 32768): [W][16] the register part of the sub-transforms' twiddles, float2
  glfer::DeviceTable<float> d_xtaps;    // odd taper counts (spectro16x.hip): the last taper alone, [4][n/16][4]
  glfer::DeviceTable<float> d_ltaps;    // odd taper counts, LDS-resident half tables (spectro16xl.hip)
  glfer::DeviceTable<float> d_ytaps;    // five tapers at N = 4096, register-resident half tables (spectro16y.hip); empty: not exactly symmetric
  glfer::DeviceTable<float> d_iqtaps;   // complex I/Q rows (spectro16c.hip): [ntapers][4][n/16][4] one scaled float per sample and taper; empty: not supported
  glfer::DeviceTable<float> d_ataps;    // adaptive weights (spectro16a.hip): [2 ceil(ntapers/2)][4][n/16][4] the tapers UNSCALED, an odd count's last row zeros; empty: not supported
  std::unique_ptr<glfer_yqueue> yq;     // spectro16y.hip's queue form: the plan's ticket counters (N = 4096, odd taper counts)
  glfer::DeviceTable<uint16_t> d_lagmap;   // HP-ARMA: [t][p_e+1] lag held by each matrix cell
  glfer::DeviceTable<int> d_rot_sched;  // HP-ARMA: [rot_steps][8] the Jacobi sweep as steps of up to eight column-disjoint rotations (j | k << 8, -1 = none)
  int rot_steps = 0, rot_width = 8;
  glfer::DeviceTable<float> d_unit;     // HP-ARMA: [n/2+1] exp(-2 pi i k/n), float2
  // harmonic F-test (mtm.c:124-136): built on first use by ftest_tables, all of it or nothing
  std::mutex ftest_mu;                  // held while the F tables are looked for and made
  glfer::DeviceTable<float> d_ftaps_mu_first;   // [hn][taper 0..ntapers-1][hn], each [2n] alone in slot 0 of the packed layout
  float *d_ftaps = nullptr;         // = d_ftaps_mu_first + 2n: [ntapers+1][2n], taper j, then hn
  glfer::DeviceTable<float> d_ftaps2;   // the paired form (round 5): [ceil((ntapers+1)/2)][2n] with (hn_scale hn, taper 0), (taper 1, taper 2) ... as (re, im), halved;
  float *d_ftaps2_nomu = nullptr;   //   then [ceil(ntapers/2)][2n] with (taper 0, taper 1) ... (mu_live = 0); one allocation
  glfer::DeviceTable<double> d_U0;      // [ntapers]
  float *d_rows_cj = nullptr;       // [ntapers] 1 / (n (1 + sig_j)), in d_U0's allocation behind it: the rows' weights of the rows-and-F entries
  float sum_U0_sqr = 0.0f;
  float hn_scale = 1.0f;            // the power of two hn is multiplied by in d_ftaps2 (see SpectroParams::ft_mu_unscale)
  float spec_unscale = 1.0f;
  bool nonlin = false;
  glfer::IngestRing *ring = nullptr;   // the host entries' chunk ring, kept between calls (ingest.cpp)
  // side streams of the piecewise mean pass (glfer_hip.cpp launch_mean_inkernel): [0] runs the hop means of piece c+1
  // beside piece c's estimator launch, [1] takes every other estimator launch; made on first use
  hipStream_t aux[2] = {nullptr, nullptr};
  std::vector<hipEvent_t> aux_events;  // their events, made once (hipEventCreate per piece cost more than a piece's kernels)
  bool aux_busy = false;               // one call at a time forks onto the side streams; a second one meanwhile stays on its own stream
};

// The F-test's tables, made on the first F call of a plan (any entry) and kept with it.  Safe from several threads; a failed
// attempt leaves the plan as it was, and the next call tries again.  plan.cpp
int ftest_tables(glfer_hip_plan *p);

// frames [first, first+nframes) of a device-resident stream (virtual base allowed); psd and/or
// halfcomplex spectra out.  Asynchronous on `st`.  Defined in glfer_hip.cpp.
// tail_fresh >= 0: the LAST frame of the call is the file source's trailing partial block with that
// many fresh samples (wav_fmt.c:102-119); see glfer_hip_spectrogram_wav_ex.
int glfer_run_device(glfer_hip_plan *p, const void *d_stream, size_t nsamples, size_t first, size_t nframes,
                     float *d_psd, float *d_spec, hipStream_t st, long tail_fresh = -1);
