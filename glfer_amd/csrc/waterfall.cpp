// waterfall.cpp -- the display and waterfall entries of include/glfer_hip.h: compute_floor, update_avg_* and the display
// mapping of main_window_draw (g_main.c:1081-1236) for one stream, for equal streams (batch) and for packed streams of unequal
// length (ragged), and the two halves of a waterfall whose columns are spread over several GPUs.  What the entries have in common
// has one definition each, in front of them: the display options of a call (DisplayOptions), the small device table
// (DisplayTable), the opening checks and the epilogue of the batch forms, compute_floor over a run of rows (floor_rows); the
// averaging-argument rule is plan.h's.  The launch sequences stay each entry's own.
#include "plan.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>

#include "host_tables.h"
#include "ragged_cols.hpp"
#include "spectro_params.h"

extern "C" hipError_t glfer_launch_floor(const float *psd, size_t nframes, int bins, int pitch, int m, float *stats,
                                         hipStream_t st);
extern "C" int glfer_avgmap_applies(size_t walk, int bins, int depth, int minbin, int maxbin);
extern "C" hipError_t glfer_launch_avgmap(int mode, const float *psd, size_t fbeg, size_t nframes, int bins, int depth,
                                          int minbin, int maxbin, int max0, int scale_log, double thr255,
                                          double one_m_thr, const float *levels, const unsigned char *colortab,
                                          const double *log_thr, unsigned char *rgb, short *lev, hipStream_t st);
extern "C" hipError_t glfer_launch_avgmap_batch(int mode, const float *psd, size_t fbeg, size_t nframes, int bins, int depth,
                                                int minbin, int maxbin, int max0, int scale_log, double thr255, double one_m_thr,
                                                const float *levels, const unsigned char *colortab, const double *log_thr,
                                                unsigned char *rgb, short *lev, unsigned nb, long long psd_bs, long long lv_bs,
                                                long long col_bs, hipStream_t st);
extern "C" hipError_t glfer_launch_levels_batch(const float *stats, size_t nframes, int scale_log, float overlap, float *state,
                                                long long stats_bs, long long levels_bs, float *levels, float *chunk_state,
                                                unsigned nb, hipStream_t st);
extern "C" hipError_t glfer_launch_map_batch(const float *psd, const double *avg, size_t nframes, int n, int psd_pitch, int scale_log,
                                             double thr255, double one_m_thr, const float *levels, const unsigned char *colortab,
                                             const double *log_thr, unsigned char *rgb, short *lev, unsigned nb, long long src_bs,
                                             long long levels_bs, long long rgb_bs, long long lev_bs, hipStream_t st);
extern "C" hipError_t glfer_launch_avgmap_ragged(int mode, const float *psd, const glfer::RaggedColsEntry *streams, size_t n, int bins,
                                                 int depth, int minbin, int maxbin, int max0, int scale_log, double thr255,
                                                 double one_m_thr, const float *levels, const unsigned char *colortab,
                                                 const double *log_thr, unsigned char *rgb, short *lev, hipStream_t st);
extern "C" hipError_t glfer_launch_levels_ragged(const float *stats, const glfer::RaggedColsEntry *streams, size_t n, int scale_log,
                                                 float overlap, float *state, float *levels, float *chunk_state, hipStream_t st);
extern "C" hipError_t glfer_launch_map_ragged(const double *avg, const glfer::RaggedColsEntry *streams, size_t n, int bins, int scale_log,
                                              double thr255, double one_m_thr, const float *levels, const unsigned char *colortab,
                                              const double *log_thr, unsigned char *rgb, short *lev, hipStream_t st);

using glfer::data_device;
using glfer::DeviceGuard;
using glfer::hip_fail;
using glfer::RaggedColsEntry;

// ---- the shared pieces
static bool scale_type_ok(const glfer_hip_display &d) { return d.scale_type >= GLFER_SCALE_LIN && d.scale_type <= GLFER_SCALE_LOG_MAX0; }

// The display options of a call, resolved once from a glfer_hip_display.  Every entry takes them from here: the entries are
// compared bit for bit, so the fixed levels must round alike in all of them (float mx / mn, double arithmetic, as g_main.c has it).
struct DisplayOptions {
  int scale_log;
  double thr255, one_m_thr;                                                    // the threshold, as the map kernels take it
  float mx = 0.0f, mn = 0.0f, dmax = 0.0f, dmin = 0.0f;                        // the fixed levels (autoscale off)
  explicit DisplayOptions(const glfer_hip_display &d) {
    scale_log = d.scale_type == GLFER_SCALE_LOG || d.scale_type == GLFER_SCALE_LOG_MAX0;
    const float thr_level = d.thr_level / 100.0;                               // g_main.c:1099
    thr255 = 255.0 * thr_level;
    one_m_thr = 1.0 - thr_level;
    if (d.autoscale) return;
    mx = pow(10.0, d.max_level_db / 10.0);                                     // g_main.c:1125-1139
    mn = pow(10.0, d.min_level_db / 10.0);
    mn = (mx > mn ? mn : mx / 10.0);
    dmax = scale_log ? (float)(10.0 * log10(mx)) : mx;
    dmin = scale_log ? (float)(10.0 * log10(mn)) : mn;
  }
};

namespace glfer {
hipError_t floor_rows(const float *d_psd, size_t rows, int bins, int pitch, float *d_stats, hipStream_t st) {
  const int m = bins - (int)(bins * 0.95);                                     // fft.c:271: i = N2*0.95 .. N2-1
  const size_t piece = (size_t)1 << 22;
  for (size_t r0 = 0; r0 < rows; r0 += piece) {
    const hipError_t e = glfer_launch_floor(d_psd + r0 * (size_t)pitch, std::min(piece, rows - r0), bins, pitch, m, d_stats + r0 * 4, st);
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}
}  // namespace glfer

// The small device table of a batch or ragged call: the palette, the dB steps and the carried states of disps[0..n) as
// [n][3] floats {first_buffer, display_max_lvl, display_min_lvl}.  One stream-ordered allocation, one upload
// (Scratch::upload).  On an error nothing is left allocated.
struct DisplayTable {
  explicit DisplayTable(hipStream_t st) : block(st) {}
  glfer::Scratch<unsigned char> block;
  const unsigned char *d_tab = nullptr;
  const double *d_thr = nullptr;
  float *d_state = nullptr;
};
static hipError_t display_table_upload(const glfer_hip_display *disps, size_t n, DisplayTable *t) {
  const size_t thr_bytes = (2 * glfer::kLogThrK + 1) * sizeof(double), bytes = 768 + thr_bytes + n * 3 * sizeof(float);
  std::vector<unsigned char> host(bytes);
  glfer::make_palette(disps[0].palette, host.data());
  memcpy(host.data() + 768, glfer::log_thresholds(), thr_bytes);
  float *h_state = reinterpret_cast<float *>(host.data() + 768 + thr_bytes);
  for (size_t b = 0; b < n; b++) {
    h_state[b * 3 + 0] = disps[b].first_buffer != 0 ? 1.0f : 0.0f;
    h_state[b * 3 + 1] = disps[b].display_max_lvl;
    h_state[b * 3 + 2] = disps[b].display_min_lvl;
  }
  const hipError_t e = t->block.upload(host.data(), bytes);
  if (e != hipSuccess) return e;
  t->d_tab = t->block.get();
  t->d_thr = reinterpret_cast<const double *>(t->block.get() + 768);
  t->d_state = reinterpret_cast<float *>(t->block.get() + 768 + thr_bytes);
  return hipSuccess;
}

// update_avg_* inside the mapping (avg_fused_kernel<.., MAP>): the PSD batch the columns belong to,
// their first row in it, and update_avg's arguments
struct MapAverages {
  int mode, depth, minbin, maxbin, max0;
  const float *d_batch;
  size_t first;
};

// The mapping part of main_window_draw for `nframes` columns: level tracking, then the pixel map of the
// PSD rows, of averaged rows, or (fused) of the averages taken on the way.
// d_levels_in: the columns' levels already known (the walk was done elsewhere -- over ALL columns of a
// waterfall whose rows are spread over several GPUs, glfer_hip_levels_host): no walk, d_stats unused,
// the carried state in *d untouched.
static int display_columns(glfer_hip_display *d, const float *d_psd, const double *d_avg, const MapAverages *fused,
                           const float *d_stats, size_t nframes, int bins, unsigned char *d_rgb, short *d_lev,
                           float *d_levels, void *hip_stream, const float *d_levels_in = nullptr, int psd_pitch = 0) {
  if (!d || (!d_stats && !d_levels_in) || !d_rgb || bins < 1) return GLFER_E_ARG;
  if (psd_pitch == 0) psd_pitch = bins;                  // floats from one row of d_psd to the next (cfg.psd_pitch)
  if (psd_pitch < bins || (fused && psd_pitch != bins)) return GLFER_E_ARG;
  if ((d_psd != nullptr) + (d_avg != nullptr) + (fused != nullptr) != 1) return GLFER_E_ARG;
  if (!scale_type_ok(*d)) return GLFER_E_ARG;
  if (nframes == 0) return GLFER_OK;
  hipStream_t st = (hipStream_t)hip_stream;
  DeviceGuard guard(data_device(d_rgb));
  HIP_TRY(guard.error());
  const DisplayOptions o(*d);

  // one stream-ordered allocation: the palette, the table of the dB steps, the levels rows (when
  // the caller does not want them) and the chunk states of the autoscale walk
  const size_t lev_floats = (d_levels || d_levels_in) ? 0 : nframes * 4;
  const size_t st_floats = (d->autoscale && !d_levels_in) ? glfer_levels_scratch_floats(nframes) : 0;
  const size_t thr_bytes = (2 * glfer::kLogThrK + 1) * sizeof(double);
  glfer::Scratch<unsigned char> block(st);
  HIP_TRY(block.take(768 + thr_bytes + (lev_floats + st_floats) * sizeof(float)));
  unsigned char *const scratch = block.get();
  unsigned char *d_tab = scratch;
  double *d_thr = reinterpret_cast<double *>(scratch + 768);
  float *fs = reinterpret_cast<float *>(scratch + 768 + thr_bytes);
  float *levels = d_levels_in ? const_cast<float *>(d_levels_in) : (d_levels ? d_levels : fs);
  float *chunk_state = st_floats ? fs + lev_floats : nullptr;
  int rc = GLFER_OK;
  auto fail = [&](hipError_t err) { rc = hip_fail(err, "glfer_hip_display_device"); };
  unsigned char tab[768];
  glfer::make_palette(d->palette, tab);
  // pageable source: hipMemcpyAsync stages it before returning, so `tab` may go out of scope
  hipError_t e = hipMemcpyAsync(d_tab, tab, 768, hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipMemcpyAsync(d_thr, glfer::log_thresholds(), thr_bytes, hipMemcpyHostToDevice, st);
  if (e != hipSuccess) fail(e);

  if (rc == GLFER_OK && !d_levels_in) {
    if (d->autoscale) {
      e = glfer_launch_levels(d_stats, nframes, o.scale_log, 1, d->first_buffer, d->overlap, d->display_max_lvl,
                              d->display_min_lvl, levels, chunk_state, st);
    } else {
      e = glfer_launch_levels_fixed(nframes, o.dmax, o.dmin, o.mx, o.mn, levels, st);
    }
    if (e != hipSuccess) fail(e);
  }
  if (rc == GLFER_OK) {
    if (fused)
      e = glfer_launch_avgmap(fused->mode, fused->d_batch, fused->first, fused->first + nframes, bins, fused->depth,
                              fused->minbin, fused->maxbin, fused->max0, o.scale_log, o.thr255, o.one_m_thr, levels, d_tab, d_thr,
                              d_rgb, d_lev, st);
    else
      e = glfer_launch_map(d_psd, d_avg, nframes, bins, psd_pitch, o.scale_log, o.thr255, o.one_m_thr, levels, d_tab, d_thr, d_rgb,
                           d_lev, st);
    if (e != hipSuccess) fail(e);
  }
  float last[4] = {0, 0, 0, 0};
  if (rc == GLFER_OK && !d_levels_in) {
    e = hipMemcpyAsync(last, levels + (nframes - 1) * 4, sizeof last, hipMemcpyDeviceToHost, st);
    if (e != hipSuccess) fail(e);
  }
  block.release();                           // (stream-ordered: before the wait, not after it)
  e = hipStreamSynchronize(st);              // the carried state comes back to the host
  if (e != hipSuccess && rc == GLFER_OK) fail(e);
  if (rc == GLFER_OK && !d_levels_in) {
    d->display_max_lvl = last[2];
    d->display_min_lvl = last[3];
    if (d->autoscale) d->first_buffer = 0;                                     // g_main.c:1120
  }
  return rc;
}

extern "C" {

int glfer_hip_display_device(glfer_hip_display *d, const float *d_psd, const double *d_avg, const float *d_stats,
                             size_t nframes, int bins, unsigned char *d_rgb, short *d_lev, float *d_levels,
                             void *hip_stream) {
  if (!d || (d_psd == nullptr) == (d_avg == nullptr)) return GLFER_E_ARG;
  return display_columns(d, d_psd, d_avg, nullptr, d_stats, nframes, bins, d_rgb, d_lev, d_levels, hip_stream, nullptr, d->psd_pitch);
}

// compute_floor + update_avg_* + the display mapping of main_window_draw (g_main.c:1109-1236) for a
// batch of PSD rows in one call.  The level tracking is a chain over the columns (g_main.c:1122-1123)
// fed by every column's floor statistics, so a row is read twice -- once for its statistics (and its
// moving sums), once to be mapped -- and the chain walk costs ~0.1 us per column of LATENCY however
// few columns it is given (its chunks warm up over the 4096 columns before them, display.hip).
// Cache-sized tiles (rows still in the 256 MiB Infinity Cache when the map reads them) were
// measured: 15 M rows/s against 117 M stage by stage over the whole batch
// (profiles/r02_aux_sweep.txt) -- the chain's latency per tile swamps the saved HBM read.  So the
// stages run over tiles that only bound the scratch (averaged rows: 8 B/bin, 4 GiB per tile).
}  // extern "C"

// The route of a waterfall over `nframes` rows (glfer_hip_waterfall_device, and every stream of
// glfer_hip_waterfall_batch_device): averages inside the mapping kernel (*fused) or staged, and the rows per tile.
// Tiles only bound the scratch: the level walk costs its ~0.13 ms of latency per display call
// however few columns it gets, so fewer, larger tiles are faster (two 65536-row tiles: 116 M rows/s
// against 147 M stage by stage).  The averages are taken inside the mapping kernel where that form
// applies (no averaged rows in memory at all: GLFER_WATERFALL_FUSED=0 forces the staged form, for
// A/B runs and tests); staged, averaged rows are 8 B per bin: 4 GiB of them per tile.  Otherwise
// only the 16 B of statistics per row are scratch.
static void waterfall_route(int avg_mode, int depth, int minbin, int maxbin, int bins, int pitch, size_t nframes, bool *fused_out,
                            size_t *tile_out) {
  const bool averaging = avg_mode != 0;
  bool fused = averaging && pitch == bins;               // (the average-in-the-map kernel walks dense rows)
  if (const char *e = getenv("GLFER_WATERFALL_FUSED")) fused = fused && atoi(e) != 0;
  size_t tile = (averaging && !fused) ? std::max<size_t>(16384, ((size_t)4 << 30) / ((size_t)bins * sizeof(double))) : (size_t)1 << 22;
  if (const char *e = getenv("GLFER_WATERFALL_TILE")) {    // rows per tile, for tests of the tile seams and for tuning
    const long v = atol(e);
    if (v >= 64) tile = (size_t)v;
  }
  tile = std::min(tile, nframes);
  tile = (nframes + (nframes + tile - 1) / tile - 1) / ((nframes + tile - 1) / tile);   // equal tiles: no short last one
  // the form's chunking depends on the number of rows it walks, and the last tile may be a few rows
  // shorter than the others: the fused form is taken only if it applies to BOTH lengths
  const size_t last_tile = nframes - (nframes - 1) / tile * tile;
  if (fused) fused = glfer_avgmap_applies(tile, bins, depth, minbin, maxbin) != 0 &&
                     glfer_avgmap_applies(last_tile, bins, depth, minbin, maxbin) != 0;
  *fused_out = fused;
  *tile_out = tile;
}

// Rows [row0, row0 + nframes) of the batch d_psd.  row0 > 0 / d_levels_in: the second phase of a
// waterfall whose columns are spread over several GPUs (glfer_hip_waterfall_map_device) -- the moving
// sums of the first rows reach back into the batch's rows before row0, the levels are given.
static int waterfall_columns(glfer_hip_display *d, int avg_mode, int depth, int minbin, int maxbin, int max0,
                             const float *d_batch, size_t row0, size_t nframes, int bins, unsigned char *d_rgb, short *d_lev,
                             float *d_stats, void *hip_stream, const float *d_levels_in, int pitch = 0) {
  if (pitch == 0) pitch = bins;                          // floats from one PSD row to the next (cfg.psd_pitch)
  const float *d_psd = d_batch ? d_batch + row0 * (size_t)pitch : nullptr;
  if (!d || !d_psd || !d_rgb || bins < 1 || bins > 32769 || pitch < bins) return GLFER_E_ARG;
  const bool averaging = avg_mode != 0;
  if (averaging && !glfer::avg_args_ok(avg_mode, depth, minbin, maxbin, bins)) return GLFER_E_ARG;
  if (nframes == 0) return GLFER_OK;
  hipStream_t st = (hipStream_t)hip_stream;
  DeviceGuard guard(data_device(d_psd));
  HIP_TRY(guard.error());
  bool fused = false;
  size_t tile = 0;
  waterfall_route(avg_mode, depth, minbin, maxbin, bins, pitch, nframes, &fused, &tile);
  const size_t back = averaging ? (size_t)depth : 0;       // rows re-read in front of a tile to restart the sliding sums
  glfer::Scratch<float> stats(st);
  glfer::Scratch<double> avg(st), ret(st);
  if (!d_stats && !d_levels_in) HIP_TRY(stats.take(tile * 4));
  if (averaging && !fused) {
    hipError_t e = avg.take((tile + back) * (size_t)bins);
    if (e == hipSuccess) e = ret.take((tile + back) * 4);
    if (e != hipSuccess) return hip_fail(e, "hipMallocAsync(waterfall tile)");
  }
  int rc = GLFER_OK;
  for (size_t f0 = 0; rc == GLFER_OK && f0 < nframes; f0 += tile) {
    const size_t nf = std::min(tile, nframes - f0);
    float *tstats = d_stats ? d_stats + f0 * 4 : stats.get();
    const float *tlevels = d_levels_in ? d_levels_in + f0 * 4 : nullptr;
    unsigned char *trgb = d_rgb + f0 * (size_t)bins * 3;
    short *tlev = d_lev ? d_lev + f0 * (size_t)bins : nullptr;
    if (tstats) rc = glfer_hip_floor_device_pitched(d_psd + f0 * (size_t)pitch, nf, bins, pitch, tstats, st);
    if (rc != GLFER_OK) break;
    if (fused) {
      // the sliding sums of the tile's first rows reach back into the rows before it by themselves
      const MapAverages ma{avg_mode, depth, minbin, maxbin, max0 ? 1 : 0, d_batch, row0 + f0};
      rc = display_columns(d, nullptr, nullptr, &ma, tstats, nf, bins, trgb, tlev, nullptr, st, tlevels);
      continue;
    }
    const double *src_avg = nullptr;
    if (averaging) {
      // the sums of the tile's first rows reach `depth` rows back: run from there (from an empty
      // state at row 0 of the batch, as update_avg does after alloc_avg) and use the tile's rows
      const size_t lead = std::min(back, row0 + f0);
      // (update_avg's `bins` is its rows' stride; the band is minbin..maxbin, the averaged rows are dense)
      rc = glfer_hip_avg_device(avg_mode, d_batch + (row0 + f0 - lead) * (size_t)pitch, nf + lead, pitch, bins, depth, minbin, maxbin, max0,
                                avg.get(), ret.get(), st);
      src_avg = avg.get() + lead * (size_t)bins;
    }
    if (rc == GLFER_OK)
      rc = display_columns(d, averaging ? nullptr : d_psd + f0 * (size_t)pitch, src_avg, nullptr, tstats, nf, bins, trgb, tlev,
                           nullptr, st, tlevels, pitch);
  }
  return rc;
}

extern "C" {

int glfer_hip_waterfall_device(glfer_hip_display *d, int avg_mode, int depth, int minbin, int maxbin, int max0,
                               const float *d_psd, size_t nframes, int bins, unsigned char *d_rgb, short *d_lev,
                               float *d_stats, void *hip_stream) {
  return waterfall_columns(d, avg_mode, depth, minbin, maxbin, max0, d_psd, 0, nframes, bins, d_rgb, d_lev, d_stats, hip_stream,
                           nullptr, d ? d->psd_pitch : 0);
}

// The two halves of glfer_hip_waterfall_device for columns that live on several GPUs.  The level
// tracking (g_main.c:1111-1124) is ONE chain over all columns, fed by 16 bytes of floor statistics
// per column; everything else is per column.  So: every GPU computes its rows and their statistics,
// the statistics meet on the host, ONE walk over them (here: on `device`, the walk of
// glfer_hip_display_device) gives every column its levels, and every GPU maps its own rows with its
// slice of the levels.  Nothing but 16 + 16 bytes per column crosses between GPUs, through the host.
int glfer_hip_levels_host(glfer_hip_display *d, const float *h_stats, size_t nframes, float *h_levels, int device) {
  if (!d || !h_stats || !h_levels) return GLFER_E_ARG;
  if (!scale_type_ok(*d)) return GLFER_E_ARG;
  if (nframes == 0) return GLFER_OK;
  DeviceGuard guard(device);
  HIP_TRY(guard.error());
  const DisplayOptions o(*d);
  const size_t st_floats = d->autoscale ? glfer_levels_scratch_floats(nframes) : 0;
  glfer::Scratch<float> block(nullptr);
  HIP_TRY(block.take(nframes * 8 + st_floats));
  float *const buf = block.get();
  float *d_stats = buf, *levels = buf + nframes * 4, *chunk_state = st_floats ? buf + nframes * 8 : nullptr;
  int rc = GLFER_OK;
  hipError_t e = hipMemcpyAsync(d_stats, h_stats, nframes * 4 * sizeof(float), hipMemcpyHostToDevice, nullptr);
  if (e == hipSuccess) {
    if (d->autoscale) {
      e = glfer_launch_levels(d_stats, nframes, o.scale_log, 1, d->first_buffer, d->overlap, d->display_max_lvl,
                              d->display_min_lvl, levels, chunk_state, nullptr);
    } else {
      e = glfer_launch_levels_fixed(nframes, o.dmax, o.dmin, o.mx, o.mn, levels, nullptr);
    }
  }
  if (e == hipSuccess) e = hipMemcpyAsync(h_levels, levels, nframes * 4 * sizeof(float), hipMemcpyDeviceToHost, nullptr);
  if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
  if (e != hipSuccess) rc = hip_fail(e, "glfer_hip_levels_host");
  if (rc == GLFER_OK) {
    d->display_max_lvl = h_levels[(nframes - 1) * 4 + 2];
    d->display_min_lvl = h_levels[(nframes - 1) * 4 + 3];
    if (d->autoscale) d->first_buffer = 0;                                     // g_main.c:1120
  }
  return rc;
}

int glfer_hip_waterfall_map_device(const glfer_hip_display *d, int avg_mode, int depth, int minbin, int maxbin, int max0,
                                   const float *d_batch, size_t first, size_t nframes, int bins, const float *d_levels,
                                   unsigned char *d_rgb, short *d_lev, void *hip_stream) {
  if (!d || !d_levels) return GLFER_E_ARG;
  glfer_hip_display copy = *d;               // the carried state is not touched: the walk was glfer_hip_levels_host's
  return waterfall_columns(&copy, avg_mode, depth, minbin, maxbin, max0, d_batch, first, nframes, bins, d_rgb, d_lev, nullptr,
                           hip_stream, d_levels, d->psd_pitch);
}

}  // extern "C"

// ---- many streams in one call: what the batch and the ragged waterfall share
static bool same_display_options(const glfer_hip_display &a, const glfer_hip_display &b) {
  return a.scale_type == b.scale_type && a.autoscale == b.autoscale && a.overlap == b.overlap && a.max_level_db == b.max_level_db &&
         a.min_level_db == b.min_level_db && a.thr_level == b.thr_level && a.palette == b.palette && a.psd_pitch == b.psd_pitch;
}

// The checks both entries open with: one display plan over all streams, waterfall_columns' rules for the rows and the averaging
// arguments.  false: the entry returns *rc at once (GLFER_OK: no streams).  *pitch: floats from one PSD row to the next.
static bool waterfall_batch_opens(const glfer_hip_display *disps, size_t nstreams, int avg_mode, int depth, int minbin, int maxbin, int bins,
                                  int *pitch, int *rc) {
  *rc = GLFER_OK;
  if (nstreams == 0) return false;
  *rc = GLFER_E_ARG;
  if (!disps) return false;
  for (size_t b = 1; b < nstreams; b++)                  // one plan, many streams
    if (!same_display_options(disps[0], disps[b])) return false;
  *pitch = disps[0].psd_pitch == 0 ? bins : disps[0].psd_pitch;
  if (bins < 1 || bins > 32769 || *pitch < bins) return false;
  if (avg_mode != 0 && !glfer::avg_args_ok(avg_mode, depth, minbin, maxbin, bins)) return false;
  *rc = GLFER_OK;
  return true;
}

// The stream-ordered scratch of such a call (waterfall_batch_finish gives it back before its wait): the statistics of all rows
// (only without d_stats), the levels with the walks' chunk states behind them, the averaged rows of a staged group and their
// return values.
struct WaterfallScratch {
  explicit WaterfallScratch(hipStream_t st) : own_stats(st), levels(st), avg(st), ret(st) {}
  float *stats = nullptr;                                 // the caller's d_stats, or own_stats
  glfer::Scratch<float> own_stats, levels;
  glfer::Scratch<double> avg, ret;
  void release() {
    avg.release();
    ret.release();
    levels.release();
    own_stats.release();
  }
};
// (after a failure nothing more is asked for, and nothing is kept)
static hipError_t waterfall_scratch_take(WaterfallScratch *s, float *d_stats, size_t rows, size_t level_floats, size_t avg_rows, size_t bins) {
  hipError_t e = d_stats ? hipSuccess : s->own_stats.take(rows * 4);
  s->stats = d_stats ? d_stats : s->own_stats.get();
  if (e == hipSuccess) e = s->levels.take(level_floats);
  if (e == hipSuccess && avg_rows) e = s->avg.take(avg_rows * bins);
  if (e == hipSuccess && avg_rows) e = s->ret.take(avg_rows * 4);
  if (e != hipSuccess) s->release();
  return e;
}

// The end of such a call: the carried states come down (autoscale), the scratch and the table go back -- stream-ordered, before
// the synchronisation -- and after it the displays take their states: those of the streams `live` names, or all of them.
static int waterfall_batch_finish(int rc, glfer_hip_display *disps, size_t nstreams, const std::vector<RaggedColsEntry> *live,
                                  const DisplayOptions &o, DisplayTable &t, WaterfallScratch &s, hipStream_t st,
                                  const char *entry) {
  const bool autoscale = disps[0].autoscale != 0;
  std::vector<float> back_state(autoscale ? nstreams * 3 : 0);
  hipError_t e = hipSuccess;
  if (rc == GLFER_OK && autoscale) e = hipMemcpyAsync(back_state.data(), t.d_state, nstreams * 3 * sizeof(float), hipMemcpyDeviceToHost, st);
  if (e != hipSuccess) rc = hip_fail(e, entry);
  s.release();
  t.block.release();
  e = hipStreamSynchronize(st);              // the carried states come back to the host
  if (e != hipSuccess && rc == GLFER_OK) rc = hip_fail(e, entry);
  if (rc != GLFER_OK) return rc;
  auto store = [&](size_t b) {
    disps[b].display_max_lvl = autoscale ? back_state[b * 3 + 1] : o.mx;
    disps[b].display_min_lvl = autoscale ? back_state[b * 3 + 2] : o.mn;
    if (autoscale) disps[b].first_buffer = 0;                                  // g_main.c:1120
  };
  if (live)
    for (const RaggedColsEntry &x : *live) store((size_t)x.stream);
  else
    for (size_t b = 0; b < nstreams; b++) store(b);
  return rc;
}

// ---- the ragged entries' own rules (ragged_cols.hpp)
namespace glfer {
bool stream_is_capturing(hipStream_t st) {
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  if (st != hipStreamPerThread && hipStreamIsCapturing(st, &cs) == hipSuccess) return cs != hipStreamCaptureStatusNone;
  (void)hipGetLastError();
  return false;
}
bool ragged_rows_ok(const size_t *row_starts, size_t nstreams) {
  if (nstreams > 0x7fffffffu) return false;
  for (size_t b = 0; b < nstreams; b++)
    if (row_starts[b + 1] < row_starts[b] || row_starts[b + 1] - row_starts[b] > 0x7fffffffu) return false;
  return true;
}
std::vector<RaggedColsEntry> ragged_streams(const size_t *row_starts, size_t nstreams) {
  std::vector<RaggedColsEntry> s;
  for (size_t b = 0; b < nstreams; b++)
    if (row_starts[b + 1] > row_starts[b])
      s.push_back(RaggedColsEntry{(long long)row_starts[b], (long long)row_starts[b], (long long)(row_starts[b + 1] - row_starts[b]), 0, 0, (int)b});
  return s;
}
}  // namespace glfer

extern "C" {

// glfer_hip_waterfall_device over many streams of one display plan (glfer_hip.h).  The route -- fused or staged average, the
// frame tiles, the avgmap shape -- is that entry's for ONE stream's frames (waterfall_route); every launch it leads to covers
// the batch: the floor statistics of all rows at once (the rows of all streams are one run), then per tile the autoscale walk
// (blockIdx.y the stream, its carried state in a device table that stays there from tile to tile), and the map with a stream
// dimension (fused: avg_fused_kernel<.., MAP, .., BAT>; staged: glfer_launch_avg_batch, then the map of the averaged rows).
// One upload (palette, dB table, states), one download of the states and one synchronisation per call.
int glfer_hip_waterfall_batch_device(glfer_hip_display *disps, size_t nstreams, int avg_mode, int depth, int minbin, int maxbin,
                                     int max0, const float *d_psd, size_t nframes, int bins, unsigned char *d_rgb, short *d_lev,
                                     float *d_stats, void *hip_stream) {
  int pitch = 0, rc = GLFER_OK;
  if (!waterfall_batch_opens(disps, nstreams, avg_mode, depth, minbin, maxbin, bins, &pitch, &rc)) return rc;
  if (nframes == 0) return GLFER_OK;
  if (!d_psd || !d_rgb || !scale_type_ok(disps[0])) return GLFER_E_ARG;
  if (nframes > (SIZE_MAX / sizeof(double) / (size_t)pitch) / nstreams) return GLFER_E_ARG;
  hipStream_t st = (hipStream_t)hip_stream;
  DeviceGuard guard(data_device(d_psd));
  HIP_TRY(guard.error());
  const bool averaging = avg_mode != 0, autoscale = disps[0].autoscale != 0;
  bool fused = false;
  size_t tile = 0;
  waterfall_route(avg_mode, depth, minbin, maxbin, bins, pitch, nframes, &fused, &tile);
  const bool staged = averaging && !fused;
  const DisplayOptions o(disps[0]);
  const size_t back = averaging ? (size_t)depth : 0;
  const size_t bins_z = (size_t)bins, rows_bs = nframes * (size_t)pitch, cols = nframes * bins_z;
  const size_t chunk = 65535;                            // streams per launch: the grid's y limit
  // staged: streams per group, the averaged rows of a group within the single-stream entry's 4 GiB per tile
  size_t group = chunk;
  if (staged) group = std::max<size_t>(1, std::min(group, ((size_t)4 << 30) / ((tile + back) * bins_z * sizeof(double))));

  DisplayTable t(st);
  HIP_TRY(display_table_upload(disps, nstreams, &t));
  auto fail = [&](hipError_t err, const char *what) {
    if (rc == GLFER_OK) rc = hip_fail(err, what);
  };
  // scratch: statistics of all rows, a tile's levels and chunk states, a group's averaged rows (staged)
  const size_t st_floats = autoscale ? glfer_levels_scratch_floats(tile) : 0;
  WaterfallScratch s(st);
  hipError_t e = waterfall_scratch_take(&s, d_stats, nstreams * nframes, nstreams * (tile * 4 + st_floats),
                                        staged ? std::min(group, nstreams) * (tile + back) : 0, bins_z);
  if (e != hipSuccess) fail(e, "scratch (waterfall, batch)");
  float *stats = s.stats, *levels = s.levels.get(), *chunk_state = levels ? levels + nstreams * tile * 4 : nullptr;

  // compute_floor of every row: the streams' rows are one run of nstreams x nframes rows
  if (rc == GLFER_OK) {
    e = glfer::floor_rows(d_psd, nstreams * nframes, bins, pitch, stats, st);
    if (e != hipSuccess) fail(e, "compute_floor launch (batch)");
  }
  for (size_t f0 = 0; rc == GLFER_OK && f0 < nframes; f0 += tile) {
    const size_t nf = std::min(tile, nframes - f0);
    // the tile's levels, [nstreams][nf][4]
    if (autoscale) {
      for (size_t c0 = 0; rc == GLFER_OK && c0 < nstreams; c0 += chunk) {
        const unsigned nb = (unsigned)std::min(nstreams - c0, chunk);
        e = glfer_launch_levels_batch(stats + (c0 * nframes + f0) * 4, nf, o.scale_log, disps[0].overlap, t.d_state + c0 * 3,
                                      (long long)(nframes * 4), (long long)(nf * 4), levels + c0 * nf * 4,
                                      chunk_state + c0 * glfer_levels_scratch_floats(nf), nb, st);
        if (e != hipSuccess) fail(e, "level tracking launch (batch)");
      }
    } else {
      e = glfer_launch_levels_fixed(nstreams * nf, o.dmax, o.dmin, o.mx, o.mn, levels, st);
      if (e != hipSuccess) fail(e, "levels launch (batch)");
    }
    if (rc != GLFER_OK) break;
    if (fused) {
      // the sliding sums of the tile's first rows reach back into the stream's rows before it by themselves
      for (size_t c0 = 0; rc == GLFER_OK && c0 < nstreams; c0 += chunk) {
        const unsigned nb = (unsigned)std::min(nstreams - c0, chunk);
        e = glfer_launch_avgmap_batch(avg_mode, d_psd + c0 * rows_bs, f0, f0 + nf, bins, depth, minbin, maxbin, max0 ? 1 : 0, o.scale_log,
                                      o.thr255, o.one_m_thr, levels + c0 * nf * 4, t.d_tab, t.d_thr, d_rgb + (c0 * cols + f0 * bins_z) * 3,
                                      d_lev ? d_lev + c0 * cols + f0 * bins_z : nullptr, nb, (long long)rows_bs, (long long)nf,
                                      (long long)nframes, st);
        if (e != hipSuccess) fail(e, "average-and-map launch (batch)");
      }
      continue;
    }
    if (!averaging) {
      for (size_t c0 = 0; rc == GLFER_OK && c0 < nstreams; c0 += chunk) {
        const unsigned nb = (unsigned)std::min(nstreams - c0, chunk);
        e = glfer_launch_map_batch(d_psd + c0 * rows_bs + f0 * (size_t)pitch, nullptr, nf, bins, pitch, o.scale_log, o.thr255, o.one_m_thr,
                                   levels + c0 * nf * 4, t.d_tab, t.d_thr, d_rgb + (c0 * cols + f0 * bins_z) * 3,
                                   d_lev ? d_lev + c0 * cols + f0 * bins_z : nullptr, nb, (long long)rows_bs, (long long)(nf * 4),
                                   (long long)(cols * 3), (long long)cols, st);
        if (e != hipSuccess) fail(e, "map launch (batch)");
      }
      continue;
    }
    // staged: the sums of the tile's first rows reach `depth` rows back -- run from there (from an empty state at the stream's
    // row 0, as update_avg does after alloc_avg) and map the tile's rows
    const size_t lead = std::min(back, f0), arows = nf + lead;
    for (size_t c0 = 0; rc == GLFER_OK && c0 < nstreams; c0 += group) {
      const unsigned nb = (unsigned)std::min(nstreams - c0, group);
      e = glfer_launch_avg_batch(avg_mode, d_psd + c0 * rows_bs + (f0 - lead) * (size_t)pitch, arows, pitch, bins, depth, minbin, maxbin,
                                 max0 ? 1 : 0, s.avg.get(), s.ret.get(), nb, (long long)rows_bs, (long long)(arows * bins_z), (long long)(arows * 4), st);
      if (e != hipSuccess) fail(e, "update_avg launch (waterfall, batch)");
      if (rc == GLFER_OK) {
        e = glfer_launch_map_batch(nullptr, s.avg.get() + lead * bins_z, nf, bins, bins, o.scale_log, o.thr255, o.one_m_thr, levels + c0 * nf * 4,
                                   t.d_tab, t.d_thr, d_rgb + (c0 * cols + f0 * bins_z) * 3, d_lev ? d_lev + c0 * cols + f0 * bins_z : nullptr,
                                   nb, (long long)(arows * bins_z), (long long)(nf * 4), (long long)(cols * 3), (long long)cols, st);
        if (e != hipSuccess) fail(e, "map launch (waterfall, batch)");
      }
    }
  }
  return waterfall_batch_finish(rc, disps, nstreams, nullptr, o, t, s, st, "glfer_hip_waterfall_batch_device");
}

// glfer_hip_waterfall_batch_device for packed rows of streams of unequal length (glfer_hip.h).  Every stream takes the route
// glfer_hip_waterfall_device takes for its own frame count (waterfall_route): the per-row stages -- compute_floor, the plain
// map, the fixed levels -- run over the packed rows as one run; the autoscale walk, the average-and-map kernel and the staged
// average read a per-stream table (ragged_cols.hpp).  Streams whose route is the fused one and streams whose route is staged are
// two classes with a launch set each.  A stream its route would cut into tiles sends the whole call through the single entry.
int glfer_hip_waterfall_ragged_device(glfer_hip_display *disps, size_t nstreams, int avg_mode, int depth, int minbin, int maxbin,
                                      int max0, const float *d_psd, const size_t *row_starts, int bins, unsigned char *d_rgb,
                                      short *d_lev, float *d_stats, void *hip_stream) {
  int pitch = 0, rc = GLFER_OK;
  if (!waterfall_batch_opens(disps, nstreams, avg_mode, depth, minbin, maxbin, bins, &pitch, &rc)) return rc;
  if (!scale_type_ok(disps[0])) return GLFER_E_ARG;
  if (!row_starts || !glfer::ragged_rows_ok(row_starts, nstreams)) return GLFER_E_ARG;
  const size_t rows_lo = row_starts[0], rows_hi = row_starts[nstreams];
  if (rows_hi > SIZE_MAX / sizeof(double) / (size_t)pitch) return GLFER_E_ARG;
  if (rows_hi == rows_lo) return GLFER_OK;
  if (!d_psd || !d_rgb) return GLFER_E_ARG;
  hipStream_t st = (hipStream_t)hip_stream;
  if (glfer::stream_is_capturing(st)) return GLFER_E_ARG;
  DeviceGuard guard(data_device(d_psd));
  HIP_TRY(guard.error());
  const bool averaging = avg_mode != 0, autoscale = disps[0].autoscale != 0;
  const size_t bins_z = (size_t)bins;

  // every stream's own route
  std::vector<RaggedColsEntry> all = glfer::ragged_streams(row_starts, nstreams), fused_s, staged_s;
  bool tiled = false;
  for (const RaggedColsEntry &e : all) {
    bool fused = false;
    size_t tile = 0;
    waterfall_route(avg_mode, depth, minbin, maxbin, bins, pitch, (size_t)e.nframes, &fused, &tile);
    if (tile < (size_t)e.nframes) tiled = true;
    if (averaging) (fused ? fused_s : staged_s).push_back(e);
  }
  if (tiled) {
    // stream by stream through the single entry (on copies: an error leaves disps as it was)
    std::vector<glfer_hip_display> copy(disps, disps + nstreams);
    for (const RaggedColsEntry &e : all) {
      const size_t r = (size_t)e.row0;
      rc = waterfall_columns(&copy[e.stream], avg_mode, depth, minbin, maxbin, max0, d_psd + r * (size_t)pitch, 0, (size_t)e.nframes,
                             bins, d_rgb + r * bins_z * 3, d_lev ? d_lev + r * bins_z : nullptr, d_stats ? d_stats + r * 4 : nullptr,
                             st, nullptr, pitch);
      if (rc != GLFER_OK) return rc;
    }
    std::copy(copy.begin(), copy.end(), disps);
    return GLFER_OK;
  }
  const DisplayOptions o(disps[0]);
  DisplayTable t(st);
  HIP_TRY(display_table_upload(disps, nstreams, &t));
  auto fail = [&](hipError_t err, const char *what) {
    if (rc == GLFER_OK) rc = hip_fail(err, what);
  };

  // scratch, indexed by packed row: statistics, levels; the chunk states of the walks; a group's averaged rows
  size_t st_floats = 0;
  if (autoscale)
    for (const RaggedColsEntry &x : all) st_floats += glfer_levels_scratch_floats((size_t)x.nframes);
  // staged: groups of streams whose averaged rows stay within the single entry's 4 GiB (one stream alone always goes)
  const size_t group_rows_max = std::max<size_t>(1, ((size_t)4 << 30) / (bins_z * sizeof(double)));
  std::vector<size_t> group_end;                          // staged_s[group_end[g-1] .. group_end[g])
  size_t scratch_rows = 0;
  for (size_t i = 0, in_group = 0; i < staged_s.size(); i++) {
    const size_t n = (size_t)staged_s[i].nframes;
    if (in_group && in_group + n > group_rows_max) {
      group_end.push_back(i);
      in_group = 0;
    }
    staged_s[i].out0 = (long long)in_group;               // the averaged rows of a group are packed on their own
    in_group += n;
    scratch_rows = std::max(scratch_rows, in_group);
    if (i + 1 == staged_s.size()) group_end.push_back(i + 1);
  }
  WaterfallScratch s(st);
  hipError_t e = waterfall_scratch_take(&s, d_stats, rows_hi, rows_hi * 4 + st_floats, scratch_rows, bins_z);
  if (e != hipSuccess) fail(e, "scratch (waterfall, ragged)");
  float *stats = s.stats, *levels = s.levels.get(), *chunk_state = levels ? levels + rows_hi * 4 : nullptr;

  // compute_floor of every row: the packed rows are one run
  if (rc == GLFER_OK) {
    e = glfer::floor_rows(d_psd + rows_lo * (size_t)pitch, rows_hi - rows_lo, bins, pitch, stats + rows_lo * 4, st);
    if (e != hipSuccess) fail(e, "compute_floor launch (ragged)");
  }
  if (rc == GLFER_OK) {
    if (autoscale) {
      e = glfer_launch_levels_ragged(stats, all.data(), all.size(), o.scale_log, disps[0].overlap, t.d_state, levels, chunk_state, st);
      if (e != hipSuccess) fail(e, "level tracking launch (ragged)");
    } else {
      e = glfer_launch_levels_fixed(rows_hi - rows_lo, o.dmax, o.dmin, o.mx, o.mn, levels + rows_lo * 4, st);
      if (e != hipSuccess) fail(e, "levels launch (ragged)");
    }
  }
  if (rc == GLFER_OK && !averaging) {
    const size_t map_piece = (size_t)1 << 30;
    for (size_t r0 = rows_lo; rc == GLFER_OK && r0 < rows_hi; r0 += map_piece) {
      e = glfer_launch_map(d_psd + r0 * (size_t)pitch, nullptr, std::min(map_piece, rows_hi - r0), bins, pitch, o.scale_log, o.thr255,
                           o.one_m_thr, levels + r0 * 4, t.d_tab, t.d_thr, d_rgb + r0 * bins_z * 3, d_lev ? d_lev + r0 * bins_z : nullptr, st);
      if (e != hipSuccess) fail(e, "map launch (ragged)");
    }
  }
  if (rc == GLFER_OK && !fused_s.empty()) {
    e = glfer_launch_avgmap_ragged(avg_mode, d_psd, fused_s.data(), fused_s.size(), bins, depth, minbin, maxbin, max0 ? 1 : 0, o.scale_log,
                                   o.thr255, o.one_m_thr, levels, t.d_tab, t.d_thr, d_rgb, d_lev, st);
    if (e != hipSuccess) fail(e, "average-and-map launch (ragged)");
  }
  for (size_t g = 0, i0 = 0; rc == GLFER_OK && g < group_end.size(); i0 = group_end[g++]) {
    const RaggedColsEntry *gs = staged_s.data() + i0;
    const size_t gn = group_end[g] - i0;
    // (update_avg's `bins` is its rows' stride; the band is minbin..maxbin, the averaged rows are dense)
    e = glfer_launch_avg_ragged(avg_mode, d_psd, gs, gn, pitch, bins, depth, minbin, maxbin, max0 ? 1 : 0, s.avg.get(), s.ret.get(), st);
    if (e != hipSuccess) fail(e, "update_avg launch (ragged waterfall)");
    if (rc == GLFER_OK) {
      e = glfer_launch_map_ragged(s.avg.get(), gs, gn, bins, o.scale_log, o.thr255, o.one_m_thr, levels, t.d_tab, t.d_thr, d_rgb, d_lev, st);
      if (e != hipSuccess) fail(e, "map launch (ragged waterfall)");
    }
  }
  // (a stream without rows keeps its display as it is)
  return waterfall_batch_finish(rc, disps, nstreams, &all, o, t, s, st, "glfer_hip_waterfall_ragged_device");
}

}  // extern "C"
