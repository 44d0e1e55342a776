// plan_tables.h -- the host side of a plan: the configuration checks and every table a plan uploads, one named builder per
// device layout.  Host code with no HIP runtime call (plan.cpp uploads what these return), built with host_tables.o's flags:
// the tables are reproducible bit for bit (tests/c_plan_tables.cpp prints them against tests/golden/plan_tables.txt).
#pragma once
#include "../../include/glfer_hip.h"

#include <stddef.h>
#include <stdint.h>

#include <vector>

namespace glfer {

// ---- one builder per layout.  The sources of a table's rows, where a builder takes them as (ntap, window, tapers, sig): tapers
// [ntap][n] with sig [ntap] (multitaper), or tapers NULL and ntap = 1 for the periodogram's window [n] (NULL: rectangular, which the
// reference never multiplies by -- ones, fft.c:132,139)
size_t tap_slot(int n, int pair, int i, int which);
void periodogram_pair_table(int n, const float *window, bool nonlin, double scale, float *taps);   // [2n], zeroed by the caller
void mtm_pair_tables(int n, int ntapers, const double *tapers, const double *sig, float *taps);
void mtm_last_table(int n, int ntapers, const double *tapers, const double *sig, float *xtaps);
bool build_y_half_table(int n, const float *taps, const float *xtaps, float *half);
std::vector<float> h_tables(int n, int ntap, const float *window, const double *tapers, const double *sig);
std::vector<float> h_rotations(int n);
std::vector<float> w_tables(int n, int ntap, const float *window, const double *tapers, const double *sig, bool nonlin);
std::vector<float> w_combine_twiddles(int n);
std::vector<float> big_register_twiddles(int n);
std::vector<float> lds_half_tables(int n, int ntapers, const double *tapers, const double *sig);   // empty: not symmetric, or too large
std::vector<float> lane_order_rows(int n, int rows_in, int rows_out, const float *flat);           // the I/Q and adaptive tables' order
std::vector<float> twiddles16(int logn, int lanes);
std::vector<uint16_t> hparma_lag_map(int t, int ncol);
std::vector<float> unit_circle(int n);
std::vector<int> jacobi_schedule(int ncol, int width);                                              // empty: more than 64 columns

// The F-test's tables (mtm.c:76-83, 124-136), made on the first F call of a plan
struct FtestTables {
  std::vector<double> U0;        // [T]
  std::vector<float> hn;         // [n]
  float sum_U0_sqr = 0.0f;
  float hn_scale = 1.0f;         // the power of two hn is multiplied by in `paired` (see SpectroParams::ft_mu_unscale)
  std::vector<float> taps;       // [hn][taper 0..T-1][hn], each [2n] alone in slot 0 of the packed layout
  std::vector<float> cj;         // [T] 1 / (n (1 + sig_j)): the rows' weights of the rows-and-F entries
  std::vector<float> paired;     // [r_mu][2n] with (hn_scale hn, taper 0), (taper 1, taper 2) ... halved, then [ceil(T/2)][2n] without hn
  int r_mu = 0;                  // ceil((T+1)/2): the rows of `paired` that come before the block without mu
};
void build_ftest_tables(int n, int T, const double *tapers, const double *sig, FtestTables *out);

// ---- a plan's host half
// What glfer_hip_iq_supported / glfer_hip_adaptive_supported answer (GLFER_OK or GLFER_E_ARG): which plans carry those tables
int iq_config_ok(const glfer_hip_config *cfg);
int adaptive_config_ok(const glfer_hip_config *cfg);

// gl_dpss through the cache of the last four results (the same doubles, bit for bit); false: the eigen-solve did not converge
bool cached_dpss(int n, int kmax, float w, std::vector<double> *tapers, std::vector<double> *sig);

// The tables of a plan and the scalars it keeps.  An empty vector: this plan has no such table.
struct PlanTables {
  glfer_hip_config cfg;            // the configuration as the plan runs it (LMP: rectangular window, no limiter)
  int hop = 0, keep = 0, bins = 0, pitch = 0, lmp_av = 0;
  int ntapers = 0, npairs = 0, htapers = 0, wtapers = 0, rot_steps = 0;
  float spec_unscale = 1.0f;
  bool nonlin = false;
  std::vector<float> window;       // [n] as the reference stores it (unit power)
  std::vector<double> tapers, sig; // [ntapers][n], [ntapers]
  std::vector<float> taps, tw, htaps, htw, hrot, wtaps, wtw, wcomb, bigtw, xtaps, ytaps, ltaps, iqtaps, ataps, unit;
  std::vector<uint16_t> lagmap;
  std::vector<int> rot_sched;
};
int plan_config_ok(const glfer_hip_config *cfg);     // glfer_hip_plan_create's refusals, in its order: GLFER_OK or the code
// cfg has passed plan_config_ok.  rot_width: rotations a step of the Jacobi schedule holds (8 or 16).  GLFER_OK or GLFER_E_NUMERIC
int build_plan_tables(const glfer_hip_config &cfg, int rot_width, PlanTables *out);

}  // namespace glfer
