// plan.cpp -- the plan of include/glfer_hip.h: check the configuration, build its host tables (plan_tables.h), upload them.
// Also the F-test's lazy second half of the plan, and the entries that hand a plan's host tables to tests.
#include "plan.h"

#include <cstdlib>
#include <cstring>
#include <new>

#include "host_tables.h"
#include "plan_tables.h"
#include "spectro_params.h"

using glfer::DeviceGuard;
using glfer::DeviceTable;
using glfer::hip_fail;

extern "C" {

int glfer_hip_plan_create(const glfer_hip_config *cfg, glfer_hip_plan **out) {
  if (!cfg || !out) return GLFER_E_ARG;
  *out = nullptr;
  if (const int rc = glfer::plan_config_ok(cfg); rc != GLFER_OK) return rc;

  // --- host tables
  // GLFER_HPARMA_WIDTH=16: sixteen rotations per step of the Jacobi schedule, each over 4 lanes (A/B runs)
  const int rot_width = [] { const char *e = getenv("GLFER_HPARMA_WIDTH"); return e && atoi(e) == 16 ? 16 : 8; }();
  glfer::PlanTables t;
  if (const int rc = glfer::build_plan_tables(*cfg, rot_width, &t); rc != GLFER_OK) return rc;
  glfer_hip_plan *p = new (std::nothrow) glfer_hip_plan();
  if (!p) return GLFER_E_NOMEM;
  p->cfg = t.cfg;
  p->n = cfg->n;
  p->hop = t.hop;
  p->keep = t.keep;
  p->bins = t.bins;
  p->lanes = cfg->n / 16;
  p->pitch = t.pitch;
  p->lmp_av = t.lmp_av;
  p->ntapers = t.ntapers;
  p->npairs = t.npairs;
  p->htapers = t.htapers;
  p->wtapers = t.wtapers;
  p->rot_steps = t.rot_steps;
  p->rot_width = rot_width;
  p->spec_unscale = t.spec_unscale;
  p->nonlin = t.nonlin;
  p->window = std::move(t.window);
  p->tapers = std::move(t.tapers);
  p->sig = std::move(t.sig);

  // --- device tables: every table the plan has, and nothing for an empty one
  DeviceGuard guard(cfg->device);
  hipError_t e = guard.error();
  auto up = [&e](auto &table, const auto &host) {
    if (e == hipSuccess && !host.empty()) e = table.upload(host);
  };
  up(p->d_taps, t.taps);
  if (cfg->mode == GLFER_MODE_FFT && cfg->window_type != GLFER_WIN_RECTANGULAR) up(p->d_window, p->window);   // prepare_audio's multiply, fft.c:139-146
  up(p->d_tw, t.tw);
  up(p->d_htaps, t.htaps);
  up(p->d_htw, t.htw);
  up(p->d_hrot, t.hrot);
  up(p->d_wtaps, t.wtaps);
  up(p->d_wtw, t.wtw);
  up(p->d_wcomb, t.wcomb);
  up(p->d_bigtw, t.bigtw);
  up(p->d_xtaps, t.xtaps);
  up(p->d_ytaps, t.ytaps);
  up(p->d_iqtaps, t.iqtaps);
  up(p->d_ataps, t.ataps);
  if (e == hipSuccess && !t.xtaps.empty() && p->n == 4096) {      // spectro16y.hip's ticket counters, zeroed once
    p->yq.reset(new glfer_yqueue);
    up(p->yq->d_counters, std::vector<unsigned>((size_t)glfer_yqueue::SLOTS * glfer_yqueue::PITCH, 0u));
  }
  up(p->d_ltaps, t.ltaps);
  up(p->d_lagmap, t.lagmap);
  up(p->d_rot_sched, t.rot_sched);
  up(p->d_unit, t.unit);
  if (e != hipSuccess) {
    int rc = hip_fail(e, "plan_create");
    glfer_hip_plan_destroy(p);
    return rc;
  }
  *out = p;
  return GLFER_OK;
}

void glfer_hip_plan_destroy(glfer_hip_plan *p) {
  if (!p) return;
  DeviceGuard guard(p->cfg.device);
  glfer::ingest_ring_free(p->ring);
  for (hipStream_t a : p->aux)
    if (a) (void)hipStreamDestroy(a);
  for (hipEvent_t ev : p->aux_events) (void)hipEventDestroy(ev);
  delete p;                                                        // (its DeviceTables free themselves, on the plan's device)
}

int glfer_hip_hop(const glfer_hip_plan *p) { return p ? p->hop : GLFER_E_ARG; }
int glfer_hip_bins(const glfer_hip_plan *p) { return p ? p->bins : GLFER_E_ARG; }
int glfer_hip_num_tapers(const glfer_hip_plan *p) { return p ? p->ntapers : GLFER_E_ARG; }
size_t glfer_hip_num_frames(const glfer_hip_plan *p, size_t nsamples) {
  return p ? nsamples / (size_t)p->hop : 0;
}

int glfer_hip_get_window(const glfer_hip_plan *p, float *w) {
  if (!p || !w) return GLFER_E_ARG;
  memcpy(w, p->window.data(), (size_t)p->n * sizeof(float));
  return GLFER_OK;
}

int glfer_hip_get_tapers(const glfer_hip_plan *p, double *tapers, double *sig) {
  if (!p || p->cfg.mode != GLFER_MODE_MTM) return GLFER_E_ARG;
  if (tapers) memcpy(tapers, p->tapers.data(), p->tapers.size() * sizeof(double));
  if (sig) memcpy(sig, p->sig.data(), p->sig.size() * sizeof(double));
  return GLFER_OK;
}

int glfer_hip_make_window(int window_type, int n, float *window) {
  if (!window || n < 2 || window_type < 0 || window_type > 7) return GLFER_E_ARG;
  glfer::make_window(window_type, n, window);
  return GLFER_OK;
}

int glfer_hip_y_half_tables(int n, int kmax, double nw, float *half, float *pairs, float *last) {
  if (!half || n != 4096 || kmax != 4 || !(nw > 0.0)) return GLFER_E_ARG;
  const int nt = kmax + 1;
  std::vector<double> tapers((size_t)nt * n), sig(nt);
  if (!glfer::make_dpss(n, kmax, nw, tapers.data(), sig.data())) return GLFER_E_NUMERIC;
  std::vector<float> taps((size_t)2 * ((nt + 1) / 2) * n, 0.0f), xtaps((size_t)n);
  glfer::mtm_pair_tables(n, nt, tapers.data(), sig.data(), taps.data());
  glfer::mtm_last_table(n, nt, tapers.data(), sig.data(), xtaps.data());
  if (pairs) memcpy(pairs, taps.data(), (size_t)4 * n * sizeof(float));
  if (last) memcpy(last, xtaps.data(), (size_t)n * sizeof(float));
  return glfer::build_y_half_table(n, taps.data(), xtaps.data(), half) ? 1 : 0;
}

int glfer_hip_iq_supported(const glfer_hip_config *cfg) { return glfer::iq_config_ok(cfg); }

int glfer_hip_iq_tables(const glfer_hip_config *cfg, float *table) {
  if (glfer_hip_iq_supported(cfg) != GLFER_OK) return GLFER_E_ARG;
  const int n = cfg->n;
  if (cfg->mode == GLFER_MODE_FFT) {
    if (cfg->window_type < 0 || cfg->window_type > 7) return GLFER_E_ARG;
    if (!table) return 1;
    std::vector<float> w(n);
    glfer::make_window(cfg->window_type, n, w.data());
    glfer::make_iq_table(n, 1, cfg->window_type == GLFER_WIN_RECTANGULAR ? nullptr : w.data(), nullptr, nullptr, table);
    return 1;
  }
  if (cfg->mtm_k < 0 || cfg->mtm_k > 31 || !(cfg->mtm_w > 0.0f)) return GLFER_E_ARG;
  const int nt = cfg->mtm_k + 1;
  if (!table) return nt;
  std::vector<double> tapers((size_t)nt * n), sig(nt);
  if (!glfer::make_dpss(n, cfg->mtm_k, (double)cfg->mtm_w, tapers.data(), sig.data())) return GLFER_E_NUMERIC;
  glfer::make_iq_table(n, nt, nullptr, tapers.data(), sig.data(), table);
  return nt;
}

void glfer_hip_y_queue_shape(int *blocks, int *chunk) {
  if (blocks) *blocks = GLFER_YQ_BLOCKS;
  if (chunk) *chunk = GLFER_YQ_CHUNK;
}

int glfer_hip_make_dpss(int n, int kmax, double nw, double *tapers, double *sig) {
  if (!tapers || !sig || n < 2 || kmax < 0 || kmax > 31 || !(nw > 0.0)) return GLFER_E_ARG;
  return glfer::make_dpss(n, kmax, nw, tapers, sig) ? GLFER_OK : GLFER_E_NUMERIC;
}

}  // extern "C"

// The caller has the plan's device current.  Every table is uploaded into a local owner first; the plan takes them, and its
// alias pointers are set, only when all three are there.
int ftest_tables(glfer_hip_plan *p) {
  std::lock_guard<std::mutex> lock(p->ftest_mu);
  if (p->d_ftaps) return GLFER_OK;       // tables of mtm.c:76-83, 124-136, once per plan
  const int n = p->n, T = p->ntapers;
  glfer::FtestTables f;
  glfer::build_ftest_tables(n, T, p->tapers.data(), p->sig.data(), &f);
  // [U0: T doubles][c_j: T floats] in one allocation
  std::vector<double> u0_cj((size_t)T + ((size_t)T + 1) / 2, 0.0);
  memcpy(u0_cj.data(), f.U0.data(), (size_t)T * sizeof(double));
  memcpy(u0_cj.data() + T, f.cj.data(), (size_t)T * sizeof(float));
  DeviceTable<float> taps, paired;
  DeviceTable<double> u0;
  hipError_t e = taps.upload(f.taps);
  if (e == hipSuccess) e = u0.upload(u0_cj);
  if (e == hipSuccess) e = paired.upload(f.paired);
  if (e != hipSuccess) return hip_fail(e, "ftest tables");
  p->sum_U0_sqr = f.sum_U0_sqr;
  p->hn_scale = f.hn_scale;
  p->d_ftaps_mu_first = std::move(taps);
  p->d_U0 = std::move(u0);
  p->d_rows_cj = reinterpret_cast<float *>(p->d_U0.get() + T);
  p->d_ftaps2 = std::move(paired);
  p->d_ftaps2_nomu = p->d_ftaps2.get() + (size_t)f.r_mu * 2 * n;
  p->d_ftaps = p->d_ftaps_mu_first.get() + (size_t)2 * n;
  return GLFER_OK;
}
