// c_plan_tables.cpp -- every host table of a plan (glfer_amd/csrc/plan_tables.h) over a grid of configurations, the smallest size
// that reaches each branch of the builders: one line per table with the configuration, the table's name, its length and the
// 64-bit FNV-1a hash of its bytes, and one line per scalar the plan keeps.  tests/golden/plan_tables.txt holds the same lines
// as the plan made them before the builders had names; tests/test_plan_tables_host.py requires equality line by line.
// Built with g++ against plan_tables.cpp and host_tables.cpp only: no GPU, no HIP runtime.
#include "plan_tables.h"

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

namespace {

struct Case {
  int mode, n, window;
  float limiter_a;
  int enable_limiter, sub_mean, mtm_k;
  float mtm_w;
  int t, p_e, lmp_av, width;
  bool ftest;
};

Case fft(int n, int window, float a = 0.0f) { return Case{GLFER_MODE_FFT, n, window, a, 0, 0, 0, 0.0f, 0, 0, 0, 8, false}; }
Case mtm(int n, int kmax, bool ftest = false, int sub_mean = 0) {
  return Case{GLFER_MODE_MTM, n, GLFER_WIN_RECTANGULAR, 0.0f, 0, sub_mean, kmax, 2.5f, 0, 0, 0, 8, ftest};
}
Case hparma(int n, int t, int p_e, int width) { return Case{GLFER_MODE_HPARMA, n, GLFER_WIN_RECTANGULAR, 0.0f, 0, 0, 0, 0.0f, t, p_e, 0, width, false}; }

std::vector<Case> grid() {
  std::vector<Case> g;
  // FFT: the small layout (8, 128), packed only (256), h (512), h and w (2048), w alone with the taps placeholder and the 4N
  // scale (32768), wcomb of two floats (65536)
  for (int window : {GLFER_WIN_RECTANGULAR, GLFER_WIN_HANNING})
    for (int n : {8, 128, 256, 512, 2048, 32768, 65536}) g.push_back(fft(n, window));
  // RA9MB: unscaled taps and no h, no w (512); unscaled w (32768)
  g.push_back(fft(512, GLFER_WIN_HANNING, 0.5f));
  g.push_back(fft(32768, GLFER_WIN_HANNING, 0.5f));
  // LMP with a Hann window and a limiter in the configuration: both overridden
  g.push_back(Case{GLFER_MODE_LMP, 512, GLFER_WIN_HANNING, 0.5f, 1, 0, 0, 0.0f, 0, 0, 4, 8, false});
  // MTM, w = 2.5: 4 tapers (no x); 3 and 5 tapers (x, l); 5 at 4096 (x, l, y, the queue); 7 at 4096 (l dropped by the 80 KiB
  // gate); 5 at 2048 (w with tapers); 5 at 8192 (h multitaper); 5 at 32768 (no packed table); one taper; and one plan with mean
  // removal, whose I/Q and adaptive tables are refused.  The F-test's tables: 5 tapers at 256 and 2048, 4 tapers at 256.
  g.push_back(mtm(256, 3, true));
  g.push_back(mtm(256, 2));
  g.push_back(mtm(256, 4, true));
  g.push_back(mtm(256, 4, false, GLFER_SUBMEAN_EXACT));   // (the same tapers again: from the cache)
  g.push_back(mtm(4096, 4));
  g.push_back(mtm(4096, 6));
  g.push_back(mtm(2048, 4, true));
  g.push_back(mtm(8192, 4));
  g.push_back(mtm(32768, 4));
  g.push_back(mtm(256, 0));
  // HP-ARMA: the smallest plan; 33 columns at both schedule widths (80 and 63 steps); 65 columns (no schedule)
  g.push_back(hparma(32, 8, 3, 8));
  g.push_back(hparma(256, 64, 32, 8));
  g.push_back(hparma(256, 64, 32, 16));
  g.push_back(hparma(256, 128, 64, 8));
  return g;
}

glfer_hip_config config_of(const Case &c) {
  glfer_hip_config cfg;
  memset(&cfg, 0, sizeof cfg);
  cfg.mode = c.mode;
  cfg.n = c.n;
  cfg.overlap = 0.5f;
  cfg.window_type = c.window;
  cfg.limiter_a = c.limiter_a;
  cfg.enable_limiter = c.enable_limiter;
  cfg.sub_mean = c.sub_mean;
  cfg.mtm_w = c.mtm_w;
  cfg.mtm_k = c.mtm_k;
  cfg.hparma_t = c.t;
  cfg.hparma_p_e = c.p_e;
  cfg.lmp_av = c.lmp_av;
  return cfg;
}

std::string tag_of(const Case &c) {
  char buf[256];
  snprintf(buf, sizeof buf, "mode=%d,n=%d,win=%d,a=%g,lim=%d,submean=%d,k=%d,w=%g,t=%d,pe=%d,lmp=%d,width=%d", c.mode, c.n, c.window,
           (double)c.limiter_a, c.enable_limiter, c.sub_mean, c.mtm_k, (double)c.mtm_w, c.t, c.p_e, c.lmp_av, c.width);
  return buf;
}

template <class T>
void table(const std::string &tag, const char *name, const std::vector<T> &v) {
  uint64_t h = 14695981039346656037ull;
  const unsigned char *b = reinterpret_cast<const unsigned char *>(v.data());
  for (size_t i = 0; i < v.size() * sizeof(T); i++) h = (h ^ b[i]) * 1099511628211ull;
  printf("%s %s %zu %016llx\n", tag.c_str(), name, v.size(), (unsigned long long)h);
}
void scalar(const std::string &tag, const char *name, double v) { printf("%s %s = %a\n", tag.c_str(), name, v); }

}  // namespace

int main() {
  for (const Case &c : grid()) {
    const std::string tag = tag_of(c);
    const glfer_hip_config cfg = config_of(c);
    if (glfer::plan_config_ok(&cfg) != GLFER_OK) {
      printf("%s refused\n", tag.c_str());
      return 1;
    }
    glfer::PlanTables t;
    if (glfer::build_plan_tables(cfg, c.width, &t) != GLFER_OK) {
      printf("%s failed\n", tag.c_str());
      return 1;
    }
    scalar(tag, "ntapers", t.ntapers);
    scalar(tag, "npairs", t.npairs);
    scalar(tag, "htapers", t.htapers);
    scalar(tag, "wtapers", t.wtapers);
    scalar(tag, "spec_unscale", t.spec_unscale);
    scalar(tag, "nonlin", t.nonlin);
    scalar(tag, "rot_steps", t.rot_steps);
    scalar(tag, "window_type", t.cfg.window_type);
    scalar(tag, "limiter_a", t.cfg.limiter_a);
    scalar(tag, "enable_limiter", t.cfg.enable_limiter);
    table(tag, "window", t.window);
    table(tag, "tapers", t.tapers);
    table(tag, "sig", t.sig);
    table(tag, "taps", t.taps);
    table(tag, "tw", t.tw);
    table(tag, "htaps", t.htaps);
    table(tag, "htw", t.htw);
    table(tag, "hrot", t.hrot);
    table(tag, "wtaps", t.wtaps);
    table(tag, "wtw", t.wtw);
    table(tag, "wcomb", t.wcomb);
    table(tag, "bigtw", t.bigtw);
    table(tag, "xtaps", t.xtaps);
    table(tag, "ytaps", t.ytaps);
    table(tag, "ltaps", t.ltaps);
    table(tag, "iqtaps", t.iqtaps);
    table(tag, "ataps", t.ataps);
    table(tag, "lagmap", t.lagmap);
    table(tag, "rot_sched", t.rot_sched);
    table(tag, "unit", t.unit);
    if (c.ftest) {
      glfer::FtestTables f;
      glfer::build_ftest_tables(c.n, t.ntapers, t.tapers.data(), t.sig.data(), &f);
      scalar(tag, "sum_U0_sqr", f.sum_U0_sqr);
      scalar(tag, "hn_scale", f.hn_scale);
      table(tag, "U0", f.U0);
      table(tag, "hn", f.hn);
      table(tag, "ftaps", f.taps);
      table(tag, "cj", f.cj);
      table(tag, "ftaps2", f.paired);
    }
  }
  return 0;
}
