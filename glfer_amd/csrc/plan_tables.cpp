// plan_tables.cpp -- the host half of a plan: configuration checks and table builders (plan_tables.h).  No HIP runtime call.
//
// A plan is what fft_init()/mtm_init() build in the reference (fft.c:168-187, mtm.c:88-151): window or DPSS tapers, here laid
// out for the kernels with the 1/N normalisation (fft.c:212-216), the eigenvalue weights 1/(1+sig_j) (mtm.c:214-219) and the
// 1/2 of the re/im packing folded in, so the kernel's epilogue is a single add.
#include "plan_tables.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <mutex>
#include <utility>

#include "host_tables.h"
#include "hparma_frames.h"
#include "spectro_adaptive_params.h"
#include "spectro_params.h"

namespace glfer {

static const double kTwoPi = 2.0 * 3.14159265358979323846;

static bool is_pow2(int n) { return n > 0 && (n & (n - 1)) == 0; }

// sample i under row j of a table's sources (plan_tables.h): taper j, or the periodogram's window, or one
static double source(int n, int j, int i, const float *window, const double *tapers) {
  return tapers ? tapers[(size_t)j * n + i] : (window ? (double)window[i] : 1.0);
}

// Device layout of the taper tables, the order the kernel's lanes read them in: sample i of a
// frame belongs to lane t = i mod T at register m = i / T (T = n/16 lanes per frame); a lane
// fetches registers m, m+1 of both tapers of a pair with one 16-byte load:
//   taps[pair][m/2][t][4] = { taper 2p @m, taper 2p+1 @m, taper 2p @m+1, taper 2p+1 @m+1 }
size_t tap_slot(int n, int pair, int i, int which) {
  if (n < 256) return ((size_t)pair * n + i) * 2 + which;       // spectro_small.hip: [pair][i][2]
  const int T = n / 16, t = i % T, m = i / T;
  return (size_t)pair * n * 2 + ((size_t)(m / 2) * T + t) * 4 + (size_t)(m & 1) * 2 + which;
}

// The periodogram's one pair: taps[pair][i] = (taper 2*pair, taper 2*pair+1)[i], interleaved, the second of the pair zeros.
// psd = |X|^2/N (fft.c:212-216): `scale` on every sample, or the plain window where RA9MB / the limiter act first (nonlin)
void periodogram_pair_table(int n, const float *window, bool nonlin, double scale, float *taps) {
  for (int i = 0; i < n; i++) {
    const double w = source(n, 0, i, window, nullptr);             // fft.c:132,139: no multiply when rectangular
    taps[tap_slot(n, 0, i, 0)] = nonlin ? (float)w : (float)(w * scale);
  }
}

// spectro16y.hip's half-table form (five tapers at N = 4096): what a lane keeps in registers, from the tables the plan
// builds for the full-table form -- taps (the two pairs, tap_slot layout) and xtaps (the last taper, [4][n/16][4]).
// DPSS tapers are symmetric (even order) or antisymmetric (odd order) about the frame centre; the half table is built only
// if the SCALED FLOATS have that symmetry exactly (a == b, a == -b as float comparisons: a zero of either sign gives a
// product that is a zero either way, and no sum or power can tell them apart), because rows from half tables must be the
// full-table form's rows bit for bit.  Layout: spectro_params.h, glfer_yhalf_residue().  false: `half` is left alone.
bool build_y_half_table(int n, const float *taps, const float *xtaps, float *half) {
  if (n != 4096) return false;
  const int T = n / 16;
  auto last = [&](int i) { return xtaps[((size_t)((i / T) / 4) * T + (size_t)(i % T)) * 4 + (size_t)((i / T) & 3)]; };
  for (int i = 0; i < n / 2; i++) {
    for (int j = 0; j < 4; j++) {
      const float a = taps[tap_slot(n, j / 2, i, j & 1)], b = taps[tap_slot(n, j / 2, n - 1 - i, j & 1)];
      if (!((j & 1) ? b == -a : b == a)) return false;
    }
    if (!(last(n - 1 - i) == last(i))) return false;
  }
  for (int t = 0; t < T; t++) {
    const int r = (int)glfer_yhalf_residue((unsigned)t);
    float *row = half + (size_t)t * GLFER_YHALF_FLOATS;
    for (int m = 0; m < 8; m++) {
      for (int j = 0; j < 4; j++) row[16 * (j / 2) + 2 * m + (j & 1)] = taps[tap_slot(n, j / 2, r + T * m, j & 1)];
      row[32 + m] = last(r + T * m);
    }
  }
  return true;
}

// The scaled float tables of a multitaper plan with an odd taper count: the pairs (taps, tap_slot layout:
// psd += |FFT(v_j x)|^2 / N / (1+sig_j), mtm.c:212-219, and the 1/2 of the packing) and the last taper alone (xtaps,
// [4][n/16][4]; |Y|^2 = |E|^2/4 in the shared transform, so its scale carries 1/4 instead of 1/2).
void mtm_pair_tables(int n, int ntapers, const double *tapers, const double *sig, float *taps) {
  for (int j = 0; j < ntapers; j++) {
    const double scale = std::sqrt(1.0 / (2.0 * n * (1.0 + sig[j])));
    for (int i = 0; i < n; i++)
      taps[tap_slot(n, j / 2, i, j & 1)] = (float)(tapers[(size_t)j * n + i] * scale);
  }
}
void mtm_last_table(int n, int ntapers, const double *tapers, const double *sig, float *xtaps) {
  const int T = n / 16, j = ntapers - 1;
  const double scale = std::sqrt(1.0 / (4.0 * n * (1.0 + sig[j])));
  for (int i = 0; i < n; i++) {
    const int t = i % T, m = i / T;
    xtaps[((size_t)(m / 4) * T + t) * 4 + (size_t)(m & 3)] = (float)(tapers[(size_t)j * n + i] * scale);
  }
}

// [slots][lanes] (cos,sin): the twiddles of a 2^logn-point transform at 16 points a lane
std::vector<float> twiddles16(int logn, int lanes) {
  std::vector<float> tw((size_t)2 * make_twiddles16(logn, nullptr) * lanes, 0.0f);
  make_twiddles16(logn, tw.data());
  return tw;
}

// Real-input form of the linear periodogram (spectro16h.hip): z[i] = y[2i] + i*y[2i+1], lane t of n/32 holds points
// i = t + (n/32)*m; |X|^2/N needs the inputs scaled by sqrt(1/(4N)).  [ntap][8][n/32][4].
// Multitaper at N >= 8192 takes the same form, one taper after the other on the frame held in registers: the packed N-point
// form would need the whole N-point exchange buffer (139 KB at N = 16384: one workgroup per CU), the real-input form half of
// it.  Each taper carries its weight: sqrt(1 / (4N (1 + sig_j))).
std::vector<float> h_tables(int n, int ntap, const float *window, const double *tapers, const double *sig) {
  const int th = n / 32;
  std::vector<float> htaps((size_t)ntap * n);
  for (int j = 0; j < ntap; j++) {
    const double scale = std::sqrt(1.0 / (4.0 * n * (tapers ? 1.0 + sig[j] : 1.0)));
    for (int m = 0; m < 16; m++)
      for (int t = 0; t < th; t++)
        for (int e = 0; e < 2; e++) {
          const int i = 2 * (t + th * m) + e;
          htaps[(size_t)j * n + ((size_t)(m / 2) * th + t) * 4 + (size_t)(m & 1) * 2 + e] = (float)(source(n, j, i, window, tapers) * scale);
        }
  }
  return htaps;
}
// (cos,sin)(2 pi t/n), t < n/32: the real-input form's split rotation
std::vector<float> h_rotations(int n) {
  const int th = n / 32;
  std::vector<float> hrot((size_t)2 * th);
  for (int t = 0; t < th; t++) {
    const double ang = kTwoPi * t / n;
    hrot[2 * t] = (float)std::cos(ang);
    hrot[2 * t + 1] = (float)std::sin(ang);
  }
  return hrot;
}

// The same real-input form with wavefront-private 1024-point sub-transforms (spectro16w.hip), N >= 2048: z index
// n = W*(t + 64 m) + w for wavefront w, lane t, register m.  [ntap][W][8][64][4].
// nonlin (RA9MB / limiter, N = 32768 only): the plain window, the scale follows the limiter as post_scale
std::vector<float> w_tables(int n, int ntap, const float *window, const double *tapers, const double *sig, bool nonlin) {
  const int W = n / 2 / 1024;
  std::vector<float> wtaps((size_t)ntap * n);
  for (int j = 0; j < ntap; j++) {
    const double scale = std::sqrt(1.0 / (4.0 * n * (tapers ? 1.0 + sig[j] : 1.0)));
    for (int w = 0; w < W; w++)
      for (int m = 0; m < 16; m++)
        for (int t = 0; t < 64; t++)
          for (int e = 0; e < 2; e++) {
            const int i = 2 * (W * (t + 64 * m) + w) + e;
            const double v = source(n, j, i, window, tapers);
            wtaps[((((size_t)j * W + w) * 8 + m / 2) * 64 + t) * 4 + (size_t)(m & 1) * 2 + e] = (float)(nonlin ? v : v * scale);
          }
  }
  return wtaps;
}
// the wavefront-private form's combine / split twiddles per lane; N >= 65536 computes them in the kernels (two floats stand in)
std::vector<float> w_combine_twiddles(int n) {
  const int M = n / 2, W = M / 1024, LF = 64 * W, IPL = LF <= 512 ? 512 / LF : 1;
  std::vector<float> wcomb(n <= 32768 ? (size_t)2 * IPL * W * LF : 2);
  for (int i = 0; i < IPL && n <= 32768; i++)
    for (int ww = 0; ww < W; ww++)
      for (int u = 0; u < LF; u++) {
        const long long k1 = u + (long long)LF * i;
        const double ang = ww == 0 ? kTwoPi * (double)k1 / n : kTwoPi * (double)((ww * k1) % M) / M;
        wcomb[2 * ((size_t)(i * W + ww) * LF + u)] = (float)std::cos(ang);
        wcomb[2 * ((size_t)(i * W + ww) * LF + u) + 1] = (float)std::sin(ang);
      }
  return wcomb;
}
// spectro_big.hip: W_M^(w k1), k1 = t + 64 m, is exp(-2 pi i w t / M) (one sincos per lane) times this table's entry.  [W][16]
std::vector<float> big_register_twiddles(int n) {
  const int M = n / 2, W = M / 1024;
  std::vector<float> bt((size_t)W * 16 * 2);
  for (int w = 0; w < W; w++)
    for (int m = 0; m < 16; m++) {
      const double ang = -kTwoPi * (double)(((long long)64 * w * m) % M) / M;
      bt[2 * ((size_t)w * 16 + m)] = (float)std::cos(ang);
      bt[2 * ((size_t)w * 16 + m) + 1] = (float)std::sin(ang);
    }
  return bt;
}

// Odd taper counts with half tables that stay in LDS (spectro16xl.hip): DPSS tapers are symmetric (even order) or
// antisymmetric (odd order) about the frame centre, so samples n < N/2 suffice.  Built only if the tapers have that symmetry
// to 1e-7 of their peak and the tables leave room for two blocks per CU (80 KiB); empty otherwise.
std::vector<float> lds_half_tables(int n, int ntapers, const double *tapers, const double *sig) {
  const int T = n / 16, nfull = (ntapers + 1) / 2 - 1;
  std::vector<float> ltaps;
  bool sym = true;
  for (int j = 0; j < ntapers && sym; j++) {
    const double *v = &tapers[(size_t)j * n];
    double peak = 0.0, dev = 0.0;
    for (int i = 0; i < n / 2; i++) {
      peak = std::max(peak, std::fabs(v[i]));
      dev = std::max(dev, std::fabs(v[n - 1 - i] - ((j & 1) ? -v[i] : v[i])));
    }
    sym = dev <= 1e-7 * peak;
  }
  const size_t lds = ((size_t)(n + n / 16) * (T >= 256 ? 1 : 256 / T) + 16 * 17 + 8 + (size_t)nfull * 8 * T + 4 * T) * 8;
  if (!sym || lds > 80 * 1024) return ltaps;
  ltaps.resize((size_t)nfull * 8 * T * 2 + (size_t)8 * T);
  for (int j = 0; j < ntapers; j++) {
    const bool last = j == ntapers - 1;
    const double scale = std::sqrt(1.0 / ((last ? 4.0 : 2.0) * n * (1.0 + sig[j])));
    for (int m = 0; m < 8; m++)
      for (int t = 0; t < T; t++) {
        const float val = (float)(tapers[(size_t)j * n + t + T * m] * scale);
        if (last) ltaps[(size_t)nfull * 8 * T * 2 + (size_t)m * T + t] = val;
        else ltaps[(((size_t)(j / 2) * 8 + m) * T + t) * 2 + (j & 1)] = val;
      }
  }
  return ltaps;
}

// One float per sample and row in the order a lane's four 16-byte loads take them: [row][m/4][t][4] for sample t + T m of
// flat[row][n].  The complex I/Q rows' table (spectro16c.hip) and the adaptive weights' (spectro16a.hip: two rows a round, so
// rows_out rounds an odd count up and the last row stays zeros).
std::vector<float> lane_order_rows(int n, int rows_in, int rows_out, const float *flat) {
  const int T = n / 16;
  std::vector<float> out((size_t)rows_out * n, 0.0f);
  for (int j = 0; j < rows_in; j++)
    for (int i = 0; i < n; i++) {
      const int t = i % T, m = i / T;
      out[(size_t)j * n + ((size_t)(m / 4) * T + t) * 4 + (size_t)(m & 3)] = flat[(size_t)j * n + i];
    }
  return out;
}

// HP-ARMA: which lag each cell of the t x (p_e+1) matrix holds after the reference's fill (hparma.c:89-102).  r_xx is
// matrix(0,t,0,p_e) (hparma.c:64): its rows are contiguous (util.c:153-160), lags 0..t-1 are written into row 0 past its
// p_e+1 columns, and the Toeplitz loop then copies cells that it may already have rewritten.  Simulated here with lag labels
// instead of values.
std::vector<uint16_t> hparma_lag_map(int t, int ncol) {
  std::vector<int> flat((size_t)(t + 1) * ncol, -1);
  for (int i = 0; i < t; i++) flat[i] = i;                       // r_xx[0][i] = r(i)
  for (int i = 1; i < t; i++)
    for (int j = 0; j < ncol; j++) flat[(size_t)i * ncol + j] = flat[std::abs(j - i)];
  std::vector<uint16_t> lagmap((size_t)t * ncol);
  for (size_t i = 0; i < lagmap.size(); i++) lagmap[i] = (uint16_t)(flat[i] < 0 ? 0 : flat[i]);
  return lagmap;
}
// HP-ARMA: [n/2+1] exp(-2 pi i k/n)
std::vector<float> unit_circle(int n) {
  std::vector<float> unit((size_t)2 * (n / 2 + 1));
  for (int k = 0; k <= n / 2; k++) {
    const double ang = -kTwoPi * k / n;
    unit[2 * k] = (float)std::cos(ang);
    unit[2 * k + 1] = (float)std::sin(ang);
  }
  return unit;
}
// The Jacobi sweep of compute_svd (util.c:301-355) as a STATIC SCHEDULE of steps of up to `width` rotations that share
// no column: [steps][width], j | k << 8, or -1.  Two rotations that share a column must keep the order of the reference's
// row-cyclic walk -- nothing else orders them (a rotation touches its two columns only, its skip tests are its own) -- so the
// walk is a DAG in which (j, k) waits for the last earlier rotation on column j and the last on column k; list scheduling by
// longest remaining path fills steps of eight: 80 steps for 33 columns (66 would be full steps; anti-diagonal by anti-diagonal
// it is 94).  Width 16 (each rotation over 4 lanes, A/B runs): 63 steps for 33 columns -- the critical path.
std::vector<int> jacobi_schedule(int ncol, int width) {
  std::vector<int> rot_sched;
  if (ncol < 2 || ncol > 64) return rot_sched;
  std::vector<std::pair<int, int>> rots;
  for (int j = 0; j < ncol - 1; j++)
    for (int k = j + 1; k < ncol; k++) rots.push_back({j, k});
  const int R = (int)rots.size();
  std::vector<std::vector<int>> succ(R);
  std::vector<int> indeg(R, 0), lastc(ncol, -1), lp(R, 1);
  for (int i = 0; i < R; i++) {
    const int cs[2] = {rots[i].first, rots[i].second};
    int seen = -1;
    for (int c : cs) {
      if (lastc[c] >= 0 && lastc[c] != seen) {
        succ[lastc[c]].push_back(i);
        indeg[i]++;
        seen = lastc[c];
      }
      lastc[c] = i;
    }
  }
  for (int i = R - 1; i >= 0; i--)
    for (int s : succ[i]) lp[i] = std::max(lp[i], 1 + lp[s]);
  std::vector<int> ready;
  for (int i = 0; i < R; i++)
    if (!indeg[i]) ready.push_back(i);
  int done = 0;
  while (done < R) {
    std::sort(ready.begin(), ready.end(), [&](int a, int b) { return lp[a] != lp[b] ? lp[a] > lp[b] : a < b; });
    const int take = std::min<int>(width, (int)ready.size());
    std::vector<int> cur(ready.begin(), ready.begin() + take);
    ready.erase(ready.begin(), ready.begin() + take);
    for (int g = 0; g < width; g++) rot_sched.push_back(g < take ? (rots[cur[g]].first | rots[cur[g]].second << 8) : -1);
    for (int i : cur) {
      done++;
      for (int s : succ[i])
        if (--indeg[s] == 0) ready.push_back(s);
    }
  }
  return rot_sched;
}

void build_ftest_tables(int n, int T, const double *tapers, const double *sig, FtestTables *out) {
  FtestTables &f = *out;
  f.U0.resize(T);
  f.hn.resize(n);
  make_ftest_tables(n, T - 1, tapers, f.U0.data(), f.hn.data(), &f.sum_U0_sqr);
  // [hn][taper 0..T-1][hn]: the one-launch form starts with hn (mu first), the spectrum-by-spectrum form ends with it
  f.taps.assign((size_t)(T + 2) * 2 * n, 0.0f);
  for (int j = -1; j <= T; j++)
    for (int i = 0; i < n; i++)
      f.taps[(size_t)(j + 1) * 2 * n + tap_slot(n, 0, i, 0)] = (j >= 0 && j < T) ? (float)tapers[(size_t)j * n + i] : f.hn[i];
  // c_j = 1 / (n (1 + sig_j)), the rows' weights of the rows-and-F entries (the tables above stay unscaled)
  f.cj.resize((size_t)T);
  for (int j = 0; j < T; j++) f.cj[j] = (float)(1.0 / ((double)n * (1.0 + sig[j])));
  // the paired form's tables: two real sequences per N-point transform (re / im), each halved (X_a = (Z[k] + conj Z[N-k]) / 2)
  // hn = sum_j U0_j v_j / sum(U0^2) has the 2-norm 1 / sqrt(sum(U0^2)) against a taper's 1: sharing a transform with taper 0 as it is,
  // mu would come out of the separation with the rounding of a spectrum ~ sqrt(sum(U0^2)) times its size (up to 128 at N = 16384),
  // and mu U0_j carries that into every residual.  A power of two brings hn to a taper's size; the kernel takes it out of mu again.
  {
    int ex = 0;
    (void)frexpf(sqrtf(f.sum_U0_sqr), &ex);                       // sqrt(sum U0^2) = m 2^ex, 1/2 <= m < 1
    f.hn_scale = f.sum_U0_sqr > 0.0f && ex > 0 && ex < 64 ? ldexpf(1.0f, ex - 1) : 1.0f;
  }
  const int r_mu = (T + 2) / 2, r_nomu = (T + 1) / 2;
  f.r_mu = r_mu;
  f.paired.assign((size_t)(r_mu + r_nomu) * 2 * n, 0.0f);
  auto seq = [&](int s_, int i, bool with_mu) -> float {          // sequence s_ of the call: hn first when mu is live, then the tapers
    const int j = with_mu ? s_ - 1 : s_;
    if (j >= T) return 0.0f;
    return 0.5f * (j < 0 ? f.hn_scale * f.hn[i] : (float)tapers[(size_t)j * n + i]);
  };
  for (int r = 0; r < r_mu + r_nomu; r++) {
    const bool with_mu = r < r_mu;
    const int rr = with_mu ? r : r - r_mu;
    for (int i = 0; i < n; i++) {
      f.paired[(size_t)r * 2 * n + tap_slot(n, 0, i, 0)] = seq(2 * rr, i, with_mu);
      f.paired[(size_t)r * 2 * n + tap_slot(n, 0, i, 1)] = seq(2 * rr + 1, i, with_mu);
    }
  }
}

int iq_config_ok(const glfer_hip_config *cfg) {
  if (!cfg) return GLFER_E_ARG;
  if (cfg->mode != GLFER_MODE_FFT && cfg->mode != GLFER_MODE_MTM) return GLFER_E_ARG;
  if (!is_pow2(cfg->n) || cfg->n < 256 || cfg->n > 16384) return GLFER_E_ARG;
  if (cfg->sub_mean != 0 || cfg->limiter_a > 0.0f || cfg->enable_limiter != 0) return GLFER_E_ARG;
  if (cfg->sample_format < 0 || cfg->sample_format > 2) return GLFER_E_ARG;
  return GLFER_OK;
}

int adaptive_config_ok(const glfer_hip_config *cfg) {
  if (!cfg) return GLFER_E_ARG;
  if (cfg->mode != GLFER_MODE_MTM || cfg->mtm_k < 1 || cfg->mtm_k + 1 > GLFER_ADAPTIVE_KMAX) return GLFER_E_ARG;   // K = 2 .. 8 tapers
  if (cfg->n < 256 || cfg->n > 4096 || (cfg->n & (cfg->n - 1))) return GLFER_E_ARG;
  return iq_config_ok(cfg);                                                    // mean removal, limiter, RA9MB, the sample format
}

// gl_dpss (g-l_dpss.c:288-347) is the expensive part of mtm_init -- 0.1-0.3 s at N = 16384 with 9 tapers -- and the
// *_multi / *_workers entries make a plan per worker and call: the last few results are kept (same doubles, bit for bit)
bool cached_dpss(int n, int kmax, float w, std::vector<double> *tapers, std::vector<double> *sig) {
  struct Kept { int n, kmax; float w; std::vector<double> tapers, sig; };
  static std::mutex mu;
  static std::vector<Kept> kept;
  {
    std::lock_guard<std::mutex> lock(mu);
    for (const Kept &k : kept)
      if (k.n == n && k.kmax == kmax && k.w == w) {
        *tapers = k.tapers;
        *sig = k.sig;
        return true;
      }
  }
  tapers->resize((size_t)(kmax + 1) * n);
  sig->resize(kmax + 1);
  if (!make_dpss(n, kmax, (double)w, tapers->data(), sig->data())) return false;
  std::lock_guard<std::mutex> lock(mu);
  if (kept.size() >= 4) kept.erase(kept.begin());
  kept.push_back(Kept{n, kmax, w, *tapers, *sig});
  return true;
}

int plan_config_ok(const glfer_hip_config *cfg) {
  if (!cfg) return GLFER_E_ARG;
  const int n = cfg->n;
  // any power of two the user can type (g_options.c:386-387): 8 .. 128 through spectro_small.hip,
  // 256 .. 16384 through the 16-points-per-lane kernels, 32768 through spectro16w.hip alone, 65536 .. 1048576
  // through spectro_big.hip (sub-transforms and combine as two kernels around a scratch in HBM)
  if (!is_pow2(n) || n < 8 || n > (1 << 20)) return GLFER_E_ARG;
  // HP-ARMA: the frame, its autocorrelation's zero tail and the matrix live in one wavefront's LDS -- any power of two from 32 up to what
  // fits 160 KB (N = 32768 with t = 128, p_e = 32: 137 KB, one frame in flight per CU); round 5 (it was 256 .. 16384)
  if (cfg->mode == GLFER_MODE_HPARMA && (n < 32 || n > 32768)) return GLFER_E_ARG;
  if (!(cfg->overlap >= 0.0f) || !(cfg->overlap < 1.0f)) return GLFER_E_ARG;   // g_options.c:1030
  if (cfg->mode != GLFER_MODE_FFT && cfg->mode != GLFER_MODE_MTM && cfg->mode != GLFER_MODE_HPARMA &&
      cfg->mode != GLFER_MODE_LMP)
    return GLFER_E_ARG;
  if (cfg->mode == GLFER_MODE_LMP && (cfg->lmp_av < 1 || cfg->lmp_av > 4096)) return GLFER_E_ARG;
  if (cfg->mode == GLFER_MODE_HPARMA) {
    const int t = cfg->hparma_t, ncol = cfg->hparma_p_e + 1;
    if (t < 2 || ncol < 2 || ncol > t || t > n || ncol > 256 || t > 65535) return GLFER_E_ARG;   // p_e+1 <= t (hparma.c:107)
    if (glfer_hparma_lds_bytes(n, t, ncol) > 160 * 1024) return GLFER_E_ARG;   // (hparma_frames.h: the frame's LDS, as its launcher asks for it)
  }
  if (cfg->sample_format < 0 || cfg->sample_format > 2) return GLFER_E_ARG;
  if (cfg->mode == GLFER_MODE_MTM && (cfg->mtm_k < 0 || cfg->mtm_k > 31 || !(cfg->mtm_w > 0.0f)))
    return GLFER_E_ARG;
  if (cfg->mode == GLFER_MODE_FFT && (cfg->window_type < 0 || cfg->window_type > 7)) return GLFER_E_ARG;
  if ((int)(n * (1.0 - cfg->overlap)) <= 0) return GLFER_E_ARG;                  // the hop, fft.c:70
  // cfg.psd_pitch: floats from one PSD row to the next in the DEVICE entries' d_psd (0 = dense, N/2+1).  The LMP statistic
  // and the host / file entries (their rows go home through a dense ring) keep dense rows.
  const int bins = n / 2 + 1, pitch = cfg->psd_pitch ? cfg->psd_pitch : bins;
  if (cfg->psd_pitch < 0 || pitch < bins || (cfg->psd_pitch && cfg->mode == GLFER_MODE_LMP)) return GLFER_E_ARG;
  return GLFER_OK;
}

int build_plan_tables(const glfer_hip_config &cfg_in, int rot_width, PlanTables *out) {
  PlanTables &p = *out;
  p = PlanTables();
  p.cfg = cfg_in;
  const glfer_hip_config &cfg = p.cfg;
  const int n = cfg.n;
  const bool small = n < 256, huge = n > 16384;
  p.hop = (int)(n * (1.0 - cfg.overlap));                          // fft.c:70
  p.keep = n - p.hop;                                              // fft.c:71
  p.bins = n / 2 + 1;
  p.pitch = cfg.psd_pitch ? cfg.psd_pitch : p.bins;
  int logn = 0;
  while ((1 << logn) < n) logn++;

  p.window.assign(n, 1.0f);
  // LMP (lmp.c:101-181): the periodogram of the raw assembled frame -- lmp.c:114-116 overwrites what
  // prepare_audio left in inbuf_fft, so window (rectangular anyway, source.c:395), a and limiter
  // have no effect -- followed by the per-bin statistic over the last lmp_av periodograms
  const bool lmp = cfg.mode == GLFER_MODE_LMP, mtm = cfg.mode == GLFER_MODE_MTM;
  if (lmp) {
    p.cfg.window_type = GLFER_WIN_RECTANGULAR;
    p.cfg.limiter_a = 0.0f;
    p.cfg.enable_limiter = 0;
    p.lmp_av = cfg.lmp_av;
  }
  const bool periodogram = cfg.mode == GLFER_MODE_FFT || lmp;
  if (periodogram) {
    p.ntapers = 1;
    p.npairs = 1;
    make_window(cfg.window_type, n, p.window.data());
    p.nonlin = (cfg.limiter_a > 0.0f) || (cfg.enable_limiter == 1);
    // psd = |X|^2/N (fft.c:212-216); the pair packing contributes |Z_k|^2+|Z_{N-k}|^2 = 2|X_k|^2
    // (N = 32768 runs the real-input form only: its inputs carry sqrt(1/(4N)), see w_tables)
    const double scale = std::sqrt(1.0 / ((huge ? 4.0 : 2.0) * n));
    p.spec_unscale = (float)scale;
  } else if (mtm) {
    p.ntapers = cfg.mtm_k + 1;                                     // mtm.c:189: j = 0..kmax inclusive
    p.npairs = (p.ntapers + 1) / 2;
    if (!cached_dpss(n, cfg.mtm_k, cfg.mtm_w, &p.tapers, &p.sig)) return GLFER_E_NUMERIC;
  }
  // the rows of the window / taper tables below: the tapers, or the periodogram's window (NULL: rectangular)
  const float *window = cfg.window_type == GLFER_WIN_RECTANGULAR ? nullptr : p.window.data();
  const double *tapers = mtm ? p.tapers.data() : nullptr, *sig = mtm ? p.sig.data() : nullptr;

  // --- the packed pairs (spectro16.hip, spectro_small.hip) and their twiddles; four floats stand in where no packed form runs
  if (huge || cfg.mode == GLFER_MODE_HPARMA) {
    p.taps.assign(4, 0.0f);
  } else if (periodogram) {
    p.taps.assign((size_t)2 * n, 0.0f);
    periodogram_pair_table(n, window, p.nonlin, (double)std::sqrt(1.0 / (2.0 * n)), p.taps.data());
  } else {
    p.taps.assign((size_t)2 * p.npairs * n, 0.0f);
    mtm_pair_tables(n, p.ntapers, tapers, sig, p.taps.data());
  }
  p.tw = (!small && !huge) ? twiddles16(logn, n / 16) : std::vector<float>(2, 0.0f);

  // --- real-input form (spectro16h.hip): the linear periodogram from N = 512, multitaper from N = 8192
  if (!huge && ((periodogram && !p.nonlin && n >= 512) || (mtm && n >= 8192))) {
    p.htapers = mtm ? p.ntapers : 1;
    p.htaps = h_tables(n, p.htapers, window, tapers, sig);
    p.htw = twiddles16(logn - 1, n / 32);
    p.hrot = h_rotations(n);
  }

  // --- wavefront-private real-input form (spectro16w.hip, N >= 2048; spectro_big.hip above 16384)
  if (((periodogram && (!p.nonlin || huge)) || mtm) && n >= 2048) {
    p.wtapers = mtm ? p.ntapers : 1;
    p.wtaps = w_tables(n, p.wtapers, window, tapers, sig, p.nonlin);
    p.wtw = twiddles16(10, 64);
    p.wcomb = w_combine_twiddles(n);
    if (huge) p.bigtw = big_register_twiddles(n);
  }

  // --- odd taper count (spectro16x.hip): the last taper shares a transform with the next frame's
  if (mtm && (p.ntapers & 1) && p.ntapers >= 3 && !small && !huge) {
    p.xtaps.resize((size_t)n);
    mtm_last_table(n, p.ntapers, tapers, sig, p.xtaps.data());
    // five tapers at N = 4096 (spectro16y.hip): the half tables a lane keeps in registers, where the float tables are
    // exactly (anti)symmetric; otherwise (and for every other taper count) the plan keeps the full-table form
    if (n == 4096 && p.ntapers == 5) {
      p.ytaps.resize((size_t)(n / 16) * GLFER_YHALF_FLOATS);
      if (!build_y_half_table(n, p.taps.data(), p.xtaps.data(), p.ytaps.data())) p.ytaps.clear();
    }
    if (n <= 4096) p.ltaps = lds_half_tables(n, p.ntapers, tapers, sig);
  }

  // --- complex I/Q rows (spectro16c.hip); made with the plan so that the entries allocate and copy nothing (stream capture)
  if (iq_config_ok(&p.cfg) == GLFER_OK) {
    std::vector<float> flat((size_t)p.ntapers * n);
    make_iq_table(n, p.ntapers, mtm ? nullptr : window, tapers, sig, flat.data());
    p.iqtaps = lane_order_rows(n, p.ntapers, p.ntapers, flat.data());
  }
  // --- adaptive weights (spectro16a.hip): the tapers themselves, float(v_j) with nothing folded in, in the I/Q table's order
  if (adaptive_config_ok(&p.cfg) == GLFER_OK) {
    const std::vector<float> flat(p.tapers.begin(), p.tapers.end());
    p.ataps = lane_order_rows(n, p.ntapers, 2 * ((p.ntapers + 1) / 2), flat.data());
  }

  if (cfg.mode == GLFER_MODE_HPARMA) {
    const int t = cfg.hparma_t, ncol = cfg.hparma_p_e + 1;
    p.rot_sched = jacobi_schedule(ncol, rot_width);
    p.rot_steps = (int)(p.rot_sched.size() / rot_width);
    p.lagmap = hparma_lag_map(t, ncol);
    p.unit = unit_circle(n);
  }
  return GLFER_OK;
}

}  // namespace glfer
