// ysegbench.hip -- where does the single-stream third of spectro16y_kernel's iteration go?  (C3: N = 4096, five tapers, half
// tables, frame pairs from the queue: the product form.)  Wave 0 of one workgroup records s_memtime at every GLFER_STAMP /
// GLFER_SEG_STAMP mark of its iterations; the tool prints the mean duration of each phase of a steady-state iteration and its
// share (profiles/y_shared_segment.txt).  The marks cost a lot themselves (a clock read, a counter and a store each, in every
// wavefront's instruction stream a branch with the scheduling fenced around it: the stamped kernel runs at half the product's
// rate), so the shares are to be read against the same table of another build, not as product timings.
//   hipcc --offload-arch=gfx950 -O3 -std=c++20 -fno-slp-vectorize -Iglfer_amd/csrc tools/ysegbench.hip \
//         glfer_amd/csrc/host_tables.cpp -o tools/bin/ysegbench && tools/bin/ysegbench [nframes] [hop in sixteenths of N]
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
constexpr int kRounds = 96, kSlots = 32, kBlock = 8;
__device__ unsigned long long *g_stamps;          // [kRounds][kSlots]: a round starts at GLFER_STAMP(0); slots 16.. = GLFER_SEG_STAMP
__device__ int g_round;
#define YSEG_RECORD(slot, opens)                                                                     \
  do {                                                                                               \
    if (blockIdx.x == kBlock && threadIdx.x == 0) {                                                  \
      __builtin_amdgcn_sched_barrier(0);                                                             \
      const unsigned long long c_ = __builtin_amdgcn_s_memtime();                                    \
      if (opens) g_round++;                                                                          \
      if (g_round > 0 && g_round <= kRounds) g_stamps[(g_round - 1) * kSlots + (slot)] = c_;         \
      __builtin_amdgcn_sched_barrier(0);                                                             \
    }                                                                                                \
  } while (0)
#define GLFER_STAMP(id) YSEG_RECORD((id), (id) == 0)
#define GLFER_SEG_STAMP(id) YSEG_RECORD(16 + (id), false)
#define GLFER_NO_LAUNCHERS
#include "spectro16y.hip"
#include "host_tables.h"

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e_)); return 1; } } while (0)

int main(int argc, char **argv) {
  const int nframes = argc > 1 ? atoi(argv[1]) : 262144;
  const int hop16 = argc > 2 ? atoi(argv[2]) : 16;
  constexpr int LOGN = 12, N = 1 << LOGN, P = N / 2 + 1, T = 5, NP = 3, TT = N / 16;
  if (nframes < 2 || (hop16 != 16 && hop16 != 8 && hop16 != 4)) { printf("usage: ysegbench [nframes >= 2] [16 | 8 | 4]\n"); return 1; }
  const int H = N / 16 * hop16;
  std::vector<double> tapers((size_t)T * N), sig(T);
  if (!glfer::make_dpss(N, T - 1, 2.5, tapers.data(), sig.data())) { printf("dpss failed\n"); return 1; }
  // the tables as tools/yqbench builds them: pair tables, the last taper, and the half table by residue
  std::vector<float> taps((size_t)2 * NP * N, 0.0f), xt(N);
  for (int j = 0; j < T; j++)
    for (int i = 0; i < N; i++) {
      const int t = i % TT, m = i / TT;
      taps[(size_t)(j / 2) * N * 2 + ((size_t)(m / 2) * TT + t) * 4 + (size_t)(m & 1) * 2 + (j & 1)] =
          (float)(tapers[(size_t)j * N + i] * sqrt(1.0 / (2.0 * N * (1.0 + sig[j]))));
    }
  for (int i = 0; i < N; i++) {
    const int t = i % TT, m = i / TT;
    xt[((size_t)(m / 4) * TT + t) * 4 + (size_t)(m & 3)] = (float)(tapers[(size_t)(T - 1) * N + i] * sqrt(1.0 / (4.0 * N * (1.0 + sig[T - 1]))));
  }
  std::vector<float> yt((size_t)TT * GLFER_YHALF_FLOATS);
  {
    auto pairv = [&](int j, int i) { return taps[(size_t)(j / 2) * N * 2 + ((size_t)((i / TT) / 2) * TT + i % TT) * 4 + (size_t)((i / TT) & 1) * 2 + (j & 1)]; };
    auto lastv = [&](int i) { return xt[((size_t)((i / TT) / 4) * TT + i % TT) * 4 + (size_t)((i / TT) & 3)]; };
    for (int t = 0; t < TT; t++) {
      const int r = (int)glfer_yhalf_residue((unsigned)t);
      for (int m = 0; m < 8; m++) {
        for (int j = 0; j < 4; j++) yt[(size_t)t * GLFER_YHALF_FLOATS + 16 * (j / 2) + 2 * m + (j & 1)] = pairv(j, r + TT * m);
        yt[(size_t)t * GLFER_YHALF_FLOATS + 32 + m] = lastv(r + TT * m);
      }
    }
  }
  std::vector<float> tw((size_t)2 * glfer::make_twiddles16(LOGN, nullptr) * TT);
  glfer::make_twiddles16(LOGN, tw.data());
  const size_t ns = (size_t)nframes * H + (N - H);
  std::vector<float> x(ns);
  unsigned s = 12345;
  for (size_t i = 0; i < ns; i++) { s = s * 1664525u + 1013904223u; x[i] = (float)((s >> 8) * (1.0 / 16777216.0) - 0.5) + 0.3f * sinf(0.01f * (float)i); }
  float *d_x, *d_taps, *d_xt, *d_yt, *d_psd;
  float2 *d_tw;
  unsigned *d_counter;
  unsigned long long *d_st;
  CK(hipMalloc((void **)&d_x, ns * 4));
  CK(hipMalloc((void **)&d_taps, taps.size() * 4));
  CK(hipMalloc((void **)&d_xt, xt.size() * 4));
  CK(hipMalloc((void **)&d_yt, yt.size() * 4));
  CK(hipMalloc((void **)&d_tw, tw.size() * 4));
  CK(hipMalloc((void **)&d_psd, (size_t)nframes * P * 4));
  CK(hipMalloc((void **)&d_counter, 128));
  CK(hipMemset(d_counter, 0, 128));
  CK(hipMalloc((void **)&d_st, (size_t)kRounds * kSlots * 8));
  CK(hipMemcpy(d_x, x.data(), ns * 4, hipMemcpyHostToDevice));
  CK(hipMemcpy(d_taps, taps.data(), taps.size() * 4, hipMemcpyHostToDevice));
  CK(hipMemcpy(d_xt, xt.data(), xt.size() * 4, hipMemcpyHostToDevice));
  CK(hipMemcpy(d_yt, yt.data(), yt.size() * 4, hipMemcpyHostToDevice));
  CK(hipMemcpy(d_tw, tw.data(), tw.size() * 4, hipMemcpyHostToDevice));
  CK(hipMemcpyToSymbol(HIP_SYMBOL(g_stamps), &d_st, sizeof d_st));
  SpectroParams sp = {};
  sp.stream = d_x + (N - H); sp.frame0 = 0; sp.nframes = nframes; sp.H = H; sp.R = N - H; sp.npairs = NP; sp.fmt = GLFER_FMT_F32;
  sp.taps = d_taps; sp.tw = d_tw; sp.xtaps = d_xt; sp.ytaps = d_yt; sp.spec_unscale = 1.0f;
  sp.pitch = P; sp.psd = d_psd;
  auto kq = glfer::spectro16y_kernel<GLFER_FMT_F32, 0, 0, 0, 0, 1, 1>;
  const size_t shy = (size_t)glfer::LaunchY::LDS_WORDS * 8;
  CK(hipFuncSetAttribute(reinterpret_cast<const void *>(kq), hipFuncAttributeMaxDynamicSharedMemorySize, (int)shy));
  hipEvent_t e0, e1;
  CK(hipEventCreate(&e0));
  CK(hipEventCreate(&e1));
  const int chunk = 4;
  unsigned base = 0;
  const long long nchunks = glfer_yq_chunks(nframes, chunk);
  const unsigned grid = glfer_yq_grid(nchunks);
  if (grid <= (unsigned)kBlock) { printf("too few frames for workgroup %d\n", kBlock); return 1; }
  printf("ysegbench: %d frames, hop %d (%d/16 of N), half tables, f32, queue chunk %d, grid %u; wave 0 of workgroup %d\n", nframes, H, hop16, chunk, grid, kBlock);
  for (int rep = 0; rep < 4; rep++) {                // the last launch's stamps are read
    int zero = 0;
    CK(hipMemcpyToSymbol(HIP_SYMBOL(g_round), &zero, sizeof zero));
    CK(hipMemset(d_st, 0, (size_t)kRounds * kSlots * 8));
    SpectroParams q = sp;
    q.yq_counter = d_counter; q.yq_base = base; q.yq_chunk = chunk;
    CK(hipEventRecord(e0));
    hipLaunchKernelGGL(kq, dim3(grid), dim3(256), shy, 0, q);
    CK(hipGetLastError());
    CK(hipEventRecord(e1));
    CK(hipEventSynchronize(e1));
    base += (unsigned)nchunks;
    float ms;
    CK(hipEventElapsedTime(&ms, e0, e1));
    printf("launch %d: %.3f ms  %.2f Mframes/s (stamped build)\n", rep, ms, nframes / (ms * 1e-3) / 1e6);
  }
  std::vector<unsigned long long> st((size_t)kRounds * kSlots);
  CK(hipMemcpy(st.data(), d_st, st.size() * 8, hipMemcpyDeviceToHost));
  // an iteration = rounds 3 j (dual), 3 j + 1 (dual), 3 j + 2 (shared); the fold's marks (slots 16..19) lie behind the second
  // dual round's end and were recorded under its round number.  A phase = (round of the iteration, slot) of its end; its
  // start is the previous phase's end.  Marks that a build does not have stay 0 and are skipped.
  struct Phase { int r, slot; const char *name; bool segment; };
  const Phase ph[] = {
      {0, 15, "dual round 1", false},
      {1, 0, "(between the dual rounds)", false},
      {1, 15, "dual round 2", false},
      {1, 16, "fold: power sums over the wavefront", true},
      {1, 17, "fold: LDS writes / partials issued", true},
      {1, 18, "fold: barrier", true},
      {1, 19, "fold: scales, mirror reads", true},
      {2, 0, "fold: second barrier (or: scales)", true},
      {2, 1, "shared: form z, pass 0 butterflies, writes issued", true},
      {2, 3, "shared: next samples requested (write drain)", true},
      {2, 4, "shared: write-to-read barrier 0", true},
      {2, 20, "shared: exchange 0 read wait", true},
      {2, 22, "shared: release barrier 0", true},
      {2, 5, "shared: pass 1 butterflies, writes issued", true},
      {2, 7, "shared: write drain 1", true},
      {2, 8, "shared: write-to-read barrier 1", true},
      {2, 21, "shared: exchange 1 read wait", true},
      {2, 23, "shared: release barrier 1", true},
      {2, 9, "shared: pass 2 butterflies (+ mirror entries)", true},
      {2, 12, "separate: mirror writes issued", true},
      {2, 13, "separate: barrier", true},
      {2, 14, "separate: mirror reads, fold, rows issued", true},
      {2, 15, "separate: final barrier", true},
      {3, 0, "loop top (to the next iteration's first round)", false},
  };
  const int nph = (int)(sizeof ph / sizeof ph[0]);
  std::vector<double> sum(nph, 0.0);
  int cnt = 0;
  for (int j = 3; 3 * j + 3 < kRounds; j++) {         // steady state: from the fourth iteration
    auto at = [&](int r, int slot) { return st[(size_t)(3 * j + r) * kSlots + slot]; };
    if (!at(0, 0) || !at(3, 0)) continue;
    unsigned long long prev = at(0, 0);
    bool ok = true;
    std::vector<double> d(nph, 0.0);
    for (int i = 0; i < nph; i++) {
      const unsigned long long c = at(ph[i].r, ph[i].slot);
      if (!c) continue;                              // a mark this build does not have
      if (c < prev) { ok = false; break; }
      d[i] = (double)(c - prev);
      prev = c;
    }
    if (!ok) continue;
    for (int i = 0; i < nph; i++) sum[i] += d[i];
    cnt++;
  }
  if (!cnt) { printf("no complete iterations recorded\n"); return 1; }
  double tot = 0, seg = 0;
  for (int i = 0; i < nph; i++) { tot += sum[i] / cnt; if (ph[i].segment) seg += sum[i] / cnt; }
  printf("%d steady-state iterations averaged; s_memtime ticks, share of the iteration\n", cnt);
  for (int i = 0; i < nph; i++)
    if (sum[i] > 0) printf("  %-52s %8.2f  %5.1f %%\n", ph[i].name, sum[i] / cnt, 100.0 * sum[i] / cnt / tot);
  printf("  %-52s %8.2f  %5.1f %%\n", "single-stream third (fold + shared + separate)", seg, 100.0 * seg / tot);
  printf("  %-52s %8.2f\n", "iteration", tot);
  return 0;
}
