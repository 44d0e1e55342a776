// yqbench.hip -- what a workgroup of spectro16y_kernel (C3: N = 4096, five tapers, half tables) pays at its start and
// how evenly a launch ends, for the static stride and for the queue form (profiles/y_frame_queue.txt).  Every workgroup
// records the 100 MHz clock at entry, in front of its first iteration (= its first round start) and behind its last one
// (GLFER_BLOCK_MARK: nothing inside the loop, so the steady state runs as in the product):
//   (a) entry -> first round start, against a steady-state iteration ((lives - start-ups) / frame pairs)
//   (b) idle slot-time at the end of the launch: sum over the resident slots of (kernel end - the slot's last end)
//       over slots x kernel time; a slot's last end = one of the `slots` latest workgroup ends
// and the time of each launch shape with the stamps in (the product kernel carries none).
//   hipcc --offload-arch=gfx950 -O3 -std=c++20 -fno-slp-vectorize -Iglfer_amd/csrc tools/yqbench.hip \
//         glfer_amd/csrc/host_tables.cpp -o tools/bin/yqbench && tools/bin/yqbench [nframes] [overlap16: hop in sixteenths of N]
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
__device__ unsigned long long *g_rec;             // [blocks][4]: entry, first round start, end
#define GLFER_BLOCK_MARK(k)                                                                          \
  do {                                                                                               \
    if (threadIdx.x == 0) g_rec[(size_t)blockIdx.x * 4 + (k)] = __builtin_amdgcn_s_memrealtime();    \
  } while (0)
#define GLFER_NO_LAUNCHERS
#include "spectro16y.hip"
#include "host_tables.h"

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e_)); return 1; } } while (0)

int main(int argc, char **argv) {
  const int nframes = argc > 1 ? atoi(argv[1]) : 262144;
  const int hop16 = argc > 2 ? atoi(argv[2]) : 16;
  constexpr int LOGN = 12, N = 1 << LOGN, P = N / 2 + 1, T = 5, NP = 3, TT = N / 16;
  if (nframes < 2 || (hop16 != 16 && hop16 != 8 && hop16 != 4)) { printf("usage: yqbench [nframes >= 2] [16 | 8 | 4]\n"); return 1; }
  const int H = N / 16 * hop16;
  std::vector<double> tapers((size_t)T * N), sig(T);
  if (!glfer::make_dpss(N, T - 1, 2.5, tapers.data(), sig.data())) { printf("dpss failed\n"); return 1; }
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
  float *d_x, *d_taps, *d_xt, *d_yt, *d_psd[2];
  float2 *d_tw;
  unsigned *d_counter;
  unsigned long long *d_rec;
  const size_t max_blocks = 8192;
  CK(hipMalloc((void **)&d_x, ns * 4));
  CK(hipMalloc((void **)&d_taps, taps.size() * 4));
  CK(hipMalloc((void **)&d_xt, xt.size() * 4));
  CK(hipMalloc((void **)&d_yt, yt.size() * 4));
  CK(hipMalloc((void **)&d_tw, tw.size() * 4));
  CK(hipMalloc((void **)&d_psd[0], (size_t)nframes * P * 4));
  CK(hipMalloc((void **)&d_psd[1], (size_t)nframes * P * 4));
  CK(hipMalloc((void **)&d_counter, 128));
  CK(hipMemset(d_counter, 0, 128));
  CK(hipMalloc((void **)&d_rec, max_blocks * 4 * 8));
  CK(hipMemcpy(d_x, x.data(), ns * 4, hipMemcpyHostToDevice));
  CK(hipMemcpy(d_taps, taps.data(), taps.size() * 4, hipMemcpyHostToDevice));
  CK(hipMemcpy(d_xt, xt.data(), xt.size() * 4, hipMemcpyHostToDevice));
  CK(hipMemcpy(d_yt, yt.data(), yt.size() * 4, hipMemcpyHostToDevice));
  CK(hipMemcpy(d_tw, tw.data(), tw.size() * 4, hipMemcpyHostToDevice));
  CK(hipMemcpyToSymbol(HIP_SYMBOL(g_rec), &d_rec, sizeof d_rec));
  SpectroParams sp = {};
  // frame f reads samples [f*H - R, f*H + H) of the stream: its sample 0 sits R floats into the buffer
  sp.stream = d_x + (N - H); sp.frame0 = 0; sp.nframes = nframes; sp.H = H; sp.R = N - H; sp.npairs = NP; sp.fmt = GLFER_FMT_F32;
  sp.taps = d_taps; sp.tw = d_tw; sp.xtaps = d_xt; sp.ytaps = d_yt; sp.spec_unscale = 1.0f;
  sp.pitch = P;
  auto ks = glfer::spectro16y_kernel<GLFER_FMT_F32, 0, 0, 0, 0, 1, 0>;
  auto kq = glfer::spectro16y_kernel<GLFER_FMT_F32, 0, 0, 0, 0, 1, 1>;
  const size_t shy = (size_t)glfer::LaunchY::LDS_WORDS * 8;
  CK(hipFuncSetAttribute(reinterpret_cast<const void *>(ks), hipFuncAttributeMaxDynamicSharedMemorySize, (int)shy));
  CK(hipFuncSetAttribute(reinterpret_cast<const void *>(kq), hipFuncAttributeMaxDynamicSharedMemorySize, (int)shy));
  hipEvent_t e0, e1;
  CK(hipEventCreate(&e0));
  CK(hipEventCreate(&e1));
  unsigned base = 0;
  const int slots = 512;
  std::vector<unsigned long long> rec(max_blocks * 4);
  printf("yqbench: %d frames, hop %d (%d/16 of N), half tables, f32; times in us of the 100 MHz clock\n", nframes, H, hop16);
  // chunk 0 = the static stride at grid min(pairs, 8192); chunk C >= 1 = the queue form
  auto run = [&](int chunk, int reps) -> int {
    float best = 1e9f;
    unsigned grid = 0;
    for (int rep = 0; rep < reps; rep++) {
      CK(hipMemset(d_rec, 0, max_blocks * 4 * 8));
      SpectroParams q = sp;
      q.psd = d_psd[chunk ? 1 : 0];
      CK(hipEventRecord(e0));
      if (chunk == 0) {
        const long long work = ((long long)nframes + 1) / 2;
        grid = (unsigned)(work < 8192 ? work : 8192);
        if (grid >= 64) grid &= ~7u;
        hipLaunchKernelGGL(ks, dim3(grid), dim3(256), shy, 0, q);
      } else {
        q.yq_counter = d_counter; q.yq_base = base; q.yq_chunk = chunk;
        const long long nchunks = glfer_yq_chunks(nframes, chunk);
        grid = glfer_yq_grid(nchunks);
        hipLaunchKernelGGL(kq, dim3(grid), dim3(256), shy, 0, q);
        base += (unsigned)nchunks;
      }
      CK(hipGetLastError());
      CK(hipEventRecord(e1));
      CK(hipEventSynchronize(e1));
      float ms;
      CK(hipEventElapsedTime(&ms, e0, e1));
      if (rep > 0) best = std::min(best, ms);
    }
    CK(hipMemcpy(rec.data(), d_rec, (size_t)grid * 4 * 8, hipMemcpyDeviceToHost));
    double start_sum = 0, life_sum = 0;
    const double iters = (double)(((long long)nframes + 1) / 2);
    unsigned long long tmin = ~0ull, tmax = 0;
    std::vector<unsigned long long> ends;
    std::vector<double> starts;
    for (unsigned b = 0; b < grid; b++) {
      const unsigned long long *r = &rec[(size_t)b * 4];
      if (!r[0] || !r[2]) continue;
      starts.push_back((double)(r[1] - r[0]) / 100.0);
      start_sum += starts.back();
      life_sum += (double)(r[2] - r[0]) / 100.0;
      tmin = std::min(tmin, r[0]);
      tmax = std::max(tmax, r[2]);
      ends.push_back(r[2]);
    }
    if (ends.empty()) { printf("no records\n"); return 1; }
    std::sort(ends.begin(), ends.end());
    std::sort(starts.begin(), starts.end());
    const size_t nb = ends.size(), ns_ = std::min<size_t>(slots, nb);
    double idle = 0;
    for (size_t i = nb - ns_; i < nb; i++) idle += (double)(tmax - ends[i]) / 100.0;
    const double span_us = (double)(tmax - tmin) / 100.0;
    const double iter_us = (life_sum - start_sum) / iters;
    char label[48];
    if (chunk) snprintf(label, sizeof label, "queue, chunk %d, grid %u", chunk, grid);
    else snprintf(label, sizeof label, "static stride, grid %u", grid);
    printf("%-30s best of %d: %.3f ms  %.2f Mframes/s (stamped build)\n", label, reps - 1, best, nframes / (best * 1e-3) / 1e6);
    printf("    (a) entry -> first round start: mean %.2f  median %.2f  p90 %.2f  max %.2f us; steady-state iteration %.2f us; "
           "start-ups %.0f x mean / (%d slots x %.0f us) = %.2f %% of slot-time\n",
           start_sum / nb, starts[nb / 2], starts[nb * 9 / 10], starts[nb - 1], iter_us, (double)nb, slots, span_us,
           100.0 * start_sum / (slots * span_us));
    printf("    (b) first entry -> last end %.1f us; idle slot-time at the end %.0f us over %zu slots = %.2f %% of slot-time "
           "(first of the last %zu ends %.1f us before the last)\n",
           span_us, idle, ns_, 100.0 * idle / (ns_ * span_us), ns_, (double)(tmax - ends[nb - ns_]) / 100.0);
    return 0;
  };
  for (int round = 0; round < 2; round++)
    for (int chunk : {0, 1, 2, 4, 8})
      if (run(chunk, 4)) return 1;
  // the two launch shapes' rows, bit for bit (the last queue run was chunk 8)
  std::vector<float> a((size_t)nframes * P), b((size_t)nframes * P);
  CK(hipMemcpy(a.data(), d_psd[0], a.size() * 4, hipMemcpyDeviceToHost));
  CK(hipMemcpy(b.data(), d_psd[1], b.size() * 4, hipMemcpyDeviceToHost));
  printf("queue rows vs static rows, %d frames: %s\n", nframes, memcmp(a.data(), b.data(), a.size() * 4) ? "ROWS DIFFER" : "bit-identical");
  return 0;
}
