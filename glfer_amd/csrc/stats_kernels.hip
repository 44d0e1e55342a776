// stats_kernels.hip -- per-bin epilogues over spectra the estimator kernels have produced, and the
// frame-preparation kernel.  Built with -ffp-contract=off: the float/double expression order of
// the reference IS the contract here (every statement below is the reference's statement with the
// same operand types).
//   lmp_kernel, lmp_ring_kernel, lmp_ring_any_kernel   lmp.c:132-160   detection statistic over the ring of the last nl
//                   periodograms: three forms by ring size, each placed over one stream, a batch or ragged streams (LmpPlace)
//   ftest_kernel    mtm.c:203-210, 222-233   harmonic F statistic from the tapered spectra and mu
//   prepare_kernel  fft.c:98-156    what prepare_audio leaves in inbuf_fft, for a batch of frames
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <type_traits>
#include <algorithm>
#include <vector>
#include "spectro_params.h"
#include "ragged_cols.hpp"
#include "lmp_groups.h"

#ifndef GLFER_LMP_RING
#define GLFER_LMP_RING 1    /* 0: every frame through lmp_kernel (one thread per frame and bin, nl row reads each) */
#endif

namespace glfer {
hipError_t allow_dynamic_lds(const void *kernel, size_t bytes);   // plan.h / glfer_hip.cpp

// a / d for many a and one d, correctly rounded: with y = RN(1/d) (one true division), q0 = RN(a y),
// r = a - d q0 (exact in an fma), RN(q0 + r y) = RN(a/d) (Markstein) -- the divisors here are the
// small integers nl and nl - 1, the dividends sums of a few float32 bins: nothing over- or underflows.
struct SmallDivisor {
  double d, y;
  __device__ __forceinline__ SmallDivisor(double dd, double recip) : d(dd), y(recip) {}   // recip = RN(1/dd), from the host: IEEE division either side
  __device__ __forceinline__ double operator()(double a) const {
    const double q0 = a * y;
    return __builtin_fma(__builtin_fma(-d, q0, a), y, q0);
  }
};

// ---- the LMP statistic.  The reference keeps the last nl periodograms in a ring written round-robin (slot = frame mod nl, zero
// before its first write) and sums over the SLOTS in slot order; slot j of frame f holds frame f - ((f - j) mod nl).  What is
// computed from a ring is stated once, below; the three kernels differ in where they keep the ring.
// c_neg = -sqrt(nl / 2.0) and c_den = 2.0 * sqrt(2.0 * nl) are the expression's constants (lmp.c:156), evaluated once on the host
// (IEEE sqrt: the same doubles), the two reciprocals SmallDivisor's (they were a true f64 division each, per bin: two fifths of
// the first kernel's instructions).
struct LmpConsts {
  double c_neg, c_den, recip_nl, recip_nl1;
};
static LmpConsts lmp_consts(int nl) { return LmpConsts{-sqrt(nl / 2.0), 2.0 * sqrt(2.0 * nl), 1.0 / (double)nl, 1.0 / (double)(nl - 1)}; }

// the statistic from the ring's mean and the sum of its squared deviations
__device__ __forceinline__ float lmp_value(double my, double sy, int nl, const LmpConsts &c, const SmallDivisor &by_nl1) {
  sy = by_nl1(sy);
  double v_hat = my * my - sy;                                     // lmp.c:153-159
  if (v_hat < 0.0) v_hat = 0.0;
  v_hat = 0.5 * (my - sqrt(v_hat));
  float r = c.c_neg + (nl * my) / (c.c_den * v_hat);
  if (r <= 1.0e-3) r = 1e-3;
  return r;
}
__device__ __forceinline__ float lmp_bin0() { return 1e-3; }       // lmp.c:160

// the two sums over a ring of NL registers, straight-line code; slot(j): what slot j holds
template <int NL, class Slot>
__device__ __forceinline__ void lmp_ring_sums(Slot slot, const SmallDivisor &by_nl, double &my, double &sy) {
#pragma unroll
  for (int j = 0; j < NL; j++) my += slot(j);                      // lmp.c:134-140
  my = by_nl(my);
#pragma unroll
  for (int j = 0; j < NL; j++) {                                   // lmp.c:143-149
    const double t = slot(j) - my;
    sy += t * t;
  }
}

// Where a block works is uniform over the block and stays in scalar registers:
//   One    : blockIdx.y is the group or frame, blockIdx.x the 256 bins; the block origin is the launch's own `first`, so
//            `f0 + k < end` folds to blockIdx.y * G + k < nframes;
//   Batch  : the same with blockIdx.z the stream (two strides) -- every stream has the same row_first / first / nframes;
//   Ragged : blockIdx.x is the launch's flat list of groups (lmp_groups.h; the entry found by bisection, ragged_cols.hpp: the
//            stream's first row, its frame count, its first block), blockIdx.y the 256 bins -- every stream whole from frame 0.
enum class LmpPlace { One, Batch, Ragged };
// (In the kernels' arguments the placement comes before the constants: what a block needs for its first decision -- is its frame,
// is its bin in range -- then lies in the first 64 bytes with the pointers; profiles/lmp_one_body_rate.txt, section 3.)
struct LmpStreams {
  long long row_first, first, nframes;   // One, Batch: rows holds frames row_first ..; out frames [first, first + nframes) of each stream
  long long origin;                      // Batch: the frame block (., 0, .) starts at (<= first with the register ring); One: that is `first`
  int origin_mod;                        // that frame mod nl (lmp_kernel)
  long long row_stride, out_stride;      // Batch: floats from one stream's rows / outputs to the next's
  RaggedCols r;                          // Ragged
};
struct LmpWhere {
  const float *rows;                     // the stream's row of frame row_first
  float *out;                            // its output row of frame first
  long long row_first, first, end, f0;   // f0: the block's first frame; end: one past the stream's last
  unsigned g;                            // the block's place after `origin` (Ragged: after the stream's frame 0), in blocks: < 2^31
  int i;                                 // the thread's bin
};
template <LmpPlace P>
__device__ __forceinline__ LmpWhere lmp_where(const float *rows, float *out, int bins, int G, const LmpStreams &s) {
  LmpWhere w;
  if constexpr (P == LmpPlace::Ragged) {
    const RaggedColsEntry e = ragged_cols_find(s.r, blockIdx.x);
    w.rows = rows + (size_t)e.row0 * bins;
    w.out = out + (size_t)e.row0 * bins;
    w.row_first = 0;
    w.first = 0;
    w.end = e.nframes;
    w.g = (unsigned)((long long)blockIdx.x - e.blk0);
    w.f0 = (long long)w.g * G;
    w.i = blockIdx.y * 256 + threadIdx.x;
  } else {
    w.rows = rows;
    w.out = out;
    if constexpr (P == LmpPlace::Batch) {
      w.rows += (long long)blockIdx.z * s.row_stride;
      w.out += (long long)blockIdx.z * s.out_stride;
    }
    w.row_first = s.row_first;
    w.first = s.first;
    w.end = s.first + s.nframes;
    w.g = blockIdx.y;                                              // < 65535
    w.f0 = (P == LmpPlace::Batch ? s.origin : s.first) + (long long)blockIdx.y * G;
    w.i = blockIdx.x * 256 + threadIdx.x;
  }
  return w;
}

// One thread per (frame, bin): a block is a frame, the ring is re-read from the rows (frame f - d is d rows up, zero before the
// stream's frame 0).  f mod nl is taken in 32 bits from the host's origin mod nl and the block's place after it.
// (Round 2's first form took f % nl in 64 bits and (jl - j + nl) % nl per term, two f64 square
// roots of constants and three f64 divisions per bin: 7x the time of the periodograms under it.)
// NL > 0: nl is that constant -- the ring's rows are loaded once into registers and the two sums are
// straight-line code, one copy per rotation of the ring (f mod nl is the same for the whole
// workgroup); NL = 0: any nl, by loops.
template <int NL, LmpPlace P>
__global__ __launch_bounds__(256) void lmp_kernel(const float *__restrict__ rows_all, float *__restrict__ out_all, int bins, int nl_arg,
                                                  LmpStreams s, LmpConsts c) {
  const int nl = NL > 0 ? NL : nl_arg;
  const LmpWhere p = lmp_where<P>(rows_all, out_all, bins, 1, s);
  const int i = p.i;
  const long long f = p.f0;
  if (f >= p.end || i >= bins) return;
  float *o = p.out + (size_t)(f - p.first) * bins;
  if (i == 0) {
    o[0] = lmp_bin0();
    return;
  }
  const int jl = (int)(((unsigned)s.origin_mod + p.g % (unsigned)nl) % (unsigned)nl);   // f mod nl
  const float *col = p.rows + (size_t)(f - p.row_first) * bins + i;   // this frame's row; frame f - d is d rows up
  const SmallDivisor by_nl((double)nl, c.recip_nl), by_nl1((double)(nl - 1), c.recip_nl1);
  double my = 0.0, sy = 0.0;
  if constexpr (NL > 0) {
    float v[NL];                                                   // v[d]: bin i of frame f - d (zero before the first frame)
#pragma unroll
    for (int d = 0; d < NL; d++) v[d] = (long long)d <= f ? *(col - (size_t)d * bins) : 0.0f;
    // slot j holds frame f - ((jl - j) mod nl); the sums run over the slots in slot order
    auto sums = [&](auto rc) {
      constexpr int R = decltype(rc)::value;
      lmp_ring_sums<NL>([&](int j) { return v[(R - j + NL) % NL]; }, by_nl, my, sy);
    };
    if (jl == 0) sums(std::integral_constant<int, 0>{});
    if constexpr (NL > 1) { if (jl == 1) sums(std::integral_constant<int, 1 % (NL > 0 ? NL : 1)>{}); }
    if constexpr (NL > 2) { if (jl == 2) sums(std::integral_constant<int, 2 % (NL > 0 ? NL : 1)>{}); }
    if constexpr (NL > 3) { if (jl == 3) sums(std::integral_constant<int, 3 % (NL > 0 ? NL : 1)>{}); }
    if constexpr (NL > 4) { if (jl == 4) sums(std::integral_constant<int, 4 % (NL > 0 ? NL : 1)>{}); }
    if constexpr (NL > 5) { if (jl == 5) sums(std::integral_constant<int, 5 % (NL > 0 ? NL : 1)>{}); }
    if constexpr (NL > 6) { if (jl == 6) sums(std::integral_constant<int, 6 % (NL > 0 ? NL : 1)>{}); }
    if constexpr (NL > 7) { if (jl == 7) sums(std::integral_constant<int, 7 % (NL > 0 ? NL : 1)>{}); }
    static_assert(NL <= 8, "rotations are spelled out up to 8");
  } else {
    int d = jl;                                                    // slot j holds frame f - ((jl - j) mod nl)
    for (int j = 0; j < nl; j++) {                                 // lmp.c:134-140
      const float v = (long long)d <= f ? *(col - (size_t)d * bins) : 0.0f;
      my += v;
      d = d == 0 ? nl - 1 : d - 1;
    }
    my = by_nl(my);
    d = jl;
    for (int j = 0; j < nl; j++) {                                 // lmp.c:143-149
      const float v = (long long)d <= f ? *(col - (size_t)d * bins) : 0.0f;
      sy += (v - my) * (v - my);
      d = d == 0 ? nl - 1 : d - 1;
    }
  }
  o[i] = lmp_value(my, sy, nl, c, by_nl1);
}

// The same statistic, a thread walking G consecutive frames of its bin with the ring in registers,
// indexed by SLOT as the reference's is (slot = frame mod nl): a group starts at a frame that is a
// multiple of NL, so the slot a frame goes into is known at compile time and the sums run over the
// slots in slot order with no rotation at all.  One row read per frame (plus NL - 1 per group)
// instead of NL: lmp_kernel's blocks of consecutive frames land on different XCDs, each with its own
// L2, and the re-reads came from HBM -- 40 KB per frame where 16 are needed.
// One stream: the launcher sends the frames up to the first multiple of NL through lmp_kernel, so a launch's `first` is a
// multiple of NL and its block origin.  A batch has no such head launch: its first group starts at the multiple of NL at or below `first` and the frames
// before `first` go through the ring without being summed or stored.
template <int NL, int G, LmpPlace P>
__global__ __launch_bounds__(256) void lmp_ring_kernel(const float *__restrict__ rows_all, float *__restrict__ out_all, int bins, LmpStreams s,
                                                       LmpConsts c) {
  static_assert(G % NL == 0, "a group is whole turns of the ring");
  const LmpWhere p = lmp_where<P>(rows_all, out_all, bins, G, s);
  const int i = p.i;
  const long long f0 = p.f0, end = p.end;                          // f0: a multiple of NL
  if (i >= bins || f0 >= end) return;
  const float *col = p.rows + (size_t)(f0 - p.row_first) * bins + i;   // row of frame f0; frame f0 + k is k rows down
  float w[NL], r[G];
  // Frame f0 - NL + j sits in slot j; slot 0 is f0's own before it is ever summed.  Read what the rows hold, zero the rest: the
  // callers' rows reach back min(NL - 1, first) frames from `first` (lmp_rows_reach and glfer_run_device's `back` in
  // glfer_hip.cpp), so wherever f0 >= first (one stream, ragged) every such frame >= 0 is also >= row_first and this IS the test
  // "the frame exists"; in a batch's first group a frame in [0, row_first) reads as zero too, and is overwritten before frame
  // `first` is summed.
#pragma unroll
  for (int j = 0; j < NL; j++) w[j] = (j > 0 && f0 - NL + j >= p.row_first) ? *(col - (size_t)(NL - j) * bins) : 0.0f;
#pragma unroll
  for (int k = 0; k < G; k++) r[k] = f0 + k < end ? col[(size_t)k * bins] : 0.0f;
  const SmallDivisor by_nl((double)NL, c.recip_nl), by_nl1((double)(NL - 1), c.recip_nl1);
#pragma unroll
  for (int k = 0; k < G; k++) {
    if (f0 + k >= end) return;
    w[k % NL] = r[k];
    if constexpr (P == LmpPlace::Batch) {
      if (f0 + k < p.first) continue;                              // before the call's first frame: into the ring only
    }
    float *o = p.out + (size_t)(f0 + k - p.first) * bins;
    if (i == 0) {
      o[0] = lmp_bin0();
      continue;
    }
    double my = 0.0, sy = 0.0;
    lmp_ring_sums<NL>([&](int j) { return w[j]; }, by_nl, my, sy);
    o[i] = lmp_value(my, sy, NL, c, by_nl1);
  }
}

// The same for ANY ring size up to 64 (round 4; lmp_av is a free entry of glfer's options dialog): the thread's ring in LDS
// ([slot][thread]: a column of its own, no barrier), the slot of a frame taken as frame mod nl at run time, the sums over the slots in
// slot order by loops.  One row read per frame (plus nl - 1 per group of G) where lmp_kernel<0> reads 2 nl: lmp_av = 16 at N = 4096
// ran at 16.5 M frames/s, a tenth of the rate of the periodograms under it.  Groups of G frames from `first` (from the stream's
// frame 0 when ragged).
template <LmpPlace P>
__global__ __launch_bounds__(256) void lmp_ring_any_kernel(const float *__restrict__ rows_all, float *__restrict__ out_all, int bins, int nl,
                                                           int G, LmpStreams s, LmpConsts c) {
  extern __shared__ float ring[];                                  // [nl][256]
  const LmpWhere p = lmp_where<P>(rows_all, out_all, bins, G, s);
  const int i = p.i;
  const long long f0 = p.f0, row0 = p.row_first, first = p.first;
  const long long last = p.end, end = f0 + G < last ? f0 + G : last;
  if (f0 >= last) return;
  const bool live = i < bins;
  float *w = ring + threadIdx.x;
  const float *col = p.rows + (live ? (size_t)i : 0);
  // what the ring holds when frame f0 arrives: frames f0 - nl + 1 .. f0 - 1 in their slots (zero before the stream), f0's own slot still to come
  for (int d = 1; d < nl; d++) {
    const long long f = f0 - d;
    const int slot = (int)(((f % nl) + nl) % nl);
    w[slot * 256] = (f >= 0 && live) ? col[(size_t)(f - row0) * bins] : 0.0f;
  }
  const SmallDivisor by_nl((double)nl, c.recip_nl), by_nl1((double)(nl - 1), c.recip_nl1);
  int slot = (int)(f0 % nl);
  for (long long f = f0; f < end; f++) {
    w[slot * 256] = live ? col[(size_t)(f - row0) * bins] : 0.0f;
    slot = slot + 1 == nl ? 0 : slot + 1;
    if (!live) continue;
    float *o = p.out + (size_t)(f - first) * bins;
    if (i == 0) {
      o[0] = lmp_bin0();
      continue;
    }
    double my = 0.0, sy = 0.0;
    for (int j = 0; j < nl; j++) my += w[j * 256];                 // lmp.c:134-140
    my = by_nl(my);
    for (int j = 0; j < nl; j++) {                                 // lmp.c:143-149
      const double t = w[j * 256] - my;
      sy += t * t;
    }
    o[i] = lmp_value(my, sy, nl, c, by_nl1);
  }
}

// One thread per (frame, bin).  spec: [ntap + 1][nframes][n] halfcomplex spectra (fft_radix2.c
// layout) of the frame under taper j, the last one under hn (mu); mu_live = 0: mu is all zeros (the
// reference build without FFTW never writes it, mtm.c:173).
// ROWS: the multitaper row of the frame too (mtm.c:212-219 over fft_psd, fft.c:212-216), from the same spectra:
// psd[fi][i] = sum_j cj[j] |y_j[i]|^2 with cj[j] = 1 / (n (1 + sig_j)), rows `pitch` floats apart (glfer_hip_mtm_rows_ftest_device).
template <bool ROWS>
__global__ __launch_bounds__(256) void ftest_kernel(const float *__restrict__ spec, long long nframes, int n, int ntap,
                                                    const double *__restrict__ U0, float sum_U0_sqr, int mu_live,
                                                    float *__restrict__ ftest, const float *__restrict__ cj, float *__restrict__ psd,
                                                    int pitch) {
  const long long fi = blockIdx.y;
  const int i = blockIdx.x * 256 + threadIdx.x;
  const int bins = n / 2 + 1;
  if (fi >= nframes || i >= bins) return;
  const int k = ntap - 1;                                          // params->kmax
  const size_t fstride = (size_t)nframes * n;
  const float *mu = spec + (size_t)ntap * fstride + (size_t)fi * n;
  const float mur = mu_live ? mu[i] : 0.0f;                        // mu[i]
  const float mui = mu_live ? mu[(n - i) % n] : 0.0f;              // mu[n_fft - i]  (i = 0: unused)
  float ft = 0.0;                                                  // mtm.c:179-186
  double tmpr, tmpi, num_ftest;
  if (i < (n + 1) / 2) {
    for (int j = 0; j < ntap; j++) {                               // mtm.c:203-210
      const float *ob = spec + (size_t)j * fstride + (size_t)fi * n;
      if (i == 0) {
        tmpr = ob[0] - mur * U0[j];
        ft += tmpr * tmpr;
      } else {
        tmpr = ob[i] - mur * U0[j];
        tmpi = ob[n - i] - mui * U0[j];
        ft += tmpr * tmpr + tmpi * tmpi;
      }
    }
  }
  if (i == 0) num_ftest = k * (mur * mur) * sum_U0_sqr;            // mtm.c:222-223
  else num_ftest = k * (mur * mur + mui * mui) * sum_U0_sqr;       // mtm.c:225, 230 (the Nyquist bin counts mu[n/2] twice)
  ftest[(size_t)fi * bins + i] = num_ftest / ft;
  if constexpr (ROWS) {
    float row = 0.0f;
    for (int j = 0; j < ntap; j++) {
      const float *ob = spec + (size_t)j * fstride + (size_t)fi * n;
      const float re = ob[i], im = (i == 0 || 2 * i == n) ? 0.0f : ob[n - i];     // no imaginary part at DC and Nyquist
      row += cj[j] * (re * re + im * im);
    }
    psd[(size_t)fi * (size_t)pitch + i] = row;
  }
}

// prepare_audio's output (fft.c:98-156) for frames [frame0, frame0 + nframes): history / zero
// history, RA9MB, window (NULL = rectangular: no multiply, fft.c:132,139), limiter.
template <int FMT>
__global__ __launch_bounds__(256) void prepare_kernel(SpectroParams p, int n, const float *__restrict__ window,
                                                      float *__restrict__ out) {
  const long long fi = blockIdx.x;
  if (fi >= p.nframes) return;
  const long long s0 = (p.frame0 + fi) * (long long)p.H - p.R;
  constexpr int esz = FMT == GLFER_FMT_F32 ? 4 : (FMT == GLFER_FMT_S16 ? 2 : 1);
  const char *base = reinterpret_cast<const char *>(p.stream);
  for (int i = threadIdx.x; i < n; i += 256) {
    const long long s = s0 + i;
    float x = 0.0f;
    if (s >= 0 && !(p.history_mode && i < p.R)) {
      if constexpr (FMT == GLFER_FMT_F32) x = *reinterpret_cast<const float *>(base + s * esz);
      else if constexpr (FMT == GLFER_FMT_S16) x = (float)*reinterpret_cast<const short *>(base + s * esz) / 32768;
      else x = ((float)*reinterpret_cast<const unsigned char *>(base + s) - 128) / 128;
    }
    float y;
    if (p.a > 0.0) {                                               // fft.c:127-136
      y = x / (p.a + x * x);
      if (window) y *= window[i];
    } else if (window) {                                           // fft.c:139-146
      y = window[i] * x;
    } else {                                                       // fft.c:147-148
      y = x;
    }
    if (p.limiter) {                                               // fft.c:151-156
      // (the reference's log is C's: double.  In device C++ log(float) is the float overload, up to an ulp of ftmp away,
      // which exp(0.1 ftmp) turns into several units in the last place of a small |y|^0.1: stockham16.hpp limiter_value)
      const float ftmp = (float)log((double)fabsf(y));
      y = (y > 0 ? exp(ftmp * 0.1) : -exp(ftmp * 0.1));
    }
    out[(size_t)fi * n + i] = y;
  }
}

}  // namespace glfer
using namespace glfer;

namespace {

template <int V>
using Int = std::integral_constant<int, V>;

// fn(NL, G), as integral constants, for nl's row of the ring sizes with a register form (lmp_groups.h: the only list of them --
// the instantiations are made from it); false where nl has none
template <size_t K = 0, class F>
bool lmp_ring_pair(int nl, F &&fn) {
  if constexpr (K < sizeof(glfer_lmp_ring_groups) / sizeof(glfer_lmp_ring_groups[0])) {
    if (nl != glfer_lmp_ring_groups[K][0]) return lmp_ring_pair<K + 1>(nl, fn);
    fn(Int<glfer_lmp_ring_groups[K][0]>{}, Int<glfer_lmp_ring_groups[K][1]>{});
    return true;
  } else {
    return false;
  }
}

int lmp_form(int nl) { return GLFER_LMP_RING ? glfer_lmp_form(nl) : GLFER_LMP_FORM_FRAMES; }

struct LmpCall {   // what every launch of a call is given
  const float *rows;
  float *out;
  int bins, nl;
  hipStream_t st;
};

// One launch of the form's kernel over `blocks` groups of G frames (G = 1: frames) of nb streams (a batch; else 1).  The
// rotation copies lmp_kernel<NL > 0> are one stream's: the head frames of a register-ring call.
template <LmpPlace P>
hipError_t lmp_launch(int form, const LmpCall &c, const LmpStreams &s, size_t blocks, unsigned nb, int G) {
  const unsigned bin_blocks = (unsigned)((c.bins + 255) / 256);
  const dim3 grid = P == LmpPlace::Ragged ? dim3((unsigned)blocks, bin_blocks) : dim3(bin_blocks, (unsigned)blocks, nb);
  const LmpConsts k = lmp_consts(c.nl);
  if (form == GLFER_LMP_FORM_REGISTERS) {
    lmp_ring_pair(c.nl, [&](auto NL, auto GC) {
      hipLaunchKernelGGL((lmp_ring_kernel<NL, GC, P>), grid, dim3(256), 0, c.st, c.rows, c.out, c.bins, s, k);
    });
  } else if (form == GLFER_LMP_FORM_LDS) {
    const size_t lds = (size_t)c.nl * 256 * sizeof(float);
    const hipError_t e = allow_dynamic_lds((const void *)lmp_ring_any_kernel<P>, lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(lmp_ring_any_kernel<P>, grid, dim3(256), lds, c.st, c.rows, c.out, c.bins, c.nl, G, s, k);
  } else {
    auto frames = [&](auto NL) { hipLaunchKernelGGL((lmp_kernel<NL, P>), grid, dim3(256), 0, c.st, c.rows, c.out, c.bins, c.nl, s, k); };
    bool fixed = false;
    if constexpr (P == LmpPlace::One) fixed = lmp_ring_pair(c.nl, [&](auto NL, auto) { frames(NL); });   // 4: the reference's default (glfer.c:252)
    if (!fixed) frames(Int<0>{});
  }
  return hipGetLastError();
}

// One stream or a batch: frames [s.origin, s.first + s.nframes) in blocks counted from s.origin, at most 65535 (blockIdx.y) a
// launch.  The ring in LDS takes a stream of 64 frames or more, in ONE launch (G grows until it is); shorter ones go frame by frame.
template <LmpPlace P>
hipError_t lmp_launches(int form, const LmpCall &c, LmpStreams s, unsigned nb) {
  size_t G = 1;
  if (form == GLFER_LMP_FORM_REGISTERS) {
    G = (size_t)glfer_lmp_ring_group(c.nl);
  } else if (form == GLFER_LMP_FORM_LDS && s.nframes >= 64) {
    for (G = 64; ((size_t)s.nframes + G - 1) / G > 65535;) G *= 2;
  } else {
    form = GLFER_LMP_FORM_FRAMES;
  }
  const long long origin = s.origin, first = s.first, end = s.first + s.nframes;
  const size_t blocks = ((size_t)(end - origin) + G - 1) / G;
  LmpCall cc = c;
  for (size_t b0 = 0; b0 < blocks; b0 += 65535) {
    s.origin = origin + (long long)(b0 * G);
    s.origin_mod = (int)(s.origin % c.nl);
    if (P == LmpPlace::One) {                                      // one stream: a launch is told the frames from its own first block on
      s.first = s.origin;
      s.nframes = end - s.origin;
      cc.out = c.out + (size_t)(s.origin - first) * c.bins;
    }
    const hipError_t e = lmp_launch<P>(form, cc, s, std::min<size_t>(65535, blocks - b0), nb, (int)G);
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

}  // namespace

// rows: periodograms of frames [row0, ..) (global frame indices), [.][bins]; out: frames [first, first + nframes).
extern "C" hipError_t glfer_launch_lmp(const float *rows, long long row0, long long first, size_t nframes, int bins,
                                       int nl, float *out, hipStream_t st) {
  if (nframes == 0) return hipSuccess;
  if (nl < 1 || bins < 1 || nframes > 65535u * 65535ull) return hipErrorInvalidValue;
  const LmpCall c{rows, out, bins, nl, st};
  LmpStreams s{row0, first, (long long)nframes, first, 0, 0, 0, RaggedCols{nullptr, 0}};
  int form = lmp_form(nl);
  // the ring sizes with a register form: the frames up to the first multiple of nl one by one (at most
  // nl - 1 of them, below), the rest in groups through lmp_ring_kernel
  if (form == GLFER_LMP_FORM_REGISTERS) {
    const size_t head = std::min<size_t>(nframes, (size_t)((nl - first % nl) % nl));
    if (head < nframes) {
      s.origin = first + (long long)head;
      const hipError_t e = lmp_launches<LmpPlace::One>(form, c, s, 1);
      if (e != hipSuccess) return e;
    }
    if (head == 0) return hipSuccess;
    s.origin = first;
    s.nframes = (long long)head;                                  // what is left for the frame-by-frame kernel
    form = GLFER_LMP_FORM_FRAMES;
  }
  return lmp_launches<LmpPlace::One>(form, c, s, 1);
}

// glfer_launch_lmp over nb <= 65535 streams (blockIdx.z): stream b's rows at rows + b * row_stride floats (frames row0 ..), its
// outputs at out + b * out_stride.  The forms are glfer_launch_lmp's by ring size; the register ring takes no head launch
// (lmp_ring_kernel), so a call is ONE launch per 65535 groups or frames, whatever nb is.
extern "C" hipError_t glfer_launch_lmp_batch(const float *rows, long long row0, long long first, size_t nframes, int bins, int nl,
                                             float *out, unsigned nb, long long row_stride, long long out_stride, hipStream_t st) {
  if (nframes == 0 || nb == 0) return hipSuccess;
  if (nl < 1 || bins < 1 || nb > 65535u || nframes > 65535u * 65535ull) return hipErrorInvalidValue;
  const int form = lmp_form(nl);
  const long long origin = form == GLFER_LMP_FORM_REGISTERS ? first - first % nl : first;   // the multiple of nl at or below `first`
  const LmpStreams s{row0, first, (long long)nframes, origin, 0, row_stride, out_stride, RaggedCols{nullptr, 0}};
  return lmp_launches<LmpPlace::Batch>(form, LmpCall{rows, out, bins, nl, st}, s, nb);
}

// The statistic over packed rows of streams of unequal length, every stream whole from its frame 0: stream b is rows
// [row_starts[b], row_starts[b + 1]) of `rows`, its outputs the same rows of `out`.  One launch per piece of the block list
// (lmp_groups.h: one piece up to 2^31 - 1 groups); the group length is the call's, chosen by the ring size alone.
extern "C" hipError_t glfer_launch_lmp_ragged(const float *rows, const size_t *row_starts, size_t nstreams, int bins, int nl, float *out,
                                              hipStream_t st) {
  if (nstreams == 0) return hipSuccess;
  if (nl < 1 || bins < 1 || !row_starts) return hipErrorInvalidValue;
  const int form = lmp_form(nl);
  const int G = GLFER_LMP_RING ? glfer_lmp_ragged_group(nl) : 1;
  std::vector<glfer_lmp_group_entry> groups(nstreams);
  const size_t n = glfer_lmp_group_table(row_starts, nstreams, G, GLFER_LMP_PIECE_BLOCKS, groups.data(), nullptr);
  if (n == 0) return hipSuccess;
  RaggedTable tab;
  for (size_t k = 0; k < n; k++) {
    const glfer_lmp_group_entry &g = groups[k];
    if (tab.pieces.size() <= g.piece) tab.pieces.push_back(RaggedPiece{tab.e.size(), 0, 0});
    RaggedColsEntry e = {};
    e.row0 = e.out0 = g.row0;
    e.nframes = g.nframes;
    e.blk0 = g.blk0;
    e.stream = (int)g.stream;
    tab.e.push_back(e);
    tab.pieces.back().count++;
    tab.pieces.back().blocks = g.blk0 + (g.nframes + G - 1) / G;
  }
  Scratch<RaggedColsEntry> d_tab(st);
  hipError_t err = ragged_upload({&tab}, d_tab);
  if (err != hipSuccess || !d_tab) return err;
  for (const RaggedPiece &pc : tab.pieces) {
    const LmpStreams s{0, 0, 0, 0, 0, 0, 0, tab.cols(d_tab.get(), pc)};
    err = lmp_launch<LmpPlace::Ragged>(form, LmpCall{rows, out, bins, nl, st}, s, (size_t)pc.blocks, 1, G);
    if (err != hipSuccess) break;
  }
  return err;
}

extern "C" hipError_t glfer_launch_ftest(const float *spec, size_t nframes, int n, int ntap, const double *U0,
                                         float sum_U0_sqr, int mu_live, float *ftest, hipStream_t st) {
  if (nframes == 0) return hipSuccess;
  if (nframes > 65535 || ntap < 1) return hipErrorInvalidValue;    // the caller chunks the frames
  hipLaunchKernelGGL(ftest_kernel<false>, dim3((unsigned)((n / 2 + 1 + 255) / 256), (unsigned)nframes), dim3(256), 0, st, spec,
                     (long long)nframes, n, ntap, U0, sum_U0_sqr, mu_live, ftest, (const float *)nullptr, (float *)nullptr, 0);
  return hipGetLastError();
}

// the same with the multitaper rows of the frames beside F (psd rows `pitch` floats apart, pitch >= n/2+1)
extern "C" hipError_t glfer_launch_ftest_rows(const float *spec, size_t nframes, int n, int ntap, const double *U0,
                                              float sum_U0_sqr, int mu_live, float *ftest, const float *cj, float *psd, int pitch,
                                              hipStream_t st) {
  if (nframes == 0) return hipSuccess;
  if (nframes > 65535 || ntap < 1 || !cj || !psd || pitch < n / 2 + 1) return hipErrorInvalidValue;
  hipLaunchKernelGGL(ftest_kernel<true>, dim3((unsigned)((n / 2 + 1 + 255) / 256), (unsigned)nframes), dim3(256), 0, st, spec,
                     (long long)nframes, n, ntap, U0, sum_U0_sqr, mu_live, ftest, cj, psd, pitch);
  return hipGetLastError();
}

extern "C" hipError_t glfer_launch_prepare(const SpectroParams *p, int n, const float *window, float *out,
                                           hipStream_t st) {
  if (p->nframes <= 0) return hipSuccess;
  const dim3 grid((unsigned)p->nframes), block(256);
  switch (p->fmt) {
    case GLFER_FMT_F32: hipLaunchKernelGGL(prepare_kernel<GLFER_FMT_F32>, grid, block, 0, st, *p, n, window, out); break;
    case GLFER_FMT_S16: hipLaunchKernelGGL(prepare_kernel<GLFER_FMT_S16>, grid, block, 0, st, *p, n, window, out); break;
    case GLFER_FMT_U8: hipLaunchKernelGGL(prepare_kernel<GLFER_FMT_U8>, grid, block, 0, st, *p, n, window, out); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}
