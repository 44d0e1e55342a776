// spectro16a.hip -- Thomson's adaptively weighted multitaper rows of one real channel, and their degrees of freedom, in one pass
// (gfx950).  Rows of N/2+1 bins.  The JK instantiations add a third row, the jackknife variance of ln psd (the epilogue's end).
//
// For frame f and bin k = 0 .. N/2, with v_j the plan's K unit-energy tapers, lambda_j = 1 - beta_j their concentrations
// (beta_j = max(-sig_j, 0)) and x_f the N values the transform sees (zeroed history included):
//     E_j[k]  = |FFT(v_j x_f)[k]|^2 / N                 the eigenspectra: no 1 / (1 + sig_j) in them
//     sigma2  = sum_n x_f[n]^2 / N                      B_j = beta_j sigma2 / N, the bound on taper j's broadband leakage
//     S       = (E_0 + E_1) / 2, then `iters` sweeps of
//         u_j = (lambda_0 S + B_0) / (lambda_j S + B_j)   (u_0 = 1; a quotient whose denominator is 0 counts as 1)
//         w_j = lambda_j u_j^2
//         S   = sum_j w_j E_j / sum_j w_j
//     psd[k]  = S after the last sweep: a weighted MEAN of the eigenspectra (the fixed-weight row of spectro16.hip is a weighted
//               SUM, about K times larger on a flat spectrum)
//     dof[k]  = 2 (sum_j w_j)^2 / sum_j w_j^2 of the last sweep's weights, between 2 and 2 K
// w_j is the textbook d_j^2 = lambda_j S^2 / (lambda_j S + B_j)^2 (Thomson 1982 section V; Percival & Walden 368a, 370a) with the
// factor common to all j cancelled: u_j <= 1 and sum w >= lambda_0, so nothing underflows to 0 / 0 and a silent frame gives
// exact zero rows and dof = 2 (sum lambda)^2 / sum lambda^2, never NaN.  The result is DEFINED BY THE SWEEP COUNT, not by
// convergence: on the skirts of a strong carrier the fixed-point equation has several roots and a few bins need tens of sweeps
// (include/glfer_hip.h), so a tolerance would make a row depend on more than its frame.  All sums run in the fixed order
// j = 0, 1, ..., so sweep m's bits do not depend on how many sweeps follow.
//
// Layout: spectro16cx.hip's skeleton -- persistent blocks over rounds of (frame group, taper PAIR), the next round's loads issued
// from inside the passes, one packed transform per round -- but the two sequences in the re / im parts are tapers 2r and 2r + 1
// of the SAME frame: Z = FFT(x (v_2r + i v_2r+1)).  They are taken apart through the mirror bins as in that kernel
//     A = Z[k] + conj Z[N-k] = 2 X_2r[k]        B = (Z[k] - conj Z[N-k]) / i = 2 X_2r+1[k]
// and |A|^2 / (4N), |B|^2 / (4N) -- powers of two, exact -- are the two eigenspectra of the lane's nine bins k <= N/2.  An odd K
// ends with a lone taper: the plan's table carries a row of zeros behind it, so the round is the same code, and the B half is
// dropped.
//
// WHERE THE EIGENSPECTRA LIVE: in the lane's registers, [GLFER_ADAPTIVE_KMAX = 8][9 bins] = 72 of them, until the frame's last
// round; the lane that separated a bin also runs its sweeps and stores it, so they never cross lanes, LDS or HBM.
// The round index is wave-uniform, so "eigenspectra 2r and 2r + 1" is a select on a scalar condition per register, not an indexed
// array (and not stores under a branch: those went to scratch, see the selects below).  sigma2 comes from the samples a lane holds at the frame's first round: sixteen squares in order, a butterfly
// over the frame's lanes of a wavefront (every lane adds the same two values at every step, so all of them hold the same bits),
// and for frames wider than a wavefront the per-wavefront values through LDS, summed in wavefront order.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "stockham16.hpp"
#include "spectro_adaptive_params.h"

#ifndef GLFER16_STAGGER
#define GLFER16_STAGGER 8     /* as spectro16.hip */
#endif
// What a round prefetches from the hook inside the passes (spectro16cx.hip's meaning): 2 = the next round's two table rows and
// (at a frame's last round) the next frame's samples; 1 = the samples only.
#ifndef GLFER16A_PREFETCH
#define GLFER16A_PREFETCH 2
#endif
#ifndef GLFER16A_WAVES_PER_SIMD
#define GLFER16A_WAVES_PER_SIMD 2
#endif
#ifndef GLFER16A_TW1_REGS
#define GLFER16A_TW1_REGS 0
#endif

namespace glfer {

// the argument block through a pointer the compiler cannot see through (spectro16cx.hip's cross_kernarg): what the epilogue
// reads is loaded there and not held in scalar registers across the round loop
__device__ __forceinline__ const __attribute__((address_space(4))) AdaptiveParams *adaptive_kernarg() {
  const __attribute__((address_space(4))) AdaptiveParams *kp =
      (const __attribute__((address_space(4))) AdaptiveParams *)__builtin_amdgcn_kernarg_segment_ptr();
  asm volatile("" : "+s"(kp));
  return kp;
}

// BAT: the instantiations a batch launches -- blockIdx.y is the stream.  JK: the jackknife form (the epilogue's second half)
template <int LOGN, int FMT, int BAT, int JK = 0, int WPS = GLFER16A_WAVES_PER_SIMD, int STG = GLFER16_STAGGER>
__global__ __launch_bounds__(Launch16<LOGN>::BLOCK, WPS) void spectro16a_kernel(AdaptiveParams p) {
  using C = Plan16<LOGN>;
  using L = Launch16<LOGN>;
  constexpr int N = C::N, T = C::T, NPASS = C::NPASS, FPB = L::FPB, PADN = L::PADN;
  constexpr int TW1 = 15;                       // pass-1 (Ls=16) twiddles: shared LDS table
  constexpr int NTWR = C::NTW - TW1;            // later passes: per lane, in registers
  constexpr int PF = GLFER16A_PREFETCH;
  constexpr int KMAX = GLFER_ADAPTIVE_KMAX;
  constexpr unsigned csz = FMT == GLFER_FMT_F32 ? 4 : (FMT == GLFER_FMT_S16 ? 2 : 1);   // bytes of a sample
  constexpr int R = C::radix(NPASS - 1), B = 16 / R;   // after the passes register rho = b + B*brev(q',R) holds bin t + T*(b + B*q')
  constexpr int WPF = T > 64 ? T / 64 : 1;             // wavefronts per frame
  __shared__ v2f32 lds[L::LDS_WORDS];
  __shared__ float s2slot[2][FPB * WPF];               // T > 64: a frame's sum of squares, per wavefront

  const unsigned tid = threadIdx.x;
  const unsigned t = tid % T;
  const unsigned fl = tid / T;
  v2f32 *xb = lds + fl * PADN;
  v2f32 *tw1 = lds + FPB * PADN;                // [k][q] = W_256^(k*q), k,q < 16

  // ---- twiddles, as spectro16.hip: pass 1's table to LDS, the later passes' per-lane values to registers
  {
    const v2f32 *tw = reinterpret_cast<const v2f32 *>(p.tw);
    if (tid < 256) {
      const unsigned k = tid >> 4, q = tid & 15;
      tw1[k * 17 + q] = q ? tw[(q - 1) * T + k] : v2f32{1.0f, 0.0f};
    }
  }
  constexpr int NT = NTWR > 0 ? NTWR : 1;
  float twr[NT], twi[NT];
  {
    const v2f32 *tw = reinterpret_cast<const v2f32 *>(p.tw) + t;
#pragma unroll
    for (int e = 0; e < NTWR; e++) {
      const v2f32 w = tw[(TW1 + e) * T];
      twr[e] = w.x;
      twi[e] = w.y;
    }
  }
  __syncthreads();
  constexpr bool TW1R = (GLFER16A_TW1_REGS) != 0;
  Tw1Source<TW1R> tw1row;
  tw1row.init(tw1 + (t & 15) * 17);

  // two table rows a round: an odd K's table ends with a row of zeros, the lone taper's partner
  const int nrounds = (p.ntap + 1) >> 1;
  const __amdgpu_buffer_rsrc_t trsrc = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<float *>(p.taps), 0, 2 * nrounds * N * 4, 0x00020000);
  const unsigned stride = gridDim.x * (unsigned)FPB;        // (at most 4096 blocks of at most 16 frames)

  // ---- registers filled ahead of use: the frame's samples (once per frame) and the NEXT round's two table rows
  float px[16], pw0[16], pw1[16];
  auto prefetch_x = [&](long long fblk, unsigned t) {
    // spectro16cx.hip's gather in single samples: index of frame-relative sample j is sblk + flc*H + j, the descriptor starts at
    // sample max(sblk, 0), samples before the stream get an offset past the range and read 0
    const unsigned flc = FPB == 1 || (unsigned)fblk + fl < (unsigned)p.nframes ? fl : (unsigned)(p.nframes - 1 - fblk);   // clamp: loads stay in range
    // once per frame: everything but the frame count comes from the argument block here, so that none of it -- nor the sixteen
    // lane masks of the history test below, which are loop invariants otherwise -- is held in scalar registers across the rounds
    const __attribute__((address_space(4))) AdaptiveParams *kp = adaptive_kernarg();
    const int H = kp->H, R = kp->R, history_mode = kp->history_mode;
    const char *stream = reinterpret_cast<const char *>(kp->stream) + (BAT != 0 ? (long long)blockIdx.y * kp->batch_stride : 0);
    const long long sblk = (kp->frame0 + fblk) * (long long)H - R;
    const long long sbase = sblk > 0 ? sblk : 0;
    const __amdgpu_buffer_rsrc_t xrsrc = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<char *>(stream) + sbase * (long long)csz, 0, 0x7fffffff, 0x00020000);
    const int lrel = (int)(sblk - sbase) + (int)(flc * (unsigned)H + t);   // lane's first sample, relative to sbase
    if (sblk >= 0 && history_mode == 0) {          // wave-uniform: no per-element predicate needed
      static_for<0, 16>([&](auto mc) {
        constexpr int m = decltype(mc)::value;
        px[m] = buf_sample<FMT>(xrsrc, (unsigned)lrel * csz, (unsigned)(T * m) * csz);
      });
    } else {
      // first frames of the stream, or history zeroed in every frame: per-element offset, forced out of range where zero is due
      static_for<0, 16>([&](auto mc) {
        constexpr int m = decltype(mc)::value;
        const int j = T * m + (int)t;
        const int rel = lrel + T * m;
        const bool ok = history_mode ? (j >= R) : (rel >= 0);
        const float a = buf_sample<FMT>(xrsrc, ok ? (unsigned)rel * csz : 0x80000000u, 0u);
        px[m] = ok ? a : 0.0f;             // raw 0 is not sample 0.0 for u8 ((0-128)/128)
      });
    }
  };
  auto prefetch_taps = [&](int rnd, unsigned t) {
    // table layout [taper][m/4][lane][4] = v_j at samples t + T*m .. t + T*(m+3): four 16-byte loads per taper
    static_for<0, 2>([&](auto hc) {
      constexpr int h = decltype(hc)::value;
      const unsigned tap_p = (unsigned)(2 * rnd + h) * (N * 4u);      // byte offset of this taper's table (uniform)
      static_for<0, 4>([&](auto mc) {
        constexpr int mq = decltype(mc)::value;
        typedef float v4f32 __attribute__((ext_vector_type(4)));
        const v4f32 q = __builtin_bit_cast(v4f32, __builtin_amdgcn_raw_buffer_load_b128(trsrc, t * 16u, tap_p + (unsigned)(T * mq) * 16u, 0));
        float *pw = h ? pw1 : pw0;
        pw[4 * mq] = q.x;
        pw[4 * mq + 1] = q.y;
        pw[4 * mq + 2] = q.z;
        pw[4 * mq + 3] = q.w;
      });
    });
  };

  if constexpr (STG > 0) {
    // de-phase co-resident blocks so that their VALU, LDS and load phases interleave
    const unsigned ph = (blockIdx.x >> 8) & 3;
    for (unsigned i = 0; i < ph; i++) __builtin_amdgcn_s_sleep(STG);
  }
  long long fblk = (long long)xcd_block_index() * FPB;
  if (fblk >= p.nframes) return;
  int rnd = 0;
  if constexpr (PF >= 1) prefetch_x(fblk, t);
  if constexpr (PF >= 2) prefetch_taps(0, t);

  // the eigenspectra, by taper and bin register (bins k <= N/2: the registers with b + B q' <= 8; the others stay unused)
  // (every index below is a compile-time constant)
  float es[KMAX][16];
  static_for<0, KMAX>([&](auto jc) {
    static_for<0, 16>([&](auto rc) { es[decltype(jc)::value][decltype(rc)::value] = 0.0f; });
  });

  float s2 = 0.0f;                                   // the frame's sum of squares (T <= 64), else this wavefront's part of it
  unsigned par = 0;
  asm volatile("" : "+v"(par));                      // (kept in a vector register: the scalar ones are the scarce kind here)

  while (true) {
    const unsigned tl = t;
    if constexpr (PF < 1) {
      if (rnd == 0) prefetch_x(fblk, tl);
    }
    if constexpr (PF < 2) prefetch_taps(rnd, tl);
    if (rnd == 0) {
      // ---- sum of the frame's squares, in a fixed order: the lane's sixteen, then a butterfly over the frame's lanes of this
      // wavefront (both partners add the same two values: every lane ends with the same bits)
      float s = 0.0f;
#pragma unroll
      for (int m = 0; m < 16; m++) s = __builtin_fmaf(px[m], px[m], s);
      constexpr int WL = T < 64 ? T : 64;
#pragma unroll
      for (int d = 1; d < WL; d <<= 1) {
#pragma clang fp contract(off)
        s = s + __shfl_xor(s, d, 64);
      }
      s2 = s;
      if constexpr (T > 64) {
        // slots of the frame's parity: the previous frame's epilogue may still be reading the other set; the barriers of the
        // passes lie between this write and the epilogue's reads, and between those reads and the next write of these slots
        par ^= 1u;
        if ((tl & 63u) == 0) s2slot[par][fl * WPF + (tl >> 6)] = s;
      }
    }
    // ---- z = x (v_2r + i v_2r+1)
    float zr[16], zi[16];
#pragma unroll
    for (int m = 0; m < 16; m++) {
      zr[m] = px[m] * pw0[m];
      zi[m] = px[m] * pw1[m];
    }

    // ---- which round comes next (wave-uniform)
    int nrnd = rnd + 1;
    long long nfblk = fblk;
    if (nrnd == nrounds) {
      nrnd = 0;
      nfblk += stride;
    }
    const bool has_next = nfblk < p.nframes;

    // ---- Stockham passes; the next round's loads go out after the first exchange's writes
    stockham16_passes<LOGN, NT>(zr, zi, xb, tl, tw1row, twr, twi, [&] {
      if (has_next) {
        if constexpr (PF >= 2) prefetch_taps(nrnd, tl);
        if constexpr (PF >= 1) {
          if (nrnd == 0) prefetch_x(nfblk, tl);
        }
      }
    });

    // ---- the exchange of spectro16cx.hip: Z to LDS by bin, one barrier, and every lane reads the mirror bins of its bins
    // k <= N/2.  xb is the transform's own buffer; the passes left it free (GLFER16_BARRIER_AFTER_READS)
    frame_sync<T>();
    static_for<0, 16>([&](auto rc) {
      constexpr int rho = decltype(rc)::value;
      constexpr int b = rho % B, qp = brev(rho / B, R);
      xb[(int)tl + T * (b + B * qp)] = v2f32{zr[rho], zi[rho]};
    });
    frame_sync<T>();
    const float escale = 0.25f * adaptive_kernarg()->inv_n;       // the two halves of the separation, and 1 / N: a power of two
    float ea[16], eb[16];
    static_for<0, 16>([&](auto rc) {
      constexpr int rho = decltype(rc)::value;
      constexpr int b = rho % B, qp = brev(rho / B, R);
      if constexpr (b + B * qp <= 8) {
        const int k = (int)tl + T * (b + B * qp);
        const v2f32 zm = xb[(N - k) & (N - 1)];                    // Z[N-k] (k = 0: Z[0] itself; k = N/2: itself)
        float ar, ai, br, bi;
        {
#pragma clang fp contract(off)
          ar = zr[rho] + zm.x;                                     // A = Z[k] + conj Z[N-k] = 2 X_2r[k]
          ai = zi[rho] - zm.y;
          br = zi[rho] + zm.y;                                     // B = (Z[k] - conj Z[N-k]) / i = 2 X_2r+1[k]
          bi = zm.x - zr[rho];
        }
        ea[rho] = escale * __builtin_fmaf(ar, ar, ai * ai);
        eb[rho] = escale * __builtin_fmaf(br, br, bi * bi);
      } else {
        ea[rho] = eb[rho] = 0.0f;
      }
    });
    // mirror bins read: the barrier that frees the buffer for the next round's first-pass writes
    if constexpr (GLFER16_BARRIER_AFTER_READS != 0) frame_sync<T>();
    // the round's two eigenspectra to their registers (rnd is wave-uniform; a lone last taper's B half is dropped below: the
    // sweeps read tapers j < K only)
    static_for<0, KMAX / 2>([&](auto pc) {
      constexpr int pr = decltype(pc)::value;
      // (selects of values, not stores under a branch: the branches' common stores are merged into one store through a
      // pointer chosen at run time otherwise, and the array goes to scratch)
      const bool mine = rnd == pr;
      static_for<0, 16>([&](auto rc) {
        constexpr int r = decltype(rc)::value;
        if constexpr (r % B + B * brev(r / B, R) <= 8) {
          es[2 * pr][r] = mine ? ea[r] : es[2 * pr][r];
          es[2 * pr + 1][r] = mine ? eb[r] : es[2 * pr + 1][r];
        }
      });
    });

    if (nrnd == 0) {
      // ---- the frame's last round: sigma2, the sweeps over the lane's nine bins, the stores.  Bin N/2 is register
      // b + B q' = 8 of lane 0 alone.
      float ssum = s2;
      if constexpr (T > 64) {
        ssum = 0.0f;
#pragma unroll
        for (int w = 0; w < WPF; w++) {
#pragma clang fp contract(off)
          ssum = ssum + s2slot[par][fl * WPF + w];
        }
      }
      if ((unsigned)fblk + fl < (unsigned)p.nframes) {
        const size_t f = (size_t)fblk + fl;
        // the weights, the sweep count, the output pointers and their pitch are read from the argument block HERE, once per frame
        const __attribute__((address_space(4))) AdaptiveParams *kp = adaptive_kernarg();
        const int K = kp->ntap, iters = kp->iters;
        const float inv_n = kp->inv_n;
        const float sigma2 = ssum * inv_n;
        float lam[KMAX], bj[KMAX];
        static_for<0, KMAX>([&](auto jc) {
          constexpr int j = decltype(jc)::value;
          lam[j] = kp->lam[j];
          bj[j] = kp->beta[j] * sigma2 * inv_n;                    // B_j: one rounding, the second factor is a power of two
        });
        const long long rpitch = kp->row_pitch;
        const long long roff = BAT != 0 ? (long long)blockIdx.y * kp->row_batch_stride : 0;
        float *const o_psd = kp->psd ? kp->psd + roff : nullptr;
        float *const o_dof = kp->dof ? kp->dof + roff : nullptr;

        float S[16], dofv[16];
        // one sweep over the lane's bins; LAST: the degrees of freedom of this sweep's weights as well
        auto sweep = [&](auto lastc) {
          constexpr bool LAST = decltype(lastc)::value;
          static_for<0, 16>([&](auto rc) {
#pragma clang fp contract(off)
            constexpr int rho = decltype(rc)::value;
            constexpr int c = rho % B + B * brev(rho / B, R);
            if constexpr (c <= 8) {
              const float s = S[rho];
              const float num = __builtin_fmaf(lam[0], s, bj[0]);
              float sw = lam[0], sw2 = lam[0] * lam[0], acc = lam[0] * es[0][rho];
              static_for<1, KMAX>([&](auto jc) {
                constexpr int j = decltype(jc)::value;
                if (j < K) {
                  const float den = __builtin_fmaf(lam[j], s, bj[j]);
                  const float u = den == 0.0f ? 1.0f : num / den;
                  const float w = (lam[j] * u) * u;
                  sw = sw + w;
                  if constexpr (LAST) sw2 = __builtin_fmaf(w, w, sw2);
                  acc = __builtin_fmaf(w, es[j][rho], acc);
                }
              });
              S[rho] = acc / sw;
              if constexpr (LAST) dofv[rho] = (2.0f * sw) * sw / sw2;
            }
          });
        };
        static_for<0, 16>([&](auto rc) {
#pragma clang fp contract(off)
          constexpr int r = decltype(rc)::value;
          S[r] = 0.5f * (es[0][r] + es[1][r]);
          dofv[r] = 0.0f;
        });
        for (int it = 1; it < iters; it++) sweep(std::false_type{});
        if constexpr (JK == 0) {
          sweep(std::true_type{});

          static_for<0, 16>([&](auto rc) {
            constexpr int rho = decltype(rc)::value;
            constexpr int c = rho % B + B * brev(rho / B, R);
            if constexpr (c <= 8) {
              if (c < 8 || tl == 0) {
                const unsigned k = tl + (unsigned)(T * c);
                if (o_psd) o_psd[f * (size_t)rpitch + k] = S[rho];
                if (o_dof) o_dof[f * (size_t)rpitch + k] = dofv[rho];
              }
            }
          });
        } else {
          // ---- THE JACKKNIFE FORM: bin by bin, the last sweep with its K weights kept, the delete-one estimates over them, the
          // three stores -- no array of dof or logvar, and one bin's weights live at a time.  The last sweep is sweep(LAST)'s
          // arithmetic operation for operation, so psd and dof are the bits of the JK = 0 form at the same sweep count;
          // iters = 0: no sweep, w_j = lambda_j (the eigenvalue-weighted mean).  With the weights HELD FIXED
          //     S_(i) = sum_{j != i} w_j E_j / sum_{j != i} w_j      summed in the order j = 0, 1, ... without i, never as
          //                                                          total - term (one dominant taper would lose every bit)
          //     l_i   = ln(S_(i) / S)                                of the ratio, which lies near 1: a row 200 dB down does not
          //                                                          carry |ln S| ulps into differences of a few 1e-3
          //     logvar = ((K - 1) / K) sum_i (l_i - mean l)^2
          // S == 0 gives 0; S > 0 with a delete-one estimate of 0 (or a ratio that leaves the float range) gives +inf; never NaN.
          float *const o_lv = kp->logvar ? kp->logvar + roff : nullptr;
          const float kf = (float)K;
          static_for<0, 16>([&](auto rc) {
#pragma clang fp contract(off)
            constexpr int rho = decltype(rc)::value;
            constexpr int c = rho % B + B * brev(rho / B, R);
            if constexpr (c <= 8) {
              const float s = S[rho];
              const float num = __builtin_fmaf(lam[0], s, bj[0]);
              float w[KMAX];
              w[0] = lam[0];
              float sw = lam[0], sw2 = lam[0] * lam[0], acc = lam[0] * es[0][rho];
              static_for<1, KMAX>([&](auto jc) {
                constexpr int j = decltype(jc)::value;
                float wj = 0.0f;                                   // a taper the plan does not have: weight 0, its terms add 0
                if (j < K) {
                  const float den = __builtin_fmaf(lam[j], s, bj[j]);
                  const float u = den == 0.0f ? 1.0f : num / den;
                  wj = iters == 0 ? lam[j] : (lam[j] * u) * u;
                  sw = sw + wj;
                  sw2 = __builtin_fmaf(wj, wj, sw2);
                  acc = __builtin_fmaf(wj, es[j][rho], acc);
                }
                w[j] = wj;
              });
              const float psd = acc / sw;
              const float dof = (2.0f * sw) * sw / sw2;
              float l[KMAX], lsum = 0.0f;
              float pn = 0.0f, pd = 0.0f;          // the terms j < i, summed once: every delete-one sum begins with the same ones
              bool unbounded = false;
              static_for<0, KMAX>([&](auto ic) {
                constexpr int i = decltype(ic)::value;
                float li = 0.0f;
                if (i < K) {
                  float ni = pn, di = pd;
                  static_for<i + 1, KMAX>([&](auto jc) {
                    constexpr int j = decltype(jc)::value;
                    ni = __builtin_fmaf(w[j], es[j][rho], ni);
                    di = di + w[j];
                  });
                  li = ni == 0.0f ? -__builtin_inff() : __builtin_logf((ni / di) / psd);
                  unbounded = unbounded || !(__builtin_fabsf(li) < __builtin_inff());
                  lsum = lsum + li;
                  pn = __builtin_fmaf(w[i], es[i][rho], pn);
                  pd = pd + w[i];
                }
                l[i] = li;
              });
              const float lbar = lsum / kf;
              float ss = 0.0f;
              static_for<0, KMAX>([&](auto ic) {
                constexpr int i = decltype(ic)::value;
                const float d = i < K ? l[i] - lbar : 0.0f;
                ss = __builtin_fmaf(d, d, ss);
              });
              float lv = ((kf - 1.0f) / kf) * ss;
              lv = unbounded || !(lv >= 0.0f) ? __builtin_inff() : lv;
              lv = psd == 0.0f ? 0.0f : lv;
              if (c < 8 || tl == 0) {
                const unsigned k = tl + (unsigned)(T * c);
                if (o_psd) o_psd[f * (size_t)rpitch + k] = psd;
                if (o_dof) o_dof[f * (size_t)rpitch + k] = dof;
                if (o_lv) o_lv[f * (size_t)rpitch + k] = lv;
              }
            }
          });
        }
      }
    }
    if (!has_next) break;
    fblk = nfblk;
    rnd = nrnd;
  }
}

}  // namespace glfer

// ---------------------------------------------------------------------------
// host-side launcher (called from adaptive.cpp).  One translation unit per LOGN (-DGLFER_LOGN=...).
#include "launch16.hpp"
using namespace glfer;

#if !defined(GLFER_LOGN) || GLFER_LOGN < 8 || GLFER_LOGN > 12
#error "compile with -DGLFER_LOGN=<log2 of the block size>, 8 .. 12"
#endif
#define GLFER_CAT2(a, b) a##b
#define GLFER_CAT(a, b) GLFER_CAT2(a, b)

// JK: the jackknife instantiations; they take iters = 0 as well (no sweep, w_j = lambda_j)
template <int FMT, int BAT, int JK = 0>
static hipError_t launch16a_fmt(const AdaptiveParams &p, hipStream_t st) {
  constexpr int L = GLFER_LOGN;
  using LC = Launch16<L>;
  // persistent blocks, spectro16cx.hip's shape: enough to fill every CU at the kernel's occupancy, never more than the work
  const long long work = ((long long)p.nframes + LC::FPB - 1) / LC::FPB;
  if (work <= 0) return hipSuccess;
  if (p.ntap < 2 || p.ntap > GLFER_ADAPTIVE_KMAX || p.iters < (JK != 0 ? 0 : 1) || p.iters > GLFER_ADAPTIVE_ITERS_MAX) return hipErrorInvalidValue;
  const long long resident = resident_workgroups(GLFER16A_WAVES_PER_SIMD, LC::BLOCK);
  const unsigned grid = persistent_grid(work, glfer_batch_cap(4 * resident, p.nbatch));
  return launch(spectro16a_kernel<L, FMT, BAT, JK>, batch_grid(grid, p), dim3(LC::BLOCK), 0, st, p);
}

extern "C" hipError_t GLFER_CAT(glfer_launch_adaptive16_n, GLFER_LOGN)(const AdaptiveParams *p, hipStream_t st) {
  return with_fmt(p->fmt, [&](auto F) { return p->nbatch > 1 ? launch16a_fmt<F(), 1>(*p, st) : launch16a_fmt<F(), 0>(*p, st); });
}

// the jackknife launcher of this size, where the Makefile's JLOGNS list names it (spectro_adaptive_params.h's GLFER_LAUNCHERS16J)
#ifdef GLFER_JACKKNIFE
extern "C" hipError_t GLFER_CAT(glfer_launch_jackknife16_n, GLFER_LOGN)(const AdaptiveParams *p, hipStream_t st) {
  return with_fmt(p->fmt, [&](auto F) { return p->nbatch > 1 ? launch16a_fmt<F(), 1, 1>(*p, st) : launch16a_fmt<F(), 0, 1>(*p, st); });
}
#endif
