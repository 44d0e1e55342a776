// spectro16cx.hip -- two real channels in one pass: multitaper auto-spectra, cross-spectrum and coherence, rows of N/2+1 bins (gfx950).
//
// The samples are pairs x[n], y[n] of two real channels, interleaved x, y, x, y, ... in the plan's sample format (spectro16c.hip's
// memory layout, a stereo recording's).  With X_j = FFT(v_j x_f), Y_j = FFT(v_j y_f) over the plan's tapers and
// c_j = 1 / (N (1 + sig_j)), for k = 0 .. N/2:
//     Sxx[k] = sum_j c_j |X_j[k]|^2      Syy[k] = sum_j c_j |Y_j[k]|^2      Sxy[k] = sum_j c_j X_j[k] conj(Y_j[k])
//     coh[k] = |Sxy[k]|^2 / (Sxx[k] Syy[k]), clamped to [0, 1], exactly 0 where Sxx[k] Syy[k] is 0
//
// Layout: spectro16c.hip's skeleton -- persistent blocks over rounds of (frame group, taper), one buffer load per pair, the plan's
// I/Q table (sqrt(c_j) folded in), the next round's loads issued from inside the passes -- and one packed transform per taper:
// Z = FFT(v_j (x + i y)) = X_j + i Y_j.  After the passes the two spectra are taken apart through the mirror bins as spectro16.hip's
// FT == 2 branch does it: Z to LDS by bin, one barrier, and for the nine registers of a lane that hold bins k <= N/2
//     A = Z[k] + conj Z[N-k] = 2 X_j[k]        B = (Z[k] - conj Z[N-k]) / i = 2 Y_j[k]
// without contraction; then |A|^2, |B|^2 and A conj(B) go into four running sums per register.  The 1/2 of the separation is a power
// of two: the sums are scaled by 1/4 at the store, so no table beyond the I/Q one is needed.  At k = 0 and k = N/2 the mirror of
// Z[k] is Z[k] itself: Im A and Im B are exact zeros there and so is Im Sxy.
//
// At the frame's last taper the quotient is formed in double from the unscaled sums (nine bins a lane, once per frame), so spectra
// anywhere in float range neither underflow the product nor overflow the square.  Each output is stored only if its pointer is
// not NULL (a wave-uniform choice).
//
// Both channels ride one transform: a channel's separated spectrum carries the rounding of the PAIR, not its own (include/glfer_hip.h).
//
// Segment averaging (the WELCH instantiations, glfer_hip_welch_cross_device): the same body with rounds of (row group, segment,
// taper).  The four sums run on over the L consecutive frames of a row before the one epilogue, so a plan of ONE window (an FFT
// plan, where a single frame's coherence is identically 1) gives the csd / coherence estimate of L averaged segments from one pass
// over the samples, with nothing between the frames' transforms and the row but registers.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "stockham16.hpp"
#include "spectro_cross_params.h"

#ifndef GLFER16_STAGGER
#define GLFER16_STAGGER 8     /* as spectro16.hip */
#endif
// What a round prefetches from the hook inside the passes (spectro16c.hip's meaning): 2 = the next round's table values and (at a
// frame's last round) the next frame's samples; 1 = the samples only, the table values are loaded at the top of their round.
// The live set is the transform's 32 registers, 36 sums (four for each of the nine bin registers), the lane's twiddles and the
// 48 prefetch registers: 20 more than spectro16c.hip holds, and too many for three wavefronts per SIMD from N = 1024 on (168
// registers: 7 to 92 spilled there).  So every size runs at two per SIMD with the whole next round prefetched, pass 1's twiddles
// in registers at N = 256 and in the shared LDS table elsewhere: 184 to 212 registers, no spill of either kind, no scratch
// (profiles/cross_kernel_resources.txt).  N = 16384 is not built: 1024 lanes a frame are four wavefronts per SIMD and 128
// registers whatever the launch bounds say, of which the twiddles take 54, the transform 32 and the sums 36.
#ifndef GLFER16CX_PREFETCH
#define GLFER16CX_PREFETCH 2
#endif
#ifndef GLFER16CX_WAVES_PER_SIMD
#define GLFER16CX_WAVES_PER_SIMD 2
#endif
#ifndef GLFER16CX_TW1_REGS
#if defined(GLFER_LOGN) && GLFER_LOGN == 8
#define GLFER16CX_TW1_REGS 1
#else
#define GLFER16CX_TW1_REGS 0
#endif
#endif

namespace glfer {

// One pair by one range-checked buffer load (out-of-range offsets read 0): spectro16c.hip's buf_iq_sample, restated here because
// that translation unit keeps it to itself.  first / second: the two values in memory order.
template <int FMT>
__device__ __forceinline__ void buf_pair_sample(__amdgpu_buffer_rsrc_t rsrc, unsigned voff_bytes, unsigned soff_bytes, float &first,
                                                float &second) {
  if constexpr (FMT == GLFER_FMT_F32) {
    typedef unsigned v2u32 __attribute__((ext_vector_type(2)));
    const v2u32 v = __builtin_amdgcn_raw_buffer_load_b64(rsrc, voff_bytes, soff_bytes, GLFER_X_LOAD_AUX);
    first = __uint_as_float(v.x);
    second = __uint_as_float(v.y);
  } else if constexpr (FMT == GLFER_FMT_S16) {
    const unsigned v = __builtin_amdgcn_raw_buffer_load_b32(rsrc, voff_bytes, soff_bytes, GLFER_X_LOAD_AUX);
    first = (float)(short)(v & 0xffffu) / 32768.0f;
    second = (float)(short)(v >> 16) / 32768.0f;
  } else {
    const unsigned v = (unsigned short)__builtin_amdgcn_raw_buffer_load_b16(rsrc, voff_bytes, soff_bytes, GLFER_X_LOAD_AUX);
    first = ((float)(v & 0xffu) - 128.0f) / 128.0f;
    second = ((float)(v >> 8) - 128.0f) / 128.0f;
  }
}

// The kernel's argument block as the kernel was launched with it, through a pointer the compiler cannot see through: what is read
// from it is loaded where it is used and not held in scalar registers across the round loop (the scarce kind here)
__device__ __forceinline__ const __attribute__((address_space(4))) CrossParams *cross_kernarg() {
  const __attribute__((address_space(4))) CrossParams *kp =
      (const __attribute__((address_space(4))) CrossParams *)__builtin_amdgcn_kernarg_segment_ptr();
  asm volatile("" : "+s"(kp));
  return kp;
}

// BAT: the instantiations a batch launches -- blockIdx.y is the stream (the convention of glfer_batch_select)
// WELCH: segment averaging (glfer_hip_welch_cross_device).  p.nframes counts output ROWS; row r sums the frames
// frame0 + r * step + s, s = 0 .. segments - 1, segments outermost and the tapers inside, and its sums are stored times p.scale.
// Rounds are (row group, segment, taper): the samples are fetched at every segment's first taper, the sums and the "has a sample"
// bits run on across the row's segments.  WELCH = 0 is the one-frame-a-row form: one segment, step 1, scale 1/4.
template <int LOGN, int FMT, int BAT, int WELCH, int WPS = GLFER16CX_WAVES_PER_SIMD, int STG = GLFER16_STAGGER>
__global__ __launch_bounds__(Launch16<LOGN>::BLOCK, WPS) void spectro16cx_kernel(CrossParams p) {
  if constexpr (BAT != 0) p.stream = reinterpret_cast<const char *>(p.stream) + (long long)blockIdx.y * p.batch_stride;
  using C = Plan16<LOGN>;
  using L = Launch16<LOGN>;
  constexpr int N = C::N, T = C::T, NPASS = C::NPASS, FPB = L::FPB, PADN = L::PADN;
  constexpr int TW1 = 15;                       // pass-1 (Ls=16) twiddles: shared LDS table
  constexpr int NTWR = C::NTW - TW1;            // later passes: per lane, in registers
  constexpr int PF = GLFER16CX_PREFETCH;
  constexpr unsigned csz = FMT == GLFER_FMT_F32 ? 8 : (FMT == GLFER_FMT_S16 ? 4 : 2);   // bytes of a pair
  constexpr int R = C::radix(NPASS - 1), B = 16 / R;   // after the passes register rho = b + B*brev(q',R) holds bin t + T*(b + B*q')
  constexpr int WPF = T > 64 ? T / 64 : 1;             // wavefronts per frame
  __shared__ v2f32 lds[L::LDS_WORDS];
  __shared__ unsigned nzslot[2][FPB * WPF];            // T > 64: which channels of a frame hold a sample that is not zero, per wavefront

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
  constexpr bool TW1R = (GLFER16CX_TW1_REGS) != 0;
  Tw1Source<TW1R> tw1row;
  tw1row.init(tw1 + (t & 15) * 17);

  const __amdgpu_buffer_rsrc_t trsrc = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<float *>(p.taps), 0, p.ntap * N * 4, 0x00020000);
  const unsigned stride = gridDim.x * (unsigned)FPB;        // (at most 4096 blocks of at most 16 frames)

  // ---- registers filled ahead of use: the frame's pairs in memory order (once per frame) and the NEXT round's table
  float pa[16], pb[16], pw[16];
  auto prefetch_x = [&](long long fblk, int seg, unsigned t) {
    // spectro16c.hip's gather, in pairs: index of frame-relative pair j is sblk + flc*H + j, the descriptor starts at pair
    // max(sblk, 0), pairs before the stream get an offset past the range and read 0
    // (fblk < nframes <= 2^31 - 1 and fl < 16: the sum fits 32 bits unsigned)
    // WELCH: fblk counts rows, the block's rows lie step frames apart and this is segment seg of each: the descriptor starts at
    // the first row's frame and a lane's row adds flc * step * H pairs to its offset, which the entry keeps inside the
    // descriptor's range ((FPB - 1) step H + N pairs are at most 2^31 - 1 bytes: glfer_hip_welch_cross_supported)
    const unsigned flc = FPB == 1 || (unsigned)fblk + fl < (unsigned)p.nframes ? fl : (unsigned)(p.nframes - 1 - fblk);   // clamp: loads stay in range
    const char *stream = reinterpret_cast<const char *>(p.stream);
    int H = p.H, R = p.R, history_mode = p.history_mode;
    long long frame = p.frame0 + fblk;
    unsigned lhop = (unsigned)H;                             // pairs from one lane row's frame to the next one's
    if constexpr (WELCH != 0) {
      // once per segment: everything but the row count comes from the argument block here, so that none of it is a scalar
      // register held across the rounds (four instantiations spilled two to four of them otherwise)
      const __attribute__((address_space(4))) CrossParams *kp = cross_kernarg();
      const long long step = kp->step;
      stream = reinterpret_cast<const char *>(kp->stream) + (BAT != 0 ? (long long)blockIdx.y * kp->batch_stride : 0);
      H = kp->H, R = kp->R, history_mode = kp->history_mode;
      frame = kp->frame0 + fblk * step + seg;
      lhop = FPB == 1 ? 0u : (unsigned)step * (unsigned)H;
    }
    const long long sblk = frame * (long long)H - R;
    const long long sbase = sblk > 0 ? sblk : 0;
    const __amdgpu_buffer_rsrc_t xrsrc = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<char *>(stream) + sbase * (long long)csz, 0, 0x7fffffff, 0x00020000);
    const int lrel = (int)(sblk - sbase) + (int)(flc * lhop + t);   // lane's first pair, relative to sbase
    if (sblk >= 0 && history_mode == 0) {          // wave-uniform: no per-element predicate needed
      static_for<0, 16>([&](auto mc) {
        constexpr int m = decltype(mc)::value;
        buf_pair_sample<FMT>(xrsrc, (unsigned)lrel * csz, (unsigned)(T * m) * csz, pa[m], pb[m]);
      });
    } else {
      // first frames of the stream, or history zeroed in every frame: per-element offset, forced out of range where zero is due
      static_for<0, 16>([&](auto mc) {
        constexpr int m = decltype(mc)::value;
        const int j = T * m + (int)t;
        const int rel = lrel + T * m;
        const bool ok = history_mode ? (j >= R) : (rel >= 0);
        float a, b;
        buf_pair_sample<FMT>(xrsrc, ok ? (unsigned)rel * csz : 0x80000000u, 0u, a, b);
        pa[m] = ok ? a : 0.0f;             // raw 0 is not sample 0.0 for u8 ((0-128)/128)
        pb[m] = ok ? b : 0.0f;
      });
    }
  };
  auto prefetch_taps = [&](int tap, unsigned t) {
    // table layout [taper][m/4][lane][4] = v_j at samples t + T*m .. t + T*(m+3): four 16-byte loads per round
    const unsigned tap_p = (unsigned)tap * (N * 4u);               // byte offset of this taper's table (uniform)
    static_for<0, 4>([&](auto mc) {
      constexpr int mq = decltype(mc)::value;
      typedef float v4f32 __attribute__((ext_vector_type(4)));
      const v4f32 q = __builtin_bit_cast(v4f32, __builtin_amdgcn_raw_buffer_load_b128(trsrc, t * 16u, tap_p + (unsigned)(T * mq) * 16u, 0));
      pw[4 * mq] = q.x;
      pw[4 * mq + 1] = q.y;
      pw[4 * mq + 2] = q.z;
      pw[4 * mq + 3] = q.w;
    });
  };

  if constexpr (STG > 0) {
    // de-phase co-resident blocks so that their VALU, LDS and load phases interleave
    const unsigned ph = (blockIdx.x >> 8) & 3;
    for (unsigned i = 0; i < ph; i++) __builtin_amdgcn_s_sleep(STG);
  }
  long long fblk = (long long)xcd_block_index() * FPB;
  if (fblk >= p.nframes) return;
  int tap = 0, seg = 0;
  if constexpr (PF >= 1) prefetch_x(fblk, 0, t);
  if constexpr (PF >= 2) prefetch_taps(0, t);

  // the four running sums, by bin register (bins k <= N/2: the registers with b + B q' <= 8; the others stay unused)
  float sxx[16], syy[16], sre[16], sim[16];
#pragma unroll
  for (int r = 0; r < 16; r++) sxx[r] = syy[r] = sre[r] = sim[r] = 0.0f;

  // bit 0 / bit 1: the frame's x / y samples are not all zero.  A silent channel's spectrum is zero, but the packed transform
  // leaves its rounding there (a real input's transform is Hermitian to rounding only), and a quotient of two roundings is no
  // coherence: the frame's rows of a channel without a sample are stored as the exact zeros they are.  T <= 64: the frame lives in
  // one wavefront, a ballot answers; else every wavefront leaves its bits in LDS at the frame's first round, in the slots of
  // the frame's parity (the previous frame's epilogue may still be reading the other set), and the epilogue reads them all --
  // the barriers of the passes lie in between.  WELCH: a row's bits are those of its segments OR-ed (a channel is silent when it
  // is in every one of them); the parity flips per segment, written at the segment's first round and read after its last
  // round's passes, so the barriers still lie between a write and its read and between a read and the next write of its slots.
  unsigned nz = 0, par = 0;
  asm volatile("" : "+v"(par));                      // (kept in a vector register: the scalar ones are the scarce kind here)

  while (true) {
    const unsigned tl = t;
    if constexpr (PF < 1) prefetch_x(fblk, seg, tl);
    if constexpr (PF < 2) prefetch_taps(tap, tl);
    if (tap == 0) {
      bool xnz = false, ynz = false;
#pragma unroll
      for (int m = 0; m < 16; m++) {
        xnz |= pa[m] != 0.0f;
        ynz |= pb[m] != 0.0f;
      }
      const unsigned long long bx = __ballot(xnz), by = __ballot(ynz);
      if constexpr (T > 64) {
        par ^= 1u;
        if ((tl & 63u) == 0) nzslot[par][fl * WPF + (tl >> 6)] = (bx ? 1u : 0u) | (by ? 2u : 0u);
      } else {
        const unsigned sh = (unsigned)(__lane_id() & ~(T - 1));            // the frame's lanes of this wavefront
        const unsigned long long fm = (T == 64 ? ~0ull : ((1ull << T) - 1)) << sh;
        const unsigned bits = ((bx & fm) ? 1u : 0u) | ((by & fm) ? 2u : 0u);
        nz = WELCH != 0 && seg != 0 ? nz | bits : bits;
      }
    }
    // ---- z = (x + i y) v_j
    float zr[16], zi[16];
#pragma unroll
    for (int m = 0; m < 16; m++) {
      zr[m] = pa[m] * pw[m];
      zi[m] = pb[m] * pw[m];
    }

    // ---- which round comes next (wave-uniform)
    int ntap = tap + 1, nseg = seg;
    long long nfblk = fblk;
    if (ntap == p.ntap) {
      ntap = 0;
      if constexpr (WELCH != 0) {
        if (++nseg == cross_kernarg()->segments) nseg = 0;
      }
      if (nseg == 0) nfblk += stride;
    }
    const bool has_next = nfblk < p.nframes;

    // ---- Stockham passes; the next round's loads go out after the first exchange's writes
    stockham16_passes<LOGN, NT>(zr, zi, xb, tl, tw1row, twr, twi, [&] {
      if (has_next) {
        if constexpr (PF >= 2) {
          if (WELCH == 0 || p.ntap != 1) prefetch_taps(ntap, tl);       // (one window: the table loaded before the loop is kept)
        }
        if constexpr (PF >= 1) {
          if (ntap == 0) prefetch_x(nfblk, nseg, tl);
        }
      }
    });

    // ---- the exchange of spectro16.hip's FT == 2 branch: Z to LDS by bin, one barrier, and every lane reads the mirror bins of
    // its bins k <= N/2.  xb is the transform's own buffer; the passes left it free (GLFER16_BARRIER_AFTER_READS)
    frame_sync<T>();
    static_for<0, 16>([&](auto rc) {
      constexpr int rho = decltype(rc)::value;
      constexpr int b = rho % B, qp = brev(rho / B, R);
      xb[(int)tl + T * (b + B * qp)] = v2f32{zr[rho], zi[rho]};
    });
    frame_sync<T>();
    static_for<0, 16>([&](auto rc) {
      constexpr int rho = decltype(rc)::value;
      constexpr int b = rho % B, qp = brev(rho / B, R);
      if constexpr (b + B * qp <= 8) {
        const int k = (int)tl + T * (b + B * qp);
        const v2f32 zm = xb[(N - k) & (N - 1)];                    // Z[N-k] (k = 0: Z[0] itself; k = N/2: itself)
        float ar, ai, br, bi;
        {
#pragma clang fp contract(off)
          ar = zr[rho] + zm.x;                                     // A = Z[k] + conj Z[N-k] = 2 X[k]
          ai = zi[rho] - zm.y;
          br = zi[rho] + zm.y;                                     // B = (Z[k] - conj Z[N-k]) / i = 2 Y[k]
          bi = zm.x - zr[rho];
        }
        sxx[rho] = __builtin_fmaf(ar, ar, __builtin_fmaf(ai, ai, sxx[rho]));
        syy[rho] = __builtin_fmaf(br, br, __builtin_fmaf(bi, bi, syy[rho]));
        sre[rho] = __builtin_fmaf(ar, br, __builtin_fmaf(ai, bi, sre[rho]));            // A conj(B)
        sim[rho] = __builtin_fmaf(ai, br, __builtin_fmaf(-ar, bi, sim[rho]));
      }
    });
    // mirror bins read: the barrier that frees the buffer for the next round's first-pass writes
    if constexpr (GLFER16_BARRIER_AFTER_READS != 0) frame_sync<T>();

    if constexpr (WELCH != 0 && T > 64) {
      if (ntap == 0) {                                   // a segment's last taper: its bits join the row's
        if (seg == 0) nz = 0;
#pragma unroll
        for (int w = 0; w < WPF; w++) nz |= nzslot[par][fl * WPF + w];
      }
    }
    if (ntap == 0 && nseg == 0) {
      // ---- the row's last taper: the quotient in double from the unscaled sums, then the stores (1/4: the two halves of the
      // separation; WELCH: p.scale, 1/4 over the segments).  Bin N/2 is register b + B q' = 8 of lane 0 alone.
      // (the per-frame form collects its bits here, as it always did: merged with the block above, its instantiations at
      // N >= 2048 come out with other register counts)
      if constexpr (WELCH == 0 && T > 64) {
        nz = 0;
#pragma unroll
        for (int w = 0; w < WPF; w++) nz |= nzslot[par][fl * WPF + w];
      }
      if ((unsigned)fblk + fl < (unsigned)p.nframes) {
        const size_t f = (size_t)fblk + fl;
        // the four output pointers and their pitches are read from the kernel's argument block HERE, once per frame, through a
        // pointer the compiler cannot see through: held across the loop they were the scalar registers that spilled
        const __attribute__((address_space(4))) CrossParams *kp = cross_kernarg();
        const float scale = WELCH != 0 ? kp->scale : 0.25f;
        const long long rpitch = kp->row_pitch, xpitch = kp->sxy_pitch;
        const long long roff = BAT != 0 ? (long long)blockIdx.y * kp->row_batch_stride : 0;
        float *const o_sxx = kp->sxx ? kp->sxx + roff : nullptr;
        float *const o_syy = kp->syy ? kp->syy + roff : nullptr;
        float *const o_coh = kp->coh ? kp->coh + roff : nullptr;
        float2 *const o_sxy = kp->sxy ? kp->sxy + (BAT != 0 ? (long long)blockIdx.y * kp->sxy_batch_stride : 0) : nullptr;
        if (nz != 3u) {                                  // a channel without a sample: its spectrum and the cross-spectrum are zero
#pragma unroll
          for (int r = 0; r < 16; r++) {
            if (!(nz & 1u)) sxx[r] = 0.0f;
            if (!(nz & 2u)) syy[r] = 0.0f;
            sre[r] = sim[r] = 0.0f;
          }
        }
        static_for<0, 16>([&](auto rc) {
          constexpr int rho = decltype(rc)::value;
          constexpr int c = rho % B + B * brev(rho / B, R);
          if constexpr (c <= 8) {
            if (c < 8 || tl == 0) {
              const unsigned k = tl + (unsigned)(T * c);
              if (o_sxx) o_sxx[f * (size_t)rpitch + k] = scale * sxx[rho];
              if (o_syy) o_syy[f * (size_t)rpitch + k] = scale * syy[rho];
              if (o_sxy) o_sxy[f * (size_t)xpitch + k] = float2{scale * sre[rho], scale * sim[rho]};
              if (o_coh) {
#pragma clang fp contract(off)
                const double den = (double)sxx[rho] * (double)syy[rho];
                const double num = (double)sre[rho] * (double)sre[rho] + (double)sim[rho] * (double)sim[rho];
                double q = den > 0.0 ? num / den : 0.0;
                q = q > 1.0 ? 1.0 : q;
                o_coh[f * (size_t)rpitch + k] = (float)q;
              }
            }
          }
        });
      }
#pragma unroll
      for (int r = 0; r < 16; r++) sxx[r] = syy[r] = sre[r] = sim[r] = 0.0f;
    }
    if (!has_next) break;
    fblk = nfblk;
    tap = ntap;
    seg = nseg;
  }
}

}  // namespace glfer

// ---------------------------------------------------------------------------
// host-side launcher (called from cross.cpp).  One translation unit per LOGN (-DGLFER_LOGN=...).
#include "launch16.hpp"
using namespace glfer;

#if !defined(GLFER_LOGN) || GLFER_LOGN < 8 || GLFER_LOGN > 13
#error "compile with -DGLFER_LOGN=<log2 of the block size>, 8 .. 13"
#endif
#define GLFER_CAT2(a, b) a##b
#define GLFER_CAT(a, b) GLFER_CAT2(a, b)

template <int FMT, int BAT, int WELCH>
static hipError_t launch16cx_fmt(const CrossParams &p, hipStream_t st) {
  constexpr int L = GLFER_LOGN;
  using LC = Launch16<L>;
  // persistent blocks, spectro16.hip's shape: enough to fill every CU at the kernel's occupancy, never more than the work
  const long long work = ((long long)p.nframes + LC::FPB - 1) / LC::FPB;
  if (work <= 0 || p.ntap <= 0) return hipSuccess;
  const long long resident = resident_workgroups(GLFER16CX_WAVES_PER_SIMD, LC::BLOCK);
  const unsigned grid = persistent_grid(work, glfer_batch_cap(4 * resident, p.nbatch));
  return launch(spectro16cx_kernel<L, FMT, BAT, WELCH>, batch_grid(grid, p), dim3(LC::BLOCK), 0, st, p);
}

extern "C" hipError_t GLFER_CAT(glfer_launch_spectro16cx_n, GLFER_LOGN)(const CrossParams *p, hipStream_t st) {
  // segments != 0: the segment-averaging instantiations (p->nframes counts rows)
  return with_fmt(p->fmt, [&](auto F) {
    if (p->segments != 0) return p->nbatch > 1 ? launch16cx_fmt<F(), 1, 1>(*p, st) : launch16cx_fmt<F(), 0, 1>(*p, st);
    return p->nbatch > 1 ? launch16cx_fmt<F(), 1, 0>(*p, st) : launch16cx_fmt<F(), 0, 0>(*p, st);
  });
}
