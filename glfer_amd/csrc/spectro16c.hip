// spectro16c.hip -- complex I/Q input: frame -> taper -> N-point FFT -> |Z|^2 -> taper sum, two-sided rows of N bins (gfx950).
//
// The samples are complex baseband z[n] = I[n] + i Q[n], interleaved I, Q, I, Q, ... in the plan's sample format, and the row
// of a frame is P[k] = sum_j |Z_j[k]|^2, k = 0 .. N-1, with Z_j = FFT(w_j z) and the scale sqrt(1/N) (periodogram, fft.c:212-216)
// or sqrt(1/(N (1 + sig_j))) (multitaper, mtm.c:212-219) folded into the table w_j.
//
// Layout: spectro16.hip's -- N/16 lanes per frame, 16 complex points t + T m per lane, the Stockham passes of stockham16.hpp,
// persistent blocks over rounds of (frame group, taper), the next round's loads issued from inside the passes.  What that
// kernel packs into the re / im parts of its transform are two REAL tapered copies of the frame, which it has to take apart
// again through the mirror bins (an LDS round trip and two barriers per frame); here re and im are the signal's own parts,
// every bin k of the transform is a bin of the row, and after the last pass register rho = b + B brev(q', R) of lane t holds bin
// t + T (b + B q'): sixteen sums in sixteen registers, each stored to its own column.  No fold, no barrier beyond the passes'.
//
// One load brings a whole complex sample (8, 4 or 2 bytes), one table value serves both parts, one transform serves one taper:
// any taper count, no pairing and no odd-taper form.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "stockham16.hpp"
#include "spectro_iq_params.h"

#ifndef GLFER16_STAGGER
#define GLFER16_STAGGER 8     /* as spectro16.hip */
#endif
#ifndef GLFER16_WAVES_PER_SIMD
/* spectro16.hip's choice per size: this form holds the same 48 prefetch registers and nothing for a fold */
#if defined(GLFER_LOGN) && (GLFER_LOGN == 10 || GLFER_LOGN == 11)
#define GLFER16_WAVES_PER_SIMD 2
#else
#define GLFER16_WAVES_PER_SIMD 3
#endif
#endif
#ifndef GLFER16_TW1_REGS
#define GLFER16_TW1_REGS 1
#endif

// What a round prefetches from the hook inside the passes, by size: 2 = the next round's table values and (at a frame's last
// round) the next frame's samples, spectro16.hip's scheme; 1 (N = 8192) = the samples only, the table values are loaded at the top
// of their round -- with both in flight two registers spilled; 0 (N = 16384: 1024 lanes a frame, four wavefronts per SIMD, 128
// registers of which 54 are the lane's twiddles) = nothing, samples and table are loaded at the top of every round (a frame's
// samples once per taper, from L2).  No instantiation spills: profiles/iq_kernel_resources.txt.
constexpr int spectro16c_prefetch(int logn) { return logn <= 12 ? 2 : logn == 13 ? 1 : 0; }

namespace glfer {

// One complex sample by one range-checked buffer load (out-of-range offsets read 0): wav_fmt.c:104-117 on each part.
// first / second: the two values in memory order.
template <int FMT>
__device__ __forceinline__ void buf_iq_sample(__amdgpu_buffer_rsrc_t rsrc, unsigned voff_bytes, unsigned soff_bytes, float &first,
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

// BAT: the instantiations a batch launches -- blockIdx.y is the stream (the convention of glfer_batch_select)
template <int LOGN, int FMT, int BAT, int WPS = GLFER16_WAVES_PER_SIMD, int STG = GLFER16_STAGGER>
__global__ __launch_bounds__(Launch16<LOGN>::BLOCK, WPS) void spectro16c_kernel(IqParams p) {
  if constexpr (BAT != 0) {
    const long long b = (long long)blockIdx.y;
    p.stream = reinterpret_cast<const char *>(p.stream) + b * p.batch_stride;
    p.psd = p.psd + b * p.psd_batch_stride;
  }
  using C = Plan16<LOGN>;
  using L = Launch16<LOGN>;
  constexpr int N = C::N, T = C::T, NPASS = C::NPASS, FPB = L::FPB, PADN = L::PADN;
  constexpr int TW1 = 15;                       // pass-1 (Ls=16) twiddles: shared LDS table
  constexpr int NTWR = C::NTW - TW1;            // later passes: per lane, in registers
  constexpr int PF = spectro16c_prefetch(LOGN);
  constexpr unsigned csz = FMT == GLFER_FMT_F32 ? 8 : (FMT == GLFER_FMT_S16 ? 4 : 2);   // bytes of a complex sample
  __shared__ v2f32 lds[L::LDS_WORDS];

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
  constexpr bool TW1R = (GLFER16_TW1_REGS) != 0 && (LOGN == 10 || LOGN == 11 || LOGN == 8);
  Tw1Source<TW1R> tw1row;
  tw1row.init(tw1 + (t & 15) * 17);

  const __amdgpu_buffer_rsrc_t trsrc = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<float *>(p.taps), 0, p.ntap * N * 4, 0x00020000);
  const long long stride = (long long)gridDim.x * FPB;

  // ---- registers filled ahead of use: the frame's samples in memory order (once per frame) and the NEXT round's table
  float pa[16], pb[16], pw[16];
  auto prefetch_x = [&](long long fblk, unsigned t) {
    // as spectro16.hip's gather, in complex samples: index of frame-relative sample j is sblk + flc*H + j, the descriptor
    // starts at sample max(sblk, 0), samples before the stream get an offset past the range and read 0
    // (fblk < nframes <= 2^31 - 1 and fl < 16: the sum fits 32 bits unsigned)
    const unsigned flc = FPB == 1 || (unsigned)fblk + fl < (unsigned)p.nframes ? fl : (unsigned)(p.nframes - 1 - fblk);   // clamp: loads stay in range
    const long long sblk = (p.frame0 + fblk) * (long long)p.H - p.R;
    const long long sbase = sblk > 0 ? sblk : 0;
    const __amdgpu_buffer_rsrc_t xrsrc = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<char *>(reinterpret_cast<const char *>(p.stream)) + sbase * (long long)csz, 0, 0x7fffffff, 0x00020000);
    const int lrel = (int)(sblk - sbase) + (int)(flc * (unsigned)p.H + t);   // lane's first sample, relative to sbase
    if (sblk >= 0 && p.history_mode == 0) {        // wave-uniform: no per-element predicate needed
      static_for<0, 16>([&](auto mc) {
        constexpr int m = decltype(mc)::value;
        buf_iq_sample<FMT>(xrsrc, (unsigned)lrel * csz, (unsigned)(T * m) * csz, pa[m], pb[m]);
      });
    } else {
      // first frames of the stream, or history zeroed in every frame: per-element offset, forced out of range where zero is due
      static_for<0, 16>([&](auto mc) {
        constexpr int m = decltype(mc)::value;
        const int j = T * m + (int)t;
        const int rel = lrel + T * m;
        const bool ok = p.history_mode ? (j >= p.R) : (rel >= 0);
        float a, b;
        buf_iq_sample<FMT>(xrsrc, ok ? (unsigned)rel * csz : 0x80000000u, 0u, a, b);
        pa[m] = ok ? a : 0.0f;             // raw 0 is not sample 0.0 for u8 ((0-128)/128)
        pb[m] = ok ? b : 0.0f;
      });
    }
  };
  auto prefetch_taps = [&](int tap, unsigned t) {
    // table layout [taper][m/4][lane][4] = w_j at samples t + T*m .. t + T*(m+3): four 16-byte loads per round
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
  int tap = 0;
  if constexpr (PF >= 1) prefetch_x(fblk, t);
  if constexpr (PF >= 2) prefetch_taps(0, t);

  float acc[16];
#pragma unroll
  for (int r = 0; r < 16; r++) acc[r] = 0.0f;
  const bool swap = (p.flags & GLFER_IQ_SWAP) != 0;
  // GLFER_IQ_CENTERED: bin k goes to column (k + N/2) mod N = k ^ N/2: for the lane's bins t + T c a flip of c's top bit, applied
  // to the byte offset T c * 4 of the store (t < T stays outside it)
  const unsigned cshift = (p.flags & GLFER_IQ_CENTERED) ? 8u * T * 4u : 0u;

  while (true) {
    // N = 16384 (1024 lanes a frame: four wavefronts per SIMD, 128 registers): the lane's index is made opaque per round, so that
    // the dozen addresses derived from it are recomputed here (a few VALU operations) instead of held across the loop
    unsigned tl = t;
    if constexpr (LOGN == 14) {
      asm volatile("" : "+v"(tl));
      tw1row.init(tw1 + (tl & 15) * 17);
    }
    if constexpr (PF < 1) prefetch_x(fblk, tl);
    if constexpr (PF < 2) prefetch_taps(tap, tl);
    // ---- z = (I + i Q) w_j; GLFER_IQ_SWAP: the first value of a pair is Q (a wave-uniform choice of registers)
    float zr[16], zi[16];
    if (swap) {
#pragma unroll
      for (int m = 0; m < 16; m++) {
        zr[m] = pb[m] * pw[m];
        zi[m] = pa[m] * pw[m];
      }
    } else {
#pragma unroll
      for (int m = 0; m < 16; m++) {
        zr[m] = pa[m] * pw[m];
        zi[m] = pb[m] * pw[m];
      }
    }

    // ---- which round comes next (wave-uniform)
    int ntap = tap + 1;
    long long nfblk = fblk;
    if (ntap == p.ntap) {
      ntap = 0;
      nfblk += stride;
    }
    const bool has_next = nfblk < p.nframes;

    // ---- Stockham passes; the next round's loads go out after the first exchange's writes
    stockham16_passes<LOGN, NT>(zr, zi, xb, tl, tw1row, twr, twi, [&] {
      if (has_next) {
        if constexpr (PF >= 2) prefetch_taps(ntap, tl);
        if constexpr (PF >= 1) {
          if (ntap == 0) prefetch_x(nfblk, tl);
        }
      }
    });

#pragma unroll
    for (int r = 0; r < 16; r++)
      acc[r] = __builtin_fmaf(zr[r], zr[r], __builtin_fmaf(zi[r], zi[r], acc[r]));

    if (ntap == 0) {
      // ---- the frame's last taper: register rho = b + B*brev(q',R) holds bin t + T*(b + B*q')
      constexpr int R = C::radix(NPASS - 1), B = 16 / R;
      if constexpr (FPB == 1) {
        // one frame per block: the row is wave-uniform -- a descriptor on it and 32-bit lane offsets, no per-lane pointer to keep
        const __amdgpu_buffer_rsrc_t orsrc = __builtin_amdgcn_make_buffer_rsrc(
            p.psd + (size_t)fblk * (size_t)p.pitch, 0, N * 4, 0x00020000);
        static_for<0, 16>([&](auto rc) {
          constexpr int rho = decltype(rc)::value;
          constexpr int c = rho % B + B * brev(rho / B, R);
          __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(acc[rho]), orsrc, tl * 4u, (unsigned)(T * c) * 4u ^ cshift, 0);
        });
      } else if ((unsigned)fblk + fl < (unsigned)p.nframes) {
        float *o = p.psd + ((size_t)fblk + fl) * (size_t)p.pitch + tl;
        static_for<0, 16>([&](auto rc) {
          constexpr int rho = decltype(rc)::value;
          constexpr int c = rho % B + B * brev(rho / B, R);
          o[(unsigned)(T * c) ^ (cshift >> 2)] = acc[rho];
        });
      }
#pragma unroll
      for (int r = 0; r < 16; r++) acc[r] = 0.0f;
    }
    if (!has_next) break;
    fblk = nfblk;
    tap = ntap;
  }
}

}  // namespace glfer

// ---------------------------------------------------------------------------
// host-side launcher (called from glfer_hip.cpp).  One translation unit per LOGN (-DGLFER_LOGN=...).
#include "launch16.hpp"
using namespace glfer;

#ifndef GLFER_LOGN
#error "compile with -DGLFER_LOGN=<log2 of the block size>"
#endif
#define GLFER_CAT2(a, b) a##b
#define GLFER_CAT(a, b) GLFER_CAT2(a, b)

template <int FMT, int BAT>
static hipError_t launch16c_fmt(const IqParams &p, hipStream_t st) {
  constexpr int L = GLFER_LOGN;
  using LC = Launch16<L>;
  // persistent blocks, spectro16.hip's shape: enough to fill every CU at the kernel's occupancy, never more than the work
  const long long work = ((long long)p.nframes + LC::FPB - 1) / LC::FPB;
  if (work <= 0 || p.ntap <= 0) return hipSuccess;
  const long long resident = resident_workgroups(GLFER16_WAVES_PER_SIMD, LC::BLOCK);
  const unsigned grid = persistent_grid(work, glfer_batch_cap(4 * resident, p.nbatch));
  return launch(spectro16c_kernel<L, FMT, BAT>, batch_grid(grid, p), dim3(LC::BLOCK), 0, st, p);
}

extern "C" hipError_t GLFER_CAT(glfer_launch_spectro16c_n, GLFER_LOGN)(const IqParams *p, hipStream_t st) {
  return with_fmt(p->fmt, [&](auto F) { return p->nbatch > 1 ? launch16c_fmt<F(), 1>(*p, st) : launch16c_fmt<F(), 0>(*p, st); });
}
