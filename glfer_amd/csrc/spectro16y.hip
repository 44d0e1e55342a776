// spectro16y.hip -- multitaper, odd taper count, N = 4096: the two frames that share their last
// taper's transform (spectro16x.hip) are also carried through the full rounds TOGETHER, interleaved
// in every wavefront (stockham16_passes2): while frame A's exchange writes drain through the LDS
// pipe the wavefront does frame B's butterflies, and every workgroup barrier serves both frames.
//
// tools/stampbench on the one-frame-at-a-time kernels: a round is ~36 % butterflies, ~37 % waiting
// to issue the 2x16 ds_write_b64 of the two exchanges (all four wavefronts of a frame burst into
// the LDS pipe at the same moment, 80 B/clk) and ~28 % barriers; more resident blocks do not help
// (2 and 3 per CU measure the same).  Here the overlap is built into the instruction stream.
//
// Both frames use the same taper pair in the same round, so one set of 32 prefetch VGPRs serves
// both; per lane: 2x32 transform registers, 2x16 accumulators, 2x16 samples, 32 taper values,
// 30 twiddles -- 256 VGPRs, 2 blocks (8 wavefronts) per CU, two 35 KB exchange buffers per block.
// Per frame the arithmetic is exactly spectro16x.hip's (same pairing, same scales), so the rows are
// bit-identical to it.
//
// HALF (five tapers, no in-kernel mean): the taper tables stay in registers as mirror-symmetric half tables.  DPSS tapers
// satisfy v_k[N-1-n] = (-1)^k v_k[n], and the plan's scaled float tables keep that to the bit (glfer_hip.cpp builds the
// half table only then).  In pass 0 lane t takes the samples r + 256 m of residue r = glfer_yhalf_residue(t) instead of
// r = t: residues r and 255 - r then sit at mirrored positions of one 16-lane DPP row, so for m >= 8 a lane's taper value
// is +- its row_mirror partner's value at 15 - m, taken as the DPP operand of the multiply itself.  A lane keeps m = 0..7
// of every taper, 40 floats loaded once per workgroup, and the steady-state loop has no table loads left (they were L2
// hits that queued behind other wavefronts' HBM misses on the CU's in-order return path: profiles/y_half_tapers.txt).
// The permutation touches the sample gather and the column of the first exchange's writes only; what every lane reads
// back from that exchange, and everything after it, is unchanged, and per frame the same operations meet the same values
// in the same order: the rows are bit-identical to the full-table form's.
//
// QUEUE (the plain forms: no in-kernel mean, one stream): one workgroup per resident slot, and frame pairs handed out in
// chunks of p.yq_chunk consecutive pairs.  A workgroup's first chunk is the static one (xcd_block_index()); every later one is
// gridDim.x + a ticket drawn from p.yq_counter.  Lane 0 of wavefront 0 draws the ticket (a vector atomic add with return) at
// the start of a chunk's first iteration, parks it in the pad word of the pass-1 twiddle table in front of the barrier of the
// mirror fold, and every wavefront reads it behind that barrier: the next chunk is known two dual rounds after it was asked
// for and before the shared round's hook requests its samples.  A ticket at or past the end ends the workgroup after the
// iteration in flight; a workgroup draws exactly one ticket per chunk it takes, so a launch of P chunks draws P tickets
// whatever the order (P - gridDim.x that succeed, gridDim.x that fail), and the host passes the counter's value before the
// launch as p.yq_base instead of zeroing it.  Which workgroup takes a pair changes nothing that is computed for it.
//
// SEG (the half-table forms outside the ragged build): behind the second dual round an iteration has one transform left and
// nothing to hide its LDS latency under, so that third of the iteration makes as few LDS round trips as it can.  The sums
// accA / accB stay in registers through the shared round (32 transform registers there against 64 in a dual round); in front
// of it only the wavefronts' power totals and the queue ticket cross a barrier (where the other forms also fold the mirror
// bins through both buffers, "the barrier of the mirror fold" above).  The shared round goes through both exchange buffers
// (stockham16_passes_pp: no barrier that only releases a buffer), its last butterfly stage writes the upper-half bins as
// 16-byte entries {Re Z, Im Z, accA, accB}, and the separation folds psd = acc[k] + acc[N-k] from the mirror entry it reads
// anyway (separate_fold_and_store).  13 barriers per iteration instead of 16, one LDS round trip fewer; per frame the same
// operations on the same values in the same order, so the rows are bit-identical to every other form's
// (profiles/y_shared_segment.txt).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "odd_taper.hpp"

#ifndef GLFER16Y_DPP_SUM
#define GLFER16Y_DPP_SUM 1
#endif
#ifndef GLFER16Y_SKEW
#define GLFER16Y_SKEW 1           /* stockham16_passes2s: frame B's exchange reads and the buffer-release barrier under frame A's arithmetic (+1.5 %,
                                     profiles/r03_y_skew.txt); 2: the shared round's barrier in front of its last stage too (stockham16_passes1s) */
#endif
#ifndef GLFER16Y_HALF
#define GLFER16Y_HALF 1           /* the half-table form where the plan has the table (0: every plan keeps the full-table form);
                                     1: all 40 floats resident, 2: the pairs' 32 resident, the last taper's 8 loaded per iteration */
#endif
#ifndef GLFER16Y_TW1_REGS
#define GLFER16Y_TW1_REGS 1       /* the lane's 15 pass-1 twiddles in registers instead of 15 LDS reads per transform (where they fit without a spill:
                                     not with history zeroed per frame, not the 75 % mean form): +1.5...2 %, profiles/r03_y_tw1_regs.txt */
#endif

// tools/yqbench only: GLFER_BLOCK_MARK(k) records a workgroup's clock at entry (0), in front of its first iteration (1) and
// behind its last (2).  Expands to nothing in the product build.
#ifndef GLFER_BLOCK_MARK
#define GLFER_BLOCK_MARK(k)
#endif

// GLFER_RAGGED (the Makefile compiles this source once more with it): the instantiations of the ragged batches -- the stream
// and its own frames come from SpectroParams::ragged[blockIdx.y] (GLFER_STREAM_SELECT, spectro_params.h) -- under names of their
// own, so that the instantiations without it are compiled from the code they were.
#ifdef GLFER_RAGGED
#define spectro16y_kernel spectro16y_ragged_kernel
#define glfer_launch_spectro16y_n12 glfer_launch_spectro16y_ragged_n12
#endif
// The half-table forms' single-stream third: the mirror fold inside the separation's LDS pass and the shared round through
// both exchange buffers (see the kernel's SEG; profiles/y_shared_segment.txt).  0 keeps the fold in front of the shared round
// and the one-buffer passes, as the full-table and mean forms do; the ragged instantiations stay with that.
#ifndef GLFER16Y_ONE_MIRROR_PASS
#ifdef GLFER_RAGGED
#define GLFER16Y_ONE_MIRROR_PASS 0
#else
#define GLFER16Y_ONE_MIRROR_PASS 1
#endif
#endif

namespace glfer {

hipError_t allow_dynamic_lds(const void *kernel, size_t bytes);   // plan.h / glfer_hip.cpp: once per device, kernel and size class

struct LaunchY {
  static constexpr int N = 4096, T = 256, PADN = N + N / 16;
  static constexpr int LDS_WORDS = 2 * PADN + 16 * 17 + 4;       // two exchange buffers, pass-1 twiddles, power partials
};

// ABL (tools/xbench timing ablations only; results are wrong): 1 = skip the shared round
// KM > 0: per-hop mean removal (fft.c:86-96, the reference's default) inside the kernel, for a hop of
// KM of a lane's 16 sample registers (KM = 16, 8, 4: overlap 0, 50, 75 %).  A frame spans NH = 16/KM
// hops, each a fixed group of registers; frames A and A+1 share all but one.  The sums are taken from
// the NEXT iteration's samples once they are in registers (lane partial in register order, a
// butterfly over the wavefront, the four wavefronts through LDS across the barriers that end the
// shared round), and x - mu is formed once, before the frames' first round.  A hop's mean comes from
// the same lanes' same registers in the same order whichever frame it is seen in.
template <int FMT, int ABL = 0, int HIST = 0, int KM = 0, int BAT = 0, int HALF = 0, int QUEUE = 0>
__global__ __launch_bounds__(256, 2) void spectro16y_kernel(SpectroParams p) {
  GLFER_BLOCK_MARK(0);
  // the stream of the batch (blockIdx.y; 0 outside a batch); the mean forms only in their batch instantiations (BAT), so that the
  // single-stream ones keep their registers
  if constexpr (KM == 0 || BAT != 0) GLFER_STREAM_SELECT(p);
  static_assert(KM == 0 || (HIST == 0 && (KM == 16 || KM == 8 || KM == 4)), "in-kernel mean removal: history from the stream");
  // (the hop sums of the mean forms reduce across lanes in lane order: a lane permutation would change their bits)
  static_assert(HALF == 0 || (KM == 0 && GLFER16_X0_ROWS != 0 && GLFER16_BARRIER_AFTER_READS != 0), "half tables: the plain forms, row layout of exchange 0");
  static_assert(QUEUE == 0 || (KM == 0 && BAT == 0 && ABL == 0), "frame queue: the plain single-stream forms");
  constexpr bool SEG = HALF != 0 && GLFER16Y_ONE_MIRROR_PASS != 0;
  static_assert(!SEG || ABL == 0, "the ablation reads the folded sums in front of the shared round");
  constexpr int NH = KM > 0 ? 16 / KM : 1;
  __shared__ float mred[KM > 0 ? 4 * (NH + 1) : 1];
  using C = Plan16<12>;
  using L = LaunchY;
  constexpr int N = L::N, T = L::T, PADN = L::PADN, NPASS = C::NPASS;
  constexpr int TW1 = 15;
  constexpr int NT = C::NTW - TW1;
  constexpr unsigned esz = FMT == GLFER_FMT_F32 ? 4 : (FMT == GLFER_FMT_S16 ? 2 : 1);
  typedef float v4f32 __attribute__((ext_vector_type(4)));
  extern __shared__ __attribute__((aligned(16))) v2f32 lds[];   // L::LDS_WORDS entries (72 KB: above the static limit); 16 bytes: the mirror entries of the half-table forms

  const unsigned t = threadIdx.x;
  const unsigned rc = HALF ? glfer_yhalf_residue(t) : t;   // the lane's residue in pass 0: samples rc + T*m, column rc of exchange 0
  v2f32 *xbA = lds, *xbB = lds + PADN;
  v2f32 *tw1 = lds + 2 * PADN;
  float *red = reinterpret_cast<float *>(lds + 2 * PADN + 16 * 17);   // [2][4]

  {
    const v2f32 *tw = reinterpret_cast<const v2f32 *>(p.tw);
    const unsigned k = t >> 4, q = t & 15;
    tw1[k * 17 + q] = q ? tw[(q - 1) * T + k] : v2f32{1.0f, 0.0f};
  }
  float twr[NT], twi[NT];
  {
    const v2f32 *tw = reinterpret_cast<const v2f32 *>(p.tw) + t;
#pragma unroll
    for (int e = 0; e < NT; e++) {
      const v2f32 w = tw[(TW1 + e) * T];
      twr[e] = w.x;
      twi[e] = w.y;
    }
  }
  __syncthreads();
  const v2f32 *tw1row = tw1 + (t & 15) * 17;
  constexpr bool TW1R = GLFER16Y_TW1_REGS != 0 && HIST == 0 && KM != 4;
  v2f32 tw1reg[16];
  if constexpr (TW1R) {
#pragma unroll
    for (int q = 0; q < 16; q++) tw1reg[q] = tw1row[q];
  }

  const __amdgpu_buffer_rsrc_t trsrc = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<float *>(p.taps), 0, p.npairs * 2 * N * 4, 0x00020000);
  const __amdgpu_buffer_rsrc_t vrsrc = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<float *>(p.xtaps), 0, N * 4, 0x00020000);
  const unsigned toff = t * 16u;
  const int NP = p.npairs - 1;                       // full (two-taper) rounds per frame
  const long long stride = (long long)gridDim.x * 2;

  // (loads are unconditional -- a frame index past the end re-reads the last frame -- so that the
  // compiler has nothing to turn into selects; what such a slot computes is dropped)
  auto load_x = [&](float (&dst)[16], long long f) {
    load_frame16<FMT, T, HIST>(p, rc, 0u, f < p.nframes ? f : (long long)p.nframes - 1, dst);
  };
  v2f32 pt[16];          // full round: the next taper pair; shared round: pt[0..7] = the last taper
  auto prefetch_taps = [&](int pair) {
    const unsigned tap_p = (unsigned)pair * (N * 8u);
    static_for<0, 8>([&](auto mc) {
      constexpr int mh = decltype(mc)::value;
      const v4f32 q = __builtin_bit_cast(v4f32, __builtin_amdgcn_raw_buffer_load_b128(trsrc, toff, tap_p + (unsigned)(T * mh) * 16u, 0));
      pt[2 * mh] = v2f32{q.x, q.y};
      pt[2 * mh + 1] = v2f32{q.z, q.w};
    });
  };
  auto prefetch_last = [&] {                         // [m/4][T][4] floats: samples t + T*(4*(m/4) + j)
    static_for<0, 4>([&](auto mc) {
      constexpr int mq = decltype(mc)::value;
      const v4f32 q = __builtin_bit_cast(v4f32, __builtin_amdgcn_raw_buffer_load_b128(vrsrc, toff, (unsigned)(T * mq) * 16u, 0));
      pt[2 * mq] = v2f32{q.x, q.y};
      pt[2 * mq + 1] = v2f32{q.z, q.w};
    });
  };

  // HALF: [lane][40] floats = pair 0 (m = 0..7 as (even, odd) taper), pair 1, the last taper
  v2f32 hp[16];
  float hl[8];
  const __amdgpu_buffer_rsrc_t yrsrc = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<float *>(p.ytaps), 0, HALF ? T * GLFER_YHALF_FLOATS * 4 : 0, 0x00020000);
  const unsigned yoff = t * (unsigned)(GLFER_YHALF_FLOATS * 4);
  auto load_half_last = [&] {
    static_for<0, 2>([&](auto cc) {
      constexpr int c = decltype(cc)::value;
      const v4f32 q = __builtin_bit_cast(v4f32, __builtin_amdgcn_raw_buffer_load_b128(yrsrc, yoff, 128u + c * 16u, 0));
      hl[4 * c] = q.x;
      hl[4 * c + 1] = q.y;
      hl[4 * c + 2] = q.z;
      hl[4 * c + 3] = q.w;
    });
  };
  if constexpr (HALF != 0) {
    static_for<0, 8>([&](auto cc) {
      constexpr int c = decltype(cc)::value;
      const v4f32 q = __builtin_bit_cast(v4f32, __builtin_amdgcn_raw_buffer_load_b128(yrsrc, yoff, c * 16u, 0));
      hp[2 * c] = v2f32{q.x, q.y};
      hp[2 * c + 1] = v2f32{q.z, q.w};
    });
    if constexpr (HALF == 1) load_half_last();
  }
  // the row_mirror partner's value (lane t ^ 15: residue 255 - rc); all lanes are active wherever this is used
  auto mirror = [](float v) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x140, 0xf, 0xf, true));
  };
  // taper pair P at register m: (v_2P, v_2P+1)[rc + T*m]; the upper half from the partner, the odd taper negated
  auto half_pair = [&](auto pc, auto mc) {
    constexpr int P = decltype(pc)::value, m = decltype(mc)::value;
    if constexpr (m < 8) return hp[P * 8 + m];
    else return v2f32{mirror(hp[P * 8 + 15 - m].x), -mirror(hp[P * 8 + 15 - m].y)};
  };

  // QUEUE: a chunk is `span` frames from a multiple of span; fEnd = the end of the chunk fA lies in, fresh = fA is its first pair
  const long long span = QUEUE ? 2LL * p.yq_chunk : 2;
  unsigned *qword = reinterpret_cast<unsigned *>(tw1 + 16);   // (column 16 of the table's padded rows is never read)
  long long fA = (long long)xcd_block_index() * span;
  if (fA >= p.nframes) return;
  long long fEnd = fA + span < p.nframes ? fA + span : (long long)p.nframes, next_chunk = 0;
  bool fresh = true;
  float xA[16], xB[16];
  load_x(xA, fA);
  if (fA + 1 < p.nframes) load_x(xB, fA + 1);
  else {
#pragma unroll
    for (int m = 0; m < 16; m++) xB[m] = 0.0f;
  }
  if constexpr (HALF == 0) prefetch_taps(0);

  // ---- KM: the hop sums of frames A (NH hops) and B (its newest hop), wavefront-reduced, into mred
  auto publish_hop_sums = [&] {
    static_for<0, NH + 1>([&](auto qc) {
      constexpr int q = decltype(qc)::value;
      float sm = 0.0f;
      static_for<0, KM>([&](auto mc) {
        constexpr int m = decltype(mc)::value;
        sm += q < NH ? xA[q * KM + m] : xB[(NH - 1) * KM + m];
      });
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) sm += __shfl_xor(sm, o);
      if ((t & 63u) == 0) mred[(t >> 6) * (NH + 1) + q] = sm;
    });
  };
  // (after a barrier) x - mu for both frames: frame B's hops are frame A's moved down by one
  auto subtract_hop_means = [&] {
    float mu[NH + 1];
#pragma unroll
    for (int q = 0; q <= NH; q++)
      mu[q] = ((mred[q] + mred[(NH + 1) + q]) + (mred[2 * (NH + 1) + q] + mred[3 * (NH + 1) + q])) / (float)p.H;   // fft.c:91
#pragma unroll
    for (int m = 0; m < 16; m++) {
      xA[m] = xA[m] - mu[m / (KM ? KM : 1)];
      xB[m] = xB[m] - mu[m / (KM ? KM : 1) + 1];
    }
  };
  // p.means (GLFER_SUBMEAN_EXACT): the hop means are given -- taken in the reference's own order by
  // hop_means_seq_kernel, means[global hop index]; the newest hop of frame F of the stream is hop F
  auto subtract_table_means = [&](long long fa) {      // fa: frame A's index in the launch
    float mu[NH + 1];
    const long long F = p.frame0 + fa;
#pragma unroll
    for (int q = 0; q < NH; q++) mu[q] = p.means[F - (NH - 1) + q];
    mu[NH] = p.means[fa + 1 < p.nframes ? F + 1 : F];  // frame B's newest hop (no frame B: its registers are zeroed afterwards)
#pragma unroll
    for (int m = 0; m < 16; m++) {
      xA[m] = xA[m] - mu[m / (KM ? KM : 1)];
      xB[m] = xB[m] - mu[m / (KM ? KM : 1) + 1];
    }
  };
  if constexpr (KM > 0) {
    if (p.means) {
      subtract_table_means(fA);
    } else {
      publish_hop_sums();
      __syncthreads();
      subtract_hop_means();
      __syncthreads();                               // mred is free again
    }
    if (fA + 1 >= p.nframes) {
#pragma unroll
      for (int m = 0; m < 16; m++) xB[m] = 0.0f;
    }
  }

  constexpr int RL = C::radix(NPASS - 1), BL = 16 / RL;
  auto rho_of = [](int m) constexpr { return (m % BL) + BL * brev(m / BL, RL); };   // register of bin t + T*m

  GLFER_BLOCK_MARK(1);
  while (true) {                                     // one iteration: frames A = fA and B = fA + 1
    long long nfA = fA + stride;
    bool has_next = nfA < p.nframes;
    unsigned ticket = 0;
    if constexpr (QUEUE != 0) {
      if (fresh && t == 0) ticket = __hip_atomic_fetch_add(p.yq_counter, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    float psdA[8], psdB[8], nyqA, nyqB;               // (SEG: the fold happens in the separation, these stay unused)
    int hxA, hxB;
    float accA[16], accB[16];                         // (SEG: live through the shared round)
    {
#pragma unroll
      for (int r = 0; r < 16; r++) accA[r] = accB[r] = 0.0f;     // (dead when NP >= 1: pair 0 overwrites)
      if constexpr (HALF != 0) {
        // ---- five tapers: the two full rounds written out, their tables in registers (same operations as the loop below)
        static_for<0, 2>([&](auto pc) {
          constexpr int P = decltype(pc)::value;
          float zrA[16], ziA[16], zrB[16], ziB[16];
          GLFER_STAMP(0);                            // dual round start
          static_for<0, 16>([&](auto mc) {
            constexpr int m = decltype(mc)::value;
            const v2f32 w = half_pair(pc, mc);
            zrA[m] = xA[m] * w.x;
            ziA[m] = xA[m] * w.y;
            zrB[m] = xB[m] * w.x;
            ziB[m] = xB[m] * w.y;
          });
          auto dual = [&](const auto &tw1sel) {
            auto hook = [] {};
            if constexpr (GLFER16Y_SKEW != 0) stockham16_passes2s<12, NT>(zrA, ziA, xbA, zrB, ziB, xbB, t, rc, tw1sel, twr, twi, hook);
            else stockham16_passes2<12, NT>(zrA, ziA, xbA, zrB, ziB, xbB, t, rc, tw1sel, twr, twi, hook);
          };
          if constexpr (TW1R) dual(tw1reg);
          else dual(tw1row);
#pragma unroll
          for (int r = 0; r < 16; r++) {
            if constexpr (P == 0) {                  // the first pair starts the sums (no zeroing pass)
              accA[r] = __builtin_fmaf(zrA[r], zrA[r], ziA[r] * ziA[r]);
              accB[r] = __builtin_fmaf(zrB[r], zrB[r], ziB[r] * ziB[r]);
            } else {
              accA[r] = __builtin_fmaf(zrA[r], zrA[r], __builtin_fmaf(ziA[r], ziA[r], accA[r]));
              accB[r] = __builtin_fmaf(zrB[r], zrB[r], __builtin_fmaf(ziB[r], ziB[r], accB[r]));
            }
          }
          GLFER_STAMP(15);                           // dual round end
        });
        if constexpr (HALF == 2) load_half_last();   // (the transform registers are dead here)
      } else
      for (int pair = 0; pair < NP; pair++) {
        // ---- one full round of both frames: re = x*taper(2*pair), im = x*taper(2*pair+1)
        float zrA[16], ziA[16], zrB[16], ziB[16];
        GLFER_STAMP(0);                              // dual round start
#pragma unroll
        for (int m = 0; m < 16; m++) {
          zrA[m] = xA[m] * pt[m].x;
          ziA[m] = xA[m] * pt[m].y;
          zrB[m] = xB[m] * pt[m].x;
          ziB[m] = xB[m] * pt[m].y;
        }
        auto dual = [&](const auto &tw1sel) {
          auto hook = [&] {
            if (pair + 1 < NP) prefetch_taps(pair + 1);
            else prefetch_last();
          };
          if constexpr (GLFER16Y_SKEW != 0) stockham16_passes2s<12, NT>(zrA, ziA, xbA, zrB, ziB, xbB, t, tw1sel, twr, twi, hook);
          else stockham16_passes2<12, NT>(zrA, ziA, xbA, zrB, ziB, xbB, t, tw1sel, twr, twi, hook);
        };
        if constexpr (TW1R) dual(tw1reg);
        else dual(tw1row);
        if (pair == 0) {                             // the first pair starts the sums (no zeroing pass)
#pragma unroll
          for (int r = 0; r < 16; r++) {
            accA[r] = __builtin_fmaf(zrA[r], zrA[r], ziA[r] * ziA[r]);
            accB[r] = __builtin_fmaf(zrB[r], zrB[r], ziB[r] * ziB[r]);
          }
        } else {
#pragma unroll
          for (int r = 0; r < 16; r++) {
            accA[r] = __builtin_fmaf(zrA[r], zrA[r], __builtin_fmaf(ziA[r], ziA[r], accA[r]));
            accB[r] = __builtin_fmaf(zrB[r], zrB[r], __builtin_fmaf(ziB[r], ziB[r], accB[r]));
          }
        }
        GLFER_STAMP(15);                             // dual round end
      }
      // ---- mirror fold psd[k] = acc[k] + acc[N-k] of both frames (upper half through LDS, entry
      // k - N/2) and the frames' powers for the shared round's scales
      float eA = 0.0f, eB = 0.0f;
#pragma unroll
      for (int r = 0; r < 16; r++) {
        eA += accA[r];
        eB += accB[r];
      }
#if GLFER16Y_DPP_SUM
      eA = wave_total_f32(eA);
      eB = wave_total_f32(eB);
#else
#pragma unroll
      for (int w = 1; w < 64; w <<= 1) {
        eA += __shfl_xor(eA, w);
        eB += __shfl_xor(eB, w);
      }
#endif
      GLFER_SEG_STAMP(0);                            // fold start (sums over the wavefront done)
      [[maybe_unused]] float *foldA = reinterpret_cast<float *>(xbA), *foldB = reinterpret_cast<float *>(xbB);
      if constexpr (!SEG) static_for<8, 16>([&](auto mc) {   // the buffers are free: barrier after the last reads
        constexpr int m = decltype(mc)::value;
        foldA[t + T * (m - 8)] = accA[rho_of(m)];
        foldB[t + T * (m - 8)] = accB[rho_of(m)];
      });
      // (SEG: the mirror fold rides in the separation's LDS pass, separate_fold_and_store; only the scales' power totals and
      // the queue ticket cross this barrier)
      if ((t & 63) == 0) {
        red[t >> 6] = eA;
        red[4 + (t >> 6)] = eB;
      }
      if constexpr (QUEUE != 0) {
        if (fresh && t == 0) *qword = ticket - p.yq_base;
      }
      GLFER_SEG_STAMP(1);                            // fold writes / power partials issued
      __syncthreads();
      GLFER_SEG_STAMP(2);                            // through the barrier behind them
      if constexpr (QUEUE != 0) {
        if (fresh) next_chunk = ((long long)gridDim.x + (long long)(unsigned)__builtin_amdgcn_readfirstlane((int)*qword)) * span;
        nfA = fA + 2 < fEnd ? fA + 2 : next_chunk;
        has_next = nfA < p.nframes;
      }
      eA = (red[0] + red[1]) + (red[2] + red[3]);
      eB = (red[4] + red[5]) + (red[6] + red[7]);
      hxA = scale_exponent(eA);
      hxB = scale_exponent(eB);
      if constexpr (!SEG) {
      static_for<0, 8>([&](auto mc) {
        constexpr int m = decltype(mc)::value;
        const int k = T * m + (int)t;
        float oa = foldA[N / 2 - k], ob = foldB[N / 2 - k];   // acc[N-k]; entry N/2 (k = 0) is never written
        if constexpr (m == 0) {
          if (t == 0) {
            oa = accA[rho_of(0)];
            ob = accB[rho_of(0)];
          }
        }
        psdA[m] = accA[rho_of(m)] + oa;
        psdB[m] = accB[rho_of(m)] + ob;
      });
      nyqA = 2.0f * accA[rho_of(8)];
      nyqB = 2.0f * accB[rho_of(8)];
      GLFER_SEG_STAMP(3);                            // fold reads issued
      __syncthreads();                               // fold buffers read: free for the next writes
      }
    }

    if constexpr (ABL == 1) {
      if (has_next) {
        if constexpr (HALF == 0) prefetch_taps(0);
        load_x(xA, nfA);
        load_x(xB, nfA + 1);
      }
      if (t == 0) p.psd[(size_t)fA * (size_t)p.pitch] = psdA[0] + psdB[0] + nyqA + nyqB + (float)(hxA + hxB);
      if (!has_next) break;
      fA = nfA;
      continue;
    }
    // ---- shared round: re = sA*(xA*v), im = sB*(xB*v), v the last taper
    float zr[16], zi[16];
    GLFER_STAMP(0);                                  // shared round start
    {
      const float sA = scale_in(hxA), sB = scale_in(hxB);
      if constexpr (HALF != 0) {
        static_for<0, 16>([&](auto mc) {             // (the last of five tapers has even order: no sign)
          constexpr int m = decltype(mc)::value;
          float v;
          if constexpr (m < 8) v = hl[m];
          else v = mirror(hl[15 - m]);
          zr[m] = (xA[m] * v) * sA;
          zi[m] = (xB[m] * v) * sB;
        });
      } else {
#pragma unroll
        for (int m = 0; m < 16; m++) {
          const float v = (m & 1) ? pt[m / 2].y : pt[m / 2].x;
          zr[m] = (xA[m] * v) * sA;
          zi[m] = (xB[m] * v) * sB;                  // no frame B: xB is all zeros (set below)
        }
      }
    }
    // the next iteration's samples and first taper pair go out after the first exchange's writes
    auto shared_round = [&](const auto &tw1sel) {
      auto hook = [&] {
        if (has_next) {
          if constexpr (HALF == 0) prefetch_taps(0);
          load_x(xA, nfA);
          load_x(xB, nfA + 1);
        }
      };
      if constexpr (SEG) {
        // exchange 0 through xbA, exchange 1 through xbB, the mirror entries of the separation through xbA again.  Both
        // buffers are free here: their last readers were the second dual round's exchange-1 reads, in front of that round's
        // buffer-release barrier (and the power totals' barrier above).
        stockham16_passes_pp<12, NT>(zr, zi, xbA, xbB, t, rc, tw1sel, twr, twi, hook, [&](auto qc, auto regc) {
          constexpr int q = decltype(qc)::value, reg = decltype(regc)::value;
          if constexpr (q >= 8) mirror_entry_write<12, q>(xbA, t, zr[reg], zi[reg], accA[reg], accB[reg]);
        });
      } else
      if constexpr (GLFER16Y_SKEW >= 2) stockham16_passes1s<12, NT>(zr, zi, xbA, t, rc, tw1sel, twr, twi, hook);
      else stockham16_passes<12, NT>(zr, zi, xbA, t, rc, tw1sel, twr, twi, hook);
    };
    if constexpr (TW1R) shared_round(tw1reg);
    else shared_round(tw1row);
    if constexpr (KM > 0) {
      if (has_next && !p.means) publish_hop_sums();  // the next iteration's samples are in registers (requested during the passes above)
    }
    // The barrier that ends either routine is the iteration's last.  SEG: it frees xbA (the mirror entries' readers) for the
    // next iteration's pass-0 writes; xbB's last readers were the shared round's exchange-1 reads, which every wavefront had in
    // registers before it arrived at the barrier behind the mirror entries -- two barriers in front of those writes.
    if constexpr (SEG) separate_fold_and_store<12>(p, zr, zi, accA, accB, xbA, t, fA, hxA, hxB);
    else
    separate_and_store<12, 1>(p, zr, zi, xbA, t, 0u, fA, hxA, hxB,
                              [&](auto mc) { if constexpr (decltype(mc)::value == 8) return nyqA; else return psdA[decltype(mc)::value]; },
                              [&](auto mc) { if constexpr (decltype(mc)::value == 8) return nyqB; else return psdB[decltype(mc)::value]; });
    GLFER_STAMP(15);                                 // shared round end (separated, stored)
    if constexpr (KM > 0) {
      if (has_next) {                                // (separate_and_store's barriers lie between the sums and this)
        if (p.means) subtract_table_means(nfA);
        else subtract_hop_means();
      }
    }
    if (!has_next) break;
    if constexpr (QUEUE != 0) {
      fresh = fA + 2 >= fEnd;
      if (fresh) fEnd = nfA + span < p.nframes ? nfA + span : (long long)p.nframes;
    }
    fA = nfA;
    if (fA + 1 >= p.nframes) {
#pragma unroll
      for (int m = 0; m < 16; m++) xB[m] = 0.0f;
    }
  }
  GLFER_BLOCK_MARK(2);
}

}  // namespace glfer

#ifndef GLFER_NO_LAUNCHERS
#include "launch16.hpp"
using namespace glfer;

// The queue form (p.yq_counter set by the host, which keeps the ticket base: glfer_hip.cpp): one workgroup per resident slot
#ifndef GLFER_RAGGED                                 /* (the queue form: one stream) */
template <int FMT>
static hipError_t launch16y_queue(const SpectroParams &p, hipStream_t st) {
  if (p.mean_inkernel || p.nbatch > 1 || p.yq_chunk < 1) return hipErrorInvalidValue;
  const unsigned grid = glfer_yq_grid(glfer_yq_chunks(p.nframes, p.yq_chunk));
  constexpr size_t shmem = (size_t)LaunchY::LDS_WORDS * 8;
  constexpr int HALF = GLFER16Y_HALF;
  if (HALF != 0 && p.ytaps && p.npairs == 3) {
    if (p.history_mode) return launch_dynamic_lds(spectro16y_kernel<FMT, 0, 1, 0, 0, HALF, 1>, dim3(grid), dim3(256), shmem, st, p);
    return launch_dynamic_lds(spectro16y_kernel<FMT, 0, 0, 0, 0, HALF, 1>, dim3(grid), dim3(256), shmem, st, p);
  }
  if (p.history_mode) return launch_dynamic_lds(spectro16y_kernel<FMT, 0, 1, 0, 0, 0, 1>, dim3(grid), dim3(256), shmem, st, p);
  return launch_dynamic_lds(spectro16y_kernel<FMT, 0, 0, 0, 0, 0, 1>, dim3(grid), dim3(256), shmem, st, p);
}
#endif

template <int FMT>
static hipError_t launch16y_fmt(const SpectroParams &p, hipStream_t st) {
  const long long work = ((long long)p.nframes + 1) / 2;
  if (work == 0) return hipSuccess;
#ifdef GLFER_RAGGED
  if (p.yq_counter || !p.ragged || p.nbatch < 2) return hipErrorInvalidValue;
#else
  if (p.yq_counter) return launch16y_queue<FMT>(p, st);
#endif
  const long long resident = 256LL * 2;
  const dim3 grid = batch_grid(persistent_grid(work, glfer_batch_cap(16 * resident, p.nbatch)), p);   // tools/xbench: 16x beats 4x by ~2 %
  constexpr size_t shmem = (size_t)LaunchY::LDS_WORDS * 8;
  {
    // (the plain kernel's limit is asked for whichever form is then chosen)
    hipError_t e = allow_dynamic_lds(reinterpret_cast<const void *>(p.history_mode ? spectro16y_kernel<FMT, 0, 1> : spectro16y_kernel<FMT, 0, 0>), shmem);
    if (e != hipSuccess) return e;
  }
  if (p.mean_inkernel) {
    if (p.history_mode) return hipErrorInvalidValue;
    const int km = p.H % 256 == 0 ? p.H / 256 : 0;
    return with_value<16, 8, 4>(km, [&](auto K) {
#ifndef GLFER_RAGGED                                 /* (the ragged build is always a launch over several streams: the BAT forms) */
      if (!(p.nbatch > 1)) return launch_dynamic_lds(spectro16y_kernel<FMT, 0, 0, K(), 0>, dim3(grid.x, 1), dim3(256), shmem, st, p);
#endif
      return launch_dynamic_lds(spectro16y_kernel<FMT, 0, 0, K(), 1>, grid, dim3(256), shmem, st, p);
    });
  }
  if (GLFER16Y_HALF != 0 && p.ytaps && p.npairs == 3) {   // five tapers, exactly (anti)symmetric tables: the half-table form
    if (p.history_mode) return launch_dynamic_lds(spectro16y_kernel<FMT, 0, 1, 0, 0, GLFER16Y_HALF>, grid, dim3(256), shmem, st, p);
    return launch_dynamic_lds(spectro16y_kernel<FMT, 0, 0, 0, 0, GLFER16Y_HALF>, grid, dim3(256), shmem, st, p);
  }
  if (p.history_mode) return launch(spectro16y_kernel<FMT, 0, 1>, grid, dim3(256), shmem, st, p);
  return launch(spectro16y_kernel<FMT, 0, 0>, grid, dim3(256), shmem, st, p);
}

// N = 4096, odd taper counts >= 3; needs p->xtaps (glfer_hip.cpp builds it)
extern "C" hipError_t glfer_launch_spectro16y_n12(const SpectroParams *p, hipStream_t st) {
  if (!p->xtaps || p->npairs < 2 || p->nonlin || p->spec) return hipErrorInvalidValue;
  if (p->frame0 * (long long)p->H < (long long)p->R) return hipErrorInvalidValue;   // no zero-history path here
  return with_fmt(p->fmt, [&](auto F) { return launch16y_fmt<F()>(*p, st); });
}
#endif  // GLFER_NO_LAUNCHERS
