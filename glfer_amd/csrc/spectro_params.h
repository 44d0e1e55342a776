/* spectro_params.h -- kernel argument block shared by the launchers and the C-ABI layer. */
#ifndef GLFER_SPECTRO_PARAMS_H
#define GLFER_SPECTRO_PARAMS_H

#include <hip/hip_runtime.h>

enum { GLFER_FMT_F32 = 0, GLFER_FMT_S16 = 1, GLFER_FMT_U8 = 2 };

/* One stream of a ragged launch (glfer_hip_spectrogram_ragged_device): SpectroParams::ragged[blockIdx.y].  The offsets are
   relative to the launch's own stream / psd / means (virtual bases, so they may be negative); frame0 and nframes are the
   stream's own piece of this launch (its head, its body or its tail frames).  nframes <= 0: nothing for this stream here.
   ftest_off (glfer_hip_mtm_ftest_ragged_device / _rows_ftest_ragged_device): the stream's first F row of this launch,
   (R_b + frame0) * (N/2+1) floats from the launch's ftest -- F rows are dense whatever the PSD pitch, so it is not psd_off.
   Only spectro16_kernel's FT forms read it (appended: the rows kernels load the fields they always did).  F alone leaves
   psd NULL and psd_off 0, so that the select's psd + psd_off stays NULL. */
struct GlferRaggedEntry {
  long long stream_off;    /* bytes                                                          */
  long long psd_off;       /* floats                                                         */
  long long means_off;     /* floats (with given hop means)                                  */
  long long frame0;
  int nframes;
  int reserved;
  long long ftest_off;     /* floats (the F forms)                                            */
};
/* One stream of a ragged hop-means / corrected-copy launch (submean_seq.hip, spectro16.hip's submean kernels, RAG forms) */
struct GlferRaggedHops {
  const void *in;          /* the stream's first hop of the launch                           */
  float *out;              /* its corrected copy (the copy kernels)                          */
  float *means;            /* its hop means: written by the means kernel, read by the copy kernels (NULL there: summed by the kernel) */
  long long nhops;
};

struct SpectroParams {
  const void *stream;      /* device: sample stream (f32 / s16 / u8)                        */
  long long frame0;        /* index of this launch's first frame in the whole stream        */
  int nframes;             /* frames in this launch                                          */
  int H;                   /* hop = (int)(N*(1.0-overlap))            fft.c:70               */
  int R;                   /* N - H samples of history per frame      fft.c:71               */
  int npairs;              /* ceil(T/2) complex transforms per frame                         */
  int history_mode;        /* 0: zeros before sample 0 only; 1: history zeroed every frame   */
  int fmt;                 /* GLFER_FMT_*                                                    */
  int nonlin;              /* RA9MB / limiter path (periodogram only)                        */
  int limiter;             /* fft.c:151-156                                                  */
  float a;                 /* fft.c:127-136                                                  */
  float post_scale;        /* nonlin path: sqrt(1/(2N)) applied after the limiter            */
  float spec_unscale;      /* factor folded into taper 0 (undone for the spectrum output)    */
  const float *taps;       /* device: [npairs][N][2] taper pairs interleaved, weights and 1/(2N) folded */
  const float2 *tw;        /* device: [slots][N/16] per-lane inter-pass twiddles (cos,sin)    */
  /* real-input (N/2-point) form of a single taper, spectro16h.hip; NULL when not built for this plan */
  const float *htaps;      /* device: [8][N/32][4] window as (w[2n],w[2n+1]) pairs, sqrt(1/(4N)) folded */
  const float2 *htw;       /* device: [slots][N/32] inter-pass twiddles of the N/2-point transform      */
  int htapers;             /* windows in htaps: 0/1 = periodogram; > 1 = multitaper via the real-input form, [htapers] tables */
  const float2 *hrot;      /* device: [N/32] (cos,sin)(2 pi t/N), the lane part of the post twiddle     */
  /* real-input form with wavefront-private 1024-point transforms, spectro16w.hip (N >= 2048); NULL when not built */
  const float *wtaps;      /* device: [wtapers][W][8][64][4] window/taper pairs in lane order, sqrt(1/(4N(1+sig))) folded */
  int wtapers;             /* tables in wtaps: 1 = periodogram window; > 1 = the tapers of mtm_do       */
  const float2 *wtw;       /* device: [27][64] inter-pass twiddles of the 1024-point transform          */
  const float2 *wcomb;     /* device: [IPL*W][64 W] (cos,sin): [i][0] = 2 pi k1/N, [i][w] = 2 pi w k1/M, k1 = u + 64 W i */
  const float2 *bigtw;     /* device: [W][16] (cos,sin)(-2 pi 64 w m / M), spectro_big.hip (N >= 32768); NULL when not built */
  /* odd taper counts, spectro16x.hip: the last taper alone; NULL when not built for this plan */
  const float *xtaps;      /* device: [4][N/16][4] last taper, sqrt(1/(4N(1+sig))) folded               */
  /* odd taper counts with LDS-resident half tables, spectro16xl.hip; NULL when not built */
  const float *ltaps;      /* device: [npairs-1][8][N/16][2] pair halves, then [8][N/16] the last taper */
  /* five tapers at N = 4096, spectro16y.hip's half-table form: the tables a lane keeps in registers; NULL when not built */
  const float *ytaps;      /* device: [256][GLFER_YHALF_FLOATS], see glfer_yhalf_residue()                */
  /* spectro16y.hip's queue form (the plain forms, one stream): frame pairs handed out in chunks from a counter the plan owns.
     yq_counter NULL: the static stride.  The counter is never reset: a launch of P chunks draws exactly P tickets, the host
     (glfer_hip.cpp) keeps the value it has before the launch and the kernel subtracts it.  32 bits, modulo 2^32 on both sides:
     only the difference is used, and a launch has fewer than 2^31 chunks. */
  unsigned *yq_counter;    /* device                                                         */
  unsigned yq_base;        /* the counter's value when this launch starts                    */
  int yq_chunk;            /* consecutive frame pairs per ticket                             */
  struct glfer_yqueue *yq; /* HOST: the plan's counters (glfer_hip.cpp); kernels do not touch it */
  float *psd;              /* device: [nframes][pitch], the first N/2+1 floats of a row are its bins */
  int pitch;               /* floats from one PSD row to the next (cfg.psd_pitch; N/2+1 = dense)      */
  float *spec;             /* device, optional: [nframes][N] halfcomplex spectrum            */
  /* harmonic F statistic (mtm.c:165-174, 203-233) inside spectro16_kernel; ftest NULL = off.  taps then holds
     [rounds][2N] tables with ONE taper each (im part zero): hn first when ft_mu_live, then tapers 0..ntap-1 */
  float *ftest;            /* device: [nframes][N/2+1]                                        */
  const double *ft_U0;     /* device: [ntap]                                                  */
  float ft_sum_U0_sqr;
  int ft_mu_live;          /* 0: mu is all zeros (the reference build without FFTW, mtm.c:173) */
  int ft_nseq;             /* > 0: the PAIRED form (round 5): taps holds [ceil(ft_nseq / 2)][2N] tables with TWO real sequences each
                              (re: sequence 2r, im: sequence 2r+1, both scaled by 1/2; the sequences are hn -- when ft_mu_live --
                              then tapers 0..ntap-1), one N-point transform per pair, the two spectra separated through the
                              mirror bins (X_a = Z[k] + conj Z[N-k], X_b = (Z[k] - conj Z[N-k]) / i)                 */
  float ft_mu_unscale;     /* the paired form: hn rides in its table times a power of two that brings it to a taper's size (hn is
                              ~ 1/sqrt(sum U0^2) of one, and a sequence comes out of the separation with an error of an ulp of the
                              LARGER of the pair); mu = its spectrum times this, the inverse power: exact                */
  int mean_inkernel;       /* per-hop mean removal (fft.c:86-96) inside spectro16h.hip: the stream is the RAW one;
                              only where the hop is 2, 4, 8 or 16 sixteenths of N               */
  const float *means;      /* device, optional (with mean_inkernel): means[h] = the mean of hop h of the whole stream (virtual
                              base), taken in the reference's own order (submean_seq.hip, GLFER_SUBMEAN_EXACT); the kernel
                              subtracts these instead of summing the hops itself                */
  /* spectro16h.hip's table form with the means PRODUCED INSIDE THE SAME LAUNCH (round 4): the first nprod workgroups take the
     hop means in the reference's own order (the 64-hops-side-by-side chains of submean_seq.hip) while the others transform;
     a consumer workgroup waits for the chunks its frames' hops lie in.  nprod = 0: the means table was filled by an earlier launch. */
  int nprod;               /* producer workgroups at the head of the grid                                            */
  int prod_chunk;          /* hops per chunk of means_ready (a multiple of 64)                                       */
  float *means_out;        /* = means, writable                                                                       */
  unsigned *means_ready;   /* device: [ceil(prod_nhops / prod_chunk)] hop groups of the chunk that are written (zeroed before the launch) */
  long long prod_hop0;     /* the hops to produce: [prod_hop0, prod_hop0 + prod_nhops) of the whole stream             */
  long long prod_nhops;
  /* round 5, the LOCK-STEPPED fused launch (prod_front_frames > 0): the consumer workgroups walk the stream in eight fronts (one per
     XCD: consumer workgroup w belongs to front w mod 8 and takes the front's next range of frames), producer workgroup j serves front
     j mod 8 and stays at most prod_look hops ahead of what that front's consumers have finished, so that the estimator's read of a
     hop comes out of the Infinity Cache the producers filled a few tens of microseconds earlier.  means_ready then holds one flag
     per 64-hop group (prod_chunk = 64), followed by front_done[8] (consumer workgroups finished per front).                     */
  long long prod_front_frames;   /* frames per front: (consumer workgroups / 8) x frames per workgroup                                */
  int prod_block_frames;         /* frames per consumer workgroup                                                                    */
  int prod_look;                 /* hops a front's producers may run ahead of its finished consumers                                  */
  unsigned *front_done;          /* device: [8]                                                                                     */
  /* update_avg_plain (avg.c:108-159) INSIDE spectro16h.hip's periodogram kernel (round 5): avg != NULL.  A frame slot walks
     consecutive frames and keeps the last depth-1 PSD rows of its bins in registers; the window's sum is taken in double per
     bin and divided by depth+1 as the reference does once its window is full (avg.c:138-139,155).  EVERY frame of the launch
     has its full window: the launcher hands over frames whose depth-1 predecessors are computable (>= the first frame
     that lies inside the stream) and belong to the same averaging state; a slot recomputes them in front of its range. */
  double *avg;             /* device: [nframes][avg_nout] doubles, row i = frame frame0 + i; columns outside the band 1e-15 */
  double *avg_ret;         /* device, optional: [nframes][4] = {band mean (avg.c:147), peak bin or -1, 0, effdepth}        */
  int avg_depth;           /* 1..4                                                                                           */
  int avg_minbin, avg_maxbin, avg_nout;
  /* the stream dimension (glfer_hip_spectrogram_batch_device): blockIdx.y is the stream of the batch; a kernel moves stream and
     psd on by blockIdx.y times these strides at entry (glfer_batch_select) and walks its frames inside that stream as before.
     nbatch <= 1 with zero strides: one stream, the grid and the rows of the single-stream entry.                            */
  int nbatch;              /* streams in this launch (gridDim.y); 0 or 1: one                                              */
  long long batch_stride;  /* bytes from one stream's sample 0 (virtual base) to the next one's                             */
  long long psd_batch_stride;   /* floats from one stream's first row to the next one's                                     */
  long long means_batch_stride; /* floats from one stream's given hop-means table (means) to the next one's                  */
  long long avg_batch_stride;   /* doubles from one stream's first averaged row (avg) to the next one's                        */
  long long avg_ret_batch_stride;   /* doubles from one stream's first return values (avg_ret) to the next one's               */
  long long ftest_batch_stride; /* floats from one stream's first F row (ftest) to the next one's (glfer_hip_mtm_ftest_batch_device:
                                   psd NULL and psd_batch_stride 0 there); spectro16_kernel's FT forms add it at entry (their ragged
                                   instantiations take GlferRaggedEntry::ftest_off instead)                                    */
  /* the multitaper rows beside F (glfer_hip_mtm_rows_ftest_device): psd != NULL with ftest, pitch and psd_batch_stride as for the rows */
  const float *ft_cj;      /* device: [ntap], 1 / (N (1 + sig_j)): the weight of taper j's |y_j|^2 in the row (mtm.c:212-219, fft.c:212-216).
                              The F tables hold the tapers unscaled, so the rows' weights ride here; read by the ROWS forms only.
                              (Appended: every earlier member keeps its offset.)                                                     */
  /* ragged batches (glfer_hip_spectrogram_ragged_device): streams of unequal length in one launch.  ragged != NULL: blockIdx.y
     indexes this device table, one entry per stream of the launch (nbatch of them), and the entry -- not the batch strides --
     gives the stream's samples, rows, hop means, frame0 and nframes; the launch's own frame0 / nframes are those of its longest
     stream (the launchers size the grid and check the range with them).  The kernels' ragged instantiations only.             */
  const struct GlferRaggedEntry *ragged;
};

/* spectro16y.hip's half-table form (N = 4096, T = 256 lanes, five tapers).  In pass 0 lane t = 16 j + p holds the samples
   r + 256 m of residue r = glfer_yhalf_residue(t), so that residues r and 255 - r sit at mirrored positions of one 16-lane
   row: glfer_yhalf_residue(t ^ 15) = 255 - glfer_yhalf_residue(t).  Sample (r, m) mirrors to (255 - r, 15 - m) about the
   frame centre, so a lane keeps m = 0..7 only and takes m >= 8 from lane t ^ 15 at 15 - m, with the taper's parity as sign.
   ytaps[t][e]: e = 16 P + 2 m + k for taper 2 P + k of pair P = 0, 1 at m = 0..7
   (scale sqrt(1/(2N(1+sig)))), e = 32 + m for the last taper (scale sqrt(1/(4N(1+sig)))). */
enum { GLFER_YHALF_FLOATS = 40 };
static inline __host__ __device__ unsigned glfer_yhalf_residue(unsigned t) {
  const unsigned j = t >> 4, p = t & 15u;
  return p < 8u ? 8u * j + p : 240u - 8u * j + p;
}

/* spectro16y.hip's queue form: chunks of a launch (= the tickets it draws) and its grid -- one workgroup per resident slot
   (256 CUs x 2), fewer when there are fewer chunks, whole XCD slices from 64 up (xcd_block_index) */
enum { GLFER_YQ_BLOCKS = 512, GLFER_YQ_CHUNK = 4 };   /* 4: profiles/y_frame_queue.txt, the chunk sweep */
static inline long long glfer_yq_chunks(int nframes, int chunk) {
  return (((long long)nframes + 1) / 2 + chunk - 1) / chunk;
}
static inline unsigned glfer_yq_grid(long long nchunks) {
  unsigned grid = (unsigned)(nchunks < GLFER_YQ_BLOCKS ? nchunks : GLFER_YQ_BLOCKS);
  if (grid >= 64) grid &= ~7u;
  return grid;
}

/* A launcher's persistent grid for a batch: `cap` workgroups for the whole launch, shared among its streams, so that
   gridDim.x x nbatch stays near the single-stream cap.  The caller keeps gridDim.x a multiple of 8 once it is >= 64
   (xcd_block_index: with gridDim.x a multiple of 8 the linear workgroup id of (x, y) is x modulo 8 as well). */
static inline long long glfer_batch_cap(long long cap, int nbatch) {
  return nbatch > 1 ? (cap + nbatch - 1) / nbatch : cap;
}
static inline unsigned glfer_batch_y(const SpectroParams &p) { return p.nbatch > 1 ? (unsigned)p.nbatch : 1u; }

#ifdef __HIPCC__
/* kernel entry: this workgroup's stream of the batch */
__device__ __forceinline__ void glfer_batch_select(SpectroParams &p) {
  const long long b = (long long)blockIdx.y;
  p.stream = reinterpret_cast<const char *>(p.stream) + b * p.batch_stride;
  p.psd = p.psd + b * p.psd_batch_stride;
  if (p.means) p.means = p.means + b * p.means_batch_stride;
}
/* kernel entry of the ragged instantiations: this workgroup's stream of the launch and its own frames; false: the stream has
   no frames in this launch and the workgroup leaves (uniformly, before its first barrier) */
__device__ __forceinline__ bool glfer_ragged_select(SpectroParams &p) {
  const GlferRaggedEntry e = p.ragged[blockIdx.y];
  if (e.nframes <= 0) return false;
  p.stream = reinterpret_cast<const char *>(p.stream) + e.stream_off;
  p.psd = p.psd + e.psd_off;
  if (p.means) p.means = p.means + e.means_off;
  p.frame0 = e.frame0;
  p.nframes = e.nframes;
  return true;
}
/* what a kernel does at entry: the stream of the batch, or -- the ragged instantiations -- the stream's table entry */
#ifdef GLFER_RAGGED
#define GLFER_STREAM_SELECT(p) do { if (!glfer_ragged_select(p)) return; } while (0)
#else
#define GLFER_STREAM_SELECT(p) glfer_batch_select(p)
#endif
/* the same for the average taken inside the launch (glfer_hip_spectrogram_avg_batch_device; psd_batch_stride 0 when no PSD rows are
   asked for, so that psd stays NULL) */
__device__ __forceinline__ void glfer_batch_select_avg(SpectroParams &p) {
  glfer_batch_select(p);
  const long long b = (long long)blockIdx.y;
  p.avg = p.avg + b * p.avg_batch_stride;
  p.avg_ret = p.avg_ret + b * p.avg_ret_batch_stride;
}
#endif

/* THE TABLE OF BUILT ESTIMATOR LAUNCHERS: X(kind, block, logn, twin), one entry per launcher glfer_launch_<kind>_n<logn> --
     kind     the source spectro16*.hip and the stem of the launcher's name
     block    the argument block it takes: S = SpectroParams, IQ = IqParams (spectro_iq_params.h), CX = CrossParams
              (spectro_cross_params.h)
     logn     log2 of the block size the source is compiled for (the Makefile's LOGNS lists)
     twin     1: built once more with -DGLFER_RAGGED as glfer_launch_<kind>_ragged_n<logn> (the stream from SpectroParams::ragged;
              the Makefile's RAGGED_OBJS); 0: no ragged twin
   The prototypes and the lookups launcher16() (below), launcher16_iq() and launcher16_cx() (beside their argument blocks) are
   generated from it; tests/test_launch_table_host.py holds the Makefile's lists and the library's symbols against it. */
#define GLFER_LAUNCHERS16(X)                                                                                                                  \
  X(spectro16, S, 8, 1) X(spectro16, S, 9, 1) X(spectro16, S, 10, 1) X(spectro16, S, 11, 1) X(spectro16, S, 12, 1) X(spectro16, S, 13, 1) X(spectro16, S, 14, 1) \
  X(spectro16h, S, 9, 1) X(spectro16h, S, 10, 1) X(spectro16h, S, 11, 1) X(spectro16h, S, 12, 1) X(spectro16h, S, 13, 1) X(spectro16h, S, 14, 1) \
  X(spectro16w, S, 11, 1) X(spectro16w, S, 12, 1) X(spectro16w, S, 13, 1) X(spectro16w, S, 14, 1) X(spectro16w, S, 15, 0)                       \
  X(spectro16x, S, 8, 1) X(spectro16x, S, 9, 1) X(spectro16x, S, 10, 1)                                                                       \
  X(spectro16xl, S, 8, 1) X(spectro16xl, S, 9, 1) X(spectro16xl, S, 10, 1) X(spectro16xl, S, 11, 1)                                           \
  X(spectro16y, S, 12, 1)                                                                                                                     \
  X(spectro16c, IQ, 8, 0) X(spectro16c, IQ, 9, 0) X(spectro16c, IQ, 10, 0) X(spectro16c, IQ, 11, 0) X(spectro16c, IQ, 12, 0) X(spectro16c, IQ, 13, 0) X(spectro16c, IQ, 14, 0) \
  X(spectro16cx, CX, 8, 0) X(spectro16cx, CX, 9, 0) X(spectro16cx, CX, 10, 0) X(spectro16cx, CX, 11, 0) X(spectro16cx, CX, 12, 0) X(spectro16cx, CX, 13, 0)
enum glfer_kind16 { GLFER_KIND_spectro16, GLFER_KIND_spectro16h, GLFER_KIND_spectro16w, GLFER_KIND_spectro16x, GLFER_KIND_spectro16xl,
                    GLFER_KIND_spectro16y };
#define GLFER_BLOCK16_S SpectroParams
#define GLFER_BLOCK16_IQ IqParams
#define GLFER_BLOCK16_CX CrossParams
#define GLFER_TWIN16_0(...)
#define GLFER_TWIN16_1(...) __VA_ARGS__

#ifdef __cplusplus
extern "C" {
#endif
struct IqParams;
struct CrossParams;
#define GLFER_PROTO16(k, b, l, t)                                                        \
  hipError_t glfer_launch_##k##_n##l(const struct GLFER_BLOCK16_##b *p, hipStream_t st); \
  GLFER_TWIN16_##t(hipError_t glfer_launch_##k##_ragged_n##l(const struct GLFER_BLOCK16_##b *p, hipStream_t st);)
GLFER_LAUNCHERS16(GLFER_PROTO16)
#undef GLFER_PROTO16
size_t glfer_levels_scratch_floats(size_t nframes);
hipError_t glfer_launch_levels(const float *stats, size_t nframes, int scale_log, int autoscale,
                               int first_buffer, float overlap, float max_lvl0, float min_lvl0,
                               float *levels, float *chunk_state, hipStream_t st);
hipError_t glfer_launch_levels_fixed(size_t nframes, float dmax, float dmin, float max_lvl, float min_lvl,
                                     float *levels, hipStream_t st);
hipError_t glfer_launch_map(const float *psd, const double *avg, size_t nframes, int n, int psd_pitch, int scale_log,
                            double thr255, double one_m_thr, const float *levels,
                            const unsigned char *colortab, const double *log_thr, unsigned char *rgb, short *lev,
                            hipStream_t st);
hipError_t glfer_launch_submean(const void *in, float *out, int H, long long nhops, int fmt,
                                hipStream_t st, const float *means /* NULL: summed by the kernel */);
/* the same over nb streams (blockIdx.y): stream b reads in + b * in_bstride bytes, writes out + b * out_bstride floats and
   takes means + b * means_bstride; nb <= 65535 */
hipError_t glfer_launch_submean_batch(const void *in, float *out, int H, long long nhops, int fmt, hipStream_t st, const float *means,
                                      unsigned nb, long long in_bstride, long long out_bstride, long long means_bstride);
hipError_t glfer_launch_hop_means_seq_batch(const void *in, float *means, int H, long long nhops, int fmt, unsigned nb,
                                            long long in_bstride, long long means_bstride, hipStream_t st);
/* the two over nb streams of unequal length: tab[b] (device) holds stream b's pointers and its own hop count, max_nhops (the
   longest) sizes the grid; with_means: the copy subtracts tab[b].means instead of summing the hops itself */
hipError_t glfer_launch_hop_means_seq_ragged(const GlferRaggedHops *tab, unsigned nb, int H, long long max_nhops, int fmt, hipStream_t st);
hipError_t glfer_launch_submean_ragged(const GlferRaggedHops *tab, unsigned nb, int H, long long max_nhops, int fmt, int with_means,
                                       hipStream_t st);
#ifdef __cplusplus
}
/* The lookups.  GLFER_LOOKUP16 hands an entry to GLFER_LOOKUP16_<block>; the header of an argument block defines its own as
   `if (<kind and logn match>) return <launcher, or its ragged twin>;` and the other two as nothing (this one: S; the IQ and CX
   entries in spectro_iq_params.h and spectro_cross_params.h).  Nothing built: nullptr, which the routing functions
   (glfer_hip.cpp, cross.cpp) turn into hipErrorInvalidValue. */
#define GLFER_PICK16_0(k, l) nullptr
#define GLFER_PICK16_1(k, l) glfer_launch_##k##_ragged_n##l
#define GLFER_LOOKUP16_S(k, l, t) if (kind == GLFER_KIND_##k && logn == l) return ragged ? GLFER_PICK16_##t(k, l) : glfer_launch_##k##_n##l;
#define GLFER_LOOKUP16_IQ(k, l, t)
#define GLFER_LOOKUP16_CX(k, l, t)
#define GLFER_LOOKUP16(k, b, l, t) GLFER_LOOKUP16_##b(k, l, t)
typedef hipError_t (*glfer_launcher16_fn)(const SpectroParams *, hipStream_t);
static inline glfer_launcher16_fn launcher16(glfer_kind16 kind, int logn, bool ragged) {
  GLFER_LAUNCHERS16(GLFER_LOOKUP16)
  return nullptr;
}
#undef GLFER_LOOKUP16_S
#undef GLFER_LOOKUP16_IQ
#undef GLFER_LOOKUP16_CX
/* log2 of a block size, -1 when it is no power of two (the lookups then find nothing) */
static inline int glfer_logn(int n) { return n > 0 && (n & (n - 1)) == 0 ? __builtin_ctz((unsigned)n) : -1; }
#endif
#endif
