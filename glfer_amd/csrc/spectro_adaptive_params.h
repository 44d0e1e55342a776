/* spectro_adaptive_params.h -- kernel argument block of spectro16a.hip (Thomson's adaptively weighted multitaper rows of one real
   channel and their degrees of freedom), shared by its launchers and the C-ABI layer (adaptive.cpp).  A block of its own:
   SpectroParams, IqParams and CrossParams stay as they are, so no other kernel's arguments move. */
#ifndef GLFER_SPECTRO_ADAPTIVE_PARAMS_H
#define GLFER_SPECTRO_ADAPTIVE_PARAMS_H

#include <hip/hip_runtime.h>
#include "spectro_params.h"

enum { GLFER_ADAPTIVE_KMAX = 8,        /* tapers whose eigenspectra a lane keeps in registers (spectro16a.hip)                 */
       GLFER_ADAPTIVE_ITERS_MAX = 64 };

struct AdaptiveParams {
  const void *stream;      /* device: sample 0 of the stream (virtual base), f32 / s16 / u8                                    */
  long long frame0;        /* index of this launch's first frame in the whole stream                                          */
  int nframes;             /* frames in this launch                                                                           */
  int H;                   /* hop, in samples                                                                                 */
  int R;                   /* N - H samples of history per frame                                                              */
  int ntap;                /* K tapers, 2 .. GLFER_ADAPTIVE_KMAX: ceil(K / 2) packed transforms a frame                        */
  int history_mode;        /* 0: zeros before sample 0 only; 1: history zeroed every frame                                    */
  int fmt;                 /* GLFER_FMT_*                                                                                     */
  int iters;               /* sweeps, 1 .. GLFER_ADAPTIVE_ITERS_MAX (the jackknife form: 0 as well, w_j = lambda_j)            */
  float inv_n;             /* 1 / N, a power of two                                                                           */
  const float *taps;       /* device: the plan's unit-energy tapers UNSCALED, one float per sample: [2 ceil(K/2)][4][N/16][4];
                              an odd K's last row is zeros (the lone taper's partner)                                         */
  const float2 *tw;        /* device: the plan's per-lane inter-pass twiddles (SpectroParams::tw)                             */
  float *psd, *dof;        /* device: [nframes][row_pitch], the first N/2 + 1 floats of a row are its bins; NULL: not wanted   */
  long long row_pitch;     /* floats from one row to the next, >= N/2 + 1                                                     */
  int nbatch;              /* streams in this launch (gridDim.y); 0 or 1: one                                                 */
  long long batch_stride;  /* bytes from one stream's sample 0 to the next one's                                              */
  long long row_batch_stride;   /* floats from one stream's first row to the next one's                                       */
  float lam[GLFER_ADAPTIVE_KMAX];    /* lambda_j = 1 - beta_j, rounded to float (glfer_hip_adaptive_weights)                   */
  float beta[GLFER_ADAPTIVE_KMAX];   /* beta_j = max(-sig_j, 0) formed in double, rounded to float                             */
  float *logvar;           /* device, the jackknife form alone (appended: no field above moves): the jackknife variance of
                              ln psd, rows as psd's; NULL: not wanted                                                         */
};

/* THE TABLE OF BUILT ADAPTIVE LAUNCHERS: X(logn), one entry per launcher glfer_launch_adaptive16_n<logn> (spectro16a.hip compiled
   with -DGLFER_LOGN=<logn>: the Makefile's ALOGNS list).  tests/test_adaptive_host.py holds the list, this table and the library's
   symbols against one another, as tests/test_launch_table_host.py does for spectro_params.h's table.
   N = 8192 is not in it: its instantiations spill (10 vector registers, profiles/adaptive_kernel_resources.txt). */
#define GLFER_LAUNCHERS16A(X) X(8) X(9) X(10) X(11) X(12)
/* THE TABLE OF BUILT JACKKNIFE LAUNCHERS: X(logn), one entry per launcher glfer_launch_jackknife16_n<logn> -- the JK
   instantiations of the same kernel, built in spectro16a.hip's translation units of the Makefile's JLOGNS list (-DGLFER_JACKKNIFE).
   tests/test_jackknife_host.py holds the list, this table and the library's symbols against one another.  A size whose JK
   instantiations do not fit two wavefronts per SIMD without a spill is left out of both (profiles/jackknife_kernel_resources.txt). */
#define GLFER_LAUNCHERS16J(X) X(8) X(9) X(10) X(11) X(12)

#ifdef __cplusplus
extern "C" {
#define GLFER_PROTO16A(l) hipError_t glfer_launch_adaptive16_n##l(const struct AdaptiveParams *p, hipStream_t st);
GLFER_LAUNCHERS16A(GLFER_PROTO16A)
#undef GLFER_PROTO16A
#define GLFER_PROTO16J(l) hipError_t glfer_launch_jackknife16_n##l(const struct AdaptiveParams *p, hipStream_t st);
GLFER_LAUNCHERS16J(GLFER_PROTO16J)
#undef GLFER_PROTO16J
}
/* the launcher built for a block size, or nullptr */
static inline hipError_t (*launcher16_adaptive(int logn))(const AdaptiveParams *, hipStream_t) {
#define GLFER_LOOKUP16A(l) if (logn == l) return glfer_launch_adaptive16_n##l;
  GLFER_LAUNCHERS16A(GLFER_LOOKUP16A)
#undef GLFER_LOOKUP16A
  return nullptr;
}
static inline hipError_t (*launcher16_jackknife(int logn))(const AdaptiveParams *, hipStream_t) {
#define GLFER_LOOKUP16J(l) if (logn == l) return glfer_launch_jackknife16_n##l;
  GLFER_LAUNCHERS16J(GLFER_LOOKUP16J)
#undef GLFER_LOOKUP16J
  return nullptr;
}
#endif
#endif
