/* spectro_iq_params.h -- kernel argument block of spectro16c.hip (complex I/Q input), shared by its launchers and the C-ABI
   layer.  A block of its own: SpectroParams stays as it is, so no other kernel's arguments move. */
#ifndef GLFER_SPECTRO_IQ_PARAMS_H
#define GLFER_SPECTRO_IQ_PARAMS_H

#include <hip/hip_runtime.h>
#include "spectro_params.h"

/* include/glfer_hip.h's flag bits (the kernels do not include the public header) */
#ifndef GLFER_IQ_CENTERED
#define GLFER_IQ_CENTERED 1u
#define GLFER_IQ_SWAP     2u
#endif

struct IqParams {
  const void *stream;      /* device: complex sample 0 of the stream (virtual base), I and Q interleaved, f32 / s16 / u8 pairs */
  long long frame0;        /* index of this launch's first frame in the whole stream                      */
  int nframes;             /* frames in this launch                                                      */
  int H;                   /* hop, in complex samples                                                    */
  int R;                   /* N - H complex samples of history per frame                                 */
  int ntap;                /* tapers (1: the periodogram's window): one transform each                   */
  int history_mode;        /* 0: zeros before sample 0 only; 1: history zeroed every frame               */
  int fmt;                 /* GLFER_FMT_* of each part                                                   */
  unsigned flags;          /* GLFER_IQ_CENTERED | GLFER_IQ_SWAP                                          */
  const float *taps;       /* device: [ntap][4][N/16][4], w_j at samples t + (N/16) m, m = 4 q .. 4 q + 3, scale folded */
  const float2 *tw;        /* device: the plan's per-lane inter-pass twiddles (SpectroParams::tw)        */
  float *psd;              /* device: [nframes][pitch], the first N floats of a row are its bins         */
  long long pitch;         /* floats from one row to the next, >= N                                      */
  int nbatch;              /* streams in this launch (gridDim.y); 0 or 1: one                            */
  long long batch_stride;  /* bytes from one stream's sample 0 to the next one's                         */
  long long psd_batch_stride;   /* floats from one stream's first row to the next one's                  */
};

/* the launchers glfer_launch_spectro16c_n<logn>(const IqParams *, hipStream_t): declared by spectro_params.h's table of built
   launchers (its IQ entries); the one built for a block size, or nullptr */
#ifdef __cplusplus
#define GLFER_LOOKUP16_IQ(k, l, t) if (logn == l) return glfer_launch_##k##_n##l;
#define GLFER_LOOKUP16_S(k, l, t)
#define GLFER_LOOKUP16_CX(k, l, t)
static inline hipError_t (*launcher16_iq(int logn))(const IqParams *, hipStream_t) {
  GLFER_LAUNCHERS16(GLFER_LOOKUP16)
  return nullptr;
}
#undef GLFER_LOOKUP16_S
#undef GLFER_LOOKUP16_IQ
#undef GLFER_LOOKUP16_CX
#endif
#endif
