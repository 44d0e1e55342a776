/* spectro_cross_params.h -- kernel argument block of spectro16cx.hip (two real channels: multitaper auto- and cross-spectra and
   their coherence), shared by its launchers and the C-ABI layer.  A block of its own: SpectroParams and IqParams stay as they are,
   so no other kernel's arguments move. */
#ifndef GLFER_SPECTRO_CROSS_PARAMS_H
#define GLFER_SPECTRO_CROSS_PARAMS_H

#include <hip/hip_runtime.h>
#include "spectro_params.h"

struct CrossParams {
  const void *stream;      /* device: pair 0 of the stream (virtual base), x and y interleaved, f32 / s16 / u8 pairs        */
  long long frame0;        /* index of this launch's first frame in the whole stream                                       */
  int nframes;             /* frames in this launch                                                                        */
  int H;                   /* hop, in sample pairs                                                                         */
  int R;                   /* N - H pairs of history per frame                                                             */
  int ntap;                /* tapers: one packed transform each                                                            */
  int history_mode;        /* 0: zeros before pair 0 only; 1: history zeroed every frame                                   */
  int fmt;                 /* GLFER_FMT_* of each channel                                                                  */
  const float *taps;       /* device: the plan's I/Q table (IqParams::taps): v_j sqrt(1 / (N (1 + sig_j))), [ntap][4][N/16][4] */
  const float2 *tw;        /* device: the plan's per-lane inter-pass twiddles (SpectroParams::tw)                          */
  float *sxx, *syy, *coh;  /* device: [nframes][row_pitch], the first N/2 + 1 floats of a row are its bins; NULL: not wanted */
  float2 *sxy;             /* device: [nframes][sxy_pitch] (re, im), N/2 + 1 bins a row; NULL: not wanted                  */
  long long row_pitch;     /* floats from one row of sxx / syy / coh to the next, >= N/2 + 1                               */
  long long sxy_pitch;     /* float2 from one row of sxy to the next, >= N/2 + 1                                           */
  int nbatch;              /* streams in this launch (gridDim.y); 0 or 1: one                                              */
  long long batch_stride;  /* bytes from one stream's pair 0 to the next one's                                             */
  long long row_batch_stride;   /* floats from one stream's first row of sxx / syy / coh to the next one's                 */
  long long sxy_batch_stride;   /* float2 from one stream's first row of sxy to the next one's                             */
  /* segment averaging (glfer_hip_welch_cross_device), appended: the offsets above do not move.  segments == 0: the one-frame-a-row
     form, the three are not read.  Else nframes counts ROWS and row r sums the frames frame0 + r * step + s, s < segments         */
  int segments;            /* L: frames summed into a row                                                                  */
  float scale;             /* what the sums are stored times: 0.25 / L rounded once (0.25: the two halves of the separation) */
  long long step;          /* frames from one row's first frame to the next row's, >= 1                                    */
};

/* the launchers glfer_launch_spectro16cx_n<logn>(const CrossParams *, hipStream_t): declared by spectro_params.h's table of built
   launchers (its CX entries); the one built for a block size, or nullptr */
#ifdef __cplusplus
#define GLFER_LOOKUP16_CX(k, l, t) if (logn == l) return glfer_launch_##k##_n##l;
#define GLFER_LOOKUP16_S(k, l, t)
#define GLFER_LOOKUP16_IQ(k, l, t)
static inline hipError_t (*launcher16_cx(int logn))(const CrossParams *, hipStream_t) {
  GLFER_LAUNCHERS16(GLFER_LOOKUP16)
  return nullptr;
}
#undef GLFER_LOOKUP16_S
#undef GLFER_LOOKUP16_IQ
#undef GLFER_LOOKUP16_CX
#endif
#endif
