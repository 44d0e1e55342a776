/* hparma_frames.h -- the frame list of the HP-ARMA kernel (hparma.hip): what a frame takes of a CU, how many frames a launch
 * keeps in flight, and the flat frame list of a launch over many streams.  hparma_kernel runs one wavefront per frame and
 * hands frames out from a queue; over a batch or ragged streams the launch's frames are ONE flat list g = 0 .. total - 1 in
 * stream order, every stream whole.  A stream with frames owns the consecutive flat frames [g0, g0 + nframes); a stream
 * without frames owns none and has no entry -- so g0 is strictly increasing and a wavefront finds its entry by bisection.
 * The queue's ticket is 32 bits: the list is cut into pieces of at most `piece_frames` frames, g0 counts from the piece's
 * first frame, and a stream is never split.
 * Host only, integers only, plain C99 and C++ (tests/c_hparma_frames.c walks it without a GPU). */
#ifndef GLFER_HPARMA_FRAMES_H
#define GLFER_HPARMA_FRAMES_H

#include <stddef.h>

#define GLFER_HPARMA_PIECE_FRAMES 0x7fffffffll   /* frames of one launch: the ticket is 32 bits */

/* LDS bytes of a frame: [x (N floats + a zero tail of 128 when t <= 128) overlaid later by A (t * ncol floats)] [Q ncol * ncol]
 * [r t] [S ncol] [a ncol] (hparma_kernel's layout; ncol = p_e + 1) */
static inline size_t glfer_hparma_lds_bytes(int n, int t, int ncol) {
  const int xlen = n + (t <= 128 ? 128 : 0);            /* the frame and its zero tail (the autocorrelation's two-lag walk) */
  const int big = xlen > t * ncol ? xlen : t * ncol;
  return (size_t)(big + ncol * ncol + t + 2 * ncol) * sizeof(float);
}

/* frames in flight: one wavefront each, as many per CU as its 160 KiB of LDS hold, on 256 CUs -- a launch's grid is the
 * smaller of this and its frames, and the rest come by ticket */
static inline long long glfer_hparma_resident(size_t lds_bytes) {
  return 256LL * (long long)(lds_bytes ? (160 * 1024) / lds_bytes : 8);
}

typedef struct {
  size_t stream;       /* its index in the call */
  long long g0;        /* its first flat frame, counted from its piece's first frame */
  long long nframes;   /* its frames */
  size_t piece;        /* the piece (launch) it belongs to */
} glfer_hparma_frames_entry;

/* The table of counts[0 .. nstreams) frames per stream (<= 0: none).  out: room for nstreams entries, or NULL to count only.
 * Returns the entries; *npieces (optional) receives the pieces.  A piece is closed when the next stream's frames would take
 * it past piece_frames (a stream has at most 2^31 - 1 frames, so at GLFER_HPARMA_PIECE_FRAMES every stream fits a piece). */
static inline size_t glfer_hparma_frame_table(const long long *counts, size_t nstreams, long long piece_frames,
                                              glfer_hparma_frames_entry *out, size_t *npieces) {
  size_t n = 0, pieces = 0;
  long long in_piece = 0;
  for (size_t b = 0; b < nstreams; b++) {
    const long long frames = counts[b];
    if (frames <= 0) continue;
    if (pieces == 0 || in_piece + frames > piece_frames) {
      pieces++;
      in_piece = 0;
    }
    if (out) {
      out[n].stream = b;
      out[n].g0 = in_piece;
      out[n].nframes = frames;
      out[n].piece = pieces - 1;
    }
    in_piece += frames;
    n++;
  }
  if (npieces) *npieces = pieces;
  return n;
}

#endif
