/* frame_cuts.h -- the frame and hop arithmetic every launcher of glfer_hip.cpp shares: how a range of frames is cut into
 * head / body / tail, and which hops a corrected copy or a table of hop means covers.  The batch and ragged entries promise
 * rows that are bit for bit the single-stream entry's; that holds because all of them cut with these functions.
 * Host only, integers only, plain C99 and C++ (tests/c_frame_cuts.c walks it without a GPU). */
#ifndef GLFER_FRAME_CUTS_H
#define GLFER_FRAME_CUTS_H

#include <stddef.h>

#include "../../include/glfer_hip.h"

/* bytes of one sample (GLFER_FMT_* of spectro_params.h are the GLFER_SAMPLES_* values) */
static inline size_t glfer_sample_size(int fmt) { return fmt == GLFER_SAMPLES_F32 ? 4 : (fmt == GLFER_SAMPLES_S16 ? 2 : 1); }

/* ceil(keep / hop): the first frame whose history lies inside the stream (the frames before it reach back before sample 0:
 * zero history, fft.c:103-108) -- and the whole hops a frame reaches back */
static inline size_t glfer_first_inside(size_t keep, size_t hop) { return (keep + hop - 1) / hop; }

/* The frame group of a route's kernel: the shared-odd-taper kernels work on groups of G consecutive frames (frame f shares its
 * last transform with frame f + G/2), every other route takes frames one by one. */
static inline size_t glfer_frame_group(int shared_odd, int n) {
  const size_t lanes = (size_t)n / 16;
  return shared_odd ? 2 * (lanes >= 256 ? 1 : 256 / lanes) : 1;
}

/* Frames [lo, hi) (lo <= hi) cut into head [lo, b0), body [b0, b1), tail [b1, hi).  The body is the union of the whole groups
 * [kG, (k+1)G) inside [max(lo, first_inside), hi): groups are aligned to GLOBAL frame indices, so a frame's result does not
 * depend on how the stream was cut into launches, chunks or shards as long as the cuts fall on multiples of GLFER_FRAME_ALIGN.
 * No such group: b0 = b1 = hi, everything is head. */
typedef struct { size_t b0, b1; } glfer_frame_cut;
static inline glfer_frame_cut glfer_cut_frames(size_t lo, size_t hi, size_t first_inside, size_t G) {
  glfer_frame_cut c;
  const size_t inside = lo > first_inside ? lo : first_inside;
  c.b0 = (inside + G - 1) / G * G;
  c.b1 = hi / G * G;
  if (c.b0 >= c.b1) c.b0 = c.b1 = hi;
  return c;
}

/* hops [lo, lo + n) of a stream (hop h = samples [h * hop, (h + 1) * hop): frame f ends with hop f) */
typedef struct { size_t lo, n; } glfer_hop_span;

/* the whole hops below its own that a frame reads: none with ZERO_ALWAYS history (no kernel loads what it would zero) */
static inline size_t glfer_hops_back(int history_mode, size_t first_inside) { return history_mode ? 0 : first_inside; }

/* The hops a corrected copy holds for frames [first, first + nframes): every frame's own hop and the hops_back before it, clipped
 * at the stream's start.  tail_fresh: the last hop is a trailing partial block laid over the previous hop's samples, which are
 * rebuilt from the CORRECTED previous hop -- so the copy reaches down to hop last - 1 at least. */
static inline glfer_hop_span glfer_copy_hops(size_t first, size_t nframes, size_t hops_back, int tail_fresh) {
  glfer_hop_span h;
  h.lo = first > hops_back ? first - hops_back : 0;
  if (tail_fresh && first + nframes > 1 && h.lo > first + nframes - 2) h.lo = first + nframes - 2;
  h.n = nframes ? first + nframes - h.lo : 0;
  return h;
}

/* The hops a body's table of hop means holds: those of frames [b0 - lead, b1) and their history, first_inside hops back (the
 * body lies inside the stream: b0 - lead >= first_inside).  lead: 0 for the rows entries, depth - 1 for the averages, whose
 * slots recompute that many frames in front of the body.  An empty body needs none. */
static inline glfer_hop_span glfer_means_hops(size_t b0, size_t b1, size_t lead, size_t first_inside) {
  glfer_hop_span h;
  h.lo = b1 > b0 ? b0 - lead - first_inside : 0;
  h.n = b1 > b0 ? b1 - h.lo : 0;
  return h;
}

#endif
