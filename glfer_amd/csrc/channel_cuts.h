/* channel_cuts.h -- the hop and piece arithmetic of the channel entries (glfer_hip.h, "Multi-channel recordings"): which hops of
 * an interleaved recording a range of frames reads, how far apart the de-interleaved planes lie, and how a call whose planes
 * would not fit a byte budget is cut into pieces of frames.  The channel entries promise the rows of the single-stream entry on
 * a contiguous copy of a channel; that holds because every piece is cut by rule (1) of "Cutting a stream" (boundaries on global
 * multiples of GLFER_FRAME_ALIGN) and carries the halo of rule (2).
 * Host only, integers only, plain C99 and C++ (tests/c_channel_cuts.c walks it without a GPU). */
#ifndef GLFER_CHANNEL_CUTS_H
#define GLFER_CHANNEL_CUTS_H

#include <stddef.h>

#include "frame_cuts.h"

#define GLFER_MAX_CHANNELS 64

/* The selection of a channel entry as the bytes the kernel takes: select == NULL is every channel in order (nselect ignored).
 * Returns the number selected, 0 for a channel count or a selection outside 1 .. 64 or an index that is no channel. */
static inline int glfer_channel_selection(int channels, const int *select, int nselect, unsigned char sel[GLFER_MAX_CHANNELS]) {
  int j;
  if (channels < 1 || channels > GLFER_MAX_CHANNELS) return 0;
  if (!select) {
    for (j = 0; j < channels; j++) sel[j] = (unsigned char)j;
    return channels;
  }
  if (nselect < 1 || nselect > GLFER_MAX_CHANNELS) return 0;
  for (j = 0; j < nselect; j++) {
    if (select[j] < 0 || select[j] >= channels) return 0;
    sel[j] = (unsigned char)select[j];
  }
  return nselect;
}

/* the whole hops in front of its own that a piece's first frame needs: ceil((N - H) / H) of history, and the lmp_av - 1 frames an
 * LMP plan's ring reaches back (recomputed, not carried); lmp_av <= 1 for the other modes */
static inline size_t glfer_channel_halo(size_t keep, size_t hop, size_t lmp_av) {
  return glfer_first_inside(keep, hop) + (lmp_av > 1 ? lmp_av - 1 : 0);
}

/* the hops frames [first, first + nframes) read: their own and the halo, none below hop 0 */
static inline glfer_hop_span glfer_channel_hops(size_t first, size_t nframes, size_t halo) {
  return glfer_copy_hops(first, nframes, halo, 0);
}

/* samples from one plane to the next for planes of `nsamples` samples of `esz` bytes: the bytes rounded up to 16, so that every
 * plane of a 16-byte aligned block starts 16-byte aligned (and an integer-sample pitch is even, as the batch entry asks) */
static inline size_t glfer_plane_pitch(size_t nsamples, size_t esz) { return (nsamples * esz + 15) / 16 * 16 / esz; }

/* bytes of the nplanes planes that hold the hops of frames [first, first + nframes) */
static inline size_t glfer_planes_bytes(size_t first, size_t nframes, size_t halo, size_t hop, size_t esz, size_t nplanes) {
  return nplanes * glfer_plane_pitch(glfer_channel_hops(first, nframes, halo).n * hop, esz) * esz;
}

/* The piece that starts at frame `at` of a call over frames [.., end): returns its end.  Pieces end on GLOBAL multiples of
 * GLFER_FRAME_ALIGN (or at `end`).  A piece holds as many whole groups of GLFER_FRAME_ALIGN frames as keep its planes within
 * `budget` bytes -- but never fewer than GLFER_FRAME_ALIGN frames while the call has that many left: the minimum-size piece (one
 * group, and up to GLFER_FRAME_ALIGN - 1 frames in front of it when `at` is off the grid) is taken whatever the budget. */
static inline size_t glfer_channel_piece_end(size_t at, size_t end, size_t halo, size_t hop, size_t esz, size_t nplanes,
                                             size_t budget) {
  const size_t A = GLFER_FRAME_ALIGN;
  if (glfer_planes_bytes(at, end - at, halo, hop, esz, nplanes) <= budget) return end;
  /* the largest e = k * A > at with the planes of [at, e) within the budget: the bytes grow with e, so bisect over k */
  size_t lo = at / A + 1, hi = (end - 1) / A;        /* lo * A: the first boundary above at; hi * A < end */
  if (lo * A - at < A) lo++;                         /* the minimum-size piece */
  if (lo > hi) return end;
  if (glfer_planes_bytes(at, lo * A - at, halo, hop, esz, nplanes) > budget) return lo * A;
  while (lo < hi) {
    const size_t mid = lo + (hi - lo + 1) / 2;
    if (glfer_planes_bytes(at, mid * A - at, halo, hop, esz, nplanes) <= budget) lo = mid;
    else hi = mid - 1;
  }
  return lo * A;
}

#endif
