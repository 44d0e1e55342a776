/* drift_cuts.h -- the integer arithmetic of the drift search (glfer_hip.h, "Drift search"): which drift ranges a block length
 * admits, the offset of a drift at a frame, the blocks of a run of rows, and how the spectrogram-level entry cuts its blocks
 * into pieces whose rows fit a byte budget.
 * Host only, integers only, plain C99 and C++ (tests/c_drift_cuts.c walks it without a GPU); the kernel (drift.hip) restates
 * the offset for the device. */
#ifndef GLFER_DRIFT_CUTS_H
#define GLFER_DRIFT_CUTS_H

#include <stddef.h>
#include <stdint.h>

#define GLFER_DRIFT_MAX_FRAMES 4096
#define GLFER_DRIFT_MAX_DRIFTS 255
/* the frame grid of "Cutting a stream", rule (1) (GLFER_FRAME_ALIGN of glfer_hip.h, restated so that this header stands alone) */
#define GLFER_DRIFT_ROW_ALIGN 32

/* frames 2 .. 4096, step >= 1, dmin <= 0 <= dmax inside -(frames - 1) .. frames - 1, at most 255 drifts */
static inline int glfer_drift_args_ok(size_t frames, size_t step, int dmin, int dmax) {
  if (frames < 2 || frames > GLFER_DRIFT_MAX_FRAMES || step < 1) return 0;
  if (dmin > 0 || dmax < 0 || dmin < -(int)(frames - 1) || dmax > (int)(frames - 1)) return 0;
  return dmax - dmin + 1 <= GLFER_DRIFT_MAX_DRIFTS;
}

/* o(d, t) = sgn(d) ((2 |d| t + (T - 1)) div (2 (T - 1))): d t / (T - 1) rounded half away from zero (T >= 2, t < T) */
static inline int glfer_drift_offset(int frames, int d, int t) {
  const int a = d < 0 ? -d : d, o = (2 * a * t + (frames - 1)) / (2 * (frames - 1));
  return d < 0 ? -o : o;
}

/* blocks of `frames` rows, `step` rows apart, in a run of nrows rows: (nrows - frames) / step + 1, none in a shorter run */
static inline size_t glfer_drift_blocks(size_t nrows, size_t frames, size_t step) {
  if (frames < 1 || step < 1 || nrows < frames) return 0;
  return (nrows - frames) / step + 1;
}

/* rows blocks [0, nb) span: (nb - 1) step + frames; SIZE_MAX where that wraps.  nb >= 1 */
static inline size_t glfer_drift_span(size_t nb, size_t frames, size_t step) {
  if (nb - 1 > (SIZE_MAX - frames) / step) return SIZE_MAX;
  return (nb - 1) * step + frames;
}

/* The rows the spectrogram-level entry computes for a piece whose blocks span frames [a, e) of a call over frames [A, E): the
 * piece's own and those that complete its first and last group of GLFER_DRIFT_ROW_ALIGN frames inside the call, so that every
 * frame is computed in the company it has in the one-shot run, whatever the cut (rule (1) of "Cutting a stream"). */
static inline size_t glfer_drift_piece_lo(size_t a, size_t A) {
  const size_t g = a / GLFER_DRIFT_ROW_ALIGN * GLFER_DRIFT_ROW_ALIGN;
  return g < A ? A : g;
}
static inline size_t glfer_drift_piece_hi(size_t e, size_t E) {
  const size_t R = GLFER_DRIFT_ROW_ALIGN;
  if (e > SIZE_MAX - R) return E;
  const size_t g = (e + R - 1) / R * R;
  return g > E ? E : g;
}

/* rows a piece of nb blocks may take: its span and the 2 (GLFER_DRIFT_ROW_ALIGN - 1) rows that complete its end groups */
static inline size_t glfer_drift_piece_rows(size_t nb, size_t frames, size_t step) {
  const size_t s = glfer_drift_span(nb, frames, step), extra = 2 * (GLFER_DRIFT_ROW_ALIGN - 1);
  return s > SIZE_MAX - extra ? SIZE_MAX : s + extra;
}

/* Blocks of the next piece when `left` blocks remain: as many as keep glfer_drift_piece_rows times row_bytes within `budget`
 * bytes, one block at least whatever the budget. */
static inline size_t glfer_drift_piece_blocks(size_t left, size_t frames, size_t step, size_t row_bytes, size_t budget) {
  const size_t rows = budget / row_bytes, fixed = frames + 2 * (GLFER_DRIFT_ROW_ALIGN - 1);
  size_t nb;
  if (left <= 1 || rows < fixed) return left < 1 ? left : 1;
  nb = (rows - fixed) / step + 1;
  return nb < left ? nb : left;
}

#endif
