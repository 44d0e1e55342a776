/* lmp_groups.h -- the block list of the ragged LMP statistic (stats_kernels.hip, glfer_launch_lmp_ragged): streams of unequal
 * length, packed rows, every stream whole from its frame 0.  A launch's blocks are one flat list; a stream with frames owns
 * ceil(frames / G) consecutive blocks of it, groups of G frames counted from the stream's frame 0, and a stream without frames
 * owns none and has no entry -- so blk0 is strictly increasing and a block finds its entry by bisection (ragged_cols.hpp).  The
 * grid's x limit cuts the list into pieces of at most `piece_blocks` blocks; blk0 counts from the piece's first block.
 * Host only, integers only, plain C99 and C++ (tests/c_lmp_groups.c walks it without a GPU). */
#ifndef GLFER_LMP_GROUPS_H
#define GLFER_LMP_GROUPS_H

#include <stddef.h>

#define GLFER_LMP_PIECE_BLOCKS 0x7fffffffll   /* blocks of one launch: the grid's x limit */

/* The ring sizes whose ring is kept in registers, each with the frames a block walks (lmp_ring_kernel's G: whole turns of the
 * ring).  The only list of them: the forms below read it, and the kernels are instantiated from it (stats_kernels.hip). */
#ifdef __cplusplus
constexpr      /* (template arguments there) */
#else
static const
#endif
int glfer_lmp_ring_groups[][2] = {{2, 16}, {3, 15}, {4, 16}, {8, 16}};
static inline int glfer_lmp_ring_group(int nl) {   /* 0: no register form */
  for (size_t k = 0; k < sizeof(glfer_lmp_ring_groups) / sizeof(glfer_lmp_ring_groups[0]); k++)
    if (glfer_lmp_ring_groups[k][0] == nl) return glfer_lmp_ring_groups[k][1];
  return 0;
}

/* the three forms of the statistic's kernels, by ring size (glfer_launch_lmp's rule) */
enum { GLFER_LMP_FORM_FRAMES = 0, GLFER_LMP_FORM_REGISTERS = 1, GLFER_LMP_FORM_LDS = 2 };
static inline int glfer_lmp_form(int nl) {
  if (glfer_lmp_ring_group(nl)) return GLFER_LMP_FORM_REGISTERS;
  return nl > 1 && nl <= 64 ? GLFER_LMP_FORM_LDS : GLFER_LMP_FORM_FRAMES;
}
/* frames per block: the table's with the register ring, 64 with the ring in LDS, one frame a block frame by frame.  One value
 * per call, whatever the streams' lengths. */
static inline int glfer_lmp_ragged_group(int nl) {
  const int form = glfer_lmp_form(nl);
  if (form == GLFER_LMP_FORM_REGISTERS) return glfer_lmp_ring_group(nl);
  return form == GLFER_LMP_FORM_LDS ? 64 : 1;
}

typedef struct {
  size_t stream;       /* its index in the call */
  long long row0;      /* its first row: row_starts[stream] */
  long long nframes;   /* its rows */
  long long blk0;      /* its first block, counted from its piece's first block */
  size_t piece;        /* the piece (launch) it belongs to */
} glfer_lmp_group_entry;

/* The table of row_starts[0 .. nstreams] (non-decreasing; ragged_rows_ok) for groups of G frames.  out: room for nstreams
 * entries, or NULL to count only.  Returns the entries; *npieces (optional) receives the pieces.  An entry is never split: a
 * piece is closed when the next stream's blocks would take it past piece_blocks (a stream has at most 2^31 - 1 frames, so at
 * GLFER_LMP_PIECE_BLOCKS every stream fits a piece). */
static inline size_t glfer_lmp_group_table(const size_t *row_starts, size_t nstreams, int G, long long piece_blocks,
                                           glfer_lmp_group_entry *out, size_t *npieces) {
  size_t n = 0, pieces = 0;
  long long in_piece = 0;
  for (size_t b = 0; b < nstreams; b++) {
    const long long frames = (long long)(row_starts[b + 1] - row_starts[b]);
    if (frames <= 0) continue;
    const long long blocks = (frames + G - 1) / G;
    if (pieces == 0 || in_piece + blocks > piece_blocks) {
      pieces++;
      in_piece = 0;
    }
    if (out) {
      out[n].stream = b;
      out[n].row0 = (long long)row_starts[b];
      out[n].nframes = frames;
      out[n].blk0 = in_piece;
      out[n].piece = pieces - 1;
    }
    in_piece += blocks;
    n++;
  }
  if (npieces) *npieces = pieces;
  return n;
}

#endif
