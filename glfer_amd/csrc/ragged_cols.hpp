// ragged_cols.hpp -- the per-stream table of the ragged forms of the per-column kernels (aux_kernels.hip, display.hip):
// streams of unequal length, packed rows, one launch.  A launch's blocks are ONE flat list (blockIdx.x): an entry owns the
// blocks [blk0, next entry's blk0), in the unit of the kernel it is made for -- chunks of the stream's own chunk length
// (avg_fused_kernel), chunks of AVG_CHUNK (avg_cum_kernel) or LEV_CHUNK (levels_kernel), rows (avg_norm_kernel, map_kernel).
// Only streams with work in the launch have an entry, so blk0 is strictly increasing and a block finds its entry by bisection
// (uniform over the block: scalar loads).  A 2-D grid (blockIdx.y the stream, blocks past the stream's end leaving at once)
// needs nstreams x the LONGEST stream's blocks, whatever the other streams' lengths; the flat list has the blocks there is work
// for and no 65 535-stream limit.  Tables are built on the host per call and live in stream-ordered scratch.
#ifndef GLFER_RAGGED_COLS_HPP
#define GLFER_RAGGED_COLS_HPP

#include <hip/hip_runtime.h>

#include <initializer_list>
#include <vector>

#include "scratch.hpp"

namespace glfer {

struct RaggedColsEntry {
  long long row0;      // the stream's first row in the packed input (PSD rows, statistics) and in outputs packed the same way
  long long out0;      // its first row in the launch's own output where that is packed differently (averaged rows in scratch)
  long long nframes;   // its frame count: the chunks, their lead-in rows and effdepth are the stream's own
  long long blk0;      // its first block of the launch
  int chunk;           // avg_fused_kernel: the chunk length a launch over this stream alone takes
  int stream;          // its index in the call (the row of the carried display state)
};
struct RaggedCols {
  const RaggedColsEntry *tab;
  int n;
};

#if defined(__HIPCC__)
__device__ __forceinline__ RaggedColsEntry ragged_cols_find(const RaggedCols &r, long long blk) {
  int lo = 0, hi = r.n - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (r.tab[mid].blk0 <= blk) lo = mid;
    else hi = mid - 1;
  }
  return r.tab[lo];
}
#endif

// ---- host side: the tables of one launcher call

// One launch's entries, in stream order.  The grid's x limit cuts it into pieces of at most 2^31 - 1 blocks (a stream has at
// most 2^31 - 1 frames, so an entry always fits one); blk0 counts from the piece's first block.
struct RaggedPiece {
  size_t first, count;     // entries of the table
  long long blocks;
};
struct RaggedTable {
  std::vector<RaggedColsEntry> e;
  std::vector<RaggedPiece> pieces;
  size_t base = 0;         // the table's first entry in the uploaded block (ragged_upload)
  void add(RaggedColsEntry x, long long blocks) {
    if (pieces.empty() || pieces.back().blocks + blocks > 0x7fffffffll || pieces.back().count == 0x40000000u)
      pieces.push_back(RaggedPiece{e.size(), 0, 0});
    x.blk0 = pieces.back().blocks;
    pieces.back().blocks += blocks;
    pieces.back().count++;
    e.push_back(x);
  }
  RaggedCols cols(const RaggedColsEntry *d_tabs, const RaggedPiece &p) const { return RaggedCols{d_tabs + base + p.first, (int)p.count}; }
};
// the tables of a call into ONE stream-ordered allocation, one copy, on d_tabs' stream (empty tables: d_tabs stays empty)
inline hipError_t ragged_upload(std::initializer_list<RaggedTable *> tabs, Scratch<RaggedColsEntry> &d_tabs) {
  std::vector<RaggedColsEntry> all;
  for (RaggedTable *t : tabs) {
    t->base = all.size();
    all.insert(all.end(), t->e.begin(), t->e.end());
  }
  d_tabs.release();
  return all.empty() ? hipSuccess : d_tabs.upload(all.data(), all.size());
}

// ---- the ragged entries' own rules (waterfall.cpp)
// true where `st` is being captured into a graph: the per-stream tables are uploaded from host memory that is gone when the call
// returns, which a captured copy would read at every replay
bool stream_is_capturing(hipStream_t st);
// row_starts of nstreams streams: non-decreasing, at most 2^31 - 1 rows a stream
bool ragged_rows_ok(const size_t *row_starts, size_t nstreams);
// the streams that have rows, as the ragged launchers take them (out0 = row0: outputs packed as the rows are)
std::vector<RaggedColsEntry> ragged_streams(const size_t *row_starts, size_t nstreams);

}  // namespace glfer

#endif
