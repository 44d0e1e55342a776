/* Walks glfer_amd/csrc/frame_cuts.h as a C99 caller and prints what it returns; tests/test_frame_cuts_host.py checks the lines
 * against the definitions.  Host only. */
#include <stdio.h>

#include "frame_cuts.h"

int main(void) {
  static const size_t FI[] = {0, 1, 3, 7}, GS[] = {1, 2, 8, 16};
  static const int NS[] = {256, 512, 1024, 2048, 4096, 8192, 16384};
  for (int fmt = 0; fmt < 3; fmt++) printf("size %d %zu\n", fmt, glfer_sample_size(fmt));
  for (size_t hop = 1; hop <= 9; hop++)
    for (size_t keep = 0; keep <= 30; keep++) printf("inside %zu %zu %zu\n", keep, hop, glfer_first_inside(keep, hop));
  for (size_t i = 0; i < sizeof NS / sizeof *NS; i++)
    printf("group %d %zu %zu\n", NS[i], glfer_frame_group(1, NS[i]), glfer_frame_group(0, NS[i]));
  for (size_t lo = 0; lo <= 40; lo++)
    for (size_t hi = lo; hi <= lo + 40; hi++)
      for (size_t i = 0; i < 4; i++) {
        const size_t fi = FI[i];
        for (size_t g = 0; g < 4; g++) {
          const glfer_frame_cut c = glfer_cut_frames(lo, hi, fi, GS[g]);
          const glfer_hop_span m = glfer_means_hops(c.b0, c.b1, 0, fi);
          printf("cut %zu %zu %zu %zu %zu %zu\n", lo, hi, fi, GS[g], c.b0, c.b1);
          printf("means %zu %zu 0 %zu %zu %zu\n", c.b0, c.b1, fi, m.lo, m.n);
        }
        /* the averages' body: from depth - 1 = 3 frames above the first frame inside, to the end of the call */
        const size_t b0 = glfer_cut_frames(lo, hi, fi, 1).b0 + 3;
        if (b0 < hi) {
          const glfer_hop_span m = glfer_means_hops(b0, hi, 3, fi);
          printf("means %zu %zu 3 %zu %zu %zu\n", b0, hi, fi, m.lo, m.n);
        }
        /* frames [lo, hi) through a corrected copy: history from the stream, or ZERO_ALWAYS; with and without a fresh tail */
        for (int hm = 0; hm < 2; hm++)
          for (int fresh = 0; fresh < 2; fresh++) {
            const size_t back = glfer_hops_back(hm, fi);
            const glfer_hop_span h = glfer_copy_hops(lo, hi - lo, back, fresh);
            printf("copy %zu %zu %zu %d %zu %zu\n", lo, hi - lo, back, fresh, h.lo, h.n);
          }
      }
  return 0;
}
