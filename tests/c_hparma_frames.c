/* Walks glfer_amd/csrc/hparma_frames.h as a C99 caller: reads lines from stdin --
 *     lds n t ncol
 *     table piece_frames nstreams counts[0] ... counts[nstreams - 1]
 * -- and prints "lds bytes resident" for the first kind, and for the second "case entries pieces" followed by one
 * "entry stream g0 nframes piece" line per entry.  tests/test_hparma_batch_host.py checks the lines against a restatement.
 * Host only. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "hparma_frames.h"

int main(void) {
  char kind[16];
  while (scanf("%15s", kind) == 1) {
    if (strcmp(kind, "lds") == 0) {
      int n, t, ncol;
      if (scanf("%d %d %d", &n, &t, &ncol) != 3) return 3;
      const size_t bytes = glfer_hparma_lds_bytes(n, t, ncol);
      printf("lds %zu %lld\n", bytes, glfer_hparma_resident(bytes));
      continue;
    }
    if (strcmp(kind, "table") != 0) return 5;
    long long piece_frames;
    size_t nstreams;
    if (scanf("%lld %zu", &piece_frames, &nstreams) != 2) return 3;
    long long *counts = (long long *)malloc((nstreams + 1) * sizeof *counts);
    glfer_hparma_frames_entry *e = (glfer_hparma_frames_entry *)malloc((nstreams + 1) * sizeof *e);
    if (!counts || !e) return 2;
    for (size_t b = 0; b < nstreams; b++)
      if (scanf("%lld", &counts[b]) != 1) return 3;
    size_t pieces = 0, pieces_counted = 0;
    const size_t n = glfer_hparma_frame_table(counts, nstreams, piece_frames, e, &pieces);
    if (glfer_hparma_frame_table(counts, nstreams, piece_frames, NULL, &pieces_counted) != n || pieces_counted != pieces) return 4;
    printf("case %zu %zu\n", n, pieces);
    for (size_t k = 0; k < n; k++) printf("entry %zu %lld %lld %zu\n", e[k].stream, e[k].g0, e[k].nframes, e[k].piece);
    free(counts);
    free(e);
  }
  return 0;
}
