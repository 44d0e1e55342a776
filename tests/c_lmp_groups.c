/* Walks glfer_amd/csrc/lmp_groups.h as a C99 caller: reads cases from stdin, one per line --
 *     nl piece_blocks nstreams row_starts[0] ... row_starts[nstreams]
 * -- and prints the form and group length of the ring size, then the table: "case G form entries pieces" followed by one
 * "entry stream row0 nframes blk0 piece" line per entry.  tests/test_lmp_host.py checks the lines against a restatement.
 * Host only. */
#include <stdio.h>
#include <stdlib.h>

#include "lmp_groups.h"

int main(void) {
  int nl;
  long long piece_blocks;
  size_t nstreams;
  while (scanf("%d %lld %zu", &nl, &piece_blocks, &nstreams) == 3) {
    size_t *starts = (size_t *)malloc((nstreams + 1) * sizeof *starts);
    glfer_lmp_group_entry *e = (glfer_lmp_group_entry *)malloc((nstreams + 1) * sizeof *e);
    if (!starts || !e) return 2;
    for (size_t b = 0; b <= nstreams; b++)
      if (scanf("%zu", &starts[b]) != 1) return 3;
    const int G = glfer_lmp_ragged_group(nl);
    size_t pieces = 0, pieces_counted = 0;
    const size_t n = glfer_lmp_group_table(starts, nstreams, G, piece_blocks, e, &pieces);
    if (glfer_lmp_group_table(starts, nstreams, G, piece_blocks, NULL, &pieces_counted) != n || pieces_counted != pieces) return 4;
    printf("case %d %d %zu %zu\n", G, glfer_lmp_form(nl), n, pieces);
    for (size_t k = 0; k < n; k++) printf("entry %zu %lld %lld %lld %zu\n", e[k].stream, e[k].row0, e[k].nframes, e[k].blk0, e[k].piece);
    free(starts);
    free(e);
  }
  return 0;
}
