/* Walks glfer_amd/csrc/drift_cuts.h as a C99 caller and prints what it returns; tests/test_drift_host.py checks the lines against
 * the definitions.  Host only. */
#include <stdio.h>

#include "drift_cuts.h"

int main(void) {
  static const int TS[] = {2, 3, 5, 16, 17};
  /* the admissible ranges and what lies just outside them */
  static const int ARGS[][4] = {{2, 1, -1, 1},   {2, 1, -2, 1},   {1, 1, 0, 0},      {16, 0, -15, 15},    {16, 1, -15, 16}, {16, 1, 1, 15},
                                {16, 1, -15, -1}, {16, 3, 0, 0},   {4096, 1, -127, 127}, {4096, 1, -128, 127}, {4097, 1, 0, 0},  {256, 256, -254, 0},
                                {256, 256, 0, 254}, {256, 7, -255, 0}, {3, 9, -2, 2},      {3, 9, -3, 0}};
  for (size_t i = 0; i < sizeof ARGS / sizeof ARGS[0]; i++)
    printf("args %d %d %d %d %d\n", ARGS[i][0], ARGS[i][1], ARGS[i][2], ARGS[i][3],
           glfer_drift_args_ok((size_t)ARGS[i][0], (size_t)ARGS[i][1], ARGS[i][2], ARGS[i][3]));
  for (size_t i = 0; i < sizeof TS / sizeof TS[0]; i++)
    for (int d = -(TS[i] - 1); d <= TS[i] - 1; d++)
      for (int t = 0; t < TS[i]; t++) printf("off %d %d %d %d\n", TS[i], d, t, glfer_drift_offset(TS[i], d, t));
  for (size_t T = 2; T <= 17; T += 5)
    for (size_t step = 1; step <= T + 3; step += (T + 2) / 2)
      for (size_t F = 0; F <= 3 * T + 4; F++) printf("blocks %zu %zu %zu %zu\n", F, T, step, glfer_drift_blocks(F, T, step));
  /* piece lists under shrinking budgets: the call's first frame on and off the frame grid */
  static const size_t SHAPES[][4] = {{16, 16, 40, 0}, {16, 4, 100, 7}, {64, 67, 9, 33}, {2, 1, 300, 64}, {17, 17, 1, 5}, {256, 64, 12, 31}};
  for (size_t c = 0; c < sizeof SHAPES / sizeof SHAPES[0]; c++) {
    const size_t T = SHAPES[c][0], step = SHAPES[c][1], nblocks = SHAPES[c][2], first = SHAPES[c][3], row_bytes = 4 * 129;
    const size_t end = first + glfer_drift_span(nblocks, T, step);
    for (size_t budget = glfer_drift_piece_rows(nblocks, T, step) * row_bytes + 1;; budget /= 2) {
      size_t b0 = 0, guard = 0;
      while (b0 < nblocks && guard++ < 100000) {
        const size_t nb = glfer_drift_piece_blocks(nblocks - b0, T, step, row_bytes, budget);
        if (nb < 1 || nb > nblocks - b0) return 2;
        const size_t a = first + b0 * step, e = a + glfer_drift_span(nb, T, step);
        printf("piece %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", T, step, nblocks, first, budget, b0, nb, glfer_drift_piece_rows(nb, T, step),
               glfer_drift_piece_lo(a, first), glfer_drift_piece_hi(e, end));
        b0 += nb;
      }
      if (b0 != nblocks) return 3;
      if (budget == 0) break;
    }
  }
  return 0;
}
