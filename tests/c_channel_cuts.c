/* Walks glfer_amd/csrc/channel_cuts.h as a C99 caller and prints what it returns; tests/test_channels_host.py checks the lines
 * against the definitions.  Host only. */
#include <stdio.h>

#include "channel_cuts.h"

int main(void) {
  /* N = 1024 at overlaps 0, 0.3, 0.5, 0.75, 0.875: H = (int)(N * (1.0 - overlap)), keep = N - H */
  static const size_t HOPS[] = {1024, 716, 512, 256, 128};
  static const size_t ESZ[] = {4, 2, 1};
  for (size_t i = 0; i < 5; i++) {
    const size_t hop = HOPS[i], keep = 1024 - hop;
    for (size_t lmp_av = 0; lmp_av <= 4; lmp_av += 4) {
      const size_t halo = glfer_channel_halo(keep, hop, lmp_av);
      printf("halo %zu %zu %zu %zu\n", keep, hop, lmp_av, halo);
      const size_t firsts[] = {0, 1, halo, halo + 5};
      for (size_t k = 0; k < 4; k++)
        for (size_t nframes = 0; nframes <= 9; nframes += 3) {
          const glfer_hop_span h = glfer_channel_hops(firsts[k], nframes, halo);
          printf("hops %zu %zu %zu %zu %zu\n", firsts[k], nframes, halo, h.lo, h.n);
        }
    }
  }
  for (size_t e = 0; e < 3; e++)
    for (size_t n = 0; n <= 70; n++) printf("pitch %zu %zu %zu\n", n, ESZ[e], glfer_plane_pitch(n, ESZ[e]));
  /* piece lists under shrinking budgets: hop 256 of N = 1024 (halo 3) and hop 4096 of N = 4096 (halo 0); stereo and one plane */
  static const size_t PH[][2] = {{256, 3}, {4096, 0}, {128, 10}};
  static const size_t RANGES[][2] = {{0, 200}, {33, 97}, {33, 96}, {5, 40}, {64, 65}, {100, 357}};
  for (size_t c = 0; c < 3; c++)
    for (size_t e = 0; e < 3; e++)
      for (size_t planes = 1; planes <= 2; planes++)
        for (size_t r = 0; r < 6; r++) {
          const size_t hop = PH[c][0], halo = PH[c][1], first = RANGES[r][0], end = RANGES[r][1];
          const size_t all = glfer_planes_bytes(first, end - first, halo, hop, ESZ[e], planes);
          for (size_t budget = all + 1; budget > 0; budget /= 2) {
            size_t at = first, guard = 0;
            while (at < end && guard++ < 1000) {
              const size_t to = glfer_channel_piece_end(at, end, halo, hop, ESZ[e], planes, budget);
              printf("piece %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", hop, halo, ESZ[e], planes, first, end, budget, at, to,
                     glfer_planes_bytes(at, to - at, halo, hop, ESZ[e], planes));
              if (to <= at) return 2;
              at = to;
            }
            if (at != end) return 3;
          }
        }
  /* the selection: all channels, a list, and what is refused */
  {
    unsigned char sel[GLFER_MAX_CHANNELS];
    static const int rev[] = {2, 1, 0, 1}, bad[] = {0, 3}, neg[] = {-1};
    printf("select %d\n", glfer_channel_selection(3, NULL, 99, sel));
    const int nrev = glfer_channel_selection(3, rev, 4, sel);
    printf("select %d %d %d %d\n", nrev, sel[0], sel[1], sel[3]);
    printf("select %d %d %d %d %d %d %d\n", glfer_channel_selection(3, bad, 2, sel), glfer_channel_selection(3, neg, 1, sel),
           glfer_channel_selection(0, NULL, 0, sel), glfer_channel_selection(65, NULL, 0, sel), glfer_channel_selection(3, rev, 0, sel),
           glfer_channel_selection(3, rev, 65, sel), glfer_channel_selection(64, NULL, 0, sel));
  }
  return 0;
}
