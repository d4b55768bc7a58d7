/* frame_grid_driver.c — nlk_frame_grid and nlk_strip_plan (bwd-nlkalman_amd/host/frame_grid.c) as a stand-alone
 * program for tests/test_frame_grid.py. Arguments: triples H PSZ HALO. For each and for world = 1 .. 64: the plan of
 * an H-row frame into an array of exactly `world` records (so that a sanitizer sees a record too many), one line
 * "h H psz PSZ halo HALO world W code C" and, for code 0, one line "gy0 gy1 Y0 Y1 own0 own1" per rank. Links
 * frame_grid.c alone. */
#include <stdio.h>
#include <stdlib.h>

#include "nlk_hip.h"

int main(int argc, char **argv) {
  for (int i = 1; i + 2 < argc; i += 3) {
    const int h = atoi(argv[i]), psz = atoi(argv[i + 1]), halo = atoi(argv[i + 2]);
    struct nlkalman_params P = {psz, halo, 0, 1, 1, 1, 0.f, 1.f, 1.f}; /* a first frame: the spatial radius is the halo */
    struct nlk_frame_grid g;
    if (nlk_frame_grid(psz, h, &P, 0, 0, &g) != NLK_OK || g.halo != halo) return 2;
    for (int world = 1; world <= 64; ++world) {
      struct nlk_strip_plan *plan = malloc(sizeof *plan * world);
      if (!plan) return 3;
      const int code = nlk_strip_plan(h, &g, world, plan);
      printf("h %d psz %d halo %d world %d code %d\n", h, psz, halo, world, code);
      for (int r = 0; code == NLK_OK && r < world; ++r)
        printf("%d %d %d %d %d %d\n", plan[r].gy0, plan[r].gy1, plan[r].Y0, plan[r].Y1, plan[r].own0, plan[r].own1);
      free(plan);
    }
  }
  return 0;
}
