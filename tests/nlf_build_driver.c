/* nlf_build_driver.c — nlk_nlf_build (bwd-nlkalman_amd/host/nlf_build.c) as a stand-alone program for
 * tests/test_nlf.py. Links nlf_build.c alone. Reads cases from the file named on the command line, each
 *   ch nbins lo hi rho count      then count bins  N n m v  ("nan" is read as NaN)
 * and prints per case "rc R" and, for R = 0, the lines "s S inv_dx D", "kept K_0 ...", "x ...", and per channel
 * "G c ...", "slope c ...", "islope c ...", "sigma c ..." (each float "%.9g"). */
#include <stdio.h>
#include <stdlib.h>

#include "nlk_hip.h"

static void row(const char *name, int c, const float *v, int n) {
  if (c >= 0) printf("%s %d", name, c);
  else printf("%s", name);
  for (int j = 0; j < n; ++j) printf(" %.9g", (double)v[j]);
  printf("\n");
}

int main(int argc, char **argv) {
  FILE *f = argc > 1 ? fopen(argv[1], "r") : NULL;
  if (!f) { printf("error: cannot open the file\n"); return 1; }
  int ch, nbins, count;
  float lo, hi, rho;
  while (fscanf(f, "%d %d %f %f %f %d", &ch, &nbins, &lo, &hi, &rho, &count) == 6) {
    if (count < 0 || count > 1 << 20) return 2;
    struct nlk_curve_bin *bins = calloc(count ? (size_t)count : 1, sizeof *bins);
    struct nlk_nlf_table *t = malloc(sizeof *t); /* (its own allocation: a write past it is seen) */
    if (!bins || !t) return 2;
    for (int i = 0; i < count; ++i)
      if (fscanf(f, "%d %d %f %f", &bins[i].nblocks, &bins[i].nsel, &bins[i].mean, &bins[i].var) != 4) return 2;
    const int rc = nlk_nlf_build(t, bins, ch, nbins, lo, hi, rho);
    printf("rc %d\n", rc);
    if (rc == 0) {
      printf("s %.9g inv_dx %.9g\nkept", (double)t->s, (double)t->inv_dx);
      for (int c = 0; c < ch; ++c) printf(" %d", t->kept[c]);
      printf("\n");
      row("x", -1, t->x, nbins + 1);
      for (int c = 0; c < ch; ++c) {
        row("G", c, t->G[c], nbins + 1);
        row("slope", c, t->slope[c], nbins);
        row("islope", c, t->islope[c], nbins);
        row("sigma", c, t->sigma[c], nbins + 1);
      }
    }
    free(t);
    free(bins);
  }
  fclose(f);
  return 0;
}
