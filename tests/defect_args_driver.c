/* defect_args_driver.c — seq_defect_parse (bwd-nlkalman_amd/host/seq_args.c) as a stand-alone program for
 * tests/test_defect_map.py: one line per argument, "k K r R n N code C" (K as "%.9g"; K = -1, R = -1, N = -1 are what
 * the caller had before the call: a refused text leaves them). Links seq_args.c alone. */
#include <stdio.h>

#include "seq_step.h"

int main(int argc, char **argv) {
  for (int i = 1; i < argc; ++i) {
    float k = -1.f;
    int r = -1, n = -1;
    const int code = seq_defect_parse(argv[i], &k, &r, &n);
    printf("k %.9g r %d n %d code %d\n", (double)k, r, n, code);
  }
  return 0;
}
