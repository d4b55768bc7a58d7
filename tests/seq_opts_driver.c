/* seq_opts_driver.c — seq_opts_read and seq_opts_arity (bwd-nlkalman_amd/host/seq_args.c) as a stand-alone program for
 * tests/test_seq_run.py. The arguments are vectors separated by "//", each MODE ARG...: MODE = "order" walks the
 * vector as main_seq.c does (the table's rows once each, in their order, until an argument is none of those left),
 * MODE = "any" as main_y4m.c does (every row at every place; an argument that is no shared option is stepped over).
 * Per vector one stdout line: "read N N ... stop AT of O despike K R defect K R N sure S" (N: what every call
 * returned, the last of them 0 or -1; AT: the index of the first argument not read; floats as "%.9g"); what
 * seq_opts_read prints goes to stderr under the name "prog". With "arity NAME ..." as the only vector: one line of
 * seq_opts_arity's values. Links seq_args.c alone. */
#include <stdio.h>
#include <string.h>

#include "seq_step.h"

int main(int argc, const char **argv) {
  if (argc > 1 && !strcmp(argv[1], "arity")) {
    for (int i = 2; i < argc; ++i) printf(i > 2 ? " %d" : "%d", seq_opts_arity(argv[i]));
    printf("\n");
    return 0;
  }
  for (int a = 1; a < argc;) {
    int b = a;
    while (b < argc && strcmp(argv[b], "//")) ++b;
    const int any = !strcmp(argv[a], "any"), n = b - (a + 1);
    const char **v = argv + a + 1;
    struct seq_opts o;
    memset(&o, 0, sizeof o);
    int at = 0, from = 0;
    printf("read");
    for (;;) {
      const int got = seq_opts_read(&o, n, v, at, any ? NULL : &from, "prog");
      printf(" %d", got);
      if (got < 0 || (got == 0 && (!any || at >= n))) break;
      at += got ? got : 1; /* (any: an argument of the tool's own is stepped over) */
    }
    printf(" stop %d of %d despike %.9g %d defect %.9g %d %d sure %d\n", at, o.of, (double)o.despike_k, o.despike_r,
           (double)o.defect_k, o.defect_r, o.defect_n, o.sure);
    fflush(stdout);
    a = b + 1;
  }
  return 0;
}
