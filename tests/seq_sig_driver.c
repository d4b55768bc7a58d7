/* seq_sig_driver.c — seq_sig_parse (bwd-nlkalman_amd/host/seq_args.c) as a stand-alone program for
 * tests/test_seq_sig.py: one line per argument, "mode M a A b B sigma S code C" (M: 0 number, 1 auto, 2 vst,
 * 3 vst:A,B; the floats as "%.9g"). Links seq_args.c alone. */
#include <stdio.h>

#include "seq_step.h"

int main(int argc, char **argv) {
  for (int i = 1; i < argc; ++i) {
    struct seq_sig sig;
    const int code = seq_sig_parse(argv[i], &sig);
    printf("mode %d a %.9g b %.9g sigma %.9g code %d\n", sig.mode, (double)sig.a, (double)sig.b, (double)sig.sigma, code);
  }
  return 0;
}
