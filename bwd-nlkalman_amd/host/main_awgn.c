/* main_awgn.c — `awgn`: drop-in for imscript's noise tool (reference: lib/imscript-lite/src/awgn.c, random.c,
 * smapa.h), which scripts/nlkalman-seq-gt.sh:30-39 runs once per frame:
 *
 *   awgn sigma [in [out]]        out = in + sigma * N(0, 1), SRAND from the environment
 *
 * Same noise bit for bit (nlk_dev_awgn: the reference's LCG and Box-Muller branch on the GPU), same usage text
 * and status on a wrong argument count. SRAND is read as smapa.h reads it (sscanf "%lf", default 0) and
 * converted to the 32-bit seed as the reference's x86-64 build converts it. Files are read and written by
 * extension through host/imgio.c; "-" (stdin / stdout), which the reference's default arguments name, is not
 * supported and is refused with status 1. Behind NLK_SERVER like the other tools: the request carries no
 * environment, so the client appends its SRAND as one last argument, which nlk_tool_awgn takes off again. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "cli_server.h"
#include "imgio.h"
#include "nlk_hip.h"

nlk_ctx *nlkalman_hip_context(void);

static nlk_ctx *C;
#define CHK(call)                                                \
  do {                                                           \
    if ((call) != NLK_OK) {                                      \
      fprintf(stderr, "awgn (hip): %s\n", nlk_last_error(C));    \
      cli_exit(EXIT_FAILURE);                                    \
    }                                                            \
  } while (0)

/* smapa.h's SRAND(): the value when the variable parses as a number, else 0; then the reference's
 * xsrand(unsigned) of that double, as gcc compiles it on x86-64 (through a 64-bit integer) */
static uint32_t srand_seed(const char *sv) {
  double y;
  if (!sv || sscanf(sv, "%lf", &y) != 1) return 0;
  if (!(y > -9.2e18 && y < 9.2e18)) return 0;
  return (uint32_t)(int64_t)y;
}

static int awgn(int c, char **v, const char *srand_text) {
  if (c != 4 && c != 3 && c != 2) {
    fprintf(stderr, "usage:\n\t%s sigma [in [out]]\n", *v);
    return EXIT_FAILURE;
  }
  const float s = atof(v[1]);
  const char *in = c > 2 ? v[2] : "-";
  const char *out = c > 3 ? v[3] : "-";
  if (!strcmp(in, "-") || !strcmp(out, "-")) {
    fprintf(stderr, "awgn: standard input / output (\"-\") is not supported: name the input and output files\n");
    return EXIT_FAILURE;
  }
  int w, h, pd;
  float *x = cli_host_keep(img_read(in, &w, &h, &pd));
  if (!x) return EXIT_FAILURE;
  const size_t n = (size_t)w * h * pd;
  C = nlkalman_hip_context();
  void *d = NULL;
  CHK(cli_dev_alloc(C, &d, n * sizeof(float)));
  CHK(nlk_h2d(C, d, x, n * sizeof(float)));
  CHK(nlk_dev_awgn(C, (float *)d, (const float *)d, n, s, srand_seed(srand_text)));
  CHK(nlk_d2h(C, x, d, n * sizeof(float)));
  if (img_write(out, x, w, h, pd)) {
    fprintf(stderr, "awgn: cannot write %s\n", out);
    return EXIT_FAILURE;
  }
  return EXIT_SUCCESS;
}

/* the resident server's entry: argv is the client's, followed by "SRAND=<value>" or "SRAND" (unset) */
int nlk_tool_awgn(int argc, const char **argv) {
  const char *last = argc > 1 ? argv[argc - 1] : "";
  if (strncmp(last, "SRAND", 5) || (last[5] && last[5] != '=')) {
    fprintf(stderr, "awgn: a request without its SRAND argument\n");
    return EXIT_FAILURE;
  }
  return awgn(argc - 1, (char **)argv, last[5] ? last + 6 : NULL);
}

#ifndef NLK_TOOL_NO_MAIN
int main(int argc, const char **argv) {
  const char *sv = getenv("SRAND");
  char tag[512];
  snprintf(tag, sizeof tag, sv ? "SRAND=%s" : "SRAND", sv);
  const char **av = malloc(sizeof(char *) * (argc + 2));
  memcpy(av, argv, sizeof(char *) * argc);
  av[argc] = tag;
  av[argc + 1] = NULL;
  const int remote = cli_remote("awgn", argc + 1, av); /* a resident server (NLK_SERVER), if there is one */
  free(av);
  return remote >= 0 ? remote : awgn(argc, (char **)argv, sv);
}
#endif
