/* main_sigma.c — `nlk-sigma`: the noise standard deviation of image files, measured on the GPU
 * (nlk_dev_estimate_sigma, include/nlk_hip.h: a block-DCT percentile estimator; the reference has no such tool,
 * its users add the noise themselves and know sigma).
 *
 *   nlk-sigma [--step N] [--frac F] [--kmin N] FILE...
 *
 * One line per file on stdout: FILE sigma sigma_0 ... sigma_{ch-1}, each value printed "%.9g" (a float read back
 * from that text is the same float). Status 1 with a usage line when no file is named, before any device is
 * opened; status 1 with a message for an unreadable file or a refused parameter. Behind NLK_SERVER like the
 * other tools. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "cli_server.h"
#include "imgio.h"
#include "nlk_hip.h"

nlk_ctx *nlkalman_hip_context(void);

static nlk_ctx *C;
#define CHK(call)                                                   \
  do {                                                              \
    if ((call) != NLK_OK) {                                         \
      fprintf(stderr, "nlk-sigma (hip): %s\n", nlk_last_error(C));  \
      cli_exit(EXIT_FAILURE);                                       \
    }                                                               \
  } while (0)

int nlk_tool_sigma(int argc, const char **argv) {
  struct nlk_sigma_params p;
  nlk_sigma_default_params(&p);
  int a = 1;
  for (; a + 1 < argc && !strncmp(argv[a], "--", 2); a += 2) {
    if (!strcmp(argv[a], "--step")) p.step = atoi(argv[a + 1]);
    else if (!strcmp(argv[a], "--frac")) p.frac = (float)atof(argv[a + 1]);
    else if (!strcmp(argv[a], "--kmin")) p.kmin = atoi(argv[a + 1]);
    else break;
  }
  if (a >= argc || !strncmp(argv[a], "--", 2)) {
    fprintf(stderr, "usage: %s [--step N] [--frac F] [--kmin N] FILE...\n", argc > 0 ? argv[0] : "nlk-sigma");
    return EXIT_FAILURE;
  }
  for (; a < argc; ++a) {
    int w, h, ch;
    float *x = cli_host_keep(img_read(argv[a], &w, &h, &ch));
    if (!x) {
      fprintf(stderr, "nlk-sigma: cannot read %s\n", argv[a]);
      return EXIT_FAILURE;
    }
    const size_t bytes = (size_t)w * h * ch * sizeof(float);
    C = nlkalman_hip_context();
    void *d_img = NULL, *d_sigma = NULL;
    CHK(cli_dev_alloc(C, &d_img, bytes));
    CHK(cli_dev_alloc(C, &d_sigma, (size_t)(1 + ch) * sizeof(float)));
    CHK(nlk_h2d(C, d_img, x, bytes));
    CHK(nlk_dev_estimate_sigma(C, (float *)d_sigma, NULL, (const float *)d_img, w, h, ch, &p));
    float *s = cli_host_keep(malloc((size_t)(1 + ch) * sizeof(float)));
    CHK(nlk_d2h(C, s, d_sigma, (size_t)(1 + ch) * sizeof(float)));
    printf("%s", argv[a]);
    for (int i = 0; i <= ch; ++i) printf(" %.9g", (double)s[i]);
    printf("\n");
    fflush(stdout);
    CHK(cli_dev_free(C, d_sigma));
    CHK(cli_dev_free(C, d_img));
    cli_host_release(); /* this file's image and values */
  }
  return EXIT_SUCCESS;
}

#ifndef NLK_TOOL_NO_MAIN
int main(int argc, const char **argv) {
  if (argc < 2) { /* nothing to ask a server for either */
    fprintf(stderr, "usage: %s [--step N] [--frac F] [--kmin N] FILE...\n", argv[0]);
    return EXIT_FAILURE;
  }
  const int remote = cli_remote("nlk-sigma", argc, argv); /* a resident server (NLK_SERVER), if there is one */
  return remote >= 0 ? remote : nlk_tool_sigma(argc, argv);
}
#endif
