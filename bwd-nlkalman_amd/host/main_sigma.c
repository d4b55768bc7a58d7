/* main_sigma.c — `nlk-sigma`: the noise standard deviation of image files, measured on the GPU
 * (nlk_dev_estimate_sigma, include/nlk_hip.h: a block-DCT percentile estimator; the reference has no such tool,
 * its users add the noise themselves and know sigma).
 *
 *   nlk-sigma [--step N] [--frac F] [--kmin N] [--curve | --nlf [--nbins N] [--nmin N]] FILE...
 *
 * One line per file on stdout: FILE sigma sigma_0 ... sigma_{ch-1}, each value printed "%.9g" (a float read back
 * from that text is the same float). With --curve the line is FILE a_0 b_0 ... a_{ch-1} b_{ch-1}: the noise curve
 * var = a mean + b of every channel (nlk_dev_estimate_noise_curve and its defaults). With --nlf there is one line per
 * channel, FILE C K x_0 sigma_0 ... x_nbins sigma_nbins: the channel, the bins it kept and the noise level at every
 * knot of the table nlk_nlf_build makes of that curve's bins (NLK_NLF_RHO; "nan" where the channel kept none). Status 1 with a usage line when no file is named, before any device is
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

#define USAGE "usage: %s [--step N] [--frac F] [--kmin N] [--curve | --nlf [--nbins N] [--nmin N]] FILE...\n"

int nlk_tool_sigma(int argc, const char **argv) {
  struct nlk_sigma_params p;
  struct nlk_curve_params q;
  nlk_sigma_default_params(&p);
  nlk_curve_default_params(&q);
  int a = 1, curve = 0, nlf = 0, curve_only = 0;
  while (a < argc && !strncmp(argv[a], "--", 2)) {
    if (!strcmp(argv[a], "--curve")) { curve = 1; a += 1; continue; }
    if (!strcmp(argv[a], "--nlf")) { nlf = 1; a += 1; continue; }
    if (a + 1 >= argc) break;
    if (!strcmp(argv[a], "--step")) p.step = q.step = atoi(argv[a + 1]);
    else if (!strcmp(argv[a], "--frac")) p.frac = q.frac = (float)atof(argv[a + 1]);
    else if (!strcmp(argv[a], "--kmin")) p.kmin = q.kmin = atoi(argv[a + 1]);
    else if (!strcmp(argv[a], "--nbins")) { q.nbins = atoi(argv[a + 1]); curve_only = 1; }
    else if (!strcmp(argv[a], "--nmin")) { q.nmin = atoi(argv[a + 1]); curve_only = 1; }
    else break;
    a += 2;
  }
  if (a >= argc || !strncmp(argv[a], "--", 2) || (curve_only && !curve && !nlf) || (curve && nlf)) {
    fprintf(stderr, USAGE, argc > 0 ? argv[0] : "nlk-sigma");
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
    if (nlf) {
      if (ch > NLK_NLF_MAX_CH) {
        fprintf(stderr, "nlk-sigma: --nlf: %s has %d channels, at most %d\n", argv[a], ch, NLK_NLF_MAX_CH);
        return EXIT_FAILURE;
      }
      const size_t nb = q.nbins > 0 ? (size_t)q.nbins : 1, bin_bytes = sizeof(struct nlk_curve_bin) * ch * nb;
      void *d_bins = NULL;
      CHK(cli_dev_alloc(C, &d_img, bytes));
      CHK(cli_dev_alloc(C, &d_sigma, sizeof(float) * 2 * ch));
      CHK(cli_dev_alloc(C, &d_bins, bin_bytes));
      CHK(nlk_h2d(C, d_img, x, bytes));
      CHK(nlk_dev_estimate_noise_curve(C, (float *)d_sigma, (struct nlk_curve_bin *)d_bins, (const float *)d_img, w, h, ch, &q));
      struct nlk_curve_bin *bins = cli_host_keep(malloc(bin_bytes));
      struct nlk_nlf_table *tab = cli_host_keep(malloc(sizeof *tab));
      CHK(nlk_d2h(C, bins, d_bins, bin_bytes));
      if (nlk_nlf_build(tab, bins, ch, q.nbins, q.lo, q.hi, NLK_NLF_RHO) != NLK_OK) {
        fprintf(stderr, "nlk-sigma: --nlf: refused parameters\n");
        return EXIT_FAILURE;
      }
      for (int c = 0; c < ch; ++c) {
        printf("%s %d %d", argv[a], c, tab->kept[c]);
        for (int j = 0; j <= tab->nbins; ++j) printf(" %.9g %.9g", (double)tab->x[j], (double)tab->sigma[c][j]);
        printf("\n");
      }
      fflush(stdout);
      CHK(cli_dev_free(C, d_bins));
      CHK(cli_dev_free(C, d_sigma));
      CHK(cli_dev_free(C, d_img));
      cli_host_release();
      continue;
    }
    const int nval = curve ? 2 * ch : 1 + ch; /* values on the line */
    CHK(cli_dev_alloc(C, &d_img, bytes));
    CHK(cli_dev_alloc(C, &d_sigma, (size_t)nval * sizeof(float)));
    CHK(nlk_h2d(C, d_img, x, bytes));
    if (curve)
      CHK(nlk_dev_estimate_noise_curve(C, (float *)d_sigma, NULL, (const float *)d_img, w, h, ch, &q));
    else
      CHK(nlk_dev_estimate_sigma(C, (float *)d_sigma, NULL, (const float *)d_img, w, h, ch, &p));
    float *s = cli_host_keep(malloc((size_t)nval * sizeof(float)));
    CHK(nlk_d2h(C, s, d_sigma, (size_t)nval * sizeof(float)));
    printf("%s", argv[a]);
    for (int i = 0; i < nval; ++i) printf(" %.9g", (double)s[i]);
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
    fprintf(stderr, USAGE, argv[0]);
    return EXIT_FAILURE;
  }
  const int remote = cli_remote("nlk-sigma", argc, argv); /* a resident server (NLK_SERVER), if there is one */
  return remote >= 0 ? remote : nlk_tool_sigma(argc, argv);
}
#endif
