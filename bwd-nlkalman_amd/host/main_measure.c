/* main_measure.c — `nlk-measure`: the error measures of image files against a reference file, on the GPU
 * (nlk_dev_sqdiff_sum and nlk_dev_ssim, include/nlk_hip.h). What scripts/psnr.sh does for one pair of files with
 * three plambda processes, for any number of files in one resident process, and the SSIM beside it.
 *
 *   nlk-measure [--range L] REF FILE...
 *
 * One line per FILE on stdout: FILE MSE RMSE PSNR SSIM, each number printed "%.9g". With n the number of samples,
 * MSE = the squared-error sum / n, RMSE = sqrt(MSE), PSNR = 20 log10(L / RMSE) ("inf" at MSE = 0), SSIM = the mean
 * over the channels (d_ssim[0]); L is 255 unless --range gives it. This is plain double arithmetic on purpose: it
 * does NOT imitate plambda's stack of floats, so its digits are not those of psnr.sh. OUT/measures of
 * nlkalman-seq-gt does imitate it (main_seq.c: write_measures) and stays as it is.
 *
 * REF is uploaded once. Status 1 with a usage line when fewer than two files are named, before any device is opened;
 * status 1 with a message for an unreadable file, for a FILE whose size or channel count differs from REF's, for an
 * image smaller than 11 x 11 and for a range that is not positive. Behind NLK_SERVER like the other tools. */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "cli_server.h"
#include "imgio.h"
#include "nlk_hip.h"

nlk_ctx *nlkalman_hip_context(void);

static nlk_ctx *C;
#define CHK(call)                                                     \
  do {                                                                \
    if ((call) != NLK_OK) {                                           \
      fprintf(stderr, "nlk-measure (hip): %s\n", nlk_last_error(C));  \
      cli_exit(EXIT_FAILURE);                                         \
    }                                                                 \
  } while (0)

#define USAGE "usage: %s [--range L] REF FILE...\n"

int nlk_tool_measure(int argc, const char **argv) {
  float range = 255.f;
  int a = 1;
  while (a + 1 < argc && !strcmp(argv[a], "--range")) {
    range = (float)atof(argv[a + 1]);
    a += 2;
  }
  if (argc - a < 2 || !strncmp(argv[a], "--", 2)) {
    fprintf(stderr, USAGE, argc > 0 ? argv[0] : "nlk-measure");
    return EXIT_FAILURE;
  }
  if (!(range > 0.f && range <= 3.402823466e38f)) {
    fprintf(stderr, "nlk-measure: --range must be positive and finite\n");
    return EXIT_FAILURE;
  }
  const char *ref_name = argv[a++];
  int w, h, ch;
  float *ref = cli_host_keep(img_read(ref_name, &w, &h, &ch));
  if (!ref) {
    fprintf(stderr, "nlk-measure: cannot read %s\n", ref_name);
    return EXIT_FAILURE;
  }
  if (w < 11 || h < 11) {
    fprintf(stderr, "nlk-measure: %s is %d x %d, smaller than the 11 x 11 window\n", ref_name, w, h);
    return EXIT_FAILURE;
  }
  const size_t n = (size_t)w * h * ch, bytes = n * sizeof(float);
  C = nlkalman_hip_context();
  void *d_ref = NULL, *d_img = NULL, *d_res = NULL;
  CHK(cli_dev_alloc(C, &d_ref, bytes));
  CHK(cli_dev_alloc(C, &d_img, bytes));
  CHK(cli_dev_alloc(C, &d_res, (size_t)(2 + ch) * sizeof(double))); /* squared-error sum | ssim, ssim_0 ... */
  CHK(nlk_h2d(C, d_ref, ref, bytes));
  double *res = cli_host_keep(malloc((size_t)(2 + ch) * sizeof(double)));
  for (; a < argc; ++a) {
    int w1, h1, c1;
    float *x = img_read(argv[a], &w1, &h1, &c1);
    if (!x) {
      fprintf(stderr, "nlk-measure: cannot read %s\n", argv[a]);
      return EXIT_FAILURE;
    }
    if (w1 != w || h1 != h || c1 != ch) {
      fprintf(stderr, "nlk-measure: %s is %dx%dx%d, %s is %dx%dx%d\n", argv[a], w1, h1, c1, ref_name, w, h, ch);
      free(x);
      return EXIT_FAILURE;
    }
    const int rc = nlk_h2d(C, d_img, x, bytes);
    free(x);
    CHK(rc);
    CHK(nlk_dev_sqdiff_sum(C, (double *)d_res, (const float *)d_ref, (const float *)d_img, n));
    CHK(nlk_dev_ssim(C, (double *)d_res + 1, NULL, (const float *)d_ref, (const float *)d_img, w, h, ch, range));
    CHK(nlk_d2h(C, res, d_res, (size_t)(2 + ch) * sizeof(double)));
    const double mse = res[0] / (double)n, rmse = sqrt(mse);
    printf("%s %.9g %.9g ", argv[a], mse, rmse);
    if (mse == 0.0) printf("inf");
    else printf("%.9g", 20.0 * log10((double)range / rmse));
    printf(" %.9g\n", res[1]);
    fflush(stdout);
  }
  CHK(cli_dev_free(C, d_res));
  CHK(cli_dev_free(C, d_img));
  CHK(cli_dev_free(C, d_ref));
  cli_host_release(); /* the reference image and the values */
  return EXIT_SUCCESS;
}

#ifndef NLK_TOOL_NO_MAIN
int main(int argc, const char **argv) {
  if (argc < 3) { /* nothing to ask a server for either */
    fprintf(stderr, USAGE, argv[0]);
    return EXIT_FAILURE;
  }
  const int remote = cli_remote("nlk-measure", argc, argv); /* a resident server (NLK_SERVER), if there is one */
  return remote >= 0 ? remote : nlk_tool_measure(argc, argv);
}
#endif
