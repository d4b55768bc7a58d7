/* main_bmflow.c — `bmflow`, the block-matching optical flow of two image files (nlk_dev_bm_flow, include/nlk_hip.h):
 * tvl1flow's sibling, with the same reading of its inputs (any format the I/O layer reads; colour is reduced to
 * luminance by nlk_dev_gray) and the same output (the flow by extension, .flo / .tif / .pfm, two interleaved channels).
 *
 *   bmflow I0 I1 OUT [FSCALE [RADIUS]]      FSCALE: finest level that is matched (default 1); RADIUS: 1..3 (default 2) */
#include <stdio.h>
#include <stdlib.h>

#include "imgio.h"
#include "nlk_hip.h"

nlk_ctx *nlkalman_hip_context(void); /* libnlkalman.so: the process-wide device context */

static int fail_hip(const char *what, nlk_ctx *c) {
  fprintf(stderr, "bmflow: %s: %s\n", what, nlk_last_error(c));
  return EXIT_FAILURE;
}

int main(int argc, const char **argv) {
  if (argc < 4 || argc > 6) {
    fprintf(stderr, "usage: %s I0 I1 OUT [FSCALE [RADIUS]]\n", *argv);
    return EXIT_FAILURE;
  }
  struct nlk_bmflow_params P;
  nlk_bmflow_default_params(&P);
  if (argc > 4) P.fscale = atoi(argv[4]);
  if (argc > 5) P.radius = atoi(argv[5]);
  if (P.fscale < 0 || P.radius < 1 || P.radius > 3) {
    fprintf(stderr, "bmflow: FSCALE must be >= 0 and RADIUS 1..3\n");
    return EXIT_FAILURE;
  }
  int nx, ny, c0, nx2, ny2, c1;
  float *I0 = img_read(argv[1], &nx, &ny, &c0);
  if (!I0) { fprintf(stderr, "ERROR: could not read image from file \"%s\"\n", argv[1]); return EXIT_FAILURE; }
  float *I1 = img_read(argv[2], &nx2, &ny2, &c1);
  if (!I1) { fprintf(stderr, "ERROR: could not read image from file \"%s\"\n", argv[2]); return EXIT_FAILURE; }
  if (nx != nx2 || ny != ny2) {
    fprintf(stderr, "ERROR: input images size mismatch %dx%d != %dx%d\n", nx, ny, nx2, ny2);
    return EXIT_FAILURE;
  }
  if (c0 == 2 || c0 > 4 || c1 == 2 || c1 > 4) {
    fprintf(stderr, "ERROR: non-scalarizable image\n");
    return EXIT_FAILURE;
  }
  nlk_ctx *c = nlkalman_hip_context();
  const size_t n = (size_t)nx * ny, cmax = (size_t)(c0 > c1 ? c0 : c1);
  void *d_im = NULL, *d_g0 = NULL, *d_g1 = NULL, *d_flow = NULL;
  if (nlk_dev_alloc(c, &d_im, n * cmax * sizeof(float)) || nlk_dev_alloc(c, &d_g0, n * sizeof(float)) ||
      nlk_dev_alloc(c, &d_g1, n * sizeof(float)) || nlk_dev_alloc(c, &d_flow, 2 * n * sizeof(float)))
    return fail_hip("allocation", c);
  if (nlk_h2d(c, d_im, I0, n * c0 * sizeof(float)) || nlk_dev_gray(c, (float *)d_g0, (float *)d_im, nx, ny, c0) ||
      nlk_sync(c) ||
      nlk_h2d(c, d_im, I1, n * c1 * sizeof(float)) || nlk_dev_gray(c, (float *)d_g1, (float *)d_im, nx, ny, c1))
    return fail_hip("upload", c);
  if (nlk_dev_bm_flow(c, (float *)d_flow, (float *)d_g0, (float *)d_g1, nx, ny, &P)) return fail_hip("flow", c);
  float *flow = malloc(2 * n * sizeof(float));
  if (!flow || nlk_d2h(c, flow, d_flow, 2 * n * sizeof(float))) return fail_hip("download", c);
  if (img_write(argv[3], flow, nx, ny, 2)) {
    fprintf(stderr, "ERROR: could not write \"%s\"\n", argv[3]);
    return EXIT_FAILURE;
  }
  return EXIT_SUCCESS;
}
