/* main_despike.c — `nlk-despike`: the defective-pixel filter of one image file on the GPU (nlk_dev_despike,
 * include/nlk_hip.h; DESIGN.md §9: the reference has no such tool).
 *
 *   nlk-despike [-r R] THR IN OUT
 *
 * A sample that lies more than THR (finite, >= 0, in the image's own units) outside the range of its ring, the samples
 * of its channel at Chebyshev distance R (1, the default, or 2), becomes the ring's median; OUT is IN otherwise, bit for
 * bit in a float format. One line on stdout: the replaced samples of every channel, "n_0 ... n_{ch-1}". Status 1 with a
 * usage line for anything else on the command line, before any device is opened; status 1 with a message for an
 * unreadable or unwritable file. The sequence tools' --despike K applies the same filter with THR = K sigma. Not behind
 * NLK_SERVER. */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "imgio.h"
#include "nlk_hip.h"

nlk_ctx *nlkalman_hip_context(void);

static nlk_ctx *C;
#define CHK(call)                                                     \
  do {                                                                \
    if ((call) != NLK_OK) {                                           \
      fprintf(stderr, "nlk-despike (hip): %s\n", nlk_last_error(C));  \
      return EXIT_FAILURE;                                            \
    }                                                                 \
  } while (0)

#define USAGE "usage: %s [-r 1|2] THR IN OUT     THR: finite, >= 0\n"

int main(int argc, const char **argv) {
  int a = 1, radius = 1;
  if (argc > 2 && !strcmp(argv[1], "-r")) {
    radius = !strcmp(argv[2], "1") ? 1 : !strcmp(argv[2], "2") ? 2 : 0;
    a = 3;
  }
  char *end = NULL;
  const float thr = argc == a + 3 ? strtof(argv[a], &end) : -1.f;
  if (argc != a + 3 || !radius || end == argv[a] || *end || !(thr >= 0.f) || !isfinite(thr)) {
    fprintf(stderr, USAGE, argc > 0 ? argv[0] : "nlk-despike");
    return EXIT_FAILURE;
  }
  int w, h, ch;
  float *x = img_read(argv[a + 1], &w, &h, &ch);
  if (!x) {
    fprintf(stderr, "nlk-despike: cannot read %s\n", argv[a + 1]);
    return EXIT_FAILURE;
  }
  if (ch > 16) {
    fprintf(stderr, "nlk-despike: %s has %d channels, at most 16\n", argv[a + 1], ch);
    return EXIT_FAILURE;
  }
  const size_t bytes = (size_t)w * h * ch * sizeof(float);
  C = nlkalman_hip_context();
  void *d_in = NULL, *d_out = NULL, *d_count = NULL;
  uint32_t count[16];
  CHK(nlk_dev_alloc(C, &d_in, bytes));
  CHK(nlk_dev_alloc(C, &d_out, bytes));
  CHK(nlk_dev_alloc(C, &d_count, sizeof count));
  CHK(nlk_h2d(C, d_in, x, bytes));
  CHK(nlk_dev_despike(C, (float *)d_out, (const float *)d_in, (uint32_t *)d_count, w, h, ch, radius, thr));
  CHK(nlk_d2h(C, x, d_out, bytes));
  CHK(nlk_d2h(C, count, d_count, sizeof(uint32_t) * ch));
  CHK(nlk_dev_free(C, d_count));
  CHK(nlk_dev_free(C, d_out));
  CHK(nlk_dev_free(C, d_in));
  if (img_write(argv[a + 2], x, w, h, ch)) {
    fprintf(stderr, "nlk-despike: cannot write %s\n", argv[a + 2]);
    return EXIT_FAILURE;
  }
  free(x);
  for (int c = 0; c < ch; ++c) printf(c ? " %u" : "%u", count[c]);
  printf("\n");
  return EXIT_SUCCESS;
}
