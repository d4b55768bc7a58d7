/* main_defects.c — `nlk-defects`: the defect map learned over a list of image files on the GPU (nlk_dev_defect_step and
 * nlk_defect_schedule, include/nlk_hip.h; DESIGN.md §9: the reference has no such tool). nlk-despike's sibling.
 *
 *   nlk-defects [-r R] [-n N] K SIGMA OUTMAP FILE...
 *
 * The files are the frames of one sensor, in order, all of one size. Frame t is tested against the running mean of the
 * frames 0 .. t - 1 (window N = 2 .. 4096, default 32) at thr = K SIGMA / sqrt(min(t, N)) and ring radius R (1, the
 * default, or 2); K and SIGMA are finite and > 0, SIGMA in the images' own units. One line per frame on stdout: the
 * samples of every channel that the step replaced, "n_0 ... n_{ch-1}" (the first frame: zeros). OUTMAP gets the map of
 * the last step as an image of the frames' size: 255 where a sample's mean is flagged, 0 elsewhere, per channel. Status
 * 1 with a usage line for anything else on the command line, before any device is opened; status 1 with a message for
 * an unreadable or unwritable file or a frame of another size. The sequence tools' --defect-map K[,R[,N]] runs the same
 * steps at the run's sigma. Not behind NLK_SERVER. */
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
      fprintf(stderr, "nlk-defects (hip): %s\n", nlk_last_error(C));  \
      return EXIT_FAILURE;                                            \
    }                                                                 \
  } while (0)

#define USAGE "usage: %s [-r 1|2] [-n N] K SIGMA OUTMAP FILE...     K, SIGMA: finite, > 0; N: 2 .. 4096 (default 32)\n"

/* a finite number > 0, the whole text; else 0 */
static float positive(const char *text) {
  char *end = NULL;
  const float v = strtof(text, &end);
  return end != text && !*end && isfinite(v) && v > 0.f ? v : 0.f;
}

int main(int argc, const char **argv) {
  int a = 1, radius = 1, window = 32, bad = 0;
  while (a + 1 < argc && (!strcmp(argv[a], "-r") || !strcmp(argv[a], "-n"))) {
    char *end = NULL;
    const long v = strtol(argv[a + 1], &end, 10);
    if (end == argv[a + 1] || *end) bad = 1;
    else if (argv[a][1] == 'r') { radius = (int)v; bad |= v != 1 && v != 2; }
    else { window = (int)v; bad |= v < 2 || v > 4096; }
    a += 2;
  }
  const float k = argc >= a + 4 ? positive(argv[a]) : 0.f, sigma = argc >= a + 4 ? positive(argv[a + 1]) : 0.f;
  if (bad || argc < a + 4 || !(k > 0.f) || !(sigma > 0.f)) {
    fprintf(stderr, USAGE, argc > 0 ? argv[0] : "nlk-defects");
    return EXIT_FAILURE;
  }
  const char *outmap = argv[a + 2];
  const int nfiles = argc - (a + 3);
  int w = 0, h = 0, ch = 0;
  size_t n = 0, bytes = 0;
  void *d_in = NULL, *d_out = NULL, *d_mean[2] = {NULL, NULL}, *d_map = NULL, *d_count = NULL;
  uint32_t count[16];
  float *x = NULL;
  for (int t = 0; t < nfiles; ++t) {
    const char *name = argv[a + 3 + t];
    int fw, fh, fch;
    free(x);
    x = img_read(name, &fw, &fh, &fch);
    if (!x) {
      fprintf(stderr, "nlk-defects: cannot read %s\n", name);
      return EXIT_FAILURE;
    }
    if (t == 0) {
      if (fch > 16) {
        fprintf(stderr, "nlk-defects: %s has %d channels, at most 16\n", name, fch);
        return EXIT_FAILURE;
      }
      w = fw; h = fh; ch = fch;
      n = (size_t)w * h * ch;
      bytes = n * sizeof(float);
      C = nlkalman_hip_context();
      CHK(nlk_dev_alloc(C, &d_in, bytes));
      CHK(nlk_dev_alloc(C, &d_out, bytes));
      CHK(nlk_dev_alloc(C, &d_mean[0], bytes));
      CHK(nlk_dev_alloc(C, &d_mean[1], bytes));
      CHK(nlk_dev_alloc(C, &d_map, n));
      CHK(nlk_dev_alloc(C, &d_count, sizeof count));
    } else if (fw != w || fh != h || fch != ch) {
      fprintf(stderr, "nlk-defects: %s is %dx%dx%d, the first frame %dx%dx%d\n", name, fw, fh, fch, w, h, ch);
      return EXIT_FAILURE;
    }
    float thr = 0.f, gain = 1.f;
    if (t > 0 && nlk_defect_schedule(t, window, k * sigma, &thr, &gain) != NLK_OK) return EXIT_FAILURE;
    CHK(nlk_h2d(C, d_in, x, bytes));
    CHK(nlk_dev_defect_step(C, (float *)d_out, (const float *)d_in, (float *)d_mean[(t + 1) & 1],
                            t > 0 ? (const float *)d_mean[t & 1] : NULL, (uint8_t *)d_map, (uint32_t *)d_count, w, h, ch,
                            radius, thr, gain));
    CHK(nlk_d2h(C, count, d_count, sizeof(uint32_t) * ch));
    for (int c = 0; c < ch; ++c) printf(c ? " %u" : "%u", count[c]);
    printf("\n");
  }
  uint8_t *map = malloc(n);
  if (!map) return EXIT_FAILURE;
  CHK(nlk_d2h(C, map, d_map, n));
  for (size_t i = 0; i < n; ++i) x[i] = map[i] ? 255.f : 0.f;
  free(map);
  void *all[] = {d_count, d_map, d_mean[1], d_mean[0], d_out, d_in};
  for (int i = 0; i < 6; ++i) CHK(nlk_dev_free(C, all[i]));
  if (img_write(outmap, x, w, h, ch)) {
    fprintf(stderr, "nlk-defects: cannot write %s\n", outmap);
    return EXIT_FAILURE;
  }
  free(x);
  return EXIT_SUCCESS;
}
