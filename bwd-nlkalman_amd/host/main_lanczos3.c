/* main_lanczos3.c — `lanczos3_decompose`, `lanczos3_recompose`: drop-ins for the Lanczos-3 pyramid tools that
 * scripts/msnlkalman-lz3-seq.sh runs around the filter (reference: lib/ms-lanczos3/lanczos3_decompose.m,
 * lanczos3_recompose.m, Octave scripts). One source; the tool is chosen by the program name, a trailing ".m"
 * ignored, so that symlinks named like the scripts work. Same arguments:
 *
 *   lanczos3_decompose input prefix levels suffix           level s -> <prefix><s><suffix>, s < levels
 *   lanczos3_recompose output prefix levels suffix [factor]  levels -> output, gblur factor (default 0)
 *
 * With fewer arguments the usage line goes to stdout and the status is 0, as the scripts do; extra arguments
 * are ignored. The pyramid runs on the GPU (nlk_dev_lz3_*): the levels stay resident between the kernels. */
#include <errno.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>

#include "cli_server.h"
#include "imgio.h"
#include "nlk_hip.h"

nlk_ctx *nlkalman_hip_context(void);

static nlk_ctx *C;
#define CHK(call)                                                   \
  do {                                                              \
    if ((call) != NLK_OK) {                                         \
      fprintf(stderr, "lanczos3 (hip): %s\n", nlk_last_error(C));   \
      cli_exit(EXIT_FAILURE);                                       \
    }                                                               \
  } while (0)

struct dimg {
  float *d;
  int w, h, ch;
};

static float *dev_alloc(size_t floats) {
  void *d = NULL;
  CHK(cli_dev_alloc(C, &d, floats * sizeof(float)));
  return (float *)d;
}

static void save(const char *path, const float *d, int w, int h, int ch) {
  const size_t bytes = (size_t)w * h * ch * sizeof(float);
  float *host = cli_host_keep(malloc(bytes));
  if (!host) { fprintf(stderr, "out of memory\n"); cli_exit(EXIT_FAILURE); }
  CHK(nlk_d2h(C, host, d, bytes));
  if (img_write(path, host, w, h, ch)) { fprintf(stderr, "cannot write %s\n", path); cli_exit(EXIT_FAILURE); }
}

/* the whole string is a number (blanks around it allowed), like the scripts' str2num of a plain number */
static int parse_int(const char *s, long *v) {
  char *end;
  errno = 0;
  *v = strtol(s, &end, 10);
  while (*end == ' ' || *end == '\t') ++end;
  return end != s && !*end && !errno;
}
static int parse_double(const char *s, double *v) {
  char *end;
  errno = 0;
  *v = strtod(s, &end);
  while (*end == ' ' || *end == '\t') ++end;
  return end != s && !*end && !errno;
}

static int decompose(int argc, char **argv) {
  if (argc < 5) {
    printf("Usage: lanczos3_decompose.m input prefix levels suffix\n");
    return EXIT_SUCCESS;
  }
  long levels;
  if (!parse_int(argv[3], &levels)) {
    fprintf(stderr, "lanczos3_decompose: levels must be a number, not `%s`\n", argv[3]);
    return EXIT_FAILURE;
  }
  char name[4096];
  int w, h, ch;
  float *host = cli_host_keep(img_read(argv[1], &w, &h, &ch));
  if (!host) return EXIT_FAILURE;
  snprintf(name, sizeof name, "%s%d%s", argv[2], 0, argv[4]);
  if (img_write(name, host, w, h, ch)) { fprintf(stderr, "cannot write %s\n", name); return EXIT_FAILURE; }
  if (levels <= 1) return EXIT_SUCCESS;
  C = nlkalman_hip_context();
  float *cur = dev_alloc((size_t)w * h * ch);
  CHK(nlk_h2d(C, cur, host, (size_t)w * h * ch * sizeof(float)));
  float *next = dev_alloc((size_t)((w + 1) / 2) * ((h + 1) / 2) * ch);  /* every later level fits in either */
  for (long s = 1; s < levels; ++s) {
    CHK(nlk_dev_lz3_down(C, next, cur, w, h, ch));
    w = (w + 1) / 2;
    h = (h + 1) / 2;
    snprintf(name, sizeof name, "%s%ld%s", argv[2], s, argv[4]);
    save(name, next, w, h, ch);
    float *t = cur;
    cur = next;
    next = t;
  }
  return EXIT_SUCCESS;
}

static int recompose(int argc, char **argv) {
  if (argc < 5) {
    printf("Usage: lanczos3_recompose.m input prefix levels suffix [factor]\n");
    return EXIT_SUCCESS;
  }
  long levels;
  double g = 0.0;
  if (!parse_int(argv[3], &levels)) {
    fprintf(stderr, "lanczos3_recompose: levels must be a number, not `%s`\n", argv[3]);
    return EXIT_FAILURE;
  }
  if (argc > 5 && !parse_double(argv[5], &g)) {
    fprintf(stderr, "lanczos3_recompose: factor must be a number, not `%s`\n", argv[5]);
    return EXIT_FAILURE;
  }
  if (!(g >= 0.0 && g < 33.0)) {
    fprintf(stderr, "lanczos3_recompose: factor %g is out of range (0 <= factor < 33)\n", g);
    return EXIT_FAILURE;
  }
  /* the coarsest level: levels - 1, or the last one before the first missing file (level 0 must be there) */
  char name[4096];
  long top = 0;
  while (top + 1 < levels) {
    snprintf(name, sizeof name, "%s%ld%s", argv[2], top + 1, argv[4]);
    if (access(name, F_OK) != 0) break;
    ++top;
  }
  struct dimg lv[64];
  if (top >= 64) { fprintf(stderr, "lanczos3_recompose: at most 64 levels\n"); return EXIT_FAILURE; }
  float *host[64];
  for (long l = 0; l <= top; ++l) {  /* every file is read before the device is touched */
    snprintf(name, sizeof name, "%s%ld%s", argv[2], l, argv[4]);
    host[l] = cli_host_keep(img_read(name, &lv[l].w, &lv[l].h, &lv[l].ch));
    if (!host[l]) return EXIT_FAILURE;
    if (l > 0 && (lv[l].w != (lv[l - 1].w + 1) / 2 || lv[l].h != (lv[l - 1].h + 1) / 2 || lv[l].ch != lv[0].ch)) {
      fprintf(stderr, "lanczos3_recompose: %s is %dx%dx%d, the level above it needs %dx%dx%d\n", name, lv[l].w,
              lv[l].h, lv[l].ch, (lv[l - 1].w + 1) / 2, (lv[l - 1].h + 1) / 2, lv[0].ch);
      return EXIT_FAILURE;
    }
  }
  if (top == 0) {
    if (img_write(argv[1], host[0], lv[0].w, lv[0].h, lv[0].ch)) { fprintf(stderr, "cannot write %s\n", argv[1]); return EXIT_FAILURE; }
    return EXIT_SUCCESS;
  }
  C = nlkalman_hip_context();
  for (long l = 0; l <= top; ++l) {
    const size_t n = (size_t)lv[l].w * lv[l].h * lv[l].ch;
    lv[l].d = dev_alloc(n);
    CHK(nlk_h2d(C, lv[l].d, host[l], n * sizeof(float)));
  }
  /* R_l = Y_l + up(gblur(R_{l+1} - down(Y_l))), in place over Y_l */
  for (long l = top - 1; l >= 0; --l)
    CHK(nlk_dev_lz3_recompose_step(C, lv[l].d, lv[l].d, lv[l].w, lv[l].h, lv[l + 1].d, lv[l + 1].w, lv[l + 1].h,
                                   lv[0].ch, (float)g));
  save(argv[1], lv[0].d, lv[0].w, lv[0].h, lv[0].ch);
  return EXIT_SUCCESS;
}

/* the program name without its directory and a trailing ".m" */
static void tool_name(const char *argv0, char *out, size_t cap) {
  const char *base = strrchr(argv0, '/');
  snprintf(out, cap, "%s", base ? base + 1 : argv0);
  const size_t n = strlen(out);
  if (n > 2 && !strcmp(out + n - 2, ".m")) out[n - 2] = 0;
}

/* the two tools as one function that looks at the name it is called by: main() below, or the resident server */
int nlk_tool_lanczos3(int argc, const char **argv_c) {
  char **argv = (char **)argv_c;
  char name[256];
  tool_name(argv[0], name, sizeof name);
  if (!strcmp(name, "lanczos3_decompose")) return decompose(argc, argv);
  if (!strcmp(name, "lanczos3_recompose")) return recompose(argc, argv);
  fprintf(stderr, "%s: call me as lanczos3_decompose or lanczos3_recompose\n", name);
  return EXIT_FAILURE;
}

#ifndef NLK_TOOL_NO_MAIN
int main(int argc, const char **argv) {
  char name[256];
  tool_name(argv[0], name, sizeof name);
  const int remote = cli_remote(name, argc, argv); /* a resident server (NLK_SERVER), if there is one */
  return remote >= 0 ? remote : nlk_tool_lanczos3(argc, argv);
}
#endif
