/* seq_args.c — the grammar of the sequence tools' SIG argument, of --of's, --despike's and --defect-map's values and the
 * one reader of the options all four tools share (seq_step.h). Plain C: nothing of the device libraries is needed to
 * link it. */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "seq_step.h"

int seq_sig_parse(const char *text, struct seq_sig *sig) {
  memset(sig, 0, sizeof *sig);
  if (!strncmp(text, "vst", 3)) { /* "vst" measures the curve, "vst:A,B" is told it */
    sig->mode = text[3] ? SEQ_SIG_VST_GIVEN : SEQ_SIG_VST;
    return text[3] && (sscanf(text + 3, ":%f,%f", &sig->a, &sig->b) != 2 || !(sig->a >= 0.f) || !(sig->b >= 0.f) ||
                       !(sig->a + sig->b > 0.f) || !(sig->a + sig->b <= 3e38f));
  }
  if (!strcmp(text, "auto")) sig->mode = SEQ_SIG_AUTO;
  else if (!strcmp(text, "nlf")) sig->mode = SEQ_SIG_NLF;
  else sig->sigma = atof(text);
  return 0;
}

int seq_despike_parse(const char *text, float *k, int *r) {
  char *end = NULL;
  const float v = text ? strtof(text, &end) : 0.f;
  int radius = 1;
  if (!text || end == text || !isfinite(v) || !(v > 0.f)) return 1;
  if (*end == ',') { /* ",R": one digit, 1 or 2 */
    if ((end[1] != '1' && end[1] != '2') || end[2]) return 1;
    radius = end[1] - '0';
  } else if (*end) return 1;
  *k = v;
  *r = radius;
  return 0;
}

int seq_defect_parse(const char *text, float *k, int *r, int *n) {
  char *end = NULL;
  const float v = text ? strtof(text, &end) : 0.f;
  int radius = 1, window = SEQ_DEFECT_N;
  if (!text || end == text || !isfinite(v) || !(v > 0.f)) return 1;
  if (*end == ',') { /* ",R": one digit, 1 or 2 */
    if (end[1] != '1' && end[1] != '2') return 1;
    radius = end[1] - '0';
    end += 2;
    if (*end == ',') { /* ",N": digits only, 2 .. 4096 */
      const char *p = end + 1;
      long w = 0;
      if (!*p || *p == '0') return 1;
      for (; *p >= '0' && *p <= '9' && w <= 4096; ++p) w = 10 * w + (*p - '0');
      if (*p || w < 2 || w > 4096) return 1;
      window = (int)w;
      end = (char *)p;
    }
  }
  if (*end) return 1;
  *k = v;
  *r = radius;
  *n = window;
  return 0;
}

int seq_of_mode(const char *name) {
  if (name && !strcmp(name, "tvl1")) return SEQ_OF_TVL1;
  if (name && !strcmp(name, "bm")) return SEQ_OF_BM;
  return -1;
}

/* ---- the shared options: one row each, in the order main_seq.c admits them */
static int opt_of(const char *text, struct seq_opts *o) {
  const int of = seq_of_mode(text);
  if (of >= 0) o->of = of;
  return of < 0;
}
static int opt_despike(const char *text, struct seq_opts *o) { return seq_despike_parse(text, &o->despike_k, &o->despike_r); }
static int opt_defect(const char *text, struct seq_opts *o) {
  return seq_defect_parse(text, &o->defect_k, &o->defect_r, &o->defect_n);
}
static int opt_sure(const char *text, struct seq_opts *o) {
  (void)text;
  o->sure = 1;
  return 0;
}
static const struct {
  const char *name;
  int arity;        /* entries of argv: 1 a flag, 2 an option and its value */
  const char *want; /* the line of a refused or missing value (prog, text) */
  int (*set)(const char *text, struct seq_opts *o);
} seq_opt_rows[] = {{"--of", 2, SEQ_OF_WANT, opt_of},
                    {"--despike", 2, SEQ_DESPIKE_WANT, opt_despike},
                    {"--defect-map", 2, SEQ_DEFECT_WANT, opt_defect},
                    {"--sure", 1, NULL, opt_sure}};
#define SEQ_OPT_ROWS ((int)(sizeof seq_opt_rows / sizeof seq_opt_rows[0]))

int seq_opts_arity(const char *name) {
  for (int i = 0; i < SEQ_OPT_ROWS; ++i)
    if (!strcmp(name, seq_opt_rows[i].name)) return seq_opt_rows[i].arity;
  return 0;
}

int seq_opts_read(struct seq_opts *o, int argc, const char **argv, int at, int *from, const char *prog) {
  for (int i = from ? *from : 0; at < argc && i < SEQ_OPT_ROWS; ++i) {
    if (strcmp(argv[at], seq_opt_rows[i].name)) continue;
    const char *text = seq_opt_rows[i].arity == 2 && at + 1 < argc ? argv[at + 1] : NULL;
    if (seq_opt_rows[i].set(text, o)) {
      fprintf(stderr, seq_opt_rows[i].want, prog, text ? text : "");
      return -1;
    }
    if (from) *from = i + 1;
    return seq_opt_rows[i].arity;
  }
  return 0;
}
