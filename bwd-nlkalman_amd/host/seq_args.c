/* seq_args.c — the grammar of the sequence tools' SIG argument and of --despike's and --defect-map's values (seq_step.h). Plain C: nothing of the device libraries
 * is needed to link it. */
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
