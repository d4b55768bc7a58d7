/* seq_step.h — what `nlkalman-seq` (host/main_seq.c) and `nlkalman-y4m` (host/main_y4m.c) share: the FPM option
 * string and one step of the forward recursion on device-resident frames, through the device C-ABI. */
#ifndef NLK_SEQ_STEP_H
#define NLK_SEQ_STEP_H

#include "nlk_hip.h"
#include "nlkalman.h"

/* every field "not given": nlkalman_default_params fills those in */
void seq_unset_params(struct nlkalman_params *p);
/* "a b  c" -> argv {prog, a, b, c}; returns argc (the vector and its strings are never freed) */
int seq_split(const char *prog, const char *s, const char ***argv_out);
/* FPM: the options of nlkalman-flt (--f1_p ... --f2_l ..., -v) as one string, into f1, f2 and *verbose; exits with
 * the parser's message on an unknown option, as nlkalman-flt does */
void seq_parse_fpm(const char *prog, const char *fpm, struct nlkalman_params *f1, struct nlkalman_params *f2,
                   int *verbose);

struct seq_step {
  nlk_ctx *ctx;
  int w, h, ch;
  float sigma;
  const struct nlkalman_params *f1, *f2;
  const float *vst_ab; /* SIG = vst: the coefficients [ch][2] and the scale of the transform; NULL: no transform */
  float vst_s;
  int fscale;          /* backward flow: finest scale, data weight (lambda) and occlusion threshold */
  float dw, th;
  float *d_rgb;        /* the noisy RGB frame; with vst_ab it is transformed in place */
  float *d_noisy, *d_tmp, *d_warp; /* work images of the frame's size ... */
  float *d_g0, *d_g1, *d_occ;      /* ... of w * h floats ... */
  float *d_flow;                   /* ... and of 2 * w * h; afterwards d_flow and d_occ hold the flow and its mask */
  const float *prev_flt1, *prev_flt2; /* the previous frame's outputs (opponent space); both NULL on the first frame */
  float *flt1, *flt2;  /* out: this frame's (opponent space) */
};
/* variance stabilisation, rgb2opp, then FLT1 and FLT2: spatial on the first frame, afterwards gray -> TV-L1 flow
 * noisy_t -> flt2_{t-1} -> occlusion mask -> warp + FLT1 -> warp + FLT2 (scripts/nlkalman-seq.sh:39-101).
 * Asynchronous on the context's stream; returns the first failing call's code (nlk_last_error has the message). */
int seq_forward_step(const struct seq_step *s);

#endif
