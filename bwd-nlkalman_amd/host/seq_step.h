/* seq_step.h — what `nlkalman-seq`, `nlkalman-lsmo-seq` (host/main_seq.c) and `nlkalman-y4m` (host/main_y4m.c) share:
 * the FPM and SPM option strings, one step of the forward recursion and one step of the lag-1 smoother on
 * device-resident frames, through the device C-ABI. */
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
/* SPM: the options of nlkalman-smo (--s1_p ..., -v) as one string, into s1 and *verbose, likewise */
void seq_parse_spm(const char *prog, const char *spm, struct nlkalman_params *s1, int *verbose);

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

/* ---- the lag-1 smoother (scripts/nlkalman-lsmo-seq.sh:87-108): as soon as frame i is filtered, frame i - 1 is
 * smoothed against flt2_i. The flow flt2_{i-1} -> flt2_i it needs comes from one of two sources. */
enum {
  SEQ_LAG1_OFF = 0,
  SEQ_LAG1_TVL1,  /* the script's: a second TV-L1 flow per frame */
  SEQ_LAG1_INV    /* the inverse of the backward flow that the forward step of frame i left in d_flow */
};
/* fixed-point steps of nlk_dev_flow_invert in SEQ_LAG1_INV: the count at which the inverted flow was measured against
 * the script's own flow on the CPU oracle (the table of DESIGN.md §9: within 0.05 dB at sigma <= 20, 0.15 dB at 40) */
#define SEQ_LAG1_INVERT_STEPS 4
/* "tvl1" | "inv" -> the mode; anything else: SEQ_LAG1_OFF */
int seq_lag1_mode(const char *name);

struct seq_lag1 {
  nlk_ctx *ctx;
  int w, h, ch;
  float sigma;
  const struct nlkalman_params *s1;
  int mode;            /* SEQ_LAG1_TVL1 | SEQ_LAG1_INV */
  int fscale;          /* forward flow: finest scale and data weight (TVL1 only), occlusion threshold (both) */
  float dw, th;
  float *d_tmp, *d_warp;  /* work images of the frame's size ... */
  float *d_g0, *d_g1;     /* ... and of w * h floats (TVL1 only) */
  const float *d_bflow;   /* INV: the backward flow noisy_i -> flt2_{i-1} */
  float *d_fflow, *d_focc; /* out: the forward flow (2 * w * h) and its mask (w * h) */
  const float *prev_flt2, *cur_flt2; /* flt2_{i-1}, flt2_i (opponent space) */
  float *lsm1;         /* out: the smoothed frame i - 1 (opponent space) */
};
/* gray of both frames -> TV-L1 flow flt2_{i-1} -> flt2_i (or the inverted backward flow) -> occlusion mask -> warp of
 * flt2_i -> SMO1(flt1 = flt2_{i-1}, smo0 = the warp). Asynchronous on the context's stream; returns the first failing
 * call's code. */
int seq_lag1_step(const struct seq_lag1 *s);

#endif
