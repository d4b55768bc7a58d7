/* seq_step.h — what `nlkalman-seq`, `nlkalman-seq-gt`, `nlkalman-lsmo-seq` (host/main_seq.c) and `nlkalman-y4m`
 * (host/main_y4m.c) share, each stated once: the SIG argument (its grammar in host/seq_args.c, which links by itself;
 * its first-frame resolution here), the FPM and SPM option strings, the work images, one step of the forward recursion,
 * one smoother step (the lag-1 smoother's, and the whole-sequence backward pass's) and the way an opponent-space frame
 * becomes an output frame, on device-resident frames through the device C-ABI. */
#ifndef NLK_SEQ_STEP_H
#define NLK_SEQ_STEP_H

#include <stdio.h>

#include "nlk_hip.h"
#include "nlkalman.h"

/* ---- SIG: a number | auto | vst | vst:A,B | nlf */
enum {
  SEQ_SIG_NUMBER = 0, /* the noise standard deviation itself */
  SEQ_SIG_AUTO,       /* measured on the first frame (nlk_dev_estimate_sigma) */
  SEQ_SIG_VST,        /* var = a y + b, the pair of every channel measured on the first frame ... */
  SEQ_SIG_VST_GIVEN,  /* ... or given: every channel uses (a, b) */
  SEQ_SIG_NLF         /* a noise-level function of any shape: the bins of the first frame's noise curve as a table */
};
#define SEQ_SIG_MAX_CH 16 /* channels of a variance-stabilised frame (nlk_dev_vst_forward's limit) */
struct seq_sig {
  int mode;
  float a, b;                       /* SEQ_SIG_VST_GIVEN */
  float sigma;                      /* the sigma of the run: SEQ_SIG_NUMBER as given, else 0 until seq_sig_resolve */
  float vst_ab[2 * SEQ_SIG_MAX_CH]; /* vst, resolved: the coefficients [ch][2] and the scale of the transform */
  float vst_s;
  struct nlk_nlf_table nlf;         /* nlf, resolved: the table of nlk_nlf_build (its s is the sigma of the run) */
};
/* the grammar, nothing else: no device call, no output. 0, or 1 for a "vst..." that is neither "vst" nor "vst:A,B" with
 * A, B >= 0, not both 0, A + B <= 3e38 (the caller prints SEQ_SIG_WANT under its own name); sig->mode is set either
 * way. "nlf" is the whole word. Anything that is not "auto", "nlf" or "vst..." is a number as atof reads it.
 * (host/seq_args.c) */
int seq_sig_parse(const char *text, struct seq_sig *sig);
#define SEQ_SIG_WANT "%s: SIG = %s: want vst or vst:A,B with A, B >= 0, not both 0\n" /* (prog, text) */
/* the first frame's work, d_rgb being that frame as pushed: measures what the mode asks for, downloads it, fills
 * sigma, vst_ab and vst_s (nlf: the table, from the bins of nlk_dev_estimate_noise_curve at its defaults and
 * NLK_NLF_RHO) and prints the one line "sigma S" | "vst a_0 b_0 ... sigma S" | "nlf kept K_0 ... sigma S" (K_c: the
 * bins channel c kept; each float "%.9g") to `report`; SEQ_SIG_NUMBER: nothing to do. Returns NLK_OK, the code of a failed device call (nlk_last_error has the
 * message), or SEQ_SIG_REFUSED after a message under `prog` on stderr: more than SEQ_SIG_MAX_CH channels under vst
 * or nlf, or a frame that gives no positive sigma (nlf: a channel that kept no bin). */
#define SEQ_SIG_REFUSED 1
int seq_sig_resolve(nlk_ctx *ctx, struct seq_sig *sig, const float *d_rgb, int w, int h, int ch, FILE *report,
                    const char *prog);
/* the coefficients of the transform, NULL when the run has none */
static inline const float *seq_sig_vst(const struct seq_sig *sig) {
  return sig->mode == SEQ_SIG_VST || sig->mode == SEQ_SIG_VST_GIVEN ? sig->vst_ab : NULL;
}
/* the table of the transform, NULL when the run has none */
static inline const struct nlk_nlf_table *seq_sig_nlf(const struct seq_sig *sig) {
  return sig->mode == SEQ_SIG_NLF ? &sig->nlf : NULL;
}

/* ---- FPM, SPM (every field starts as cli_params_unset leaves it, host/cli_args.h) */
/* "a b  c" -> argv {prog, a, b, c}; returns argc (the vector and its strings are never freed) */
int seq_split(const char *prog, const char *s, const char ***argv_out);
/* FPM: the options of nlkalman-flt (--f1_p ... --f2_l ..., -v) as one string, into f1, f2 and *verbose; exits with
 * the parser's message on an unknown option, as nlkalman-flt does */
void seq_parse_fpm(const char *prog, const char *fpm, struct nlkalman_params *f1, struct nlkalman_params *f2,
                   int *verbose);
/* SPM: the options of nlkalman-smo (--s1_p ..., -v) as one string, into s1 and *verbose, likewise */
void seq_parse_spm(const char *prog, const char *spm, struct nlkalman_params *s1, int *verbose);
/* every field not given: the default of the three stages at this sigma */
void seq_default_params(struct nlkalman_params *f1, struct nlkalman_params *f2, struct nlkalman_params *s1, float sigma);

/* ---- the work images of a run */
struct seq_work {
  float *d_noisy, *d_tmp, *d_warp; /* of the frame's size ... */
  float *d_g0, *d_g1, *d_occ;      /* ... of w * h floats ... */
  float *d_flow;                   /* ... and of 2 * w * h: after a forward step d_flow and d_occ hold its flow and mask */
  float *d_fflow, *d_focc;         /* with_smoother only: the lag-1 smoother's flow (2 * w * h) and mask (w * h) */
};
/* one device allocation per image; returns the first failing call's code (what was allocated stays for seq_work_free) */
int seq_work_alloc(nlk_ctx *ctx, struct seq_work *k, int w, int h, int ch, int with_smoother);
void seq_work_free(nlk_ctx *ctx, struct seq_work *k);

/* ---- the flow estimator of a run: every flow that a step computes comes from it */
enum {
  SEQ_OF_TVL1 = 0, /* the scripts': nlk_dev_tvl1_flow at OPM's FSCALE and DW */
  SEQ_OF_BM        /* nlk_dev_bm_flow at OPM's FSCALE (its other parameters are the defaults; DW is ignored) */
};
/* "tvl1" | "bm" -> the estimator; anything else: -1 (the caller prints SEQ_OF_WANT under its own name) */
int seq_of_mode(const char *name);
#define SEQ_OF_WANT "%s: --of %s: want tvl1 or bm\n" /* (prog, text) */

/* ---- --despike K[,R]: defective pixels (nlk_dev_despike, include/nlk_hip.h) are taken out of every
 * noisy frame before the filter sees it, at thr = K sigma and ring radius R. The grammar, nothing else (host/seq_args.c):
 * "K" or "K,R" with K finite and > 0 and R = 1 or 2 (default 1) -> 0 and *k, *r; anything else: 1, *k and *r as they
 * were (the caller prints SEQ_DESPIKE_WANT under its own name). K = 4 is the value DESIGN.md §9's table was made with. */
int seq_despike_parse(const char *text, float *k, int *r);
#define SEQ_DESPIKE_WANT "%s: --despike %s: want K or K,R with K > 0 and R = 1 or 2\n" /* (prog, text) */

/* ---- --defect-map K[,R[,N]]: a defect map learned over time (nlk_dev_defect_step, include/nlk_hip.h).
 * Streaming: frame t is cleaned with the evidence of the frames 0 .. t - 1, whose running mean (no motion compensation)
 * is tested at thr = K sigma / sqrt(min(t, N)) and ring radius R (nlk_defect_schedule). The grammar, nothing else
 * (host/seq_args.c): "K", "K,R" or "K,R,N" with K finite and > 0, R = 1 or 2 (default 1) and N = 2 .. 4096 (default
 * 32) -> 0 and *k, *r, *n; anything else: 1, and they stay as they were (the caller prints SEQ_DEFECT_WANT under its own
 * name). K = 4, N = 32 are the values DESIGN.md §9's table was made with. */
#define SEQ_DEFECT_N 32
int seq_defect_parse(const char *text, float *k, int *r, int *n);
#define SEQ_DEFECT_WANT "%s: --defect-map %s: want K, K,R or K,R,N with K > 0, R = 1 or 2 and N = 2 .. 4096\n" /* (prog, text) */
/* the state of a run: the two mean planes (of the frame's size; the steps swap them) and the index of the next frame */
struct seq_defects {
  float k;
  int r, n;
  long t;
  float *d_mean[2];
};
/* one device allocation per plane, t = 0; returns the first failing call's code (what was allocated stays for
 * seq_defects_free) */
int seq_defects_alloc(nlk_ctx *ctx, struct seq_defects *d, float k, int r, int n, int w, int h, int ch);
void seq_defects_free(nlk_ctx *ctx, struct seq_defects *d);

/* ---- one step of the forward recursion */
struct seq_step {
  nlk_ctx *ctx;
  int w, h, ch;
  int of;                    /* SEQ_OF_TVL1 | SEQ_OF_BM */
  const struct seq_sig *sig; /* resolved */
  const struct nlkalman_params *f1, *f2;
  int fscale;                /* backward flow: finest scale, data weight (lambda) and occlusion threshold */
  float dw, th;
  const struct seq_work *work;
  struct seq_defects *defects; /* NULL: off; else the defect map of the run: the step reads and advances it */
  float despike_k;           /* 0: off; else the noisy frame is despiked at thr = despike_k * sig->sigma ... */
  int despike_r;             /* ... and this ring radius (1 or 2) */
  /* per frame: */
  float *d_rgb;              /* the noisy RGB frame; under vst and nlf it is transformed in place, and despiked likewise */
  const float *prev_flt1, *prev_flt2; /* the previous frame's outputs (opponent space); both NULL on the first frame */
  float *flt1, *flt2;        /* out: this frame's (opponent space) */
};
/* variance stabilisation, then with `defects` the step of the defect map (in the domain where the run's sigma holds:
 * nlk_dev_defect_step reads d_rgb and the mean of the frames before, writes work->d_noisy and the other mean plane, then
 * a copy back to d_rgb; defects->t advances; with defects == NULL nothing is allocated or launched that was not
 * before), then with despike_k != 0 the defective-pixel filter (in the domain where the run's sigma
 * holds, before rgb2opp and the flow's gray image: nlk_dev_despike into work->d_noisy, which is free at that point, and
 * a copy back to d_rgb; with despike_k == 0 nothing is launched that was not before), rgb2opp, then FLT1 and FLT2: spatial on the first frame, afterwards gray -> flow (TV-L1, or
 * under SEQ_OF_BM block matching) noisy_t -> flt2_{t-1} -> occlusion mask -> warp + FLT1 -> warp + FLT2 (scripts/nlkalman-seq.sh:39-101).
 * Asynchronous on the context's stream; returns the first failing call's code (nlk_last_error has the message). */
int seq_forward_step(const struct seq_step *s);

/* ---- the error estimate of a forward step without clean frames: Monte-Carlo SURE (include/nlk_hip.h: nlk_dev_probe_add,
 * nlk_dev_sure_terms). The noise of frame t is independent of everything before it, so the estimate holds
 * for the recursion's frame t with the previous outputs held fixed; it costs one more FLT1 and FLT2, on a perturbed
 * frame. Under vst / nlf the estimate is in the stabilised domain, at the run's sigma. With despike_k != 0 the probe goes
 * on the frame the filter saw, the despiked one (work->d_noisy): the estimate treats the despiked frame as the data. */
#define SEQ_SURE_EPS_REL 0.05f /* the probe, in units of sigma: the middle of the plateau 0.025 .. 0.1 of DESIGN.md §9's table */
#define SEQ_SURE_BLOCK 16      /* the tile of nlk_dev_sure_terms */
#define SEQ_SURE_FRAME_STEP 0xD1B54A32D192ED03ull /* the seed of frame t = seed + t * this (mod 2^64) */
struct seq_sure {
  float eps_rel;  /* eps = eps_rel * sigma */
  uint64_t seed;
  int block;
  float *d_probe, *d_flt1, *d_flt2; /* of the frame's size: the perturbed frame and its two estimates */
  double *d_blocks;                 /* NULL, or the map of flt2's terms, [nby][nbx][ch][2] (nlk_dev_sure_terms) */
};
/* eps_rel, seed, block = the defaults above, seed 0; NLK_SURE_EPS (> 0) and NLK_SURE_SEED (strtoull, any base) override;
 * one device allocation per image, with_map: also the map. Returns the first failing call's code (what was allocated
 * stays for seq_sure_free). */
int seq_sure_alloc(nlk_ctx *ctx, struct seq_sure *u, int w, int h, int ch, int with_map);
void seq_sure_free(nlk_ctx *ctx, struct seq_sure *u);
/* after seq_forward_step(s) of frame t (t = 0: the first), while work->d_noisy, d_flow and d_occ still hold that step's
 * values: the probe on d_noisy, the two warps again when there is a previous frame, FLT1', then FLT2' with FLT1' as its
 * basic estimate, and the terms of flt1 into d_slot[0 .. 2 ch), those of flt2 into d_slot[2 ch .. 4 ch) (device doubles,
 * R_c and D_c interleaved). Writes u's images and work->d_warp, nothing else: s->flt1, s->flt2 and what a following
 * seq_lag1_step reads stay as they are. Asynchronous on the context's stream; returns the first failing call's code. */
int seq_sure_step(const struct seq_step *s, const struct seq_sure *u, long t, double *d_slot);
/* the estimate of one pass of one frame from its 2 ch downloaded terms, added over the channels */
struct seq_sure_est { double mse, psnr, resid, div; }; /* MSE_hat, 10 log10(255^2 / MSE_hat), R / N, D / (eps N) */
struct seq_sure_est seq_sure_estimate(const double *terms, int w, int h, int ch, float sigma, float eps_rel);

/* ---- one smoother step: frame i is smoothed against a later frame's estimate. The lag-1 smoother
 * (scripts/nlkalman-lsmo-seq.sh:87-108) does it as soon as frame i + 1 is filtered, next = flt2_{i+1}; the backward pass
 * of the whole sequence (scripts/nlkalman-seq.sh:117-150) from the last frame down, next = smo1_{i+1}. The flow
 * flt2_i -> next it needs comes from one of two sources. */
enum {
  SEQ_LAG1_OFF = 0,
  SEQ_LAG1_TVL1,  /* the scripts': a flow of its own (TV-L1, or under SEQ_OF_BM block matching) */
  SEQ_LAG1_INV    /* the inverse of the backward flow that the forward step of frame i + 1 left in work->d_flow */
};
/* fixed-point steps of nlk_dev_flow_invert in SEQ_LAG1_INV: the count at which the inverted flow was measured against
 * the script's own flow on the CPU oracle (the table of DESIGN.md §9: within 0.05 dB at sigma <= 20, 0.15 dB at 40) */
#define SEQ_LAG1_INVERT_STEPS 4
/* "tvl1" | "inv" -> the mode; anything else: SEQ_LAG1_OFF */
int seq_lag1_mode(const char *name);

struct seq_lag1 {
  nlk_ctx *ctx;
  int w, h, ch;
  const struct seq_sig *sig; /* resolved */
  const struct nlkalman_params *s1;
  int mode;                  /* SEQ_LAG1_TVL1 | SEQ_LAG1_INV */
  int of;                    /* SEQ_LAG1_TVL1: the estimator of that flow, SEQ_OF_TVL1 | SEQ_OF_BM */
  int fscale;                /* forward flow: finest scale and data weight (TVL1 only), occlusion threshold (both) */
  float dw, th;
  const struct seq_work *work; /* d_tmp, d_warp; TVL1: d_g0, d_g1; INV: d_flow, the backward flow next -> flt2_i */
  float *d_fflow, *d_focc;   /* out: the forward flow (2 * w * h) and its mask (w * h); TVL1 may use work->d_flow, d_occ */
  /* per frame: */
  const float *flt2, *next;  /* flt2_i and flt2_{i+1} | smo1_{i+1} (opponent space) */
  float *smo1;               /* out: the smoothed frame i (opponent space) */
};
/* gray of both frames -> TV-L1 flow flt2_i -> next (or the inverted backward flow) -> occlusion mask -> warp of next ->
 * SMO1(flt1 = flt2_i, smo0 = the warp). Asynchronous on the context's stream; returns the first failing call's code. */
int seq_lag1_step(const struct seq_lag1 *s);

/* ---- an opponent-space frame as output: d_tmp = its RGB copy, transformed back under vst
 * (nlk_dev_vst_inverse, mode 1) and nlf (nlk_dev_nlf_inverse). Returns the first failing call's code. */
int seq_output_rgb(nlk_ctx *ctx, float *d_tmp, const float *d_opp, int w, int h, int ch, const struct seq_sig *sig);

#endif
