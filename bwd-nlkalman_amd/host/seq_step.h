/* seq_step.h — what `nlkalman-seq`, `nlkalman-seq-gt`, `nlkalman-lsmo-seq` (host/main_seq.c) and `nlkalman-y4m`
 * (host/main_y4m.c) share, each stated once: the SIG argument and the options of all four tools (their grammar and
 * their one reader in host/seq_args.c, which links by itself), the FPM, SPM and OPM strings, and the run (struct
 * seq_run: options, SIG, parameters, flow settings, work images and the state of --defect-map and --sure) with its
 * steps: the first frame, one step of the forward recursion, its error estimate, one smoother step (the lag-1
 * smoother's, and the whole-sequence backward pass's) and the way an opponent-space frame becomes an output frame, on
 * device-resident frames through the device C-ABI. A new option is a field of seq_opts, a row of the reader's table
 * and what the step does with it; the two mains carry nothing per option. */
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

/* ---- the options all four tools share: --of tvl1|bm, --despike K[,R], --defect-map K[,R[,N]], --sure. All zeros: the
 * run without any of them */
struct seq_opts {
  int of;           /* SEQ_OF_TVL1 | SEQ_OF_BM */
  float despike_k;  /* 0: off; else every noisy frame is despiked at thr = despike_k * sigma ... */
  int despike_r;    /* ... and this ring radius (1 or 2) */
  float defect_k;   /* 0: off; else the defect map of the run, its threshold in sigma ... */
  int defect_r, defect_n; /* ... its ring radius (1 or 2) and window */
  int sure;         /* the error estimate of every forward step */
};
/* One reader (host/seq_args.c: a table of one row per option, in the order above). argv[at] against the rows
 * *from .. (from == NULL: every row): 0 when at >= argc or it names none of them, else the number of entries read
 * (1: a flag, 2: an option and its value), *o set and *from = the row after the one that matched, so that a tool which
 * passes the same `from` again admits the options once each, in the table's order (main_seq.c), and a tool that passes
 * NULL in any order (main_y4m.c). A value that is missing or refused: the option's SEQ_*_WANT line under `prog` on
 * stderr (a missing value as ""), -1, *o and *from as they were. */
int seq_opts_read(struct seq_opts *o, int argc, const char **argv, int at, int *from, const char *prog);
/* what seq_opts_read would read at this name: 0 (not a shared option), 1 or 2 */
int seq_opts_arity(const char *name);

/* ---- the run: what every step of it needs, stated once. A tool fills opts (seq_opts_read), sig (seq_sig_parse), the
 * parameters (seq_run_params) and the flow settings (seq_parse_opm), opens the run when the frame size is known, calls
 * seq_run_first_frame on the first frame and then the steps. */
struct seq_flow { /* of one flow: finest scale, data weight (lambda; TV-L1 only) and occlusion threshold */
  int fscale;
  float dw, th;
};
struct seq_work { /* the work images */
  float *d_noisy, *d_tmp, *d_warp; /* of the frame's size ... */
  float *d_g0, *d_g1, *d_occ;      /* ... of w * h floats ... */
  float *d_flow;                   /* ... and of 2 * w * h: after a forward step d_flow and d_occ hold its flow and mask */
  float *d_fflow, *d_focc;         /* with_smoother only: the lag-1 smoother's flow (2 * w * h) and mask (w * h) */
};
struct seq_sure { /* --sure */
  float eps_rel;  /* eps = eps_rel * sigma */
  uint64_t seed;
  float *d_probe, *d_flt1, *d_flt2; /* of the frame's size: the perturbed frame and its two estimates */
};
struct seq_run {
  nlk_ctx *ctx;
  int w, h, ch;
  struct seq_opts opts;
  struct seq_sig sig;                /* resolved by seq_run_first_frame */
  struct nlkalman_params f1, f2, s1; /* as seq_run_params left them until seq_run_first_frame fills the defaults in */
  struct seq_flow bwd, fwd;          /* the backward flow of a forward step, the forward flow of a smoother step */
  struct seq_work work;
  struct { long t; float *d_mean[2]; } defects; /* --defect-map: the index of the next frame, the two mean planes (of
                                                    the frame's size; the steps swap them) */
  struct seq_sure sure;
};
/* FPM and SPM: every field as cli_params_unset leaves it (host/cli_args.h), then FPM, the options of nlkalman-flt
 * (--f1_p ... --f2_l ..., -v) as one string, into f1, f2 and *verbose, and with spm != NULL SPM, the options of
 * nlkalman-smo (--s1_p ..., -v), into s1 and *verbose; either exits with the parser's message under its `prog` on an
 * unknown option, as nlkalman-flt does (the two `prog` strings are kept). Returns 1 when a filtering iteration is
 * switched off (f1_p or f2_p == 0: both are needed; the caller prints its line), else 0. */
int seq_run_params(struct seq_run *r, const char *fpm_prog, const char *fpm, const char *spm_prog, const char *spm,
                   int *verbose);
/* OPM: "FSCALE1 DW1 TH1 FSCALE2 DW2 TH2" into bwd and fwd; three_too: "FSCALE DW TH" alone sets both. Returns 1 for
 * any other count of numbers (the caller prints its line), else 0. */
int seq_parse_opm(const char *opm, struct seq_flow *bwd, struct seq_flow *fwd, int three_too);
/* ctx, the frame size, and one device allocation per work image (with_smoother: d_fflow and d_focc too); with
 * opts.defect_k != 0 the two mean planes, with opts.sure the three images of the probe and eps_rel, seed = the defaults
 * below (NLK_SURE_EPS, > 0, and NLK_SURE_SEED, strtoull in any base, override). Nothing is allocated for an option that
 * is off. Returns the first failing call's code (what was allocated stays for seq_run_close). */
int seq_run_open(struct seq_run *r, nlk_ctx *ctx, int w, int h, int ch, int with_smoother);
/* the first frame, on the device as pushed: seq_sig_resolve, then every parameter not given becomes the default of its
 * stage at the run's sigma. Returns what seq_sig_resolve returns. */
int seq_run_first_frame(struct seq_run *r, const float *d_rgb, FILE *report, const char *prog);
void seq_run_close(struct seq_run *r);

/* ---- one step of the forward recursion: what differs per frame */
struct seq_step {
  float *d_rgb;              /* the noisy RGB frame; under vst and nlf it is transformed in place, and despiked likewise */
  const float *prev_flt1, *prev_flt2; /* the previous frame's outputs (opponent space); both NULL on the first frame */
  float *flt1, *flt2;        /* out: this frame's (opponent space) */
};
/* variance stabilisation, then with opts.defect_k != 0 the step of the defect map (in the domain where the run's sigma
 * holds: nlk_dev_defect_step reads d_rgb and the mean of the frames before, writes work.d_noisy and the other mean plane,
 * then a copy back to d_rgb; defects.t advances), then with opts.despike_k != 0 the defective-pixel filter (in the same
 * domain, before rgb2opp and the flow's gray image: nlk_dev_despike into work.d_noisy, which is free at that point, and
 * a copy back to d_rgb); with either off nothing of it is launched. Then rgb2opp, FLT1 and FLT2: spatial on the first
 * frame, afterwards gray -> flow (TV-L1, or under SEQ_OF_BM block matching; bwd) noisy_t -> flt2_{t-1} -> occlusion mask
 * -> warp + FLT1 -> warp + FLT2 (scripts/nlkalman-seq.sh:39-101).
 * Asynchronous on the context's stream; returns the first failing call's code (nlk_last_error has the message). */
int seq_forward_step(struct seq_run *r, const struct seq_step *s);

/* ---- the error estimate of a forward step without clean frames: Monte-Carlo SURE (include/nlk_hip.h: nlk_dev_probe_add,
 * nlk_dev_sure_terms). The noise of frame t is independent of everything before it, so the estimate holds
 * for the recursion's frame t with the previous outputs held fixed; it costs one more FLT1 and FLT2, on a perturbed
 * frame. Under vst / nlf the estimate is in the stabilised domain, at the run's sigma. With despike_k != 0 the probe goes
 * on the frame the filter saw, the despiked one (work->d_noisy): the estimate treats the despiked frame as the data. */
#define SEQ_SURE_EPS_REL 0.05f /* the probe, in units of sigma: the middle of the plateau 0.025 .. 0.1 of DESIGN.md §9's table */
#define SEQ_SURE_BLOCK 16      /* the tile of nlk_dev_sure_terms */
#define SEQ_SURE_FRAME_STEP 0xD1B54A32D192ED03ull /* the seed of frame t = seed + t * this (mod 2^64) */
/* (a run opened with opts.sure) after seq_forward_step(r, s) of frame t (t = 0: the first), while work.d_noisy, d_flow and
 * d_occ still hold that step's values: the probe on d_noisy, the two warps again when there is a previous frame, FLT1',
 * then FLT2' with FLT1' as its basic estimate, and the terms of flt1 into d_slot[0 .. 2 ch), those of flt2 into
 * d_slot[2 ch .. 4 ch) (device doubles, R_c and D_c interleaved). Writes the images of r->sure and work.d_warp, nothing
 * else: s->flt1, s->flt2 and what a following seq_lag1_step reads stay as they are. Asynchronous on the context's
 * stream; returns the first failing call's code. */
int seq_sure_step(const struct seq_run *r, const struct seq_step *s, long t, double *d_slot);
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

struct seq_lag1 { /* what differs per step */
  int mode;                  /* SEQ_LAG1_TVL1 (the run's estimator at fwd's scale and data weight) | SEQ_LAG1_INV (of
                                work.d_flow, the backward flow next -> flt2_i) */
  float *d_fflow, *d_focc;   /* out: the forward flow (2 * w * h) and its mask (w * h); TVL1 may use work.d_flow, d_occ */
  const float *flt2, *next;  /* flt2_i and flt2_{i+1} | smo1_{i+1} (opponent space) */
  float *smo1;               /* out: the smoothed frame i (opponent space) */
};
/* gray of both frames -> flow flt2_i -> next (or the inverted backward flow) -> occlusion mask (fwd's threshold) -> warp
 * of next -> SMO1(flt1 = flt2_i, smo0 = the warp) on work.d_tmp, d_warp, d_g0, d_g1. Asynchronous on the context's stream;
 * returns the first failing call's code. */
int seq_lag1_step(const struct seq_run *r, const struct seq_lag1 *s);

/* ---- an opponent-space frame as output: d_tmp = its RGB copy, transformed back under vst
 * (nlk_dev_vst_inverse, mode 1) and nlf (nlk_dev_nlf_inverse). Returns the first failing call's code. */
int seq_output_rgb(nlk_ctx *ctx, float *d_tmp, const float *d_opp, int w, int h, int ch, const struct seq_sig *sig);

#endif
