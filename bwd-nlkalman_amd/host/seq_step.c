/* seq_step.c — see seq_step.h */
#include "seq_step.h"

#include <math.h>
#include <stdlib.h>
#include <string.h>

#include "cli_args.h"

int seq_split(const char *prog, const char *s, const char ***argv_out) {
  char *buf = strdup(s ? s : "");
  int n = 1, cap = 64;
  const char **av = malloc(sizeof(char *) * cap);
  av[0] = prog;
  for (char *t = strtok(buf, " \t\n"); t; t = strtok(NULL, " \t\n")) {
    if (n + 1 >= cap) av = realloc(av, sizeof(char *) * (cap *= 2));
    av[n++] = t;
  }
  *argv_out = av;
  return n;
}

void seq_parse_fpm(const char *prog, const char *fpm, struct nlkalman_params *f1, struct nlkalman_params *f2,
                   int *verbose) {
  const struct cli_option fopts[] = {
      CLI_FILTER_ROWS("f1", f1),
      CLI_FILTER_ROWS("f2", f2),
      {CLI_INT, 'v', "verbose", verbose, "verbose output"},
      {CLI_END, 0, NULL, NULL, NULL}};
  const char **av;
  const int ac = seq_split(prog, fpm, &av);
  cli_parse(fopts, prog, "filtering parameters", ac, av);
}

void seq_parse_spm(const char *prog, const char *spm, struct nlkalman_params *s1, int *verbose) {
  const struct cli_option sopts[] = {
      CLI_SMOOTHER_ROWS("s1", s1),
      {CLI_INT, 'v', "verbose", verbose, "verbose output"},
      {CLI_END, 0, NULL, NULL, NULL}};
  const char **av;
  const int ac = seq_split(prog, spm, &av);
  cli_parse(sopts, prog, "smoothing parameters", ac, av);
}

void seq_default_params(struct nlkalman_params *f1, struct nlkalman_params *f2, struct nlkalman_params *s1, float sigma) {
  nlkalman_default_params(f1, sigma, FLT1);
  nlkalman_default_params(f2, sigma, FLT2);
  nlkalman_default_params(s1, sigma, SMO1);
}

int seq_lag1_mode(const char *name) {
  if (name && !strcmp(name, "tvl1")) return SEQ_LAG1_TVL1;
  if (name && !strcmp(name, "inv")) return SEQ_LAG1_INV;
  return SEQ_LAG1_OFF;
}

#define TRY(call)                     \
  do {                                \
    const int rc_ = (call);           \
    if (rc_ != NLK_OK) return rc_;    \
  } while (0)

/* SIG = nlf: the bins of the first frame's noise curve (the estimator's defaults) as the table of nlk_nlf_build */
static int seq_sig_resolve_nlf(nlk_ctx *C, struct seq_sig *sig, const float *d_rgb, int w, int h, int ch, FILE *report,
                               const char *prog) {
  if (ch > SEQ_SIG_MAX_CH) {
    fprintf(stderr, "%s: SIG = nlf: %d channels are too many\n", prog, ch);
    return SEQ_SIG_REFUSED;
  }
  struct nlk_curve_params p;
  nlk_curve_default_params(&p);
  struct nlk_curve_bin bins[SEQ_SIG_MAX_CH * NLK_NLF_MAX_BINS];
  const size_t curve_bytes = sizeof(float) * 2 * ch, bin_bytes = sizeof(struct nlk_curve_bin) * ch * p.nbins;
  void *d_est = NULL;
  TRY(nlk_dev_alloc(C, &d_est, curve_bytes + bin_bytes));
  struct nlk_curve_bin *d_bins = (struct nlk_curve_bin *)((char *)d_est + curve_bytes);
  int rc = nlk_dev_estimate_noise_curve(C, d_est, d_bins, d_rgb, w, h, ch, &p);
  if (rc == NLK_OK) rc = nlk_d2h(C, bins, d_bins, bin_bytes);
  if (rc != NLK_OK) return rc;
  nlk_dev_free(C, d_est);
  if (nlk_nlf_build(&sig->nlf, bins, ch, p.nbins, p.lo, p.hi, NLK_NLF_RHO) != NLK_OK || !(sig->nlf.s > 0.f)) {
    int c = 0;
    while (c < ch - 1 && sig->nlf.kept[c] > 0) ++c;
    fprintf(stderr, "%s: SIG = nlf: the first frame gives no noise level for channel %d (no bin of its curve is kept)\n",
            prog, c);
    return SEQ_SIG_REFUSED;
  }
  sig->sigma = sig->nlf.s; /* the scale of the transform = the sigma of the run */
  fprintf(report, "nlf kept");
  for (int c = 0; c < ch; ++c) fprintf(report, " %d", sig->nlf.kept[c]);
  fprintf(report, " sigma %.9g\n", (double)sig->sigma);
  fflush(report);
  return NLK_OK;
}

int seq_sig_resolve(nlk_ctx *C, struct seq_sig *sig, const float *d_rgb, int w, int h, int ch, FILE *report,
                    const char *prog) {
  if (sig->mode == SEQ_SIG_NUMBER) return NLK_OK;
  if (sig->mode == SEQ_SIG_NLF) return seq_sig_resolve_nlf(C, sig, d_rgb, w, h, ch, report, prog);
  const int vst = sig->mode != SEQ_SIG_AUTO;
  if (vst && ch > SEQ_SIG_MAX_CH) {
    fprintf(stderr, "%s: SIG = vst: %d channels are too many\n", prog, ch);
    return SEQ_SIG_REFUSED;
  }
  if (sig->mode == SEQ_SIG_VST_GIVEN) {
    for (int c = 0; c < ch; ++c) { sig->vst_ab[2 * c] = sig->a; sig->vst_ab[2 * c + 1] = sig->b; }
  } else { /* the noise curve of the first frame, or its noise level (the first of 1 + ch values) */
    const size_t bytes = sizeof(float) * (vst ? 2 * ch : 1 + ch);
    void *d_est = NULL;
    TRY(nlk_dev_alloc(C, &d_est, bytes));
    int rc = vst ? nlk_dev_estimate_noise_curve(C, d_est, NULL, d_rgb, w, h, ch, NULL)
                 : nlk_dev_estimate_sigma(C, d_est, NULL, d_rgb, w, h, ch, NULL);
    if (rc == NLK_OK) rc = vst ? nlk_d2h(C, sig->vst_ab, d_est, bytes) : nlk_d2h(C, &sig->sigma, d_est, sizeof(float));
    if (rc != NLK_OK) return rc;
    nlk_dev_free(C, d_est);
  }
  if (vst) sig->sigma = sig->vst_s = nlk_vst_scale(sig->vst_ab, ch); /* the scale of the transform = the sigma of the run */
  if (!(sig->sigma > 0.f)) {
    if (vst)
      fprintf(stderr, "%s: SIG = vst: the first frame gives no noise curve (a_0 = %g, b_0 = %g)\n", prog,
              (double)sig->vst_ab[0], (double)sig->vst_ab[1]);
    else
      fprintf(stderr, "%s: SIG = auto: the first frame gives sigma = %g\n", prog, (double)sig->sigma);
    return SEQ_SIG_REFUSED;
  }
  if (vst) {
    fprintf(report, "vst");
    for (int c = 0; c < 2 * ch; ++c) fprintf(report, " %.9g", (double)sig->vst_ab[c]);
    fprintf(report, " ");
  }
  fprintf(report, "sigma %.9g\n", (double)sig->sigma);
  fflush(report);
  return NLK_OK;
}

int seq_work_alloc(nlk_ctx *C, struct seq_work *k, int w, int h, int ch, int with_smoother) {
  const size_t npix = (size_t)w * h, bytes = npix * ch * sizeof(float);
  const struct { float **p; size_t bytes; } want[] = {
      {&k->d_noisy, bytes}, {&k->d_tmp, bytes}, {&k->d_warp, bytes}, {&k->d_g0, npix * 4}, {&k->d_g1, npix * 4},
      {&k->d_occ, npix * 4}, {&k->d_flow, npix * 8}, {&k->d_fflow, npix * 8}, {&k->d_focc, npix * 4}};
  memset(k, 0, sizeof *k);
  for (int i = 0; i < (with_smoother ? 9 : 7); ++i) {
    void *d = NULL;
    TRY(nlk_dev_alloc(C, &d, want[i].bytes));
    *want[i].p = (float *)d;
  }
  return NLK_OK;
}

void seq_work_free(nlk_ctx *C, struct seq_work *k) {
  float *all[] = {k->d_noisy, k->d_tmp, k->d_warp, k->d_g0, k->d_g1, k->d_occ, k->d_flow, k->d_fflow, k->d_focc};
  for (int i = 0; i < 9; ++i)
    if (all[i]) nlk_dev_free(C, all[i]);
  memset(k, 0, sizeof *k);
}

int seq_defects_alloc(nlk_ctx *C, struct seq_defects *d, float k, int r, int n, int w, int h, int ch) {
  memset(d, 0, sizeof *d);
  d->k = k; d->r = r; d->n = n;
  for (int i = 0; i < 2; ++i) {
    void *p = NULL;
    TRY(nlk_dev_alloc(C, &p, (size_t)w * h * ch * sizeof(float)));
    d->d_mean[i] = (float *)p;
  }
  return NLK_OK;
}

void seq_defects_free(nlk_ctx *C, struct seq_defects *d) {
  for (int i = 0; i < 2; ++i)
    if (d->d_mean[i]) nlk_dev_free(C, d->d_mean[i]);
  memset(d, 0, sizeof *d);
}

/* the TV-L1 parameters of a w x h flow with this finest scale and data weight (lambda) */
static struct nlk_tvl1_params seq_flow_params(int w, int h, int fscale, float dw) {
  struct nlk_tvl1_params of;
  nlk_tvl1_default_params(&of);
  of.lambda = dw; of.fscale = fscale;
  of.nscales = nlk_tvl1_scales(w, h, of.nscales, of.zfactor);
  if (of.nscales < of.fscale) of.fscale = of.nscales;
  return of;
}

int seq_of_mode(const char *name) {
  if (name && !strcmp(name, "tvl1")) return SEQ_OF_TVL1;
  if (name && !strcmp(name, "bm")) return SEQ_OF_BM;
  return -1;
}

/* the flow g0 -> g1 of a run's estimator: TV-L1 at this finest scale and data weight, or block matching at this finest
 * scale (its other parameters are the defaults) */
static int seq_flow(nlk_ctx *C, int of, float *d_flow, const float *d_g0, const float *d_g1, int w, int h, int fscale,
                    float dw) {
  if (of == SEQ_OF_BM) {
    struct nlk_bmflow_params bm;
    nlk_bmflow_default_params(&bm);
    bm.fscale = fscale < 0 ? 0 : fscale;
    return nlk_dev_bm_flow(C, d_flow, d_g0, d_g1, w, h, &bm);
  }
  const struct nlk_tvl1_params tv = seq_flow_params(w, h, fscale, dw);
  return nlk_dev_tvl1_flow(C, d_flow, d_g0, d_g1, w, h, &tv, NULL);
}

/* the gray image of an opponent-space frame, as the flow tool reads its RGB file (d_tmp: of the frame's size) */
static int gray_of_opp(nlk_ctx *C, float *d_gray, float *d_tmp, const float *d_opp, int w, int h, int ch) {
  TRY(nlk_d2d(C, d_tmp, d_opp, (size_t)w * h * ch * sizeof(float)));
  TRY(nlk_dev_opp2rgb(C, d_tmp, w, h, ch));
  return nlk_dev_gray(C, d_gray, d_tmp, w, h, ch);
}

int seq_output_rgb(nlk_ctx *C, float *d_tmp, const float *d_opp, int w, int h, int ch, const struct seq_sig *sig) {
  const size_t n = (size_t)w * h * ch;
  TRY(nlk_d2d(C, d_tmp, d_opp, n * sizeof(float)));
  TRY(nlk_dev_opp2rgb(C, d_tmp, w, h, ch));
  if (seq_sig_vst(sig)) TRY(nlk_dev_vst_inverse(C, d_tmp, d_tmp, n, ch, sig->vst_ab, sig->vst_s, 1));
  if (seq_sig_nlf(sig)) TRY(nlk_dev_nlf_inverse(C, d_tmp, d_tmp, n, ch, &sig->nlf));
  return NLK_OK;
}

int seq_forward_step(const struct seq_step *s) {
  nlk_ctx *C = s->ctx;
  const struct seq_work *k = s->work;
  const int w = s->w, h = s->h, ch = s->ch;
  const float sigma = s->sig->sigma;
  const size_t bytes = (size_t)w * h * ch * sizeof(float);
  if (seq_sig_vst(s->sig))
    TRY(nlk_dev_vst_forward(C, s->d_rgb, s->d_rgb, (size_t)w * h * ch, ch, s->sig->vst_ab, s->sig->vst_s));
  if (seq_sig_nlf(s->sig)) TRY(nlk_dev_nlf_forward(C, s->d_rgb, s->d_rgb, (size_t)w * h * ch, ch, &s->sig->nlf));
  if (s->defects) { /* d_noisy = the frame without the sites the mean of the frames before flags, and d_rgb too */
    struct seq_defects *d = s->defects;
    float thr = 0.f, gain = 1.f;
    if (d->t > 0) TRY(nlk_defect_schedule(d->t, d->n, d->k * sigma, &thr, &gain));
    TRY(nlk_dev_defect_step(C, k->d_noisy, s->d_rgb, d->d_mean[(d->t + 1) & 1], d->t > 0 ? d->d_mean[d->t & 1] : NULL,
                            NULL, NULL, w, h, ch, d->r, thr, gain));
    TRY(nlk_d2d(C, s->d_rgb, k->d_noisy, bytes));
    ++d->t;
  }
  if (s->despike_k != 0.f) { /* d_noisy = the despiked frame, and d_rgb too: the flow's gray image is made of it */
    TRY(nlk_dev_despike(C, k->d_noisy, s->d_rgb, NULL, w, h, ch, s->despike_r, s->despike_k * sigma));
    TRY(nlk_d2d(C, s->d_rgb, k->d_noisy, bytes));
  } else {
    TRY(nlk_d2d(C, k->d_noisy, s->d_rgb, bytes));
  }
  TRY(nlk_dev_rgb2opp(C, k->d_noisy, w, h, ch));
  if (!s->prev_flt2) {
    TRY(nlk_dev_filter_frame(C, s->flt1, k->d_noisy, NULL, NULL, w, h, ch, sigma, s->f1));
    TRY(nlk_dev_filter_frame(C, s->flt2, k->d_noisy, NULL, s->flt1, w, h, ch, sigma, s->f2));
    return NLK_OK;
  }
  /* backward flow noisy_t -> flt2_{t-1}, occlusion mask (script lines 57-73) */
  TRY(nlk_dev_gray(C, k->d_g0, s->d_rgb, w, h, ch));
  TRY(gray_of_opp(C, k->d_g1, k->d_tmp, s->prev_flt2, w, h, ch));
  TRY(seq_flow(C, s->of, k->d_flow, k->d_g0, k->d_g1, w, h, s->fscale, s->dw));
  TRY(nlk_dev_occlusion_mask(C, k->d_occ, k->d_flow, w, h, s->th));
  TRY(nlk_dev_warp_bicubic(C, k->d_warp, s->prev_flt1, k->d_flow, k->d_occ, w, h, ch));
  TRY(nlk_dev_filter_frame(C, s->flt1, k->d_noisy, k->d_warp, NULL, w, h, ch, sigma, s->f1));
  TRY(nlk_dev_warp_bicubic(C, k->d_warp, s->prev_flt2, k->d_flow, k->d_occ, w, h, ch));
  TRY(nlk_dev_filter_frame(C, s->flt2, k->d_noisy, k->d_warp, s->flt1, w, h, ch, sigma, s->f2));
  return NLK_OK;
}

int seq_sure_alloc(nlk_ctx *C, struct seq_sure *u, int w, int h, int ch, int with_map) {
  const size_t bytes = (size_t)w * h * ch * sizeof(float);
  memset(u, 0, sizeof *u);
  u->eps_rel = SEQ_SURE_EPS_REL;
  u->block = SEQ_SURE_BLOCK;
  const char *e = getenv("NLK_SURE_EPS");
  if (e && atof(e) > 0.0) u->eps_rel = (float)atof(e);
  if ((e = getenv("NLK_SURE_SEED"))) u->seed = strtoull(e, NULL, 0);
  float **want[] = {&u->d_probe, &u->d_flt1, &u->d_flt2};
  for (int i = 0; i < 3; ++i) {
    void *d = NULL;
    TRY(nlk_dev_alloc(C, &d, bytes));
    *want[i] = (float *)d;
  }
  if (with_map) {
    const size_t nbx = (w + u->block - 1) / u->block, nby = (h + u->block - 1) / u->block;
    void *d = NULL;
    TRY(nlk_dev_alloc(C, &d, nbx * nby * ch * 2 * sizeof(double)));
    u->d_blocks = (double *)d;
  }
  return NLK_OK;
}

void seq_sure_free(nlk_ctx *C, struct seq_sure *u) {
  void *all[] = {u->d_probe, u->d_flt1, u->d_flt2, u->d_blocks};
  for (int i = 0; i < 4; ++i)
    if (all[i]) nlk_dev_free(C, all[i]);
  u->d_probe = u->d_flt1 = u->d_flt2 = NULL;
  u->d_blocks = NULL;
}

int seq_sure_step(const struct seq_step *s, const struct seq_sure *u, long t, double *d_slot) {
  nlk_ctx *C = s->ctx;
  const struct seq_work *k = s->work;
  const int w = s->w, h = s->h, ch = s->ch;
  const float sigma = s->sig->sigma;
  const uint64_t seed = u->seed + (uint64_t)t * SEQ_SURE_FRAME_STEP;
  TRY(nlk_dev_probe_add(C, u->d_probe, k->d_noisy, (size_t)w * h * ch, u->eps_rel * sigma, seed));
  const int temporal = s->prev_flt2 != NULL;
  if (temporal) TRY(nlk_dev_warp_bicubic(C, k->d_warp, s->prev_flt1, k->d_flow, k->d_occ, w, h, ch));
  TRY(nlk_dev_filter_frame(C, u->d_flt1, u->d_probe, temporal ? k->d_warp : NULL, NULL, w, h, ch, sigma, s->f1));
  if (temporal) TRY(nlk_dev_warp_bicubic(C, k->d_warp, s->prev_flt2, k->d_flow, k->d_occ, w, h, ch));
  TRY(nlk_dev_filter_frame(C, u->d_flt2, u->d_probe, temporal ? k->d_warp : NULL, u->d_flt1, w, h, ch, sigma, s->f2));
  TRY(nlk_dev_sure_terms(C, d_slot, NULL, k->d_noisy, s->flt1, u->d_flt1, w, h, ch, u->block, seed));
  TRY(nlk_dev_sure_terms(C, d_slot + 2 * ch, u->d_blocks, k->d_noisy, s->flt2, u->d_flt2, w, h, ch, u->block, seed));
  return NLK_OK;
}

struct seq_sure_est seq_sure_estimate(const double *terms, int w, int h, int ch, float sigma, float eps_rel) {
  double R = 0.0, D = 0.0;
  for (int c = 0; c < ch; ++c) { R += terms[2 * c]; D += terms[2 * c + 1]; }
  const double n = (double)w * h * ch, eps = (double)(eps_rel * sigma);
  struct seq_sure_est e;
  e.mse = nlk_sure_mse(R, D, n, (double)sigma, eps);
  e.psnr = 10.0 * log10(255.0 * 255.0 / e.mse); /* (NaN for an estimate that is not positive) */
  e.resid = R / n;
  e.div = D / (eps * n);
  return e;
}

int seq_lag1_step(const struct seq_lag1 *s) {
  nlk_ctx *C = s->ctx;
  const struct seq_work *k = s->work;
  const int w = s->w, h = s->h, ch = s->ch;
  if (s->mode == SEQ_LAG1_INV) {
    TRY(nlk_dev_flow_invert(C, s->d_fflow, k->d_flow, w, h, SEQ_LAG1_INVERT_STEPS));
  } else {
    /* forward flow flt2_i -> next, both as the flow tool reads their RGB files (script lines 90-96) */
    TRY(gray_of_opp(C, k->d_g0, k->d_tmp, s->flt2, w, h, ch));
    TRY(gray_of_opp(C, k->d_g1, k->d_tmp, s->next, w, h, ch));
    TRY(seq_flow(C, s->of, s->d_fflow, k->d_g0, k->d_g1, w, h, s->fscale, s->dw));
  }
  TRY(nlk_dev_occlusion_mask(C, s->d_focc, s->d_fflow, w, h, s->th));
  TRY(nlk_dev_warp_bicubic(C, k->d_warp, s->next, s->d_fflow, s->d_focc, w, h, ch));
  TRY(nlk_dev_smooth_frame(C, s->smo1, s->flt2, k->d_warp, NULL, w, h, ch, s->sig->sigma, s->s1));
  return NLK_OK;
}
