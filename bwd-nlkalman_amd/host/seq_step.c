/* seq_step.c — see seq_step.h */
#include "seq_step.h"

#include <math.h>
#include <stdlib.h>
#include <string.h>

#include "cli_args.h"

/* "a b  c" -> argv {prog, a, b, c}; returns argc (the vector and its strings are never freed) */
static int seq_split(const char *prog, const char *s, const char ***argv_out) {
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

int seq_run_params(struct seq_run *r, const char *fpm_prog, const char *fpm, const char *spm_prog, const char *spm,
                   int *verbose) {
  cli_params_unset(&r->f1); cli_params_unset(&r->f2); cli_params_unset(&r->s1);
  const struct cli_option fopts[] = {
      CLI_FILTER_ROWS("f1", &r->f1),
      CLI_FILTER_ROWS("f2", &r->f2),
      {CLI_INT, 'v', "verbose", verbose, "verbose output"},
      {CLI_END, 0, NULL, NULL, NULL}};
  const struct cli_option sopts[] = {
      CLI_SMOOTHER_ROWS("s1", &r->s1),
      {CLI_INT, 'v', "verbose", verbose, "verbose output"},
      {CLI_END, 0, NULL, NULL, NULL}};
  const char **av;
  int ac = seq_split(fpm_prog, fpm, &av);
  cli_parse(fopts, fpm_prog, "filtering parameters", ac, av);
  if (spm) {
    ac = seq_split(spm_prog, spm, &av);
    cli_parse(sopts, spm_prog, "smoothing parameters", ac, av);
  }
  return r->f1.patch_sz == 0 || r->f2.patch_sz == 0;
}

int seq_parse_opm(const char *opm, struct seq_flow *bwd, struct seq_flow *fwd, int three_too) {
  const int n = sscanf(opm, "%d %f %f %d %f %f", &bwd->fscale, &bwd->dw, &bwd->th, &fwd->fscale, &fwd->dw, &fwd->th);
  if (n == 3 && three_too) *fwd = *bwd;
  return n != 6 && !(n == 3 && three_too);
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
  nlk_dev_free(C, d_est);
  if (rc != NLK_OK) return rc;
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
    nlk_dev_free(C, d_est);
    if (rc != NLK_OK) return rc;
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

int seq_run_open(struct seq_run *r, nlk_ctx *C, int w, int h, int ch, int with_smoother) {
  const size_t npix = (size_t)w * h, bytes = npix * ch * sizeof(float);
  struct seq_work *k = &r->work;
  struct seq_sure *u = &r->sure;
  r->ctx = C;
  r->w = w; r->h = h; r->ch = ch;
  memset(k, 0, sizeof *k);
  memset(&r->defects, 0, sizeof r->defects);
  memset(u, 0, sizeof *u);
  /* the work images (the last two for the smoother), the mean planes of --defect-map, the images of --sure */
  const struct { float **p; size_t bytes; int on; } want[] = {
      {&k->d_noisy, bytes, 1}, {&k->d_tmp, bytes, 1}, {&k->d_warp, bytes, 1}, {&k->d_g0, npix * 4, 1},
      {&k->d_g1, npix * 4, 1}, {&k->d_occ, npix * 4, 1}, {&k->d_flow, npix * 8, 1},
      {&k->d_fflow, npix * 8, with_smoother}, {&k->d_focc, npix * 4, with_smoother},
      {&r->defects.d_mean[0], bytes, r->opts.defect_k != 0.f}, {&r->defects.d_mean[1], bytes, r->opts.defect_k != 0.f},
      {&u->d_probe, bytes, r->opts.sure}, {&u->d_flt1, bytes, r->opts.sure}, {&u->d_flt2, bytes, r->opts.sure}};
  for (size_t i = 0; i < sizeof want / sizeof want[0]; ++i) {
    void *d = NULL;
    if (!want[i].on) continue;
    TRY(nlk_dev_alloc(C, &d, want[i].bytes));
    *want[i].p = (float *)d;
  }
  u->eps_rel = SEQ_SURE_EPS_REL;
  const char *e = getenv("NLK_SURE_EPS");
  if (e && atof(e) > 0.0) u->eps_rel = (float)atof(e);
  if ((e = getenv("NLK_SURE_SEED"))) u->seed = strtoull(e, NULL, 0);
  return NLK_OK;
}

void seq_run_close(struct seq_run *r) {
  const struct seq_work *k = &r->work;
  float *all[] = {k->d_noisy, k->d_tmp, k->d_warp, k->d_g0, k->d_g1, k->d_occ, k->d_flow, k->d_fflow, k->d_focc,
                  r->defects.d_mean[0], r->defects.d_mean[1], r->sure.d_probe, r->sure.d_flt1, r->sure.d_flt2};
  for (size_t i = 0; i < sizeof all / sizeof all[0]; ++i)
    if (all[i]) nlk_dev_free(r->ctx, all[i]);
  memset(&r->work, 0, sizeof r->work);
  memset(&r->defects, 0, sizeof r->defects);
  memset(&r->sure, 0, sizeof r->sure);
}

int seq_run_first_frame(struct seq_run *r, const float *d_rgb, FILE *report, const char *prog) {
  const int rc = seq_sig_resolve(r->ctx, &r->sig, d_rgb, r->w, r->h, r->ch, report, prog);
  if (rc != NLK_OK) return rc;
  nlkalman_default_params(&r->f1, r->sig.sigma, FLT1);
  nlkalman_default_params(&r->f2, r->sig.sigma, FLT2);
  nlkalman_default_params(&r->s1, r->sig.sigma, SMO1);
  return NLK_OK;
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

/* the flow g0 -> g1 of the run's estimator: TV-L1 at this finest scale and data weight, or block matching at this finest
 * scale (its other parameters are the defaults) */
static int seq_flow(const struct seq_run *r, float *d_flow, const float *d_g0, const float *d_g1, const struct seq_flow *f) {
  if (r->opts.of == SEQ_OF_BM) {
    struct nlk_bmflow_params bm;
    nlk_bmflow_default_params(&bm);
    bm.fscale = f->fscale < 0 ? 0 : f->fscale;
    return nlk_dev_bm_flow(r->ctx, d_flow, d_g0, d_g1, r->w, r->h, &bm);
  }
  const struct nlk_tvl1_params tv = seq_flow_params(r->w, r->h, f->fscale, f->dw);
  return nlk_dev_tvl1_flow(r->ctx, d_flow, d_g0, d_g1, r->w, r->h, &tv, NULL);
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

int seq_forward_step(struct seq_run *r, const struct seq_step *s) {
  nlk_ctx *C = r->ctx;
  const struct seq_work *k = &r->work;
  const struct seq_opts *o = &r->opts;
  const struct seq_sig *sig = &r->sig;
  const int w = r->w, h = r->h, ch = r->ch;
  const float sigma = sig->sigma;
  const size_t bytes = (size_t)w * h * ch * sizeof(float);
  if (seq_sig_vst(sig)) TRY(nlk_dev_vst_forward(C, s->d_rgb, s->d_rgb, (size_t)w * h * ch, ch, sig->vst_ab, sig->vst_s));
  if (seq_sig_nlf(sig)) TRY(nlk_dev_nlf_forward(C, s->d_rgb, s->d_rgb, (size_t)w * h * ch, ch, &sig->nlf));
  if (o->defect_k != 0.f) { /* d_noisy = the frame without the sites the mean of the frames before flags, and d_rgb too */
    const long t = r->defects.t;
    float *const *d_mean = r->defects.d_mean;
    float thr = 0.f, gain = 1.f;
    if (t > 0) TRY(nlk_defect_schedule(t, o->defect_n, o->defect_k * sigma, &thr, &gain));
    TRY(nlk_dev_defect_step(C, k->d_noisy, s->d_rgb, d_mean[(t + 1) & 1], t > 0 ? d_mean[t & 1] : NULL, NULL, NULL, w, h,
                            ch, o->defect_r, thr, gain));
    TRY(nlk_d2d(C, s->d_rgb, k->d_noisy, bytes));
    ++r->defects.t;
  }
  if (o->despike_k != 0.f) { /* d_noisy = the despiked frame, and d_rgb too: the flow's gray image is made of it */
    TRY(nlk_dev_despike(C, k->d_noisy, s->d_rgb, NULL, w, h, ch, o->despike_r, o->despike_k * sigma));
    TRY(nlk_d2d(C, s->d_rgb, k->d_noisy, bytes));
  } else {
    TRY(nlk_d2d(C, k->d_noisy, s->d_rgb, bytes));
  }
  TRY(nlk_dev_rgb2opp(C, k->d_noisy, w, h, ch));
  if (!s->prev_flt2) {
    TRY(nlk_dev_filter_frame(C, s->flt1, k->d_noisy, NULL, NULL, w, h, ch, sigma, &r->f1));
    TRY(nlk_dev_filter_frame(C, s->flt2, k->d_noisy, NULL, s->flt1, w, h, ch, sigma, &r->f2));
    return NLK_OK;
  }
  /* backward flow noisy_t -> flt2_{t-1}, occlusion mask (script lines 57-73) */
  TRY(nlk_dev_gray(C, k->d_g0, s->d_rgb, w, h, ch));
  TRY(gray_of_opp(C, k->d_g1, k->d_tmp, s->prev_flt2, w, h, ch));
  TRY(seq_flow(r, k->d_flow, k->d_g0, k->d_g1, &r->bwd));
  TRY(nlk_dev_occlusion_mask(C, k->d_occ, k->d_flow, w, h, r->bwd.th));
  TRY(nlk_dev_warp_bicubic(C, k->d_warp, s->prev_flt1, k->d_flow, k->d_occ, w, h, ch));
  TRY(nlk_dev_filter_frame(C, s->flt1, k->d_noisy, k->d_warp, NULL, w, h, ch, sigma, &r->f1));
  TRY(nlk_dev_warp_bicubic(C, k->d_warp, s->prev_flt2, k->d_flow, k->d_occ, w, h, ch));
  TRY(nlk_dev_filter_frame(C, s->flt2, k->d_noisy, k->d_warp, s->flt1, w, h, ch, sigma, &r->f2));
  return NLK_OK;
}

int seq_sure_step(const struct seq_run *r, const struct seq_step *s, long t, double *d_slot) {
  nlk_ctx *C = r->ctx;
  const struct seq_work *k = &r->work;
  const struct seq_sure *u = &r->sure;
  const int w = r->w, h = r->h, ch = r->ch;
  const float sigma = r->sig.sigma;
  const uint64_t seed = u->seed + (uint64_t)t * SEQ_SURE_FRAME_STEP;
  TRY(nlk_dev_probe_add(C, u->d_probe, k->d_noisy, (size_t)w * h * ch, u->eps_rel * sigma, seed));
  const int temporal = s->prev_flt2 != NULL;
  if (temporal) TRY(nlk_dev_warp_bicubic(C, k->d_warp, s->prev_flt1, k->d_flow, k->d_occ, w, h, ch));
  TRY(nlk_dev_filter_frame(C, u->d_flt1, u->d_probe, temporal ? k->d_warp : NULL, NULL, w, h, ch, sigma, &r->f1));
  if (temporal) TRY(nlk_dev_warp_bicubic(C, k->d_warp, s->prev_flt2, k->d_flow, k->d_occ, w, h, ch));
  TRY(nlk_dev_filter_frame(C, u->d_flt2, u->d_probe, temporal ? k->d_warp : NULL, u->d_flt1, w, h, ch, sigma, &r->f2));
  TRY(nlk_dev_sure_terms(C, d_slot, NULL, k->d_noisy, s->flt1, u->d_flt1, w, h, ch, SEQ_SURE_BLOCK, seed));
  TRY(nlk_dev_sure_terms(C, d_slot + 2 * ch, NULL, k->d_noisy, s->flt2, u->d_flt2, w, h, ch, SEQ_SURE_BLOCK, seed));
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

int seq_lag1_step(const struct seq_run *r, const struct seq_lag1 *s) {
  nlk_ctx *C = r->ctx;
  const struct seq_work *k = &r->work;
  const int w = r->w, h = r->h, ch = r->ch;
  if (s->mode == SEQ_LAG1_INV) {
    TRY(nlk_dev_flow_invert(C, s->d_fflow, k->d_flow, w, h, SEQ_LAG1_INVERT_STEPS));
  } else {
    /* forward flow flt2_i -> next, both as the flow tool reads their RGB files (script lines 90-96) */
    TRY(gray_of_opp(C, k->d_g0, k->d_tmp, s->flt2, w, h, ch));
    TRY(gray_of_opp(C, k->d_g1, k->d_tmp, s->next, w, h, ch));
    TRY(seq_flow(r, s->d_fflow, k->d_g0, k->d_g1, &r->fwd));
  }
  TRY(nlk_dev_occlusion_mask(C, s->d_focc, s->d_fflow, w, h, r->fwd.th));
  TRY(nlk_dev_warp_bicubic(C, k->d_warp, s->next, s->d_fflow, s->d_focc, w, h, ch));
  TRY(nlk_dev_smooth_frame(C, s->smo1, s->flt2, k->d_warp, NULL, w, h, ch, r->sig.sigma, &r->s1));
  return NLK_OK;
}
