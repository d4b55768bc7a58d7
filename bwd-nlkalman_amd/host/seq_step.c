/* seq_step.c — see seq_step.h */
#include "seq_step.h"

#include <stdlib.h>
#include <string.h>

#include "cli_args.h"

void seq_unset_params(struct nlkalman_params *p) {
  p->patch_sz = p->search_sz_x = p->search_sz_t = -1;
  p->npatches_x = p->npatches_t = p->npatches_tagg = -1;
  p->dista_lambda = p->beta_x = p->beta_t = -1.f;
}

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
      {CLI_INT, 0, "f1_p", &f1->patch_sz, "patch size"},
      {CLI_INT, 0, "f1_sx", &f1->search_sz_x, "search radius (spatial filtering)"},
      {CLI_INT, 0, "f1_st", &f1->search_sz_t, "search radius (temporal filtering)"},
      {CLI_INT, 0, "f1_nx", &f1->npatches_x, "number of similar patches spatial"},
      {CLI_INT, 0, "f1_nt", &f1->npatches_t, "number of similar patches kalman"},
      {CLI_INT, 0, "f1_nt_agg", &f1->npatches_tagg, "number of similar patches kalman spatial average"},
      {CLI_FLOAT, 0, "f1_bx", &f1->beta_x, "noise multiplier in spatial filtering"},
      {CLI_FLOAT, 0, "f1_bt", &f1->beta_t, "noise multiplier in kalman filtering"},
      {CLI_FLOAT, 0, "f1_l", &f1->dista_lambda, "noisy patch weight in patch distance"},
      {CLI_INT, 0, "f2_p", &f2->patch_sz, "patch size"},
      {CLI_INT, 0, "f2_sx", &f2->search_sz_x, "search radius (spatial filtering)"},
      {CLI_INT, 0, "f2_st", &f2->search_sz_t, "search radius (temporal filtering)"},
      {CLI_INT, 0, "f2_nx", &f2->npatches_x, "number of similar patches spatial"},
      {CLI_INT, 0, "f2_nt", &f2->npatches_t, "number of similar patches kalman"},
      {CLI_INT, 0, "f2_nt_agg", &f2->npatches_tagg, "number of similar patches kalman spatial average"},
      {CLI_FLOAT, 0, "f2_bx", &f2->beta_x, "noise multiplier in spatial filtering"},
      {CLI_FLOAT, 0, "f2_bt", &f2->beta_t, "noise multiplier in kalman filtering"},
      {CLI_FLOAT, 0, "f2_l", &f2->dista_lambda, "noisy patch weight in patch distance"},
      {CLI_INT, 'v', "verbose", verbose, "verbose output"},
      {CLI_END, 0, NULL, NULL, NULL}};
  const char **av;
  const int ac = seq_split(prog, fpm, &av);
  cli_parse(fopts, prog, "filtering parameters", ac, av);
}

void seq_parse_spm(const char *prog, const char *spm, struct nlkalman_params *s1, int *verbose) {
  const struct cli_option sopts[] = {
      {CLI_INT, 0, "s1_p", &s1->patch_sz, "patch size"},
      {CLI_INT, 0, "s1_st", &s1->search_sz_t, "search region radius"},
      {CLI_INT, 0, "s1_nt", &s1->npatches_t, "number of similar patches kalman"},
      {CLI_INT, 0, "s1_nt_agg", &s1->npatches_tagg, "number of similar patches kalman spatial average"},
      {CLI_FLOAT, 0, "s1_bt", &s1->beta_t, "noise multiplier in kalman filtering"},
      {CLI_FLOAT, 0, "s1_l", &s1->dista_lambda, "noisy patch weight in patch distance"},
      {CLI_INT, 'v', "verbose", verbose, "verbose output"},
      {CLI_END, 0, NULL, NULL, NULL}};
  const char **av;
  const int ac = seq_split(prog, spm, &av);
  cli_parse(sopts, prog, "smoothing parameters", ac, av);
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

int seq_forward_step(const struct seq_step *s) {
  nlk_ctx *C = s->ctx;
  const int w = s->w, h = s->h, ch = s->ch;
  const size_t bytes = (size_t)w * h * ch * sizeof(float);
  if (s->vst_ab) TRY(nlk_dev_vst_forward(C, s->d_rgb, s->d_rgb, (size_t)w * h * ch, ch, s->vst_ab, s->vst_s));
  TRY(nlk_d2d(C, s->d_noisy, s->d_rgb, bytes));
  TRY(nlk_dev_rgb2opp(C, s->d_noisy, w, h, ch));
  if (!s->prev_flt2) {
    TRY(nlk_dev_filter_frame(C, s->flt1, s->d_noisy, NULL, NULL, w, h, ch, s->sigma, s->f1));
    TRY(nlk_dev_filter_frame(C, s->flt2, s->d_noisy, NULL, s->flt1, w, h, ch, s->sigma, s->f2));
    return NLK_OK;
  }
  /* backward flow noisy_t -> flt2_{t-1}, occlusion mask (script lines 57-73) */
  struct nlk_tvl1_params of;
  nlk_tvl1_default_params(&of);
  of.lambda = s->dw; of.fscale = s->fscale;
  of.nscales = nlk_tvl1_scales(w, h, of.nscales, of.zfactor);
  if (of.nscales < of.fscale) of.fscale = of.nscales;
  TRY(nlk_dev_gray(C, s->d_g0, s->d_rgb, w, h, ch));
  TRY(nlk_d2d(C, s->d_tmp, s->prev_flt2, bytes));
  TRY(nlk_dev_opp2rgb(C, s->d_tmp, w, h, ch));
  TRY(nlk_dev_gray(C, s->d_g1, s->d_tmp, w, h, ch));
  TRY(nlk_dev_tvl1_flow(C, s->d_flow, s->d_g0, s->d_g1, w, h, &of, NULL));
  TRY(nlk_dev_occlusion_mask(C, s->d_occ, s->d_flow, w, h, s->th));
  TRY(nlk_dev_warp_bicubic(C, s->d_warp, s->prev_flt1, s->d_flow, s->d_occ, w, h, ch));
  TRY(nlk_dev_filter_frame(C, s->flt1, s->d_noisy, s->d_warp, NULL, w, h, ch, s->sigma, s->f1));
  TRY(nlk_dev_warp_bicubic(C, s->d_warp, s->prev_flt2, s->d_flow, s->d_occ, w, h, ch));
  TRY(nlk_dev_filter_frame(C, s->flt2, s->d_noisy, s->d_warp, s->flt1, w, h, ch, s->sigma, s->f2));
  return NLK_OK;
}

int seq_lag1_step(const struct seq_lag1 *s) {
  nlk_ctx *C = s->ctx;
  const int w = s->w, h = s->h, ch = s->ch;
  const size_t bytes = (size_t)w * h * ch * sizeof(float);
  if (s->mode == SEQ_LAG1_INV) {
    TRY(nlk_dev_flow_invert(C, s->d_fflow, s->d_bflow, w, h, SEQ_LAG1_INVERT_STEPS));
  } else {
    /* forward flow flt2_{i-1} -> flt2_i, both as the flow tool reads their RGB files (script lines 90-96) */
    struct nlk_tvl1_params of;
    nlk_tvl1_default_params(&of);
    of.lambda = s->dw; of.fscale = s->fscale;
    of.nscales = nlk_tvl1_scales(w, h, of.nscales, of.zfactor);
    if (of.nscales < of.fscale) of.fscale = of.nscales;
    TRY(nlk_d2d(C, s->d_tmp, s->prev_flt2, bytes));
    TRY(nlk_dev_opp2rgb(C, s->d_tmp, w, h, ch));
    TRY(nlk_dev_gray(C, s->d_g0, s->d_tmp, w, h, ch));
    TRY(nlk_d2d(C, s->d_tmp, s->cur_flt2, bytes));
    TRY(nlk_dev_opp2rgb(C, s->d_tmp, w, h, ch));
    TRY(nlk_dev_gray(C, s->d_g1, s->d_tmp, w, h, ch));
    TRY(nlk_dev_tvl1_flow(C, s->d_fflow, s->d_g0, s->d_g1, w, h, &of, NULL));
  }
  TRY(nlk_dev_occlusion_mask(C, s->d_focc, s->d_fflow, w, h, s->th));
  TRY(nlk_dev_warp_bicubic(C, s->d_warp, s->cur_flt2, s->d_fflow, s->d_focc, w, h, ch));
  TRY(nlk_dev_smooth_frame(C, s->lsm1, s->prev_flt2, s->d_warp, NULL, w, h, ch, s->sigma, s->s1));
  return NLK_OK;
}
