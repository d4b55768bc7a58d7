/* nlf_build.c — nlk_nlf_build (include/nlk_hip.h): the table of the noise-level-function transform from the bins of
 * nlk_dev_estimate_noise_curve. Host only, double arithmetic, plain C: nothing of the device libraries is needed to
 * link it (libnlk_hip.so links it in and exports it). The steps a-g are those of the header. */
#include <math.h>
#include <string.h>

#include "nlk_hip.h"

/* g at s = 1: the piecewise-linear map through (x_j, g_j) with the slopes kappa_j, its end segments extended */
static double g_at(double y, const double *x, const double *g, const double *kappa, int nbins, double lo, double hi) {
  double t = (y - lo) / (hi - lo) * nbins;
  if (!(t > 0.0)) t = 0.0;
  if (t > nbins - 1) t = nbins - 1;
  const int j = (int)floor(t);
  return g[j] + kappa[j] * (y - x[j]);
}

int nlk_nlf_build(struct nlk_nlf_table *t, const struct nlk_curve_bin *bins, int ch, int nbins, float lo_, float hi_,
                  float rho_) {
  if (!t || !bins || ch < 1 || ch > NLK_NLF_MAX_CH || nbins < 1 || nbins > NLK_NLF_MAX_BINS) return NLK_EINVAL;
  if (!(hi_ > lo_) || !(hi_ <= 3.402823466e38f) || !(lo_ >= -3.402823466e38f)) return NLK_EINVAL;
  if (!(rho_ > 0.f && rho_ <= 1.f)) return NLK_EINVAL;
  const double lo = lo_, hi = hi_, rho = rho_, dx = (hi - lo) / nbins;
  enum { NB = NLK_NLF_MAX_BINS };
  static const double nan_ = NAN;
  double x[NB + 1], g[NLK_NLF_MAX_CH][NB + 1], kappa[NLK_NLF_MAX_CH][NB], g0[NLK_NLF_MAX_CH], span = 0.0;
  int valid = 1;
  memset(t, 0, sizeof *t);
  t->ch = ch; t->nbins = nbins; t->lo = lo_; t->hi = hi_;
  t->inv_dx = (float)(nbins / (hi - lo));
  for (int j = 0; j <= nbins; ++j) t->x[j] = (float)(x[j] = lo + j * dx);
  for (int c = 0; c < ch; ++c) {
    /* a. the bins kept */
    double n[NB], m[NB], v[NB], vs[NB], sorted[NB], sig[NB + 1];
    int nk = 0;
    for (int q = 0; q < nbins; ++q) {
      const struct nlk_curve_bin *b = bins + (size_t)c * nbins + q;
      if (b->nsel > 0 && b->var > 0.f && b->var <= 3.402823466e38f) { n[nk] = b->nsel; m[nk] = b->mean; v[nk] = b->var; ++nk; }
    }
    t->kept[c] = nk;
    if (nk == 0) {
      valid = 0;
      for (int j = 0; j <= nbins; ++j) t->sigma[c][j] = (float)nan_;
      continue;
    }
    /* b. smoothing over the neighbours in K */
    for (int k = 0; k < nk; ++k) {
      double num = 2.0 * n[k] * v[k], den = 2.0 * n[k];
      if (k > 0) { num += n[k - 1] * v[k - 1]; den += n[k - 1]; }
      if (k + 1 < nk) { num += n[k + 1] * v[k + 1]; den += n[k + 1]; }
      vs[k] = num / den;
    }
    /* c. the floor, rho^2 times the median */
    memcpy(sorted, vs, sizeof(double) * nk);
    for (int i = 1; i < nk; ++i) { /* (at most 64 values: insertion sort) */
      const double key = sorted[i];
      int j = i;
      for (; j > 0 && sorted[j - 1] > key; --j) sorted[j] = sorted[j - 1];
      sorted[j] = key;
    }
    const double med = nk & 1 ? sorted[nk / 2] : 0.5 * (sorted[nk / 2 - 1] + sorted[nk / 2]);
    for (int k = 0; k < nk; ++k)
      if (vs[k] < rho * rho * med) vs[k] = rho * rho * med;
    /* d. the deviation at the knots */
    for (int j = 0, k = 0; j <= nbins; ++j) {
      double vj;
      if (x[j] <= m[0]) vj = vs[0];
      else if (x[j] >= m[nk - 1]) vj = vs[nk - 1];
      else {
        while (k + 2 < nk && m[k + 1] <= x[j]) ++k; /* m_k <= x_j < m_{k+1} (the knots increase: k only moves up) */
        vj = vs[k] + (x[j] - m[k]) / (m[k + 1] - m[k]) * (vs[k + 1] - vs[k]);
      }
      sig[j] = sqrt(vj);
      t->sigma[c][j] = (float)sig[j];
    }
    /* e. the slopes and the map at s = 1 */
    g[c][0] = 0.0;
    for (int j = 0; j < nbins; ++j) {
      kappa[c][j] = 2.0 / (sig[j] + sig[j + 1]);
      g[c][j + 1] = g[c][j] + kappa[c][j] * (x[j + 1] - x[j]);
    }
    g0[c] = g_at(0.0, x, g[c], kappa[c], nbins, lo, hi);
    span += g_at(255.0, x, g[c], kappa[c], nbins, lo, hi) - g0[c];
  }
  /* f. the scale */
  const double s = valid ? 255.0 / (span / ch) : nan_;
  t->s = (float)s;
  /* g. the float tables */
  for (int c = 0; c < ch; ++c)
    for (int j = 0; j <= nbins; ++j) {
      t->G[c][j] = valid ? (float)(s * (g[c][j] - g0[c])) : (float)nan_;
      if (j < nbins) {
        t->slope[c][j] = valid ? (float)(s * kappa[c][j]) : (float)nan_;
        t->islope[c][j] = valid ? (float)(1.0 / (s * kappa[c][j])) : (float)nan_;
      }
    }
  return NLK_OK;
}
