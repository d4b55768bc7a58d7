// tu_sigma.hip — the noise-level and the noise-curve estimator's entry points of include/nlk_hip.h (kernels: k_sigma.h)
#include "k_sigma.h"
#include "nlk_internal.h"

#include <math.h>

static_assert(sizeof(NlkCurveBin) == sizeof(struct nlk_curve_bin), "k_curve_final writes struct nlk_curve_bin");

namespace {

// what both estimators derive from the sizes alone
struct SigShape {
  int nbx, nby;
  size_t n;       // blocks per channel
  size_t groups;  // pass 2 and 3: workgroups per channel ...
  size_t share;   // ... and keys per workgroup
  dim3 grid1;     // pass 1
  size_t tile;    // bytes of its LDS tile, 0: the blocks come straight from the image
};

int sig_check(nlk_ctx* c, const char* who, int w, int h, int step, float frac, int low_max, int high_min) {
  if (w < 8 || h < 8) return fail(c, NLK_EINVAL, "%s: a %d x %d image holds no 8 x 8 block", who, w, h);
  if (step < 1) return fail(c, NLK_EINVAL, "%s: step = %d, must be at least 1", who, step);
  if (!(frac > 0.f && frac <= 1.f)) return fail(c, NLK_EINVAL, "%s: frac = %g, must be in (0, 1]", who, (double)frac);
  if (low_max < 1 || low_max > 14 || high_min < 1 || high_min > 14)
    return fail(c, NLK_EINVAL, "%s: low_max = %d, high_min = %d, must be in 1..14", who, low_max, high_min);
  return NLK_OK;
}

int sig_shape(nlk_ctx* c, const char* who, SigShape* s, int w, int h, int ch, int step, size_t max_groups) {
  s->nbx = (w - 8) / step + 1;
  s->nby = (h - 8) / step + 1;
  s->n = (size_t)s->nbx * s->nby;
  if (s->n > 0x7fffffffull) return fail(c, NLK_EINVAL, "%s: %zu blocks per channel are too many", who, s->n);
  s->groups = (s->n + 2047) / 2048;
  if (s->groups > max_groups) s->groups = max_groups;
  s->share = ((s->n + s->groups - 1) / s->groups + NLK_SIG_SUM_THREADS - 1) / NLK_SIG_SUM_THREADS * NLK_SIG_SUM_THREADS;
  s->groups = (s->n + s->share - 1) / s->share;
  s->grid1 = dim3((s->nbx + NLK_SIG_TBX - 1) / NLK_SIG_TBX, (s->nby + NLK_SIG_TBY - 1) / NLK_SIG_TBY, ch);
  s->tile = step <= 8 ? (size_t)nlk_sig_pitch(step) * nlk_sig_tile_h(step) * sizeof(float) : 0;
  if (s->tile > NLK_SIG_LDS_MAX) s->tile = 0;
  return NLK_OK;
}

// pass 2: the K-th key of every slot, a digit per level; hist(level) launches the estimator's k_*_hist
template <class Hist>
int sig_select(nlk_ctx* c, NlkSigState* state, const uint32_t* hist_buf, dim3 slots, float frac, int kmin, int nmin,
               Hist hist) {
  for (int level = 0; level < 4; ++level) {
    if (level > 0) {
      hist(level);
      HIPCHK(c, hipGetLastError());
    }
    hipLaunchKernelGGL(k_sigma_pick, slots, dim3(NLK_SIG_THREADS), 0, c->stream, state, hist_buf, level, frac, kmin,
                       nmin);
    HIPCHK(c, hipGetLastError());
  }
  return NLK_OK;
}

}  // namespace

extern "C" {

void nlk_sigma_default_params(struct nlk_sigma_params* p) {
  if (!p) return;
  p->step = 4;
  p->frac = 0.05f;
  p->kmin = 64;
  p->low_max = 5;
  p->high_min = 8;
}

int nlk_dev_estimate_sigma(nlk_ctx* c, float* d_sigma, int* d_counts, const float* d_img, int w, int h, int ch,
                           const struct nlk_sigma_params* prms) {
  const char* who = "nlk_dev_estimate_sigma";
  if (!c || !d_sigma || !d_img || ch < 1 || ch > 65535) return fail(c, NLK_EINVAL, "%s: bad argument", who);
  struct nlk_sigma_params p;
  nlk_sigma_default_params(&p);
  if (prms) p = *prms;
  SigShape s;
  int rc = sig_check(c, who, w, h, p.step, p.frac, p.low_max, p.high_min);
  if (!rc) rc = sig_shape(c, who, &s, w, h, ch, p.step, NLK_SIG_MAX_GROUPS);
  if (rc) return rc;
  const size_t n = s.n, groups = s.groups;
  NLK_USE_DEVICE(c);

  // scratch, grown on demand and kept: histograms [ch][4][256] | state [ch] | counts [ch][groups] | partials
  // [ch][groups][64] | keys [ch][n]
  const size_t o_state = (size_t)ch * 1024 * sizeof(uint32_t);
  const size_t o_count = o_state + (size_t)ch * sizeof(NlkSigState);
  const size_t o_part = (o_count + (size_t)ch * groups * sizeof(int) + 7) & ~(size_t)7;
  const size_t o_keys = o_part + (size_t)ch * groups * 64 * sizeof(double);
  rc = reserve(c, c->sig, o_keys + (size_t)ch * n * sizeof(uint32_t));
  if (rc) return rc;
  char* base = (char*)c->sig.p;
  uint32_t* hist = (uint32_t*)base;
  NlkSigState* state = (NlkSigState*)(base + o_state);
  int* count = (int*)(base + o_count);
  double* part = (double*)(base + o_part);
  uint32_t* keys = (uint32_t*)(base + o_keys);
  HIPCHK(c, hipMemsetAsync(hist, 0, o_state, c->stream));

  // pass 1
  if (s.grid1.y > 65535) return fail(c, NLK_EINVAL, "%s: %d block rows are too many", who, s.nby);
  if (s.tile)
    hipLaunchKernelGGL(k_sigma_keys<true>, s.grid1, dim3(NLK_SIG_THREADS), s.tile, c->stream, keys, hist, d_img, w, h,
                       ch, p.step, s.nbx, s.nby, p.low_max);
  else
    hipLaunchKernelGGL(k_sigma_keys<false>, s.grid1, dim3(NLK_SIG_THREADS), 0, c->stream, keys, hist, d_img, w, h, ch,
                       p.step, s.nbx, s.nby, p.low_max);
  HIPCHK(c, hipGetLastError());

  // pass 2 (nmin = 1: a channel without a block has K = 0 already)
  const dim3 grid2((unsigned)groups, ch);
  rc = sig_select(c, state, hist, dim3(ch), p.frac, p.kmin, 1, [&](int level) {
    hipLaunchKernelGGL(k_sigma_hist, grid2, dim3(NLK_SIG_THREADS), 0, c->stream, hist, (const uint32_t*)keys,
                       (const NlkSigState*)state, n, level);
  });
  if (rc) return rc;

  // pass 3
  hipLaunchKernelGGL(k_sigma_sums, grid2, dim3(NLK_SIG_SUM_THREADS), 0, c->stream, part, count, (const uint32_t*)keys,
                     (const NlkSigState*)state, d_img, w, ch, p.step, s.nbx, n, s.share);
  HIPCHK(c, hipGetLastError());
  hipLaunchKernelGGL(k_sigma_final, dim3(1), dim3(NLK_SIG_THREADS), 0, c->stream, d_sigma, d_counts,
                     (const double*)part, (const int*)count, (const NlkSigState*)state, ch, (int)groups, p.high_min);
  HIPCHK(c, hipGetLastError());
  return NLK_OK;
}

void nlk_curve_default_params(struct nlk_curve_params* p) {
  if (!p) return;
  p->step = 4;
  p->frac = 0.1f;
  p->kmin = 32;
  p->low_max = 5;
  p->high_min = 8;
  p->nbins = 16;
  p->lo = 0.f;
  p->hi = 256.f;
  p->nmin = 32;
}

int nlk_dev_estimate_noise_curve(nlk_ctx* c, float* d_curve, struct nlk_curve_bin* d_bins, const float* d_img, int w,
                                 int h, int ch, const struct nlk_curve_params* prms) {
  const char* who = "nlk_dev_estimate_noise_curve";
  if (!c || !d_curve || !d_img || ch < 1 || ch > 65535) return fail(c, NLK_EINVAL, "%s: bad argument", who);
  struct nlk_curve_params p;
  nlk_curve_default_params(&p);
  if (prms) p = *prms;
  int rc = sig_check(c, who, w, h, p.step, p.frac, p.low_max, p.high_min);
  if (rc) return rc;
  if (p.nbins < 1 || p.nbins > NLK_CURVE_MAX_BINS)
    return fail(c, NLK_EINVAL, "%s: nbins = %d, must be in 1..%d", who, p.nbins, NLK_CURVE_MAX_BINS);
  if (!(p.hi > p.lo && fabsf(p.lo) <= 3.402823466e38f && fabsf(p.hi) <= 3.402823466e38f))
    return fail(c, NLK_EINVAL, "%s: lo = %g, hi = %g, must be finite with lo < hi", who, (double)p.lo, (double)p.hi);
  if (p.nmin < 1 || p.kmin < 1)
    return fail(c, NLK_EINVAL, "%s: nmin = %d, kmin = %d, must be at least 1", who, p.nmin, p.kmin);
  SigShape s;
  if ((rc = sig_shape(c, who, &s, w, h, ch, p.step, NLK_CURVE_MAX_GROUPS))) return rc;
  const size_t n = s.n, groups = s.groups;
  NLK_USE_DEVICE(c);

  // scratch, grown on demand and kept: histograms [ch][nbins][4][256] | state [ch][nbins] | counts [ch][nbins][groups]
  // | sums of means [ch][nbins][groups] | partials [ch][nbins][groups][64] | block means [ch][n] | keys [ch][n] |
  // bins [ch][n]
  const size_t slots = (size_t)ch * p.nbins;
  const size_t o_state = slots * 1024 * sizeof(uint32_t);
  const size_t o_count = o_state + slots * sizeof(NlkSigState);
  const size_t o_msum = (o_count + slots * groups * sizeof(int) + 7) & ~(size_t)7;
  const size_t o_part = o_msum + slots * groups * sizeof(double);
  const size_t o_means = o_part + slots * groups * 64 * sizeof(double);
  const size_t o_keys = o_means + (size_t)ch * n * sizeof(double);
  const size_t o_bins = o_keys + (size_t)ch * n * sizeof(uint32_t);
  rc = reserve(c, c->curve, o_bins + (size_t)ch * n);
  if (rc) return rc;
  char* base = (char*)c->curve.p;
  uint32_t* hist = (uint32_t*)base;
  NlkSigState* state = (NlkSigState*)(base + o_state);
  int* count = (int*)(base + o_count);
  double* msum = (double*)(base + o_msum);
  double* part = (double*)(base + o_part);
  double* means = (double*)(base + o_means);
  uint32_t* keys = (uint32_t*)(base + o_keys);
  uint8_t* bins = (uint8_t*)(base + o_bins);
  HIPCHK(c, hipMemsetAsync(hist, 0, o_state, c->stream));

  // pass 1
  if (s.grid1.y > 65535) return fail(c, NLK_EINVAL, "%s: %d block rows are too many", who, s.nby);
  const bool lhist = p.nbins <= NLK_CURVE_LDS_BINS;
#define NLK_CURVE_KEYS(S, L)                                                                                         \
  hipLaunchKernelGGL((k_curve_keys<S, L>), s.grid1, dim3(NLK_SIG_THREADS), s.tile, c->stream, keys, bins, means, hist, \
                     d_img, w, h, ch, p.step, s.nbx, s.nby, p.low_max, p.nbins, p.lo, p.hi)
  if (s.tile && lhist) NLK_CURVE_KEYS(true, true);
  else if (s.tile) NLK_CURVE_KEYS(true, false);
  else if (lhist) NLK_CURVE_KEYS(false, true);
  else NLK_CURVE_KEYS(false, false);
#undef NLK_CURVE_KEYS
  HIPCHK(c, hipGetLastError());

  // pass 2
  rc = sig_select(c, state, hist, dim3(p.nbins, ch), p.frac, p.kmin, p.nmin, [&](int level) {
    if (lhist)
      hipLaunchKernelGGL(k_curve_hist<true>, dim3((unsigned)groups, ch), dim3(NLK_SIG_THREADS), 0, c->stream, hist,
                         (const uint32_t*)keys, (const uint8_t*)bins, (const NlkSigState*)state, n, level, p.nbins);
    else
      hipLaunchKernelGGL(k_curve_hist<false>, dim3((unsigned)groups, ch), dim3(NLK_SIG_THREADS), 0, c->stream, hist,
                         (const uint32_t*)keys, (const uint8_t*)bins, (const NlkSigState*)state, n, level, p.nbins);
  });
  if (rc) return rc;

  // pass 3
  hipLaunchKernelGGL(k_curve_sums, dim3((unsigned)groups, p.nbins, ch), dim3(NLK_SIG_SUM_THREADS), 0, c->stream, part,
                     count, msum, (const uint32_t*)keys, (const uint8_t*)bins, (const double*)means,
                     (const NlkSigState*)state, d_img, w, ch, p.step, s.nbx, n, s.share);
  HIPCHK(c, hipGetLastError());
  hipLaunchKernelGGL(k_curve_final, dim3(ch), dim3(NLK_SIG_THREADS), 0, c->stream, d_curve, (NlkCurveBin*)d_bins,
                     (const double*)part, (const int*)count, (const double*)msum, (const NlkSigState*)state, p.nbins,
                     (int)groups, p.high_min);
  HIPCHK(c, hipGetLastError());
  return NLK_OK;
}

}  // extern "C"
