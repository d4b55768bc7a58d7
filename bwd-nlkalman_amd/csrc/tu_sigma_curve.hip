// tu_sigma_curve.hip — signal-dependent noise: the noise-curve estimator's and the variance-stabilising transform's
// entry points of include/nlk_hip.h (kernels: k_sigma_curve.h, k_vst.h)
#include "k_sigma_curve.h"
#include "k_vst.h"
#include "nlk_internal.h"

#include <math.h>

static_assert(sizeof(NlkCurveBin) == sizeof(struct nlk_curve_bin), "k_curve_final writes struct nlk_curve_bin");

namespace {

// the per-channel constants of the transform, in double; false for coefficients it refuses
bool vst_coef(NlkVstCoef* k, double* span, const float* ab, int ch) {
  for (int c = 0; c < ch; ++c) {
    const double a = ab[2 * c], b = ab[2 * c + 1];
    if (!(a >= 0.0 && b >= 0.0 && a <= 3.402823466e38 && b <= 3.402823466e38) || (a == 0.0 && b == 0.0)) return false;
    const double u0 = 0.375 * a * a + b, ru0 = sqrt(u0);
    if (k) {
      k->a[c] = (float)a;
      k->u0[c] = (float)u0;
      k->ru0[c] = (float)ru0;
      k->floor_[c] = a > 0.0 ? (float)(-2.0 * ru0 / a) : -INFINITY;
    }
    if (span) span[c] = 2.0 * 255.0 / (sqrt(255.0 * a + u0) + ru0);
  }
  return true;
}

int vst_run(nlk_ctx* c, const char* who, float* out, const float* in, size_t n, int ch, const float* ab, float s,
            int mode, bool inverse) {
  if (!c || !ab || (n && (!out || !in))) return fail(c, NLK_EINVAL, "%s: bad argument", who);
  if (ch < 1 || ch > NLK_VST_MAX_CH) return fail(c, NLK_EINVAL, "%s: ch = %d, must be in 1..%d", who, ch, NLK_VST_MAX_CH);
  if (!(s > 0.f && s <= 3.402823466e38f)) return fail(c, NLK_EINVAL, "%s: s = %g, must be positive and finite", who, (double)s);
  if (mode != 0 && mode != 1) return fail(c, NLK_EINVAL, "%s: mode = %d, must be 0 or 1", who, mode);
  NlkVstCoef k = {};
  if (!vst_coef(&k, nullptr, ab, ch))
    return fail(c, NLK_EINVAL, "%s: every (a, b) must be finite, non-negative and not (0, 0)", who);
  if (n == 0) return NLK_OK;
  NLK_USE_DEVICE(c);
  const uint64_t per_block = (uint64_t)NLK_VST_THREADS * 8;  // a thread takes about 8 samples, 4096 workgroups at most
  uint64_t blocks = (n + per_block - 1) / per_block;
  if (blocks > 4096) blocks = 4096;
  if (inverse)
    hipLaunchKernelGGL(k_vst<true>, dim3((unsigned)blocks), dim3(NLK_VST_THREADS), 0, c->stream, out, in, (uint64_t)n,
                       ch, k, s, mode);
  else
    hipLaunchKernelGGL(k_vst<false>, dim3((unsigned)blocks), dim3(NLK_VST_THREADS), 0, c->stream, out, in, (uint64_t)n,
                       ch, k, s, mode);
  HIPCHK(c, hipGetLastError());
  return NLK_OK;
}

}  // namespace

extern "C" {

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
  if (w < 8 || h < 8) return fail(c, NLK_EINVAL, "%s: a %d x %d image holds no 8 x 8 block", who, w, h);
  if (p.step < 1) return fail(c, NLK_EINVAL, "%s: step = %d, must be at least 1", who, p.step);
  if (!(p.frac > 0.f && p.frac <= 1.f)) return fail(c, NLK_EINVAL, "%s: frac = %g, must be in (0, 1]", who, (double)p.frac);
  if (p.low_max < 1 || p.low_max > 14 || p.high_min < 1 || p.high_min > 14)
    return fail(c, NLK_EINVAL, "%s: low_max = %d, high_min = %d, must be in 1..14", who, p.low_max, p.high_min);
  if (p.nbins < 1 || p.nbins > NLK_CURVE_MAX_BINS)
    return fail(c, NLK_EINVAL, "%s: nbins = %d, must be in 1..%d", who, p.nbins, NLK_CURVE_MAX_BINS);
  if (!(p.hi > p.lo && fabsf(p.lo) <= 3.402823466e38f && fabsf(p.hi) <= 3.402823466e38f))
    return fail(c, NLK_EINVAL, "%s: lo = %g, hi = %g, must be finite with lo < hi", who, (double)p.lo, (double)p.hi);
  if (p.nmin < 1 || p.kmin < 1)
    return fail(c, NLK_EINVAL, "%s: nmin = %d, kmin = %d, must be at least 1", who, p.nmin, p.kmin);
  const int nbx = (w - 8) / p.step + 1, nby = (h - 8) / p.step + 1;
  const size_t n = (size_t)nbx * nby;  // blocks per channel
  if (n > 0x7fffffffull) return fail(c, NLK_EINVAL, "%s: %zu blocks per channel are too many", who, n);
  NLK_USE_DEVICE(c);

  // pass 2 and 3: workgroups per channel and keys per workgroup, functions of n alone (as nlk_dev_estimate_sigma,
  // with 64 shares at most: pass 3 runs one workgroup per share and bin)
  size_t groups = (n + 2047) / 2048;
  if (groups > 64) groups = 64;
  const size_t share = ((n + groups - 1) / groups + NLK_SIG_SUM_THREADS - 1) / NLK_SIG_SUM_THREADS * NLK_SIG_SUM_THREADS;
  groups = (n + share - 1) / share;

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
  int rc = reserve(c, c->curve, o_bins + (size_t)ch * n);
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
  const dim3 grid1((nbx + NLK_SIG_TBX - 1) / NLK_SIG_TBX, (nby + NLK_SIG_TBY - 1) / NLK_SIG_TBY, ch);
  if (grid1.y > 65535) return fail(c, NLK_EINVAL, "%s: %d block rows are too many", who, nby);
  const size_t tile = p.step <= 8 ? (size_t)nlk_sig_pitch(p.step) * nlk_sig_tile_h(p.step) * sizeof(float) : 0;
  const bool staged = tile && tile <= NLK_SIG_LDS_MAX;
  const bool lhist = p.nbins <= NLK_CURVE_LDS_BINS;
#define NLK_CURVE_KEYS(S, L)                                                                                       \
  hipLaunchKernelGGL((k_curve_keys<S, L>), grid1, dim3(NLK_SIG_THREADS), S ? tile : 0, c->stream, keys, bins, means, \
                     hist, d_img, w, h, ch, p.step, nbx, nby, p.low_max, p.nbins, p.lo, p.hi)
  if (staged && lhist) NLK_CURVE_KEYS(true, true);
  else if (staged) NLK_CURVE_KEYS(true, false);
  else if (lhist) NLK_CURVE_KEYS(false, true);
  else NLK_CURVE_KEYS(false, false);
#undef NLK_CURVE_KEYS
  HIPCHK(c, hipGetLastError());

  // pass 2: the K_q-th key of every bin, a digit per level
  for (int level = 0; level < 4; ++level) {
    if (level > 0) {
      if (lhist)
        hipLaunchKernelGGL(k_curve_hist<true>, dim3((unsigned)groups, ch), dim3(NLK_SIG_THREADS), 0, c->stream, hist,
                           (const uint32_t*)keys, (const uint8_t*)bins, (const NlkSigState*)state, n, level, p.nbins);
      else
        hipLaunchKernelGGL(k_curve_hist<false>, dim3((unsigned)groups, ch), dim3(NLK_SIG_THREADS), 0, c->stream, hist,
                           (const uint32_t*)keys, (const uint8_t*)bins, (const NlkSigState*)state, n, level, p.nbins);
      HIPCHK(c, hipGetLastError());
    }
    hipLaunchKernelGGL(k_curve_pick, dim3(p.nbins, ch), dim3(NLK_SIG_THREADS), 0, c->stream, state,
                       (const uint32_t*)hist, level, p.frac, p.kmin, p.nmin);
    HIPCHK(c, hipGetLastError());
  }

  // pass 3
  hipLaunchKernelGGL(k_curve_sums, dim3((unsigned)groups, p.nbins, ch), dim3(NLK_SIG_SUM_THREADS), 0, c->stream, part,
                     count, msum, (const uint32_t*)keys, (const uint8_t*)bins, (const double*)means,
                     (const NlkSigState*)state, d_img, w, ch, p.step, nbx, n, share);
  HIPCHK(c, hipGetLastError());
  hipLaunchKernelGGL(k_curve_final, dim3(ch), dim3(NLK_SIG_THREADS), 0, c->stream, d_curve, (NlkCurveBin*)d_bins,
                     (const double*)part, (const int*)count, (const double*)msum, (const NlkSigState*)state, p.nbins,
                     (int)groups, p.high_min);
  HIPCHK(c, hipGetLastError());
  return NLK_OK;
}

float nlk_vst_scale(const float* ab, int ch) {
  double span[NLK_VST_MAX_CH];
  if (!ab || ch < 1 || ch > NLK_VST_MAX_CH || !vst_coef(nullptr, span, ab, ch)) return NAN;
  double sum = 0.0;
  for (int c = 0; c < ch; ++c) sum += span[c];
  return (float)(255.0 / (sum / (double)ch));
}

int nlk_dev_vst_forward(nlk_ctx* c, float* out, const float* in, size_t n, int ch, const float* ab, float s) {
  return vst_run(c, "nlk_dev_vst_forward", out, in, n, ch, ab, s, 0, false);
}

int nlk_dev_vst_inverse(nlk_ctx* c, float* out, const float* in, size_t n, int ch, const float* ab, float s,
                        int mode) {
  return vst_run(c, "nlk_dev_vst_inverse", out, in, n, ch, ab, s, mode, true);
}

}  // extern "C"
