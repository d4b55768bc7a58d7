// tu_vst.hip — signal-dependent noise: the variance-stabilising transform's entry points of include/nlk_hip.h
// (kernel: k_vst.h; the noise curve that gives its coefficients is tu_sigma.hip's)
#include "k_vst.h"
#include "nlk_internal.h"

#include <math.h>

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
