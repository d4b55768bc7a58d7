// tu_ssim.hip — the quality measure's entry point of include/nlk_hip.h (kernels: k_ssim.h)
#include "k_ssim.h"
#include "nlk_internal.h"

#include <math.h>

extern "C" {

int nlk_dev_ssim(nlk_ctx* c, double* d_ssim, float* d_map, const float* d_a, const float* d_b, int w, int h, int ch,
                 float range) {
  const char* who = "nlk_dev_ssim";
  if (!c || !d_ssim || !d_a || !d_b) return fail(c, NLK_EINVAL, "%s: bad argument", who);
  if (w < NLK_SSIM_TAPS || h < NLK_SSIM_TAPS)
    return fail(c, NLK_EINVAL, "%s: a %d x %d image holds no %d x %d window", who, w, h, NLK_SSIM_TAPS, NLK_SSIM_TAPS);
  if (ch < 1 || ch > NLK_SSIM_MAX_CH)
    return fail(c, NLK_EINVAL, "%s: ch = %d, must be in 1..%d", who, ch, NLK_SSIM_MAX_CH);
  if (!(range > 0.f && range <= 3.402823466e38f))
    return fail(c, NLK_EINVAL, "%s: range = %g, must be positive and finite", who, (double)range);
  const int vw = w - 2 * NLK_SSIM_R, vh = h - 2 * NLK_SSIM_R;
  const dim3 grid((vw + NLK_SSIM_TX - 1) / NLK_SSIM_TX, (vh + NLK_SSIM_TY - 1) / NLK_SSIM_TY, ch);
  if (grid.y > 65535) return fail(c, NLK_EINVAL, "%s: %d rows are too many", who, h);
  const size_t tiles = (size_t)grid.x * grid.y;
  if (tiles > 0x7fffffffull) return fail(c, NLK_EINVAL, "%s: %zu tiles per channel are too many", who, tiles);
  NLK_USE_DEVICE(c);
  // the partials [ch][tiles]: grown on demand and kept
  int rc = reserve(c, c->ssim, (size_t)ch * tiles * sizeof(double));
  if (rc) return rc;
  double* part = (double*)c->ssim.p;

  NlkSsimWin win;
  double sum = 0.0;
  for (int k = 0; k < NLK_SSIM_TAPS; ++k) {
    const double d = (double)(k - NLK_SSIM_R);
    sum += win.g[k] = exp(-(d * d) / (2.0 * 1.5 * 1.5));
  }
  for (int k = 0; k < NLK_SSIM_TAPS; ++k) win.g[k] /= sum;
  const double L = (double)range, c1 = (0.01 * L) * (0.01 * L), c2 = (0.03 * L) * (0.03 * L);

  hipLaunchKernelGGL(k_ssim_tile, grid, dim3(NLK_SSIM_THREADS), 0, c->stream, part, d_map, d_a, d_b, w, h, ch, win, c1,
                     c2);
  HIPCHK(c, hipGetLastError());
  hipLaunchKernelGGL(k_ssim_final, dim3(1), dim3(NLK_SSIM_THREADS), 0, c->stream, d_ssim, (const double*)part, ch,
                     (int)tiles, (double)vw * (double)vh);
  HIPCHK(c, hipGetLastError());
  return NLK_OK;
}

}  // extern "C"
