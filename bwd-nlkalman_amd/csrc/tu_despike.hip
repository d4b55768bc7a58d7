// tu_despike.hip — the defective-pixel filter: nlk_dev_despike of include/nlk_hip.h (kernel: k_despike.h)
#include "k_despike.h"
#include "nlk_internal.h"

#include <math.h>

extern "C" int nlk_dev_despike(nlk_ctx* c, float* out, const float* in, uint32_t* d_count, int w, int h, int ch,
                               int radius, float thr) {
  const char* who = "nlk_dev_despike";
  if (!c || !out || !in) return fail(c, NLK_EINVAL, "%s: bad argument", who);
  if (out == in) return fail(c, NLK_EINVAL, "%s: out == in (the stencil reads its neighbours)", who);
  if (w < 1 || h < 1 || ch < 1 || ch > 16)
    return fail(c, NLK_EINVAL, "%s: w = %d, h = %d, ch = %d, must be >= 1 and ch <= 16", who, w, h, ch);
  if (radius != 1 && radius != 2) return fail(c, NLK_EINVAL, "%s: radius = %d, must be 1 or 2", who, radius);
  if (!(thr >= 0.f && thr <= 3.402823466e38f))
    return fail(c, NLK_EINVAL, "%s: thr = %g, must be finite and >= 0", who, (double)thr);
  // the kernel's indices: a row of w ch floats is indexed with int, and the grid is one dimension
  const int64_t W = (int64_t)w * ch, nbx = (W + DESPIKE_THREADS - 1) / DESPIKE_THREADS;
  const int64_t blocks = nbx * ((h + DESPIKE_ROWS - 1) / DESPIKE_ROWS);
  if (W > 0x7fffffff - 2 * DESPIKE_THREADS || blocks > 0x7fffffff)
    return fail(c, NLK_EUNSUP, "%s: a %d x %d x %d image is too large", who, w, h, ch);
  NLK_USE_DEVICE(c);
  if (d_count) HIPCHK(c, hipMemsetAsync(d_count, 0, sizeof(uint32_t) * ch, c->stream));
  const dim3 grid((unsigned)blocks), block(DESPIKE_THREADS);
  if (radius == 1)
    hipLaunchKernelGGL(k_despike<1>, grid, block, 0, c->stream, out, in, d_count, w, h, ch, thr, (int)nbx);
  else
    hipLaunchKernelGGL(k_despike<2>, grid, block, 0, c->stream, out, in, d_count, w, h, ch, thr, (int)nbx);
  HIPCHK(c, hipGetLastError());
  return NLK_OK;
}
