// tu_defect.hip — one step of the defect map learned over time: nlk_dev_defect_step of include/nlk_hip.h (kernel: k_defect.h)
#include "k_defect.h"
#include "nlk_internal.h"

#include <math.h>

extern "C" int nlk_dev_defect_step(nlk_ctx* c, float* out, const float* in, float* mean_out, const float* mean_in,
                                   uint8_t* d_map, uint32_t* d_count, int w, int h, int ch, int radius, float thr,
                                   float gain) {
  const char* who = "nlk_dev_defect_step";
  if (!c || !out || !in || !mean_out) return fail(c, NLK_EINVAL, "%s: bad argument", who);
  if (w < 1 || h < 1 || ch < 1 || ch > 16)
    return fail(c, NLK_EINVAL, "%s: w = %d, h = %d, ch = %d, must be >= 1 and ch <= 16", who, w, h, ch);
  if (radius != 1 && radius != 2) return fail(c, NLK_EINVAL, "%s: radius = %d, must be 1 or 2", who, radius);
  if (!(thr >= 0.f && thr <= 3.402823466e38f))
    return fail(c, NLK_EINVAL, "%s: thr = %g, must be finite and >= 0", who, (double)thr);
  if (!(gain > 0.f && gain <= 1.f)) return fail(c, NLK_EINVAL, "%s: gain = %g, must be in (0, 1]", who, (double)gain);
  // the stencil reads the neighbours of both inputs while other workgroups write both outputs: no two planes may overlap
  const size_t n = (size_t)w * h * ch;
  const float* plane[4] = {out, in, mean_out, mean_in};
  for (int i = 0; i < 4; ++i)
    for (int j = i + 1; j < 4; ++j)
      if (plane[i] && plane[j] && plane[i] < plane[j] + n && plane[j] < plane[i] + n)
        return fail(c, NLK_EINVAL, "%s: out, in, mean_out and mean_in must not overlap (the stencil reads neighbours)", who);
  // the kernel's indices: a row of w ch floats is indexed with int, and the grid is one dimension
  const int64_t W = (int64_t)w * ch, nbx = (W + DESPIKE_THREADS - 1) / DESPIKE_THREADS;
  const int64_t blocks = nbx * ((h + DESPIKE_ROWS - 1) / DESPIKE_ROWS);
  const int64_t flat = (int64_t)((n + DESPIKE_THREADS - 1) / DESPIKE_THREADS);
  if (W > 0x7fffffff - 2 * DESPIKE_THREADS || blocks > 0x7fffffff || flat > 0x7fffffff)
    return fail(c, NLK_EUNSUP, "%s: a %d x %d x %d image is too large", who, w, h, ch);
  NLK_USE_DEVICE(c);
  if (d_count) HIPCHK(c, hipMemsetAsync(d_count, 0, sizeof(uint32_t) * ch, c->stream));
  const dim3 grid((unsigned)blocks), block(DESPIKE_THREADS);
  if (!mean_in)
    hipLaunchKernelGGL(k_defect_first, dim3((unsigned)flat), block, 0, c->stream, out, in, mean_out, d_map, n);
  else if (radius == 1)
    hipLaunchKernelGGL(k_defect_step<1>, grid, block, 0, c->stream, out, in, mean_out, mean_in, d_map, d_count, w, h, ch,
                       thr, gain, (int)nbx);
  else
    hipLaunchKernelGGL(k_defect_step<2>, grid, block, 0, c->stream, out, in, mean_out, mean_in, d_map, d_count, w, h, ch,
                       thr, gain, (int)nbx);
  HIPCHK(c, hipGetLastError());
  return NLK_OK;
}
