// tu_sure.hip — the error estimate's entry points of include/nlk_hip.h (kernels: k_sure.h)
#include "k_sure.h"
#include "nlk_internal.h"

extern "C" {

int nlk_dev_probe_add(nlk_ctx* c, float* out, const float* in, size_t n, float eps, uint64_t seed) {
  const char* who = "nlk_dev_probe_add";
  if (!c || (n && (!out || !in))) return fail(c, NLK_EINVAL, "%s: bad argument", who);
  if (!(eps >= -3.402823466e38f && eps <= 3.402823466e38f))
    return fail(c, NLK_EINVAL, "%s: eps = %g is not finite", who, (double)eps);
  if (n == 0) return NLK_OK;
  const uint64_t threads = ((uint64_t)n + NLK_PROBE_RUN - 1) / NLK_PROBE_RUN;
  const uint64_t blocks = (threads + NLK_PROBE_THREADS - 1) / NLK_PROBE_THREADS;
  if (blocks > 0x7fffffffull) return fail(c, NLK_EINVAL, "%s: n = %zu is too large", who, n);
  NLK_USE_DEVICE(c);
  const bool vec = (((uintptr_t)out | (uintptr_t)in) & 15) == 0;
  if (vec)
    hipLaunchKernelGGL(k_probe_add<true>, dim3((unsigned)blocks), dim3(NLK_PROBE_THREADS), 0, c->stream, out, in,
                       (uint64_t)n, eps, seed);
  else
    hipLaunchKernelGGL(k_probe_add<false>, dim3((unsigned)blocks), dim3(NLK_PROBE_THREADS), 0, c->stream, out, in,
                       (uint64_t)n, eps, seed);
  HIPCHK(c, hipGetLastError());
  return NLK_OK;
}

int nlk_dev_sure_terms(nlk_ctx* c, double* d_total, double* d_blocks, const float* d_y, const float* d_f,
                       const float* d_fp, int w, int h, int ch, int block, uint64_t seed) {
  const char* who = "nlk_dev_sure_terms";
  if (!c || !d_total || !d_y || !d_f || !d_fp) return fail(c, NLK_EINVAL, "%s: bad argument", who);
  if (w < 1 || h < 1) return fail(c, NLK_EINVAL, "%s: a %d x %d image holds no sample", who, w, h);
  if (ch < 1 || ch > NLK_SURE_MAX_CH)
    return fail(c, NLK_EINVAL, "%s: ch = %d, must be in 1..%d", who, ch, NLK_SURE_MAX_CH);
  if (block < NLK_SURE_MIN_BLOCK || block > NLK_SURE_MAX_BLOCK)
    return fail(c, NLK_EINVAL, "%s: block = %d, must be in %d..%d", who, block, NLK_SURE_MIN_BLOCK, NLK_SURE_MAX_BLOCK);
  const int nbx = (w + block - 1) / block, nby = (h + block - 1) / block;
  const uint64_t tiles = (uint64_t)nbx * nby;
  if (tiles > 0x7ffffff0ull) return fail(c, NLK_EINVAL, "%s: %llu tiles are too many", who, (unsigned long long)tiles);
  NLK_USE_DEVICE(c);
  double* blocks = d_blocks;
  if (!blocks) {  // the tiles' sums: grown on demand and kept
    int rc = reserve(c, c->sure, (size_t)tiles * ch * 2 * sizeof(double));
    if (rc) return rc;
    blocks = (double*)c->sure.p;
  }
  const int ntiles = (int)tiles;
  const dim3 grid((ntiles + NLK_SURE_WAVES - 1) / NLK_SURE_WAVES), wg(NLK_SURE_THREADS);
  if (ch == 1)
    hipLaunchKernelGGL(k_sure_blocks<1>, grid, wg, 0, c->stream, blocks, d_y, d_f, d_fp, w, h, ch, block, nbx, ntiles,
                       seed);
  else if (ch == 3)
    hipLaunchKernelGGL(k_sure_blocks<3>, grid, wg, 0, c->stream, blocks, d_y, d_f, d_fp, w, h, ch, block, nbx, ntiles,
                       seed);
  else
    hipLaunchKernelGGL(k_sure_blocks<0>, grid, wg, 0, c->stream, blocks, d_y, d_f, d_fp, w, h, ch, block, nbx, ntiles,
                       seed);
  HIPCHK(c, hipGetLastError());
  hipLaunchKernelGGL(k_sure_final, dim3(1), dim3(NLK_SURE_FINAL_THREADS), 0, c->stream, d_total,
                     (const double*)blocks, ntiles, 2 * ch);
  HIPCHK(c, hipGetLastError());
  return NLK_OK;
}

double nlk_sure_mse(double R, double D, double n, double sigma, double eps) {
  const double s2 = sigma * sigma;
  return R / n - s2 + 2.0 * s2 * D / (eps * n);
}

}  // extern "C"
