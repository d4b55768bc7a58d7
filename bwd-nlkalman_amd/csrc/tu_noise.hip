// tu_noise.hip — the noise and error-measure entry points of include/nlk_hip.h (kernels: k_noise.h)
#include "k_noise.h"
#include "nlk_internal.h"

#include <math.h>

namespace {

// the LCG of lib/imscript-lite/src/random.c:19-31 and its jumps: jt.a[b], jt.c[b] = 2^b steps
void lcg_jumps(NlkLcgJump* jt) {
  uint64_t a = 6364136223846793005ull, c = 1442695040888963407ull;
  for (int b = 0; b < 64; ++b) {
    jt->a[b] = a;
    jt->c[b] = c;
    c = a * c + c;  // (a, c) after itself
    a = a * a;
  }
}

}  // namespace

extern "C" {

int nlk_dev_awgn(nlk_ctx* c, float* out, const float* in, size_t n, float sigma, uint32_t seed) {
  if (!c || (n && (!out || !in))) return fail(c, NLK_EINVAL, "nlk_dev_awgn: bad argument");
  if (n == 0) return NLK_OK;
  if (n > ((uint64_t)1 << 62)) return fail(c, NLK_EINVAL, "nlk_dev_awgn: n = %zu is too large", n);
  NLK_USE_DEVICE(c);
  NlkLcgJump jt;
  lcg_jumps(&jt);
  int nbits = 1;  // 2 i0 < 2n < 2^nbits
  while (nbits < 64 && ((uint64_t)2 * n) >> nbits) ++nbits;
  const uint64_t threads = (n + NLK_AWGN_RUN - 1) / NLK_AWGN_RUN;
  const uint64_t blocks = (threads + NLK_AWGN_THREADS - 1) / NLK_AWGN_THREADS;
  if (blocks > 0xffffffffull) return fail(c, NLK_EINVAL, "nlk_dev_awgn: n = %zu is too large", n);
  hipLaunchKernelGGL(k_awgn, dim3((unsigned)blocks), dim3(NLK_AWGN_THREADS), 0, c->stream, out, in, (uint64_t)n,
                     sigma, (uint64_t)seed, jt, nbits);
  HIPCHK(c, hipGetLastError());
  return NLK_OK;
}

int nlk_dev_noise_affine(nlk_ctx* c, float* out, const float* in, size_t n, int ch, const float* ab, uint32_t seed) {
  if (!c || !ab || (n && (!out || !in))) return fail(c, NLK_EINVAL, "nlk_dev_noise_affine: bad argument");
  if (ch < 1 || ch > NLK_NOISE_MAX_CH)
    return fail(c, NLK_EINVAL, "nlk_dev_noise_affine: ch = %d, must be in 1..%d", ch, NLK_NOISE_MAX_CH);
  NlkNoiseAb k = {};
  for (int i = 0; i < ch; ++i) {
    k.a[i] = ab[2 * i];
    k.b[i] = ab[2 * i + 1];
    if (!(fabsf(k.a[i]) <= 3.402823466e38f && fabsf(k.b[i]) <= 3.402823466e38f))
      return fail(c, NLK_EINVAL, "nlk_dev_noise_affine: channel %d: a = %g, b = %g are not finite", i, (double)k.a[i],
                  (double)k.b[i]);
  }
  if (n == 0) return NLK_OK;
  if (n > ((uint64_t)1 << 62)) return fail(c, NLK_EINVAL, "nlk_dev_noise_affine: n = %zu is too large", n);
  NLK_USE_DEVICE(c);
  NlkLcgJump jt;
  lcg_jumps(&jt);
  int nbits = 1;  // 2 i0 < 2n < 2^nbits
  while (nbits < 64 && ((uint64_t)2 * n) >> nbits) ++nbits;
  const uint64_t threads = (n + NLK_AWGN_RUN - 1) / NLK_AWGN_RUN;
  const uint64_t blocks = (threads + NLK_AWGN_THREADS - 1) / NLK_AWGN_THREADS;
  if (blocks > 0xffffffffull) return fail(c, NLK_EINVAL, "nlk_dev_noise_affine: n = %zu is too large", n);
  hipLaunchKernelGGL(k_noise_affine, dim3((unsigned)blocks), dim3(NLK_AWGN_THREADS), 0, c->stream, out, in,
                     (uint64_t)n, ch, k, (uint64_t)seed, jt, nbits);
  HIPCHK(c, hipGetLastError());
  return NLK_OK;
}

int nlk_dev_sqdiff_sum(nlk_ctx* c, double* sum, const float* a, const float* b, size_t n) {
  if (!c || !sum || (n && (!a || !b))) return fail(c, NLK_EINVAL, "nlk_dev_sqdiff_sum: bad argument");
  NLK_USE_DEVICE(c);
  // the partials: a fixed-size scratch, reserved once (it never grows, so no call frees it under a running one)
  int rc = reserve(c, c->sqd, NLK_SQD_MAX_BLOCKS * sizeof(double));
  if (rc) return rc;
  double* part = (double*)c->sqd.p;
  const uint64_t per_block = (uint64_t)NLK_SQD_THREADS * NLK_SQD_PER_THREAD;
  const uint64_t want = (n + per_block - 1) / per_block;
  const int blocks = (int)(want < NLK_SQD_MAX_BLOCKS ? want : NLK_SQD_MAX_BLOCKS);  // a function of n alone
  if (blocks > 0) {
    hipLaunchKernelGGL(k_sqdiff_partial, dim3(blocks), dim3(NLK_SQD_THREADS), 0, c->stream, part, a, b,
                       (uint64_t)n);
    HIPCHK(c, hipGetLastError());
  }
  hipLaunchKernelGGL(k_sqdiff_final, dim3(1), dim3(NLK_SQD_THREADS), 0, c->stream, sum, (const double*)part, blocks);
  HIPCHK(c, hipGetLastError());
  return NLK_OK;
}

}  // extern "C"
