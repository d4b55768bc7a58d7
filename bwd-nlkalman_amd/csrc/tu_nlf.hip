// tu_nlf.hip — a noise-level function of any shape: the transform's entry points of include/nlk_hip.h
// (kernel: k_nlf.h; the table is made on the host by host/nlf_build.c from the bins of tu_sigma.hip's noise curve)
#include "k_nlf.h"
#include "nlk_internal.h"

#include <math.h>

namespace {

static_assert(NLK_NLF_CH == NLK_NLF_MAX_CH && NLK_NLF_ROW == NLK_NLF_MAX_BINS + 1, "k_nlf.h and nlk_hip.h disagree");

// the device copy of `t`, in the context: uploaded when the table differs from the one the context holds (the
// comparison is of 12.7 KB on the host), not on every call
int nlf_device_table(nlk_ctx* c, const nlk_nlf_table* t) {
  const size_t bytes = sizeof(float) * NLK_NLF_TABLE_FLOATS;
  float packed[NLK_NLF_TABLE_FLOATS];
  memcpy(packed, t->x, sizeof t->x);
  memcpy(packed + NLK_NLF_ROW, t->G, sizeof t->G);
  memcpy(packed + (1 + NLK_NLF_CH) * NLK_NLF_ROW, t->slope, sizeof t->slope);
  memcpy(packed + (1 + 2 * NLK_NLF_CH) * NLK_NLF_ROW, t->islope, sizeof t->islope);
  if (c->nlf_host && c->nlf.p && !memcmp(c->nlf_host, packed, bytes)) return NLK_OK;
  if (!c->nlf_host && !(c->nlf_host = (float*)malloc(bytes))) return fail(c, NLK_ENOMEM, "nlf table: out of memory");
  const int rc = reserve(c, c->nlf, bytes);
  if (rc) return rc;
  memset(c->nlf_host, 0xff, bytes);  // (not a table, should the upload fail)
  HIPCHK(c, hipMemcpyAsync(c->nlf.p, packed, bytes, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));  // packed[] is on the stack
  memcpy(c->nlf_host, packed, bytes);
  return NLK_OK;
}

int nlf_run(nlk_ctx* c, const char* who, float* out, const float* in, size_t n, int ch, const nlk_nlf_table* t,
            bool inverse) {
  if (!c || !t || (n && (!out || !in))) return fail(c, NLK_EINVAL, "%s: bad argument", who);
  if (t->ch < 1 || t->ch > NLK_NLF_MAX_CH || t->nbins < 1 || t->nbins > NLK_NLF_MAX_BINS)
    return fail(c, NLK_EINVAL, "%s: the table has ch = %d, nbins = %d, must be in 1..%d and 1..%d", who, t->ch, t->nbins,
                NLK_NLF_MAX_CH, NLK_NLF_MAX_BINS);
  if (ch != t->ch) return fail(c, NLK_EINVAL, "%s: ch = %d, the table's is %d", who, ch, t->ch);
  if (!(t->s > 0.f && t->s <= 3.402823466e38f))
    return fail(c, NLK_EINVAL, "%s: the table's s = %g, must be positive and finite (a channel kept no bin?)", who,
                (double)t->s);
  if (n == 0) return NLK_OK;
  NLK_USE_DEVICE(c);
  const int rc = nlf_device_table(c, t);
  if (rc) return rc;
  const uint64_t per_block = (uint64_t)NLK_NLF_THREADS * 8;  // a thread takes about 8 samples, 4096 workgroups at most
  uint64_t blocks = (n + per_block - 1) / per_block;
  if (blocks > 4096) blocks = 4096;
  const float* tab = (const float*)c->nlf.p;
  if (inverse)
    hipLaunchKernelGGL(k_nlf<true>, dim3((unsigned)blocks), dim3(NLK_NLF_THREADS), 0, c->stream, out, in, (uint64_t)n,
                       ch, t->nbins, t->lo, t->inv_dx, tab);
  else
    hipLaunchKernelGGL(k_nlf<false>, dim3((unsigned)blocks), dim3(NLK_NLF_THREADS), 0, c->stream, out, in, (uint64_t)n,
                       ch, t->nbins, t->lo, t->inv_dx, tab);
  HIPCHK(c, hipGetLastError());
  return NLK_OK;
}

}  // namespace

extern "C" {

int nlk_dev_nlf_forward(nlk_ctx* c, float* out, const float* in, size_t n, int ch, const struct nlk_nlf_table* t) {
  return nlf_run(c, "nlk_dev_nlf_forward", out, in, n, ch, t, false);
}

int nlk_dev_nlf_inverse(nlk_ctx* c, float* out, const float* in, size_t n, int ch, const struct nlk_nlf_table* t) {
  return nlf_run(c, "nlk_dev_nlf_inverse", out, in, n, ch, t, true);
}

}  // extern "C"
