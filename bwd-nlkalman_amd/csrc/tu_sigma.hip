// tu_sigma.hip — the noise-level estimator's entry points of include/nlk_hip.h (kernels: k_sigma.h)
#include "k_sigma.h"
#include "nlk_internal.h"

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
  if (!c || !d_sigma || !d_img || ch < 1 || ch > 65535) return fail(c, NLK_EINVAL, "nlk_dev_estimate_sigma: bad argument");
  struct nlk_sigma_params p;
  nlk_sigma_default_params(&p);
  if (prms) p = *prms;
  if (w < 8 || h < 8)
    return fail(c, NLK_EINVAL, "nlk_dev_estimate_sigma: a %d x %d image holds no 8 x 8 block", w, h);
  if (p.step < 1) return fail(c, NLK_EINVAL, "nlk_dev_estimate_sigma: step = %d, must be at least 1", p.step);
  if (!(p.frac > 0.f && p.frac <= 1.f))
    return fail(c, NLK_EINVAL, "nlk_dev_estimate_sigma: frac = %g, must be in (0, 1]", (double)p.frac);
  if (p.low_max < 1 || p.low_max > 14 || p.high_min < 1 || p.high_min > 14)
    return fail(c, NLK_EINVAL, "nlk_dev_estimate_sigma: low_max = %d, high_min = %d, must be in 1..14", p.low_max,
                p.high_min);
  const int nbx = (w - 8) / p.step + 1, nby = (h - 8) / p.step + 1;
  const size_t n = (size_t)nbx * nby;  // blocks per channel
  if (n > 0x7fffffffull) return fail(c, NLK_EINVAL, "nlk_dev_estimate_sigma: %zu blocks per channel are too many", n);
  NLK_USE_DEVICE(c);

  // pass 2 and 3: workgroups per channel and keys per workgroup, functions of n alone
  size_t groups = (n + 2047) / 2048;
  if (groups > NLK_SIG_MAX_GROUPS) groups = NLK_SIG_MAX_GROUPS;
  const size_t share = ((n + groups - 1) / groups + NLK_SIG_SUM_THREADS - 1) / NLK_SIG_SUM_THREADS * NLK_SIG_SUM_THREADS;
  groups = (n + share - 1) / share;

  // scratch, grown on demand and kept: histograms [ch][4][256] | state [ch] | counts [ch][groups] | partials
  // [ch][groups][64] | keys [ch][n]
  const size_t o_state = (size_t)ch * 1024 * sizeof(uint32_t);
  const size_t o_count = o_state + (size_t)ch * sizeof(NlkSigState);
  const size_t o_part = (o_count + (size_t)ch * groups * sizeof(int) + 7) & ~(size_t)7;
  const size_t o_keys = o_part + (size_t)ch * groups * 64 * sizeof(double);
  int rc = reserve(c, c->sig, o_keys + (size_t)ch * n * sizeof(uint32_t));
  if (rc) return rc;
  char* base = (char*)c->sig.p;
  uint32_t* hist = (uint32_t*)base;
  NlkSigState* state = (NlkSigState*)(base + o_state);
  int* count = (int*)(base + o_count);
  double* part = (double*)(base + o_part);
  uint32_t* keys = (uint32_t*)(base + o_keys);
  HIPCHK(c, hipMemsetAsync(hist, 0, o_state, c->stream));

  // pass 1
  const dim3 grid1((nbx + NLK_SIG_TBX - 1) / NLK_SIG_TBX, (nby + NLK_SIG_TBY - 1) / NLK_SIG_TBY, ch);
  if (grid1.y > 65535) return fail(c, NLK_EINVAL, "nlk_dev_estimate_sigma: %d block rows are too many", nby);
  const size_t lds = p.step <= 8 ? (size_t)nlk_sig_pitch(p.step) * nlk_sig_tile_h(p.step) * sizeof(float) : 0;
  if (lds && lds <= NLK_SIG_LDS_MAX)
    hipLaunchKernelGGL(k_sigma_keys<true>, grid1, dim3(NLK_SIG_THREADS), lds, c->stream, keys, hist, d_img, w, h, ch,
                       p.step, nbx, nby, p.low_max);
  else
    hipLaunchKernelGGL(k_sigma_keys<false>, grid1, dim3(NLK_SIG_THREADS), 0, c->stream, keys, hist, d_img, w, h, ch,
                       p.step, nbx, nby, p.low_max);
  HIPCHK(c, hipGetLastError());

  // pass 2: the K-th key, a digit per level
  const dim3 grid2((unsigned)groups, ch);
  for (int level = 0; level < 4; ++level) {
    if (level > 0) {
      hipLaunchKernelGGL(k_sigma_hist, grid2, dim3(NLK_SIG_THREADS), 0, c->stream, hist, (const uint32_t*)keys,
                         (const NlkSigState*)state, n, level);
      HIPCHK(c, hipGetLastError());
    }
    hipLaunchKernelGGL(k_sigma_pick, dim3(ch), dim3(NLK_SIG_THREADS), 0, c->stream, state, (const uint32_t*)hist,
                       level, p.frac, p.kmin);
    HIPCHK(c, hipGetLastError());
  }

  // pass 3
  hipLaunchKernelGGL(k_sigma_sums, grid2, dim3(NLK_SIG_SUM_THREADS), 0, c->stream, part, count, (const uint32_t*)keys,
                     (const NlkSigState*)state, d_img, w, ch, p.step, nbx, n, share);
  HIPCHK(c, hipGetLastError());
  hipLaunchKernelGGL(k_sigma_final, dim3(1), dim3(NLK_SIG_THREADS), 0, c->stream, d_sigma, d_counts,
                     (const double*)part, (const int*)count, (const NlkSigState*)state, ch, (int)groups, p.high_min);
  HIPCHK(c, hipGetLastError());
  return NLK_OK;
}

}  // extern "C"
