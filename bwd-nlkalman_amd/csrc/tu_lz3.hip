// tu_lz3.hip — the Lanczos-3 pyramid entry points of include/nlk_hip.h (kernels: k_lz3.h)
#include <math.h>

#include "k_lz3.h"
#include "nlk_internal.h"

namespace {

// the Lanczos-3 window sin(pi x) sin(pi x / 3) / (pi^2 x^2 / 3), |x| < 3
double lz3_window(double x) {
  const double pi = 3.14159265358979323846;
  if (x == 0.0) return 1.0;
  if (fabs(x) >= 3.0) return 0.0;
  return sin(pi * x) * sin(pi * x / 3.0) / (pi * pi * x * x / 3.0);
}

// taps in double, normalised, rounded to float once; g > 0: the gblur taps (Gaussian of length
// max(2 floor(g), 5), weights below eps * max set to 0, normalised), g == 0: the identity (one tap)
void lz3_taps(NlkLz3Taps* tp, double g, int* ng, int* anchor) {
  double k[12], s = 0.0;
  for (int t = 0; t < 12; ++t) s += k[t] = lz3_window((t - 5.5) / 2.0);
  for (int t = 0; t < 12; ++t) tp->down[t] = (float)(k[t] / s);
  double e[6], o[6], se = 0.0, so = 0.0;
  for (int t = 0; t < 6; ++t) {
    se += e[t] = lz3_window(t - 3 + 0.25);  // s = t - 3 in [-3, 2]
    so += o[t] = lz3_window(t - 2 - 0.25);  // s = t - 2 in [-2, 3]
  }
  for (int t = 0; t < 6; ++t) {
    tp->even[t] = (float)(e[t] / se);
    tp->odd[t] = (float)(o[t] / so);
  }
  if (g == 0.0) {
    *ng = 1;
    *anchor = 0;
    tp->gauss[0] = 1.f;
    return;
  }
  const int n = std::max(2 * (int)floor(g), 5);
  double w[NLK_LZ3_MAXG], mx = 0.0, sum = 0.0;
  for (int t = 0; t < n; ++t) {
    const double x = t - (n - 1) / 2.0;
    w[t] = exp(-x * x / (2.0 * g * g));
    mx = std::max(mx, w[t]);
  }
  for (int t = 0; t < n; ++t) {
    if (w[t] < 2.220446049250313e-16 * mx) w[t] = 0.0;
    sum += w[t];
  }
  for (int t = 0; t < n; ++t) tp->gauss[t] = (float)(w[t] / sum);
  *ng = n;
  // the anchor of an even-length kernel is the 1-based tap floor((n + 1) / 2), as in imfilter; only odd
  // lengths (g < 3, the pipeline's 0.7 among them) were checked against the reference's own output
  *anchor = (n + 1) / 2 - 1;
}

// channels per workgroup: all of them up to 4, fewer when the LDS image would pass 64 KiB (long gblur kernels)
size_t lz3_up_lds(int cc, int ng, bool recompose) {
  const int EW = NLK_LZ3_EW, EH = NLK_LZ3_EH, TX = NLK_LZ3_UTX;
  const int FW = EW + ng - 1, FH = EH + ng - 1;
  const size_t a = recompose ? std::max(FH * FW, EH * EW) : EH * EW;
  const size_t b = recompose ? std::max(FH * EW, EH * TX) : EH * TX;
  return (a + b) * cc * sizeof(float);
}

int lz3_down(nlk_ctx* c, float* dst, const float* src, int w, int h, int ch, const NlkLz3Taps& tp) {
  const int cc = std::min(ch, 4);
  const dim3 grid(((w + 1) / 2 + NLK_LZ3_DTX - 1) / NLK_LZ3_DTX, ((h + 1) / 2 + NLK_LZ3_DTY - 1) / NLK_LZ3_DTY,
                  (ch + cc - 1) / cc);
  switch (cc) {
    case 1: hipLaunchKernelGGL(k_lz3_down<1>, grid, dim3(NLK_LZ3_THREADS), 0, c->stream, dst, src, w, h, ch, tp); break;
    case 2: hipLaunchKernelGGL(k_lz3_down<2>, grid, dim3(NLK_LZ3_THREADS), 0, c->stream, dst, src, w, h, ch, tp); break;
    case 3: hipLaunchKernelGGL(k_lz3_down<3>, grid, dim3(NLK_LZ3_THREADS), 0, c->stream, dst, src, w, h, ch, tp); break;
    default: hipLaunchKernelGGL(k_lz3_down<4>, grid, dim3(NLK_LZ3_THREADS), 0, c->stream, dst, src, w, h, ch, tp); break;
  }
  HIPCHK(c, hipGetLastError());
  return NLK_OK;
}

template <bool R>
int lz3_up(nlk_ctx* c, float* out, int dw, int dh, const float* yh, const float* rl, const float* dl, int w, int h,
           int ch, int ng, int a, const NlkLz3Taps& tp) {
  int cc = std::min(ch, 4);
  while (cc > 1 && lz3_up_lds(cc, ng, R) > 65536) --cc;
  const size_t lds = lz3_up_lds(cc, ng, R);
  const dim3 grid((dw + NLK_LZ3_UTX - 1) / NLK_LZ3_UTX, (dh + NLK_LZ3_UTY - 1) / NLK_LZ3_UTY, (ch + cc - 1) / cc);
  const dim3 block(NLK_LZ3_THREADS);
  switch (cc) {
    case 1: hipLaunchKernelGGL((k_lz3_up<1, R>), grid, block, lds, c->stream, out, dw, dh, yh, rl, dl, w, h, ch, ng, a, tp); break;
    case 2: hipLaunchKernelGGL((k_lz3_up<2, R>), grid, block, lds, c->stream, out, dw, dh, yh, rl, dl, w, h, ch, ng, a, tp); break;
    case 3: hipLaunchKernelGGL((k_lz3_up<3, R>), grid, block, lds, c->stream, out, dw, dh, yh, rl, dl, w, h, ch, ng, a, tp); break;
    default: hipLaunchKernelGGL((k_lz3_up<4, R>), grid, block, lds, c->stream, out, dw, dh, yh, rl, dl, w, h, ch, ng, a, tp); break;
  }
  HIPCHK(c, hipGetLastError());
  return NLK_OK;
}

bool lz3_fits(int n, int big) { return big >= 1 && big >= 2 * n - 1 && big <= 2 * n + 1; }

}  // namespace

extern "C" {

int nlk_dev_lz3_down(nlk_ctx* c, float* dst, const float* src, int w, int h, int ch) {
  if (!c || !dst || !src || w < 1 || h < 1 || ch < 1) return fail(c, NLK_EINVAL, "nlk_dev_lz3_down: bad argument");
  if (dst == src) return fail(c, NLK_EINVAL, "nlk_dev_lz3_down: dst must not be src");
  NLK_USE_DEVICE(c);
  NlkLz3Taps tp;
  int ng, a;
  lz3_taps(&tp, 0.0, &ng, &a);
  return lz3_down(c, dst, src, w, h, ch, tp);
}

int nlk_dev_lz3_up(nlk_ctx* c, float* dst, int dw, int dh, const float* src, int w, int h, int ch) {
  if (!c || !dst || !src || w < 1 || h < 1 || ch < 1) return fail(c, NLK_EINVAL, "nlk_dev_lz3_up: bad argument");
  if (!lz3_fits(w, dw) || !lz3_fits(h, dh))
    return fail(c, NLK_EINVAL, "nlk_dev_lz3_up: %dx%d -> %dx%d: the output must be 2n - 1, 2n or 2n + 1 per axis", w, h,
                dw, dh);
  if (dst == src) return fail(c, NLK_EINVAL, "nlk_dev_lz3_up: dst must not be src");
  NLK_USE_DEVICE(c);
  NlkLz3Taps tp;
  int ng, a;
  lz3_taps(&tp, 0.0, &ng, &a);
  return lz3_up<false>(c, dst, dw, dh, nullptr, src, nullptr, w, h, ch, 1, 0, tp);
}

int nlk_dev_lz3_recompose_step(nlk_ctx* c, float* out, const float* yh, int w, int h, const float* rl, int wl, int hl,
                               int ch, float g) {
  if (!c || !out || !yh || !rl || w < 1 || h < 1 || ch < 1)
    return fail(c, NLK_EINVAL, "nlk_dev_lz3_recompose_step: bad argument");
  if (wl != (w + 1) / 2 || hl != (h + 1) / 2)
    return fail(c, NLK_EINVAL, "nlk_dev_lz3_recompose_step: the coarse level is %dx%d, down(%dx%d) is %dx%d", wl, hl,
                w, h, (w + 1) / 2, (h + 1) / 2);
  if (!(g >= 0.f && g < 33.f))
    return fail(c, NLK_EINVAL, "nlk_dev_lz3_recompose_step: g = %g (0 <= g < 33: at most %d Gaussian taps)", (double)g,
                NLK_LZ3_MAXG);
  if (out == rl) return fail(c, NLK_EINVAL, "nlk_dev_lz3_recompose_step: out must not be rl");
  NLK_USE_DEVICE(c);
  NlkLz3Taps tp;
  int ng, a;
  lz3_taps(&tp, (double)g, &ng, &a);
  // the scratch grows level by level in a recompose: an outgrown buffer is kept until the context goes, not
  // freed (hipFree would wait for the device between two levels)
  const size_t need = sizeof(float) * (size_t)wl * hl * ch;
  if (need > c->lz3.cap && c->lz3.p && c->lz3_nold < (int)(sizeof c->lz3_old / sizeof c->lz3_old[0])) {
    c->lz3_old[c->lz3_nold++] = c->lz3.base ? c->lz3.base : c->lz3.p;
    c->lz3 = NlkBuf{};
  }
  int rc = reserve(c, c->lz3, need);
  if (rc) return rc;
  float* dl = (float*)c->lz3.p;
  // (a) down(yh): the decompose kernel itself, so that rl - down(yh) is exactly 0 for an untouched level
  if ((rc = lz3_down(c, dl, yh, w, h, ch, tp))) return rc;
  // (b) out = yh + up(gblur(rl - down(yh)))
  return lz3_up<true>(c, out, w, h, yh, rl, dl, wl, hl, ch, ng, a, tp);
}

}  // extern "C"
