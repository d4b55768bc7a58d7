// tu_bmflow.hip — nlk_dev_bm_flow of include/nlk_hip.h (kernels: k_bmflow.h; restated in numpy by tests/bmflow_ref.py)
#include "k_bmflow.h"
#include "nlk_internal.h"

extern "C" void nlk_bmflow_default_params(struct nlk_bmflow_params* p) {
  p->fscale = 1;
  p->radius = 2;
  p->min_side = 16;
}

#define NLK_BM_MAX_LEVELS 32

static inline dim3 bm_grid(int w, int h) { return dim3(((unsigned)w + 63) / 64, ((unsigned)h + 3) / 4); }

template <int R>
static void bm_match(hipStream_t st, nlk_flow_f2* V, const float* I0, const float* I1, const NlkBmLevel& g, const nlk_flow_f2* Vc,
                     const NlkBmLevel& gc) {
  hipLaunchKernelGGL(k_bm_match<R>, dim3(((unsigned)g.nbx + NLK_BM_WAVES - 1) / NLK_BM_WAVES, (unsigned)g.nby), dim3(64 * NLK_BM_WAVES),
                     0, st, V, I0, I1, g, Vc, gc);
}

extern "C" int nlk_dev_bm_flow(nlk_ctx* c, float* flow, const float* I0, const float* I1, int w, int h,
                               const struct nlk_bmflow_params* prms) {
  const char* who = "nlk_dev_bm_flow";
  if (!c || !flow || !I0 || !I1) return fail(c, NLK_EINVAL, "%s: NULL argument", who);
  if (w < 1 || h < 1) return fail(c, NLK_EINVAL, "%s: size %d x %d", who, w, h);
  struct nlk_bmflow_params P;
  nlk_bmflow_default_params(&P);
  if (prms) P = *prms;
  if (P.radius < 1 || P.radius > 3) return fail(c, NLK_EINVAL, "%s: radius %d is outside 1..3", who, P.radius);
  if (P.fscale < 0) return fail(c, NLK_EINVAL, "%s: fscale %d is negative", who, P.fscale);
  if ((unsigned)h + 3 > 4u * 65535u) return fail(c, NLK_EUNSUP, "%s: %d rows are more than one launch covers", who, h);
  NLK_USE_DEVICE(c);
  nlk_flow_f2* out = reinterpret_cast<nlk_flow_f2*>(flow);
  if (w < NLK_BM_BLOCK || h < NLK_BM_BLOCK) {  // no room for a block: the flow is 0
    HIPCHK(c, hipMemsetAsync(flow, 0, (size_t)w * h * 2 * sizeof(float), c->stream));
    return NLK_OK;
  }
  // the levels: added while the smaller side, halved, is at least min_side (and a block fits). lv[] runs on to LS, the
  // levels that the smallest min_side would give: the scratch is laid out for those
  const int min_side = P.min_side > NLK_BM_BLOCK ? P.min_side : NLK_BM_BLOCK;
  NlkBmLevel lv[NLK_BM_MAX_LEVELS];
  int L = 0, LS = 0;
  lv[0] = NlkBmLevel{w, h, nlk_bm_blocks(w), nlk_bm_blocks(h)};
  while (LS + 1 < NLK_BM_MAX_LEVELS && (lv[LS].w < lv[LS].h ? lv[LS].w : lv[LS].h) / 2 >= NLK_BM_BLOCK) {
    const int w2 = lv[LS].w / 2, h2 = lv[LS].h / 2;
    if (L == LS && (w2 < h2 ? w2 : h2) >= min_side) ++L;
    lv[++LS] = NlkBmLevel{w2, h2, nlk_bm_blocks(w2), nlk_bm_blocks(h2)};
  }
  const int f = P.fscale < L ? P.fscale : L;
  // scratch, in floats (every piece starts at an even offset): the pyramids of both images, the block vectors as
  // matched and after the median of every matched level, the stored flows of the levels between f and 0. Laid out for
  // every fscale and min_side at once (block vectors of all levels, flows of all levels but 0 and the last: about 1.7
  // floats per pixel), so that its size depends on w and h alone and a call with other parameters never reallocates
  size_t pyr[NLK_BM_MAX_LEVELS] = {}, raw[NLK_BM_MAX_LEVELS] = {}, med[NLK_BM_MAX_LEVELS] = {}, mid[NLK_BM_MAX_LEVELS] = {};
  size_t need = 0;
  for (int l = 1; l <= LS; ++l) {
    pyr[l] = need;
    need += 2 * (((size_t)lv[l].w * lv[l].h + 1) & ~(size_t)1);
  }
  for (int l = 0; l <= LS; ++l) {
    raw[l] = need;
    need += 2 * (size_t)lv[l].nbx * lv[l].nby;
    med[l] = need;
    need += 2 * (size_t)lv[l].nbx * lv[l].nby;
  }
  for (int l = 1; l < LS; ++l) {
    mid[l] = need;
    need += 2 * (size_t)lv[l].w * lv[l].h;
  }
  const int rc = reserve(c, c->bm, need * sizeof(float));
  if (rc != NLK_OK) return rc;
  float* S = (float*)c->bm.p;
  const hipStream_t st = c->stream;
  const float* im0[NLK_BM_MAX_LEVELS];
  const float* im1[NLK_BM_MAX_LEVELS];
  im0[0] = I0;
  im1[0] = I1;
  for (int l = 1; l <= L; ++l) {
    float* d0 = S + pyr[l];
    float* d1 = d0 + (((size_t)lv[l].w * lv[l].h + 1) & ~(size_t)1);
    dim3 grid = bm_grid(lv[l].w, lv[l].h);
    grid.z = 2;
    hipLaunchKernelGGL(k_bm_down, grid, dim3(64, 4), 0, st, d0, d1, im0[l - 1], im1[l - 1], lv[l - 1].w, lv[l].w, lv[l].h);
    im0[l] = d0;
    im1[l] = d1;
  }
  for (int l = L; l >= f; --l) {
    nlk_flow_f2* V = reinterpret_cast<nlk_flow_f2*>(S + raw[l]);
    nlk_flow_f2* M = reinterpret_cast<nlk_flow_f2*>(S + med[l]);
    const nlk_flow_f2* Vc = l < L ? reinterpret_cast<const nlk_flow_f2*>(S + med[l + 1]) : nullptr;
    const NlkBmLevel& gc = lv[l < L ? l + 1 : l];
    if (P.radius == 1) bm_match<1>(st, V, im0[l], im1[l], lv[l], Vc, gc);
    else if (P.radius == 2) bm_match<2>(st, V, im0[l], im1[l], lv[l], Vc, gc);
    else bm_match<3>(st, V, im0[l], im1[l], lv[l], Vc, gc);
    hipLaunchKernelGGL(k_bm_median, bm_grid(lv[l].nbx, lv[l].nby), dim3(64, 4), 0, st, M, V, lv[l].nbx, lv[l].nby);
  }
  const nlk_flow_f2* M = reinterpret_cast<const nlk_flow_f2*>(S + med[f]);
  if (f == 0) {
    hipLaunchKernelGGL(k_bm_dense, bm_grid(w, h), dim3(64, 4), 0, st, out, M, lv[0]);
  } else {
    nlk_flow_f2* to = f == 1 ? out : reinterpret_cast<nlk_flow_f2*>(S + mid[f - 1]);
    hipLaunchKernelGGL(k_bm_up2_dense, bm_grid(lv[f - 1].w, lv[f - 1].h), dim3(64, 4), 0, st, to, lv[f - 1].w, lv[f - 1].h, M, lv[f]);
    for (int l = f - 2; l >= 0; --l) {
      const nlk_flow_f2* from = to;
      to = l == 0 ? out : reinterpret_cast<nlk_flow_f2*>(S + mid[l]);
      hipLaunchKernelGGL(k_bm_up2, bm_grid(lv[l].w, lv[l].h), dim3(64, 4), 0, st, to, lv[l].w, lv[l].h, from, lv[l + 1].w, lv[l + 1].h);
    }
  }
  HIPCHK(c, hipGetLastError());
  return NLK_OK;
}
