// tu_group_generic.hip — launchers of the LDS-DCT group kernel (k_group_lds.h): the fixed shapes 4 / 6 / 8 / 10 / 12 /
// 16 with 1 or 3 channels, and the run-time shape for everything else up to 32 x 32
#include "k_group_lds.h"
#include "nlk_internal.h"

namespace {

template <class S>
int launch_group_lds(nlk_ctx* c, const NlkRecView& v, const NlkGeom& g, const float* img, const float* cur, const float* prev, float* acc,
                     const uint8_t* active, size_t lds) {
  void (*kern)(const float*, const float*, const float*, const uint8_t*, NlkGeom, const uint32_t*, const NlkTarget*,
               const uint32_t*, const uint8_t*, const float*, const float*, float*) =
      g.smoother ? k_group_lds<S, true> : k_group_lds<S, false>;
  if (lds) HIPCHK(c, hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  const float* basis = (const float*)c->tabs.p;
  hipLaunchKernelGGL(kern, dim3(g.ngx * g.ngy), dim3(S::NT), lds, v.stream, img, cur, prev,
                     (const uint8_t*)c->vmap.p, g, (const uint32_t*)v.topk, (const NlkTarget*)v.tinfo,
                     (const uint32_t*)v.gcoords, active, basis, basis + g.p2, acc);
  HIPCHK(c, hipGetLastError());
  return NLK_OK;
}

template <int CH>
int launch_group_ch(nlk_ctx* c, const NlkRecView& v, const NlkGeom& g, const float* img, const float* cur,
                    const float* prev, float* acc, const uint8_t* active) {
  switch (g.psz) {
    case 4: return launch_group_lds<GroupFixed<4, CH>>(c, v, g, img, cur, prev, acc, active, 0);
    case 6: return launch_group_lds<GroupFixed<6, CH>>(c, v, g, img, cur, prev, acc, active, 0);
    case 8: return launch_group_lds<GroupFixed<8, CH>>(c, v, g, img, cur, prev, acc, active, 0);
    case 10: return launch_group_lds<GroupFixed<10, CH>>(c, v, g, img, cur, prev, acc, active, 0);
    case 12: return launch_group_lds<GroupFixed<12, CH>>(c, v, g, img, cur, prev, acc, active, 0);
    case 16: return launch_group_lds<GroupFixed<16, CH>>(c, v, g, img, cur, prev, acc, active, 0);
  }
  return fail(c, NLK_EUNSUP, "patch size %d not supported (4, 6, 8, 10, 12, 16)", g.psz);
}

}  // namespace

// patch sizes 17..32, and the lists of more than 128 entries that the fixed shapes are not instantiated for: every
// patch size and channel count with ch * psz^2 <= 4096 (GroupAny)
int nlk_launch_group_any(nlk_ctx* c, const NlkRecView& v, const NlkGeom& g, const float* img, const float* cur, const float* prev,
                         float* acc, const uint8_t* active) {
  if (c->deterministic) {
    if (g.psz > 16)
      return fail(c, NLK_EUNSUP, "deterministic aggregation is not available for patches above 16 x 16 (patch size %d)",
                  g.psz);
    if (g.kmax > 128 || g.gstride > 128)
      return fail(c, NLK_EUNSUP, "deterministic aggregation is not available for candidate lists of more than 128 "
                                 "entries (k = %d, group size = %d)", g.kmax, g.gstride);
    return fail(c, NLK_EUNSUP, "deterministic aggregation is not available in the generic group kernels (NLK_GENERIC_GROUP)");
  }
  if (g.psz > 32 || g.E > NLK_ANY_EMAX)
    return fail(c, NLK_EUNSUP, "patch size %d with %d channels not supported (patches up to 32 x 32, ch * psz^2 <= %d)",
                g.psz, g.ch, NLK_ANY_EMAX);
  return launch_group_lds<GroupAny>(c, v, g, img, cur, prev, acc, active, GroupAny::lds_bytes(g));
}

int nlk_launch_group_generic(nlk_ctx* c, const NlkRecView& v, const NlkGeom& g, const float* img, const float* cur,
                             const float* prev, float* acc, const uint8_t* active) {
  if (c->deterministic)
    return fail(c, NLK_EUNSUP, "deterministic aggregation is not available for candidate lists of more than 128 "
                               "entries (k = %d, group size = %d) or in the LDS-DCT kernel (NLK_GENERIC_GROUP)",
                g.kmax, g.gstride);
  if (g.ch == 1) return launch_group_ch<1>(c, v, g, img, cur, prev, acc, active);
  if (g.ch == 3) return launch_group_ch<3>(c, v, g, img, cur, prev, acc, active);
  return fail(c, NLK_EUNSUP, "%d channels not supported (1 or 3)", g.ch);
}
