// groupp_launch.h — host-side launcher of k_groupp<PSZ, SMO> (included by the tu_groupp_*.hip units,
// each of which instantiates a range of patch sizes so that `make -j` compiles them side by side)
#pragma once
#include "group_det.h"
#include "k_gather.h"
#include "k_groupp.h"
#include "nlk_internal.h"

template <int PSZ>
static int nlk_groupp_launch_t(nlk_ctx* c, const NlkRecView& v, const NlkGeom& g, const float* img, const float* cur,
                               const float* prev, float* acc, const uint8_t* active) {
  typedef NlkPP<PSZ> K;
  const bool split = nlk_det_split(c, g);
  const int npass = split ? 2 : 1;
  NlkGTile tls[2];
  size_t lds[2];
  for (int pass = 0; pass < npass; ++pass) {
    NlkGTile tl{};
    tl.split = split;
    tl.far = pass;
    // LDS tile halo = reach of the dominant kind of group; without the split the rare spatial-branch
    // groups of a temporal frame that reach further go to HBM atomics
    tl.wmax = (g.smoother || g.have_prev) ? g.wsz_t : g.wsz_x;
    if (pass == 1) tl.wmax = g.wsz_x;
    tl.tgx = tl.tgy = 1;  // one target per workgroup
    tl.ntx = g.ngx;
    tl.nty = g.ngy;
    const int rw_max = 2 * tl.wmax + g.psz;
    tl.rh_max = rw_max;
    // one aggregation access = PSZ rows x NBK blocks of PB pixels (lane = NBK * row + block): the row
    // stride with the fewest bank collisions among those addresses (two halves of 32 lanes)
    int best = 1 << 30;
    tl.rwp = rw_max;
    for (int r = rw_max; r < rw_max + 8; ++r) {
      int cost = 0;
      for (int half = 0; half < 2; ++half) {
        int cnt[32] = {0}, mx = 0;
        for (int l = 32 * half; l < 32 * half + 32 && l < PSZ * K::NBK; ++l) {
          const int v = ++cnt[((l / K::NBK) * r + K::PB * (l % K::NBK)) & 31];
          mx = v > mx ? v : mx;
        }
        cost += mx;
      }
      cost = cost * 64 + (r - rw_max);  // (ties: the narrowest)
      if (cost < best) { best = cost; tl.rwp = r; }
    }
    tl.plane = (tl.rwp * tl.rh_max + 3) & ~3;
    lds[pass] = sizeof(float) * ((size_t)2 * tl.plane + K::SCRATCH + K::gains(g.ch));
    if (lds[pass] > 160 * 1024) return fail(c, NLK_EUNSUP, "aggregation tile needs %zu bytes of LDS", lds[pass]);
    tls[pass] = tl;
  }
  int rc;
  if (c->deterministic && (rc = nlk_det_plan(c, tls, npass, g.ch + 1, v.stream))) return rc;
  for (int pass = 0; pass < npass; ++pass) {
    const NlkGTile& tl = tls[pass];
    auto kern = g.smoother ? k_groupp<PSZ, true> : k_groupp<PSZ, false>;
    HIPCHK(c, hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds[pass]));
    const float* basis = (const float*)c->tabs.p;
    hipLaunchKernelGGL(kern, dim3(nlk_xcd_grid(g.ngx * g.ngy)), dim3(64), lds[pass], v.stream, img, cur, prev, g, tl,
                       (const uint32_t*)v.topk, (const NlkTarget*)v.tinfo, (const uint32_t*)v.gcoords,
                       active, basis, basis + PSZ * PSZ, acc);
    if (c->deterministic)
      nlk_launch_gather(v.stream, acc, tl.slab, tl.tflag, tl.tcount, g, tl, g.ch + 1);
    HIPCHK(c, hipGetLastError());
  }
  return NLK_OK;
}
