// group_det.h — deterministic aggregation (k_gather.h), host side: whether a call splits into two passes, and where
// every pass of a launch keeps its slabs, "written" flags and tile-row counters (tu_group8.hip, groupp_launch.h)
#pragma once
#include "k_group_tile.h"
#include "nlk_internal.h"

// Deterministic mode runs a temporal frame's far-reaching (spatial-branch) groups in a second
// launch whose tiles have the spatial halo, so that no member ever leaves its tile (k_group_tile.h)
static inline bool nlk_det_split(const nlk_ctx* c, const NlkGeom& g) {
  return c->deterministic && g.have_prev && !g.smoother && g.wsz_x > g.wsz_t;
}

// Slabs, "written" flags and tile-row counters of ALL passes of a launch, sized from each pass's OWN tiles (ntx, nty,
// plane) and reserved before the first launch (growing a buffer frees it); the counters are cleared on `stream`.
// c->slab: the passes' slabs one after the other. c->tflag: the flags of all passes, then, 16-byte aligned, 1 + nty
// counters per pass. (Round 3 sized the far pass with the near pass's tile rows - half as many since the near tiles
// hold two grid rows - and its counters likewise: writes past the end that the allocation slack hid; found with
// NLK_DEBUG_GUARD=1.)
static inline int nlk_det_plan(nlk_ctx* c, NlkGTile* tls, int npass, int planes, hipStream_t stream) {
  size_t need = 0, nflag = 0, ncnt = 0;
  for (int pass = 0; pass < npass; ++pass) {
    const size_t ntiles = (size_t)tls[pass].ntx * tls[pass].nty;
    need += ntiles * planes * tls[pass].plane;
    nflag += ntiles;
    ncnt += 1 + (size_t)tls[pass].nty;
  }
  const size_t cnt_off = (nflag + 15) & ~(size_t)15, cnt_bytes = sizeof(int) * ncnt;
  int rc;
  if ((rc = reserve(c, c->slab, sizeof(float) * need)) || (rc = reserve(c, c->tflag, cnt_off + cnt_bytes))) return rc;
  HIPCHK(c, hipMemsetAsync((uint8_t*)c->tflag.p + cnt_off, 0, cnt_bytes, stream));
  float* slab = (float*)c->slab.p;
  uint8_t* tflag = (uint8_t*)c->tflag.p;
  int* tcount = (int*)((uint8_t*)c->tflag.p + cnt_off);
  for (int pass = 0; pass < npass; ++pass) {
    const size_t ntiles = (size_t)tls[pass].ntx * tls[pass].nty;
    tls[pass].slab = slab;
    tls[pass].tflag = tflag;
    tls[pass].tcount = tcount;
    slab += ntiles * planes * tls[pass].plane;
    tflag += ntiles;
    tcount += 1 + tls[pass].nty;
  }
  return NLK_OK;
}
