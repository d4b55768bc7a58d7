// tu_match.hip — the host side of block matching: the plan of a call's match launches (nlk_match_plan: generic or
// tiled, the tiles' shapes, LDS bytes and rounds; a plain function of geometry and switches, shown to the tests by
// nlk_host_match_plan), the one launcher the frame pipeline calls (nlk_launch_match: generic kernel, or dominant and
// wide launch), the dispatcher over the tiled launchers (tu_match_a..f.hip, one range of patch sizes each) and the
// launcher of the generic kernel (k_match_generic.h)
#include "k_match.h"
#include "k_match_generic.h"
#include "nlk_internal.h"

#define NLK_MATCH_DECL(P) \
  int nlk_launch_match_p##P(nlk_ctx*, const NlkRecView&, const NlkGeom&, const NlkTile&, size_t, const float*, int, bool);
NLK_MATCH_DECL(4) NLK_MATCH_DECL(6) NLK_MATCH_DECL(8) NLK_MATCH_DECL(10) NLK_MATCH_DECL(12) NLK_MATCH_DECL(16)
int nlk_launch_match_p8_bs(nlk_ctx*, const NlkRecView&, const NlkGeom&, const NlkTile&, size_t, const float*, int,
                           bool);  // tu_match_f.hip

namespace {

constexpr size_t LDS_LIMIT = 160 * 1024;

// rounds of 64 candidates the window of radius r takes
int window_rounds(int r) { return ((2 * r + 1) * (2 * r + 1) + 63) / 64; }

// the radius of the call's dominant window - the one the tile holds in LDS - and of the widest any target searches
int dominant_radius(const NlkGeom& g) { return (g.smoother || g.have_prev) ? g.wsz_t : g.wsz_x; }
int widest_radius(const NlkGeom& g) { return g.smoother ? g.wsz_t : (g.have_prev ? max(g.wsz_x, g.wsz_t) : g.wsz_x); }

// the tiled matching kernels exist for patch sizes 4 / 6 / 8 / 10 / 12 / 16, 1 or 3 channels and
// windows of up to 1024 candidates; everything else the reference accepts goes to k_bm_generic
bool generic_by_shape(const NlkGeom& g, const NlkSwitches& sw) {
  return !nlk_fixed_shape(g.psz, g.ch) || window_rounds(widest_radius(g)) > 16 || nlk_set(sw.generic_match);
}

// 8 x 4 targets per workgroup, four 4 x 2 blocks that share their squared differences. A small grid
// (fewer than ~2 such tiles per CU: 256 x 256, 512 x 384, a 34-row strip of a 1080p frame) is latency bound
// instead: 4 x 2 tiles, one target at a time, two targets per wavefront (C1: match 0.058 -> 0.02 ms).
// Where the two meet (round 4, temporal / first-frame match ms, blocks against target by target): 384 tiles
// 0.059 / 0.144 against 0.053 / 0.141; 486: 0.061 / 0.148 against 0.060 / 0.178; 600 (640 x 480): 0.071 / 0.188
// against 0.071 / 0.221; 950 (800 x 600): 0.087 / 0.241 against 0.095 / 0.302; 1020 (960 x 540, and the 67-row
// strips of four GPUs): 0.085 / 0.249 against 0.101 / 0.330. (Until then the limit was 1024 tiles.)
bool small_grid(const NlkGeom& g) { return (size_t)((g.ngx + 7) / 8) * ((g.ngy + 3) / 4) < 576; }

// targets per tile, and whether its blocks of targets share their squared differences
void tile_targets(const NlkGeom& g, const NlkSwitches& sw, NlkTile& tl) {
  const bool small = small_grid(g);
  tl.tgx = nlk_or(sw.mtx, small ? 4 : 8);
  tl.tgy = nlk_or(sw.mty, small ? 2 : 4);
  tl.ntx = (g.ngx + tl.tgx - 1) / tl.tgx;
  tl.block = nlk_set(sw.match_noblock) ? 0 : (nlk_set(sw.match_block) ? 1 : !small);
  // the opt-in block-summed distance order (NLK_MATCH_ORDER=block; 8 x 8 patches, k_bm_topk / k_bm_wide); everything
  // else - and the default - sums in the reference's order
  tl.order = (nlk_or(sw.match_order, 0) == 1 && g.psz == 8) ? 1 : 0;
}

// Wavefronts per workgroup and targets per block.
// 8 wavefronts per workgroup where the search radius is the temporal one (FLT1 / FLT2 temporal, SMO1), measured at
// 1080p, match ms with 8 x 8 patches: 8 x 4 tile, 4 wavefronts, blocks of 4 x 2 targets 0.305 (20 wavefronts per CU);
// 8 x 8 tile, 8 wavefronts, 4 x 2 blocks 0.294 (45 KB: three per CU = 24; tried and dropped); 8 x 4 tile, 8 wavefronts
// with a block of 2 x 2 targets each, 64 registers 0.268 (30 KB: four per CU = 32, a fifth more subtractions and
// multiplications) - the default. 10 x 10 patches and more: the same 2 x 2 blocks (4K, 12 x 12: 0.864 -> 0.762,
// 16 x 16: 1.22 -> 0.91). With the spatial radius the tiles are too large for more than the four wavefronts (8 x 8 tile
// 62 KB: 0.95 -> 1.22) - except the seven-round blocks of a first frame at 8 x 8, 441 candidates: 2 x 2 targets per
// block need 128 registers instead of 168 + spills, two 8-wavefront workgroups per CU instead of three of 4: match
// 0.947 -> 0.828. NLK_MATCH_BX2=0 keeps the 4 x 2 blocks.
void tile_blocks(const NlkGeom& g, const NlkSwitches& sw, NlkTile& tl) {
  const bool tiles84 = tl.tgx == 8 && tl.tgy == 4 && (nlk_set(sw.match_block) || !small_grid(g));  // (the tiles of a full-size frame)
  const bool bx2 = nlk_or(sw.match_bx2, 1) != 0 && tiles84 &&
                   nlk_bm_has_bx2(g.psz, nlk_bm_rounds_class(window_rounds(dominant_radius(g))));
  tl.threads = bx2 ? 512 : NLK_BM_THREADS;
  tl.bx = bx2 ? 2 : 4;
}

// LDS row stride of a region `need` floats wide whose windows are `width` candidates wide: = width (mod 32), so that
// candidate i of a window sits on bank i mod 32 and a wavefront's 64 candidate reads are conflict free
int padded_stride(int need, int width) { return need + ((width - need) % 32 + 32) % 32; }

// the LDS region of the tile: its targets' patches and the halo of the dominant window
void tile_region(const NlkGeom& g, NlkTile& tl) {
  tl.halo = dominant_radius(g);
  tl.rwp = padded_stride((tl.tgx - 1) * g.step + 2 * tl.halo + g.psz, 2 * tl.halo + 1);
  tl.rh_max = (tl.tgy - 1) * g.step + 2 * tl.halo + g.psz;
  tl.ksel_max = g.kmax;
}

// the tile of the wide launch: one wavefront per queued target, its own window of the spatial radius
NlkTile wide_tile(const NlkGeom& g, const NlkTile& tl) {
  NlkTile tw = tl;
  tw.halo = g.wsz_x;
  tw.rh_max = 2 * g.wsz_x + g.psz;
  tw.rwp = padded_stride(tw.rh_max, 2 * g.wsz_x + 1);
  return tw;
}

// the generic kernel: any patch size / channel count / search radius (k_match.h: k_bm_generic)
int launch_match_generic(nlk_ctx* c, const NlkRecView& v, const NlkGeom& g, const float* img) {
  const int wfull = 2 * max(g.wsz_x, g.wsz_t) + 1;
  const size_t lds = 8 * (size_t)g.kmax + 4 * (size_t)g.kmax + 4 * (size_t)g.gstride + 4 * (size_t)wfull * wfull + 16;
  if (lds > LDS_LIMIT)
    return fail(c, NLK_EUNSUP, "search window of %d candidates with k = %d needs %zu bytes of LDS (> 160 KiB)",
                wfull * wfull, g.kmax, lds);
  HIPCHK(c, hipFuncSetAttribute((const void*)k_bm_generic, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(k_bm_generic, dim3(nlk_xcd_grid(g.ngx * g.ngy)), dim3(64), lds, v.stream, img,
                     (const uint8_t*)c->vmap.p, g, g.kmax, v.topk, v.tinfo, v.gcoords, v.marks);
  HIPCHK(c, hipGetLastError());
  return NLK_OK;
}

// one tiled launch: the dominant one (k_bm_topk) or the wide one (k_bm_wide)
int launch_match_tiled(nlk_ctx* c, const NlkRecView& v, const NlkGeom& g, const NlkTile& tl, size_t lds,
                       const float* img, int maxm, bool wide) {
  if (tl.order == 1 && g.psz == 8) return nlk_launch_match_p8_bs(c, v, g, tl, lds, img, maxm, wide);
  switch (g.psz) {
    case 4: return nlk_launch_match_p4(c, v, g, tl, lds, img, maxm, wide);
    case 6: return nlk_launch_match_p6(c, v, g, tl, lds, img, maxm, wide);
    case 8: return nlk_launch_match_p8(c, v, g, tl, lds, img, maxm, wide);
    case 10: return nlk_launch_match_p10(c, v, g, tl, lds, img, maxm, wide);
    case 12: return nlk_launch_match_p12(c, v, g, tl, lds, img, maxm, wide);
    case 16: return nlk_launch_match_p16(c, v, g, tl, lds, img, maxm, wide);
  }
  return fail(c, NLK_EUNSUP, "patch size %d not supported (4, 6, 8, 10, 12, 16)", g.psz);
}

}  // namespace

int nlk_match_plan(const NlkGeom& g, const NlkSwitches& sw, NlkMatchPlan* mp) {
  *mp = NlkMatchPlan{};
  NlkTile& tl = mp->tl;
  mp->generic = generic_by_shape(g, sw);
  tile_targets(g, sw, tl);
  tile_blocks(g, sw, tl);
  tile_region(g, tl);
  mp->lds = nlk_bm_topk_lds(tl, g.ch, g.gstride);
  if (mp->lds > LDS_LIMIT && tl.threads > NLK_BM_THREADS && tl.tgy == 4) {
    // (very long lists: the per-wavefront list space of 8 wavefronts does not fit beside the tile - 4 wavefronts, 4 x 2 blocks)
    tl.threads = NLK_BM_THREADS;
    tl.bx = 4;
    mp->lds = nlk_bm_topk_lds(tl, g.ch, g.gstride);
  }
  if (mp->lds > LDS_LIMIT) mp->generic = true;  // (a k or window too large for the tile: the generic kernel)
  mp->maxm = window_rounds(tl.halo);
  // targets of a temporal frame without a valid previous patch search the spatial window
  // (reference: :637); when that one is the wider, they are queued for a second launch
  if (!mp->generic && g.have_prev && !g.smoother && g.wsz_x > g.wsz_t) {
    mp->tw = wide_tile(g, tl);
    mp->lds_w = nlk_bm_wide_lds(mp->tw, g.ch, g.gstride);
    mp->maxm_w = window_rounds(g.wsz_x);
    mp->wide = mp->lds_w <= LDS_LIMIT;
    if (!mp->wide) mp->generic = true;
  }
  return NLK_OK;
}

int nlk_launch_match(nlk_ctx* c, const NlkRecView& v, const NlkGeom& g, const NlkMatchPlan& mp, bool clear_queue,
                     const float* img) {
  if (mp.generic) return launch_match_generic(c, v, g, img);
  NlkTile tl = mp.tl;
  tl.nty = (g.ngy + tl.tgy - 1) / tl.tgy;
  if (mp.wide && clear_queue) HIPCHK(c, hipMemsetAsync(v.wide, 0, sizeof(uint32_t), v.stream));
  int rc = launch_match_tiled(c, v, g, tl, mp.lds, img, mp.maxm, false);
  if (rc || !mp.wide) return rc;
  NlkTile tw = mp.tw;
  tw.nty = tl.nty;
  return launch_match_tiled(c, v, g, tw, mp.lds_w, img, mp.maxm_w, true);
}

extern "C" int nlk_host_match_plan(int w, int h, int ch, const struct nlkalman_params* P, int smoother, int have_prev,
                                   int rows, int out[NLK_MATCH_PLAN_FIELDS]) {
  if (!P || !out) return fail(nullptr, NLK_EINVAL, "null parameters / output");
  struct nlk_frame_grid fg;
  if (rows == 0 && nlk_frame_grid(w, h, P, smoother, have_prev, &fg) == NLK_OK) rows = fg.ngy;  // (if not: nlk_frame_geom says why)
  NlkGeom g{};
  int rc = nlk_frame_geom(nullptr, g, w, h, ch, 0.f, P, 0, rows, smoother, have_prev != 0, false);
  if (rc) return rc;
  NlkSwitches sw;
  sw.load();
  NlkMatchPlan mp;
  if ((rc = nlk_match_plan(g, sw, &mp))) return rc;
  const NlkTile &tl = mp.tl, &tw = mp.tw;
  const int f[NLK_MATCH_PLAN_FIELDS] = {
      mp.generic, mp.wide, tl.tgx, tl.tgy, tl.bx, tl.threads, tl.block, tl.order, tl.halo, tl.rwp, tl.rh_max,
      tl.ksel_max, tl.ntx, nlk_bm_rounds_class(mp.maxm), (int)mp.lds,
      mp.wide ? tw.halo : 0, mp.wide ? tw.rwp : 0, mp.wide ? tw.rh_max : 0,
      mp.wide ? nlk_bm_rounds_class(mp.maxm_w) : 0, mp.wide ? (int)mp.lds_w : 0};
  memcpy(out, f, sizeof f);
  return NLK_OK;
}
