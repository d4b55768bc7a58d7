// tu_group8.hip — launcher of k_group8m, the 8x8 group kernel (matrix cores): whether it can take a call, its DCT
// form, the tiles of a pass, which passes read packed lists, which instantiation runs, the launches
#include "group_det.h"
#include "k_gather.h"
#include "k_group8m.h"
#include "nlk_internal.h"

typedef void NlkGroup8mKernel(const float*, const float*, const float*, const uint8_t*, NlkGeom, NlkGTile, const uint32_t*,
                              const NlkTarget*, const uint32_t*, const uint8_t*, const float*, const float*, float*);

const void* nlk_group8m_ilp_kernel(int ch, bool smoother, int sep, bool packed);  // tu_group8_ilp.hip

// the kernel for (channels, smoother, DCT form, packed lists) if this unit holds it, else nullptr: every instantiation
// of this unit is named here and nowhere else. (<1, false, 2, 0, true> is not among them: one channel in the hybrid
// form - NLK_GROUP_SEP=2, no default - spills already)
const void* nlk_group8m_kernel(int ch, bool smoother, int sep, bool packed) {
#define NLK_K(C, SMO, SEP) \
  if (ch == C && smoother == SMO && sep == SEP && !packed) return (const void*)k_group8m<C, SMO, SEP>;
#define NLK_KP(C, SEP) \
  if (ch == C && !smoother && sep == SEP && packed) return (const void*)k_group8m<C, false, SEP, 0, true>;
  NLK_K(1, false, 0) NLK_K(1, false, 2) NLK_K(1, false, 6) NLK_K(1, true, 0) NLK_K(1, true, 2) NLK_K(1, true, 6)
  NLK_K(3, false, 0) NLK_K(3, false, 2) NLK_K(3, false, 6) NLK_K(3, true, 0) NLK_K(3, true, 2) NLK_K(3, true, 6)
  NLK_KP(1, 0) NLK_KP(1, 6) NLK_KP(3, 0) NLK_KP(3, 2) NLK_KP(3, 6)
#undef NLK_K
#undef NLK_KP
  return nullptr;
}

namespace {

// floats of the gain stash behind the accumulator planes (nlk_g8_stash_floats<CH, SEP>, k_group8m.h)
size_t stash_floats(int ch, int sep) {
  if (ch == 1) return sep == 0 ? nlk_g8_stash_floats<1, 0>() : sep == 2 ? nlk_g8_stash_floats<1, 2>() : nlk_g8_stash_floats<1, 6>();
  return sep == 0 ? nlk_g8_stash_floats<3, 0>() : sep == 2 ? nlk_g8_stash_floats<3, 2>() : nlk_g8_stash_floats<3, 6>();
}

// 1. Can k_group8m take the call? Else the packed-lane kernel does (nlk_launch_groupp_a)
bool group8m_takes(const nlk_ctx* c, const NlkGeom& g, const float* img, const float* cur, const float* prev) {
  // (k_group8m addresses every patch as planes base + a 32-bit byte offset: the call's images must lie in the
  // context's slab and the slab be smaller than 4 GiB - ~119 Mpixel of RGB; beyond that the packed-lane kernel)
  const float* lo = (const float*)c->planes.p;
  const float* hi = lo + c->planes.cap / sizeof(float);
  const bool inside = img >= lo && img < hi && cur >= lo && cur < hi && (!prev || (prev >= lo && prev < hi));
  if (!inside || c->planes.cap >= ((size_t)1 << 32)) return false;
  // (the smoother's pass B reads the difference image the layout kernel made of exactly these two images)
  if (g.smoother && prev && !(c->last.diff && cur == c->last.cur && prev == c->last.prev)) return false;
  return true;
}

// 2. The DCT form.
// the matrix-core kernel's DCTs: the Kronecker form on 16 x 16 products (rounds 2-4) or the separable form on
// 4 x 4 blocks (round 5), by pass - NLK_GROUP_SEP = 0: Kronecker in both passes, 2: Kronecker statistics,
// separable filter / inverse / aggregate (pass B), 6: separable in both; the default by mode is worked out below.
// Round 5's measurements, when the separable pass A still loaded a cache line per lane:
// Default by what was measured at 1080p RGB (profiles/r05_mode_times_1080p.txt, group kernel, Kronecker -> hybrid):
// FLT1 temporal 0.796 -> 0.740 ms, FLT1 spatial 1.043 -> 0.978; FLT2 (one member per group) 0.612 -> 0.628 and the
// smoother 1.281 -> 1.322 stay with the Kronecker form.
// Single-channel frames (`r05_mode_times_1080p_gray_by_sep.txt`; the separable pass B packs 16 members per step
// there): FLT1 temporal 0.514 (Kronecker) / 0.404 (2) / 0.393 (6), first frame 0.594 / 0.487 / 0.482, the smoother
// 0.926 / 0.547 / 0.576, FLT2 0.315 / 0.331 / 0.358.
// Round 6: the smoother's pass B reads the difference image previous - image (k_layout) - one row set per member
// instead of two - and with half the cache lines to fetch the separable pass B wins there too: SMO1 group at 1080p
// RGB 1.287 ms (Kronecker, two row sets) -> 1.234 (Kronecker, difference image) -> 1.101 (separable pass B).
// Round 6, later: the separable pass A loads a row as two halves in two ADJACENT lanes (one cache line per pair
// in each load: k_group8m.h, row_read) and the vector L1, which had kept it behind the Kronecker form, stops being
// what it waits for. Group ms at 1080p, forms 0 / 2 / 6 (`r06_mode_times_1080p_by_sep.txt`, `..._gray_by_sep.txt`):
// RGB FLT1 temporal 0.804 / 0.698 / 0.662, FLT2 0.607 / 0.612 / 0.576, first frame 1.125 / 0.894 / 0.894, smoother
// 1.207 / 0.971 / 0.992; one channel FLT1 temporal 0.534 / 0.413 / 0.384, FLT2 0.316 / 0.344 / 0.304, first frame
// 0.532 / 0.403 / 0.394, smoother 0.850 / 0.563 / 0.526. So: one channel 6 everywhere; RGB 6 for the filter's temporal
// frames, the hybrid form for first frames and the smoother (Kronecker for those with fewer than 4 members).
int dct_form(const nlk_ctx* c, const NlkGeom& g, const float* prev) {
  const int sep_default = g.ch == 1 ? 6 : (!g.smoother && prev) ? 6 : (g.ntagg < 4 ? 0 : 2);
  const int sep = nlk_or(c->sw.group_sep, sep_default);
  return (sep != 0 && sep != 6) ? 2 : sep;
}

// 3. The tiles of a pass: halo, targets per tile, LDS strides
int shape_pass(nlk_ctx* c, const NlkRecView& v, const NlkGeom& g, const float* prev, int sep, bool split, int pass,
               NlkGTile* out) {
  NlkGTile tl{};
  tl.pbase = (const float*)c->planes.p;
  // (the smoother's pass B transforms previous - image: laid out once per call by k_layout; `cur` is what gets filtered)
  tl.diff = (g.smoother && prev) ? c->last.diff : nullptr;
  tl.split = split;
  tl.far = pass;
  tl.chase = v.chase.words ? v.chase.reach : 0;
  tl.chase_test_skip0 = nlk_set(c->sw.chase_test_skip0);
  tl.chase_gen = v.chase.gen;
  tl.chase_row0 = v.chase.row0;
  tl.chase_rows = v.chase.rows;
  tl.chase_planes = v.chase.planes;
  tl.chase_words = v.chase.words;
  // LDS tile halo = reach of the dominant kind of group; without the split the rare spatial-branch
  // groups of a temporal frame that reach further fall back to HBM atomics
  tl.wmax = (g.smoother || g.have_prev) ? g.wsz_t : g.wsz_x;
  if (pass == 1) tl.wmax = g.wsz_x;
  // Targets per wavefront (NLK_GTX / NLK_GTY override for experiments), measured (profiles/README.md):
  // 3 x 1 on a 1080p grid (group 1.040 ms; 4 x 1 1.049, 2 x 1 1.068: a 3-target row needs 28 floats of
  // row stride like a 2-target one, 11 KB of LDS instead of 13), 2 x 1 on smaller grids (more, shorter
  // workgroups fill the chip better: 720p 0.499 vs 0.508 ms, 640 x 480 0.194 vs 0.221), one target while
  // the tiles would not even fill the ~2560 wavefronts the chip holds (256 x 256). With a wide halo the
  // tile would leave LDS room for ~1 wavefront per SIMD: 2 x 1 at most then.
  auto tiles_with = [&](int t) { return (size_t)((g.ngx + t - 1) / t) * g.ngy; };
  const int tgx_fill = tiles_with(3) >= 30000 ? 3 : (tiles_with(2) >= 2560 ? 2 : 1);
  // (round 4, first frames at 1080p - the spatial halo, 2 wavefronts per SIMD whatever the tile: 1 x 2 targets
  // 1.029 ms, 3 x 1 1.043, 3 x 2 1.042, 1 x 3 1.052, 2 x 2 1.090, 2 x 1 1.113 (the default until then), 1 x 4 1.113,
  // 1 x 1 1.143, 4 x 1 1.164, 1 x 6 1.185)
  const bool wide_full = tl.wmax > 6 && tgx_fill == 3 && pass == 0;
  // (round 6, after the tile's strides shrank its LDS footprint - first frames at 1080p RGB: 2 x 2 targets 0.896 ms,
  // 2 x 3 0.933, 3 x 2 0.935, 1 x 2 0.939 (the default until then), 2 x 1 0.938, 1 x 3 0.953, 1 x 4 1.008; 4K RGB 3.50
  // against 3.74; one channel 3 x 2 0.430, 2 x 3 0.433, 2 x 2 0.445, 1 x 2 0.47-0.50: tools/sweep_gt_spatial.sh)
  tl.tgx = nlk_or(c->sw.gtx, wide_full ? (g.ch == 1 ? 3 : 2) : min(tgx_fill, tl.wmax > 6 ? 2 : 4));
  // (round 3, matrix-core kernel with the leaner pass A, 1080p: 3 x 2 targets 0.957 ms, 2 x 2 0.970, 3 x 1 0.976,
  // 4 x 2 1.10, 2 x 3 1.05, 3 x 3 1.04 - two target rows share the tile's vertical halo: 40 % fewer flushed bytes;
  // round 4, straight-line aggregation: 3 x 2 0.831, 2 x 2 0.851, 3 x 1 0.869, 3 x 3 0.891, 4 x 2 0.993)
  tl.tgy = nlk_or(c->sw.gty, (tgx_fill == 3 && tl.wmax <= 6) || wide_full ? 2 : 1);
  tl.ntx = (g.ngx + tl.tgx - 1) / tl.tgx;
  tl.nty = (g.ngy + tl.tgy - 1) / tl.tgy;
  tl.nty_full = tl.nty;
  tl.single = 0;
  if ((tl.tgy > 1 || tl.tgx > 1) && !c->deterministic) {
    // The launch ends when its last tile does, and a 3 x 2 tile takes 1/7 of a 1080p launch (21600 tiles on 3072
    // wavefront slots): the chip would drain for most of a tile's time. So the last ~0.8 slots' worth of tiles
    // hold one grid row (3 x 1), and the last ~0.9 slots' worth of targets go one per workgroup
    // (1080p: 16 + 6 of 269 grid rows; group 0.950 -> 0.900 ms. NLK_G8_TAIL / NLK_G8_SINGLE override)
    int tail = tl.tgy == 1 ? 0 : nlk_or(c->sw.g8_tail, (2560 + tl.ntx / 2) / tl.ntx);
    int single = nlk_or(c->sw.g8_single, (2880 + g.ngx / 2) / g.ngx);
    single = max(0, min(single, g.ngy / 8));
    tail = max(0, min(tail, g.ngy / 4));
    tl.single = single;
    const int rows = g.ngy - tl.single;
    tl.nty_full = (rows - tail) / tl.tgy;
    tl.nty = tl.nty_full + (rows - tl.nty_full * tl.tgy);
  }
  tl.nmain = nlk_g8m_grid(tl.ntx, tl.nty);
  const int rw_max = (tl.tgx - 1) * g.step + 2 * tl.wmax + g.psz;
  tl.rh_max = (tl.tgy - 1) * g.step + 2 * tl.wmax + g.psz;
  if (sep != 0 && g.ch > 1) {
    // Separable pass B (round 6). A tile update is a ds_read_b32 / ds_write_b32 of lane
    // (column g4 = lane >> 4, plane spl = (lane >> 2) & 3, row si = lane & 3): the LDS serves a 4-byte access in
    // two groups of 32 lanes, {0-31} and {32-63}, on 32 banks (MI355X_MICROARCH.md, LDS) - and a half wavefront
    // holds all FOUR planes here, two columns and four rows. With the Kronecker layout's strides (below: plane
    // stride 16 mod 32) planes 0 / 2 and 1 / 3 of a half met on the same banks: a 2-way conflict on every one of
    // the 160 tile instructions of a target (SQ_LDS_BANK_CONFLICT 1.6e6 -> 3.1e7 per C2 launch when the
    // separable pass B came in round 5). Conflict-free: row stride = 2 (mod 4) - rows si give four different
    // multiples of 2, the two columns fill the odd banks - and plane stride = 8 (mod 16) (brute force over all
    // strides: tools/lds_banks.py). At 1080p the row stride is the region's own 26 floats (28 before) and the
    // workgroup's LDS falls from ten to nine 1280-byte pieces.
    tl.rwp = rw_max + ((2 - rw_max) % 4 + 4) % 4;
    tl.plane = tl.rwp * tl.rh_max;
    tl.plane += ((8 - tl.plane) % 16 + 16) % 16;
  } else {
    // Kronecker pass B (plane = lane >> 4, pixel (pi, pj) = lane & 15; also the 16-member steps of one-channel
    // frames, whose rounds touch two planes): one aggregation access = 4x4 pixels of each plane; row stride = 4
    // (mod 8) and plane stride = 16 (mod 32 banks) make the 32 lanes of a half wavefront hit 32 banks
    tl.rwp = rw_max + ((4 - rw_max) % 8 + 8) % 8;
    tl.plane = tl.rwp * tl.rh_max;
    tl.plane += ((16 - tl.plane) % 32 + 32) % 32;
  }
  // The kernel clears the planes and copies them to a slab as float4, and reads the gain stash behind them 16 bytes
  // per lane: both need the planes' floats to be a multiple of 4. One channel's two planes of 16 (mod 32) floats are;
  // three channels' four planes always are (the separable strides, 8 (mod 16), exist for three channels only).
  if ((size_t)(g.ch + 1) * tl.plane % 4 != 0)
    return fail(c, NLK_EUNSUP, "internal: %d planes of %d floats leave the tile's float4 accesses and its gain stash unaligned",
                g.ch + 1, tl.plane);
  *out = tl;
  return NLK_OK;
}

// 4. Does a pass read packed lists?
// The packed-list instantiation (k_group8m.h; the filter's kernels only), per launch: the match phase kept packed
// lists for these rows (nlk_hip.hip: plan_frame - a tiled matcher, NLK_PACKED_LISTS not 0), the lists of the call's
// dominant targets fit a record (nlk_packed_geom), the radius of the LDS window has a byte code, and the tile's
// records fit the two registers that hold them
bool reads_packed(const NlkRecView& v, const NlkGeom& g, int sep, const NlkGTile& tl) {
  return !g.smoother && v.packed && nlk_packed_geom(g) && tl.wmax <= NLK_PL_RMAX && tl.tgx * tl.tgy <= 8 &&
         !(g.ch == 1 && sep == 2);  // (one channel in the hybrid form - NLK_GROUP_SEP=2, no default - spills already)
}

}  // namespace

int nlk_launch_group8(nlk_ctx* c, const NlkRecView& v, const NlkGeom& g, const float* img, const float* cur, const float* prev,
                      float* acc, const uint8_t* active) {
  constexpr int PSZ = 8;
  if (g.ch != 1 && g.ch != 3) return fail(c, NLK_EUNSUP, "%d channels not supported (1 or 3)", g.ch);
  if (!group8m_takes(c, g, img, cur, prev)) {
    if (v.chase.words) return fail(c, NLK_EINVAL, "internal: mask replay handed to a group kernel that cannot run it");
    return nlk_launch_groupp_a(c, v, g, img, cur, prev, acc, active);
  }
  if (v.chase.words && c->deterministic)
    return fail(c, NLK_EINVAL, "internal: mask replay handed to a group kernel that cannot run it");
  const int sep = dct_form(c, g, prev);
  const bool split = nlk_det_split(c, g);
  if (nlk_or(c->sw.gtx, 1) < 1 || nlk_or(c->sw.gty, 1) < 1)
    return fail(c, NLK_EUNSUP, "NLK_GTX / NLK_GTY: a tile holds at least 1 x 1 targets");
  const int npass = split ? 2 : 1;
  NlkGTile tls[2];
  bool packed[2] = {false, false};
  int rc;
  for (int pass = 0; pass < npass; ++pass) {
    if ((rc = shape_pass(c, v, g, prev, sep, split, pass, &tls[pass]))) return rc;
    packed[pass] = reads_packed(v, g, sep, tls[pass]);
  }
  // (a tile's target records sit one per lane of its wavefront, and the kernel reads them back by lane number; the
  // LDS limit below would let a 65 x 1 tile through)
  for (int pass = 0; pass < npass; ++pass)
    if ((long)tls[pass].tgx * tls[pass].tgy > 64)
      return fail(c, NLK_EUNSUP, "%d x %d targets per tile: at most 64, one per lane", tls[pass].tgx, tls[pass].tgy);
  if (c->deterministic && (rc = nlk_det_plan(c, tls, npass, g.ch + 1, v.stream))) return rc;
  for (int pass = 0; pass < npass; ++pass) {
    const NlkGTile& tl = tls[pass];
    const size_t lds = sizeof(float) * ((size_t)(g.ch + 1) * tl.plane + stash_floats(g.ch, sep));
    if (lds > 160 * 1024) return fail(c, NLK_EUNSUP, "aggregation tile needs %zu bytes of LDS", lds);
    const void* k = nlk_group8m_kernel(g.ch, g.smoother, sep, packed[pass]);
    // (the same kernel compiled under the max-ilp scheduler, where that is the faster one: tu_group8_ilp.hip;
    // NLK_GROUP_ILP=0 keeps this unit's)
    if (nlk_or(c->sw.group_ilp, 1) != 0)
      if (const void* k2 = nlk_group8m_ilp_kernel(g.ch, g.smoother, sep, packed[pass])) k = k2;
    if (!k) return fail(c, NLK_EUNSUP, "internal: no k_group8m for %d channels, form %d%s", g.ch, sep, packed[pass] ? ", packed lists" : "");
    NlkGroup8mKernel* kern = reinterpret_cast<NlkGroup8mKernel*>(const_cast<void*>(k));
    HIPCHK(c, hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    const float* basis = (const float*)c->tabs.p;
    hipLaunchKernelGGL(kern, dim3(tl.nmain + ((tl.single * g.ngx + 7) / 8) * 8), dim3(64), lds, v.stream, img, cur, prev,
                       (const uint8_t*)c->vmap.p, g, tl, (const uint32_t*)v.topk,
                       (const NlkTarget*)v.tinfo, (const uint32_t*)v.gcoords,
                       active, basis, basis + PSZ * PSZ, acc);
    if (c->deterministic)
      nlk_launch_gather(v.stream, acc, tl.slab, tl.tflag, tl.tcount, g, tl, g.ch + 1);
    HIPCHK(c, hipGetLastError());
  }
  // what ran, for nlk_ctx_last_group_shape (include/nlk_hip.h); nothing reads it back on a launch path
  const NlkGTile& t0 = tls[0];
  const int report[12] = {NLK_GROUP_FAMILY_8M, sep, t0.tgx, t0.tgy, t0.ntx, t0.nty,
                          t0.nty_full, t0.single, npass, t0.chase, split ? tls[1].tgx : 0, split ? tls[1].tgy : 0};
  memcpy(c->group_shape, report, sizeof report);
  c->group_packed = (packed[0] ? 1 : 0) | (npass > 1 && packed[1] ? 2 : 0);
  return NLK_OK;
}
