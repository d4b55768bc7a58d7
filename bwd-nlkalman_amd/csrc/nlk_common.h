// nlk_common.h — shared definitions of the gfx950 kernels (device + host side).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// Geometry + parameters of one frame (or row strip) call, passed by value to
// every kernel. Images are planar on the device: plane c at img + c*h*w.
struct NlkGeom {
  int w, h, ch;            // strip size (h includes the search halo rows)
  int psz, step, p2, E;    // patch size, grid step psz/2, psz^2, ch*psz^2
  int ngx, ngy, oy;        // target grid: x = gx*step, y = oy + gy*step
  int wsz_x, wsz_t;        // search radii (reference: src/nlkalman.c:637)
  int npx, npt, ntagg;     // k for spatial / temporal targets, group size
  int R;                   // reach of a group on the patch grid: max(wsz)/step
  int kmax;                // row stride of the top-k record
  int gstride;             // row stride of the group-coordinate record (>= 1)
  int have_prev, have_basic, smoother;
  float sigma2, beta_x, beta_t;
};

// Launch shape of a tiled block-matching kernel (k_match.h), passed by value beside NlkGeom; planned by
// nlk_match_plan (tu_match.hip)
struct NlkTile {
  int tgx, tgy;       // targets per tile
  int bx;             // targets per block along x: 4, or 2 (k_bm_topk<.., 2>: 12 x 12 patches, 8 wavefronts on an 8 x 4 tile)
  int ntx, nty;       // tiles
  int rwp, rh_max;    // LDS region: padded row stride (floats) / rows
  int ksel_max;       // capacity of the per-wave survivor arrays
  int halo;           // search halo held in LDS (windows reaching further read HBM/L2)
  int block;          // 4 x 2-target blocks share their squared differences (0: NLK_MATCH_NOBLOCK, target by target)
  int threads;        // k_bm_topk: threads per workgroup (256, or 512: 8 wavefronts with a block of 2 x 2 targets each)
  int order;          // summation order of the distances: 0 = the reference's (exact), 1 = block-summed (opt-in; 8 x 8 patches)
  int packed;         // != 0: the targets' packed lists (below) are written and flagged
};

// per-target record written by the matching kernel
struct NlkTarget {
  int nsel;   // number of kept candidates (0: nothing to do)
  int np0;    // kept candidates with a valid previous patch
  int nagg;   // group members that are filtered and aggregated
  int flags;  // bit0: prev_p, bit1: group marks the processed-mask, bit2: the packed lists of this target are valid
  uint64_t vbits[2];  // bit i: kept candidate i (< 128) has a valid previous patch
  uint32_t pl[16];    // the packed lists (below; NLK_PL_DWORDS words), valid where flags has NLK_TF_PACKED
};
#define NLK_TF_PACKED 4  // NlkTarget::flags
// the head of a target's record, field by field (the packed lists behind it are written by other lanes, or not at all)
static __device__ inline void nlk_target_store(NlkTarget* o, int nsel, int np0, int nagg, int flags, uint64_t v0, uint64_t v1) {
  o->nsel = nsel; o->np0 = np0; o->nagg = nagg; o->flags = flags;
  o->vbits[0] = v0; o->vbits[1] = v1;
}

// Packed lists: beside topk / gcoords the tiled matchers leave every target's two lists as displacements from the
// target's own pixel position, one byte per entry - (dy + r) << 4 | (dx + r), r = the search radius the target
// used - in a record of NLK_PL_DWORDS words inside the target's own record (NlkTarget::pl: no pointer of its own, which
// the 64-register matchers have no scalar registers to spare for): words 0-7 candidates 0..31 in list order, words 8-15 group members
// 0..31 in gcoords order (entry i in byte i & 3 of word i >> 2; bytes past a list's end are not written). A record is
// valid (NLK_TF_PACKED) when both lists have at most NLK_PL_MAX entries and r <= NLK_PL_RMAX: every entry lies in the
// target's window and therefore encodes.
// k_group8m reads a whole tile's records with two loads (k_group8m.h).
#define NLK_PL_DWORDS 16
#define NLK_PL_MAX 32
#define NLK_PL_RMAX 7
// The pair below is what the matcher's epilogue (k_match.h), k_group8m's packed-list instantiation (k_group8m.h) and
// the host entry point of the CPU test (nlk_host_packed_entry) all call.
// Encode: with q = x | y << 16 (nlk_pack_xy) and the target at (px, py), q + (r - px) + ((r - py) << 16) is
// (x - px + r) | (y - py + r) << 16 - one add, no borrow between the halves for an entry inside the window - and the
// byte is its two low nibbles folded together. nlk_pl_word is that sum, nlk_pl_encodes says whether it IS a byte of
// radius r (both halves in 0..2 r), nlk_pl_byte folds it.
static __host__ __device__ inline uint32_t nlk_pl_word(uint32_t q, int px, int py, int r) {
  return q + ((uint32_t)(r - px) + ((uint32_t)(r - py) << 16));
}
static __host__ __device__ inline bool nlk_pl_encodes(uint32_t word, int r) {
  return r >= 0 && r <= NLK_PL_RMAX && (word & 0xffffu) <= (uint32_t)(2 * r) && (word >> 16) <= (uint32_t)(2 * r);
}
static __host__ __device__ inline uint32_t nlk_pl_byte(uint32_t word) { return (word | (word >> 12)) & 0xffu; }
// Decode: the frame coordinate (nlk_pack_xy) of the entry with this byte, for the target at (px, py)
static __host__ __device__ inline uint32_t nlk_pl_decode(uint32_t byte, int px, int py, int r) {
  return (uint32_t)(px - r + (int)(byte & 15u)) | ((uint32_t)(py - r + (int)(byte >> 4)) << 16);
}
// May a target with k kept candidates (its member list is never the longer one) that searched radius r have a valid
// record? `passthrough`: the smoother's target without a valid previous patch, whose member is the target itself
static __host__ __device__ inline bool nlk_pl_target_fits(int k, int r, bool passthrough) {
  return k <= NLK_PL_MAX && r <= NLK_PL_RMAX && !passthrough;
}
// the radius a target searched with (reference: src/nlkalman.c:637), from its prev_p flag
static __host__ __device__ inline int nlk_target_radius(const NlkGeom& g, int prev_p) {
  return (g.smoother || prev_p) ? g.wsz_t : g.wsz_x;
}

static __host__ __device__ inline uint32_t nlk_pack_xy(int x, int y) {
  return (uint32_t)x | ((uint32_t)y << 16);
}
static __host__ __device__ inline int nlk_x(uint32_t p) { return (int)(p & 0xffffu); }
static __host__ __device__ inline int nlk_y(uint32_t p) { return (int)(p >> 16); }

// XCD-aware tile order. Workgroups are dealt round-robin over the 8 XCDs (blocks
// b and b+8 share an XCD and its L2, MI355X_MICROARCH.md), so block b takes tile
// (b % 8) * ceil(n/8) + b / 8: every XCD works through one contiguous band of
// tiles and re-reads of neighbouring rows hit its own L2. The grid is launched
// with 8 * ceil(n/8) blocks; the mapping is a bijection onto [0, 8*ceil(n/8)),
// indices >= n have no tile. Only speed depends on the actual placement.
static __device__ inline int nlk_xcd_tile(int b, int n) {
  const int per = (n + 7) >> 3;
  return (b & 7) * per + (b >> 3);
}
static inline int nlk_xcd_grid(int n) { return ((n + 7) >> 3) << 3; }

// LDS written by some lanes of a wavefront and read by others of the SAME wavefront: order the
// accesses without a workgroup barrier
__device__ inline void nlk_wave_lds_fence() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_s_waitcnt(0xC07F);  // lgkmcnt(0)
  __builtin_amdgcn_wave_barrier();
}
// The same without the wait: the LDS executes the DS instructions of one wavefront in the order
// they were issued, so a read issued after a write of the same wavefront returns the written
// data; only the COMPILER must be kept from moving the read above the write (the wait for the
// data itself is the ordinary lgkmcnt wait in front of its first use).
__device__ inline void nlk_wave_lds_order() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
}
