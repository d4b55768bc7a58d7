// k_group_tile.h — what the tiled group kernels share: the launch's tile description (a kernel argument of
// k_group8m, k_groupp and the gather kernel) and the small lane helpers all of them use
//
// Aggregation. A workgroup is ONE wavefront that owns a tile of tgx x tgy targets
// and a private LDS accumulator tile (ch value planes + 1 weight plane, covering
// the tile plus the search halo). Being private, the tile is updated with plain
// ds_read / add / ds_write (LDS float atomics retire about one lane per clock on
// gfx950 and made an earlier, shared-tile version of the 8x8 kernel LDS-bound: see
// profiles/). The tile is flushed once with coalesced global float atomics,
// skipping untouched entries, which cuts the HBM atomic traffic ~10x compared
// with one global atomic per patch pixel (global float atomics run at a fixed
// ~1.3 TB/s of added bytes on MI355X and would otherwise bound the kernel).
#pragma once
#include "nlk_common.h"

struct NlkGTile {
  int tgx, tgy, ntx, nty;
  // k_group8m: tile rows of tgy grid rows; the tile rows after them hold ONE grid row each, and the last `single`
  // grid rows are worked through one target per workgroup, in the workgroups after `nmain` (end of the launch)
  int nty_full, single, nmain;
  int rwp, rh_max;  // LDS accumulator region: row stride / rows
  int wmax;         // halo of the LDS tile around its targets (groups reaching further spill to HBM atomics)
  int plane;        // k_group8m / k_groupp: floats per accumulator plane (padded, see there)
  // deterministic aggregation (k_gather.h): where workgroup `tile` writes its planes instead of adding
  // them to the frame accumulator with atomics, and the flag that says it did
  float* slab;      // [tiles][planes][plane]
  uint8_t* tflag;   // [tiles]
  int* tcount;      // [1 + nty]: flagged tiles of the launch / of every tile row (zeroed by the host)
  // A temporal frame has two kinds of groups: those searched with the temporal radius and the few
  // spatial-branch ones (no valid previous patch) that reach wsz_x. Deterministic mode runs them in
  // two launches with a tile halo each (far = 0: the former only, far = 1: the latter only), so that
  // no member ever leaves its tile.
  int split, far;   // split != 0: this launch takes only the targets of kind `far`
  // k_group8m: start of the allocation that holds every planar image of the call (nlk_ctx::planes, < 4 GiB):
  // patches are addressed as this base + a 32-bit byte offset
  const float* pbase;
  const float* diff;   // k_group8m, smoother: planar (previous - image) inside the same slab, or nullptr (then the kernel subtracts)
  // k_group8m, mask replay inside the launch (chase != 0): workgroup 0 first replays the processed mask of the grid
  // rows [0, chase_rows) from the bit planes (k_commit_rows.h) and publishes every row's decisions as
  // generation-tagged words; every workgroup polls the words of its own targets instead of reading `active`.
  // The launch's own first grid row is row chase_row0 of that grid (0 for a whole-frame call, a strip's first row).
  int chase;                     // 0, or the reach (1..3) of the grid whose replay this launch runs
  int chase_test_skip0;          // test hook (NLK_CHASE_TEST_SKIP0=1): workgroup 0 does NOT replay - every workgroup
                                 // must get its decisions by replaying the rows it needs itself
  int chase_row0, chase_rows;
  const uint32_t* chase_gen;     // the generation of this launch: a device word the bit-plane kernel has just advanced
                                 // (a kernel argument would be frozen into a captured HIP graph)
  const uint32_t* chase_planes;  // [rows][planes of that reach][64]
  uint64_t* chase_words;         // [rows][64]: generation << 32 | decision bits
};

// does this target's group reach beyond the temporal radius? (np0 = its candidates with a valid previous patch)
__device__ __forceinline__ bool nlk_far_target(const NlkGeom& g, int np0) {
  return g.have_prev && !g.smoother && np0 == 0;
}

typedef float nlk_f4u __attribute__((ext_vector_type(4), aligned(4)));

template <int CTRL>
__device__ __forceinline__ float nlk_dpp(float x) {
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), CTRL, 0xF, 0xF, true));
}
#define NLK_DPP_XOR1 0xB1   // quad_perm [1,0,3,2]
#define NLK_DPP_XOR2 0x4E   // quad_perm [2,3,0,1]
#define NLK_DPP_XOR3 0x1B   // quad_perm [3,2,1,0]
#define NLK_DPP_HMIRROR 0x141  // lane u <- lane u ^ 7 inside each group of 8
#define NLK_DPP_ROR8 0x128     // lane l <- lane l ^ 8 inside each row of 16

__device__ __forceinline__ float nlk_wave_sum8(float v) {
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}
