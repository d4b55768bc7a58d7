// nlk_internal.h — what the translation units of libnlk_hip.so share: the context, error helpers,
// scratch-buffer growth and the launchers each unit exports to the frame pipeline (tu_frame.hip). (The library is built
// from several .hip files so that `make -j` compiles the big kernels in parallel.)
#pragma once
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/nlk_hip.h"
#include "nlk_common.h"

struct NlkTvMail;   // k_tvl1.h
struct NlkGTile;    // k_group_tile.h

struct NlkBuf {
  void* p = nullptr;
  size_t cap = 0;
  void* base = nullptr;  // what hipMalloc returned (NLK_DEBUG_GUARD: p sits at the END of the allocation)
};

// the mask replay a group launch runs itself (k_group8m, NlkGTile::chase): bit planes, tagged decision words and
// generation counter of the grid rows [0, rows); the launch's own first row is grid row row0
struct NlkChase {
  const uint32_t* planes = nullptr;
  uint64_t* words = nullptr;
  const uint32_t* gen = nullptr;
  int reach = 0, row0 = 0, rows = 0;
};

// what a launcher works on: the stream and the per-target records of the patch-grid rows it is
// given (the whole grid, a strip, or one band of a frame processed in bands on two streams)
struct NlkRecView {
  hipStream_t stream = nullptr;
  uint32_t* topk = nullptr;      // [targets][kmax]
  NlkTarget* tinfo = nullptr;    // [targets]
  uint32_t* gcoords = nullptr;   // [targets][gstride]
  bool packed = false;           // the match phase keeps packed lists in the target records (nlk_common.h)
  uint64_t* marks = nullptr;     // [targets]
  uint32_t* wide = nullptr;      // [0] = queue length, then the queued targets (k_bm_wide)
  NlkChase chase;                // words != nullptr: the group kernel is to replay the processed mask itself
};

// The NLK_* environment switches (variants for comparison tests and experiments, none
// needed in production) are read ONCE, when a context is created - not on every frame call - and again only
// on request (nlk_ctx_reload_switches: the tests change the environment under a live context).
// A field holds atoi(value), or NLK_UNSET when the variable does not exist.
#define NLK_UNSET (-2147483647 - 1)
#define NLK_SWITCH_LIST(X)                                                                                   \
  X(deterministic, "NLK_DETERMINISTIC") X(generic_group, "NLK_GENERIC_GROUP") X(group_packed, "NLK_GROUP_PACKED") \
  X(group_sep, "NLK_GROUP_SEP") X(group_ilp, "NLK_GROUP_ILP") X(generic_match, "NLK_GENERIC_MATCH") X(mtx, "NLK_MTX") X(mty, "NLK_MTY")    \
  X(match_bx2, "NLK_MATCH_BX2") X(match_block, "NLK_MATCH_BLOCK")              \
  X(match_noblock, "NLK_MATCH_NOBLOCK") X(match_order, "NLK_MATCH_ORDER") X(commit_wave, "NLK_COMMIT_WAVE")    \
  X(commit_band, "NLK_COMMIT_BAND") X(no_chase, "NLK_NO_CHASE") X(chase_test_skip0, "NLK_CHASE_TEST_SKIP0") X(bands, "NLK_BANDS") X(host_bands, "NLK_HOST_BANDS")                    \
  X(host_trace, "NLK_HOST_TRACE") X(gtx, "NLK_GTX") X(gty, "NLK_GTY") X(g8_tail, "NLK_G8_TAIL")              \
  X(g8_single, "NLK_G8_SINGLE") X(packed_lists, "NLK_PACKED_LISTS") X(tv_wg_pixels, "NLK_TV_WG_PIXELS") X(tv_unblocked, "NLK_TV_UNBLOCKED")      \
  X(tv_shape, "NLK_TV_SHAPE") X(tv_inline, "NLK_TV_INLINE") X(tv_look, "NLK_TV_LOOK") X(tv_trace, "NLK_TV_TRACE")
struct NlkSwitches {
#define NLK_X(field, name) int field = NLK_UNSET;
  NLK_SWITCH_LIST(NLK_X)
#undef NLK_X
  void load() {
#define NLK_X(field, name) { const char* e_ = getenv(name); field = e_ ? atoi(e_) : NLK_UNSET; }
    NLK_SWITCH_LIST(NLK_X)
#undef NLK_X
    // NLK_MATCH_ORDER = exact | block (or 0 | 1): the summation order of the patch distances (k_match.h)
    if (const char* e_ = getenv("NLK_MATCH_ORDER")) match_order = (!strcmp(e_, "block") || atoi(e_) == 1) ? 1 : 0;
  }
};
static inline bool nlk_set(int v) { return v != NLK_UNSET; }                 // the variable exists (any value)
static inline int nlk_or(int v, int dflt) { return v != NLK_UNSET ? v : dflt; }  // its value, or the default

struct nlk_ctx {
  int device = 0;
  NlkSwitches sw;                    // NLK_* switches as of nlk_ctx_create / nlk_ctx_reload_switches
  hipStream_t own_stream = nullptr;
  hipStream_t stream = nullptr;
  hipStream_t aux_stream = nullptr;  // second stream of the banded frame pipeline (run_frame)
  hipEvent_t sync_ev[8] = {};        // cross-stream dependencies of that pipeline (no timing)
  int lazy_ngx = 0, lazy_ngy = 0;    // != 0: the decision bytes of the grid rows [0, lazy_ngy) are still to be expanded
  unsigned char* lazy_dst = nullptr; //        from the tagged words into this array (nlk_ctx_flush_active; read_records)
  float* strip_acc = nullptr;        // strip calls: accumulator whose rows the layout kernel clears as it lays them out
  char err[512] = "";
  NlkBuf planes;                  // the planar copies of cur | prev | basic, one allocation (32-bit offsets between them: k_group8m.h)
  NlkBuf rowok, vmap, topk, tinfo, gcoords, marks, active, acc, tabs, wide;
  NlkBuf skew;                    // the mask replay's scratch (tu_commit.hip): the row replay's bit planes, decision bits and
                                  // row states, or the diagonal replay's mark words in step order (k_marks_skew)
  NlkBuf chase;                   // in-launch mask replay: the generation counter and the tagged decision words (zeroed when
                                  // allocated; where each sits: tu_commit.hip)
  NlkBuf ms;                      // whole-image DCT: temporary image + the two basis matrices
  NlkBuf lz3;                     // Lanczos-3 recompose step: down(yh)
  void* lz3_old[16] = {};         // ... its outgrown allocations, freed with the context (a free would synchronise the
  int lz3_nold = 0;               //     device between the levels of a recompose)
  NlkBuf tv;                      // TV-L1 pyramids and work images
  NlkBuf bm;                      // nlk_dev_bm_flow: pyramids, block vectors and the flows between levels (tu_bmflow.hip)
  NlkBuf sqd;                     // nlk_dev_sqdiff_sum: the per-workgroup partials (fixed size)
  NlkBuf sig;                     // nlk_dev_estimate_sigma: histograms, state, partials, keys (tu_sigma.hip)
  NlkBuf curve;                   // nlk_dev_estimate_noise_curve: the same per (channel, bin), block means and bins (tu_sigma.hip)
  NlkBuf ssim;                   // nlk_dev_ssim: one partial per (channel, tile) (tu_ssim.hip)
  NlkBuf sure;                    // nlk_dev_sure_terms without a map: the sums of every tile (tu_sure.hip)
  NlkBuf nlf;                     // nlk_dev_nlf_forward / _inverse: the device copy of the last table given ...
  float* nlf_host = nullptr;      // ... and what it holds (malloc), to tell a new table from it (tu_nlf.hip)
  NlkBuf slab, tflag;             // deterministic aggregation: per-tile accumulator slabs + "written" flags (k_gather.h)
  // host-pointer frame calls (nlk_frame_host): device copies of the caller's images, the streams the row bands
  // travel on and the events that order them against the kernels
  NlkBuf hw_cur, hw_prev, hw_basic, hw_out;
  hipStream_t up_stream = nullptr, dn_stream = nullptr;
  hipEvent_t band_ev[5][8] = {};  // per band: uploaded / laid out / mask rows replayed / groups filtered / rows normalised
  bool deterministic = false;     // nlk_ctx_set_deterministic / NLK_DETERMINISTIC=1
  NlkTvMail* tv_host = nullptr;   // pinned: the solver state, posted by the kernels (k_tvl1.h)
  unsigned tv_seq = 0;
  int tabs_psz = 0;
  // what a match call leaves for the group call that follows it: the geometry, the planar images and, of a smoother
  // call, planar prev - cur (k_layout; else nullptr)
  struct {
    NlkGeom g;
    const float *match, *cur, *prev, *diff;
    bool valid;
    bool packed;  // the match phase keeps packed lists (nlk_common.h) in the target records
  } last{};
  int group_packed = 0;      // nlk_ctx_last_group_packed: the last group launch read its lists packed
  int group_shape[12] = {};  // nlk_ctx_last_group_shape: written after a group launch is enqueued, read by nothing else
  // profiling: one set of NEV events per frame call, read back (and averaged)
  // only by nlk_ctx_get_timings, so the timed loop never synchronises
  static constexpr int NEV = 7, MAXSETS = 512;
  bool profiling = false;
  bool recording = false;    // the current frame call has an event set (false once MAXSETS are used)
  bool set_open = false;     // between event 0 and event 6 of a call
  unsigned set_seen = 0;     // events of the open set recorded so far
  hipEvent_t* ev = nullptr;  // [MAXSETS][NEV], created lazily
  int nsets = 0;             // completed + current
  nlk_timings tm{};
};

extern char nlk_g_err[512];  // last error without a context (nlk_hip.hip)

static inline int fail(nlk_ctx* c, int code, const char* fmt, ...) {
  char msg[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(msg, sizeof msg, fmt, ap);
  va_end(ap);
  snprintf(nlk_g_err, sizeof nlk_g_err, "%s", msg);
  if (c) snprintf(c->err, sizeof c->err, "%s", msg);
  return code;
}

#define HIPCHK(ctx, call)                                                         \
  do {                                                                            \
    hipError_t e_ = (call);                                                       \
    if (e_ != hipSuccess)                                                         \
      return fail(ctx, NLK_EHIP, "%s failed: %s (%s:%d)", #call,                  \
                  hipGetErrorString(e_), __FILE__, __LINE__);                     \
  } while (0)

// Every entry point that launches, allocates, copies or synchronises makes its context's device the
// calling thread's current one first: several contexts (NLK_DEVICES, host/multidev.c) may be driven
// from one thread in any order, and HIP launches / allocates on the CURRENT device, whatever the stream.
#define NLK_USE_DEVICE(ctx) HIPCHK(ctx, hipSetDevice((ctx)->device))

static inline int reserve(nlk_ctx* c, NlkBuf& b, size_t bytes) {
  if (bytes <= b.cap) return NLK_OK;
  if (b.p) HIPCHK(c, hipFree(b.base ? b.base : b.p));
  b.p = b.base = nullptr;
  b.cap = 0;
  // NLK_DEBUG_GUARD=1 (debugging aid): no slack, and the buffer ends where its allocation ends (allocations are
  // mapped in 2 MiB pieces), so that a kernel reading or writing past the end of a scratch buffer faults instead
  // of landing in the slack of this or in the next allocation
  static const bool guard = getenv("NLK_DEBUG_GUARD") != nullptr;
  if (guard) {
    const size_t page = (size_t)2 << 20, used = (bytes + 255) & ~(size_t)255, want = (used + page - 1) / page * page;
    if (hipMalloc(&b.base, want) != hipSuccess) return fail(c, NLK_ENOMEM, "hipMalloc of %zu bytes failed", want);
    b.p = (char*)b.base + (want - used);
    b.cap = bytes;
    return NLK_OK;
  }
  const size_t want = bytes + bytes / 8 + 256;
  if (hipMalloc(&b.p, want) != hipSuccess)
    return fail(c, NLK_ENOMEM, "hipMalloc of %zu bytes failed", want);
  b.cap = want;
  return NLK_OK;
}

// the decision bytes of the grid rows [0, ngy) exist as tagged words only, until nlk_ctx_flush_active expands them
// into `dst` (nullptr: the context's own array); ngx = 0: nothing awaits it
static inline void nlk_set_lazy_active(nlk_ctx* c, int ngx, int ngy, unsigned char* dst) {
  c->lazy_ngx = ngx;
  c->lazy_ngy = ngy;
  c->lazy_dst = dst;
}
static inline bool nlk_active_is_lazy(const nlk_ctx* c) { return c->lazy_ngx != 0; }

// the shapes the tiled matchers (k_match.h) and the LDS-DCT group kernel (k_group_lds.h) are instantiated for
static inline bool nlk_fixed_shape(int psz, int ch) {
  return (psz == 4 || psz == 6 || psz == 8 || psz == 10 || psz == 12 || psz == 16) && (ch == 1 || ch == 3);
}

// Packed lists (nlk_common.h): can the targets of a call of this geometry have them, and k_group8m's packed-list
// instantiation run it? 8 x 8 patches, the filter; the lists of the call's DOMINANT kind of target - in a temporal
// frame the targets with a valid previous patch - fit a record and its radius has a byte code. The other kind (a
// temporal frame's spatial-branch targets: npatches_x candidates, the spatial radius) is told apart target by target
// (NLK_TF_PACKED) and read as 32-bit lists by the same kernel, which keeps ONE round of 64 entries per list.
static inline bool nlk_packed_geom(const NlkGeom& g) {
  const bool t = g.smoother || g.have_prev;
  return g.psz == 8 && (g.ch == 1 || g.ch == 3) && !g.smoother && (t ? g.npt : g.npx) <= NLK_PL_MAX &&
         g.gstride <= NLK_PL_MAX && g.kmax <= 64 && (t ? g.wsz_t : g.wsz_x) <= NLK_PL_RMAX;
}

// ---- launchers (one translation unit each): every one enqueues on the view's stream and works on the view's
// records; nothing about the call in progress is read from the context
// the group launchers: `img` = the planar image the matcher saw, `cur` / `prev` = the planar frames, `active` = the
// decisions of the view's rows
typedef int NlkGroupLauncher(nlk_ctx* c, const NlkRecView& v, const NlkGeom& g, const float* img, const float* cur,
                             const float* prev, float* acc, const uint8_t* active);
// tu_group8.hip: the matrix-core group kernel for 8x8 patches
NlkGroupLauncher nlk_launch_group8;
// tu_groupp_{a,b,c}.hip: the packed-lane kernel (k_groupp.h), patch sizes 2..8 / 9..12 / 13..16, any channel count
NlkGroupLauncher nlk_launch_groupp_a, nlk_launch_groupp_b, nlk_launch_groupp_c;
// tu_group_generic.hip: the LDS-DCT kernel (k_group_lds.h), candidate lists of any length: its fixed shapes
// (nlk_fixed_shape) and its run-time shape: patch sizes up to 32, any channel count with ch * psz^2 <= 4096
NlkGroupLauncher nlk_launch_group_generic, nlk_launch_group_any;
// tu_match.hip: block matching + selection. The plan of a call's match launches, a plain function of its geometry and
// the switches (no context, no HIP call, no allocation; nlk_host_match_plan shows it to the tests): the tiled kernels'
// launch shapes for the dominant window and, in a temporal frame whose spatial radius is the larger, for the queued
// targets' wide window (nty is the launcher's: it depends on the rows it is given), or the generic kernel
struct NlkMatchPlan {
  NlkTile tl{}, tw{};            // match tiles: dominant window / wide window
  size_t lds = 0, lds_w = 0;     // their dynamic LDS bytes
  int maxm = 0, maxm_w = 0;      // rounds of 64 candidates their windows take
  bool wide = false;             // the second launch exists (k_bm_wide over the queue)
  bool generic = false;          // k_bm_generic instead of the tiled kernels
};
int nlk_match_plan(const NlkGeom& g, const NlkSwitches& sw, NlkMatchPlan* mp);
// ... and its launches for the target rows of the view (`g`: their geometry) on the view's stream: the generic kernel,
// or the dominant launch and then the wide one, whose queue length is cleared first where `clear_queue` asks for it
int nlk_launch_match(nlk_ctx* c, const NlkRecView& v, const NlkGeom& g, const NlkMatchPlan& mp, bool clear_queue,
                     const float* img);
// tu_commit.hip: the replay of the processed mask (k_commit.h) over the mark words of the grid rows
// [first, first + nrows); `marks` / `active` = whole-grid arrays, the decisions of the rows before `first` are final in
// `active`; `total` = rows of the whole grid when it is replayed band by band (first > 0 continues the band before).
// The stream is an argument: the replay works on whole-grid arrays, not on a view's records.
// Reach 0: every target is active; 1..3: the row replay on bit planes, or the diagonal one (grids wider than 2048
// targets, NLK_COMMIT_WAVE, NLK_COMMIT_BAND); above 3: whole grids only, from the coordinate lists of the context's
// own match phase
int nlk_launch_commit(nlk_ctx* c, hipStream_t stream, const uint64_t* marks, uint8_t* active, int ngx, int first,
                      int nrows, int R, int total = 0);
// ... its scratch for a grid of ngy rows replayed in `nbands` calls, reserved before the first: none of them grows it
// then (growing it between two bands would synchronise the device under the bands in flight)
int nlk_commit_reserve(nlk_ctx* c, int ngx, int R, int ngy, int nbands);
// ... the replay a group launch runs itself: bit planes of the grid rows [0, rows) + a fresh generation of tagged words
// (the counter lives on the device and is advanced by the bit-plane kernel: a step captured into a HIP graph gets a new
// generation at every replay); `chase` = what the launch, whose first row is grid row row0, is given
int nlk_chase_prepare(nlk_ctx* c, hipStream_t stream, const uint64_t* marks, int ngx, int row0, int rows, int R,
                      NlkChase* chase);
// ... and the byte per target of the grid rows [0, ngy) from the tagged words it left
int nlk_launch_active_tagged(nlk_ctx* c, hipStream_t stream, uint8_t* active, int ngx, int ngy);

// ---- nlk_hip.hip, for the frame pipeline (tu_frame.hip)
// the opening check of every call on images: context, pointers, sizes
int check_images(nlk_ctx* c, const void* out, const void* cur, int w, int h, int ch);
// the orthonormal DCT-II basis [n][n] and the aggregation window [psz][psz] a frame call uploads (nlk_host_tables)
void host_basis(float* C, int n);
void host_window(float* W, int psz);

// ---- tu_frame.hip, for nlk_host_match_plan (tu_match.hip)
// The geometry of a frame or strip call from its arguments and nlk_frame_grid, with the checks a frame call makes
// behind its opening one (check_images), in its order, with its codes and messages. Host only; `c` may be null.
int nlk_frame_geom(nlk_ctx* c, NlkGeom& g, int w, int h, int ch, float sigma, const struct nlkalman_params* P, int oy,
                   int ngy, int smoother, bool have_prev, bool have_basic);
