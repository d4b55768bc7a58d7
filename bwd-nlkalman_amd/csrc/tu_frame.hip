// tu_frame.hip — the frame pipeline behind the frame calls of include/nlk_hip.h: the plan of a frame or strip call
// (geometry from nlk_frame_grid, planar images, scratch; the match launches are planned by tu_match.hip), its phases (layout, block matching, mask replay,
// groups, normalisation) as whole-frame calls, as the strip entry points and as the host-pointer calls that move the
// frame in row bands, the profiling events the phases record, and the readers of a call's records. The kernels of the
// phases live in their own units (nlk_internal.h: the launchers); this one compiles k_frame.h.
#include <time.h>

#include "k_frame.h"
#include "nlk_internal.h"

namespace {

int upload_tables(nlk_ctx* c, int psz) {
  if (c->tabs_psz == psz) return NLK_OK;
  float host[2 * 64 * 64];
  host_basis(host, psz);
  host_window(host + psz * psz, psz);
  int rc = reserve(c, c->tabs, sizeof(float) * 2 * psz * psz);
  if (rc) return rc;
  HIPCHK(c, hipMemcpyAsync(c->tabs.p, host, sizeof(float) * 2 * psz * psz,
                           hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));  // host[] is on the stack
  c->tabs_psz = psz;
  return NLK_OK;
}

int launch_group(nlk_ctx* c, const NlkRecView& v, const NlkGeom& g, const float* img, const float* cur,
                 const float* prev, float* acc, const uint8_t* active) {
  // Default: 8x8 patches with 1 or 3 channels on the matrix cores (k_group8m.h: 1.04 ms at C2 against
  // 1.34 ms for the packed-lane kernel), everything else on the packed-lane kernel (k_groupp.h; its
  // per-lane candidate lists hold up to 128 entries). Comparison variants: NLK_GROUP_PACKED=1 (8x8 on
  // k_groupp), NLK_GENERIC_GROUP=1 (LDS-DCT kernel). Lists of more than 128
  // entries (capacity k or group size) go to the LDS-DCT kernel (k_group_lds.h): its fixed shapes where they are
  // instantiated (nlk_fixed_shape) and its run-time shape (patch size and channel count from NlkGeom) otherwise, as
  // patches above 16 do
  const bool lists_fit = g.kmax <= 128 && g.gstride <= 128;
  c->group_packed = 0;
  memset(c->group_shape, 0, sizeof c->group_shape);  // (nlk_ctx_last_group_shape: "another launcher ran", until tu_group8.hip says otherwise)
  if (g.psz > 16) return nlk_launch_group_any(c, v, g, img, cur, prev, acc, active);  // (GroupAny: 17..32)
  if (nlk_set(c->sw.generic_group) || !lists_fit)
    return nlk_fixed_shape(g.psz, g.ch) ? nlk_launch_group_generic(c, v, g, img, cur, prev, acc, active)
                                        : nlk_launch_group_any(c, v, g, img, cur, prev, acc, active);
  if (g.psz == 8 && nlk_fixed_shape(g.psz, g.ch) && !nlk_set(c->sw.group_packed))
    return nlk_launch_group8(c, v, g, img, cur, prev, acc, active);
  if (g.psz <= 8) return nlk_launch_groupp_a(c, v, g, img, cur, prev, acc, active);
  if (g.psz <= 12) return nlk_launch_groupp_b(c, v, g, img, cur, prev, acc, active);
  return nlk_launch_groupp_c(c, v, g, img, cur, prev, acc, active);
}

// the opening check of a frame call: its images and its parameters
int check_frame(nlk_ctx* c, const void* out, const void* cur, int w, int h, int ch, const struct nlkalman_params* P) {
  const int rc = check_images(c, out, cur, w, h, ch);
  return rc ? rc : (P ? NLK_OK : fail(c, NLK_EINVAL, "null parameters"));
}

// event i of the current frame call; event 0 opens a new set
// (once MAXSETS frame calls have been recorded, recording stops: the averages then cover the
// first MAXSETS calls, and no set is ever overwritten or left half-recorded)
// A set opens with event 0 and closes with event 6 (normalisation). A strip whose matching comes in
// several calls (nlk_dev_strip_match_rows) stays in ONE set: events 0 / 1 keep their first recording,
// event 2 its last, so that match_ms spans all the parts (and the halo wait between them).
void mark(nlk_ctx* c, int i) {
  if (!c->profiling) return;
  if (i == 0 && !c->set_open) {
    c->recording = c->nsets < nlk_ctx::MAXSETS;
    if (c->recording) c->nsets++;
    c->set_open = true;
    c->set_seen = 0;
  }
  if (!c->recording || c->nsets < 1) return;
  if (i <= 1 && (c->set_seen >> i) & 1u) return;
  c->set_seen |= 1u << i;
  (void)hipEventRecord(c->ev[(c->nsets - 1) * nlk_ctx::NEV + i], c->stream);
  if (i == 6) c->set_open = false;
}

}  // namespace

// The geometry of a frame or strip call (nlk_internal.h): plan_frame's, and nlk_host_match_plan's
int nlk_frame_geom(nlk_ctx* c, NlkGeom& g, int w, int h, int ch, float sigma, const struct nlkalman_params* P, int oy,
                   int ngy, int smoother, bool have_prev, bool have_basic) {
  g.w = w; g.h = h; g.ch = ch;
  g.psz = P->patch_sz;
  if (g.psz < 2 || g.psz > 32 || ch * g.psz * g.psz > 4096)
    return fail(c, NLK_EUNSUP, "patch size %d with %d channels not supported (2..32, ch * psz^2 <= 4096)", g.psz, ch);
  g.p2 = g.psz * g.psz;
  g.E = g.p2 * ch;
  struct nlk_frame_grid fg;
  if (nlk_frame_grid(w, h, P, smoother, have_prev, &fg)) return fail(c, NLK_EINVAL, "image smaller than a patch");
  g.step = fg.step;
  g.ngx = fg.ngx;
  g.oy = oy;
  g.ngy = ngy;
  if (oy < 0 || ngy < 1 || oy + (ngy - 1) * g.step + g.psz > h)
    return fail(c, NLK_EINVAL, "target rows [%d + j*%d, j < %d) leave the %d-row strip", oy,
                g.step, ngy, h);
  g.wsz_x = P->search_sz_x; g.wsz_t = P->search_sz_t;
  g.npx = P->npatches_x; g.npt = P->npatches_t; g.ntagg = P->npatches_tagg;
  if (g.wsz_x < 0 || g.wsz_t < 0 || g.ntagg < 0)
    return fail(c, NLK_EINVAL, "negative search radius or group size (call nlkalman_default_params first)");
  g.have_prev = have_prev;
  g.have_basic = have_basic;
  g.smoother = smoother != 0;
  g.sigma2 = sigma * sigma;
  g.beta_x = P->beta_x; g.beta_t = P->beta_t;
  // reach (in grid cells) of the groups that mark the processed-mask
  g.R = fg.reach;  // (R > 3: the mask replay runs from the coordinate lists, tu_commit.hip)
  g.kmax = max(max(g.npx, g.npt), 1);
  g.gstride = max(g.ntagg, 1);
  return NLK_OK;
}

extern "C" {

int nlk_ctx_set_profiling(nlk_ctx* c, int on) {
  if (!c) return NLK_EINVAL;
  if (on && !c->ev) {
    const int n = nlk_ctx::MAXSETS * nlk_ctx::NEV;
    c->ev = (hipEvent_t*)calloc(n, sizeof(hipEvent_t));
    if (!c->ev) return fail(c, NLK_ENOMEM, "event pool");
    for (int i = 0; i < n; ++i) HIPCHK(c, hipEventCreate(&c->ev[i]));
  }
  c->profiling = on != 0;
  c->recording = false;
  c->set_open = false;
  c->nsets = 0;  // (re)start averaging
  return NLK_OK;
}

// averages over every frame call recorded since profiling was switched on
int nlk_ctx_get_timings(nlk_ctx* c, struct nlk_timings* t) {
  if (!c || !t) return NLK_EINVAL;
  NLK_USE_DEVICE(c);
  memset(t, 0, sizeof *t);
  if (!c->ev || c->nsets == 0) return NLK_OK;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  double acc[6] = {0, 0, 0, 0, 0, 0};
  const int nclosed = c->nsets - ((c->set_open && c->recording) ? 1 : 0);  // (a call still under way is left out)
  if (nclosed <= 0) return NLK_OK;
  for (int s = 0; s < nclosed; ++s) {
    hipEvent_t* e = c->ev + s * nlk_ctx::NEV;
    const int a[6] = {0, 1, 2, 3, 5, 0}, b[6] = {1, 2, 3, 4, 6, 6};
    for (int i = 0; i < 6; ++i) {
      float ms = 0.f;
      HIPCHK(c, hipEventElapsedTime(&ms, e[a[i]], e[b[i]]));
      acc[i] += ms;
    }
  }
  float* dst[6] = {&t->layout_ms, &t->match_ms, &t->commit_ms, &t->group_ms, &t->normalize_ms,
                   &t->total_ms};
  for (int i = 0; i < 6; ++i) *dst[i] = (float)(acc[i] / nclosed);
  c->tm = *t;
  return NLK_OK;
}

int nlk_ctx_last_group_shape(nlk_ctx* c, int out[12]) {
  if (!c || !out) return fail(c, NLK_EINVAL, "null context / output");
  memcpy(out, c->group_shape, sizeof c->group_shape);
  return NLK_OK;
}

int nlk_ctx_last_group_packed(nlk_ctx* c) {
  if (!c) return fail(nullptr, NLK_EINVAL, "null context");  // (negative)
  return c->group_packed;
}

// ---- frame plan: geometry, planar images, scratch and the match plan of one frame or strip call
struct NlkPlan {
  NlkGeom g{};                   // the whole call: target rows [0, g.ngy) from image row g.oy
  const float *img_cur = nullptr, *img_prev = nullptr, *img_basic = nullptr, *img_match = nullptr;
  const float* img_diff = nullptr;   // smoother calls: planar prev - cur
  NlkMatchPlan mp;               // the launches of the block matching (tu_match.hip)
  bool wide0_zeroed = false;     // the layout kernel has cleared the queue length of band 0 (rows from 0)
};

// records of the target rows from `r0` on (a view into the call's buffers; `marks_ext`: the mark words go to the
// caller's array instead of the context's)
static NlkRecView view_rows(nlk_ctx* c, const NlkGeom& g, hipStream_t stream, int r0, int band,
                            uint64_t* marks_ext = nullptr) {
  const size_t t0 = (size_t)r0 * g.ngx;
  NlkRecView v;
  v.stream = stream;
  v.topk = (uint32_t*)c->topk.p + t0 * g.kmax;
  v.tinfo = (NlkTarget*)c->tinfo.p + t0;
  v.gcoords = (uint32_t*)c->gcoords.p + t0 * g.gstride;
  v.packed = c->last.packed;
  v.marks = (marks_ext ? marks_ext : (uint64_t*)c->marks.p) + t0;
  v.wide = (uint32_t*)c->wide.p + t0 + band;  // (every band: its own counter in front of its own list)
  return v;
}

// the geometry of target rows [r0, r0 + rows) of the plan
static NlkGeom band_geom(const NlkGeom& g, int r0, int rows) {
  NlkGeom b = g;
  b.oy = g.oy + r0 * g.step;
  b.ngy = rows;
  return b;
}

// layout of the pixel rows [y0, y1) (planar copies, row test of the validity map, accumulator rows cleared) and
// the validity map's column test for the rows [v0, v1) (a row needs the row tests of the psz rows from it on), on
// `stream`. `diff`: where a smoother call keeps planar prev - cur (NlkPlan::img_diff), else nullptr
static int layout_rows(nlk_ctx* c, hipStream_t stream, const float* cur, const float* prev, const float* basic,
                       float* acc_zero, const float* diff, int w, int h, int ch, int psz, int y0, int y1, int v0, int v1,
                       uint32_t* zero_word = nullptr) {
  // (every image is copied into the context's slab, one channel too: the group kernel addresses all of them from
  // one base pointer)
  const size_t img_floats = (size_t)w * h * ch;
  float* const slab = (float*)c->planes.p;
  if (y1 > y0)
    hipLaunchKernelGGL(ch == 3 ? k_layout<3> : k_layout<0>, dim3((w + 255) / 256, y1 - y0), dim3(256), 0, stream, cur, slab, prev,
                       slab + img_floats, basic, slab + 2 * img_floats, (uint8_t*)c->rowok.p, acc_zero, w, h, ch, psz,
                       1, y0, zero_word, const_cast<float*>(diff));
  if (prev && v1 > v0) {
    if (w % 4 == 0)
      hipLaunchKernelGGL(k_nan_cols4, dim3((w / 4 + 255) / 256, v1 - v0), dim3(256), 0, stream,
                         (const uint32_t*)c->rowok.p, (uint32_t*)c->vmap.p, w / 4, h, psz, v0);
    else
      hipLaunchKernelGGL(k_nan_cols, dim3((w + 255) / 256, v1 - v0), dim3(256), 0, stream, (const uint8_t*)c->rowok.p,
                         (uint8_t*)c->vmap.p, w, h, psz, v0);
  }
  HIPCHK(c, hipGetLastError());
  return NLK_OK;
}

// phase 0: checks, geometry, layout (planar copies + validity map), scratch. Runs on c->stream.
static int plan_frame(nlk_ctx* c, NlkPlan& pl, const float* cur, const float* prev, const float* basic, int w,
                      int h, int ch, float sigma, const struct nlkalman_params* P, int oy, int ngy,
                      int smoother, int nbands, float* acc_zero = nullptr, bool do_layout = true) {
  int rc = check_frame(c, cur, cur, w, h, ch, P);
  if (rc) return rc;
  NLK_USE_DEVICE(c);
  NlkGeom& g = pl.g;
  if ((rc = nlk_frame_geom(c, g, w, h, ch, sigma, P, oy, ngy, smoother, prev != nullptr, basic != nullptr))) return rc;
  // The argument checks are passed: from here on the call touches the context (scratch that regrows, planar images,
  // queue counters, then the records), so what the call before left for nlk_dev_strip_group and
  // nlk_ctx_read_records is gone - its decisions too, which may still be tagged words awaiting nlk_ctx_flush_active.
  // (Not before: a call refused above leaves all of it in place.) The state is valid again once this call's match
  // phase has been enqueued (match_done); a call refused in between leaves the context without one.
  c->last.valid = false;
  nlk_set_lazy_active(c, 0, 0, nullptr);  // (whatever replays this call's mask: `active` holds its bytes unless set again)
  const int ngrid = g.ngx * g.ngy;
  const int npix = w * h;

  mark(c, 0);
  // ---- layout: planar copies + the row test of the validity map (+ clearing the accumulator of a
  // whole-frame call) in one kernel, the column test in a second
  {
    // planar copies of the (up to) three images in ONE allocation: [cur | prev | basic]
    const size_t img_floats = (size_t)npix * ch;
    // (a smoother call keeps a fourth image, prev - cur: what the pass B of k_group8m<.., true, ..> transforms)
    const bool keep_diff = g.smoother && prev != nullptr;
    if ((rc = reserve(c, c->planes, sizeof(float) * img_floats * (keep_diff ? 4 : (basic ? 3 : (prev ? 2 : 1)))))) return rc;
    pl.img_diff = keep_diff ? (const float*)c->planes.p + 3 * img_floats : nullptr;
    pl.img_cur = (const float*)c->planes.p;
    pl.img_prev = prev ? pl.img_cur + img_floats : nullptr;
    pl.img_basic = basic ? pl.img_cur + 2 * img_floats : nullptr;
    if (prev && ((rc = reserve(c, c->rowok, npix)) || (rc = reserve(c, c->vmap, npix)))) return rc;
    if ((rc = reserve(c, c->wide, sizeof(uint32_t) * ((size_t)ngrid + nbands)))) return rc;  // per band: queue length + queue
    if (do_layout) {
      // (the layout kernel also clears the length of the first band's wide-window queue: one 6 us memset less)
      if ((rc = layout_rows(c, c->stream, cur, prev, basic, acc_zero, pl.img_diff, w, h, ch, g.psz, 0, h, 0, h,
                            (uint32_t*)c->wide.p)))
        return rc;
      pl.wide0_zeroed = true;
    }
  }
  if ((rc = upload_tables(c, g.psz))) return rc;
  if ((rc = reserve(c, c->topk, sizeof(uint32_t) * (size_t)ngrid * g.kmax)) ||
      (rc = reserve(c, c->tinfo, sizeof(NlkTarget) * (size_t)ngrid)) ||
      (rc = reserve(c, c->gcoords, sizeof(uint32_t) * (size_t)ngrid * g.gstride)) ||
      (rc = reserve(c, c->marks, sizeof(uint64_t) * (size_t)ngrid)) ||
      (rc = reserve(c, c->active, (size_t)ngrid)))
    return rc;
  mark(c, 1);

  // ---- launch shapes of the block matching (tu_match.hip)
  pl.img_match = basic ? pl.img_basic : pl.img_cur;
  if ((rc = nlk_match_plan(g, c->sw, &pl.mp))) return rc;
  // Packed lists (nlk_common.h): kept by the tiled matchers wherever k_group8m's packed instantiation could read them
  // (nlk_packed_geom; the matcher flags the targets whose record is valid, tu_group8.hip decides per launch).
  // NLK_PACKED_LISTS=0: none kept, the 32-bit lists only.
  const bool packed = !pl.mp.generic && nlk_or(c->sw.packed_lists, 1) != 0 && nlk_packed_geom(g);
  c->last = {g, pl.img_match, pl.img_cur, pl.img_prev, pl.img_diff, false, packed};  // (valid: match_done)
  return NLK_OK;
}

// the match phase of the plan is enqueued (all of it, or the part this call was asked for): the context again holds
// what nlk_dev_strip_group, nlk_dev_strip_commit_group and nlk_ctx_read_records work on
static inline void match_done(nlk_ctx* c) { c->last.valid = true; }

// phase 1 for the target rows [r0, r0 + rows) of the plan: block matching + selection on `stream`;
// leaves topk / gcoords / tinfo of those rows in the context's buffers, and their mark words there or in `marks_ext`
static int match_rows(nlk_ctx* c, const NlkPlan& pl, hipStream_t stream, int r0, int rows, int band,
                      uint64_t* marks_ext = nullptr) {
  const NlkGeom gb = band_geom(pl.g, r0, rows);
  const NlkRecView v = view_rows(c, pl.g, stream, r0, band, marks_ext);
  // (the wide queue's length is cleared here unless the layout kernel has done it)
  return nlk_launch_match(c, v, gb, pl.mp, !(pl.wide0_zeroed && r0 == 0 && band == 0), pl.img_match);
}

// The mask replay inside the group kernel's launch (k_group8m.h, NlkGTile::chase): the replay of a grid is a chain
// of ~270 dependent row steps on ONE wavefront (reach 1: 24 us of a 1.1 ms frame at 1080p, reach 2: 80 us of a 2 ms
// first frame, the rest of the chip idle) that stays far ahead of the group kernel's own progress through the rows
// (88 / 300 ns against 2.9 / 3.8 us per grid row) - so workgroup 0 of the group kernel runs it and the others pick
// their targets' decisions up as they are published. Whole-grid, single-band calls of the default kernels only
// (NLK_NO_CHASE=1: the separate kernels; first frames then go back to four bands).
static bool chase_selected(const nlk_ctx* c, const NlkGeom& g) {
  return g.R >= 1 && g.R <= 3 && g.ngx <= 2048 && g.psz == 8 && (g.ch == 1 || g.ch == 3) && g.kmax <= 128 && g.gstride <= 128 &&
         !c->deterministic && c->planes.cap < ((size_t)1 << 32) && !nlk_set(c->sw.no_chase) &&
         !nlk_set(c->sw.commit_wave) && !nlk_set(c->sw.commit_band) &&
         !nlk_set(c->sw.generic_group) && !nlk_set(c->sw.group_packed);
}

// phase 3 for the target rows [r0, r0 + rows) of the last plan (c->last); `chase`: the mask replay the launch is
// to run itself (nullptr: the decisions are in `active_rows`)
static int group_rows(nlk_ctx* c, hipStream_t stream, float* acc, const uint8_t* active_rows, int r0, int rows,
                      int band, const NlkChase* chase = nullptr) {
  const NlkGeom gb = band_geom(c->last.g, r0, rows);
  NlkRecView v = view_rows(c, c->last.g, stream, r0, band);
  if (chase) v.chase = *chase;
  return launch_group(c, v, gb, c->last.match, c->last.cur, c->last.prev, acc, active_rows);
}

// Phases 2 + 3 with the replay inside the group launch, on the context's stream: the bit planes of the grid rows
// [0, rows) of `marks`, then the groups of the last plan's target rows, whose first is grid row `row0`. The decisions
// stay tagged words; nlk_ctx_flush_active expands them into `lazy_dst` (nullptr: the context's own array) on demand.
static int chase_group(nlk_ctx* c, float* acc, const uint64_t* marks, const uint8_t* active_rows, int ngx, int row0,
                       int rows, int R, unsigned char* lazy_dst) {
  NlkChase chase;
  int rc = nlk_chase_prepare(c, c->stream, marks, ngx, row0, rows, R, &chase);
  if (rc) return rc;
  mark(c, 3);
  if ((rc = group_rows(c, c->stream, acc, active_rows, 0, c->last.g.ngy, 0, &chase))) return rc;
  nlk_set_lazy_active(c, ngx, rows, lazy_dst);
  mark(c, 4);
  return NLK_OK;
}

// Bands of a whole-frame call (NLK_BANDS=<n>, default 1 = off). The mask replay runs on ONE compute
// unit (it is a chain of dependent steps) for ~7 % of a 1080p frame's time. With the grid rows cut in
// bands on two streams, band b+1 is matched while band b's mask is replayed and band b is filtered
// while band b+1's is. Measured at C2 (profiles/README.md): 1.59 ms with one band, 1.64 with two,
// 1.77 with four - the two bands' match kernels share the chip instead of finishing one after the
// other, and the four cross-stream dependencies and the doubled launches cost what the hidden replay
// gains. Kept as an option (and as the exactness test of banding); profiling always runs one band.
// at most 8 bands, and none so thin that there is nothing to gain
static int clamp_bands(int nb, int ngy, int R) {
  nb = nb < 1 ? 1 : (nb > 8 ? 8 : nb);
  while (nb > 1 && ngy / nb < 4 * (R + 1) + 8) --nb;
  return nb;
}

static int frame_bands(const nlk_ctx* c, const NlkGeom& g) {
  if (c->profiling || c->deterministic || g.R == 0 || g.R > 3) return 1;  // (deterministic mode: one slab set, one sum order)
  // default: one band for reach 1 (the replay is 2 % of a frame); four for reach 2 / 3, i.e. spatial frames of
  // small patches: their replay was the diagonal one until round 4 (0.28 ms of a first frame at 1080p on one
  // compute unit); as the iterated row replay it takes 0.08 ms, and four bands still win (first frame at 1080p:
  // 2.09-2.10 ms with one band, 2.04-2.10 with two, 2.01-2.05 with four; 2.13 with the diagonal replay in four)
  return clamp_bands(nlk_or(c->sw.bands, g.R >= 2 ? 4 : 1), g.ngy, g.R);
}

// One band of a banded pipeline, on `s`: the mask replay of the last plan's target rows [r0, r1) behind the replay of
// the band before (`after`; nullptr: the first band), `done` recorded behind it, then the groups of those rows
static int band_step(nlk_ctx* c, hipStream_t s, float* acc, int r0, int r1, int band, hipEvent_t after, hipEvent_t done) {
  const NlkGeom& g = c->last.g;
  uint8_t* active = (uint8_t*)c->active.p;
  if (after) HIPCHK(c, hipStreamWaitEvent(s, after, 0));
  const int rc = nlk_launch_commit(c, s, (const uint64_t*)c->marks.p, active, g.ngx, r0, r1 - r0, g.R, g.ngy);
  if (rc) return rc;
  HIPCHK(c, hipEventRecord(done, s));
  return group_rows(c, s, acc, active + (size_t)r0 * g.ngx, r0, r1 - r0, band);
}

// `clear`: the accumulator is cleared by the layout kernel (whole-frame calls)
static int frame_accumulate(nlk_ctx* c, float* acc, const float* cur, const float* prev,
                            const float* basic, int w, int h, int ch, float sigma,
                            const struct nlkalman_params* P, int oy, int ngy, int smoother, bool clear) {
  if (!acc) return fail(c, NLK_EINVAL, "null accumulator");
  NlkPlan pl;
  int rc = plan_frame(c, pl, cur, prev, basic, w, h, ch, sigma, P, oy, ngy, smoother, 8, clear ? acc : nullptr);
  if (rc) return rc;
  const NlkGeom& g = pl.g;
  // (a replay that rides inside the group launch needs no bands to hide behind)
  const bool chase = chase_selected(c, g);
  const int nb = (chase && !nlk_set(c->sw.bands)) ? 1 : frame_bands(c, g);
  uint8_t* active = (uint8_t*)c->active.p;
  if (nb == 1) {
    if ((rc = match_rows(c, pl, c->stream, 0, g.ngy, 0))) return rc;
    match_done(c);
    mark(c, 2);
    if (chase)  // (the bytes of `active` only when somebody reads the records)
      return chase_group(c, acc, (const uint64_t*)c->marks.p, active, g.ngx, 0, g.ngy, g.R, nullptr);
    if ((rc = nlk_launch_commit(c, c->stream, (const uint64_t*)c->marks.p, active, g.ngx, 0, g.ngy, g.R))) return rc;
    mark(c, 3);
    if ((rc = group_rows(c, c->stream, acc, active, 0, g.ngy, 0))) return rc;
    mark(c, 4);
    return NLK_OK;
  }
  // ---- banded on two streams. Band b runs on stream b & 1; its mask replay waits for band b-1's.
  // (the replay's scratch for every band now: growing it between two bands would synchronise the device)
  if ((rc = nlk_commit_reserve(c, g.ngx, g.R, g.ngy, nb))) return rc;
  hipStream_t st[2] = {c->stream, c->aux_stream};
  hipEvent_t* ev = c->sync_ev;  // [0] layout done, [1] / [2] replay of the last even / odd band done, [3] aux stream done
  HIPCHK(c, hipEventRecord(ev[0], st[0]));
  HIPCHK(c, hipStreamWaitEvent(st[1], ev[0], 0));
  int r0[9];
  for (int b = 0; b <= nb; ++b) r0[b] = (int)((long)g.ngy * b / nb);
  for (int b = 0; b < nb; ++b)
    if ((rc = match_rows(c, pl, st[b & 1], r0[b], r0[b + 1] - r0[b], b))) return rc;
  match_done(c);
  for (int b = 0; b < nb; ++b)
    if ((rc = band_step(c, st[b & 1], acc, r0[b], r0[b + 1], b, b > 0 ? ev[1 + ((b - 1) & 1)] : nullptr, ev[1 + (b & 1)]))) return rc;
  HIPCHK(c, hipEventRecord(ev[3], st[1]));
  HIPCHK(c, hipStreamWaitEvent(st[0], ev[3], 0));
  return NLK_OK;
}

int nlk_dev_frame_accumulate(nlk_ctx* c, float* acc, const float* cur, const float* prev,
                             const float* basic, int w, int h, int ch, float sigma,
                             const struct nlkalman_params* P, int oy, int ngy, int smoother) {
  return frame_accumulate(c, acc, cur, prev, basic, w, h, ch, sigma, P, oy, ngy, smoother, false);
}

// ---- the same three phases as separate entry points (exact masks across GPUs)
// rows [r0, r0 + rows) of the strip's target rows (a whole strip: r0 = 0, rows = ngy). _part lays out the pixel
// rows [lay0, lay1) only (planar copies, row test of the validity map) and finishes the validity map of the rows
// [v0, v1): a caller matches the rows that do not depend on a halo still in flight first - laying out its own rows -
// and lays out the halo rows and matches the seam rows once they have arrived (nothing reads rows in flight, nothing
// is laid out twice). _rows lays the whole strip out again on every call.
int nlk_dev_strip_match_part(nlk_ctx* c, const float* cur, const float* prev, const float* basic, int w,
                             int h, int ch, float sigma, const struct nlkalman_params* P, int oy,
                             int ngy, int smoother, int r0, int rows, int lay0, int lay1, int v0, int v1,
                             void* marks_out, int* reach) {
  if (lay0 < 0 || lay1 > h || lay0 > lay1 || v0 < 0 || v1 > h || v0 > v1)
    return fail(c, NLK_EINVAL, "layout rows [%d, %d) / validity rows [%d, %d) outside the %d-row strip", lay0, lay1, v0, v1, h);
  // (every check that can refuse the call on its arguments runs before plan_frame touches the context)
  if (ngy >= 1 && (r0 < 0 || rows < 0 || r0 + rows > ngy))
    return fail(c, NLK_EINVAL, "rows [%d, %d) outside the strip's %d target rows", r0, r0 + rows, ngy);
  struct nlk_frame_grid fg;
  if (marks_out && P && w > 0 && h > 0 && nlk_frame_grid(w, h, P, smoother, prev != nullptr, &fg) == NLK_OK && fg.reach > 3)
    return fail(c, NLK_EUNSUP, "group reach %d grid cells > 3: 64-bit mark words cannot describe it (row strips "
                "across GPUs are limited to reach 3; whole-frame calls are not)", fg.reach);
  NlkPlan pl;
  int rc = plan_frame(c, pl, cur, prev, basic, w, h, ch, sigma, P, oy, ngy, smoother, 1, nullptr, false);
  if (rc) return rc;
  // (nlk_ctx_set_strip_accumulator: the rows laid out are also the accumulator rows cleared - no separate memset)
  if ((rc = layout_rows(c, c->stream, cur, prev, basic, c->strip_acc, pl.img_diff, w, h, ch, pl.g.psz, lay0, lay1, v0, v1)))
    return rc;
  mark(c, 1);
  // the matcher writes the mark words of these rows straight to their place in the caller's array
  if (rows > 0 && (rc = match_rows(c, pl, c->stream, r0, rows, 0, (uint64_t*)marks_out))) return rc;
  match_done(c);
  mark(c, 2);
  if (reach) *reach = pl.g.R;
  return NLK_OK;
}

int nlk_dev_strip_match_rows(nlk_ctx* c, const float* cur, const float* prev, const float* basic, int w,
                             int h, int ch, float sigma, const struct nlkalman_params* P, int oy,
                             int ngy, int smoother, int r0, int rows, void* marks_out, int* reach) {
  return nlk_dev_strip_match_part(c, cur, prev, basic, w, h, ch, sigma, P, oy, ngy, smoother, r0, rows, 0, h, 0, h,
                                  marks_out, reach);
}

int nlk_dev_strip_match(nlk_ctx* c, const float* cur, const float* prev, const float* basic, int w,
                        int h, int ch, float sigma, const struct nlkalman_params* P, int oy,
                        int ngy, int smoother, void* marks_out, int* reach) {
  return nlk_dev_strip_match_rows(c, cur, prev, basic, w, h, ch, sigma, P, oy, ngy, smoother, 0, ngy, marks_out, reach);
}

int nlk_ctx_set_strip_accumulator(nlk_ctx* c, float* acc) {
  if (!c) return NLK_EINVAL;
  c->strip_acc = acc;
  return NLK_OK;
}

int nlk_dev_mask_commit(nlk_ctx* c, const void* marks, int ngx, int ngy, int reach,
                        unsigned char* active) {
  if (!c || !marks || !active || ngx < 1 || ngy < 1 || reach < 0)
    return fail(c, NLK_EINVAL, "bad mask-commit arguments");
  NLK_USE_DEVICE(c);
  int rc = nlk_launch_commit(c, c->stream, (const uint64_t*)marks, active, ngx, 0, ngy, reach);
  mark(c, 3);
  return rc;
}

int nlk_dev_strip_group(nlk_ctx* c, float* acc, const unsigned char* active) {
  if (!c || !c->last.valid) return fail(c, NLK_EINVAL, "nlk_dev_strip_match has not run");
  if (!acc || !active) return fail(c, NLK_EINVAL, "null accumulator / active flags");
  NLK_USE_DEVICE(c);
  int rc = group_rows(c, c->stream, acc, active, 0, c->last.g.ngy, 0);
  mark(c, 4);
  return rc;
}

// Phases 2 + 3 of a strip in one call: the mask replay over the whole grid's mark words and the strip's groups. Where
// the group kernel can run the replay inside its own launch (chase_selected) only the grid rows down to the strip's
// last one are replayed, by its workgroup 0, and `active` is not written; otherwise exactly nlk_dev_mask_commit +
// nlk_dev_strip_group on `active + gy0 * ngx`.
int nlk_dev_strip_commit_group(nlk_ctx* c, float* acc, const void* marks, int ngx, int ngy, int reach, int gy0,
                               unsigned char* active) {
  if (!c || !c->last.valid) return fail(c, NLK_EINVAL, "nlk_dev_strip_match has not run");
  const NlkGeom& g = c->last.g;
  if (!acc || !marks || !active || ngx < 1 || ngy < 1 || reach < 0 || gy0 < 0 || gy0 + g.ngy > ngy || ngx != g.ngx)
    return fail(c, NLK_EINVAL, "bad strip commit / group arguments");
  NLK_USE_DEVICE(c);
  if (reach == g.R && chase_selected(c, g))  // (nlk_ctx_flush_active: rows [0, gy0 + g.ngy) of `active`)
    return chase_group(c, acc, (const uint64_t*)marks, active + (size_t)gy0 * ngx, ngx, gy0, gy0 + g.ngy, reach, active);
  int rc = nlk_launch_commit(c, c->stream, (const uint64_t*)marks, active, ngx, 0, ngy, reach);
  if (rc) return rc;
  mark(c, 3);
  rc = group_rows(c, c->stream, acc, active + (size_t)gy0 * ngx, 0, g.ngy, 0);
  mark(c, 4);
  return rc;
}

int nlk_dev_frame_normalize(nlk_ctx* c, float* out, const float* acc, const float* cur, int w,
                            int h, int ch, int y0, int y1) {
  int rc = check_images(c, out, cur, w, h, ch);
  if (rc) return rc;
  if (!acc || y0 < 0 || y1 > h || y0 > y1) return fail(c, NLK_EINVAL, "bad normalise range");
  NLK_USE_DEVICE(c);
  mark(c, 5);
  hipLaunchKernelGGL(ch == 3 ? k_normalize<3> : k_normalize<0>, dim3(2048), dim3(256), 0, c->stream, out, acc, cur, w, h, ch,
                     y0, y1);
  HIPCHK(c, hipGetLastError());
  mark(c, 6);
  return NLK_OK;
}

static int run_frame(nlk_ctx* c, float* out, const float* cur, const float* prev,
                     const float* basic, int w, int h, int ch, float sigma,
                     const struct nlkalman_params* P, int smoother) {
  int rc = check_frame(c, out, cur, w, h, ch, P);
  if (rc) return rc;
  if (P->patch_sz < 2) return fail(c, NLK_EUNSUP, "patch size %d not supported", P->patch_sz);
  NLK_USE_DEVICE(c);
  const size_t accb = sizeof(float) * (size_t)w * h * (ch + 1);
  if ((rc = reserve(c, c->acc, accb))) return rc;
  struct nlk_frame_grid fg;
  if (nlk_frame_grid(w, h, P, smoother, prev != nullptr, &fg)) {
    // no target fits (the reference's loops `px < w - psz + 1`, src/nlkalman.c:586-595, do not run): nothing is
    // aggregated and every pixel keeps its input value (:939-942)
    HIPCHK(c, hipMemcpyAsync(out, cur, sizeof(float) * (size_t)w * h * ch, hipMemcpyDeviceToDevice, c->stream));
    return NLK_OK;
  }
  rc = frame_accumulate(c, (float*)c->acc.p, cur, prev, basic, w, h, ch, sigma, P, 0, fg.ngy, smoother, true);
  if (rc) return rc;
  rc = nlk_dev_frame_normalize(c, out, (const float*)c->acc.p, cur, w, h, ch, 0, h);
  return rc;
}

int nlk_dev_filter_frame(nlk_ctx* c, float* deno1, const float* nisy1, const float* deno0,
                         const float* bsic1, int w, int h, int ch, float sigma,
                         const struct nlkalman_params* P) {
  return run_frame(c, deno1, nisy1, deno0, bsic1, w, h, ch, sigma, P, 0);
}

int nlk_dev_smooth_frame(nlk_ctx* c, float* smoo1, const float* filt1, const float* smoo0,
                         const float* bsic1, int w, int h, int ch, float sigma,
                         const struct nlkalman_params* P) {
  return run_frame(c, smoo1, filt1, smoo0, bsic1, w, h, ch, sigma, P, 1);
}

// ---- the frame functions on HOST images (what the drop-in API of include/nlkalman.h hands over: pageable
// memory, src/nlkalman.h:46-53). A 1080p RGB call moves 75 MB up and 25 MB down over PCIe, as long as its
// kernels run; done one after the other that is 3.2 ms for 1.35 ms of kernels. Here the frame travels in
// row bands: band b is laid out, matched, its mask rows replayed and its groups filtered while band b+1 is
// still on the link (the upload calls return when the host pages are staged, so the host issues them back
// to back and the kernels follow one band behind), and the rows no later band can add to are normalised
// and sent back while the last bands are still being filtered. Results: the banded pipeline's
// (frame_accumulate), i.e. the whole-frame call's decisions and sums.
static int frame_host(nlk_ctx* c, float* out_h, const float* cur_h, const float* prev_h, const float* basic_h, int w,
                      int h, int ch, float sigma, const struct nlkalman_params* P, int smoother) {
  int rc = check_frame(c, out_h, cur_h, w, h, ch, P);
  if (rc) return rc;
  NLK_USE_DEVICE(c);
  const size_t npix = (size_t)w * h, bytes = sizeof(float) * npix * ch, rowb = sizeof(float) * (size_t)w * ch;
  if ((rc = reserve(c, c->hw_cur, bytes)) || (rc = reserve(c, c->hw_out, bytes)) ||
      (prev_h && (rc = reserve(c, c->hw_prev, bytes))) || (basic_h && (rc = reserve(c, c->hw_basic, bytes))) ||
      (rc = reserve(c, c->acc, sizeof(float) * npix * (ch + 1))))
    return rc;
  float *d_cur = (float*)c->hw_cur.p, *d_out = (float*)c->hw_out.p;
  float *d_prev = prev_h ? (float*)c->hw_prev.p : nullptr, *d_basic = basic_h ? (float*)c->hw_basic.p : nullptr;
  struct nlk_frame_grid fg = {};
  const bool fits = nlk_frame_grid(w, h, P, smoother, prev_h != nullptr, &fg) == NLK_OK;  // (if not: run_frame says why)
  const int psz = fg.psz, step = fg.step, ngy = fg.ngy, wall = fg.halo, R = fg.reach;
  // (1080p: 2 bands 2.43 ms, 3 2.30, 4 2.25, 5 2.20, 6 2.22; one upload + call + download 2.9)
  const int nb = fits ? clamp_bands(nlk_or(c->sw.host_bands, 5), ngy, R) : 1;
  if (nb < 2 || R > 3 || c->deterministic || c->profiling || psz > 16) {
    // small frames, masks replayed from the coordinate lists, deterministic slabs, per-kernel timing, and
    // everything the frame call rejects: one upload, the whole-frame call, one download
    HIPCHK(c, hipMemcpyAsync(d_cur, cur_h, bytes, hipMemcpyHostToDevice, c->stream));
    if (prev_h) HIPCHK(c, hipMemcpyAsync(d_prev, prev_h, bytes, hipMemcpyHostToDevice, c->stream));
    if (basic_h) HIPCHK(c, hipMemcpyAsync(d_basic, basic_h, bytes, hipMemcpyHostToDevice, c->stream));
    if ((rc = run_frame(c, d_out, d_cur, d_prev, d_basic, w, h, ch, sigma, P, smoother))) return rc;
    HIPCHK(c, hipMemcpyAsync(out_h, d_out, bytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return NLK_OK;
  }
  if (!c->up_stream) {
    HIPCHK(c, hipStreamCreateWithFlags(&c->up_stream, hipStreamNonBlocking));
    HIPCHK(c, hipStreamCreateWithFlags(&c->dn_stream, hipStreamNonBlocking));
    for (auto& row : c->band_ev)
      for (hipEvent_t& e : row) HIPCHK(c, hipEventCreateWithFlags(&e, hipEventDisableTiming));
  }
  NlkPlan pl;
  float* acc = (float*)c->acc.p;
  if ((rc = plan_frame(c, pl, d_cur, d_prev, d_basic, w, h, ch, sigma, P, 0, ngy, smoother, 8, nullptr, false))) return rc;
  // (the replay's scratch for every band, before the first band is in flight)
  if ((rc = nlk_commit_reserve(c, pl.g.ngx, pl.g.R, pl.g.ngy, nb))) return rc;
  // the streams start behind whatever the context's stream was doing (the device images are reused call to call)
  HIPCHK(c, hipEventRecord(c->sync_ev[0], c->stream));
  HIPCHK(c, hipStreamWaitEvent(c->up_stream, c->sync_ev[0], 0));
  HIPCHK(c, hipStreamWaitEvent(c->aux_stream, c->sync_ev[0], 0));
  // Bands alternate between two streams, so that the tail of a band's kernels (a quarter of a frame does not
  // fill the chip to the end) overlaps the next band's: E_UP uploaded, E_LAY laid out, E_MASK mask rows
  // replayed, E_GRP groups filtered, E_DONE rows normalised.
  enum { E_UP, E_LAY, E_MASK, E_GRP, E_DONE };
  hipStream_t st[2] = {c->stream, c->aux_stream};
  int up0 = 0, v0 = 0, nz0 = 0, nz[9];
  nz[0] = 0;
  const bool trace = nlk_set(c->sw.host_trace);
  struct timespec ts0, ts1, ts2;
  if (trace) clock_gettime(CLOCK_MONOTONIC, &ts0);
  for (int b = 0; b < nb; ++b) {
    const int r0 = (int)((long)ngy * b / nb), r1 = (int)((long)ngy * (b + 1) / nb);
    const bool last = b + 1 == nb;
    hipStream_t s = st[b & 1];
    // pixel rows band b reads (windows, patches) and writes (group members): up to up1
    const int up1 = last ? h : min(h, (r1 - 1) * step + wall + psz);
    const size_t off = (size_t)up0 * w * ch;
    HIPCHK(c, hipMemcpyAsync(d_cur + off, cur_h + off, rowb * (up1 - up0), hipMemcpyHostToDevice, c->up_stream));
    if (prev_h) HIPCHK(c, hipMemcpyAsync(d_prev + off, prev_h + off, rowb * (up1 - up0), hipMemcpyHostToDevice, c->up_stream));
    if (basic_h) HIPCHK(c, hipMemcpyAsync(d_basic + off, basic_h + off, rowb * (up1 - up0), hipMemcpyHostToDevice, c->up_stream));
    HIPCHK(c, hipEventRecord(c->band_ev[E_UP][b], c->up_stream));
    HIPCHK(c, hipStreamWaitEvent(s, c->band_ev[E_UP][b], 0));
    if (b > 0) HIPCHK(c, hipStreamWaitEvent(s, c->band_ev[E_LAY][b - 1], 0));  // (the column test reads the rows before)
    const int v1 = last ? h : up1 - psz + 1;
    if ((rc = layout_rows(c, s, d_cur, d_prev, d_basic, acc, pl.img_diff, w, h, ch, psz, up0, up1, v0, v1))) return rc;
    HIPCHK(c, hipEventRecord(c->band_ev[E_LAY][b], s));
    if ((rc = match_rows(c, pl, s, r0, r1 - r0, b))) return rc;
    if ((rc = band_step(c, s, acc, r0, r1, b, b > 0 ? c->band_ev[E_MASK][b - 1] : nullptr, c->band_ev[E_MASK][b]))) return rc;
    HIPCHK(c, hipEventRecord(c->band_ev[E_GRP][b], s));
    // rows no later band adds to: the groups of the targets from row r1 on start at r1 * step - wall at the earliest
    nz[b + 1] = last ? h : max(nz0, min(h, r1 * step - wall));
    if (nz[b + 1] > nz0) {
      if (b > 0) HIPCHK(c, hipStreamWaitEvent(s, c->band_ev[E_GRP][b - 1], 0));
      hipLaunchKernelGGL(ch == 3 ? k_normalize<3> : k_normalize<0>, dim3(1024), dim3(256), 0, s, d_out, (const float*)acc, (const float*)d_cur, w, h,
                         ch, nz0, nz[b + 1]);
      HIPCHK(c, hipGetLastError());
    }
    HIPCHK(c, hipEventRecord(c->band_ev[E_DONE][b], s));
    up0 = up1; v0 = v1; nz0 = nz[b + 1];
  }
  match_done(c);
  if (trace) clock_gettime(CLOCK_MONOTONIC, &ts1);
  // the rows go back band by band: every upload has been issued by now, the kernels of the first bands are done
  for (int b = 0; b < nb; ++b) {
    if (nz[b + 1] <= nz[b]) continue;
    HIPCHK(c, hipStreamWaitEvent(c->dn_stream, c->band_ev[E_DONE][b], 0));
    const size_t off = (size_t)nz[b] * w * ch;
    HIPCHK(c, hipMemcpyAsync(out_h + off, d_out + off, rowb * (nz[b + 1] - nz[b]), hipMemcpyDeviceToHost, c->dn_stream));
  }
  HIPCHK(c, hipStreamSynchronize(c->dn_stream));
  HIPCHK(c, hipStreamSynchronize(c->aux_stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (trace) {
    clock_gettime(CLOCK_MONOTONIC, &ts2);
    fprintf(stderr, "nlk frame_host: %d bands, uploads + launches issued after %.3f ms, downloads done after %.3f ms\n", nb,
            (ts1.tv_sec - ts0.tv_sec) * 1e3 + (ts1.tv_nsec - ts0.tv_nsec) * 1e-6,
            (ts2.tv_sec - ts0.tv_sec) * 1e3 + (ts2.tv_nsec - ts0.tv_nsec) * 1e-6);
  }
  return NLK_OK;
}

int nlk_filter_frame_host(nlk_ctx* c, float* deno1, const float* nisy1, const float* deno0, const float* bsic1, int w,
                          int h, int ch, float sigma, const struct nlkalman_params* P) {
  if (!c) return fail(nullptr, NLK_EINVAL, "null context");
  return frame_host(c, deno1, nisy1, deno0, bsic1, w, h, ch, sigma, P, 0);
}

int nlk_smooth_frame_host(nlk_ctx* c, float* smoo1, const float* filt1, const float* smoo0, const float* bsic1, int w,
                          int h, int ch, float sigma, const struct nlkalman_params* P) {
  if (!c) return fail(nullptr, NLK_EINVAL, "null context");
  return frame_host(c, smoo1, filt1, smoo0, bsic1, w, h, ch, sigma, P, 1);
}
// How many targets of the last match phase carry a valid packed record (NLK_TF_PACKED): tests only
int nlk_ctx_count_packed(nlk_ctx* c, int* count) {
  if (!c || !count || !c->last.valid) return fail(c, NLK_EINVAL, "no frame has been processed");
  NLK_USE_DEVICE(c);
  const int n = c->last.g.ngx * c->last.g.ngy;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  NlkTarget* t = (NlkTarget*)malloc(sizeof(NlkTarget) * n);
  if (!t) return fail(c, NLK_ENOMEM, "host malloc failed");
  const hipError_t e = hipMemcpy(t, c->tinfo.p, sizeof(NlkTarget) * n, hipMemcpyDeviceToHost);
  int m = 0;
  if (e == hipSuccess)
    for (int i = 0; i < n; ++i) m += (t[i].flags & NLK_TF_PACKED) ? 1 : 0;
  free(t);
  HIPCHK(c, e);
  *count = m;
  return NLK_OK;
}

// Where a group kernel replayed the processed mask inside its own launch the decisions exist as tagged words only;
// this writes the byte per target of the replayed grid rows into the array the call was given (frame calls: the
// context's own, read by nlk_ctx_read_records) and waits for it. No-op otherwise.
int nlk_ctx_flush_active(nlk_ctx* c) {
  if (!c) return fail(nullptr, NLK_EINVAL, "null context");
  if (!nlk_active_is_lazy(c)) return NLK_OK;
  NLK_USE_DEVICE(c);
  int rc = nlk_launch_active_tagged(c, c->stream, c->lazy_dst ? c->lazy_dst : (uint8_t*)c->active.p, c->lazy_ngx, c->lazy_ngy);
  if (rc) return rc;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  nlk_set_lazy_active(c, 0, 0, nullptr);
  return NLK_OK;
}

int nlk_ctx_read_records(nlk_ctx* c, int* ngrid, int* kmax, int* gmax, unsigned char* active,
                         int* nsel, int* np0, int* nagg, unsigned int* topk,
                         unsigned int* gcoords) {
  if (!c || !c->last.valid) return fail(c, NLK_EINVAL, "no frame has been processed");
  NLK_USE_DEVICE(c);
  const NlkGeom& g = c->last.g;
  const int n = g.ngx * g.ngy;
  if (ngrid) *ngrid = n;
  if (kmax) *kmax = g.kmax;
  if (gmax) *gmax = g.gstride;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (active) {  // (the group kernel replayed the mask itself: expand its decision words now)
    int rc = nlk_ctx_flush_active(c);
    if (rc) return rc;
  }
  if (active) HIPCHK(c, hipMemcpy(active, c->active.p, n, hipMemcpyDeviceToHost));
  if (nsel || np0 || nagg) {
    NlkTarget* t = (NlkTarget*)malloc(sizeof(NlkTarget) * n);
    if (!t) return fail(c, NLK_ENOMEM, "host malloc failed");
    hipError_t e = hipMemcpy(t, c->tinfo.p, sizeof(NlkTarget) * n, hipMemcpyDeviceToHost);
    if (e == hipSuccess)
      for (int i = 0; i < n; ++i) {
        if (nsel) nsel[i] = t[i].nsel;
        if (np0) np0[i] = t[i].np0;
        if (nagg) nagg[i] = t[i].nagg;
      }
    free(t);
    HIPCHK(c, e);
  }
  if (topk)
    HIPCHK(c, hipMemcpy(topk, c->topk.p, sizeof(uint32_t) * (size_t)n * g.kmax,
                        hipMemcpyDeviceToHost));
  if (gcoords)
    HIPCHK(c, hipMemcpy(gcoords, c->gcoords.p, sizeof(uint32_t) * (size_t)n * g.gstride,
                        hipMemcpyDeviceToHost));
  return NLK_OK;
}

}  // extern "C"

