// tu_commit.hip — the replay of the raster-order processed mask (k_commit.h): which replay runs, the scratch it
// works in (nlk_ctx::skew, nlk_ctx::chase) and its launches
#include "k_commit.h"
#include "nlk_internal.h"

namespace {

// reach 1..3 on bit planes, one grid row per step; else (grids wider than the 64 words of a row, NLK_COMMIT_WAVE,
// NLK_COMMIT_BAND) the diagonal replay
bool by_rows(const nlk_ctx* c, int ngx) {
  return ngx <= 2048 && !nlk_set(c->sw.commit_wave) && !nlk_set(c->sw.commit_band);
}

// The row replay's arrays in c->skew for a grid of `rows` rows, as offsets in 32-bit words: the bit planes
// (k_commit_rows.h: NlkPlaneLayout), behind them per row the decision bits (64 words) and the row states (R x 64). The
// replay inside a group launch keeps the planes only.
struct RowArrays {
  size_t actbits, astate, end;
};
RowArrays row_arrays(int R, int rows) {
  const NlkPlaneLayout L = nlk_plane_layout(R);
  const size_t row = (size_t)L.rows_pad(rows) * 64;
  return {row * L.np, row * (L.np + 1), row * (L.np + 1 + R)};
}

// the bit planes of the grid rows [first, first + nrows) from their mark words (reach 1..3); `gen`: the in-launch
// replay's generation counter, advanced by the kernel (else nullptr)
void launch_marks_planes(hipStream_t stream, int R, const uint64_t* marks, uint32_t* planes, int ngx, int first,
                         int nrows, uint32_t* gen) {
  auto kern = R == 1 ? k_marks_planes1 : (R == 2 ? k_marks_planes<2> : k_marks_planes<3>);
  hipLaunchKernelGGL(kern, dim3(8, nrows), dim3(256), 0, stream, marks, planes, ngx, first, gen);
}

// The diagonal replay: one lane per grid row, up to `diag_band` rows per launch; more rows in pieces that start with
// the previous piece's last R rows as context (k_commit.h). A piece of `rows` rows works in diag_bytes of c->skew.
int diag_band(const nlk_ctx* c, int R) {
  const int band = nlk_or(c->sw.commit_band, 1024);
  return band < 2 * R + 2 ? 2 * R + 2 : (band > 1024 ? 1024 : band);
}
int diag_threads(int rows) { return ((rows + 63) / 64) * 64; }
size_t diag_bytes(int ngx, int R, int rows) {
  const int nsteps = ngx + (R + 1) * (rows - 1);
  return sizeof(uint32_t) * (size_t)(nsteps + 3 * NLK_CW_PHASE) * diag_threads(rows);
}

// c->chase: word [0] is the generation counter, the tagged decision words of grid row 0 start one row of 64 behind it
uint64_t* chase_words(const nlk_ctx* c) { return (uint64_t*)c->chase.p + 64; }

}  // namespace

int nlk_launch_commit(nlk_ctx* c, hipStream_t stream, const uint64_t* marks, uint8_t* active, int ngx, int first,
                      int nrows, int R, int total) {
  total = max(total, first + nrows);
  if (R == 0) {
    // a group cannot reach another grid target: nothing is ever skipped
    HIPCHK(c, hipMemsetAsync(active + (size_t)first * ngx, 1, (size_t)nrows * ngx, stream));
    return NLK_OK;
  }
  if (R <= 3 && by_rows(c, ngx)) {
    // (reach 2 / 3: the in-row chain solved by iteration); the arrays cover the whole grid
    const RowArrays A = row_arrays(R, total);
    int rc = reserve(c, c->skew, sizeof(uint32_t) * A.end);
    if (rc) return rc;
    uint32_t* planes = (uint32_t*)c->skew.p;
    uint32_t *actbits = planes + A.actbits, *astate = planes + A.astate;
    launch_marks_planes(stream, R, marks, planes, ngx, first, nrows, nullptr);
    hipLaunchKernelGGL(R == 1 ? k_mask_commit_rows1 : (R == 2 ? k_mask_commit_rows<2> : k_mask_commit_rows<3>), dim3(1),
                       dim3(64), 0, stream, (const uint32_t*)planes, actbits, astate, ngx, first, nrows);
    hipLaunchKernelGGL(k_active_bytes, dim3((ngx + 255) / 256, nrows), dim3(256), 0, stream, (const uint32_t*)actbits,
                       active, ngx, first);
    HIPCHK(c, hipGetLastError());
    return NLK_OK;
  }
  if (R <= 3) {
    const int band = diag_band(c, R);
    auto pre = R == 1 ? k_marks_skew<1> : (R == 2 ? k_marks_skew<2> : k_marks_skew<3>);
    auto kern = R == 1 ? k_mask_commit_wave<1> : (R == 2 ? k_mask_commit_wave<2> : k_mask_commit_wave<3>);
    const int end = first + nrows;
    for (int f = first; f < end;) {  // `f` = first row this piece decides
      const int ctx = f == 0 ? 0 : R;
      const int r0 = f - ctx, rows = min(band, end - r0);
      const int threads = diag_threads(rows);
      const size_t sk_bytes = diag_bytes(ngx, R, rows);
      int rc = reserve(c, c->skew, sk_bytes);
      if (rc) return rc;
      HIPCHK(c, hipMemsetAsync(c->skew.p, 0, sk_bytes, stream));
      hipLaunchKernelGGL(pre, dim3((rows * ngx + 255) / 256), dim3(256), 0, stream, marks + (size_t)r0 * ngx,
                         (uint32_t*)c->skew.p, ngx, rows, threads, (const uint8_t*)active + (size_t)r0 * ngx, ctx);
      hipLaunchKernelGGL(kern, dim3(1), dim3(threads), 0, stream, (const uint32_t*)c->skew.p,
                         active + (size_t)r0 * ngx, ngx, rows, ctx);
      f = r0 + rows;
    }
    HIPCHK(c, hipGetLastError());
    return NLK_OK;
  }
  // (2R+1)^2 neighbours do not fit the 64-bit mark words: replay from the group-coordinate lists of
  // the match phase that has just run in this context (k_mask_commit_lists)
  if (first != 0) return fail(c, NLK_EINVAL, "the list mask replay takes whole grids only");
  const int ngy = nrows;
  const NlkGeom& lg = c->last.g;
  if (!c->last.valid || lg.ngx != ngx || lg.ngy != ngy || lg.R != R || marks != (const uint64_t*)c->marks.p)
    return fail(c, NLK_EUNSUP, "group reach %d grid cells > 3: the mask replay needs the coordinate lists of the "
                "context's own match phase (row strips across GPUs are limited to reach 3)", R);
  hipLaunchKernelGGL(k_mask_commit_lists, dim3(1), dim3(1024), 0, stream, (const NlkTarget*)c->tinfo.p,
                     (const uint32_t*)c->gcoords.p, lg.gstride, active, ngx, ngy, R, lg.step, lg.oy);
  HIPCHK(c, hipGetLastError());
  return NLK_OK;
}

int nlk_commit_reserve(nlk_ctx* c, int ngx, int R, int ngy, int nbands) {
  if (R < 1 || R > 3) return NLK_OK;  // (the memset and the list replay need no scratch)
  if (by_rows(c, ngx)) return reserve(c, c->skew, sizeof(uint32_t) * row_arrays(R, ngy).end);
  // a band's first piece has the band's rows + R of context, later pieces no more
  return reserve(c, c->skew, diag_bytes(ngx, R, min(diag_band(c, R), (ngy + nbands - 1) / nbands + R)));
}

int nlk_chase_prepare(nlk_ctx* c, hipStream_t stream, const uint64_t* marks, int ngx, int row0, int rows, int R,
                      NlkChase* chase) {
  int rc = reserve(c, c->skew, sizeof(uint32_t) * row_arrays(R, rows).actbits);
  if (rc) return rc;
  const size_t wbytes = sizeof(uint64_t) * (size_t)(rows + 4 * NLK_CR_BATCH + 1) * 64;
  if (wbytes > c->chase.cap) {
    if ((rc = reserve(c, c->chase, wbytes))) return rc;
    HIPCHK(c, hipMemsetAsync(c->chase.p, 0, c->chase.cap, stream));  // (generation 0; no word of another life carries one)
  }
  launch_marks_planes(stream, R, marks, (uint32_t*)c->skew.p, ngx, 0, rows, (uint32_t*)c->chase.p);
  HIPCHK(c, hipGetLastError());
  *chase = {(const uint32_t*)c->skew.p, chase_words(c), (const uint32_t*)c->chase.p, R, row0, rows};
  return NLK_OK;
}

int nlk_launch_active_tagged(nlk_ctx* c, hipStream_t stream, uint8_t* active, int ngx, int ngy) {
  hipLaunchKernelGGL(k_active_bytes_tagged, dim3((ngx + 255) / 256, ngy), dim3(256), 0, stream,
                     (const uint64_t*)chase_words(c), active, ngx);
  HIPCHK(c, hipGetLastError());
  return NLK_OK;
}
