/* frame_grid.c — nlk_frame_grid and nlk_strip_plan (include/nlk_hip.h): the patch grid of a frame call and its split
 * into row strips, stated once for the frame pipeline (csrc/tu_frame.hip), the strips of csrc/strips.hip and
 * host/multidev.c. Host only, plain C: nothing of the device libraries is needed to link it (libnlk_hip.so links it in
 * and exports it). strips.py keeps its own statement of the plan (it imports no backend); tests/test_frame_grid.py
 * holds the two against each other. */
#include "nlk_hip.h"

int nlk_frame_grid(int w, int h, const struct nlkalman_params *P, int smoother, int have_prev,
                   struct nlk_frame_grid *out) {
  if (!P || !out || P->patch_sz < 2 || w < P->patch_sz || h < P->patch_sz) return NLK_EINVAL;
  const int psz = P->patch_sz, step = psz / 2;
  out->psz = psz;
  out->step = step;
  out->ngx = (w - psz) / step + 1;
  out->ngy = (h - psz) / step + 1;
  out->halo = smoother ? P->search_sz_t : (P->search_sz_x > P->search_sz_t ? P->search_sz_x : P->search_sz_t);
  /* in a temporal frame only groups with a valid previous patch mark the mask (reference: :931), and those are
   * searched with the temporal radius (reference: :637) */
  out->reach = ((smoother || have_prev) ? P->search_sz_t : P->search_sz_x) / step;
  return NLK_OK;
}

int nlk_strip_plan(int h, const struct nlk_frame_grid *g, int world, struct nlk_strip_plan *plan) {
  if (!g || !plan || world < 1) return NLK_EINVAL;
  if (g->ngy < world) return NLK_STRIPS_FEW_ROWS;
  for (int r = 0; r < world; ++r) {
    struct nlk_strip_plan *q = &plan[r];
    q->gy0 = (int)((long)g->ngy * r / world);
    q->gy1 = (int)((long)g->ngy * (r + 1) / world);
    const int y0 = q->gy0 * g->step - g->halo, y1 = (q->gy1 - 1) * g->step + g->halo + g->psz;
    q->Y0 = y0 > 0 ? y0 : 0;
    q->Y1 = y1 < h ? y1 : h;
    q->own0 = r > 0 ? q->gy0 * g->step : 0;
    q->own1 = r < world - 1 ? q->gy1 * g->step : h;
  }
  for (int r = 0; r + 1 < world; ++r) /* a strip may only spill into its direct neighbour's own rows */
    if (plan[r].Y1 > plan[r + 1].own1 || plan[r + 1].Y0 < plan[r].own0) return NLK_STRIPS_THIN;
  return NLK_OK;
}
