// tu_tvl1.hip — the TV-L1 optical flow of include/nlk_hip.h: the plan of a pyramid level (nlk_tv_plan), the layout of
// the flow's scratch (tv_layout), the three drivers of a level and the entry points, over the kernels of k_tvl1.h.
// Reference: lib/tvl1flow/tvl1flow_lib.c:345-474 (multiscale driver), :93-275 (one scale), main.c:26-35, 152-157
// (defaults, scale count).
#include <math.h>

#include "k_tvl1.h"
#include "nlk_internal.h"

namespace {

// normalised half kernel, exactly as the reference computes it (mask.c:229-256)
int tv_gauss_kernel(nlk_ctx* c, double sigma, int nx, int ny, NlkTvGauss* g) {
  const int rad = (int)(5 * sigma) + 1;
  if (rad > 32) return fail(c, NLK_EUNSUP, "TV-L1: Gaussian sigma %.3f too large (radius %d > 32)", sigma, rad);
  if (rad > nx || rad > ny)
    return fail(c, NLK_EUNSUP, "TV-L1: a %dx%d pyramid level is smaller than the Gaussian radius %d", nx, ny, rad);
  const double den = 2 * sigma * sigma;
  for (int i = 0; i < rad; ++i) g->b[i] = 1 / (sigma * sqrt(2.0 * 3.1415926)) * exp(-i * i / den);
  double norm = 0;
  for (int i = 0; i < rad; ++i) norm += g->b[i];
  norm *= 2;
  norm -= g->b[0];
  for (int i = 0; i < rad; ++i) g->b[i] /= norm;
  g->rad = rad;
  return NLK_OK;
}

inline dim3 tv_grid(int nx, int ny, int images = 1) { return dim3((nx + 31) / 32, (ny + 7) / 8, images); }
const dim3 tv_block(32, 8);

// two images at once: in -> out (may alias), tmp = scratch of the same size
int tv_gaussian2(nlk_ctx* c, const float* in_a, float* out_a, float* tmp_a, const float* in_b, float* out_b,
                 float* tmp_b, int nx, int ny, double sigma) {
  NlkTvGauss g;
  int rc = tv_gauss_kernel(c, sigma, nx, ny, &g);
  if (rc) return rc;
  hipLaunchKernelGGL(k_tv_gauss, tv_grid(nx, ny, 2), tv_block, 0, c->stream, in_a, tmp_a, in_b, tmp_b, nx, ny, g, 0);
  hipLaunchKernelGGL(k_tv_gauss, tv_grid(nx, ny, 2), tv_block, 0, c->stream, (const float*)tmp_a, out_a,
                     (const float*)tmp_b, out_b, nx, ny, g, 1);
  HIPCHK(c, hipGetLastError());
  return NLK_OK;
}

// ---- the plan of one pyramid level: a plain function of its size and the NLK_TV_* switches (no context, no HIP call,
// no allocation; nlk_host_tvl1_plan shows it to the tests). A wrong plan computes the same flow more slowly.
enum NlkTvDriver { NLK_TV_DRIVER_WG = 0, NLK_TV_DRIVER_BLOCKED = 1, NLK_TV_DRIVER_PLAIN = 2 };
typedef decltype(&k_tv_block<64, NLK_TV_TH, NLK_TV_BT, NLK_TV_K>) NlkTvBlockKernel;
struct NlkTvPlan {
  int driver = NLK_TV_DRIVER_WG;   // k_tv_level_wg, k_tv_block or k_tv_primal / k_tv_dual
  int wg_threads = 0;              // one workgroup: its threads
  int gx = 0, gy = 0;              // blocked and plain: the grid of 64 x 4 pixels per workgroup (k_tv_init, k_tv_warp, plain)
  // blocked: shape number, tile, threads and kernel of a batch, its grid, whether a batch judges its predecessor itself
  // (or k_tv_decide does between two batches) and the batches between two looks at the state
  int shape = 0, tw = 0, th = 0, bt = 0, bgx = 0, bgy = 0, nblocks = 0, look = 0;
  bool inline_judge = false;
  NlkTvBlockKernel kern = nullptr;
};

// the largest level one workgroup solves
size_t tv_wg_limit(const NlkSwitches& sw) {
  size_t wg_max = nlk_set(sw.tv_wg_pixels) ? (size_t)sw.tv_wg_pixels : NLK_TV_WG_PIXELS;
  if (wg_max > NLK_TV_WG_PIXELS) wg_max = NLK_TV_WG_PIXELS;  // (the kernel's LDS arrays)
  return wg_max;
}

int tv_wg_threads(size_t n) {
  // no more wavefronts than the level has pixels for: thread t owns pixel t (+ 1024 m), so a level of up to
  // 1024 pixels gets the same pixel -> lane mapping from ceil(n / 64) wavefronts as from 16, the workgroup sum adds
  // the same wavefront sums in the same order (the idle wavefronts only ever added zeros: bit-identical), and every
  // barrier and the serial sum over the wavefronts cost a fraction - the 30 x 17 and 15 x 9 levels of a 1080p flow
  // are chains of such latencies (~1.9 us an iteration with 16 wavefronts).
  return n <= (size_t)NLK_TV_THREADS ? (int)((n + 63) / 64) * 64 : NLK_TV_THREADS;
}

// shape -> tile width, tile height, threads, kernel (there is no shape 3: the other numbers keep their meaning)
struct NlkTvShape { int tw, th, bt; NlkTvBlockKernel kern; };
const NlkTvShape tv_shapes[] = {
  {64, NLK_TV_TH, NLK_TV_BT, k_tv_block<64, NLK_TV_TH, NLK_TV_BT, NLK_TV_K>},      // 0
  {64, NLK_TV_TH2, NLK_TV_BT, k_tv_block<64, NLK_TV_TH2, NLK_TV_BT, NLK_TV_K>},    // 1
  {64, NLK_TV_TH2, NLK_TV_BT2, k_tv_block<64, NLK_TV_TH2, NLK_TV_BT2, NLK_TV_K>},  // 2
  {0, 0, 0, nullptr},                                                              // 3
  {16, 16, 576, k_tv_block<16, 16, 576, NLK_TV_K>},                                // 4
};

int tv_shape(int nx, int ny, const NlkSwitches& sw) {
  // tile shape by the number of tiles: tall tiles do a quarter less halo work but need enough tiles to
  // keep every CU busy; with at least two tall tiles per CU, workgroups of 512 (two per CU) let one
  // tile load or store while the other computes
  const int nb16 = ((nx + 63) / 64) * ((ny + NLK_TV_TH - 1) / NLK_TV_TH), nb32 = ((nx + 63) / 64) * ((ny + NLK_TV_TH2 - 1) / NLK_TV_TH2);
  int shape = nb32 >= 512 ? 2 : nb16 >= 400 ? 1 : 0;
  // levels that leave most of the chip idle (fewer than 100 tiles of 64 x 16): tiles of 16 x 16 in workgroups of 576
  // (the 24 x 24 region, a pixel per thread) - a launch there is a chain of latencies (judge, load, 8 half iterations
  // between barriers, store), shorter with 9 wavefronts per workgroup than with 16; 1080p flow at fscale 1: 3.20 ->
  // 3.02 ms (profiles/README.md round 5: six shapes per level class; levels of 100-400 tiles do not respond)
  if (shape == 0 && nb16 < 100) shape = 4;
  shape = nlk_or(sw.tv_shape, shape);
  if (shape < 0 || shape >= (int)(sizeof(tv_shapes) / sizeof(tv_shapes[0])) || !tv_shapes[shape].kern) shape = 0;
  return shape;
}

NlkTvPlan nlk_tv_plan(int nx, int ny, const NlkSwitches& sw) {
  NlkTvPlan pl;
  const size_t n = (size_t)nx * ny;
  if (n <= tv_wg_limit(sw)) {  // the whole level inside one workgroup
    pl.wg_threads = tv_wg_threads(n);
    return pl;
  }
  pl.gx = (nx + 63) / 64;
  pl.gy = (ny + 3) / 4;
  pl.driver = nlk_set(sw.tv_unblocked) ? NLK_TV_DRIVER_PLAIN : NLK_TV_DRIVER_BLOCKED;
  if (pl.driver == NLK_TV_DRIVER_PLAIN) return pl;  // one launch per half iteration (kept for comparison)
  pl.shape = tv_shape(nx, ny, sw);
  const NlkTvShape& sh = tv_shapes[pl.shape];
  pl.tw = sh.tw; pl.th = sh.th; pl.bt = sh.bt; pl.kern = sh.kern;
  pl.bgx = (nx + sh.tw - 1) / sh.tw;
  pl.bgy = (ny + sh.th - 1) / sh.th;
  pl.nblocks = pl.bgx * pl.bgy;
  // judging inside the batches saves a launch per batch where the grid is small (k_tvl1.h: every workgroup re-adds all
  // partial sums, cheap for a few hundred workgroups, not for thousands)
  pl.inline_judge = pl.nblocks <= nlk_or(sw.tv_inline, 600);
  // batches between two looks at the state (a warp needs 5 to 50 iterations, mostly under 16)
  pl.look = nlk_or(sw.tv_look, 4);
  return pl;
}

// ---- the scratch of a flow call, walked once: 4 pyramids (I0, I1, u1, u2), the 10 work images of a level and 2
// temporaries at full size, the blocked driver's second state buffer, two batches' partial sums, the solver state and
// the min / max words. base = nullptr: the levels' sizes and `floats` only (every pointer null)
struct NlkTvScratch {
  int ns, W[64], H[64];
  float *I0s[64], *I1s[64], *U1[64], *U2[64];
  float *work, *tmp, *tmp2, *alt, *part;
  NlkTvState* st;
  int* mm;
  size_t floats;
};

int tv_layout(nlk_ctx* c, int w, int h, const nlk_tvl1_params& P, float* base, NlkTvScratch* S) {
  size_t off = 0;
  auto take = [&](size_t n) { float* p = base ? base + off : nullptr; off += n; return p; };
  S->ns = P.nscales;
  for (int s = 0; s < S->ns; ++s) {  // reference: zoom.c:23-35
    S->W[s] = s ? (int)((float)S->W[s - 1] * P.zfactor + 0.5) : w;
    S->H[s] = s ? (int)((float)S->H[s - 1] * P.zfactor + 0.5) : h;
    if (S->W[s] < 2 || S->H[s] < 2)
      return fail(c, NLK_EINVAL, "nlk_dev_tvl1_flow: %d scales leave a %dx%d level", S->ns, S->W[s], S->H[s]);
    const size_t n = (size_t)S->W[s] * S->H[s];
    S->I0s[s] = take(n); S->I1s[s] = take(n); S->U1[s] = take(n); S->U2[s] = take(n);
  }
  const size_t n0 = (size_t)w * h;
  S->work = take(10 * n0);
  S->tmp = take(n0);
  S->tmp2 = take(n0);
  S->alt = take(6 * n0);
  // workgroups of an iteration kernel at full size: 64 x 4 pixels each (k_tv_primal), or the smallest tiles of the
  // blocked kernel (16 x 16: tv_shapes)
  const size_t nparts_a = (size_t)((w + 63) / 64) * ((h + 3) / 4), nparts_b = (size_t)((w + 15) / 16) * ((h + 15) / 16);
  S->part = take(2 * NLK_TV_K * (nparts_a > nparts_b ? nparts_a : nparts_b));
  float* const tail = take(64);  // the state, and from its 8th float the min / max words
  S->st = (NlkTvState*)tail;
  S->mm = tail ? (int*)(tail + 8) : nullptr;
  S->floats = off;
  return NLK_OK;
}

// the opening check of the flow call (and of nlk_host_tvl1_plan, with the same codes and messages)
int tv_check(nlk_ctx* c, int w, int h, const nlk_tvl1_params* P) {
  if (w < 2 || h < 2) return fail(c, NLK_EINVAL, "nlk_dev_tvl1_flow: %dx%d image", w, h);
  if (!(P->tau > 0) || !(P->lambda > 0) || !(P->theta > 0) || !(P->zfactor > 0 && P->zfactor < 1) ||
      P->nscales < 1 || P->nscales > 64 || P->fscale < 0 || P->nwarps < 1 || !(P->epsilon > 0))
    return fail(c, NLK_EINVAL, "nlk_dev_tvl1_flow: parameter out of range");
  return NLK_OK;
}

// waits until the launch that closes a group has posted the solver state with sequence number `seq`
// (NlkTvMail): a spin on host memory, with a look at the stream now and then so that a failed
// launch cannot hang the caller
int tv_wait_mail(nlk_ctx* c, unsigned seq) {
  // system-scope acquire load pairing with the kernel's system-scope release store of `seq`
  // (k_tvl1.h: nlk_tv_post): the solver state posted before it is visible once the number matches
  unsigned* flag = &c->tv_host->seq;
  auto posted = [&]() { return __atomic_load_n(flag, __ATOMIC_ACQUIRE) == seq; };
  for (unsigned spins = 0;; ++spins) {
    if (posted()) break;
    if ((spins & 0xFFF) == 0xFFF) {
      const hipError_t q = hipStreamQuery(c->stream);
      if (q == hipSuccess) {  // everything has run
        if (posted()) break;
        return fail(c, NLK_EHIP, "TV-L1: the solver state was not posted");
      }
      if (q != hipErrorNotReady) return fail(c, NLK_EHIP, "TV-L1: %s", hipGetErrorString(q));
    }
    __builtin_ia32_pause();
  }
  return NLK_OK;
}

// ---- the three drivers of one scale (reference: tvl1flow_lib.c:93-275)
int tv_run_wg(nlk_ctx* c, const NlkTvLevel& L, const NlkTvPlan& pl) {
  hipLaunchKernelGGL(k_tv_level_wg, dim3(1), dim3(pl.wg_threads), 0, c->stream, L);
  HIPCHK(c, hipGetLastError());
  return NLK_OK;
}

int tv_run_plain(nlk_ctx* c, const NlkTvLevel& L, const NlkTvPlan& pl) {
  const dim3 grid(pl.gx, pl.gy);
  const int nparts = pl.gx * pl.gy, batch = 12;  // (iterations between two looks at the state)
  hipLaunchKernelGGL(k_tv_init, grid, dim3(256), 0, c->stream, L);
  for (int wi = 0; wi < L.nwarps; ++wi) {
    hipLaunchKernelGGL(k_tv_warp, grid, dim3(256), 0, c->stream, L);
    int launched = 0;
    while (launched < NLK_TV_MAXIT) {
      const int upto = launched + batch < NLK_TV_MAXIT ? launched + batch : NLK_TV_MAXIT;
      for (int it = launched + 1; it <= upto; ++it) {
        hipLaunchKernelGGL(k_tv_primal, grid, dim3(256), 0, c->stream, L, it);
        hipLaunchKernelGGL(k_tv_dual, grid, dim3(256), 0, c->stream, L, it, nparts);
      }
      launched = upto;
      HIPCHK(c, hipMemcpyAsync(&c->tv_host->st, L.st, sizeof(NlkTvState), hipMemcpyDeviceToHost, c->stream));
      HIPCHK(c, hipStreamSynchronize(c->stream));
      if (c->tv_host->st.stop_iter < NLK_TV_MAXIT || c->tv_host->st.last >= NLK_TV_MAXIT) break;
    }
  }
  HIPCHK(c, hipGetLastError());
  return NLK_OK;
}

// blocked driver: NLK_TV_K iterations per launch between two state buffers. A = the level's
// own arrays, B = a second set (`alt`); the host launches batches ahead and reads the state every
// few batches (each batch judges its predecessor's convergence when it starts, the launch that
// closes a group judges the last one); batches after the converged one are no-ops, so the final state sits in the
// buffer written by batch ceil(stop / K).
int tv_run_blocked(nlk_ctx* c, NlkTvLevel L, const NlkTvPlan& pl, float* alt) {
  const size_t n = (size_t)L.nx * L.ny;
  float *const u1 = L.u1, *const u2 = L.u2;
  const dim3 grid(pl.gx, pl.gy), bgrid(pl.bgx, pl.bgy);
  const int K = NLK_TV_K;
  const NlkTvBuf A = {u1, u2, L.p11, L.p12, L.p21, L.p22};
  const NlkTvBuf B = {alt, alt + n, alt + 2 * n, alt + 3 * n, alt + 4 * n, alt + 5 * n};
  hipLaunchKernelGGL(k_tv_init, grid, dim3(256), 0, c->stream, L);
  for (int wi = 0; wi < L.nwarps; ++wi) {
    hipLaunchKernelGGL(k_tv_warp, grid, dim3(256), 0, c->stream, L);
    NlkTvBuf cur = {L.u1, L.u2, L.p11, L.p12, L.p21, L.p22};
    const bool cur_is_a = cur.u1 == A.u1;
    NlkTvBuf oth = cur_is_a ? B : A;
    const NlkTvBuf first = cur, second = oth;  // buffers of the warp's first batch
    int n0 = 0, batches = 0, last_n0 = 0, last_count = 0;
    while (n0 < NLK_TV_MAXIT) {
      for (int q = 0; q < pl.look && n0 < NLK_TV_MAXIT; ++q) {
        const int count = NLK_TV_MAXIT - n0 < K ? NLK_TV_MAXIT - n0 : K;
        hipLaunchKernelGGL(pl.kern, bgrid, dim3(pl.bt), 0, c->stream, L, cur, oth, n0, count,
                           pl.inline_judge && q ? NLK_TV_MODE_JUDGE_BATCH : NLK_TV_MODE_BATCH, 0u);
        if (!pl.inline_judge)
          hipLaunchKernelGGL(k_tv_decide<NLK_TV_K>, dim3(1), dim3(256), 0, c->stream, L, n0, count, pl.nblocks);
        last_n0 = n0;
        last_count = count;
        const NlkTvBuf t = cur; cur = oth; oth = t;
        n0 += count;
        ++batches;
      }
      // the batch that ran past the stop (if any) is redone from its input, once per group
      // (it also judges the group's last batch)
      const unsigned seq = ++c->tv_seq;
      hipLaunchKernelGGL(pl.kern, bgrid, dim3(pl.bt), 0, c->stream, L, first, second, last_n0, last_count,
                         pl.inline_judge ? NLK_TV_MODE_CLOSE : NLK_TV_MODE_CLOSE_DECIDED, seq);
      int rc = tv_wait_mail(c, seq);
      if (rc) return rc;
      if (c->tv_host->st.stop_iter < NLK_TV_MAXIT || c->tv_host->st.fin_stop < NLK_TV_MAXIT ||
          c->tv_host->st.last >= NLK_TV_MAXIT)
        break;
    }
    // where the state of iteration `last` lives: written by batch ceil(last / K), batches alternate
    const int used = (c->tv_host->st.last + K - 1) / K;
    const bool final_is_start = (used % 2) == 0;
    const NlkTvBuf fin = final_is_start ? (cur_is_a ? A : B) : (cur_is_a ? B : A);
    L.u1 = fin.u1; L.u2 = fin.u2; L.p11 = fin.p11; L.p12 = fin.p12; L.p21 = fin.p21; L.p22 = fin.p22;
    if (nlk_set(c->sw.tv_trace))
      fprintf(stderr, "tvl1 %dx%d warp %d: %d iterations, %d batches launched\n", L.nx, L.ny, wi, c->tv_host->st.last, batches);
  }
  if (L.u1 != u1) {  // the level's flow belongs in the pyramid arrays
    HIPCHK(c, hipMemcpyAsync(u1, L.u1, sizeof(float) * n, hipMemcpyDeviceToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(u2, L.u2, sizeof(float) * n, hipMemcpyDeviceToDevice, c->stream));
  }
  HIPCHK(c, hipGetLastError());
  return NLK_OK;
}

// level s of the pyramids in S: its arrays and constants, its plan, the plan's driver
int tv_scale(nlk_ctx* c, const NlkTvScratch& S, int s, const nlk_tvl1_params& P) {
  const int nx = S.W[s], ny = S.H[s];
  const size_t n = (size_t)nx * ny;
  NlkTvLevel L;
  L.I0 = S.I0s[s]; L.I1 = S.I1s[s]; L.u1 = S.U1[s]; L.u2 = S.U2[s];
  L.I1x = S.work; L.I1y = L.I1x + n; L.I1wx = L.I1y + n; L.I1wy = L.I1wx + n; L.grad = L.I1wy + n;
  L.rho_c = L.grad + n; L.p11 = L.rho_c + n; L.p12 = L.p11 + n; L.p21 = L.p12 + n; L.p22 = L.p21 + n;
  L.part = S.part; L.st = S.st; L.mail = c->tv_host;
  L.nx = nx; L.ny = ny; L.nwarps = P.nwarps;
  L.l_t = P.lambda * P.theta; L.theta = P.theta; L.taut = P.tau / P.theta; L.eps2 = P.epsilon * P.epsilon;
  const NlkTvPlan pl = nlk_tv_plan(nx, ny, c->sw);
  if (pl.driver == NLK_TV_DRIVER_WG) return tv_run_wg(c, L, pl);
  if (pl.driver == NLK_TV_DRIVER_PLAIN) return tv_run_plain(c, L, pl);
  return tv_run_blocked(c, L, pl, S.alt);
}

}  // namespace

extern "C" {

void nlk_tvl1_default_params(struct nlk_tvl1_params* p) {  // reference: lib/tvl1flow/main.c:26-35
  p->tau = 0.25f; p->lambda = 0.15f; p->theta = 0.3f;
  p->nscales = 100; p->fscale = 0; p->zfactor = 0.5f;
  p->nwarps = 5; p->epsilon = 0.01f;
}

int nlk_tvl1_scales(int w, int h, int nscales, float zfactor) {  // reference: main.c:152-157
  const float N = 1 + log(hypot(w, h) / 16.0) / log(1 / zfactor);
  return N < nscales ? (int)N : nscales;
}

int nlk_dev_gray(nlk_ctx* c, float* gray, const float* im, int w, int h, int ch) {
  if (!c || !gray || !im || w <= 0 || h <= 0 || ch <= 0) return fail(c, NLK_EINVAL, "nlk_dev_gray: bad argument");
  NLK_USE_DEVICE(c);
  const int n = w * h;
  hipLaunchKernelGGL(k_tv_gray, dim3((n + 255) / 256), dim3(256), 0, c->stream, im, gray, n, ch);
  HIPCHK(c, hipGetLastError());
  return NLK_OK;
}

int nlk_dev_occlusion_mask(nlk_ctx* c, float* mask, const float* flow, int w, int h, float th) {
  if (!c || !mask || !flow || w <= 0 || h <= 0) return fail(c, NLK_EINVAL, "nlk_dev_occlusion_mask: bad argument");
  NLK_USE_DEVICE(c);
  hipLaunchKernelGGL(k_tv_occlusion, tv_grid(w, h), tv_block, 0, c->stream, flow, mask, w, h, th);
  HIPCHK(c, hipGetLastError());
  return NLK_OK;
}

int nlk_dev_tvl1_flow(nlk_ctx* c, float* flow, const float* I0, const float* I1, int w, int h,
                      const struct nlk_tvl1_params* P, int* iterations) {
  if (!c || !flow || !I0 || !I1 || !P) return fail(c, NLK_EINVAL, "nlk_dev_tvl1_flow: null argument");
  int rc = tv_check(c, w, h, P);
  if (rc) return rc;
  NLK_USE_DEVICE(c);
  NlkTvScratch S;
  if ((rc = tv_layout(c, w, h, *P, nullptr, &S))) return rc;
  if ((rc = reserve(c, c->tv, sizeof(float) * S.floats))) return rc;
  if (!c->tv_host) {
    HIPCHK(c, hipHostMalloc((void**)&c->tv_host, sizeof(NlkTvMail)));
    memset(c->tv_host, 0, sizeof(NlkTvMail));
  }
  if ((rc = tv_layout(c, w, h, *P, (float*)c->tv.p, &S))) return rc;
  const int ns = S.ns, *W = S.W, *H = S.H;
  float *const *I0s = S.I0s, *const *I1s = S.I1s, *const *U1 = S.U1, *const *U2 = S.U2;
  float *const work = S.work, *const tmp = S.tmp, *const tmp2 = S.tmp2;
  const size_t n0 = (size_t)w * h;

  // normalise both images to 0..255 with one common range, pre-smooth (reference: :376-381)
  HIPCHK(c, hipMemsetAsync(S.st, 0, sizeof(NlkTvState), c->stream));
  hipLaunchKernelGGL(k_tv_init_minmax, dim3(1), dim3(1), 0, c->stream, S.mm);
  hipLaunchKernelGGL(k_tv_minmax, dim3(512), dim3(1024), 0, c->stream, I0, I1, (int)n0, S.mm);
  hipLaunchKernelGGL(k_tv_normalize, dim3((n0 + 255) / 256), dim3(256), 0, c->stream, I0, I1, I0s[0],
                     I1s[0], (int)n0, (const int*)S.mm);
  float *tmp_b = work, *tmp2_b = work + n0;  // (the level arrays are idle while the pyramid is built)
  if ((rc = tv_gaussian2(c, I0s[0], I0s[0], tmp, I1s[0], I1s[0], tmp_b, w, h, 0.8))) return rc;
  // pyramid (reference: :384-398, zoom.c:44-79)
  const float zsigma = 0.6 * sqrt(1.0 / (P->zfactor * P->zfactor) - 1.0);
  for (int s = 1; s < ns; ++s) {
    if ((rc = tv_gaussian2(c, I0s[s - 1], tmp2, tmp, I1s[s - 1], tmp2_b, tmp_b, W[s - 1], H[s - 1], zsigma))) return rc;
    hipLaunchKernelGGL(k_tv_zoom, tv_grid(W[s], H[s], 2), tv_block, 0, c->stream, (const float*)tmp2, I0s[s],
                       (const float*)tmp2_b, I1s[s], W[s - 1], H[s - 1], W[s], H[s], P->zfactor, P->zfactor, 1.f, 0);
  }
  const size_t nc = (size_t)W[ns - 1] * H[ns - 1];
  HIPCHK(c, hipMemsetAsync(U1[ns - 1], 0, sizeof(float) * nc, c->stream));
  HIPCHK(c, hipMemsetAsync(U2[ns - 1], 0, sizeof(float) * nc, c->stream));
  // coarse to fine; scales finer than fscale only receive the upsampled flow (reference: :404-461)
  const float inv = (float)1.0 / P->zfactor;
  for (int s = ns - 1; s >= 0; --s) {
    if (s >= P->fscale)
      if ((rc = tv_scale(c, S, s, *P))) return rc;
    if (s == 0) break;
    const float fx = (float)W[s - 1] / W[s], fy = (float)H[s - 1] / H[s];  // zoom.c:94-95
    hipLaunchKernelGGL(k_tv_zoom, tv_grid(W[s - 1], H[s - 1], 2), tv_block, 0, c->stream, (const float*)U1[s],
                       U1[s - 1], (const float*)U2[s], U2[s - 1], W[s], H[s], W[s - 1], H[s - 1], fx, fy, inv, 1);
  }
  hipLaunchKernelGGL(k_tv_interleave, dim3((n0 + 255) / 256), dim3(256), 0, c->stream, (const float*)U1[0],
                     (const float*)U2[0], flow, (int)n0);
  HIPCHK(c, hipGetLastError());
  if (iterations) {  // (the only read-back, and only when asked for)
    HIPCHK(c, hipMemcpyAsync(&c->tv_host->st, S.st, sizeof(NlkTvState), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    *iterations = c->tv_host->st.iters;
  }
  return NLK_OK;
}

// the plan of every level of a flow call, as rows of ints (tests only: include/nlk_hip.h says what a row holds)
int nlk_host_tvl1_plan(int w, int h, const struct nlk_tvl1_params* P, int max_levels, int* out, int* nlevels) {
  if (!P || !out || !nlevels) return fail(nullptr, NLK_EINVAL, "nlk_host_tvl1_plan: null argument");
  int rc = tv_check(nullptr, w, h, P);
  if (rc) return rc;
  NlkTvScratch S;
  if ((rc = tv_layout(nullptr, w, h, *P, nullptr, &S))) return rc;
  if (S.ns > max_levels) return fail(nullptr, NLK_EINVAL, "nlk_host_tvl1_plan: %d levels, room for %d", S.ns, max_levels);
  NlkSwitches sw;
  sw.load();
  for (int s = 0; s < S.ns; ++s) {
    const NlkTvPlan pl = nlk_tv_plan(S.W[s], S.H[s], sw);
    const bool blocked = pl.driver == NLK_TV_DRIVER_BLOCKED;
    const int row[NLK_TVL1_PLAN_FIELDS] = {S.W[s], S.H[s], s >= P->fscale, pl.driver, blocked ? pl.bt : pl.wg_threads,
                                           pl.shape, pl.tw, pl.th, blocked ? pl.bgx : pl.gx, blocked ? pl.bgy : pl.gy,
                                           pl.inline_judge, pl.look};
    memcpy(out + s * NLK_TVL1_PLAN_FIELDS, row, sizeof row);
  }
  *nlevels = S.ns;
  return NLK_OK;
}

}  // extern "C"
