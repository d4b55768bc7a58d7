/* nlk_hip.h — thin C-ABI over the hand-written HIP (gfx950) kernels.
 *
 * This is the boundary a maintainer of the reference would bind to replace the
 * body of its three frame functions and its three image helpers. Plain
 * pointers and sizes only; every entry point returns 0 on success or a
 * negative NLK_E* code, with a message retrievable by nlk_last_error().
 * Device pointers are ordinary HIP device addresses (hipMalloc / a torch
 * tensor's data_ptr()); images keep the reference's HWC interleaved float32
 * layout, index (x + y*w)*ch + c (reference: src/nlkalman.c:555-560).
 *
 * What each entry point replaces in the reference:
 *   nlk_dev_rgb2opp / nlk_dev_opp2rgb   src/nlkalman.c:92-130
 *   nlk_dev_warp_bicubic                src/nlkalman.c:29-88
 *   nlk_dev_filter_frame                src/nlkalman.c:518-951  (nlkalman_filter_frame)
 *   nlk_dev_smooth_frame                src/nlkalman.c:1409-1865 (nlkalman_smooth_frame)
 *   nlk_dev_strip_match / nlk_dev_mask_commit / nlk_dev_strip_group
 *                                       the three phases of the frame functions:
 *                                       :605-857 (search, selection, groups), :597-600 +
 *                                       :930-931 (processed mask), :713-932 (filtering)
 *   nlk_dev_frame_accumulate/_normalize the same two functions split at
 *                                       src/nlkalman.c:939 / :1853 so that row
 *                                       strips can exchange accumulator halos
 *   nlk_dev_tvl1_flow                   lib/tvl1flow/tvl1flow_lib.c:345-474
 *                                       (Dual_TVL1_optic_flow_multiscale)
 *   nlk_tvl1_default_params / _scales   lib/tvl1flow/main.c:26-35, 152-157
 *   nlk_dev_bm_flow                     (none: hierarchical block matching, stated by tests/bmflow_ref.py)
 *   nlk_dev_gray                        lib/iio/iio.c:1048-1056 (what the flow tool's
 *                                       reader does to a colour image)
 *   nlk_dev_occlusion_mask              scripts/nlkalman-seq.sh:70-73 (plambda)
 *   nlk_dev_image_dct / nlk_dev_copy_block  lib/multiscale/multiscaler.cpp:21-107 and the
 *                                       coefficient copies of decompose / recompose
 *   nlk_dev_lz3_down / _up / _recompose_step  lib/ms-lanczos3 (lanczos3_down, lanczos3_up and
 *                                       one level of the recompose)
 *   nlk_dev_awgn                        lib/imscript-lite/src/awgn.c (SRAND=seed awgn sigma in out),
 *                                       scripts/nlkalman-seq-gt.sh:30-39
 *   nlk_dev_sqdiff_sum                  the squared-error sum of scripts/psnr.sh:9 (plambda
 *                                       "x y - 2 ^" | imprintf "%v"), times the sample count
 *   nlk_dev_estimate_sigma              nothing: the reference is told sigma; this measures it
 *   nlk_dev_estimate_noise_curve, nlk_dev_vst_forward / _inverse, nlk_dev_noise_affine
 *                                       nothing: the reference knows white noise only
 *   nlk_nlf_build, nlk_dev_nlf_forward / _inverse
 *                                       nothing, likewise
 *   nlk_dev_ssim                        nothing: the reference measures the squared error only
 *   nlk_dev_probe_add, nlk_dev_sure_terms, nlk_sure_mse
 *                                       nothing: the reference measures against clean frames only
 *   nlk_dev_yuv_to_rgb / nlk_dev_rgb_to_yuv, nlk_yuv_format_from_tag, nlk_yuv_frame_bytes
 *                                       nothing: the reference reads and writes RGB image files only
 *   nlk_dev_despike                     nothing: the reference has no counterpart (it models Gaussian noise only)
 *   nlk_dev_defect_step, nlk_defect_schedule
 *                                       nothing: the reference has no counterpart
 */
#ifndef NLK_HIP_H
#define NLK_HIP_H

#include <stddef.h>
#include <stdint.h>
#include "nlkalman.h"

#ifdef __cplusplus
extern "C" {
#endif

enum {
  NLK_OK = 0,
  NLK_ENODEV = -1,   /* no HIP device / device index out of range */
  NLK_EHIP = -2,     /* a HIP runtime call failed */
  NLK_EINVAL = -3,   /* bad argument (NULL image, non-positive size, ...) */
  NLK_EUNSUP = -4,   /* parameter combination the kernels do not cover */
  NLK_ENOMEM = -5
};

typedef struct nlk_ctx nlk_ctx; /* one per (process, device): stream + scratch */

/* per-kernel device time of a frame call, milliseconds (HIP events recorded on
 * the context's stream around each kernel; only when profiling is enabled) */
struct nlk_timings {
  float layout_ms;    /* HWC -> planar copies + validity map */
  float match_ms;     /* block matching + k-NN selection */
  float commit_ms;    /* processed-mask replay */
  float group_ms;     /* DCT + statistics + shrinkage + IDCT + aggregation */
  float normalize_ms; /* accumulator normalisation */
  float total_ms;
};

int nlk_device_count(void);
int nlk_ctx_create(nlk_ctx **ctx, int device);
void nlk_ctx_destroy(nlk_ctx *ctx);
const char *nlk_last_error(const nlk_ctx *ctx); /* ctx may be NULL: last global error */
int nlk_ctx_set_profiling(nlk_ctx *ctx, int on);
/* mean over the frame calls made since nlk_ctx_set_profiling(ctx, 1); synchronises */
int nlk_ctx_get_timings(nlk_ctx *ctx, struct nlk_timings *t);
/* Deterministic aggregation: two calls on the same inputs give bit-identical outputs. By default the
 * group kernels add their accumulator tiles to the frame with global float atomics, whose order
 * varies from run to run (as the reference's `omp atomic` adds do, src/nlkalman.c:923-931); with
 * this switch every workgroup writes its tile to a slab of its own and a gather kernel sums the
 * slabs in a fixed order. Also set by NLK_DETERMINISTIC=1 in the environment at context creation. */
int nlk_ctx_set_deterministic(nlk_ctx *ctx, int on);
/* The NLK_* environment switches (variants for comparison tests and experiments: DESIGN.md appendix) are read
 * once, by nlk_ctx_create. This reads them again - for `ctx`, or for every live context of the process when
 * ctx is NULL (the test suite changes the environment under live contexts). */
int nlk_ctx_reload_switches(nlk_ctx *ctx);
/* What the context's last group launch ran - a read-only report for tests and tools (a test that forces a tile shape
 * with NLK_GTX / NLK_GTY must see that this shape is what ran). Written after the launch is enqueued; nothing on a
 * launch path reads it. A frame worked in bands or strips reports its last launch.
 *   out[0]  kernel family: NLK_GROUP_FAMILY_OTHER (another launcher ran, or none yet), _8M (k_group8m)
 *   out[1]  DCT form of k_group8m (NLK_GROUP_SEP: 0, 2 or 6)
 *   out[2..7]  pass 0: tgx, tgy (targets per tile), ntx, nty (tiles), nty_full (tile rows of tgy grid rows; the
 *              nty - nty_full after them hold one grid row each), single (last grid rows, one target per workgroup)
 *   out[8]  launches (2: deterministic mode's near and far pass of a temporal frame)
 *   out[9]  reach of the mask replay inside the launch (0: the replay is not in the launch)
 *   out[10..11]  far pass: tgx, tgy (0 when there is none) */
enum { NLK_GROUP_FAMILY_OTHER = 0, NLK_GROUP_FAMILY_8M = 1 };
int nlk_ctx_last_group_shape(nlk_ctx *ctx, int out[12]);
/* ... and whether that launch was k_group8m's packed-list instantiation, which reads a tile's candidate and member
 * lists as one word per lane (csrc/nlk_common.h; NLK_PACKED_LISTS=0 keeps the 32-bit lists): bit 0 = pass 0,
 * bit 1 = the far pass of deterministic mode; 0 after any other launcher; negative for a null context. */
int nlk_ctx_last_group_packed(nlk_ctx *ctx);
/* run the context's work on an externally owned hipStream_t; NULL is the legacy
 * default stream itself (what torch.cuda.current_stream() is unless changed), so
 * that the kernels order with the caller's own work on that stream.
 * nlk_ctx_use_own_stream switches back to the context's private stream. */
/* Every entry point puts ALL its launches, memsets and copies on that stream, or behind it: a call that also uses
 * the context's second stream (frames worked in bands, NLK_BANDS) starts that stream behind the work already on the
 * caller's and joins it back before it returns, so the caller's stream alone orders the call with the work before and
 * after it (tests/test_stream_order.py holds every entry point to this).
 * Which calls wait for the device. The nlk_dev_* entry points only enqueue, with these exceptions: nlk_dev_tvl1_flow
 * reads its solver state back while it runs and returns with the flow complete; a frame or strip call waits once when
 * it meets a patch size other than the last one's (it uploads the DCT and window tables), nlk_dev_nlf_forward /
 * _inverse once per new table; any call may wait when a scratch buffer of the context has to grow (the old one is
 * freed). A context that has run a call of the same sizes and parameters before runs it again without waiting.
 * nlk_h2d, nlk_d2h, nlk_sync, nlk_dev_free, nlk_ctx_read_records, nlk_ctx_flush_active, nlk_ctx_count_packed,
 * nlk_ctx_get_timings and the host-pointer frame calls wait by definition. */
int nlk_ctx_set_stream(nlk_ctx *ctx, void *hip_stream);
int nlk_ctx_use_own_stream(nlk_ctx *ctx);
void *nlk_ctx_get_stream(nlk_ctx *ctx);

/* device memory + transfers (so that C callers need no HIP headers) */
int nlk_dev_alloc(nlk_ctx *ctx, void **dptr, size_t bytes);
int nlk_dev_free(nlk_ctx *ctx, void *dptr);
int nlk_h2d(nlk_ctx *ctx, void *dst_dev, const void *src_host, size_t bytes);
int nlk_d2h(nlk_ctx *ctx, void *dst_host, const void *src_dev, size_t bytes);
int nlk_d2d(nlk_ctx *ctx, void *dst_dev, const void *src_dev, size_t bytes);
int nlk_sync(nlk_ctx *ctx);
/* building blocks of the row-strip split across devices (host/multidev.c): clear, dst += src on
 * device memory, and a copy between two contexts' devices (hipMemcpyPeerAsync on dst_ctx's stream,
 * after everything enqueued so far on src_ctx's stream) */
int nlk_dev_zero(nlk_ctx *ctx, void *dptr, size_t bytes);
int nlk_dev_add(nlk_ctx *ctx, float *dst, const float *src, size_t count);
int nlk_dev_copy_peer(nlk_ctx *dst_ctx, void *dst, nlk_ctx *src_ctx, const void *src, size_t bytes);
/* page-locked host memory: transfers from / to it run at the link's rate instead of through a
 * staging copy (file-based callers that keep a pool of frame buffers: host/main_seq.c) */
int nlk_host_alloc(nlk_ctx *ctx, void **hptr, size_t bytes);
int nlk_host_free(nlk_ctx *ctx, void *hptr);

/* image helpers on device-resident HWC images (asynchronous on the ctx stream) */
int nlk_dev_rgb2opp(nlk_ctx *ctx, float *im, int w, int h, int ch);
int nlk_dev_opp2rgb(nlk_ctx *ctx, float *im, int w, int h, int ch);
int nlk_dev_warp_bicubic(nlk_ctx *ctx, float *imw, const float *im,
                         const float *of, const float *msk, int w, int h, int ch);

/* whole-frame hot path on device-resident images; deno0/bsic1 may be NULL */
int nlk_dev_filter_frame(nlk_ctx *ctx, float *deno1, const float *nisy1,
                         const float *deno0, const float *bsic1, int w, int h,
                         int ch, float sigma, const struct nlkalman_params *prms);
int nlk_dev_smooth_frame(nlk_ctx *ctx, float *smoo1, const float *filt1,
                         const float *smoo0, const float *bsic1, int w, int h,
                         int ch, float sigma, const struct nlkalman_params *prms);

/* the same two functions on HOST images (pageable memory, what src/nlkalman.h:46-53 hands over): the frame
 * travels over PCIe in row bands while the bands before it are matched and filtered, and the finished rows
 * travel back while the last bands are filtered. Synchronous: the output is complete on return. */
int nlk_filter_frame_host(nlk_ctx *ctx, float *deno1, const float *nisy1, const float *deno0,
                          const float *bsic1, int w, int h, int ch, float sigma,
                          const struct nlkalman_params *prms);
int nlk_smooth_frame_host(nlk_ctx *ctx, float *smoo1, const float *filt1, const float *smoo0,
                          const float *bsic1, int w, int h, int ch, float sigma,
                          const struct nlkalman_params *prms);

/* ---- optical flow between two frames: the dual TV-L1 method the
 * pipelines run before every filter call (scripts/nlkalman-seq.sh:57-66). Images are
 * single-channel float (w*h); `flow` receives w*h interleaved (u, v) pairs, the layout
 * nlk_dev_warp_bicubic and the .flo files use. I1(x + flow(x)) ~ I0(x). */
struct nlk_tvl1_params {
  float tau;      /* time step (0.25) */
  float lambda;   /* data attachment weight (0.15) */
  float theta;    /* tightness (0.3) */
  int nscales;    /* pyramid levels actually used: cap it with nlk_tvl1_scales() */
  int fscale;     /* finest level that is solved; finer ones get the upsampled flow */
  float zfactor;  /* pyramid factor (0.5) */
  int nwarps;     /* warps per level (5) */
  float epsilon;  /* stop when the mean squared update <= epsilon^2 (0.01) */
};
void nlk_tvl1_default_params(struct nlk_tvl1_params *p);
/* number of levels the reference's command line derives from the image size */
int nlk_tvl1_scales(int w, int h, int nscales, float zfactor);
/* `iterations` (may be NULL) receives the total number of fixed-point iterations */
int nlk_dev_tvl1_flow(nlk_ctx *ctx, float *flow, const float *I0, const float *I1, int w, int h,
                      const struct nlk_tvl1_params *prms, int *iterations);
/* luminance .299 R + .587 G + .114 B of an interleaved image (ch >= 3), copy of channel 0 otherwise */
int nlk_dev_gray(nlk_ctx *ctx, float *gray, const float *im, int w, int h, int ch);
/* 255 where |backward-difference divergence of the flow| > th, else 0 */
int nlk_dev_occlusion_mask(nlk_ctx *ctx, float *mask, const float *flow, int w, int h, float th);
/* The inverse of a flow by fixed-point steps (the lag-1 smoother's forward flow from the filter's backward flow,
 * DESIGN.md §9; restated in numpy by tests/flowinv_ref.py):
 *   inv(q) = F_iters(q),  F_0(q) = -B(q),  F_{k+1}(q) = -B~(q + F_k(q))   (B = flow, w*h interleaved (u, v) pairs)
 * B~ is the bilinear interpolation of B at (x + F.u, y + F.v), float32, every operation rounded by itself (no
 * contraction), in this order:
 *   X = fminf(fmaxf(x + F.u, 0), w - 1), Y likewise with h - 1;
 *   x0 = (int)floorf(X) clamped to 0 .. w - 1, x1 = min(x0 + 1, w - 1), fx = X - x0, the same in y;
 *   per component top = B00 + fx (B01 - B00), bot = B10 + fx (B11 - B10), val = top + fy (bot - top);  F = -val.
 * iters = 0 gives -B. The indices are clamped after the conversion, so no input, non-finite ones included, makes the
 * kernel read outside the array; what a non-finite B gives is unspecified at the pixels whose steps read it, and only
 * there. The same input gives the same bits. One pass, no scratch, no atomics, h <= 262140 (more rows: NLK_EUNSUP);
 * asynchronous on the context's stream. NLK_EINVAL for w or h < 1, iters outside 0..16, a NULL pointer or
 * inv == flow (the arrays must not overlap); the context keeps working after a refused call. */
int nlk_dev_flow_invert(nlk_ctx *ctx, float *inv, const float *flow, int w, int h, int iters);
/* A second, much cheaper flow estimator for consumers that tolerate its error (the sequence recursion: the matcher
 * searches +-5 px after the warp, the Kalman gain absorbs misalignment): hierarchical block matching.
 * Same images, layout and direction as nlk_dev_tvl1_flow: I1(q + flow(q)) ~ I0(q). Stated once, in numpy, by
 * tests/bmflow_ref.py; for finite images the kernels give its bits (float32, every operation rounded by itself), the
 * same on every run. A pyramid of 2 x 2 box means, levels added while min(w, h) / 2 >= min_side (below 8: 8); from the
 * coarsest level to level min(fscale, levels): 8 x 8 blocks at stride 4, each predicted by the coarser level's flow,
 * matched by SSD over [-radius, radius]^2 around the prediction with a parabola per axis for the sub-pel part, a 3 x 3
 * median over the block grid, bilinear interpolation between the block centres; x2 bilinear upsampling from that level
 * to level 0. An image with a side below 8 has the flow 0. */
struct nlk_bmflow_params {
  int fscale;   /* finest level that is matched; finer ones get the upsampled flow (1) */
  int radius;   /* search radius around the prediction, 1..3 (2) */
  int min_side; /* no pyramid level with a side below this (16) */
};
void nlk_bmflow_default_params(struct nlk_bmflow_params *p);
/* prms = NULL: the defaults. Asynchronous on the context's stream; its scratch belongs to the context, is sized for
 * every fscale and min_side at once (about 1.7 floats per pixel) and so grows only with the image size. No input, non-finite ones included, makes a kernel read outside an array; what a non-finite
 * image gives is unspecified. NLK_EINVAL for a NULL image, w or h < 1, radius outside 1..3 or fscale < 0; NLK_EUNSUP
 * for h > 262137; the context keeps working after a refused call. */
int nlk_dev_bm_flow(nlk_ctx *ctx, float *flow, const float *I0, const float *I1, int w, int h,
                    const struct nlk_bmflow_params *prms);

/* ---- multiscale wrapper (reference: lib/multiscale/multiscaler.cpp:21-107).
 * nlk_dev_image_dct: in-place whole-image DCT of an HWC image — forward = FFTW REDFT10 in both
 * directions divided by 4*w*h (dct_inplace), inverse = REDFT01 (idct_inplace).
 * nlk_dev_copy_block: the top-left bw x bh block of coefficients of `src` (row length sw)
 * into `dst` (row length dw): what decompose / recompose / merge_coarse do between transforms
 * (decompose.cpp:40-46, recompose.cpp:43-49, merge_coarse.cpp:37-43). */
int nlk_dev_image_dct(nlk_ctx *ctx, float *img, int w, int h, int ch, int inverse);
int nlk_dev_copy_block(nlk_ctx *ctx, float *dst, int dw, const float *src, int sw, int ch, int bw, int bh);

/* ---- Lanczos-3 pyramid of the lz3 multiscale pipeline (scripts/msnlkalman-lz3-seq.sh; the reference's
 * lib/ms-lanczos3 tools; the operations are written out in DESIGN.md §9). HWC images, any w, h, ch >= 1;
 * bit-reproducible (no atomics).
 * nlk_dev_lz3_down: dst (ceil(w/2) x ceil(h/2)) = the 12-tap Lanczos-3 half-band downsampling of src.
 * nlk_dev_lz3_up: dst (dw x dh) = the 2x Lanczos-3 upsampling of src (w x h), fitted to dw, dh: each must be
 *   2n - 1 (last sample dropped), 2n or 2n + 1 (last sample repeated), else NLK_EINVAL.
 * nlk_dev_lz3_recompose_step: one level of the recompose,
 *   out (w x h) = yh + up(gblur(rl - down(yh), g), w, h)
 *   with rl the recomposed coarser level (wl x hl = ceil(w/2) x ceil(h/2)) and gblur the separable Gaussian of
 *   max(2 floor(g), 5) taps with a half-sample symmetric boundary (g = 0: none; 0 <= g < 33). Its down is
 *   nlk_dev_lz3_down's kernel, so a level left as decomposed recomposes bit for bit. out may be yh, not rl. */
int nlk_dev_lz3_down(nlk_ctx *ctx, float *dst, const float *src, int w, int h, int ch);
int nlk_dev_lz3_up(nlk_ctx *ctx, float *dst, int dw, int dh, const float *src, int w, int h, int ch);
int nlk_dev_lz3_recompose_step(nlk_ctx *ctx, float *out, const float *yh, int w, int h, const float *rl, int wl,
                               int hl, int ch, float g);

/* ---- noise and error measure of the ground-truth loop (scripts/nlkalman-seq-gt.sh). Both are
 * asynchronous on the context's stream; n = 0 is allowed.
 * nlk_dev_awgn: out[i] = in[i] + sigma * N_i (i < n, HWC order): what `SRAND=seed awgn sigma in out` writes
 *   (lib/imscript-lite/src/awgn.c:24-26, random.c), bit for bit: the LCG reached by jump-ahead, the Box-Muller
 *   cosine branch in double in the reference's expression order, no contraction. out may be in.
 * nlk_dev_sqdiff_sum: *sum (one device double) = sum of (a[i] - b[i])^2 over i < n in double, in a fixed order
 *   (bit-reproducible: no atomics). Sums of several calls may go to consecutive doubles of one buffer and be
 *   downloaded once. */
int nlk_dev_awgn(nlk_ctx *ctx, float *out, const float *in, size_t n, float sigma, uint32_t seed);
int nlk_dev_sqdiff_sum(nlk_ctx *ctx, double *sum, const float *a, const float *b, size_t n);

/* ---- quality measure (restated in numpy by tests/ssim_ref.py): the structural similarity of Wang,
 * Bovik, Sheikh and Simoncelli (2004) in its usual form: Gaussian window, population moments, valid region.
 *   Inputs     a (the reference) and b: HWC float32 images, w >= 11, h >= 11, 1 <= ch <= 16; range = the dynamic
 *              range L, positive and finite (the tools use 255)
 *   Window     g[k] = exp(-(k - 5)^2 / (2 * 1.5^2)), k = 0..10, divided by its sum, made in double on the host; the
 *              2-D weight is g[i] g[j]
 *   Moments    every channel by itself. At each of the (w - 10)(h - 10) valid positions 5 <= x < w - 5,
 *              5 <= y < h - 5 the five window moments mu_a, mu_b, E[a^2], E[b^2], E[ab] are accumulated in double over
 *              the 121 samples, separably (rows, then columns); the float samples are converted first, so every
 *              product of two samples is exact
 *   Variances  var_a = E[a^2] - mu_a^2, var_b likewise, cov = E[ab] - mu_a mu_b
 *   Constants  C1 = (0.01 L)^2, C2 = (0.03 L)^2
 *   Value      S = (2 mu_a mu_b + C1)(2 cov + C2) / ((mu_a^2 + mu_b^2 + C1)(var_a + var_b + C2)), in double
 *   Pooling    ssim_c = the mean of S over the valid positions of channel c; ssim = the mean of the ssim_c
 * Sums are in double, in an order that depends on w, h, ch alone, without atomics: the same input gives the same bits
 * on every call. Non-finite samples are not special-cased: every position whose window holds one gets a non-finite S
 * (its channel's mean and ssim are then NaN), and no other position is affected.
 * d_ssim[0] = ssim, d_ssim[1 + c] = ssim_c (device doubles; several calls may write to consecutive slots of one
 * buffer that is downloaded once, as with nlk_dev_sqdiff_sum). d_map may be NULL; otherwise it is [h - 10][w - 10][ch]
 * float32 and receives S of every position. Asynchronous on the context's stream; the scratch is kept in the context
 * and grows on demand. NLK_EINVAL for w < 11, h < 11, ch outside 1..16, a range that is not positive and finite, or
 * a NULL pointer other than d_map; the context keeps working after a refused call. */
int nlk_dev_ssim(nlk_ctx *ctx, double *d_ssim, float *d_map, const float *d_a, const float *d_b, int w, int h, int ch,
                 float range);

/* ---- error estimate without clean frames (restated in numpy by tests/sure_ref.py): Stein's unbiased
 * risk estimate with the divergence taken by one Monte-Carlo probe (Ramani, Blu, Unser 2008). For a frame y of N
 * samples under white Gaussian noise of deviation sigma, f = the filter's output and b a vector of independent signs,
 *     MSE_hat = R / N - sigma^2 + 2 sigma^2 D / (eps N),  R = sum (y_i - f_i)^2,  D = sum b_i (f(y + eps b)_i - f(y)_i)
 *   Sign       of sample i under a 64-bit seed, all arithmetic mod 2^64:
 *                z = seed + (i + 1) 0x9E3779B97F4A7C15;  z = (z ^ z >> 30) 0xBF58476D1CE4E5B9;
 *                z = (z ^ z >> 27) 0x94D049BB133111EB;   z ^= z >> 31;   b_i = -1 if bit 63 of z is set, else +1
 *              It is recomputed wherever it is needed and never stored.
 * nlk_dev_probe_add: out[i] = in[i] + (b_i > 0 ? eps : -eps) for i < n, one float add (a float32 numpy restatement
 *   gives the same bits). out may be in; n = 0 is allowed; eps must be finite.
 * nlk_dev_sure_terms: the two sums of the HWC images y (noisy), f = filter(y), fp = filter(y + eps b), every channel
 *   by itself, i = (y w + x) ch + c:  R_c = sum ((double)y - (double)f)^2,  D_c = sum b_i ((double)fp - (double)f).
 *   d_total[2 c] = R_c, d_total[2 c + 1] = D_c (2 ch device doubles; several calls may write to consecutive slots of
 *   one buffer that is downloaded once). d_blocks may be NULL; otherwise it is [nby][nbx][ch][2] device doubles, nbx =
 *   ceil(w / block), nby = ceil(h / block), and receives the same two sums over every block x block tile (ragged at
 *   the right and bottom): the risk map. 4 <= block <= 64 (it also sets the order of summation when there is no map),
 *   1 <= ch <= 16, w, h >= 1. Sums are in double in an order that depends on (w, h, ch, block) alone, without atomics:
 *   the same input gives the same bits on every call; the totals are the tiles' sums added in a fixed order by a
 *   second launch. Non-finite samples are not special-cased: one makes the terms it enters non-finite - those of its
 *   own tile and channel (y: R; fp: D; f: both) and that channel's totals - and nothing else.
 *   Asynchronous on the context's stream; the scratch (used when d_blocks is NULL) is kept in the context and grows
 *   on demand.
 * Both: NLK_EINVAL for an argument outside what is stated or a NULL pointer other than d_blocks; the context keeps
 *   working after a refused call.
 * nlk_sure_mse: the formula on the host, from sums over n samples (of one channel, or added over the channels). */
int nlk_dev_probe_add(nlk_ctx *ctx, float *out, const float *in, size_t n, float eps, uint64_t seed);
int nlk_dev_sure_terms(nlk_ctx *ctx, double *d_total, double *d_blocks, const float *d_y, const float *d_f,
                       const float *d_fp, int w, int h, int ch, int block, uint64_t seed);
double nlk_sure_mse(double R, double D, double n, double sigma, double eps);

/* ---- noise level of an image (restated in numpy by tests/sigma_ref.py): a block-DCT percentile
 * estimator. HWC image on the 0..255 scale, w, h >= 8, ch >= 1; every channel by itself:
 *   1. every 8 x 8 block with top-left (x, y), x % step == 0, y % step == 0, x <= w - 8, y <= h - 8; a block
 *      holding a non-finite sample is skipped (warped frames carry NaN); N_c blocks are kept
 *   2. Y = C B C^T, C the orthonormal DCT-II (the filter's basis at patch size 8)
 *   3. L = the sum of Y[i][j]^2 over 1 <= i + j <= low_max
 *   4. K = min(N_c, max(kmin, ceil(frac N_c))) (the product in double); T = the K-th smallest L, found exactly;
 *      the selection is every block with L <= T, n_c >= K of them
 *   5. the mean of Y[i][j]^2 over the selection for each (i, j) with i + j >= high_min, summed in double in an
 *      order that depends on the sizes and parameters alone
 *   6. sigma_c^2 = the median of those means (the mean of the two middle ones for an even count)
 * and the pooled sigma = sqrt(mean_c sigma_c^2). Under white noise L and the high coefficients are independent,
 * so selecting on L does not bias the means; on a textured image it picks the flat blocks.
 * nlk_dev_estimate_sigma writes d_sigma[0] = sigma, d_sigma[1 + c] = sigma_c and, where d_counts is not NULL,
 * d_counts[2c] = N_c, d_counts[2c + 1] = n_c (device arrays). Asynchronous on the context's stream; its scratch is
 * kept in the context and grows on demand; the same input gives the same bits. A channel without a block gives
 * sigma_c = NaN and the counts 0, 0 (the pooled value is then NaN). NLK_EINVAL for w < 8, h < 8, step < 1, frac
 * outside (0, 1], low_max or high_min outside 1..14. prms = NULL: the defaults {4, 0.05, 64, 5, 8}. */
struct nlk_sigma_params {
  int step;      /* block grid step in pixels */
  float frac;    /* fraction of the blocks selected ... */
  int kmin;      /* ... and at least this many (all of them where there are fewer) */
  int low_max;   /* L sums 1 <= i + j <= low_max */
  int high_min;  /* the estimate uses i + j >= high_min */
};
void nlk_sigma_default_params(struct nlk_sigma_params *p);
int nlk_dev_estimate_sigma(nlk_ctx *ctx, float *d_sigma, int *d_counts, const float *d_img, int w, int h, int ch,
                           const struct nlk_sigma_params *prms);

/* ---- signal-dependent noise, var(z | y) = a y + b (shot noise plus a read floor; restated in numpy
 * by tests/curve_ref.py).
 *
 * nlk_dev_estimate_noise_curve measures (a_c, b_c) per channel: nlk_dev_estimate_sigma's estimator run per bin of
 * the block mean, then a line through the bins. With the steps 1-3 of that estimator (blocks, Y, L):
 *   2'. m = the sum of the block's 64 samples in double, in raster order, divided by 64
 *   3'. the bin q = floor((m - lo) / (hi - lo) * nbins) in double (nbins - 1 at most); a block with m outside
 *       [lo, hi) is skipped; N_q blocks are kept in bin q; a bin with N_q < nmin is dropped
 *   4'. per bin K_q = min(N_q, max(kmin, ceil(frac N_q))) (the product in double) and the selection of the bin:
 *       its blocks with L <= the K_q-th smallest L of the bin, found exactly; n_q of them. (One selection over the
 *       frame would pick the dark blocks only.)
 *   5'. v_q = the median over i + j >= high_min of the mean of Y[i][j]^2 over the selection, m_q = the mean of m over
 *       it; sums in double in an order that depends on the sizes and parameters alone
 *   6'. v = a m + b by least squares over the bins kept, weights n_q, in double. With fewer than 2 bins kept, or
 *       sum n (m - mbar)^2 = 0, or a < 0: a = 0, b = sum n v / sum n. Then, if b < 0: a = sum n m v / sum n m^2,
 *       b = 0. With no bin kept: a = b = NaN.
 * d_curve[2c], d_curve[2c + 1] = (a_c, b_c); d_bins (may be NULL) [ch][nbins] receives N_q, n_q, m_q, v_q of every
 * bin (n_q = 0 and m_q = v_q = NaN for a bin dropped or empty). Asynchronous on the context's stream; the scratch is
 * kept in the context and grows on demand; the same input gives the same bits. NLK_EINVAL as nlk_dev_estimate_sigma,
 * and for nbins outside 1..64, hi <= lo (or either not finite), nmin < 1, kmin < 1. prms = NULL: the defaults
 * {4, 0.1, 32, 5, 8, 16, 0, 256, 32}. */
struct nlk_curve_params {
  int step;      /* block grid step in pixels */
  float frac;    /* fraction of a bin's blocks selected ... */
  int kmin;      /* ... and at least this many (all of them where there are fewer) */
  int low_max;   /* L sums 1 <= i + j <= low_max */
  int high_min;  /* the estimate uses i + j >= high_min */
  int nbins;     /* bins of the block mean, 1..64 ... */
  float lo, hi;  /* ... over [lo, hi) */
  int nmin;      /* a bin needs this many blocks */
};
struct nlk_curve_bin {
  int nblocks, nsel; /* N_q, n_q */
  float mean, var;   /* m_q, v_q */
};
void nlk_curve_default_params(struct nlk_curve_params *p);
int nlk_dev_estimate_noise_curve(nlk_ctx *ctx, float *d_curve, struct nlk_curve_bin *d_bins, const float *d_img,
                                 int w, int h, int ch, const struct nlk_curve_params *prms);

/* The generalised Anscombe transform that makes such noise white, per channel c = i mod ch of n samples, with the
 * coefficients ab[2c], ab[2c + 1] = (a_c >= 0, b_c >= 0) (a HOST array) and one scale s for all channels. With
 * u0 = 3 a^2 / 8 + b and u = a y + u0:
 *   forward   g = (2 s / a) (sqrt(max(u, 0)) - sqrt(u0)), evaluated as 2 s y / (sqrt(u) + sqrt(u0)) for u > 0
 *             (stable as a -> 0; s y / sqrt(b) at a = 0). The noise of g has standard deviation s in every channel.
 *   inverse   r = max(g / s, -2 sqrt(u0) / a); mode 0: y = r sqrt(u0) + a r^2 / 4, the algebraic inverse
 *             (inverse(forward(y)) = y); mode 1 adds the closed-form unbiasing terms of Makitalo and Foi,
 *             a (1/4 + (1/4) sqrt(3/2) / D - (11/8) / D^2 + (5/8) sqrt(3/2) / D^3) with
 *             D = max(2 (sqrt(u0) + a r / 2) / a, 2 sqrt(u0) / a); nothing for a = 0.
 * float arithmetic; one pass; out may be in; NaN passes through; asynchronous on the context's stream. NLK_EINVAL
 * for a negative or non-finite coefficient, a_c = b_c = 0, s not a positive finite number, ch outside 1..16, a mode
 * other than 0 and 1.
 * nlk_vst_scale (host only): s = 255 / mean_c(span_c), span_c = 2 * 255 / (sqrt(255 a_c + u0_c) + sqrt(u0_c)), the
 * width of the transform of 0..255 at s = 1: with it a transformed frame keeps the 0..255 range that the filter's
 * sigma-dependent default parameters were tuned on, and its noise level is s. NaN for coefficients the transforms
 * refuse. */
float nlk_vst_scale(const float *ab, int ch);
int nlk_dev_vst_forward(nlk_ctx *ctx, float *out, const float *in, size_t n, int ch, const float *ab, float s);
int nlk_dev_vst_inverse(nlk_ctx *ctx, float *out, const float *in, size_t n, int ch, const float *ab, float s,
                        int mode);

/* ---- a noise-level function of any shape (gamma-encoded, tone-mapped video: DESIGN.md §9; restated in numpy by
 * tests/nlf_ref.py). The bins of nlk_dev_estimate_noise_curve, without its line: a monotone piecewise-linear map per
 * channel, with a knot at every bin edge, that makes the noise white.
 *
 * nlk_nlf_build (host only, double arithmetic, plain C: host/nlf_build.c links by itself) makes the table from the
 * bins [ch][nbins] of one frame, downloaded, and the lo, hi, nbins they were measured with. Per channel:
 *   a. K = the bins with n_q > 0 and v_q finite and > 0, in increasing q. A channel with an empty K makes the table
 *      invalid: s = NaN (the other fields are then not to be used)
 *   b. over neighbours in K (not in q): vs_k = (n_{k-1} v_{k-1} + 2 n_k v_k + n_{k+1} v_{k+1}) /
 *      (n_{k-1} + 2 n_k + n_{k+1}), a missing neighbour left out of both sums
 *   c. vs_k = max(vs_k, rho^2 median(vs)) (the mean of the two middle values for an even count): a clipped end, where
 *      the measured variance collapses, gets a bounded gain
 *   d. knots x_j = lo + j (hi - lo) / nbins, j = 0..nbins; v(x_j) = the linear interpolation of (m_k, vs_k), constant
 *      outside [m_first, m_last]; sigma_j = sqrt(v(x_j))
 *   e. at s = 1: kappa_j = 2 / (sigma_j + sigma_{j+1}), g(x_0) = 0, g(x_{j+1}) = g(x_j) + kappa_j (x_{j+1} - x_j); the
 *      end segments extend linearly, so g is a bijection of the real line
 *   f. span_c = g_c(255) - g_c(0), s = 255 / mean_c span_c: as with nlk_vst_scale the transformed frame keeps the
 *      0..255 range, and s is the noise level of the run
 *   g. x[j], G[c][j] = (float)(s (g_c(x_j) - g_c(0))) (black stays 0), slope[c][j] = (float)(s kappa_j),
 *      islope[c][j] = (float)(1 / (s kappa_j)), inv_dx = (float)(nbins / (hi - lo)); sigma[c][j] = (float)sigma_j and
 *      kept[c] = |K| for reports
 * NLK_EINVAL for a NULL argument, ch outside 1..16, nbins outside 1..64, hi <= lo (or either not finite), rho outside
 * (0, 1]; NLK_OK otherwise, also for an invalid table. NLK_NLF_RHO is the rho of the tools.
 *
 * nlk_dev_nlf_forward / nlk_dev_nlf_inverse apply it to n samples, the channel of sample i being i mod ch = the
 * table's ch. float arithmetic, every operation rounded by itself:
 *   forward   t = fminf(fmaxf((y - lo) inv_dx, 0), nbins - 1), j = (int)floorf(t), g = G[j] + (y - x[j]) slope[j]
 *   inverse   j = the number of k in 1..nbins-1 with G[k] <= g, y = x[j] + (g - G[j]) islope[j]
 * NaN gives NaN, +-inf passes through. The inverse is the algebraic one; it has no unbiasing term (a locally linear
 * map needs none to first order). One pass; out may be in; asynchronous on the context's stream. The context keeps
 * the device copy of the last table it was given: a table is uploaded when it differs from that one (which waits for
 * the stream once), not on every call. NLK_EINVAL for a NULL argument, a table whose s is not positive and finite, and
 * ch != the table's. */
#define NLK_NLF_MAX_CH 16
#define NLK_NLF_MAX_BINS 64
#define NLK_NLF_RHO 0.25f
struct nlk_nlf_table {
  int ch, nbins;
  float lo, hi, inv_dx;
  float s;                                  /* the scale = the sigma of the run; NaN: a channel kept no bin */
  int kept[NLK_NLF_MAX_CH];                 /* |K| per channel */
  float x[NLK_NLF_MAX_BINS + 1];            /* knots, [0..nbins] */
  float G[NLK_NLF_MAX_CH][NLK_NLF_MAX_BINS + 1];      /* [0..nbins] */
  float slope[NLK_NLF_MAX_CH][NLK_NLF_MAX_BINS + 1];  /* [0..nbins-1] (the rest 0) */
  float islope[NLK_NLF_MAX_CH][NLK_NLF_MAX_BINS + 1]; /* [0..nbins-1] */
  float sigma[NLK_NLF_MAX_CH][NLK_NLF_MAX_BINS + 1];  /* sigma_j of the frame's own scale, [0..nbins] */
};
int nlk_nlf_build(struct nlk_nlf_table *t, const struct nlk_curve_bin *bins, int ch, int nbins, float lo, float hi,
                  float rho);
int nlk_dev_nlf_forward(nlk_ctx *ctx, float *out, const float *in, size_t n, int ch, const struct nlk_nlf_table *t);
int nlk_dev_nlf_inverse(nlk_ctx *ctx, float *out, const float *in, size_t n, int ch, const struct nlk_nlf_table *t);

/* ---- defective pixels (stuck, hot and dead sensor sites, single-sample impulses: DESIGN.md §9; the rule is stated in
 * float32 numpy by tests/despike_ref.py). Every channel of the HWC image by itself:
 *   ring of (x, y)   the samples at Chebyshev distance exactly `radius`: 8 values for radius 1, 16 for radius 2
 *   border indices   along an axis of n samples: j = |i|; j = 2 (n - 1) - j if j >= n; then clamped to [0, n - 1] (a
 *                    reflection that does not repeat the edge; a 1 x 1 image is its own ring and is never changed)
 *   mn, mx           the ring's minimum and maximum; lo, hi its two middle order statistics (4th and 5th of 8, 8th and
 *                    9th of 16); med = (lo + hi) * 0.5f, one rounding each
 *   hit              v > mx + thr or v < mn - thr, one float add / subtract each: out = med. Anything else is copied bit
 *                    for bit, and so is a sample that is non-finite or whose ring holds a non-finite value
 * -0 and +0 compare equal; the sign of a replaced value that equals zero is unspecified. radius 2 is for an impulse
 * that reaches the RGB frame as a 2 x 2 blob (a chroma sample of a 4:2:0 stream, a defect that went through a
 * demosaic): no pixel of such a blob has another on its distance-2 ring. A blob on the border reflects onto itself and
 * is partly missed: a stated limit.
 * d_count: NULL, or ch device words: the call zeroes them and adds the replaced samples of every channel with integer
 * atomics (order-free: the same bits on every call, like the image). Asynchronous on the context's stream. NLK_EINVAL
 * for w or h < 1, ch outside 1..16, a radius other than 1 and 2, a thr that is not finite and >= 0, a NULL ctx, out or
 * in, and out == in (the stencil reads its neighbours): nothing is written and the context keeps working. NLK_EUNSUP
 * for a row of 2^31 floats or more. */
int nlk_dev_despike(nlk_ctx *ctx, float *out, const float *in, uint32_t *d_count, int w, int h, int ch, int radius,
                    float thr);

/* ---- a defect map learned over time (the rule and the schedule are stated in float32 numpy by
 * tests/defectmap_ref.py). A sensor defect sits at the same coordinates in every frame, scene and noise do not: the mean
 * of the noisy frames, taken without motion compensation, carries noise sigma / sqrt(T) while the defect keeps its
 * height, and nlk_dev_despike's range test read on that mean, at a threshold that shrinks as 1 / sqrt(T), finds what
 * the test on one frame cannot. One call per frame, every channel of the HWC frame by itself (ring, border indices, mn,
 * mx, lo, hi: as nlk_dev_despike's), every operation rounded by itself:
 *   hit        mean_in > mx + thr or mean_in < mn - thr on mean_in's ring; none where mean_in or its ring is non-finite
 *   out        at a hit (lo + hi) * 0.5f of in's ring, if in and its ring are all finite; anything else is `in`, bit for bit
 *   mean_out   mean_in + (in - mean_in) * gain for a finite `in`, else mean_in: the raw sample at a hit too (a flagged
 *              site that lost its evidence would flicker)
 * mean_in == NULL is the first frame: out = in, mean_out = in (0 at a non-finite sample), no hit; thr and gain are
 * checked and not used. The caller keeps two mean planes and swaps them. d_map: NULL, or w * h * ch bytes, every one
 * written: 1 = hit. d_count: NULL, or ch device words: the call zeroes them and adds the replaced samples of every
 * channel with integer atomics (the same bits on every call, like the planes). Asynchronous on the context's stream.
 * NLK_EINVAL for what nlk_dev_despike refuses (mean_out as out), a gain outside (0, 1], and any overlap among out, in,
 * mean_out and mean_in (the stencil reads the neighbours of both inputs): nothing is written and the context keeps
 * working. NLK_EUNSUP for a row of 2^31 floats or more. */
int nlk_dev_defect_step(nlk_ctx *ctx, float *out, const float *in, float *mean_out, const float *mean_in,
                        uint8_t *d_map, uint32_t *d_count, int w, int h, int ch, int radius, float thr, float gain);
/* the threshold and gain of the frame of index t >= 1 (the first frame, t = 0, needs neither) for a window of n_window
 * frames and k_sigma = K * sigma: gain = 1f / (float)min(t + 1, N), thr = k_sigma * sqrtf(1f / (float)min(t, N)): an
 * exact mean up to N frames, then an exponential window, whose noise is below sigma / sqrt(N), so that the threshold
 * stays on the safe side. Host only, plain C (host/defect_schedule.c). NLK_EINVAL for t < 1, n_window < 1 or a NULL
 * pointer. */
int nlk_defect_schedule(long t, int n_window, float k_sigma, float *thr, float *gain);

/* nlk_dev_awgn with a deviation that follows the signal: out[i] = (float)((double)in[i] + sqrt(max(a_c in[i] + b_c,
 * 0)) g_i), c = i mod ch, g_i exactly the normal deviate nlk_dev_awgn draws for that index and seed; ab as above
 * (host array, finite values, ch in 1..16). out may be in. */
int nlk_dev_noise_affine(nlk_ctx *ctx, float *out, const float *in, size_t n, int ch, const float *ab,
                         uint32_t seed);

/* ---- planar Y'CbCr frames as decoders deliver them (the payload of a YUV4MPEG2 frame) <-> the HWC float RGB image
 * of everything above, on the device (restated in numpy by tests/yuv_ref.py).
 * A frame is the Y plane (w x h samples), then Cb, then Cr (each cw x chh, cw = (w + sx - 1) / sx,
 * chh = (h + sy - 1) / sy), tightly packed: no row padding, plane starts at any byte (17 x 5 at 8 bit: Cb at byte 85).
 * Samples are bytes at depth 8 and little-endian uint16 above. */
struct nlk_yuv_format {
  int mono;        /* 1: luma only (ch = 1); the chroma fields are ignored */
  int sx, sy;      /* chroma subsampling per axis, 1 or 2 */
  int cosited_x;   /* horizontal chroma siting when sx == 2: 0 = centred between luma 2i and 2i+1 (420jpeg),
                      1 = on luma 2i (420mpeg2, 422). Vertical siting is always centred when sy == 2 */
  int depth;       /* bits per sample, 8..16; > 8: little-endian uint16 samples */
  int full_range;  /* 0 = limited (16..235 / 16..240 scaled by 2^(depth-8)), 1 = full */
  int matrix;      /* 601 or 709 */
};
/* host only. The format of a YUV4MPEG2 `C` tag value (NULL or "" when the tag is absent): absent, 420jpeg = 4:2:0
 * centred; 420mpeg2, 420, 420pN = 4:2:0 co-sited; 422, 422pN = 4:2:2 co-sited; 444, 444pN; mono, monoN (N = 9..16).
 * full_range = 0 and matrix = 709: the caller overrides both. Anything else (420paldv, 411, 444alpha, ...):
 * NLK_EUNSUP. */
int nlk_yuv_format_from_tag(struct nlk_yuv_format *f, const char *ctag);
/* host only. Bytes of one frame; 0 for a size < 1, a format field out of range or a size that overflows */
size_t nlk_yuv_frame_bytes(int w, int h, const struct nlk_yuv_format *f);
/* d_rgb: HWC float32 on the 0..255 scale, ch = 3 (ch = 1 for mono: the luma); d_yuv: a frame as above. Float32
 * arithmetic in the order DESIGN.md §9 writes out, without contraction: the same input gives the same bits, and
 * the numpy restatement gives them too. to_rgb interpolates the chroma (centred axis: 3/4, 1/4 of the two nearest
 * samples; co-sited: the sample or the mean of two; indices clamped) and does not clamp the result; to_yuv decimates
 * it (centred: the mean of two; co-sited: 1/4, 1/2, 1/4) and rounds to nearest even, clamped to 0 .. 2^depth - 1 (NaN
 * gives code 0). At 4:4:4 codes -> RGB -> codes is the identity. One pass each, no scratch, no atomics, any w >= 1 and
 * 1 <= h <= 524280 (8 rows per workgroup, 65535 workgroups along y in one launch; more rows: NLK_EUNSUP);
 * asynchronous on the context's stream. NLK_EINVAL for a NULL pointer, a non-positive size or a format field outside
 * the ranges above; the context keeps working after a refused call. */
int nlk_dev_yuv_to_rgb(nlk_ctx *ctx, float *d_rgb, const void *d_yuv, int w, int h, const struct nlk_yuv_format *f);
int nlk_dev_rgb_to_yuv(nlk_ctx *ctx, void *d_yuv, const float *d_rgb, int w, int h, const struct nlk_yuv_format *f);

/* Row-strip form used by the multi-GPU driver. The images are a strip of the
 * frame (h rows) that already contains the search halo; targets are the patch
 * grid rows whose first image row is oy + j*step, j in [0, ngy). `acc` is a
 * planar accumulator of (ch+1) planes of h*w floats (ch weighted sums, then
 * the weights); it is ADDED to, so the caller zeroes it and may add the halo
 * rows received from its neighbours before normalising.
 * smoother != 0 selects the nlkalman_smooth_frame statistics and gain. */
int nlk_dev_frame_accumulate(nlk_ctx *ctx, float *acc, const float *cur,
                             const float *prev, const float *basic, int w, int h,
                             int ch, float sigma,
                             const struct nlkalman_params *prms, int oy, int ngy,
                             int smoother);
/* out[y][x][c] = acc_c / acc_w where acc_w > 1e-6, else cur (rows [y0, y1)) */
int nlk_dev_frame_normalize(nlk_ctx *ctx, float *out, const float *acc,
                            const float *cur, int w, int h, int ch, int y0, int y1);

/* The three phases of nlk_dev_frame_accumulate as separate calls, for an EXACT
 * processed-mask across row strips: every rank runs `strip_match` on its strip
 * and gets one 64-bit mark word per target (grid-relative, so strips can simply
 * be concatenated in grid-row order: an all-gather), `mask_commit` replays the
 * raster order (reference: src/nlkalman.c:597-600, 930-931) over the mark words
 * of the WHOLE patch grid, and `strip_group` processes the strip's targets with
 * its slice of the resulting active flags. `marks_out` / `active` are device
 * buffers of ngx*ngy uint64 / bytes; `reach` receives the R to hand to
 * mask_commit. strip_group (and strip_commit_group) use the state the context's LAST accepted match phase left in it:
 * geometry, planar images and lists of the last nlk_dev_strip_match* call - or of a whole-frame or
 * nlk_dev_frame_accumulate call made since, whose match phase replaces that state like a strip_match over its
 * whole grid would (a strip_group after a whole-frame call is that frame's group phase, acc being a whole-frame
 * accumulator and `active` its ngx * ngy decisions).
 * Refused calls. A frame or strip call refused by its argument checks, before anything is enqueued - a NULL image or
 * parameters, a size below 1, a patch size the kernels do not cover, an image smaller than a patch, target rows that
 * leave the strip, negative radii; for nlk_dev_strip_match*: rows outside the strip's target rows, layout rows outside
 * the strip, a reach above 3 with mark words asked for - leaves that state, and the records of nlk_ctx_read_records,
 * as they were. A call that fails later (a HIP error, an allocation that fails, a matcher that needs more LDS than a
 * workgroup has) has already overwritten part of them: it leaves the context WITHOUT a match state, and
 * nlk_dev_strip_group, nlk_dev_strip_commit_group, nlk_ctx_read_records and nlk_ctx_count_packed return NLK_EINVAL
 * until a frame or strip call has been accepted again. */
int nlk_dev_strip_match(nlk_ctx *ctx, const float *cur, const float *prev,
                        const float *basic, int w, int h, int ch, float sigma,
                        const struct nlkalman_params *prms, int oy, int ngy,
                        int smoother, void *marks_out, int *reach);
/* the same for the target rows [r0, r0 + rows) of the strip only (their records and mark words land at
 * their place in the strip's arrays): lets a rank match the rows that do not depend on the previous
 * frame's halo while that halo is still in flight, and the seam rows afterwards. Every call lays the
 * strip out again (the halo may have arrived in between). */
int nlk_dev_strip_match_rows(nlk_ctx *ctx, const float *cur, const float *prev,
                             const float *basic, int w, int h, int ch, float sigma,
                             const struct nlkalman_params *prms, int oy, int ngy,
                             int smoother, int r0, int rows, void *marks_out, int *reach);
/* the same, laying out only the pixel rows [lay0, lay1) of the strip (planar copies, validity row test) and
 * finishing the validity map of the rows [v0, v1) (row y needs the row tests of rows y .. y + patch - 1): first the
 * own rows and the targets that read nothing else, then - once the previous frame's halo rows have arrived - those
 * rows and the seam targets. Nothing is read while in flight, nothing is laid out twice. */
int nlk_dev_strip_match_part(nlk_ctx *ctx, const float *cur, const float *prev,
                             const float *basic, int w, int h, int ch, float sigma,
                             const struct nlkalman_params *prms, int oy, int ngy,
                             int smoother, int r0, int rows, int lay0, int lay1, int v0, int v1,
                             void *marks_out, int *reach);
/* Strip calls: a planar (ch+1, h, w) accumulator of the strip whose rows nlk_dev_strip_match* clear while they
 * lay the same pixel rows out (all of them over a strip's calls) - saves the caller a separate clear per step.
 * NULL (the default) switches it off. */
int nlk_ctx_set_strip_accumulator(nlk_ctx *ctx, float *acc);
int nlk_dev_mask_commit(nlk_ctx *ctx, const void *marks, int ngx, int ngy, int reach,
                        unsigned char *active);
int nlk_dev_strip_group(nlk_ctx *ctx, float *acc, const unsigned char *active);
/* nlk_dev_mask_commit over the whole grid (`marks`, `active`: ngx * ngy entries) + nlk_dev_strip_group on the strip
 * whose first grid row is gy0, as one call: where the group kernel can replay the mask inside its own launch
 * (8 x 8 patches, reach <= 3, grids up to 2048 targets wide; NLK_NO_CHASE=1 switches it off) only the grid rows down
 * to the strip's last one are replayed, by the launch's first workgroup, while the others already work (`active` is
 * then not written); otherwise exactly the two calls. Same decisions, same sums (reference: src/nlkalman.c:597-600,
 * 930-931). */
int nlk_dev_strip_commit_group(nlk_ctx *ctx, float *acc, const void *marks, int ngx, int ngy, int reach, int gy0,
                               unsigned char *active);
/* After a call whose group kernel replayed the mask itself (whole-frame calls of 8 x 8 patches,
 * nlk_dev_strip_commit_group): write the decision bytes of the replayed grid rows - all of them for a frame call
 * (into the context's records, what nlk_ctx_read_records does first), rows [0, gy0 + the strip's rows) of `active`
 * for a strip - and wait. No-op otherwise. */
int nlk_ctx_flush_active(nlk_ctx *ctx);

/* per-target records of the last frame or strip call that ran a match phase (refused calls: see
 * nlk_dev_strip_match; a whole-frame call on an image smaller than a patch has no targets, runs no match phase and
 * leaves the records of the call before it), copied to host (tests only):
 * active[ngrid] (1 = processed), nsel/np0/nagg[ngrid], topk[ngrid*kmax] and
 * gcoords[ngrid*gmax] packed as x | y << 16. Any pointer may be NULL. */
int nlk_ctx_read_records(nlk_ctx *ctx, int *ngrid, int *kmax, int *gmax,
                         unsigned char *active, int *nsel, int *np0, int *nagg,
                         unsigned int *topk, unsigned int *gcoords);

/* ---- The patch grid of a frame call and its split into row strips (host only, plain C: host/frame_grid.c links by
 * itself). THE statement of both for the frame calls, csrc/strips.hip and host/multidev.c.
 *   step   patch_sz / 2: targets sit at (i * step, j * step), i < ngx, j < ngy
 *   halo   pixel rows any search window or group of the call reaches beyond its target's: search_sz_t for the
 *          smoother, else the larger of the two radii (with or without a previous frame)
 *   reach  grid cells the groups that mark the processed mask reach: the temporal radius for the smoother and for a
 *          frame with a previous frame, else the spatial one, over step (src/nlkalman.c:637, :931)
 * Returns NLK_EINVAL and writes nothing when patch_sz < 2 or the image is smaller than a patch. */
struct nlk_frame_grid { int psz, step, ngx, ngy, halo, reach; };
int nlk_frame_grid(int w, int h, const struct nlkalman_params *prms, int smoother, int have_prev,
                   struct nlk_frame_grid *out);
/* The grid rows of an h-row frame cut into `world` strips: plan[r] = grid rows [gy0, gy1), the pixel rows [Y0, Y1) the
 * strip holds (its targets' patches and the halo around them) and the pixel rows [own0, own1) it owns (normalises and
 * returns). NLK_STRIPS_FEW_ROWS (nothing written): fewer grid rows than strips; NLK_STRIPS_THIN: a strip would spill
 * beyond its direct neighbour's own rows, i.e. the strips are thinner than the halo. */
struct nlk_strip_plan { int gy0, gy1, Y0, Y1, own0, own1; };
enum { NLK_STRIPS_FEW_ROWS = 1, NLK_STRIPS_THIN = 2 };
int nlk_strip_plan(int h, const struct nlk_frame_grid *grid, int world, struct nlk_strip_plan *plan);

/* ---- One frame over several GPUs, driven from C (csrc/strips.hip; the reference's analogue is
 * the static row split of its OpenMP loop, src/nlkalman.c:586). The patch-grid rows are cut into `world` strips.
 * Per step and strip: the previous frame's halo rows come from the neighbours, the strip is matched (its interior
 * while the halo travels), every strip's 64-bit mark words go to every strip, the raster-order mask is replayed
 * over the WHOLE grid (so the output is the serial order's for any number of strips), the strip's groups are
 * filtered, the accumulator rows written outside the own rows go to their owner, the own rows are normalised.
 * Transports: RCCL over xGMI with one strip per process (grouped ncclSend / ncclRecv between neighbours, the mark
 * words as one group of ncclBroadcast; librccl is dlopen'ed - the copy the process already holds, if any), or
 * device copies with every strip in one process (`devices` may repeat an index: the whole decomposition on one
 * GPU). A step only enqueues work; nlk_strips_sync waits for it. */
typedef struct nlk_strips nlk_strips;
/* `nlocal` strips of this process = ranks rank0 .. rank0 + nlocal - 1 of `world` (nlocal == 1, or == world),
 * strip i on HIP device devices[i]. have_prev = 0: first-frame calls (no previous frame, nothing to exchange). */
int nlk_strips_create(nlk_strips **out, int nlocal, const int *devices, int rank0, int world, int w, int h,
                      int ch, float sigma, const struct nlkalman_params *prms, int smoother, int have_prev);
void nlk_strips_destroy(nlk_strips *s);
const char *nlk_strips_last_error(const nlk_strips *s);
/* one strip per process: a 128-byte communicator id made on one rank (carried to the others by whatever
 * started them), then the communicator of the world on every rank */
int nlk_rccl_unique_id(void *id128);
int nlk_strips_rccl_init(nlk_strips *s, const void *id128);
const char *nlk_strips_transport(const nlk_strips *s);
/* rows of full device-resident HWC frames (on that strip's device) into local strip `local`: cur with its halo,
 * prev with its OWN rows only (may be NULL) */
int nlk_strips_load(nlk_strips *s, int local, const float *cur_full, const float *prev_full);
/* overlap: match the interior rows while the halo travels (default 0: the two extra rounds of matching launches
 * cost more than the exchange they hide at 1080p); timing: per-phase device times, one
 * synchronisation per step (diagnosis); graph: capture the step into a HIP graph once and replay it (one strip
 * per process; falls back to plain launches by itself if the capture is refused) */
int nlk_strips_set_options(nlk_strips *s, int overlap, int timing, int graph);
/* a model, not a result: one rank of a larger world stepped ALONE with every exchange skipped (the output means
 * nothing) - what its kernels and launch gaps cost at that world size on a box with one GPU */
int nlk_strips_set_dry_run(nlk_strips *s, int on);
int nlk_strips_step(nlk_strips *s);
int nlk_strips_sync(nlk_strips *s);
/* own rows [*y0, *y1) of the output of local strip `local` (device pointer, valid until the next step); the
 * whole-grid mark words, and the decisions it used: one byte per target of the grid rows from 0 down to the strip's
 * own last row (a strip needs no later ones: the whole grid for the last strip; the rows after them are not
 * defined). Any pointer may be NULL. Call after nlk_strips_sync. */
int nlk_strips_own_rows(nlk_strips *s, int local, int *y0, int *y1, float **rows, void **marks_full,
                        unsigned char **active_full);
nlk_ctx *nlk_strips_ctx(nlk_strips *s, int local);
/* gy0, gy1 (patch-grid rows), Y0, Y1 (pixel rows held), own0, own1 (pixel rows owned) of a local strip */
int nlk_strips_geometry(nlk_strips *s, int local, int geom[6]);
/* phase_ms[7]: mean device time of [previous-frame halo, matching, mark words, mask replay, groups, accumulator
 * halos, normalisation] on local strip 0 over the steps made with timing on; *issue_us: mean host time a step
 * took to enqueue since the last call; *graph: the steps are replayed from a captured graph */
int nlk_strips_stats(nlk_strips *s, float phase_ms[7], float *issue_us, int *graph);

/* the host-side tables a frame call uploads (tests only; no device needed): the orthonormal
 * DCT-II basis [psz][psz] that stands for FFTW REDFT10/REDFT01 x the reference's scaling
 * (src/nlkalman.c:204-220, 281-298, 335-353), the aggregation window (:365-419), and the 12 x 12 matrix the
 * 12-point flow graph of the packed-lane kernel applies (csrc/k_dct12.h, evaluated on the host: column j =
 * graph(e_j)). Any pointer may be NULL. */
int nlk_host_tables(int psz, float *basis, float *window, float *basis12_regs);
/* the byte code of the packed candidate / member lists (csrc/nlk_common.h), on the host through the very functions
 * the kernels call (tests only; no device needed): an entry at displacement (dx, dy) from a target at (px, py) that
 * searched radius r and kept k candidates (passthrough: the smoother's target without a valid previous patch).
 * *byte = its code as the matcher stores it, back[0..1] = the frame coordinate (x, y) the group kernel decodes from
 * that byte; either may be NULL. NLK_EINVAL where the target cannot have a valid record (more than 32 candidates, r
 * above 7, pass-through) or the displacement lies outside the radius. */
int nlk_host_packed_entry(int px, int py, int dx, int dy, int r, int k, int passthrough, unsigned int *byte, int *back);
/* The launch plan of a frame call's block matching (csrc/tu_match.hip: nlk_match_plan), through the geometry code and
 * the planner the frame calls run (tests only; no context, no device). w x h x ch, the parameters, smoother and
 * have_prev as a frame call takes them; rows = target rows of the call (a strip, a band), 0 = the whole grid. The
 * NLK_* switches are read from the environment at the call. out[]:
 *    0 generic   the generic kernel runs instead of the tiled ones (the fields below are then not used by a launch)
 *    1 wide      a second launch takes the queued targets that search the wider spatial window
 *    2.. the dominant tile: 2 tgx, 3 tgy (targets per tile), 4 bx (targets per block along x), 5 threads per
 *        workgroup, 6 block (blocks share their squared differences), 7 order (1 = block-summed), 8 halo, 9 rwp (LDS
 *        row stride, floats), 10 rh_max (LDS rows), 11 ksel_max (list capacity), 12 ntx (tiles along x),
 *        13 rounds class (2, 7 or 16 rounds of 64 candidates: the kernel instantiation), 14 dynamic LDS bytes
 *   15.. the wide tile (all 0 without one): 15 halo, 16 rwp, 17 rh_max, 18 rounds class, 19 dynamic LDS bytes
 * Returns what the frame call returns for inputs it refuses (NLK_EUNSUP: patch size; NLK_EINVAL: image smaller than a
 * patch, rows outside the grid, negative radii) and then writes nothing. */
#define NLK_MATCH_PLAN_FIELDS 20
int nlk_host_match_plan(int w, int h, int ch, const struct nlkalman_params *prms, int smoother, int have_prev, int rows,
                        int out[NLK_MATCH_PLAN_FIELDS]);
/* The plan of every pyramid level of a TV-L1 flow call (csrc/tu_tvl1.hip: nlk_tv_plan), through the parameter check and
 * the scratch layout walk nlk_dev_tvl1_flow runs (tests only; no context, no device). The NLK_TV_* switches are read from
 * the environment at the call. out[] receives one row of NLK_TVL1_PLAN_FIELDS ints per level, finest first, and
 * *nlevels their number (prms->nscales); max_levels = the rows out[] has room for. A row:
 *    0 nx, 1 ny   the level's size
 *    2 solved     the level is at or above prms->fscale (finer levels only receive the upsampled flow; their rows show
 *                 the plan they would get)
 *    3 driver     0 one workgroup solves the level, 1 the blocked driver, 2 the plain recursion (NLK_TV_UNBLOCKED)
 *    4 threads    of the one workgroup, or of a blocked batch's workgroups
 *    5 shape, 6 tw, 7 th   blocked: the tile shape's number (0, 1, 2 or 4), tile width and height
 *    8 gx, 9 gy   the grid: of the blocked batches, or of the plain recursion's 64 x 4 pixel workgroups
 *   10 inline     blocked: a batch judges its predecessor's stop test itself (0: a k_tv_decide launch between batches)
 *   11 look       blocked: batches between two looks at the solver state
 * A field that does not apply to the level's driver is 0. Returns what nlk_dev_tvl1_flow returns, with its messages, for
 * sizes and parameters it refuses, NLK_EINVAL for a NULL pointer or max_levels below the level count, and then writes
 * nothing. */
#define NLK_TVL1_PLAN_FIELDS 12
int nlk_host_tvl1_plan(int w, int h, const struct nlk_tvl1_params *prms, int max_levels, int *out, int *nlevels);
/* how many targets of the context's last match phase carry a valid packed record (tests only; synchronises) */
int nlk_ctx_count_packed(nlk_ctx *ctx, int *count);

#ifdef __cplusplus
}
#endif
#endif /* NLK_HIP_H */
