/* main_seq.c — `nlkalman-seq`: the whole recursion of scripts/nlkalman-seq.sh in ONE process
 * with the frames resident on the GPU. Same positional arguments and the
 * same files in the output folder as the script:
 *
 *   nlkalman-seq SEQ FFR LFR SIG OUT [STP [FPM [SPM [OPM]]]]
 *     SEQ   printf pattern of the noisy frames (e.g. in/%03d.tif)      (script: $1)
 *     FFR, LFR, STP  first / last frame, frame step (default 1)         ($2, $3, $6)
 *     SIG   noise standard deviation, or "auto": measured on the first frame as the filter
 *           sees it (nlk_dev_estimate_sigma) and printed as "sigma %.9g" on stdout before
 *           that frame is filtered; the run is the one that number would have given  ($4)
 *           (every form is read by seq_sig_parse and resolved on the first frame by seq_sig_resolve, host/seq_step.h:
 *           nlkalman-y4m reads its SIG through the same two)
 *           "vst" or "vst:A,B": signal-dependent noise var = a y + b. With "vst" the pair of every channel is
 *           measured on the first frame as pushed (nlk_dev_estimate_noise_curve), with "vst:A,B" every channel
 *           uses the given pair. One line "vst a_0 b_0 ... sigma S" (S = nlk_vst_scale, each value "%.9g") goes to
 *           stdout before the first frame is filtered. Every noisy frame is transformed on the device
 *           (nlk_dev_vst_forward) before anything else sees it, the whole recursion, flows included, runs on
 *           transformed frames at sigma = S with the defaults of S, and every flt1 / flt2 / smo1 frame is
 *           transformed back (nlk_dev_vst_inverse, mode 1) after opp2rgb, before it is downloaded. The gt tool
 *           refuses these forms.
 *           "nlf": a noise-level function of any shape (gamma-encoded video, where var = a y + b does not hold). The
 *           bins of the first frame's noise curve become a monotone piecewise-linear transform per channel
 *           (nlk_nlf_build); one line "nlf kept K_0 ... sigma S" (K_c: the bins channel c kept, S the table's scale)
 *           goes to stdout, and the run is vst's with nlk_dev_nlf_forward / nlk_dev_nlf_inverse in the transform's
 *           places. The gt tool takes it as it takes "auto": every OUT/%03d.tif must exist.
 *     OUT   output folder: flt1-%03d.tif flt2-%03d.tif bflo1-%03d.flo bocc1-%03d.png and,
 *           unless SPM is "no", fflo-%03d.flo focc-%03d.png smo1-%03d.tif  ($5)
 *     FPM   extra nlkalman-flt options (--f1_p ... --f2_l ..., one string)  ($7)
 *     SPM   extra nlkalman-smo options (--s1_p ...), or "no": no smoothing  ($8)
 *     OPM   "FSCALE1 DW1 TH1 FSCALE2 DW2 TH2": finest flow scale, flow data weight (lambda)
 *           and occlusion threshold of the forward / backward pass
 *           (default "1 0.25 0.75 1 0.25 0.75", script line 11)
 *   --of tvl1|bm  in front of everything else, in all three tools (the scripts have no such thing): the flow estimator
 *           of the run. tvl1 (default): the scripts' TV-L1. bm: block matching (nlk_dev_bm_flow) wherever
 *           a flow is computed - the forward step, the backward pass, the lag-1 smoother's own flow; OPM's FSCALE and TH
 *           apply, DW is ignored. The .flo and mask files hold the flow that was used.
 *   --despike K[,R]  after --of, in front of --sure, in all three tools (the scripts have no such thing): stuck, hot and dead
 *           pixels and single-sample impulses are taken out of every noisy frame before the filter sees it
 *           (nlk_dev_despike): a sample more than K sigma outside the range of its ring (radius R = 1, the
 *           default, or 2: 2 x 2 blobs) becomes the ring's median. Under SIG = vst | nlf it runs on the transformed frame,
 *           at the run's sigma; the first frame's measurement (auto, vst, nlf) stays on the frame as read. K = 4 is the
 *           value DESIGN.md §9's table was made with. The gt tool's noisy files and measures are not touched by it.
 *           Without the option nothing of this happens: the same launches and allocations as before.
 *   --defect-map K[,R[,N]]  after --despike, in front of --sure, in all three tools (the scripts have no such thing): a
 *           defect map learned over time (nlk_dev_defect_step). A sensor defect sits at the same place in
 *           every frame, scene and noise do not: where the running mean of the noisy frames 0 .. t - 1 (window N, default
 *           32; no motion compensation) lies more than K sigma / sqrt(min(t, N)) outside the range of its ring (radius
 *           R = 1, the default, or 2), frame t's sample becomes the median of its own ring before the filter sees it.
 *           Streaming: the first frame passes as it is, the sites --despike cannot see at a high sigma are flagged a
 *           few frames later. It runs where --despike runs and in front of it when both are given. K = 4 is the value
 *           DESIGN.md §9's table was made with; a static one-pixel detail is indistinguishable from a defect (the
 *           table's static row). Without the option nothing of this happens: the same launches and allocations as before.
 *   --sure  after --defect-map, in front of the rest, in all three tools (the scripts have no such thing): the error of every
 *           flt1 / flt2 frame is estimated without clean frames by Monte-Carlo SURE (seq_sure_step, host/seq_step.h;
 *           DESIGN.md §9): one more FLT1 and FLT2 per frame, on the noisy frame plus a probe of +-eps. OUT/measures-sure
 *           gets, per pass, "F1 I MSE_hat PSNR_hat R/N div" for every frame I and "F1 total ..." (finish_sure), each
 *           value "%.9g", PSNR at 255; the gt tool adds a last stdout line "sure T_F1 T_F2". Under SIG = vst | nlf the
 *           estimate is in the stabilised domain, at the run's sigma. The smoother's outputs are not estimated.
 *           NLK_SURE_EPS (eps / sigma, default 0.05) and NLK_SURE_SEED override the probe. Without the flag nothing of
 *           this happens: the same launches, allocations, files and stdout as before.
 *
 * What the script does with four processes and ~10 image files per frame (reference:
 * scripts/nlkalman-seq.sh:30-150) happens here through the device C-ABI: per frame
 * tvl1flow(noisy_t -> flt2_{t-1}) -> occlusion mask -> warp + FLT1 -> warp + FLT2, then
 * backwards tvl1flow(flt2_t -> smo1_{t+1}) -> mask -> warp + SMO1: seq_forward_step, then seq_lag1_step against
 * smo1_{t+1} in its TV-L1 mode, on one struct seq_run (host/seq_step.h): the options below (read by seq_opts_read,
 * which nlkalman-y4m calls too), SIG, FPM / SPM / OPM, the work images and the state of --defect-map and --sure; the
 * steps take it and the frame's pointers. Frames stay in the
 * opponent colour space between steps (the script's processes convert to RGB files and back:
 * a 1e-5 rounding on the 0..255 scale is the only numerical difference). Unlike the script,
 * flows and masks are always recomputed (it reuses files left by a previous run).
 *
 * File I/O runs beside the GPU: the output files (float TIFF / .flo / PNG encoding is most of a
 * frame's wall time) are written by a pool of threads from copies of the downloaded arrays, and
 * the next input frame is decoded while the current one is filtered. NLK_SEQ_IO_THREADS sets
 * the pool size (default 6; 0 = write in line).
 *
 * Built with NLK_SEQ_GT=1 the same source is `nlkalman-seq-gt`, the ground-truth loop of
 * scripts/nlkalman-seq-gt.sh in one process:
 *
 *   nlkalman-seq-gt [--ssim] SEQ FFR LFR SIG OUT [FPM [SPM [OPM]]]
 *     SEQ   printf pattern of the CLEAN frames; frame step 1; OPM defaults to
 *           "1 0.40 0.75 1 0.40 0.75" (the gt script's own arguments and default)
 *     --ssim  (the script has no such thing) every output is also measured by nlk_dev_ssim, on the same two device
 *           images as the squared error: OUT/measures-ssim gets, per pass, "F1 - Frame SSIM  v v ..." (the mean over
 *           the channels of every frame) and "F1 - Total SSIM v" (their mean in double in frame order), each value
 *           "%.9f", and stdout a second line "ssim T_F1 T_F2[ T_S1]". Frames must be at least 11 x 11 with at most
 *           16 channels. Without the flag nothing of this happens: the same launches, files and stdout as before.
 *
 * Each clean frame is uploaded, made noisy on the GPU (nlk_dev_awgn, seed SRAND + frame number, SRAND
 * read from the environment as imscript's tools read it, default 0: the script's `SRAND=$RANDOM` is
 * not reproducible) and written as OUT/%03d.tif - or, when that file already exists, the file is read
 * and used (script lines 30-39). The recursion is nlkalman-seq's on the device noisy frame. Each RGB
 * output is measured against the resident clean frame (nlk_dev_sqdiff_sum into one device array,
 * downloaded at the end) and written as 8-bit flt1- / flt2- / smo1-%03d.png, the script's final
 * state; OUT/measures gets the script's lines with its plambda arithmetic (write_measures), and stdout
 * one line, the total MSEs as `printf "%f %f %f\n"`. With SIG = auto the noise level is measured on the first
 * NOISY frame, and there is no sigma to make noise with: every OUT/%03d.tif must exist then.
 *
 * Built with NLK_SEQ_LSMO=1 the same source is `nlkalman-lsmo-seq`, scripts/nlkalman-lsmo-seq.sh in one process: the
 * forward recursion with a smoother of lag 1 in place of the backward pass.
 *
 *   nlkalman-lsmo-seq [--flow tvl1|inv] SEQ FFR LFR SIG OUT [FPM [SPM [OPM]]]
 *     the script's arguments (no STP), SIG as above. As soon as frame i is filtered, frame i - 1 is smoothed against
 *     flt2_i (seq_lag1_step, host/seq_step.h) and written as lsm1-%03d.tif; lsm1 of the last frame is its flt2. The
 *     files are the script's: flt1- flt2- lsm1-%03d.tif, bflo-%03d.flo bocc-%03d.png and fflo-%03d.flo focc-%03d.png,
 *     the last two under the number of the LATER frame. SPM = "no": no smoothing, no fflo / focc / lsm1.
 *     --flow tvl1 (default) the script's second TV-L1 flow flt2_{i-1} -> flt2_i per frame; --flow inv: the backward
 *     flow of frame i inverted (nlk_dev_flow_invert) in its place. Only the previous frame's outputs stay resident. */
#include <errno.h>
#include <math.h>
#include <pthread.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/stat.h>

#include "imgio.h"
#include "nlk_hip.h"
#include "nlkalman.h"
#include "seq_step.h"

#ifndef NLK_SEQ_GT
#define NLK_SEQ_GT 0
#endif
#ifndef NLK_SEQ_LSMO
#define NLK_SEQ_LSMO 0
#endif
#define PROG (NLK_SEQ_GT ? "nlkalman-seq-gt" : NLK_SEQ_LSMO ? "nlkalman-lsmo-seq" : "nlkalman-seq")

nlk_ctx *nlkalman_hip_context(void); /* libnlkalman.so: the process-wide device context */

static nlk_ctx *C;
#define CHK(call)                                                    \
  do {                                                               \
    if ((call) != NLK_OK) {                                          \
      fprintf(stderr, "%s: %s\n", PROG, nlk_last_error(C));          \
      exit(1);                                                       \
    }                                                                \
  } while (0)

/* ---- write-behind: a bounded queue of (path, array) jobs served by worker threads. The arrays
 * are page-locked buffers of one frame each, recycled through a pool: downloads run at the
 * link's rate and nothing is allocated per file */
struct wjob { char *path; float *data; int w, h, ch; struct wjob *next; };
#define POOL_MAX 16
static struct { float *buf[POOL_MAX]; int n; size_t bytes; } P;  /* free buffers (under Q.mu) */
static struct {
  pthread_mutex_t mu;
  pthread_cond_t more, less;
  struct wjob *head, *tail;
  int pending, closed, failed, nthreads;
  pthread_t th[32];
} Q = {.mu = PTHREAD_MUTEX_INITIALIZER, .more = PTHREAD_COND_INITIALIZER, .less = PTHREAD_COND_INITIALIZER};
#define WQ_MAX_PENDING 12 /* arrays waiting or being written = pool size - 1 (25 MB each at 1080p RGB) */

static void *wq_worker(void *arg) {
  (void)arg;
  for (;;) {
    pthread_mutex_lock(&Q.mu);
    while (!Q.head && !Q.closed) pthread_cond_wait(&Q.more, &Q.mu);
    struct wjob *j = Q.head;
    if (!j) { pthread_mutex_unlock(&Q.mu); return NULL; }
    Q.head = j->next;
    if (!Q.head) Q.tail = NULL;
    pthread_mutex_unlock(&Q.mu);
    const int bad = img_write(j->path, j->data, j->w, j->h, j->ch);
    if (bad) fprintf(stderr, "nlkalman-seq: cannot write %s\n", j->path);
    float *data = j->data;
    free(j->path);
    free(j);
    pthread_mutex_lock(&Q.mu);
    P.buf[P.n++] = data;  /* back to the pool */
    Q.failed |= bad != 0;
    --Q.pending;
    pthread_cond_signal(&Q.less);
    pthread_mutex_unlock(&Q.mu);
  }
}

static void wq_start(void) {
  const char *e = getenv("NLK_SEQ_IO_THREADS");
  Q.nthreads = e ? atoi(e) : 6;
  if (Q.nthreads > 32) Q.nthreads = 32;
  for (int i = 0; i < Q.nthreads; ++i)
    if (pthread_create(&Q.th[i], NULL, wq_worker, NULL)) { Q.nthreads = i; break; }
}

/* a free frame buffer (waits for a writer to return one) */
static float *pool_get(size_t bytes) {
  if (bytes > P.bytes) { fprintf(stderr, "nlkalman-seq: internal: buffer of %zu bytes asked\n", bytes); exit(1); }
  pthread_mutex_lock(&Q.mu);
  while (P.n == 0) pthread_cond_wait(&Q.less, &Q.mu);
  float *b = P.buf[--P.n];
  pthread_mutex_unlock(&Q.mu);
  return b;
}

static void pool_init(size_t bytes) {
  P.bytes = bytes;
  const int want = Q.nthreads > 0 ? WQ_MAX_PENDING + 1 : 1;
  for (P.n = 0; P.n < want && P.n < POOL_MAX; ++P.n) {
    void *h = NULL;
    CHK(nlk_host_alloc(C, &h, bytes));
    P.buf[P.n] = (float *)h;
  }
}

/* takes ownership of `path` (malloc'ed) and `data` (from the pool) */
static void wq_write(char *path, float *data, int w, int h, int ch) {
  if (Q.nthreads == 0) {
    if (img_write(path, data, w, h, ch)) { fprintf(stderr, "nlkalman-seq: cannot write %s\n", path); exit(1); }
    P.buf[P.n++] = data;
    free(path);
    return;
  }
  struct wjob *j = malloc(sizeof *j);
  j->path = path; j->data = data; j->w = w; j->h = h; j->ch = ch; j->next = NULL;
  pthread_mutex_lock(&Q.mu);
  if (Q.tail) Q.tail->next = j; else Q.head = j;
  Q.tail = j;
  ++Q.pending;
  pthread_cond_signal(&Q.more);
  pthread_mutex_unlock(&Q.mu);
}

/* waits for every file; returns nonzero if one could not be written */
static int wq_finish(void) {
  pthread_mutex_lock(&Q.mu);
  Q.closed = 1;
  pthread_cond_broadcast(&Q.more);
  pthread_mutex_unlock(&Q.mu);
  for (int i = 0; i < Q.nthreads; ++i) pthread_join(Q.th[i], NULL);
  return Q.failed;
}

/* ---- read-ahead: the next input frame is decoded by a helper thread */
static struct { pthread_t th; int active; char name[1024]; float *data; int w, h, ch; float *pinned; size_t pinned_bytes; } R;
static void *ra_worker(void *arg) {
  (void)arg;
  R.data = img_read(R.name, &R.w, &R.h, &R.ch);
  const size_t bytes = (size_t)R.w * R.h * R.ch * sizeof(float);
  if (R.data && R.pinned && bytes == R.pinned_bytes) {  /* stage it where the upload is fast */
    memcpy(R.pinned, R.data, bytes);
    free(R.data);
    R.data = R.pinned;
  }
  return NULL;
}
static void ra_start(const char *name) {
  snprintf(R.name, sizeof R.name, "%s", name);
  R.active = pthread_create(&R.th, NULL, ra_worker, NULL) == 0;
}
static float *ra_get(const char *name, int *w, int *h, int *ch) {
  if (R.active && strcmp(name, R.name) == 0) {
    pthread_join(R.th, NULL);
    R.active = 0;
    *w = R.w; *h = R.h; *ch = R.ch;
    return R.data;
  }
  return img_read(name, w, h, ch);
}

/* download a device array into a pool buffer and queue it for writing */
static void write_dev(char *path, const float *d, int w, int h, int ch) {
  const size_t bytes = (size_t)w * h * ch * sizeof(float);
  float *host = pool_get(bytes);
  CHK(nlk_d2h(C, host, d, bytes));
  wq_write(path, host, w, h, ch);
}

static float *dev_frame(size_t bytes) {
  void *d = NULL;
  CHK(nlk_dev_alloc(C, &d, bytes));
  return (float *)d;
}

static char *path_of(const char *dir, const char *pattern, int i) {
  char name[256], *full = malloc(strlen(dir) + 300);
  snprintf(name, sizeof name, pattern, i);
  sprintf(full, "%s/%s", dir, name);
  return full;
}

static struct seq_run RUN; /* the run: options, SIG, parameters, flow settings, work images (host/seq_step.h) */

/* RGB copy of an opponent-space device frame (seq_output_rgb) -> file (takes ownership of `path`); d_sum != NULL: its squared
 * error against d_clean goes to that device double first (the gt tool), d_ssim != NULL: its SSIM and those of its
 * channels to those 1 + ch device doubles (the gt tool with --ssim) */
static void write_frame(char *path, const float *d_opp, float *d_tmp, int w, int h, int ch, double *d_sum,
                        double *d_ssim, const float *d_clean) {
  CHK(seq_output_rgb(C, d_tmp, d_opp, w, h, ch, &RUN.sig));
  if (d_sum) CHK(nlk_dev_sqdiff_sum(C, d_sum, d_clean, d_tmp, (size_t)w * h * ch));
  if (d_ssim) CHK(nlk_dev_ssim(C, d_ssim, NULL, d_clean, d_tmp, w, h, ch, 255.f));
  write_dev(path, d_tmp, w, h, ch);
}

/* ---- the gt tool's measures */

/* SRAND as imscript's smapa.h reads it (sscanf "%lf", default 0), converted to the 32-bit seed as the
 * reference's x86-64 build converts it (host/main_awgn.c) */
static uint32_t srand_seed(void) {
  const char *sv = getenv("SRAND");
  double y;
  if (!sv || sscanf(sv, "%lf", &y) != 1) return 0;
  if (!(y > -9.2e18 && y < 9.2e18)) return 0;
  return (uint32_t)(int64_t)y;
}

/* `plambda -c` as the script runs it: every number of the program is read as a float (strtof), every operation
 * is done in double on floats and rounded to float, the result is printed "%.15lf" - and re-read from that text
 * by the next call */
static float pl_num(const char *s) { return strtof(s, NULL); }
static void pl_out(char *s, float v) { sprintf(s, "%.15lf", (double)v); }
static void pl_sqrt(char *out, const char *x) { pl_out(out, (float)sqrt((double)pl_num(x))); }
static void pl_psnr(char *out, const char *rmse) { /* "255 RMSE / log10 20 *" */
  const float q = (float)((double)255.f / (double)pl_num(rmse));
  pl_out(out, (float)((double)(float)log10((double)q) * 20.0));
}

/* OUT/measures (scripts/nlkalman-seq-gt.sh:44-138) from the per-frame squared-error sums [pass][frame] of n
 * samples; returns the total MSEs as printed (SS of each pass) in tot[pass] */
static int write_measures(const char *out, const double *sums, int npass, int nframes, size_t n, char (*tot)[64]) {
  static const char *label[3] = {"F1", "F2", "S1"};
  char *path = path_of(out, "measures", 0);
  FILE *f = fopen(path, "w");
  if (!f) { perror(path); free(path); return 1; }
  char m[64], rmse[64], psnr[64];
  char *mm = malloc((size_t)nframes * 64 + 1), *pp = malloc((size_t)nframes * 64 + 1);
  for (int p = 0; p < npass; ++p) {
    char ss[64] = "0";
    mm[0] = pp[0] = 0;
    for (int t = 0; t < nframes; ++t) {
      /* psnr.sh: MSE = imprintf "%v" (the mean, "%g"); the frame's RMSE and PSNR */
      snprintf(m, sizeof m, "%g", sums[(size_t)p * nframes + t] / (double)n);
      pl_sqrt(rmse, m);
      pl_psnr(psnr, rmse);
      sprintf(mm + strlen(mm), "%s%s", t ? " " : "", rmse);
      sprintf(pp + strlen(pp), "%s%s", t ? " " : "", psnr);
      /* SS = plambda -c "m n SS * + n+1 /" (the stack holds floats between the operations) */
      const float prod = (float)((double)(float)t * (double)pl_num(ss));
      const float sum = (float)((double)pl_num(m) + (double)prod);
      pl_out(ss, (float)((double)sum / (double)(float)(t + 1)));
    }
    pl_sqrt(rmse, ss);
    pl_psnr(psnr, rmse);
    /* echo "F1 - Frame RMSE " ${MM[*]}: the label, a space, the list */
    fprintf(f, "%s - Frame RMSE  %s\n%s - Frame PSNR  %s\n", label[p], mm, label[p], pp);
    fprintf(f, "%s - Total RMSE %s\n%s - Total PSNR %s\n", label[p], rmse, label[p], psnr);
    snprintf(tot[p], 64, "%s", ss);
  }
  free(mm);
  free(pp);
  const int bad = fclose(f) != 0;
  if (bad) perror(path);
  free(path);
  return bad;
}

/* OUT/measures-ssim from the values [pass][frame][1 + ch] of nlk_dev_ssim: per pass the frames' SSIM (the mean over
 * the channels) and their mean, in double in frame order; the totals also go to tot[pass] */
static int write_ssim(const char *out, const double *v, int npass, int nframes, int ch, double *tot) {
  static const char *label[3] = {"F1", "F2", "S1"};
  char *path = path_of(out, "measures-ssim", 0);
  FILE *f = fopen(path, "w");
  if (!f) { perror(path); free(path); return 1; }
  for (int p = 0; p < npass; ++p) {
    double sum = 0.0;
    fprintf(f, "%s - Frame SSIM ", label[p]);
    for (int t = 0; t < nframes; ++t) {
      const double s = v[((size_t)p * nframes + t) * (1 + ch)];
      fprintf(f, " %.9f", s);
      sum += s;
    }
    tot[p] = sum / (double)nframes;
    fprintf(f, "\n%s - Total SSIM %.9f\n", label[p], tot[p]);
  }
  const int bad = fclose(f) != 0;
  if (bad) perror(path);
  free(path);
  return bad;
}

/* gt: every file written, then OUT/measures and the one stdout line (the script's `printf "%f %f %f\n"` of the
 * total MSEs as plambda printed them; bash's printf reads them as long doubles); with --ssim (d_ssims != NULL) also
 * OUT/measures-ssim and a second line, "ssim" and the total of every pass */
static int finish_gt(const char *out, const double *d_sums, const double *d_ssims, int npass, int nframes, int ch,
                     size_t n) {
  double *sums = malloc(sizeof(double) * 3 * nframes);
  CHK(nlk_d2h(C, sums, d_sums, sizeof(double) * 3 * nframes));
  double *ssims = NULL, stot[3];
  if (d_ssims) {
    ssims = malloc(sizeof(double) * 3 * nframes * (1 + ch));
    CHK(nlk_d2h(C, ssims, d_ssims, sizeof(double) * 3 * nframes * (1 + ch)));
  }
  int bad = wq_finish();
  char tot[3][64];
  bad |= write_measures(out, sums, npass, nframes, n, tot);
  if (ssims) bad |= write_ssim(out, ssims, npass, nframes, ch, stot);
  free(sums);
  free(ssims);
  if (bad) return 1;
  for (int p = 0; p < npass; ++p) printf(p ? " %Lf" : "%Lf", strtold(tot[p], NULL));
  printf("\n");
  if (d_ssims) {
    printf("ssim");
    for (int p = 0; p < npass; ++p) printf(" %.9f", stot[p]);
    printf("\n");
  }
  return 0;
}

/* ---- --sure: the error estimate of every forward step without clean frames (seq_sure_step, host/seq_step.h) */
static struct {
  double *d_terms; /* [frame][pass: flt1, flt2][ch][2] device doubles, downloaded once at the end */
  int nframes, ffr, stp;
} S;

/* OUT/measures-sure, every value "%.9g": per pass "F1 I MSE_hat PSNR_hat R/N div" for every frame I, then
 * "F1 total ..." = the means of MSE_hat, R/N and div over the frames and the PSNR of that mean MSE_hat (at 255); the gt
 * tool adds a last stdout line "sure T_F1 T_F2", the two mean MSE_hat. rc: what the run returns without --sure */
static int finish_sure(const char *out, int rc) {
  if (!RUN.opts.sure || rc) return rc;
  static const char *label[2] = {"F1", "F2"};
  const size_t per = (size_t)4 * RUN.ch;
  double *terms = malloc(sizeof(double) * per * S.nframes), tot[2];
  CHK(nlk_d2h(C, terms, S.d_terms, sizeof(double) * per * S.nframes));
  char *path = path_of(out, "measures-sure", 0);
  FILE *f = fopen(path, "w");
  if (!f) { perror(path); free(path); return 1; }
  for (int p = 0; p < 2; ++p) {
    double m = 0.0, r = 0.0, d = 0.0;
    for (int t = 0; t < S.nframes; ++t) {
      const struct seq_sure_est e = seq_sure_estimate(terms + t * per + (size_t)p * 2 * RUN.ch, RUN.w, RUN.h, RUN.ch,
                                                      RUN.sig.sigma, RUN.sure.eps_rel);
      fprintf(f, "%s %d %.9g %.9g %.9g %.9g\n", label[p], S.ffr + t * S.stp, e.mse, e.psnr, e.resid, e.div);
      m += e.mse; r += e.resid; d += e.div;
    }
    tot[p] = m / S.nframes;
    fprintf(f, "%s total %.9g %.9g %.9g %.9g\n", label[p], tot[p], 10.0 * log10(255.0 * 255.0 / tot[p]), r / S.nframes,
            d / S.nframes);
  }
  free(terms);
  const int bad = fclose(f) != 0;
  if (bad) perror(path);
  free(path);
  if (!bad && NLK_SEQ_GT) printf("sure %.9g %.9g\n", tot[0], tot[1]);
  return bad;
}

int main(int argc, const char **argv) {
  const int gt = NLK_SEQ_GT, lsmo = NLK_SEQ_LSMO;
  int want_ssim = 0, lag1 = SEQ_LAG1_TVL1;
  /* the shared options, once each in the order of seq_opts_read's table (--of, --despike, --defect-map, --sure), then
   * the tool's own; one out of place is left for the usage text or the positional arguments */
  int at = 1;
  for (int from = 0, n; (n = seq_opts_read(&RUN.opts, argc, argv, at, &from, PROG)) != 0; at += n)
    if (n < 0) return 1;
  if (lsmo && at < argc && !strcmp(argv[at], "--flow")) { /* the positional arguments follow its value */
    if (at + 1 >= argc || !(lag1 = seq_lag1_mode(argv[at + 1]))) {
      fprintf(stderr, "%s: --flow %s: want tvl1 or inv\n", PROG, at + 1 >= argc ? "" : argv[at + 1]);
      return 1;
    }
    at += 2;
  }
  if (gt && at < argc && !strcmp(argv[at], "--ssim")) { /* the positional arguments follow it */
    want_ssim = 1;
    ++at;
  }
  argv[at - 1] = argv[0]; /* argv[1 ..]: the positional arguments */
  argv += at - 1;
  argc -= at - 1;
  if (argc < 6) {
    fprintf(stderr, "usage: %s [--of tvl1|bm] [--sure] %s\n"
                    "  one-process equivalent of scripts/%s.sh (see the header of main_seq.c)\n"
                    "  --despike K[,R] (after --of, in front of --sure): a sample more than K sigma outside its ring's range (radius\n"
                    "  R = 1 | 2) becomes the ring's median before the filter sees the frame: stuck, hot and dead pixels (K = 4: the\n"
                    "  value of DESIGN.md's table)\n"
                    "  --defect-map K[,R[,N]] (after --despike, in front of --sure): a defect map learned over time: where the mean\n"
                    "  of the noisy frames before (window N = 2 .. 4096, default 32) lies more than K sigma / sqrt(frames) outside\n"
                    "  its ring's range, the frame's sample becomes its ring's median (K = 4: the value of DESIGN.md's table)\n"
                    "  --sure: OUT/measures-sure gets the Monte-Carlo SURE estimate of every flt1 / flt2 frame's error, made without\n"
                    "  clean frames (under SIG = vst | nlf: in the stabilised domain, at the run's sigma)\n", argv[0],
            gt ? "[--ssim] SEQ FFR LFR SIG OUT [FPM [SPM [OPM]]]"
            : lsmo ? "[--flow tvl1|inv] SEQ FFR LFR SIG OUT [FPM [SPM [OPM]]]" : "SEQ FFR LFR SIG OUT [STP [FPM [SPM [OPM]]]]",
            PROG);
    return 1;
  }
  const char *seq = argv[1], *out = argv[5];
  const int ffr = atoi(argv[2]), lfr = atoi(argv[3]);
  const int sig_bad = seq_sig_parse(argv[4], &RUN.sig);
  const int vst = seq_sig_vst(&RUN.sig) != NULL, auto_sigma = RUN.sig.mode != SEQ_SIG_NUMBER;
  if (vst && gt) {
    fprintf(stderr, "%s: SIG = vst is not supported by the ground-truth loop\n", PROG);
    return 1;
  }
  if (sig_bad) {
    fprintf(stderr, SEQ_SIG_WANT, PROG, argv[4]);
    return 1;
  }
  /* the gt and lsmo scripts have no STP: their FPM SPM OPM are $6 $7 $8 */
  const int a0 = gt || lsmo ? 6 : 7;
  const int stp = a0 == 7 && argc > 6 && atoi(argv[6]) > 0 ? atoi(argv[6]) : 1;
  const char *fpm = argc > a0 ? argv[a0] : "", *spm = argc > a0 + 1 ? argv[a0 + 1] : "";
  const char *opm = argc > a0 + 2 && argv[a0 + 2][0] ? argv[a0 + 2]
                    : gt ? "1 0.40 0.75 1 0.40 0.75" : "1 0.25 0.75 1 0.25 0.75";
  if (seq_parse_opm(opm, &RUN.bwd, &RUN.fwd, 0)) {
    fprintf(stderr, "%s: OPM must hold 6 numbers: FSCALE1 DW1 TH1 FSCALE2 DW2 TH2\n", PROG);
    return 1;
  }
  const int smoothing = strcmp(spm, "no") != 0;

  /* filter / smoother parameters: the options of nlkalman-flt and nlkalman-smo, same grammar */
  int verbose = 0;
  if (seq_run_params(&RUN, "nlkalman-seq (FPM)", fpm, "nlkalman-seq (SPM)", smoothing ? spm : NULL, &verbose)) {
    fprintf(stderr, "nlkalman-seq: both filtering iterations are needed (f1_p, f2_p != 0)\n");
    return 1;
  }

  /* every input frame must exist (script lines 19-28) */
  int nframes = 0;
  for (int i = ffr; i <= lfr; i += stp, ++nframes) {
    char name[1024];
    snprintf(name, sizeof name, seq, i);
    FILE *f = fopen(name, "rb");
    if (!f) { printf("ERROR: %s not found\n", name); return 1; }
    fclose(f);
  }
  if (nframes < 1) { fprintf(stderr, "nlkalman-seq: empty frame range\n"); return 1; }
  if (mkdir(out, 0777) && errno != EEXIST) { perror(out); return 1; }

  C = nlkalman_hip_context();
  wq_start();
  int w = 0, h = 0, ch = 0;
  size_t bytes = 0;
  const struct seq_work *const W = &RUN.work;
  float *d_rgb = NULL, *flt1 = NULL;
  float *d_lsm1 = NULL; /* lsmo: the smoothed frame (its flow and mask are W->d_fflow, W->d_focc) */
  float **flt2 = calloc(nframes, sizeof(float *));  /* kept for the backward pass */
  /* gt: the clean frames (all of them kept for the smoother's measures, else one buffer), the squared-error
   * sums [pass][frame] (flt1, flt2, smo1) and the output names */
  float **clean = calloc(nframes, sizeof(float *));
  double *d_sums = NULL, *d_ssims = NULL; /* (d_ssims: [pass][frame][1 + ch], with --ssim only) */
  const uint32_t seed0 = gt ? srand_seed() : 0;
  const char *ext = gt ? "png" : "tif";
  char pat[64];
#define OUTNAME(kind) (snprintf(pat, sizeof pat, "%s-%%03d.%s", kind, ext), pat)
#define SUM(pass, t) (gt ? d_sums + (size_t)(pass) * nframes + (t) : NULL)
#define SSIM(pass, t) (d_ssims ? d_ssims + ((size_t)(pass) * nframes + (t)) * (1 + ch) : NULL)
  if (gt) {
    void *d = NULL;
    CHK(nlk_dev_alloc(C, &d, sizeof(double) * 3 * nframes));
    d_sums = (double *)d;
  }

  /* ---- forward pass (script lines 30-115) */
  int t = 0;
  for (int i = ffr; i <= lfr; i += stp, ++t) {
    char name[1024];
    snprintf(name, sizeof name, seq, i);
    int w1, h1, c1;
    float *fr = ra_get(name, &w1, &h1, &c1);
    if (!fr) return 1;
    if (t == 0) {
      w = w1; h = h1; ch = c1;
      bytes = (size_t)w * h * ch * sizeof(float);
      if (want_ssim) {
        if (w < 11 || h < 11 || ch > 16) {
          fprintf(stderr, "%s: --ssim needs frames of at least 11 x 11 with at most 16 channels, %s is %dx%dx%d\n", PROG,
                  name, w, h, ch);
          return 1;
        }
        void *d = NULL;
        CHK(nlk_dev_alloc(C, &d, sizeof(double) * 3 * nframes * (1 + ch)));
        d_ssims = (double *)d;
      }
      d_rgb = dev_frame(bytes);
      CHK(seq_run_open(&RUN, C, w, h, ch, lsmo && smoothing));
      if (lsmo && smoothing) d_lsm1 = dev_frame(bytes);
      if (RUN.opts.sure) {
        void *d = NULL;
        CHK(nlk_dev_alloc(C, &d, sizeof(double) * 4 * ch * nframes));
        S.d_terms = (double *)d;
        S.nframes = nframes; S.ffr = ffr; S.stp = stp;
      }
      pool_init(bytes > (size_t)w * h * 8 ? bytes : (size_t)w * h * 8);
      if (Q.nthreads > 0) {
        void *hp = NULL;
        CHK(nlk_host_alloc(C, &hp, bytes));
        R.pinned = (float *)hp;
        R.pinned_bytes = bytes;
      }
    } else if (w1 != w || h1 != h || c1 != ch) {
      fprintf(stderr, "%s: %s: frame size differs from the first frame\n", PROG, name);
      return 1;
    }
    if (!gt) {
      CHK(nlk_h2d(C, d_rgb, fr, bytes));  /* (returns when the copy is done: the staging buffer is free again) */
    } else {
      /* the clean frame stays resident for the measures; the noisy one is OUT/%03d.tif if that exists (script
       * lines 30-39), else clean + noise, written there */
      clean[t] = smoothing || t == 0 ? dev_frame(bytes) : clean[0];
      CHK(nlk_h2d(C, clean[t], fr, bytes));
      char *npath = path_of(out, "%03d.tif", i);
      struct stat st;
      if (stat(npath, &st) == 0 && S_ISREG(st.st_mode)) {
        int w2, h2, c2;
        float *nz = img_read(npath, &w2, &h2, &c2);
        if (!nz) return 1;
        if (w2 != w || h2 != h || c2 != ch) {
          fprintf(stderr, "%s: %s is %dx%dx%d, the clean frame %dx%dx%d\n", PROG, npath, w2, h2, c2, w, h, ch);
          return 1;
        }
        CHK(nlk_h2d(C, d_rgb, nz, bytes));
        free(nz);
        free(npath);
      } else if (auto_sigma) {
        fprintf(stderr, "%s: SIG = %s needs the noisy frame %s (there is no sigma to make it with)\n", PROG, argv[4], npath);
        return 1;
      } else {
        CHK(nlk_dev_awgn(C, d_rgb, clean[t], (size_t)w * h * ch, RUN.sig.sigma, seed0 + (uint32_t)i));
        write_dev(npath, d_rgb, w, h, ch);
      }
    }
    if (fr != R.pinned) free(fr);
    if (i + stp <= lfr && Q.nthreads > 0) {  /* decode the next frame meanwhile */
      char next[1024];
      snprintf(next, sizeof next, seq, i + stp);
      ra_start(next);
    }
    if (t == 0) { /* sigma is known once the first frame is on the device, then every default that depends on it */
      const int rc = seq_run_first_frame(&RUN, d_rgb, stdout, PROG);
      if (rc == SEQ_SIG_REFUSED) return 1;
      CHK(rc);
    }
    float *n1 = dev_frame(bytes), *n2 = dev_frame(bytes);
    const struct seq_step step = {.d_rgb = d_rgb, .prev_flt1 = t ? flt1 : NULL, .prev_flt2 = t ? flt2[t - 1] : NULL,
                                  .flt1 = n1, .flt2 = n2};
    CHK(seq_forward_step(&RUN, &step));
    if (RUN.opts.sure) CHK(seq_sure_step(&RUN, &step, t, S.d_terms + (size_t)t * 4 * ch));
    if (t > 0) { /* the flow and its mask (script lines 57-73) */
      write_dev(path_of(out, lsmo ? "bflo-%03d.flo" : "bflo1-%03d.flo", i), W->d_flow, w, h, 2);
      write_dev(path_of(out, lsmo ? "bocc-%03d.png" : "bocc1-%03d.png", i), W->d_occ, w, h, 1);
    }
    write_frame(path_of(out, OUTNAME("flt1"), i), n1, W->d_tmp, w, h, ch, SUM(0, t), SSIM(0, t), clean[t]);
    write_frame(path_of(out, OUTNAME("flt2"), i), n2, W->d_tmp, w, h, ch, SUM(1, t), SSIM(1, t), clean[t]);
    if (lsmo && smoothing && t > 0) { /* smooth the previous frame (script lines 87-108) */
      const struct seq_lag1 lag = {.mode = lag1, .d_fflow = W->d_fflow, .d_focc = W->d_focc, .flt2 = flt2[t - 1],
                                   .next = n2, .smo1 = d_lsm1};
      CHK(seq_lag1_step(&RUN, &lag));
      write_dev(path_of(out, "fflo-%03d.flo", i), W->d_fflow, w, h, 2);
      write_dev(path_of(out, "focc-%03d.png", i), W->d_focc, w, h, 1);
      write_frame(path_of(out, "lsm1-%03d.tif", i - 1), d_lsm1, W->d_tmp, w, h, ch, NULL, NULL, NULL);
      if (verbose) printf("frame %d smoothed\n", i - 1);
    }
    if (flt1) nlk_dev_free(C, flt1);
    flt1 = n1;
    flt2[t] = n2;
    if ((!smoothing || lsmo) && t > 0) { nlk_dev_free(C, flt2[t - 1]); flt2[t - 1] = NULL; }
    if (verbose) printf("frame %d filtered\n", i);
  }
  if (lsmo) { /* the last frame's lsm1 is its flt2 (script lines 112-116) */
    if (smoothing) write_frame(path_of(out, "lsm1-%03d.tif", lfr), flt2[nframes - 1], W->d_tmp, w, h, ch, NULL, NULL, NULL);
    return finish_sure(out, wq_finish());
  }
  if (!smoothing) /* script line 113 */
    return finish_sure(out, gt ? finish_gt(out, d_sums, d_ssims, 2, nframes, ch, (size_t)w * h * ch) : wq_finish());

  /* ---- backward pass (script lines 117-150) */
  float **smo = calloc(nframes, sizeof(float *));
  smo[nframes - 1] = flt2[nframes - 1];
  write_frame(path_of(out, OUTNAME("smo1"), ffr + (nframes - 1) * stp), smo[nframes - 1], W->d_tmp, w, h, ch,
              SUM(2, nframes - 1), SSIM(2, nframes - 1), clean[nframes - 1]);
  for (t = nframes - 2; t >= 0; --t) {
    const int i = ffr + t * stp;
    smo[t] = dev_frame(bytes);
    const struct seq_lag1 back = {.mode = SEQ_LAG1_TVL1, .d_fflow = W->d_flow, .d_focc = W->d_occ, .flt2 = flt2[t],
                                  .next = smo[t + 1], .smo1 = smo[t]};
    CHK(seq_lag1_step(&RUN, &back));
    write_dev(path_of(out, "fflo-%03d.flo", i), W->d_flow, w, h, 2);
    write_dev(path_of(out, "focc-%03d.png", i), W->d_occ, w, h, 1);
    write_frame(path_of(out, OUTNAME("smo1"), i), smo[t], W->d_tmp, w, h, ch, SUM(2, t), SSIM(2, t), clean[t]);
    if (verbose) printf("frame %d smoothed\n", i);
  }
  return finish_sure(out, gt ? finish_gt(out, d_sums, d_ssims, 3, nframes, ch, (size_t)w * h * ch) : wq_finish());
}
