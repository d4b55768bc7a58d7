/* main_y4m.c — `nlkalman-y4m`: the forward recursion of nlkalman-seq on a YUV4MPEG2 stream, as decoders pipe it:
 *
 *   ffmpeg -i in.mkv -f yuv4mpegpipe -strict -1 - | nlkalman-y4m 20 | ffmpeg -i - out.mkv
 *
 *   nlkalman-y4m [options] SIG [IN [OUT]]      IN, OUT: a file or "-" (default: stdin, stdout)
 *     SIG            a number | auto | vst | vst:A,B | nlf (nlkalman-seq's forms and meaning, host/main_seq.c, read
 *                    and resolved by the same seq_sig_parse / seq_sig_resolve, host/seq_step.h)
 *     --matrix 601|709|auto    auto (default): 709 when W >= 1280 or H > 576, else 601
 *     --range limited|full|auto   auto (default): the header's XCOLORRANGE, else limited
 *     --fpm "..."    nlkalman-flt options, as nlkalman-seq's FPM
 *     --opm "FSCALE DW TH [FSCALE2 DW2 TH2]"   flow parameters of the backward flow (default "1 0.25 0.75") and of
 *                    the smoother's forward flow (default: the same three)
 *     --smooth tvl1|inv   the lag-1 smoother (default: none): the output is the lsm1 frames of nlkalman-lsmo-seq
 *                    (host/main_seq.c). Frame t - 1 is smoothed against flt2_t (seq_lag1_step, host/seq_step.h) and
 *                    written when frame t has been filtered; the last frame goes out as its flt2. tvl1: a second TV-L1
 *                    flow per frame, as the script; inv: the backward flow of frame t inverted (nlk_dev_flow_invert)
 *     --spm "..."    nlkalman-smo options (--s1_p ...), as nlkalman-seq's SPM
 *     (the next four are nlkalman-seq's, read by the same seq_opts_read into the run's seq_opts, host/seq_step.h; here
 *     in any place; a value it refuses ends the run where it stands on the command line)
 *     --of tvl1|bm   the flow estimator of the run, as nlkalman-seq's: tvl1 (default), or bm: block matching
 *                    (nlk_dev_bm_flow) for the backward flow and for --smooth tvl1's own flow; --opm's FSCALE and TH
 *                    apply, DW is ignored
 *     --despike K[,R]   defective pixels (stuck, hot, dead, single-sample impulses) are taken out of every frame before
 *                    the filter sees it, as nlkalman-seq's --despike (nlk_dev_despike at thr = K sigma, ring radius R = 1,
 *                    the default, or 2: the 2 x 2 blob a 4:2:0 chroma impulse becomes in RGB). K = 4 is the value
 *                    DESIGN.md §9's table was made with
 *     --defect-map K[,R[,N]]   a defect map learned over time, as nlkalman-seq's --defect-map (nlk_dev_defect_step): where
 *                    the running mean of the frames before (window N, default 32) lies more than K sigma / sqrt(frames)
 *                    outside its ring's range (radius R = 1 | 2), the frame's sample becomes its ring's median. Streaming:
 *                    frame t is cleaned with the evidence of the frames 0 .. t - 1; in front of --despike when both are given
 *     --sure         the error of every flt2 frame estimated without clean frames by Monte-Carlo SURE (seq_sure_step,
 *                    host/seq_step.h): one more FLT1 and FLT2 per frame. One stderr line per frame,
 *                    "sure T MSE_hat PSNR_hat R/N div" (T from 1, each value "%.9g", PSNR at 255), and at the end
 *                    "sure total ..." with the means over the frames; the output stream is what it is without the
 *                    option. Under SIG = vst | nlf the estimate is in the stabilised domain, at the run's sigma; with
 *                    --smooth it is still flt2's. NLK_SURE_EPS, NLK_SURE_SEED: as nlkalman-seq's.
 *     --frames N     stop after N frames
 *     --copy         convert to RGB and back only (no filter): the conversion path by itself
 *     --probe        no GPU, no output stream: parse IN, print one line
 *                    "W H FN:FD I A C depth range matrix frames" and exit (counts the frames, checks every payload)
 *     -v             one line per frame on stderr
 *
 * Per frame: payload -> pinned buffer -> nlk_h2d -> nlk_dev_yuv_to_rgb -> the forward step of nlkalman-seq
 * (host/seq_step.c) -> seq_output_rgb (nlk_dev_opp2rgb on a copy of flt2, the inverse transform under SIG = vst | nlf) ->
 * nlk_dev_rgb_to_yuv -> nlk_d2h -> the writer (emit, for every frame that goes out). The colour conversion runs on the GPU in both directions, so a 1080p
 * 4:2:0 8-bit frame crosses the link as 3.1 MB each way and the host encodes nothing. The output is the flt2 frames
 * (with --smooth: the lsm1 frames, one frame later; as many frames go out as came in, in order) in the input's
 * format under the input's header line. Only flt1 and flt2 of the previous frame stay resident: memory does not grow
 * with the stream. The whole-sequence smoother runs backwards and has no place here; --smooth is its lag-1 form.
 *
 * A reader thread and a writer thread work beside the GPU on a ring of pinned payload buffers: frame t + 1 is read
 * while frame t is filtered and frame t - 1 is written. The two copies across the link (nlk_h2d, nlk_d2h: 3 MB each,
 * ~0.1 ms) are synchronous on the main thread, so the GPU waits for them: a known limit. NLK_SEQ_IO_THREADS=0, or a ring that cannot be allocated,
 * gives in-line I/O on one pageable buffer.
 *
 * Every diagnostic goes to stderr (stdout may be the stream), the "sigma ...", "vst ..." and "nlf ..." lines of SIG = auto | vst | nlf
 * included. Exit status 0, or 1 on any error; a stream that ends inside a frame gives 1 after every complete frame
 * before it has been filtered and written (with --smooth the last of them as its flt2). */
#include <math.h>
#include <pthread.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "nlk_hip.h"
#include "nlkalman.h"
#include "seq_step.h"
#include "y4m.h"

#define PROG "nlkalman-y4m"

nlk_ctx *nlkalman_hip_context(void); /* libnlkalman.so: the process-wide device context */

static nlk_ctx *C;
#define CHK(call)                                             \
  do {                                                        \
    if ((call) != NLK_OK) {                                   \
      fprintf(stderr, "%s: %s\n", PROG, nlk_last_error(C));   \
      return 1;                                               \
    }                                                         \
  } while (0)

/* ---- the ring: slot i holds frame i, i + RING, ...; a slot goes FREE -> (reader) INPUT -> (main) OUTPUT -> (writer)
 * FREE, and every party walks the slots in order. INPUT_END / OUTPUT_END in place of a frame end the stream. */
#define RING 4
enum { FREE, INPUT, INPUT_END, OUTPUT, OUTPUT_END };
static struct {
  pthread_mutex_t mu;
  pthread_cond_t cv;
  int state[RING];
  void *buf[RING];
  int threads;         /* 0: in-line I/O on buf[0] */
  FILE *in, *out;
  const struct y4m_header *hd;
  long max_frames;     /* < 0: no limit */
  int read_failed, write_failed;
  char read_err[Y4M_ERR_MAX], write_err[Y4M_ERR_MAX];
} G = {.mu = PTHREAD_MUTEX_INITIALIZER, .cv = PTHREAD_COND_INITIALIZER, .max_frames = -1};

static void slot_wait(int i, int s1, int s2) {
  pthread_mutex_lock(&G.mu);
  while (G.state[i] != s1 && G.state[i] != s2) pthread_cond_wait(&G.cv, &G.mu);
  pthread_mutex_unlock(&G.mu);
}
static void slot_set(int i, int s) {
  pthread_mutex_lock(&G.mu);
  G.state[i] = s;
  pthread_cond_broadcast(&G.cv);
  pthread_mutex_unlock(&G.mu);
}

/* 1 = a frame in buf, 0 = the stream is over (G.read_failed says how) */
static int read_one(void *buf, long done) {
  if (G.max_frames >= 0 && done >= G.max_frames) return 0;
  const int r = y4m_read_frame(G.in, G.hd, buf, G.read_err);
  if (r < 0) G.read_failed = 1;
  return r == 1;
}
/* (the flag is the writer thread's to set and the main thread's to read: under the lock) */
static int write_has_failed(void) {
  pthread_mutex_lock(&G.mu);
  const int v = G.write_failed;
  pthread_mutex_unlock(&G.mu);
  return v;
}
static void write_one(const void *buf) {
  if (write_has_failed() || !y4m_write_frame(G.out, G.hd, buf, G.write_err)) return;
  pthread_mutex_lock(&G.mu);
  G.write_failed = 1;
  pthread_mutex_unlock(&G.mu);
}

static void *reader(void *arg) {
  (void)arg;
  for (long t = 0;; ++t) {
    const int i = (int)(t % RING);
    slot_wait(i, FREE, FREE);
    const int got = read_one(G.buf[i], t);
    slot_set(i, got ? INPUT : INPUT_END);
    if (!got) return NULL;
  }
}
static void *writer(void *arg) {
  (void)arg;
  for (long t = 0;; ++t) {
    const int i = (int)(t % RING);
    slot_wait(i, OUTPUT, OUTPUT_END);
    if (G.state[i] == OUTPUT_END) return NULL;
    write_one(G.buf[i]);
    slot_set(i, FREE);
  }
}

/* the next input frame: its buffer, or NULL at the end of the stream */
static void *frame_get(long t) {
  if (!G.threads) return read_one(G.buf[0], t) ? G.buf[0] : NULL;
  const int i = (int)(t % RING);
  slot_wait(i, INPUT, INPUT_END);
  return G.state[i] == INPUT ? G.buf[i] : NULL;
}
/* the buffer of frame t between frame_get and frame_put: once uploaded it is free to receive the output frame (with
 * --smooth the main thread holds two slots, those of frames t - 1 and t; the reader and the writer share the rest) */
static void *frame_buf(long t) { return G.buf[G.threads ? (int)(t % RING) : 0]; }
/* the same buffer, now holding the output frame */
static void frame_put(long t) {
  if (!G.threads) write_one(G.buf[0]);
  else slot_set((int)(t % RING), OUTPUT);
}

static int probe(FILE *in, const struct y4m_header *hd, const char *range, int matrix, long max_frames) {
  char err[Y4M_ERR_MAX];
  void *buf = malloc(hd->frame_bytes);
  if (!buf) { fprintf(stderr, "%s: out of memory (%zu bytes)\n", PROG, hd->frame_bytes); return 1; }
  long n = 0;
  int r = 0;
  while ((max_frames < 0 || n < max_frames) && (r = y4m_read_frame(in, hd, buf, err)) == 1) ++n;
  free(buf);
  if (r < 0) { fprintf(stderr, "%s: frame %ld: %s\n", PROG, n + 1, err); return 1; }
  printf("%d %d %d:%d %c %d:%d %s %d %s %d %ld\n", hd->w, hd->h, hd->fps_n, hd->fps_d, hd->interlace, hd->asp_n,
         hd->asp_d, hd->ctag[0] ? hd->ctag : "420jpeg", hd->fmt.depth, range, matrix, n);
  return 0;
}

/* an RGB frame, or (sig != NULL) an opponent-space frame as output (seq_output_rgb), -> codes -> buf */
static int emit(void *buf, const float *d_frame, float *d_tmp, void *d_yuv, const struct y4m_header *hd, int ch,
                const struct seq_sig *sig) {
  if (sig) CHK(seq_output_rgb(C, d_tmp, d_frame, hd->w, hd->h, ch, sig));
  CHK(nlk_dev_rgb_to_yuv(C, d_yuv, sig ? d_tmp : d_frame, hd->w, hd->h, &hd->fmt));
  CHK(nlk_d2h(C, buf, d_yuv, hd->frame_bytes));
  return 0;
}

static int usage(void) {
  fprintf(stderr,
          "usage: %s [options] SIG [IN [OUT]]     IN, OUT: a file or \"-\" (default: stdin, stdout)\n"
          "  SIG: a number | auto | vst | vst:A,B | nlf\n"
          "  --matrix 601|709|auto  --range limited|full|auto  --fpm \"...\"  --opm \"FSCALE DW TH [FSCALE2 DW2 TH2]\"\n"
          "  --smooth tvl1|inv  --spm \"...\"  --frames N  --copy  --probe  -v       (see the header of main_y4m.c)\n"
          "  --of tvl1|bm\n"
          "  --despike K[,R]  a sample more than K sigma outside its ring's range (radius R = 1 | 2) becomes the ring's median\n"
          "          before the filter sees the frame: stuck, hot and dead pixels (K = 4: the value of DESIGN.md's table)\n"
          "  --defect-map K[,R[,N]]  a defect map learned over time: where the mean of the frames before (window N = 2 .. 4096,\n"
          "          default 32) lies more than K sigma / sqrt(frames) outside its ring's range, the sample becomes its ring's median\n"
          "  --sure  one stderr line per frame, \"sure T MSE_hat PSNR_hat R/N div\": flt2's error estimated without clean\n"
          "          frames (Monte-Carlo SURE; under SIG = vst | nlf in the stabilised domain, at the run's sigma)\n", PROG);
  return 1;
}

int main(int argc, const char **argv) {
  const char *matrix_s = "auto", *range_s = "auto", *fpm = "", *opm = "1 0.25 0.75", *pos[3] = {NULL, NULL, NULL};
  const char *smooth_s = NULL, *spm = "";
  long max_frames = -1;
  int copy = 0, want_probe = 0, verbose = 0, npos = 0;
  static struct seq_run R; /* the run: options, SIG, parameters, flow settings, work images (host/seq_step.h) */
  for (int i = 1; i < argc; ++i) {
    const char *a = argv[i];
    const char **val = NULL;
    const int shared = seq_opts_arity(a); /* --of, --despike, --defect-map, --sure: nlkalman-seq's, here in any place */
    if (!strcmp(a, "--matrix")) val = &matrix_s;
    else if (!strcmp(a, "--range")) val = &range_s;
    else if (!strcmp(a, "--fpm")) val = &fpm;
    else if (!strcmp(a, "--opm")) val = &opm;
    else if (!strcmp(a, "--smooth")) val = &smooth_s;
    else if (!strcmp(a, "--spm")) val = &spm;
    if (val || shared) {
      if ((val || shared == 2) && i + 1 >= argc) { fprintf(stderr, "%s: %s needs a value\n", PROG, a); return 1; }
      if (val) *val = argv[++i];
      else if (seq_opts_read(&R.opts, argc, argv, i, NULL, PROG) < 0) return 1;
      else i += shared - 1;
    } else if (!strcmp(a, "--frames")) {
      char *e;
      if (++i >= argc || (max_frames = strtol(argv[i], &e, 10)) < 0 || *e || e == argv[i]) {
        fprintf(stderr, "%s: --frames needs a count >= 0\n", PROG);
        return 1;
      }
    } else if (!strcmp(a, "--copy")) copy = 1;
    else if (!strcmp(a, "--probe")) want_probe = 1;
    else if (!strcmp(a, "-v")) verbose = 1;
    else if (!strcmp(a, "-h") || !strcmp(a, "--help")) { usage(); return 0; }
    else if (a[0] == '-' && a[1] && !(npos == 0 && (a[1] == '.' || (a[1] >= '0' && a[1] <= '9')))) {
      fprintf(stderr, "%s: unknown option %s\n", PROG, a);
      return usage();
    } else if (npos < 3) pos[npos++] = a;
    else return usage();
  }
  if (npos < 1) return usage();
  if (seq_sig_parse(pos[0], &R.sig)) {
    fprintf(stderr, SEQ_SIG_WANT, PROG, pos[0]);
    return 1;
  }
  if (seq_parse_opm(opm, &R.bwd, &R.fwd, 1)) {
    fprintf(stderr, "%s: --opm must hold 3 or 6 numbers: FSCALE DW TH [FSCALE2 DW2 TH2]\n", PROG);
    return 1;
  }
  int smooth = SEQ_LAG1_OFF;
  if (smooth_s && !(smooth = seq_lag1_mode(smooth_s))) {
    fprintf(stderr, "%s: --smooth %s: want tvl1 or inv\n", PROG, smooth_s);
    return 1;
  }
  int matrix = 0, range = -1;
  if (!strcmp(matrix_s, "601")) matrix = 601;
  else if (!strcmp(matrix_s, "709")) matrix = 709;
  else if (strcmp(matrix_s, "auto")) { fprintf(stderr, "%s: --matrix %s: want 601, 709 or auto\n", PROG, matrix_s); return 1; }
  if (!strcmp(range_s, "limited")) range = 0;
  else if (!strcmp(range_s, "full")) range = 1;
  else if (strcmp(range_s, "auto")) { fprintf(stderr, "%s: --range %s: want limited, full or auto\n", PROG, range_s); return 1; }
  if (seq_run_params(&R, PROG " (--fpm)", fpm, PROG " (--spm)", smooth ? spm : NULL, &verbose)) {
    fprintf(stderr, "%s: both filtering iterations are needed (f1_p, f2_p != 0)\n", PROG);
    return 1;
  }

  FILE *in = !pos[1] || !strcmp(pos[1], "-") ? stdin : fopen(pos[1], "rb");
  if (!in) { fprintf(stderr, "%s: cannot open %s\n", PROG, pos[1]); return 1; }
  struct y4m_header hd;
  char err[Y4M_ERR_MAX];
  if (y4m_read_header(in, &hd, err)) { fprintf(stderr, "%s: %s\n", PROG, err); return 1; }
  if (!matrix) matrix = hd.w >= 1280 || hd.h > 576 ? 709 : 601;
  if (range < 0) range = hd.range == 1;
  hd.fmt.matrix = matrix;
  hd.fmt.full_range = range;
  if (want_probe) return probe(in, &hd, range ? "full" : "limited", matrix, max_frames);

  FILE *out = !pos[2] || !strcmp(pos[2], "-") ? stdout : fopen(pos[2], "wb");
  if (!out) { fprintf(stderr, "%s: cannot open %s\n", PROG, pos[2]); return 1; }
  if (y4m_write_header(out, &hd, err)) { fprintf(stderr, "%s: %s\n", PROG, err); return 1; }

  const int w = hd.w, h = hd.h, ch = hd.fmt.mono ? 1 : 3;
  if ((double)w * h * ch * sizeof(float) > 2e9) { /* (the frame calls index with int) */
    fprintf(stderr, "%s: a %d x %d frame is too large for the filter\n", PROG, w, h);
    return 1;
  }
  const size_t bytes = (size_t)w * h * ch * sizeof(float);
  C = nlkalman_hip_context();

  /* the ring (pinned), or one pageable buffer */
  G.in = in; G.out = out; G.hd = &hd; G.max_frames = max_frames;
  const char *e = getenv("NLK_SEQ_IO_THREADS");
  G.threads = !(e && atoi(e) == 0);
  if (G.threads) {
    int n = 0;
    for (; n < RING; ++n)
      if (nlk_host_alloc(C, &G.buf[n], hd.frame_bytes) != NLK_OK) break;
    if (n < RING) { /* not the whole ring: in-line I/O */
      while (n > 0) nlk_host_free(C, G.buf[--n]);
      G.threads = 0;
    }
  }
  if (!G.threads && !(G.buf[0] = malloc(hd.frame_bytes))) {
    fprintf(stderr, "%s: out of memory (%zu bytes)\n", PROG, hd.frame_bytes);
    return 1;
  }
  pthread_t th_r, th_w;
  if (G.threads && pthread_create(&th_r, NULL, reader, NULL)) G.threads = 0;
  if (G.threads && pthread_create(&th_w, NULL, writer, NULL)) {
    fprintf(stderr, "%s: cannot start the writer thread\n", PROG);
    return 1;
  }

  if (copy) { /* (nothing is filtered) */
    smooth = SEQ_LAG1_OFF;
    R.opts.defect_k = 0.f;
    R.opts.sure = 0;
  }
  CHK(seq_run_open(&R, C, w, h, ch, smooth));
  const struct seq_work *const W = &R.work;
  /* the codes; the RGB frame, flt1 and flt2 of this frame and the previous one, by turns, --smooth: the smoothed frame */
  void *d_yuv = NULL, *fr[6] = {0};
  CHK(nlk_dev_alloc(C, &d_yuv, hd.frame_bytes));
  for (int i = 0; i < (smooth ? 6 : 5); ++i) CHK(nlk_dev_alloc(C, &fr[i], bytes));
  float *d_rgb = fr[0], *flt1[2] = {fr[1], fr[2]}, *flt2[2] = {fr[3], fr[4]}, *d_lsm1 = fr[5];
  /* --sure: the terms of one frame (flt1's, then flt2's) and the sums of the lines printed */
  void *d_terms = NULL;
  double sure_sum[3] = {0.0, 0.0, 0.0};
  if (R.opts.sure) CHK(nlk_dev_alloc(C, &d_terms, sizeof(double) * 4 * ch));

  long t = 0;
  int failed = 0;
  for (;; ++t) {
    void *buf = frame_get(t);
    if (!buf) break;
    CHK(nlk_h2d(C, d_yuv, buf, hd.frame_bytes));
    CHK(nlk_dev_yuv_to_rgb(C, d_rgb, d_yuv, w, h, &hd.fmt));
    if (!copy) {
      if (t == 0) { /* sigma is known once the first frame is on the device, then every default that depends on it */
        const int rc = seq_run_first_frame(&R, d_rgb, stderr, PROG);
        if (rc == SEQ_SIG_REFUSED) { failed = 1; break; }
        CHK(rc);
      }
      const int cur = (int)(t & 1), prv = cur ^ 1;
      const struct seq_step step = {.d_rgb = d_rgb, .prev_flt1 = t ? flt1[prv] : NULL, .prev_flt2 = t ? flt2[prv] : NULL,
                                    .flt1 = flt1[cur], .flt2 = flt2[cur]};
      CHK(seq_forward_step(&R, &step));
      if (R.opts.sure) {
        double terms[4 * SEQ_SIG_MAX_CH];
        CHK(seq_sure_step(&R, &step, t, (double *)d_terms));
        CHK(nlk_d2h(C, terms, d_terms, sizeof(double) * 4 * ch));
        const struct seq_sure_est e = seq_sure_estimate(terms + 2 * ch, w, h, ch, R.sig.sigma, R.sure.eps_rel);
        fprintf(stderr, "sure %ld %.9g %.9g %.9g %.9g\n", t + 1, e.mse, e.psnr, e.resid, e.div);
        sure_sum[0] += e.mse; sure_sum[1] += e.resid; sure_sum[2] += e.div;
      }
      if (smooth) { /* frame t - 1 goes out smoothed, into its own buffer; frame t waits for the next one */
        if (t > 0) {
          const struct seq_lag1 lag = {.mode = smooth, .d_fflow = W->d_fflow, .d_focc = W->d_focc, .flt2 = flt2[prv],
                                       .next = flt2[cur], .smo1 = d_lsm1};
          CHK(seq_lag1_step(&R, &lag));
          if (emit(frame_buf(t - 1), d_lsm1, W->d_tmp, d_yuv, &hd, ch, &R.sig)) return 1;
          frame_put(t - 1);
          if (verbose) fprintf(stderr, "frame %ld smoothed\n", t);
        }
        if (verbose) fprintf(stderr, "frame %ld filtered\n", t + 1);
        if (write_has_failed()) {
          fprintf(stderr, "%s: %s\n", PROG, G.write_err);
          return 1;
        }
        continue;
      }
    }
    /* --copy: the RGB frame goes back as it is */
    if (emit(buf, copy ? d_rgb : flt2[t & 1], W->d_tmp, d_yuv, &hd, ch, copy ? NULL : &R.sig)) return 1;
    frame_put(t);
    if (verbose) fprintf(stderr, "frame %ld %s\n", t + 1, copy ? "converted" : "filtered");
    if (write_has_failed()) { /* nobody reads the output any more: stop filtering (the process ends, threads and all) */
      fprintf(stderr, "%s: %s\n", PROG, G.write_err);
      return 1;
    }
  }
  if (smooth && t > 0 && !failed) { /* the last frame goes out as its flt2 */
    if (emit(frame_buf(t - 1), flt2[(t - 1) & 1], W->d_tmp, d_yuv, &hd, ch, &R.sig)) return 1;
    frame_put(t - 1);
  }
  if (G.threads) {
    slot_set((int)(t % RING), OUTPUT_END); /* (slot t is the main thread's: it holds the end mark or a frame not used) */
    pthread_join(th_w, NULL);
    /* after an early `break` the reader may still wait for a slot: the process ends without joining it */
  }
  if (R.opts.sure && t > 0 && !failed)
    fprintf(stderr, "sure total %.9g %.9g %.9g %.9g\n", sure_sum[0] / t, 10.0 * log10(255.0 * 255.0 * t / sure_sum[0]),
            sure_sum[1] / t, sure_sum[2] / t);
  if (fflush(out) || (out != stdout && fclose(out))) { fprintf(stderr, "%s: write error\n", PROG); failed = 1; }
  if (G.write_failed) { fprintf(stderr, "%s: %s\n", PROG, G.write_err); failed = 1; }
  if (G.read_failed) { fprintf(stderr, "%s: frame %ld: %s\n", PROG, t + 1, G.read_err); failed = 1; }
  nlk_dev_free(C, d_yuv);
  for (int i = 0; i < 6; ++i)
    if (fr[i]) nlk_dev_free(C, fr[i]);
  if (d_terms) nlk_dev_free(C, d_terms);
  seq_run_close(&R);
  return failed;
}
