// nlk_hip.hip — C-ABI (include/nlk_hip.h) over the gfx950 kernels: the context and the small services around it
// (create and destroy, switches, streams, memory and copies, colour transforms, the warp, the host tables). The frame
// pipeline is tu_frame.hip; every other entry point lives in the unit of its kernels.
//
// One context per (process, device). All work is enqueued on the context's
// stream; scratch buffers are grown on demand and kept, so a steady-state frame
// call performs no allocation (context/alloc time is on the
// CLI critical path).
#include <math.h>
#include <time.h>

#include <algorithm>
#include <mutex>
#include <vector>

// (the 12-point flow graph of the device code, compiled for the host: nlk_host_tables lets the tests pin it)
namespace nlk_host12 {
#define NLK_HD static inline
#include "k_dct12.h"
#undef NLK_HD
}  // namespace nlk_host12

#include "k_image.h"
#include "nlk_internal.h"

char nlk_g_err[512] = "";

namespace {

// live contexts (nlk_ctx_reload_switches(NULL) re-reads the environment for all of them)
std::mutex g_live_mu;
std::vector<nlk_ctx*> g_live;

typedef NlkBuf Buf;

}  // namespace

// reference: src/nlkalman.c:365-419 ("gaussian"), float/double mix as written there
void host_window(float* W, int psz) {
  float w1[64];
  const float N2 = ((float)psz - 1.) / 2.;
  for (int n = 0; n < psz; ++n) {
    const float s = .4;
    const float x = ((float)n - N2) / N2 / s;
    w1[n] = exp(-.5 * x * x);
  }
  for (int i = 0; i < psz; ++i)
    for (int j = 0; j < psz; ++j) W[i * psz + j] = w1[i] * w1[j];
}

// orthonormal DCT-II basis = FFTW REDFT10 x the reference's scaling
// (reference: src/nlkalman.c:204-212, 281-298)
void host_basis(float* C, int n) {
  for (int k = 0; k < n; ++k)
    for (int j = 0; j < n; ++j) {
      const double s = (k == 0) ? sqrt(1.0 / n) : sqrt(2.0 / n);
      C[k * n + j] = (float)(s * cos(M_PI * (j + 0.5) * k / n));
    }
}

int check_images(nlk_ctx* c, const void* out, const void* cur, int w, int h, int ch) {
  if (!c) return fail(nullptr, NLK_EINVAL, "null context");
  if (!out || !cur) return fail(c, NLK_EINVAL, "null image pointer");
  if (w <= 0 || h <= 0 || ch <= 0) return fail(c, NLK_EINVAL, "bad image size %dx%dx%d", w, h, ch);
  if (w > 65535 || h > 65535) return fail(c, NLK_EUNSUP, "image side above 65535");
  return NLK_OK;
}

extern "C" {

int nlk_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

const char* nlk_last_error(const nlk_ctx* ctx) { return ctx ? ctx->err : nlk_g_err; }

int nlk_ctx_create(nlk_ctx** out, int device) {
  if (!out) return fail(nullptr, NLK_EINVAL, "null ctx pointer");
  *out = nullptr;
  int n = 0;
  struct timespec tt0;
  clock_gettime(CLOCK_MONOTONIC, &tt0);
  if (hipGetDeviceCount(&n) != hipSuccess || n <= 0)
    return fail(nullptr, NLK_ENODEV, "no HIP device visible (the HIP path is mandatory: there is no CPU fallback)");
  if (device < 0 || device >= n)
    return fail(nullptr, NLK_ENODEV, "device %d out of range (%d visible)", device, n);
  nlk_ctx* c = new nlk_ctx();
  c->device = device;
  const bool trace = getenv("NLK_CLI_TRACE") != nullptr;   // (where a one-shot process spends its start-up)
  auto lap = [&](const char* what) {
    if (!trace) return;
    struct timespec t;
    clock_gettime(CLOCK_MONOTONIC, &t);
    fprintf(stderr, "[nlk_ctx_create +%7.2f ms] %s\n", (t.tv_sec - tt0.tv_sec) * 1e3 + (t.tv_nsec - tt0.tv_nsec) * 1e-6, what);
  };
  lap("hipGetDeviceCount (runtime initialised)");
  if (hipSetDevice(device) != hipSuccess ||
      hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking) != hipSuccess) {
    delete c;
    return fail(nullptr, NLK_EHIP, "cannot create a stream on device %d", device);
  }
  lap("first stream");
  c->stream = c->own_stream;
  c->sw.load();
  c->deterministic = nlk_or(c->sw.deterministic, 0) != 0;
  bool ok = hipStreamCreateWithFlags(&c->aux_stream, hipStreamNonBlocking) == hipSuccess;
  for (hipEvent_t& e : c->sync_ev) ok = ok && hipEventCreateWithFlags(&e, hipEventDisableTiming) == hipSuccess;
  if (!ok) {
    nlk_ctx_destroy(c);
    return fail(nullptr, NLK_EHIP, "cannot create the second stream / events on device %d", device);
  }
  lap("second stream + events");
  {
    std::lock_guard<std::mutex> lock(g_live_mu);
    g_live.push_back(c);
  }
  *out = c;
  return NLK_OK;
}

void nlk_ctx_destroy(nlk_ctx* c) {
  if (!c) return;
  {
    std::lock_guard<std::mutex> lock(g_live_mu);
    g_live.erase(std::remove(g_live.begin(), g_live.end(), c), g_live.end());
  }
  hipSetDevice(c->device);
  hipStreamSynchronize(c->stream);
  if (c->aux_stream) hipStreamSynchronize(c->aux_stream);
  Buf* bufs[] = {&c->planes, &c->rowok, &c->vmap, &c->topk,
                 &c->tinfo, &c->gcoords, &c->marks, &c->active, &c->acc, &c->tabs, &c->wide, &c->tv, &c->bm, &c->skew, &c->chase, &c->ms, &c->lz3, &c->sqd, &c->sig, &c->curve, &c->ssim, &c->sure, &c->nlf,
                 &c->slab, &c->tflag, &c->hw_cur, &c->hw_prev, &c->hw_basic, &c->hw_out};
  for (Buf* b : bufs)
    if (b->p) hipFree(b->base ? b->base : b->p);
  for (int i = 0; i < c->lz3_nold; ++i) hipFree(c->lz3_old[i]);
  if (c->tv_host) (void)hipHostFree(c->tv_host);
  free(c->nlf_host);
  if (c->ev) {
    for (int i = 0; i < nlk_ctx::MAXSETS * nlk_ctx::NEV; ++i) (void)hipEventDestroy(c->ev[i]);
    free(c->ev);
  }
  for (hipEvent_t e : c->sync_ev)
    if (e) (void)hipEventDestroy(e);
  for (auto& row : c->band_ev)
    for (hipEvent_t e : row)
      if (e) (void)hipEventDestroy(e);
  if (c->up_stream) (void)hipStreamDestroy(c->up_stream);
  if (c->dn_stream) (void)hipStreamDestroy(c->dn_stream);
  if (c->aux_stream) (void)hipStreamDestroy(c->aux_stream);
  (void)hipStreamDestroy(c->own_stream);
  delete c;
}

int nlk_ctx_set_deterministic(nlk_ctx* c, int on) {
  if (!c) return NLK_EINVAL;
  c->deterministic = on != 0;
  return NLK_OK;
}

int nlk_ctx_reload_switches(nlk_ctx* c) {
  std::lock_guard<std::mutex> lock(g_live_mu);
  for (nlk_ctx* x : g_live)
    if (!c || x == c) {
      x->sw.load();
      if (nlk_set(x->sw.deterministic)) x->deterministic = x->sw.deterministic != 0;
    }
  return NLK_OK;
}

int nlk_ctx_set_stream(nlk_ctx* c, void* s) {
  if (!c) return NLK_EINVAL;
  c->stream = (hipStream_t)s;  // NULL is the legacy default stream (what torch uses by default)
  return NLK_OK;
}

int nlk_ctx_use_own_stream(nlk_ctx* c) {
  if (!c) return NLK_EINVAL;
  c->stream = c->own_stream;
  return NLK_OK;
}

void* nlk_ctx_get_stream(nlk_ctx* c) { return c ? (void*)c->stream : nullptr; }

int nlk_dev_alloc(nlk_ctx* c, void** d, size_t bytes) {
  if (!c || !d) return fail(c, NLK_EINVAL, "null argument");
  NLK_USE_DEVICE(c);
  if (hipMalloc(d, bytes) != hipSuccess) return fail(c, NLK_ENOMEM, "hipMalloc(%zu) failed", bytes);
  return NLK_OK;
}
int nlk_dev_free(nlk_ctx* c, void* d) {
  if (!c) return NLK_EINVAL;
  NLK_USE_DEVICE(c);
  HIPCHK(c, hipFree(d));
  return NLK_OK;
}
int nlk_h2d(nlk_ctx* c, void* d, const void* h, size_t n) {
  if (!c) return NLK_EINVAL;
  NLK_USE_DEVICE(c);
  HIPCHK(c, hipMemcpyAsync(d, h, n, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return NLK_OK;
}
int nlk_d2h(nlk_ctx* c, void* h, const void* d, size_t n) {
  if (!c) return NLK_EINVAL;
  NLK_USE_DEVICE(c);
  HIPCHK(c, hipMemcpyAsync(h, d, n, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return NLK_OK;
}
int nlk_d2d(nlk_ctx* c, void* dst, const void* src, size_t n) {
  if (!c) return NLK_EINVAL;
  NLK_USE_DEVICE(c);
  HIPCHK(c, hipMemcpyAsync(dst, src, n, hipMemcpyDeviceToDevice, c->stream));
  return NLK_OK;
}
int nlk_dev_zero(nlk_ctx* c, void* d, size_t n) {
  if (!c || !d) return fail(c, NLK_EINVAL, "null argument");
  NLK_USE_DEVICE(c);
  HIPCHK(c, hipMemsetAsync(d, 0, n, c->stream));
  return NLK_OK;
}
int nlk_dev_add(nlk_ctx* c, float* dst, const float* src, size_t n) {
  if (!c || !dst || !src) return fail(c, NLK_EINVAL, "null argument");
  if (n == 0) return NLK_OK;
  NLK_USE_DEVICE(c);
  hipLaunchKernelGGL(k_add, dim3(1024), dim3(256), 0, c->stream, dst, src, n);
  HIPCHK(c, hipGetLastError());
  return NLK_OK;
}
// everything enqueued on src_ctx's stream so far has run when the copy starts; the copy itself is
// ordered on dst_ctx's stream
int nlk_dev_copy_peer(nlk_ctx* dc, void* dst, nlk_ctx* sc, const void* src, size_t n) {
  if (!dc || !sc || !dst || !src) return fail(dc, NLK_EINVAL, "null argument");
  HIPCHK(dc, hipSetDevice(sc->device));
  HIPCHK(dc, hipEventRecord(sc->sync_ev[7], sc->stream));
  HIPCHK(dc, hipSetDevice(dc->device));
  HIPCHK(dc, hipStreamWaitEvent(dc->stream, sc->sync_ev[7], 0));
  HIPCHK(dc, hipMemcpyPeerAsync(dst, dc->device, src, sc->device, n, dc->stream));
  return NLK_OK;
}
int nlk_host_alloc(nlk_ctx* c, void** h, size_t n) {
  if (!c || !h) return NLK_EINVAL;
  NLK_USE_DEVICE(c);
  HIPCHK(c, hipHostMalloc(h, n, hipHostMallocDefault));
  return NLK_OK;
}
int nlk_host_free(nlk_ctx* c, void* h) {
  if (!c) return NLK_EINVAL;
  NLK_USE_DEVICE(c);
  if (h) HIPCHK(c, hipHostFree(h));
  return NLK_OK;
}
int nlk_sync(nlk_ctx* c) {
  if (!c) return NLK_EINVAL;
  NLK_USE_DEVICE(c);
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return NLK_OK;
}

int nlk_dev_rgb2opp(nlk_ctx* c, float* im, int w, int h, int ch) {
  int rc = check_images(c, im, im, w, h, ch);
  if (rc) return rc;
  NLK_USE_DEVICE(c);
  if (ch != 3) return NLK_OK;
  hipLaunchKernelGGL(k_rgb2opp, dim3(2048), dim3(256), 0, c->stream, im, (size_t)w * h);
  HIPCHK(c, hipGetLastError());
  return NLK_OK;
}

int nlk_dev_opp2rgb(nlk_ctx* c, float* im, int w, int h, int ch) {
  int rc = check_images(c, im, im, w, h, ch);
  if (rc) return rc;
  NLK_USE_DEVICE(c);
  if (ch != 3) return NLK_OK;
  hipLaunchKernelGGL(k_opp2rgb, dim3(2048), dim3(256), 0, c->stream, im, (size_t)w * h);
  HIPCHK(c, hipGetLastError());
  return NLK_OK;
}

int nlk_dev_warp_bicubic(nlk_ctx* c, float* imw, const float* im, const float* of,
                         const float* msk, int w, int h, int ch) {
  int rc = check_images(c, imw, im, w, h, ch);
  if (rc) return rc;
  NLK_USE_DEVICE(c);
  if (!of) return fail(c, NLK_EINVAL, "null flow");
  auto kern = ch == 3 ? k_warp_bicubic<3> : (ch == 1 ? k_warp_bicubic<1> : k_warp_bicubic<0>);
  hipLaunchKernelGGL(kern, dim3((w + 127) / 128, h), dim3(128), 0, c->stream, imw,
                     im, of, msk, w, h, ch);
  HIPCHK(c, hipGetLastError());
  return NLK_OK;
}


// the tables upload_tables() sends to the device, for tests that pin them (tests/test_fftw_pin.py)
int nlk_host_tables(int psz, float* basis, float* window, float* basis12_regs) {
  if (psz < 2 || psz > 64) return fail(nullptr, NLK_EINVAL, "patch size %d", psz);
  if (basis) host_basis(basis, psz);
  if (window) host_window(window, psz);
  if (basis12_regs)  // the matrix the 12-point flow graph of k_dct12.h (what k_groupp<12> runs) applies: graph(e_j) = column j
    for (int j = 0; j < 12; ++j) {
      float e[12] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
      e[j] = 1.f;
      nlk_host12::nlk_dct12_fast_fwd(e);
      for (int k = 0; k < 12; ++k) basis12_regs[k * 12 + j] = e[k];
    }
  return NLK_OK;
}

// The packed-list byte code for tests without a device, through the functions the kernels call (nlk_common.h): an
// entry at displacement (dx, dy) from a target at (px, py) that searched radius r and kept k candidates, `passthrough`
// as in nlk_pl_target_fits. *byte = its code (nlk_pl_word, nlk_pl_byte: the matcher's epilogue), back[0..1] = the frame
// coordinate decoded from it again (nlk_pl_decode: k_group8m); either may be null. NLK_EINVAL where the target cannot
// have a valid record (nlk_pl_target_fits: what the epilogue asks before it sets the flag) or the entry has no code.
int nlk_host_packed_entry(int px, int py, int dx, int dy, int r, int k, int passthrough, unsigned int* byte, int* back) {
  if (px < 0 || py < 0 || px + dx < 0 || py + dy < 0 || px + dx > 65535 || py + dy > 65535)
    return fail(nullptr, NLK_EINVAL, "entry (%d + %d, %d + %d) outside a frame", px, dx, py, dy);
  if (!nlk_pl_target_fits(k, r, passthrough != 0))
    return fail(nullptr, NLK_EINVAL, "no packed record for a target with %d candidates at radius %d%s", k, r,
                passthrough ? " (pass-through)" : "");
  const uint32_t word = nlk_pl_word(nlk_pack_xy(px + dx, py + dy), px, py, r);
  if (!nlk_pl_encodes(word, r))
    return fail(nullptr, NLK_EINVAL, "displacement (%d, %d) at radius %d has no packed code", dx, dy, r);
  const uint32_t b = nlk_pl_byte(word);
  if (byte) *byte = b;
  if (back) {
    const uint32_t q = nlk_pl_decode(b, px, py, r);
    back[0] = nlk_x(q);
    back[1] = nlk_y(q);
  }
  return NLK_OK;
}


}  // extern "C"

