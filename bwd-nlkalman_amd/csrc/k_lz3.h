// k_lz3.h — the Lanczos-3 pyramid of the lz3 multiscale pipeline (scripts/msnlkalman-lz3-seq.sh; the
// operations are written out in DESIGN.md §9 and tests/lz3_ref.py). HWC interleaved float images, any
// w, h, ch >= 1; every operation is separable, horizontal pass first, then vertical.
//
//   down   n -> ceil(n/2):  down[m] = sum_t k[t] x[clamp(2m + t - 5)], t = 0..11
//   up     n -> N in {2n-1, 2n, 2n+1}: output i -> i' = min(i, 2n - 1) (the fit), j = i' >> 1,
//          even i': sum_s ke[s] x[clamp(j + s - 3)], odd i': sum_s ko[s] x[clamp(j + s - 2)], s = 0..5
//   gblur  correlation with ng Gaussian taps anchored at tap a, half-sample symmetric boundary
//
// A workgroup computes a tile of output pixels for a chunk of CC <= 4 channels (gridDim.z walks the
// chunks): the clamped / mirrored input window is staged in LDS in the image's own interleaved order
// (rows of (x, c) pairs, so a wavefront's loads are contiguous when CC == ch), each pass reads the
// previous one's LDS image and the last pass writes interleaved HWC. Every sum is an explicit fmaf
// chain in tap order: the result of a pixel does not depend on the tile it falls in, and no atomics
// are used, so results are bit-reproducible (and the down of the recompose step is this same kernel).
#pragma once
#include <hip/hip_runtime.h>

#define NLK_LZ3_THREADS 256
// down: output tile (coarse pixels)
#define NLK_LZ3_DTX 32
#define NLK_LZ3_DTY 8
// up / recompose: output tile (fine pixels) and the coarse window it reads (see k_lz3_up)
#define NLK_LZ3_UTX 64
#define NLK_LZ3_UTY 16
#define NLK_LZ3_EW (NLK_LZ3_UTX / 2 + 8)
#define NLK_LZ3_EH (NLK_LZ3_UTY / 2 + 8)
#define NLK_LZ3_MAXG 64  // gblur taps

struct NlkLz3Taps {
  float down[12];
  float even[6], odd[6];     // up: ke[s - 3], ko[s - 2]
  float gauss[NLK_LZ3_MAXG];  // gblur (ng taps, anchor a)
};

__device__ __forceinline__ int lz3_clamp(int i, int n) { return min(max(i, 0), n - 1); }
// half-sample symmetric reflection, period 2n (x[-1] = x[0], x[-2] = x[1]); any n >= 1 and any i
__device__ __forceinline__ int lz3_mirror(int i, int n) {
  const int p = 2 * n;
  i %= p;
  if (i < 0) i += p;
  return i < n ? i : p - 1 - i;
}

// dst[r][k] for r < rows, k < cols * CC: channel c0 + (k % CC) of the pixel (mapx(k / CC), mapy(r)) of src
// (0 for channels past ch)
template <int CC, typename MX, typename MY>
__device__ __forceinline__ void lz3_stage(float* dst, int rows, int cols, const float* __restrict__ src, int w,
                                          int ch, int c0, MX mapx, MY mapy) {
  const int n = rows * cols * CC, rowlen = cols * CC;
  for (int i = threadIdx.x; i < n; i += NLK_LZ3_THREADS) {
    const int r = i / rowlen, k = i - r * rowlen, x = k / CC, c = k - x * CC;
    dst[i] = c0 + c < ch ? src[((size_t)mapy(r) * w + mapx(x)) * ch + c0 + c] : 0.f;
  }
}

// ---- down: one launch per level. Window: rows 2 TY + 11, columns 2 TX + 11 (all CC channels).
template <int CC>
__global__ void __launch_bounds__(NLK_LZ3_THREADS)
k_lz3_down(float* __restrict__ dst, const float* __restrict__ src, int w, int h, int ch, NlkLz3Taps tp) {
  constexpr int TX = NLK_LZ3_DTX, TY = NLK_LZ3_DTY, IW = 2 * TX + 11, IH = 2 * TY + 11;
  __shared__ float in[IH * IW * CC];
  __shared__ float hs[IH * TX * CC];
  const int dw = (w + 1) / 2, dh = (h + 1) / 2, c0 = blockIdx.z * CC;
  const int X0 = blockIdx.x * TX, Y0 = blockIdx.y * TY;
  lz3_stage<CC>(in, IH, IW, src, w, ch, c0, [=](int x) { return lz3_clamp(2 * X0 - 5 + x, w); },
                [=](int r) { return lz3_clamp(2 * Y0 - 5 + r, h); });
  __syncthreads();
  // horizontal: hs[r][ox][c] = sum_t k[t] in[r][2 ox + t][c]
  for (int i = threadIdx.x; i < IH * TX * CC; i += NLK_LZ3_THREADS) {
    const int r = i / (TX * CC), k = i - r * (TX * CC), ox = k / CC, c = k - ox * CC;
    const float* p = in + r * IW * CC + 2 * ox * CC + c;
    float s = 0.f;
#pragma unroll
    for (int t = 0; t < 12; ++t) s = fmaf(tp.down[t], p[t * CC], s);
    hs[i] = s;
  }
  __syncthreads();
  // vertical: dst[oy][ox][c] = sum_t k[t] hs[2 oy + t][ox][c]
  const int nc = min(CC, ch - c0);
  for (int i = threadIdx.x; i < TY * TX * CC; i += NLK_LZ3_THREADS) {
    const int oy = i / (TX * CC), k = i - oy * (TX * CC), ox = k / CC, c = k - ox * CC;
    if (Y0 + oy >= dh || X0 + ox >= dw || c >= nc) continue;
    const float* p = hs + 2 * oy * TX * CC + k;
    float s = 0.f;
#pragma unroll
    for (int t = 0; t < 12; ++t) s = fmaf(tp.down[t], p[t * TX * CC], s);
    dst[((size_t)(Y0 + oy) * dw + X0 + ox) * ch + c0 + c] = s;
  }
}

// ---- up (+ the recompose step's second half). Output tile TX x TY at (X0, Y0) of the dw x dh result; it
// reads coarse samples j + s with j = min(x, 2n - 1) >> 1 in [X0/2 - 1, X0/2 + TX/2 - 1] and s in [-3, 3], so
// the coarse window E is [QX0, QX0 + EW) with QX0 = X0/2 - 4, EW = TX/2 + 8 (same for rows); E[e] holds the
// coarse value at clamp(QX0 + e).
//
// RECOMPOSE: out = yh + up(gblur(rl - dl)) with dl = down(yh) (k_lz3_down, launched first). E is then the
// blurred difference: the difference F = rl - dl is staged over the window widened by the ng - 1 Gaussian
// taps, at the mirrored positions mirror(QX0 - a + p); E[e] = sum_t g[t] F[clamp(QX0 + e) - QX0 + t] — the
// up's clamp composed with gblur's mirror in the tile's index map. The plain up has ng = 1 and no yh.
// LDS: region A holds F (then E), region B the horizontal results of the blur (then of the up).
template <int CC, bool RECOMPOSE>
__global__ void __launch_bounds__(NLK_LZ3_THREADS)
k_lz3_up(float* out, int dw, int dh, const float* yh,  // (out may be yh: each output reads its own yh sample)
         const float* __restrict__ rl,
         const float* __restrict__ dl, int w, int h, int ch, int ng, int a, NlkLz3Taps tp) {
  constexpr int TX = NLK_LZ3_UTX, TY = NLK_LZ3_UTY, EW = NLK_LZ3_EW, EH = NLK_LZ3_EH;
  extern __shared__ float lds[];
  const int FW = EW + ng - 1, FH = EH + ng - 1;
  float* A = lds;
  float* B = lds + (RECOMPOSE ? max(FH * FW, EH * EW) : EH * EW) * CC;
  const int c0 = blockIdx.z * CC, X0 = blockIdx.x * TX, Y0 = blockIdx.y * TY;
  const int QX0 = X0 / 2 - 4, QY0 = Y0 / 2 - 4;
  if (RECOMPOSE) {
    {
      const int n = FH * FW * CC, rowlen = FW * CC;
      for (int i = threadIdx.x; i < n; i += NLK_LZ3_THREADS) {
        const int r = i / rowlen, k = i - r * rowlen, x = k / CC, c = k - x * CC;
        const size_t o = ((size_t)lz3_mirror(QY0 - a + r, h) * w + lz3_mirror(QX0 - a + x, w)) * ch + c0 + c;
        A[i] = c0 + c < ch ? rl[o] - dl[o] : 0.f;
      }
    }
    __syncthreads();
    // horizontal blur: B[r][e][c] = sum_t g[t] F[r][cx(e) + t][c]
    for (int i = threadIdx.x; i < FH * EW * CC; i += NLK_LZ3_THREADS) {
      const int r = i / (EW * CC), k = i - r * (EW * CC), e = k / CC, c = k - e * CC;
      const float* p = A + r * FW * CC + (lz3_clamp(QX0 + e, w) - QX0) * CC + c;
      float s = 0.f;
      for (int t = 0; t < ng; ++t) s = fmaf(tp.gauss[t], p[t * CC], s);
      B[i] = s;
    }
    __syncthreads();
    // vertical blur: E[e][k] = sum_t g[t] B[cy(e) + t][k]
    for (int i = threadIdx.x; i < EH * EW * CC; i += NLK_LZ3_THREADS) {
      const int e = i / (EW * CC), k = i - e * (EW * CC);
      const float* p = B + (lz3_clamp(QY0 + e, h) - QY0) * EW * CC + k;
      float s = 0.f;
      for (int t = 0; t < ng; ++t) s = fmaf(tp.gauss[t], p[t * EW * CC], s);
      A[i] = s;
    }
  } else {
    lz3_stage<CC>(A, EH, EW, rl, w, ch, c0, [=](int x) { return lz3_clamp(QX0 + x, w); },
                  [=](int r) { return lz3_clamp(QY0 + r, h); });
  }
  __syncthreads();
  // horizontal up: B[e][lx][c] for the tile's columns
  for (int i = threadIdx.x; i < EH * TX * CC; i += NLK_LZ3_THREADS) {
    const int e = i / (TX * CC), k = i - e * (TX * CC), lx = k / CC, c = k - lx * CC;
    const int ip = min(X0 + lx, 2 * w - 1), j = ip >> 1;
    const bool odd = ip & 1;
    const float* p = A + e * EW * CC + (j - QX0 - 3 + odd) * CC + c;
    float s = 0.f;
#pragma unroll
    for (int t = 0; t < 6; ++t) s = fmaf(odd ? tp.odd[t] : tp.even[t], p[t * CC], s);
    B[i] = s;
  }
  __syncthreads();
  // vertical up, + yh when recomposing; interleaved HWC store
  const int nc = min(CC, ch - c0);
  for (int i = threadIdx.x; i < TY * TX * CC; i += NLK_LZ3_THREADS) {
    const int ly = i / (TX * CC), k = i - ly * (TX * CC), lx = k / CC, c = k - lx * CC;
    if (Y0 + ly >= dh || X0 + lx >= dw || c >= nc) continue;
    const int ip = min(Y0 + ly, 2 * h - 1), j = ip >> 1;
    const bool odd = ip & 1;
    const float* p = B + (j - QY0 - 3 + odd) * TX * CC + k;
    float s = 0.f;
#pragma unroll
    for (int t = 0; t < 6; ++t) s = fmaf(odd ? tp.odd[t] : tp.even[t], p[t * TX * CC], s);
    const size_t o = ((size_t)(Y0 + ly) * dw + X0 + lx) * ch + c0 + c;
    out[o] = RECOMPOSE ? yh[o] + s : s;
  }
}
