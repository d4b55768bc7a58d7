// k_ssim.h — the structural similarity of two images (include/nlk_hip.h: nlk_dev_ssim; DESIGN.md §9, "Quality
// measure"): the SSIM of Wang, Bovik, Sheikh and Simoncelli (2004) with the 11-tap Gaussian window (sigma 1.5),
// population moments and the valid region, every channel by itself, all statistics in double.
//
//   k_ssim_tile   one workgroup per (tile of NLK_SSIM_TX x NLK_SSIM_TY valid positions, channel):
//                   1. the (TX + 10) x (TY + 10) samples of both images, converted to double, into LDS (a sample
//                      outside the image is 0: only positions outside the valid region see it)
//                   2. the row pass: sum_j g[j] v[y][x + j] of v = a, b, a a, b b, a b (the products of two converted
//                      floats are exact) into five double planes in LDS
//                   3. the column pass from those planes, two vertically adjacent positions per thread (12 rows read
//                      for 2 x 11 taps), S in double, the map where asked
//                   4. S of the workgroup's valid positions summed by an LDS tree with fixed pairing: one partial per
//                      (channel, tile). A position outside the valid region contributes +0 by selection, not by a
//                      product, so a non-finite value never leaves the windows that hold it.
//   k_ssim_final  one workgroup: per channel, thread t sums the partials t, t + 256, ... in order, then the tree;
//                 ssim_c = that / count, ssim = the mean of the ssim_c in channel order.
// No atomics; every order of summation depends on (w, h, ch) alone.
//
// LDS: the samples 2 x 26 x 42 doubles (17.1 KiB), the planes 5 x 26 x 32 doubles (32.5 KiB), the tree 2 KiB: 51.6
// KiB, three workgroups per CU. Every access is 8 bytes wide with the lanes of a 32-lane half on consecutive
// doubles (one 256-byte bank row): the row pass reads sample (r, x + j) with x on the lane, the column pass reads
// plane (y + i, x) with x on the lane, and both write what they read next in the same order.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define NLK_SSIM_THREADS 256
#define NLK_SSIM_TAPS 11
#define NLK_SSIM_R 5                                   // window radius: the valid region loses this much per side
#define NLK_SSIM_TX 32                                 // valid positions per tile ...
#define NLK_SSIM_TY 16                                 // ... 2 per thread
#define NLK_SSIM_SX (NLK_SSIM_TX + NLK_SSIM_TAPS - 1)  // 42 samples per tile row
#define NLK_SSIM_SY (NLK_SSIM_TY + NLK_SSIM_TAPS - 1)  // 26 tile rows
#define NLK_SSIM_MAX_CH 16

static_assert(NLK_SSIM_TX * NLK_SSIM_TY == 2 * NLK_SSIM_THREADS, "two positions per thread");
static_assert(NLK_SSIM_TX == 32, "a 32-lane half reads one row of a plane");

struct NlkSsimWin {
  double g[NLK_SSIM_TAPS];  // the normalised Gaussian, made in double on the host
};

// LDS tree over the NLK_SSIM_THREADS values of a workgroup, fixed pairing; the result is in v[0]
__device__ __forceinline__ void ssim_tree(double* v) {
#pragma unroll
  for (int half = NLK_SSIM_THREADS / 2; half > 0; half >>= 1) {
    __syncthreads();
    if ((int)threadIdx.x < half) v[threadIdx.x] += v[threadIdx.x + half];
  }
  __syncthreads();
}

// S of one position from its five window moments
__device__ __forceinline__ double ssim_value(double ma, double mb, double eaa, double ebb, double eab, double c1,
                                             double c2) {
  const double va = eaa - ma * ma, vb = ebb - mb * mb, cab = eab - ma * mb;
  return ((2.0 * ma * mb + c1) * (2.0 * cab + c2)) / ((ma * ma + mb * mb + c1) * (va + vb + c2));
}

// grid (tiles in x, tiles in y, ch); part [ch][tiles in y][tiles in x]; map [h - 10][w - 10][ch] or NULL
__global__ __launch_bounds__(NLK_SSIM_THREADS) void k_ssim_tile(double* part, float* map, const float* a,
                                                                const float* b, int w, int h, int ch, NlkSsimWin win,
                                                                double c1, double c2) {
  __shared__ double sa[NLK_SSIM_SY][NLK_SSIM_SX], sb[NLK_SSIM_SY][NLK_SSIM_SX];
  __shared__ double rows[5][NLK_SSIM_SY][NLK_SSIM_TX];
  __shared__ double red[NLK_SSIM_THREADS];
  const int t = threadIdx.x, c = blockIdx.z;
  const int x0 = blockIdx.x * NLK_SSIM_TX, y0 = blockIdx.y * NLK_SSIM_TY;  // first valid position = first sample
  const int vw = w - 2 * NLK_SSIM_R, vh = h - 2 * NLK_SSIM_R;

  // 1. the samples (x0 + x < w and y0 + r < h checked: nothing outside the images is read)
  for (int i = t; i < NLK_SSIM_SY * NLK_SSIM_SX; i += NLK_SSIM_THREADS) {
    const int r = i / NLK_SSIM_SX, x = i - r * NLK_SSIM_SX;
    double va = 0.0, vb = 0.0;
    if (x0 + x < w && y0 + r < h) {
      const size_t at = ((size_t)(y0 + r) * w + (x0 + x)) * ch + c;
      va = (double)a[at];
      vb = (double)b[at];
    }
    sa[r][x] = va;
    sb[r][x] = vb;
  }
  __syncthreads();

  // 2. rows
  for (int i = t; i < NLK_SSIM_SY * NLK_SSIM_TX; i += NLK_SSIM_THREADS) {
    const int r = i / NLK_SSIM_TX, x = i % NLK_SSIM_TX;
    double ma = 0.0, mb = 0.0, eaa = 0.0, ebb = 0.0, eab = 0.0;
#pragma unroll
    for (int j = 0; j < NLK_SSIM_TAPS; ++j) {
      const double g = win.g[j], pa = sa[r][x + j], pb = sb[r][x + j];
      ma += g * pa;
      mb += g * pb;
      eaa += g * (pa * pa);
      ebb += g * (pb * pb);
      eab += g * (pa * pb);
    }
    rows[0][r][x] = ma;
    rows[1][r][x] = mb;
    rows[2][r][x] = eaa;
    rows[3][r][x] = ebb;
    rows[4][r][x] = eab;
  }
  __syncthreads();

  // 3. columns: the positions (x, y) and (x, y + 1) of the tile
  const int x = t % NLK_SSIM_TX, y = 2 * (t / NLK_SSIM_TX);
  double m0[5], m1[5];
#pragma unroll
  for (int k = 0; k < 5; ++k) {
    double s0 = 0.0, s1 = 0.0;
#pragma unroll
    for (int i = 0; i <= NLK_SSIM_TAPS; ++i) {
      const double v = rows[k][y + i][x];
      if (i < NLK_SSIM_TAPS) s0 += win.g[i] * v;
      if (i > 0) s1 += win.g[i - 1] * v;
    }
    m0[k] = s0;
    m1[k] = s1;
  }
  const bool in0 = x0 + x < vw && y0 + y < vh, in1 = x0 + x < vw && y0 + y + 1 < vh;
  const double S0 = ssim_value(m0[0], m0[1], m0[2], m0[3], m0[4], c1, c2);
  const double S1 = ssim_value(m1[0], m1[1], m1[2], m1[3], m1[4], c1, c2);
  if (map) {
    const size_t at = ((size_t)(y0 + y) * vw + (x0 + x)) * ch + c;
    if (in0) map[at] = (float)S0;
    if (in1) map[at + (size_t)vw * ch] = (float)S1;
  }

  // 4. the tile's sum
  red[t] = (in0 ? S0 : 0.0) + (in1 ? S1 : 0.0);
  ssim_tree(red);
  if (t == 0) part[((size_t)c * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x] = red[0];
}

// one workgroup: out[1 + c] = the mean of channel c's npart partials over count positions, out[0] = their mean
__global__ __launch_bounds__(NLK_SSIM_THREADS) void k_ssim_final(double* out, const double* part, int ch, int npart,
                                                                 double count) {
  __shared__ double red[NLK_SSIM_THREADS];
  double all = 0.0;  // (every thread keeps the same running sum)
  for (int c = 0; c < ch; ++c) {
    const double* p = part + (size_t)c * npart;
    double acc = 0.0;
    for (int i = threadIdx.x; i < npart; i += NLK_SSIM_THREADS) acc += p[i];
    red[threadIdx.x] = acc;
    ssim_tree(red);
    const double mean = red[0] / count;
    __syncthreads();  // red[0] is read by all before the next channel overwrites it
    if (threadIdx.x == 0) out[1 + c] = mean;
    all += mean;
  }
  if (threadIdx.x == 0) out[0] = all / (double)ch;
}
