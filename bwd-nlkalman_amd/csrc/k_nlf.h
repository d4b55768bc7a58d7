// k_nlf.h — the noise-level-function transform of nlk_dev_nlf_forward / nlk_dev_nlf_inverse (include/nlk_hip.h,
// DESIGN.md §9): a monotone piecewise-linear map per channel of an HWC image, its knots x[0..nbins] at the bin edges
// of the noise curve. One pass, element by element (so in place is fine); every operation rounded by itself.
//   forward   t = fminf(fmaxf((y - lo) inv_dx, 0), nbins - 1), j = (int)floorf(t), g = G[j] + (y - x[j]) slope[j]
//   inverse   j = the number of k in 1..nbins-1 with G[k] <= g (G does not decrease: a binary search),
//             y = x[j] + (g - G[j]) islope[j]
// NaN: every comparison is false, j = 0, and the arithmetic gives NaN; +-inf lands in an end segment and stays.
// The device table (tu_nlf.hip keeps it in the context) is rows of NLK_NLF_ROW floats:
//   x | G[16] | slope[16] | islope[16]
// A workgroup stages x and the rows of its direction, ch (nbins + 1) floats each, in LDS: a lane's channel and segment
// vary, and 16 x 65 x 3 floats are too many for kernel arguments.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define NLK_NLF_THREADS 256
#define NLK_NLF_CH 16    // NLK_NLF_MAX_CH
#define NLK_NLF_ROW 65   // NLK_NLF_MAX_BINS + 1
#define NLK_NLF_TABLE_FLOATS ((1 + 3 * NLK_NLF_CH) * NLK_NLF_ROW)

template <bool INVERSE>
__global__ __launch_bounds__(NLK_NLF_THREADS) void k_nlf(float* out, const float* in, uint64_t n, int ch, int nbins,
                                                         float lo, float inv_dx, const float* __restrict__ tab) {
#pragma clang fp contract(off)
  __shared__ float sx[NLK_NLF_ROW];
  __shared__ float sg[NLK_NLF_CH * NLK_NLF_ROW];  // G, [ch][nbins + 1]
  __shared__ float ss[NLK_NLF_CH * NLK_NLF_ROW];  // slope | islope, likewise (the last of a row is not used)
  const int nb1 = nbins + 1;
  const float* tg = tab + NLK_NLF_ROW;
  const float* ts = tg + (INVERSE ? 2 : 1) * NLK_NLF_CH * NLK_NLF_ROW;
  for (int k = threadIdx.x; k < nb1; k += NLK_NLF_THREADS) sx[k] = tab[k];
  for (int k = threadIdx.x; k < ch * nb1; k += NLK_NLF_THREADS) {
    const int c = k / nb1, j = k - c * nb1;
    sg[k] = tg[c * NLK_NLF_ROW + j];
    ss[k] = ts[c * NLK_NLF_ROW + j];
  }
  __syncthreads();
  const float top = (float)(nbins - 1);
  const uint64_t stride = (uint64_t)gridDim.x * NLK_NLF_THREADS;
  for (uint64_t i = (uint64_t)blockIdx.x * NLK_NLF_THREADS + threadIdx.x; i < n; i += stride) {
    const int c = i <= 0xffffffffull ? (int)((uint32_t)i % (uint32_t)ch) : (int)(i % (uint64_t)ch);
    const float* G = sg + c * nb1;
    const float* S = ss + c * nb1;
    const float v = in[i];
    int j;
    if (!INVERSE) {
      const float t = fminf(fmaxf((v - lo) * inv_dx, 0.f), top);  // (fmaxf of a NaN and 0 is 0)
      j = (int)floorf(t);
      out[i] = G[j] + (v - sx[j]) * S[j];
    } else {
      j = 0;  // the largest k in 0..nbins-1 with G[k] <= g, k = 0 taken as true: 7 steps cover 127 > 63
#pragma unroll
      for (int step = 64; step; step >>= 1) {
        const int k = j + step;
        if (k < nbins && G[min(k, nbins - 1)] <= v) j = k;  // (the index stays in the row whatever is evaluated)
      }
      out[i] = sx[j] + (v - G[j]) * S[j];
    }
  }
}
