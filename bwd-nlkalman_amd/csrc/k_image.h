// k_image.h — whole-image, HBM-bound kernels outside the frame pipeline: sum of two buffers, colour
// transform, bicubic warp. Compiled in nlk_hip.hip only (plain definitions).
#pragma once
#include "nlk_common.h"

// dst += src (accumulator halo rows received from a neighbouring strip)
__global__ void k_add(float* __restrict__ dst, const float* __restrict__ src, size_t n) {
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
    dst[i] += src[i];
}

// reference: src/nlkalman.c:92-110 (in place, ch == 3)
__global__ void k_rgb2opp(float* __restrict__ im, size_t npix) {
  const float a = 1.f / sqrtf(3.f), b = 1.f / sqrtf(2.f);
  const float c = 2.f * a * sqrtf(2.f);
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < npix;
       i += (size_t)gridDim.x * blockDim.x) {
    float* p = im + 3 * i;
    const float r = p[0], g = p[1], bl = p[2];
    p[0] = a * (r + g + bl);
    p[1] = b * (r - bl);
    p[2] = c * (0.25f * r - 0.5f * g + 0.25f * bl);
  }
}

// reference: src/nlkalman.c:112-130
__global__ void k_opp2rgb(float* __restrict__ im, size_t npix) {
  const float a = 1.f / sqrtf(3.f), b = 1.f / sqrtf(2.f);
  const float c = a / b;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < npix;
       i += (size_t)gridDim.x * blockDim.x) {
    float* p = im + 3 * i;
    const float y = p[0], u = p[1], v = p[2];
    p[0] = a * y + b * u + 0.5f * c * v;
    p[1] = a * y - c * v;
    p[2] = a * y - b * u + 0.5f * c * v;
  }
}

// Keys cubic with the reference's mixed float/double evaluation
// (reference: src/nlkalman.c:36-41)
__device__ inline float nlk_cubic(const float v[4], float x) {
  return (float)(v[1] + 0.5 * x * (v[2] - v[0] +
                 x * (2.0 * v[0] - 5.0 * v[1] + 4.0 * v[2] - v[3] +
                      x * (3.0 * (v[1] - v[2]) + v[3] - v[0]))));
}

// reference: src/nlkalman.c:29-33, 43-88 — one thread per output pixel. The 16 taps are gathered first, all
// channels of a tap together (CH = 3: one 12-byte load per tap instead of three 4-byte ones; CH = 0: any channel
// count, tap by tap), then every channel is interpolated in the reference's order: columns with fy, then the row with fx.
template <int CH>
__global__ void k_warp_bicubic(float* __restrict__ imw, const float* __restrict__ im,
                               const float* __restrict__ of, const float* __restrict__ msk,
                               int w, int h, int ch) {
  const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
  if (x >= w) return;
  const size_t pix = (size_t)x + (size_t)y * w;
  float* o = imw + pix * ch;
  if (msk && msk[pix] != 0.f) {
    for (int c = 0; c < ch; ++c) o[c] = __builtin_nanf("");
    return;
  }
  float xw = x + of[pix * 2 + 0];
  float yw = y + of[pix * 2 + 1];
  xw -= 1;
  yw -= 1;
  const int ix = (int)floorf(xw), iy = (int)floorf(yw);
  const float fx = xw - ix, fy = yw - iy;
  if (CH > 0) {
    float t[4][4][CH > 0 ? CH : 1];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int sx = ix + i, sy = iy + j;
        const bool in = !(sx < 0 || sx >= w || sy < 0 || sy >= h);
        const float* p = im + ((size_t)(in ? sx : 0) + (size_t)(in ? sy : 0) * w) * CH;
#pragma unroll
        for (int c = 0; c < CH; ++c) {
          const float v = p[c];
          t[i][j][c] = in ? v : __builtin_nanf("");
        }
      }
#pragma unroll
    for (int c = 0; c < CH; ++c) {
      float v[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float col[4] = {t[i][0][c], t[i][1][c], t[i][2][c], t[i][3][c]};
        v[i] = nlk_cubic(col, fy);
      }
      o[c] = nlk_cubic(v, fx);
    }
    return;
  }
  for (int c = 0; c < ch; ++c) {
    float v[4];
    for (int i = 0; i < 4; ++i) {
      float col[4];
      for (int j = 0; j < 4; ++j) {
        const int sx = ix + i, sy = iy + j;
        col[j] = (sx < 0 || sx >= w || sy < 0 || sy >= h)
                     ? __builtin_nanf("")
                     : im[((size_t)sx + (size_t)sy * w) * ch + c];
      }
      v[i] = nlk_cubic(col, fy);
    }
    o[c] = nlk_cubic(v, fx);
  }
}
