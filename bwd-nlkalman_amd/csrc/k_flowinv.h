// k_flowinv.h — the inverse of a dense flow by fixed-point steps (nlk_dev_flow_invert, include/nlk_hip.h; restated in
// numpy by tests/flowinv_ref.py). B is the backward flow of the recursion (I1(q + B(q)) ~ I0(q)); its inverse F
// satisfies F(q) = -B(q + F(q)), and F_0 = -B, F_{k+1}(q) = -B~(q + F_k(q)) contracts to it where the slope of B is
// below 1.
//
// B~, the bilinear interpolation of B at (x + F.u, y + F.v), in the order written, every operation rounded by itself:
//   X = fminf(fmaxf(x + F.u, 0), w - 1)          Y likewise with h - 1
//   x0 = (int)floorf(X), clamped to 0 .. w - 1;  x1 = min(x0 + 1, w - 1);  fx = X - x0        the same in y
//   per component: top = B00 + fx (B01 - B00), bot = B10 + fx (B11 - B10), val = top + fy (bot - top)
//   F = -val
// The integer indices are clamped after the conversion, so no input (a NaN or an infinity included) makes the kernel
// read outside the array; what a non-finite B gives is unspecified at the pixels whose steps read it, and only there.
//
// One thread per pixel; the steps of a pixel read only B, so they run in registers. B(q) and the result are coalesced
// 8-byte accesses; the four gathers of a step land within |F| pixels of q and are served by L2. No LDS, no atomics.
#pragma once
#include <hip/hip_runtime.h>

#pragma clang fp contract(off)

#define NLK_FLOWINV_BX 64  // threads of a workgroup along x (one wavefront per row piece) ...
#define NLK_FLOWINV_BY 4   // ... and along y

// a (u, v) pair that only promises the alignment of a float
typedef float nlk_flow_f2 __attribute__((ext_vector_type(2), aligned(4)));

__device__ __forceinline__ int nlk_flowinv_clamp(int i, int n) { return i < 0 ? 0 : (i > n - 1 ? n - 1 : i); }

__global__ __launch_bounds__(NLK_FLOWINV_BX * NLK_FLOWINV_BY) void k_flow_invert(nlk_flow_f2* __restrict__ inv,
                                                                                 const nlk_flow_f2* __restrict__ B, int w,
                                                                                 int h, int iters) {
  const int x = blockIdx.x * NLK_FLOWINV_BX + threadIdx.x, y = blockIdx.y * NLK_FLOWINV_BY + threadIdx.y;
  if (x >= w || y >= h) return;
  const size_t at = (size_t)y * w + x;
  const nlk_flow_f2 b = B[at];
  float fu = -b.x, fv = -b.y;
  const float xf = (float)x, yf = (float)y, xmax = (float)(w - 1), ymax = (float)(h - 1);
  for (int k = 0; k < iters; ++k) {
    const float X = fminf(fmaxf(xf + fu, 0.f), xmax), Y = fminf(fmaxf(yf + fv, 0.f), ymax);
    const int x0 = nlk_flowinv_clamp((int)floorf(X), w), y0 = nlk_flowinv_clamp((int)floorf(Y), h);
    const int x1 = x0 + 1 < w ? x0 + 1 : w - 1, y1 = y0 + 1 < h ? y0 + 1 : h - 1;
    const float fx = X - (float)x0, fy = Y - (float)y0;
    const nlk_flow_f2 b00 = B[(size_t)y0 * w + x0], b01 = B[(size_t)y0 * w + x1];
    const nlk_flow_f2 b10 = B[(size_t)y1 * w + x0], b11 = B[(size_t)y1 * w + x1];
    const float tu = b00.x + fx * (b01.x - b00.x), bu = b10.x + fx * (b11.x - b10.x);
    const float tv = b00.y + fx * (b01.y - b00.y), bv = b10.y + fx * (b11.y - b10.y);
    fu = -(tu + fy * (bu - tu));
    fv = -(tv + fy * (bv - tv));
  }
  inv[at] = nlk_flow_f2{fu, fv};
}
