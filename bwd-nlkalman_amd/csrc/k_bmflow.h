// k_bmflow.h — the block-matching optical flow (nlk_dev_bm_flow, include/nlk_hip.h; stated once, in numpy, by
// tests/bmflow_ref.py, whose header holds the algorithm). The kernels give that restatement's bits: float32, every
// operation rounded by itself, sums in the written order. No atomics, nothing depends on the launch order.
//
// Per pyramid level, from the coarsest to the finest matched one:
//   k_bm_match   one wavefront per 8 x 8 block, four blocks of a block row per workgroup. The block's prediction is read
//                straight from the coarser level's (median-filtered) block vectors: the dense flow of that level and its
//                x2 upsampling are evaluated at the one pixel that is asked for (bm_dense_at, bm_up2_at), never stored.
//                The wave stages T (64 floats) and the window of I1 that its candidates cover, coordinates clamped, in
//                its own LDS slice: neighbouring blocks predict different vectors, so their windows are not one
//                rectangle, and the overlap is served by L2. One lane per candidate (dy, dx) of [-(R+1), R+1]^2, a second
//                round for the 17 candidates beyond 64 at R = 3; a lane sums its 64 terms in order from LDS. The window's
//                row stride is 32 + (2R + 3): lane c reads word base + c, so the 32 lanes that are served together sit
//                on 32 banks. The winner is a wavefront reduction on (cost, raster index) over the inner [-R, R]^2; the
//                parabola's neighbours are read from the lanes that hold them.
//   k_bm_median  3 x 3 median of the block vectors, per component, edges replicated: by rank, so no input (a NaN
//                included) leaves anything unset.
// then one launch gives the flow: k_bm_dense at the level itself (fscale = 0), or k_bm_up2_dense, the x2 upsampling of
// the dense flow without storing it; k_bm_up2 for every further level down to 0.
// Every index is clamped after its conversion from float, so no input makes a kernel read outside an array; what
// non-finite images give is unspecified.
#pragma once
#include <hip/hip_runtime.h>

// a (u, v) pair that only promises the alignment of a float (k_flowinv.h's)
typedef float nlk_flow_f2 __attribute__((ext_vector_type(2), aligned(4)));

#pragma clang fp contract(off)

#define NLK_BM_BLOCK 8
#define NLK_BM_STRIDE 4
#define NLK_BM_WAVES 4  // blocks (wavefronts) of a matcher workgroup

struct NlkBmLevel {
  int w, h;      // pixels
  int nbx, nby;  // blocks
};

__host__ __device__ __forceinline__ int nlk_bm_blocks(int n) { return (n - NLK_BM_BLOCK + NLK_BM_STRIDE - 1) / NLK_BM_STRIDE + 1; }
__device__ __forceinline__ int bm_origin(int i, int n) { return NLK_BM_STRIDE * i < n - NLK_BM_BLOCK ? NLK_BM_STRIDE * i : n - NLK_BM_BLOCK; }
__device__ __forceinline__ int bm_clamp(int i, int lo, int hi) { return i < lo ? lo : (i > hi ? hi : i); }

// ---- the box pyramid: level l + 1 of both images in one launch (blockIdx.z = the image)
__global__ __launch_bounds__(256) void k_bm_down(float* __restrict__ d0, float* __restrict__ d1, const float* __restrict__ s0,
                                                 const float* __restrict__ s1, int ws, int wd, int hd) {
  const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
  if (x >= wd || y >= hd) return;
  const float* s = (blockIdx.z ? s1 : s0) + (size_t)(2 * y) * ws + 2 * x;
  const nlk_flow_f2 a = *reinterpret_cast<const nlk_flow_f2*>(s), b = *reinterpret_cast<const nlk_flow_f2*>(s + ws);
  (blockIdx.z ? d1 : d0)[(size_t)y * wd + x] = ((a.x + a.y) + (b.x + b.y)) * 0.25f;
}

// ---- the dense flow of a level at one pixel: bilinear between the block centres
struct BmAxis { int k0, k1; float t; };
__device__ __forceinline__ BmAxis bm_axis(int q, int n, int nb) {
  if (nb < 2) return BmAxis{0, 0, 0.f};
  int k = q < 4 ? 0 : (q - 4) >> 2;
  if (k > nb - 2) k = nb - 2;
  const float c0 = (float)bm_origin(k, n) + 3.5f, c1 = (float)bm_origin(k + 1, n) + 3.5f;
  const float t = ((float)q - c0) / (c1 - c0);
  return BmAxis{k, k + 1, fminf(fmaxf(t, 0.f), 1.f)};
}
__device__ __forceinline__ nlk_flow_f2 bm_lerp2(nlk_flow_f2 a00, nlk_flow_f2 a01, nlk_flow_f2 a10, nlk_flow_f2 a11, float fx,
                                                float fy) {
  const float tu = a00.x + fx * (a01.x - a00.x), bu = a10.x + fx * (a11.x - a10.x);
  const float tv = a00.y + fx * (a01.y - a00.y), bv = a10.y + fx * (a11.y - a10.y);
  return nlk_flow_f2{tu + fy * (bu - tu), tv + fy * (bv - tv)};
}
struct BmDense {  // the dense flow of a level, from its block vectors
  const nlk_flow_f2* V;
  NlkBmLevel g;
  __device__ __forceinline__ nlk_flow_f2 operator()(int x, int y) const {
    const BmAxis ax = bm_axis(x, g.w, g.nbx), ay = bm_axis(y, g.h, g.nby);
    const nlk_flow_f2* r0 = V + (size_t)ay.k0 * g.nbx;
    const nlk_flow_f2* r1 = V + (size_t)ay.k1 * g.nbx;
    return bm_lerp2(r0[ax.k0], r0[ax.k1], r1[ax.k0], r1[ax.k1], ax.t, ay.t);
  }
};
struct BmStored {  // a stored flow
  const nlk_flow_f2* F;
  int w;
  __device__ __forceinline__ nlk_flow_f2 operator()(int x, int y) const { return F[(size_t)y * w + x]; }
};
// twice the flow `src` of a ws x hs level at the pixel (x, y) of the next finer level
template <class Src>
__device__ __forceinline__ nlk_flow_f2 bm_up2_at(const Src& src, int ws, int hs, int x, int y) {
  const float X = fminf(fmaxf(((float)x - 0.5f) * 0.5f, 0.f), (float)(ws - 1));
  const float Y = fminf(fmaxf(((float)y - 0.5f) * 0.5f, 0.f), (float)(hs - 1));
  const int x0 = bm_clamp((int)floorf(X), 0, ws - 1), y0 = bm_clamp((int)floorf(Y), 0, hs - 1);
  const int x1 = x0 + 1 < ws ? x0 + 1 : ws - 1, y1 = y0 + 1 < hs ? y0 + 1 : hs - 1;
  const nlk_flow_f2 v = bm_lerp2(src(x0, y0), src(x1, y0), src(x0, y1), src(x1, y1), X - (float)x0, Y - (float)y0);
  return nlk_flow_f2{v.x * 2.f, v.y * 2.f};
}

// ---- the matcher. V: this level's block vectors (out); Vc: the coarser level's, median-filtered (NULL: prediction 0)
__device__ __forceinline__ float bm_subpel(float cm, float c0, float cp) {
  const float den = (cm - 2.f * c0) + cp;
  if (!(den > 0.f)) return 0.f;
  return fminf(fmaxf((0.5f * (cm - cp)) / den, -0.5f), 0.5f);
}

template <int R>
__global__ __launch_bounds__(64 * NLK_BM_WAVES) void k_bm_match(nlk_flow_f2* __restrict__ V, const float* __restrict__ I0,
                                                                const float* __restrict__ I1, NlkBmLevel g,
                                                                const nlk_flow_f2* __restrict__ Vc, NlkBmLevel gc) {
  constexpr int S = 2 * R + 3, NC = S * S, WS = NLK_BM_BLOCK + 2 * (R + 1), LS = 32 + S, ROUNDS = (NC + 63) / 64;
  __shared__ float sW[NLK_BM_WAVES][WS * LS];
  __shared__ __attribute__((aligned(16))) float sT[NLK_BM_WAVES][64];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int by = blockIdx.y;
  int bx = blockIdx.x * NLK_BM_WAVES + wave;
  const bool live = bx < g.nbx;  // (the same in every lane of a wave)
  if (!live) bx = g.nbx - 1;
  const int ox = bm_origin(bx, g.w), oy = bm_origin(by, g.h);
  int px = 0, py = 0;
  if (Vc) {
    const nlk_flow_f2 p = bm_up2_at(BmDense{Vc, gc}, gc.w, gc.h, ox + 4, oy + 4);
    const int lim = g.w + g.h;
    px = bm_clamp((int)rintf(p.x), -lim, lim);
    py = bm_clamp((int)rintf(p.y), -lim, lim);
  }
  float* W = sW[wave];
  float* T = sT[wave];
  T[lane] = I0[(size_t)(oy + (lane >> 3)) * g.w + ox + (lane & 7)];
  for (int i = lane; i < WS * WS; i += 64) {
    const int wr = i / WS, wc = i % WS;
    const int yy = bm_clamp(oy + py + wr - (R + 1), 0, g.h - 1), xx = bm_clamp(ox + px + wc - (R + 1), 0, g.w - 1);
    W[wr * LS + wc] = I1[(size_t)yy * g.w + xx];
  }
  __syncthreads();
  float cst[ROUNDS];
  float bc = __builtin_inff();
  int bi = 0x7fffffff;
#pragma unroll
  for (int rd = 0; rd < ROUNDS; ++rd) {
    const int c = lane + 64 * rd, cc = c < NC ? c : 0;
    const int dy = cc / S, dx = cc % S;
    const float* wp = W + dy * LS + dx;
    float cost = 0.f;
#pragma unroll
    for (int r = 0; r < NLK_BM_BLOCK; ++r)
#pragma unroll
      for (int k = 0; k < NLK_BM_BLOCK; ++k) {
        const float d = T[r * NLK_BM_BLOCK + k] - wp[r * LS + k];
        cost = cost + d * d;
      }
    cst[rd] = cost;
    const bool inner = c < NC && dy >= 1 && dy <= S - 2 && dx >= 1 && dx <= S - 2;
    if (inner && (cost < bc || (cost == bc && c < bi))) { bc = cost; bi = c; }
  }
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    const float oc = __shfl_xor(bc, m);
    const int oi = __shfl_xor(bi, m);
    if (oc < bc || (oc == bc && oi < bi)) { bc = oc; bi = oi; }
  }
  bi = __shfl(bi, 0);
  if (bi < 0 || bi >= NC) bi = (R + 1) * S + (R + 1);  // (only a NaN cost gets here)
  const int wy = bi / S, wx = bi % S;                  // both in 1 .. S - 2
  float nb[5];                                         // the costs of the winner and of its four neighbours
  const int at[5] = {bi, bi - 1, bi + 1, bi - S, bi + S};
#pragma unroll
  for (int j = 0; j < 5; ++j) {
    float v = __shfl(cst[0], at[j] & 63);
    if (ROUNDS > 1) {
      const float v1 = __shfl(cst[ROUNDS - 1], at[j] & 63);
      if (at[j] >= 64) v = v1;
    }
    nb[j] = v;
  }
  if (live && lane == 0)
    V[(size_t)by * g.nbx + bx] = nlk_flow_f2{(float)(px + wx - (R + 1)) + bm_subpel(nb[1], nb[0], nb[2]),
                                             (float)(py + wy - (R + 1)) + bm_subpel(nb[3], nb[0], nb[4])};
}

// ---- 3 x 3 median of the block vectors, per component, edges replicated: the value with at most 4 smaller ones and
// more than 4 that are not larger
__device__ __forceinline__ float bm_median9(const float* v) {
  float med = v[4];
#pragma unroll
  for (int i = 0; i < 9; ++i) {
    int less = 0, leq = 0;
#pragma unroll
    for (int j = 0; j < 9; ++j) {
      less += v[j] < v[i];
      leq += v[j] <= v[i];
    }
    if (less <= 4 && leq > 4) med = v[i];
  }
  return med;
}
__global__ __launch_bounds__(256) void k_bm_median(nlk_flow_f2* __restrict__ M, const nlk_flow_f2* __restrict__ V, int nbx,
                                                   int nby) {
  const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
  if (x >= nbx || y >= nby) return;
  float u[9], v[9];
#pragma unroll
  for (int j = 0; j < 3; ++j)
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      const nlk_flow_f2 a = V[(size_t)bm_clamp(y + j - 1, 0, nby - 1) * nbx + bm_clamp(x + i - 1, 0, nbx - 1)];
      u[3 * j + i] = a.x;
      v[3 * j + i] = a.y;
    }
  M[(size_t)y * nbx + x] = nlk_flow_f2{bm_median9(u), bm_median9(v)};
}

// ---- the flow from the block vectors of the finest matched level: at that level, or one level finer
__global__ __launch_bounds__(256) void k_bm_dense(nlk_flow_f2* __restrict__ F, const nlk_flow_f2* __restrict__ M, NlkBmLevel g) {
  const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
  if (x >= g.w || y >= g.h) return;
  F[(size_t)y * g.w + x] = BmDense{M, g}(x, y);
}
__global__ __launch_bounds__(256) void k_bm_up2_dense(nlk_flow_f2* __restrict__ F, int w, int h, const nlk_flow_f2* __restrict__ M,
                                                      NlkBmLevel g) {
  const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
  if (x >= w || y >= h) return;
  F[(size_t)y * w + x] = bm_up2_at(BmDense{M, g}, g.w, g.h, x, y);
}
// ---- x2 upsampling of a stored ws x hs flow to w x h
__global__ __launch_bounds__(256) void k_bm_up2(nlk_flow_f2* __restrict__ F, int w, int h, const nlk_flow_f2* __restrict__ src,
                                                int ws, int hs) {
  const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
  if (x >= w || y >= h) return;
  F[(size_t)y * w + x] = bm_up2_at(BmStored{src, ws}, ws, hs, x, y);
}
