// k_sure.h — Monte-Carlo SURE (include/nlk_hip.h: nlk_dev_probe_add, nlk_dev_sure_terms; DESIGN.md §9, "Error
// estimate without clean frames"): the two sums of Stein's unbiased risk estimate with the divergence taken by one
// probe of independent signs (Ramani, Blu, Unser 2008).
//
//   sure_minus     b_i of sample i (the HWC index) from a 64-bit seed: one splitmix64 output per sample, its top bit.
//                  Nothing is stored: the probe and the sums recompute it.
//   k_probe_add    out[i] = in[i] + (b_i > 0 ? eps : -eps): one float add. Four consecutive samples per thread, as one
//                  16-byte access where both pointers allow it.
//   k_sure_blocks  one wavefront per block x block tile, NLK_SURE_WAVES tiles per workgroup: lane l takes the tile's
//                  positions l, l + 64, ... (row-major in the tile, so a wavefront reads 64 / block whole tile rows at
//                  a time), adds R_c += (y - f)^2 and D_c += b (fp - f) in double per channel, then a fixed cross-lane
//                  tree (offsets 32, 16, ... 1) leaves the tile's sums in lane 0, which stores them: [tile][ch][2].
//                  CH = 1 and 3 keep the accumulators of every channel in registers and read a position once; CH = 0
//                  is any channel count, one pass over the tile per channel (no dynamically indexed registers).
//                  A position outside the image contributes nothing, by selection.
//   k_sure_final   one workgroup of 1024 threads: thread t adds every span-th double of the tiles' array from t on (span =
//                  the largest multiple of 2 ch within 1024, so a thread stays with one (channel, term)), then an LDS tree
//                  over the threads of a (channel, term): total[2 c] = R_c, total[2 c + 1] = D_c.
// No atomics: every order of summation depends on (w, h, ch, block) alone.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define NLK_SURE_THREADS 256
#define NLK_SURE_WAVES 4  // tiles per workgroup of k_sure_blocks
#define NLK_SURE_FINAL_THREADS 1024
#define NLK_SURE_MAX_CH 16
#define NLK_SURE_MIN_BLOCK 4
#define NLK_SURE_MAX_BLOCK 64
#define NLK_PROBE_THREADS 256
#define NLK_PROBE_RUN 4   // consecutive samples per thread

static_assert(NLK_SURE_THREADS == 64 * NLK_SURE_WAVES, "one wavefront per tile");

// true: b_i = -1
__device__ __forceinline__ bool sure_minus(uint64_t seed, uint64_t i) {
  uint64_t z = seed + (i + 1) * 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  z ^= z >> 31;
  return (z >> 63) != 0;
}

template <bool VEC>
__global__ __launch_bounds__(NLK_PROBE_THREADS) void k_probe_add(float* out, const float* in, uint64_t n, float eps,
                                                                 uint64_t seed) {
  const uint64_t i0 = ((uint64_t)blockIdx.x * NLK_PROBE_THREADS + threadIdx.x) * NLK_PROBE_RUN;
  if (i0 >= n) return;
  if (VEC && i0 + NLK_PROBE_RUN <= n) {
    float4 v = *reinterpret_cast<const float4*>(in + i0);
    v.x += sure_minus(seed, i0) ? -eps : eps;
    v.y += sure_minus(seed, i0 + 1) ? -eps : eps;
    v.z += sure_minus(seed, i0 + 2) ? -eps : eps;
    v.w += sure_minus(seed, i0 + 3) ? -eps : eps;
    *reinterpret_cast<float4*>(out + i0) = v;
    return;
  }
  const uint64_t end = i0 + NLK_PROBE_RUN < n ? i0 + NLK_PROBE_RUN : n;
  for (uint64_t i = i0; i < end; ++i) out[i] = in[i] + (sure_minus(seed, i) ? -eps : eps);
}

// the sum of v over the 64 lanes of a wavefront in lane 0, fixed pairing
__device__ __forceinline__ double sure_wave_sum(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  return v;
}

// grid: ceil(nbx * nby / NLK_SURE_WAVES); blocks [nby][nbx][ch][2]
template <int CH>
__global__ __launch_bounds__(NLK_SURE_THREADS) void k_sure_blocks(double* blocks, const float* y, const float* f,
                                                                  const float* fp, int w, int h, int ch, int block,
                                                                  int nbx, int ntiles, uint64_t seed) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x & 63;
  const int tile = blockIdx.x * NLK_SURE_WAVES + (threadIdx.x >> 6);  // uniform in the wavefront
  if (tile >= ntiles) return;
  const int by = tile / nbx, bx = tile - by * nbx;
  const int x0 = bx * block, y0 = by * block, npos = block * block;
  double* out = blocks + (size_t)tile * ch * 2;
  if constexpr (CH > 0) {
    double R[CH], D[CH];
#pragma unroll
    for (int c = 0; c < CH; ++c) R[c] = D[c] = 0.0;
#pragma unroll 4
    for (int p = lane; p < npos; p += 64) {
      const int py = p / block, px = p - py * block;
      if (x0 + px < w && y0 + py < h) {
        const uint64_t at = ((uint64_t)(y0 + py) * w + (x0 + px)) * CH;
#pragma unroll
        for (int c = 0; c < CH; ++c) {
          const double vf = (double)f[at + c];
          const double r = (double)y[at + c] - vf, d = (double)fp[at + c] - vf;
          R[c] += r * r;
          D[c] += sure_minus(seed, at + c) ? -d : d;
        }
      }
    }
#pragma unroll
    for (int c = 0; c < CH; ++c) {
      const double r = sure_wave_sum(R[c]), d = sure_wave_sum(D[c]);
      if (lane == 0) {
        out[2 * c] = r;
        out[2 * c + 1] = d;
      }
    }
  } else {
    for (int c = 0; c < ch; ++c) {
      double R = 0.0, D = 0.0;
      for (int p = lane; p < npos; p += 64) {
        const int py = p / block, px = p - py * block;
        if (x0 + px < w && y0 + py < h) {
          const uint64_t at = ((uint64_t)(y0 + py) * w + (x0 + px)) * ch + c;
          const double vf = (double)f[at];
          const double r = (double)y[at] - vf, d = (double)fp[at] - vf;
          R += r * r;
          D += sure_minus(seed, at) ? -d : d;
        }
      }
      R = sure_wave_sum(R);
      D = sure_wave_sum(D);
      if (lane == 0) {
        out[2 * c] = R;
        out[2 * c + 1] = D;
      }
    }
  }
}

// one workgroup: total[j] = the sum over the tiles of blocks[tile][j], j < nval = 2 ch <= 32. The array is read flat, in
// rows of `span` = the largest multiple of nval within the workgroup: thread t < span keeps the value j = t % nval through
// every row (coalesced, eight independent loads in flight), then the span / nval threads of a value are added by a tree
// with fixed pairing.
__global__ __launch_bounds__(NLK_SURE_FINAL_THREADS) void k_sure_final(double* total, const double* blocks, int ntiles,
                                                                       int nval) {
  __shared__ double v[NLK_SURE_FINAL_THREADS];
  const int t = threadIdx.x, groups = NLK_SURE_FINAL_THREADS / nval, span = groups * nval;
  const size_t n = (size_t)ntiles * nval;
  double acc = 0.0;
  if (t < span) {
    size_t e = t;
    for (; e + (size_t)7 * span < n; e += (size_t)8 * span) {
      double x[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) x[k] = blocks[e + (size_t)k * span];
#pragma unroll
      for (int k = 0; k < 8; ++k) acc += x[k];
    }
    for (; e < n; e += span) acc += blocks[e];
  }
  v[t] = acc;
  int half = 1;
  while (half < groups) half <<= 1;
  for (half >>= 1; half > 0; half >>= 1) {
    __syncthreads();
    const int g = t / nval;
    if (t < span && g < half && g + half < groups) v[t] += v[t + half * nval];
  }
  __syncthreads();
  if (t < nval) total[t] = v[t];
}
