// k_noise.h — the ground-truth loop's noise and error measure (scripts/nlkalman-seq-gt.sh: awgn per frame,
// psnr.sh per output frame), DESIGN.md §9 ("Ground-truth loop").
//
//   k_awgn        out[i] = (float)((double)in[i] + (double)sigma * g_i), i the HWC index, with the reference's
//                 generator (lib/imscript-lite/src/random.c:19-31,50-53,68-75; awgn.c:24-26):
//                   s_{k+1} = A s_k + C (mod 2^64), s_0 = seed; u_k = (double)(s_{k+1} >> 32) / 4294967295.0;
//                   g_i = sqrt(-2 log(u_{2i})) * cos(2 pi u_{2i+1})
//                 A thread takes NLK_AWGN_RUN consecutive samples: it reaches s_{2 i0} by composing the affine
//                 maps s -> A^(2^b) s + C_b of the set bits of 2 i0 (host-made table), then steps on.
//   k_noise_affine  the same deviates g_i scaled per sample: out[i] = (float)((double)in[i] + sqrt(max(a_c in[i] + b_c,
//                 0)) g_i), c = i mod ch: signal-dependent (Poisson-Gaussian) noise for the curve estimator's tests
//   k_sqdiff_*    sum of ((double)a[i] - (double)b[i])^2 in double: a fixed grid of per-workgroup partials
//                 (grid-stride, then an LDS tree), then one workgroup sums the partials in a fixed order. No
//                 atomics: the same inputs give the same bits on every run.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define NLK_AWGN_THREADS 256
#define NLK_AWGN_RUN 8          // consecutive samples per thread
#define NLK_NOISE_MAX_CH 16     // k_noise_affine: channels at most
#define NLK_SQD_THREADS 256
#define NLK_SQD_PER_THREAD 8    // grid size: one workgroup per 256 * 8 samples ...
#define NLK_SQD_MAX_BLOCKS 1024 // ... at most this many (the partials of the final pass)

struct NlkLcgJump {
  uint64_t a[64], c[64];  // s -> a[b] s + c[b]: 2^b steps of the LCG
};

// 2 pi as the reference's (2*M_PI): the product of two exact doubles
#define NLK_AWGN_2PI (2 * 3.14159265358979323846)

__device__ __forceinline__ double awgn_uniform(uint64_t s) { return (double)(uint32_t)(s >> 32) / 4294967295.0; }

// s_{2 i0}: the affine maps of the set bits of k = 2 i0 (below 2^nbits), composed; the bits are uniform in their
// count, per lane in their values
__device__ __forceinline__ uint64_t awgn_seek(const NlkLcgJump& jt, int nbits, uint64_t seed, uint64_t i0) {
  const uint64_t k = 2 * i0;
  uint64_t A = 1, Cc = 0;
  for (int b = 0; b < nbits; ++b)
    if ((k >> b) & 1) {
      Cc = jt.a[b] * Cc + jt.c[b];
      A = jt.a[b] * A;
    }
  return A * seed + Cc;
}

// the next normal deviate: two steps of the LCG from s, the Box-Muller cosine branch in the reference's order
__device__ __forceinline__ double awgn_normal(uint64_t& s, uint64_t a1, uint64_t c1) {
#pragma clang fp contract(off)
  s = a1 * s + c1;
  const double x1 = awgn_uniform(s);
  s = a1 * s + c1;
  const double x2 = awgn_uniform(s);
  return sqrt((-2.0) * log(x1)) * cos(NLK_AWGN_2PI * x2);
}

__global__ __launch_bounds__(NLK_AWGN_THREADS) void k_awgn(float* out, const float* in, uint64_t n, float sigma,
                                                           uint64_t seed, NlkLcgJump jt, int nbits) {
  // one rounding per operation, as the reference's -ffp-contract=off build: no fma for sigma * g + x
#pragma clang fp contract(off)
  const uint64_t i0 = ((uint64_t)blockIdx.x * NLK_AWGN_THREADS + threadIdx.x) * NLK_AWGN_RUN;
  if (i0 >= n) return;
  uint64_t s = awgn_seek(jt, nbits, seed, i0);
  const uint64_t a1 = jt.a[0], c1 = jt.c[0];
  const double s2 = (double)sigma;
  const uint64_t end = i0 + NLK_AWGN_RUN < n ? i0 + NLK_AWGN_RUN : n;
  for (uint64_t i = i0; i < end; ++i) {
    const double y = awgn_normal(s, a1, c1);
    out[i] = (float)((double)in[i] + s2 * y);
  }
}

// k_awgn with the deviation of sample i = sqrt(max(a_c in[i] + b_c, 0)), c = i mod ch: the same deviates g_i
struct NlkNoiseAb {
  float a[NLK_NOISE_MAX_CH], b[NLK_NOISE_MAX_CH];
};

__global__ __launch_bounds__(NLK_AWGN_THREADS) void k_noise_affine(float* out, const float* in, uint64_t n, int ch,
                                                                   NlkNoiseAb ab, uint64_t seed, NlkLcgJump jt,
                                                                   int nbits) {
#pragma clang fp contract(off)
  __shared__ double la[NLK_NOISE_MAX_CH], lb[NLK_NOISE_MAX_CH];
  if ((int)threadIdx.x < ch) {
    la[threadIdx.x] = (double)ab.a[threadIdx.x];
    lb[threadIdx.x] = (double)ab.b[threadIdx.x];
  }
  __syncthreads();
  const uint64_t i0 = ((uint64_t)blockIdx.x * NLK_AWGN_THREADS + threadIdx.x) * NLK_AWGN_RUN;
  if (i0 >= n) return;
  uint64_t s = awgn_seek(jt, nbits, seed, i0);
  const uint64_t a1 = jt.a[0], c1 = jt.c[0];
  const uint64_t end = i0 + NLK_AWGN_RUN < n ? i0 + NLK_AWGN_RUN : n;
  int c = (int)(i0 % (uint64_t)ch);
  for (uint64_t i = i0; i < end; ++i) {
    const double y = awgn_normal(s, a1, c1);
    const double x = (double)in[i];
    const double var = la[c] * x + lb[c];
    out[i] = (float)(x + sqrt(var > 0.0 ? var : 0.0) * y);  // (a NaN sample stays NaN through x)
    if (++c == ch) c = 0;
  }
}

// LDS tree over the NLK_SQD_THREADS values of a workgroup, fixed pairing; the result is in v[0]
__device__ __forceinline__ void sqd_tree(double* v) {
#pragma unroll
  for (int half = NLK_SQD_THREADS / 2; half > 0; half >>= 1) {
    __syncthreads();
    if ((int)threadIdx.x < half) v[threadIdx.x] += v[threadIdx.x + half];
  }
  __syncthreads();
}

__global__ __launch_bounds__(NLK_SQD_THREADS) void k_sqdiff_partial(double* part, const float* a, const float* b,
                                                                    uint64_t n) {
#pragma clang fp contract(off)
  __shared__ double v[NLK_SQD_THREADS];
  const uint64_t stride = (uint64_t)gridDim.x * NLK_SQD_THREADS;
  double acc = 0.0;
#pragma unroll 4
  for (uint64_t i = (uint64_t)blockIdx.x * NLK_SQD_THREADS + threadIdx.x; i < n; i += stride) {
    const double d = (double)a[i] - (double)b[i];
    acc += d * d;
  }
  v[threadIdx.x] = acc;
  sqd_tree(v);
  if (threadIdx.x == 0) part[blockIdx.x] = v[0];
}

// one workgroup: *sum = the npart partials, thread t summing t, t + 256, ... in order, then the tree
__global__ __launch_bounds__(NLK_SQD_THREADS) void k_sqdiff_final(double* sum, const double* part, int npart) {
  __shared__ double v[NLK_SQD_THREADS];
  double acc = 0.0;
  for (int i = threadIdx.x; i < npart; i += NLK_SQD_THREADS) acc += part[i];
  v[threadIdx.x] = acc;
  sqd_tree(v);
  if (threadIdx.x == 0) *sum = v[0];
}
