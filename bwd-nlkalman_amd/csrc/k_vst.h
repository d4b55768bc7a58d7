// k_vst.h — the variance-stabilising transform of nlk_dev_vst_forward / nlk_dev_vst_inverse (include/nlk_hip.h,
// DESIGN.md §9): the generalised Anscombe transform for var(z | y) = a y + b, per channel of an HWC image, with
// one common scale s. One pass, element by element (so in place is fine); NaN passes through.
//   forward   u = a y + u0, u0 = 3 a^2 / 8 + b:  g = 2 s y / (sqrt(u) + sqrt(u0))  for u > 0  (= (2s/a)(sqrt(u) - sqrt(u0)),
//             stable as a -> 0 and s y / sqrt(b) at a = 0), else the value at u = 0, -2 s sqrt(u0) / a
//   inverse   r = max(g / s, -2 sqrt(u0) / a);  y = r sqrt(u0) + a r^2 / 4  (mode 0, the algebraic inverse); mode 1
//             adds the closed-form unbiasing terms a (1/4 + (1/4) sqrt(3/2) / D - (11/8) / D^2 + (5/8) sqrt(3/2) / D^3)
//             with D = max(2 (sqrt(u0) + a r / 2) / a, 2 sqrt(u0) / a) (Makitalo and Foi), nothing for a = 0
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define NLK_VST_THREADS 256
#define NLK_VST_MAX_CH 16

struct NlkVstCoef {                  // per channel, made on the host in double
  float a[NLK_VST_MAX_CH];
  float u0[NLK_VST_MAX_CH];          // 3 a^2 / 8 + b
  float ru0[NLK_VST_MAX_CH];         // sqrt(u0)
  float floor_[NLK_VST_MAX_CH];      // -2 sqrt(u0) / a, the value of g / s at u = 0 (-inf for a = 0)
};

template <bool INVERSE>
__global__ __launch_bounds__(NLK_VST_THREADS) void k_vst(float* out, const float* in, uint64_t n, int ch,
                                                         NlkVstCoef k, float s, int mode) {
  __shared__ float4 kc[NLK_VST_MAX_CH];  // a lane's channel varies: the coefficients are read from LDS
  if ((int)threadIdx.x < ch) kc[threadIdx.x] = make_float4(k.a[threadIdx.x], k.u0[threadIdx.x], k.ru0[threadIdx.x], k.floor_[threadIdx.x]);
  __syncthreads();
  const uint64_t stride = (uint64_t)gridDim.x * NLK_VST_THREADS;
  for (uint64_t i = (uint64_t)blockIdx.x * NLK_VST_THREADS + threadIdx.x; i < n; i += stride) {
    const int c = i <= 0xffffffffull ? (int)((uint32_t)i % (uint32_t)ch) : (int)(i % (uint64_t)ch);
    const float4 kk = kc[c];
    const float a = kk.x, u0 = kk.y, ru0 = kk.z, fl = kk.w;
    const float x = in[i];
    float y;
    if (!INVERSE) {
      const float u = a * x + u0;
      y = u <= 0.f ? s * fl : 2.f * s * x / (sqrtf(u) + ru0);  // (a NaN takes the second branch)
    } else {
      float r = x / s;
      if (r < fl) r = fl;  // (a NaN stays)
      y = r * ru0 + a * r * r * 0.25f;
      if (mode == 1 && a > 0.f) {
        const float d0 = 2.f * ru0 / a;
        float d = 2.f * (ru0 + a * r * 0.5f) / a;
        if (d < d0) d = d0;
        const float id = 1.f / d;
        const float c32 = 1.2247448713915890f;  // sqrt(3/2)
        y += a * (0.25f + id * (0.25f * c32 + id * (-1.375f + id * (0.625f * c32))));
      }
    }
    out[i] = y;
  }
}
