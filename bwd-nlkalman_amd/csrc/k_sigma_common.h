// k_sigma_common.h — what the noise-level estimator (k_sigma.h) and the noise-curve estimator (k_sigma_curve.h)
// share: the launch shapes, the selection state, the LDS tile of the keys pass and the DCT basis of the sums pass.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "k_dct8.h"

#define NLK_SIG_THREADS 256
#define NLK_SIG_TBX 32             // k_sigma_keys: blocks per workgroup, across ...
#define NLK_SIG_TBY 8              // ... and down
#define NLK_SIG_LDS_MAX (48 << 10) // the tile is staged in LDS where it fits in this many bytes (step <= 6)
#define NLK_SIG_SKIP 0xffffffffu   // key of a skipped block
#define NLK_SIG_MAX_GROUPS 256     // k_sigma_hist / k_sigma_sums: workgroups per channel at most
#define NLK_SIG_SUM_THREADS 1024   // k_sigma_sums: 16 wavefronts, so that each walks a short run of keys
#define NLK_SIG_AHEAD 4            // k_sigma_sums: selected blocks whose samples are loaded together

struct NlkSigState {  // per channel, between the kernels of pass 2
  uint32_t prefix;    // the digits of the K-th key found so far (after the last pick: the key itself)
  int krem;           // its rank among the keys that share them, from 1; 0: the channel has no block
  int nblocks, k;     // N_c, K
};

// the LDS tile of a workgroup of k_sigma_keys: its size in pixels and its row pitch
__host__ __device__ inline int nlk_sig_tile_w(int step) { return (NLK_SIG_TBX - 1) * step + 8; }
__host__ __device__ inline int nlk_sig_tile_h(int step) { return (NLK_SIG_TBY - 1) * step + 8; }
__host__ __device__ inline int nlk_sig_pitch(int step) { return nlk_sig_tile_w(step) | 1; }  // odd: no bank is favoured

// (1/2) cos(pi (2k + 1) i / 16), sqrt(1/8) for i = 0: the constants of k_dct8.h
__device__ __forceinline__ float sigma_basis(int i, int k) {
  using namespace nlk_d8;
  if (i == 0) return S0;
  int m = ((2 * k + 1) * i) & 31;
  if (m > 16) m = 32 - m;
  const bool neg = m > 8;
  if (neg) m = 16 - m;
  const float v = m == 1 ? E1 : m == 2 ? C1 : m == 3 ? E3 : m == 4 ? S0 : m == 5 ? E5 : m == 6 ? C3 : m == 7 ? E7 : 0.f;
  return neg ? -v : v;
}
