// k_sigma.h — the noise-level estimator of nlk_dev_estimate_sigma (include/nlk_hip.h): per channel,
// the 8 x 8 blocks on a grid of `step`, their orthonormal DCT Y, the low-frequency energy L of each, the K-th
// smallest L found exactly, and the median over the high-frequency coefficients of the mean of Y[i][j]^2 over the
// blocks with L <= that value.
//
//   k_sigma_keys   pass 1, one lane per block: the block from an LDS tile of the channel (or, where the tile of a
//                  large step does not fit, straight from the image), 8 row + 8 column transforms on registers
//                  (k_dct8.h), L as a 32-bit key (the bits of a non-negative float order as the float does;
//                  NLK_SIG_SKIP for a block holding a non-finite sample) and the histogram of the keys' top byte
//   k_sigma_pick   pass 2, one workgroup per channel: the digit of the K-th key in the current histogram; the first
//   k_sigma_hist   call also counts the blocks and fixes K. k_sigma_hist makes the next histogram, of the keys that
//                  share the digits found so far. Integer atomics in LDS and HBM: their sums do not depend on order.
//   k_sigma_sums   pass 3: a wavefront walks its share of the keys in order and transforms each selected block
//                  again, lane (i, j) holding Y[i][j] and adding its square to one double. The shares are a function
//                  of the sizes alone, so are the per-workgroup partials ...
//   k_sigma_final  ... which one workgroup adds in order; then lane (i, j) ranks its mean among the high-frequency
//                  ones, the two middle ranks give the median, and the square roots are written.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "k_sigma_common.h"

template <bool STAGED>
__global__ __launch_bounds__(NLK_SIG_THREADS) void k_sigma_keys(uint32_t* keys, uint32_t* hist0, const float* img,
                                                                int w, int h, int ch, int step, int nbx, int nby,
                                                                int low_max) {
  extern __shared__ float tile[];
  __shared__ uint32_t lh[256];
  const int tid = threadIdx.x, c = blockIdx.z;
  const int tx = tid % NLK_SIG_TBX, ty = tid / NLK_SIG_TBX;
  const int bx = blockIdx.x * NLK_SIG_TBX + tx, by = blockIdx.y * NLK_SIG_TBY + ty;
  const int x0 = blockIdx.x * NLK_SIG_TBX * step, y0 = blockIdx.y * NLK_SIG_TBY * step;
  const int pitch = STAGED ? nlk_sig_pitch(step) : 0;
  lh[tid] = 0;
  if (STAGED) {
    const int tw = nlk_sig_tile_w(step), th = nlk_sig_tile_h(step);
    for (int i = tid; i < tw * th; i += NLK_SIG_THREADS) {
      const int yy = i / tw, xx = i - yy * tw;
      const int gx = x0 + xx, gy = y0 + yy;
      tile[yy * pitch + xx] = gx < w && gy < h ? img[((size_t)gy * w + gx) * ch + c] : 0.f;
    }
  }
  __syncthreads();
  const bool live = bx < nbx && by < nby;  // (a live block lies inside the image: bx * step <= w - 8)
  if (live) {
    float b[8][8];
    bool finite = true;
#pragma unroll
    for (int r = 0; r < 8; ++r)
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        b[r][k] = STAGED ? tile[(ty * step + r) * pitch + tx * step + k]
                         : img[((size_t)(by * step + r) * w + (bx * step + k)) * ch + c];
        finite = finite && fabsf(b[r][k]) <= 3.402823466e38f;  // false for NaN and the infinities
      }
    uint32_t key = NLK_SIG_SKIP;
    if (finite) {
#pragma unroll
      for (int r = 0; r < 8; ++r) nlk_dct8_fast_fwd(b[r]);
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        float col[8];
#pragma unroll
        for (int r = 0; r < 8; ++r) col[r] = b[r][k];
        nlk_dct8_fast_fwd(col);
#pragma unroll
        for (int r = 0; r < 8; ++r) b[r][k] = col[r];
      }
      float low = 0.f;
#pragma unroll
      for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int j = 0; j < 8; ++j)
          if (i + j >= 1 && i + j <= low_max) low = __builtin_fmaf(b[i][j], b[i][j], low);
      key = __float_as_uint(low);  // low >= +0: the bits order as the values
      if (key == NLK_SIG_SKIP) key = NLK_SIG_SKIP - 1;  // (a NaN of huge samples that happens to have these bits)
      atomicAdd(&lh[key >> 24], 1u);
    }
    keys[((size_t)c * nby + by) * nbx + bx] = key;
  }
  __syncthreads();
  if (lh[tid]) atomicAdd(&hist0[c * 1024 + tid], lh[tid]);
}

// histogram [c][level] of the digit `level` (8 bits, from the top) of the keys whose higher digits are the prefix's
__global__ __launch_bounds__(NLK_SIG_THREADS) void k_sigma_hist(uint32_t* hist, const uint32_t* keys,
                                                                const NlkSigState* state, size_t n, int level) {
  __shared__ uint32_t lh[256];
  const int tid = threadIdx.x, c = blockIdx.y;
  const NlkSigState st = state[c];
  if (st.krem == 0) return;
  lh[tid] = 0;
  __syncthreads();
  const int shift = 24 - 8 * level;
  const uint32_t want = st.prefix >> (shift + 8);
  const uint32_t* kc = keys + (size_t)c * n;
  for (size_t i = (size_t)blockIdx.x * NLK_SIG_THREADS + tid; i < n; i += (size_t)gridDim.x * NLK_SIG_THREADS) {
    const uint32_t key = kc[i];
    if (key != NLK_SIG_SKIP && (key >> (shift + 8)) == want) atomicAdd(&lh[(key >> shift) & 255], 1u);
  }
  __syncthreads();
  if (lh[tid]) atomicAdd(&hist[(c * 4 + level) * 256 + tid], lh[tid]);
}

// one workgroup per channel: the digit `level` of the K-th key from histogram [c][level]
__global__ __launch_bounds__(NLK_SIG_THREADS) void k_sigma_pick(NlkSigState* state, const uint32_t* hist, int level,
                                                                float frac, int kmin) {
  __shared__ uint32_t scan[2][256];
  const int tid = threadIdx.x, c = blockIdx.x;
  const uint32_t cnt = hist[(c * 4 + level) * 256 + tid];
  int cur = 0;
  scan[0][tid] = cnt;
  __syncthreads();
  for (int d = 1; d < 256; d <<= 1) {  // inclusive sums
    scan[cur ^ 1][tid] = scan[cur][tid] + (tid >= d ? scan[cur][tid - d] : 0u);
    cur ^= 1;
    __syncthreads();
  }
  const uint32_t incl = scan[cur][tid], excl = incl - cnt, total = scan[cur][255];
  NlkSigState st = state[c];
  if (level == 0) {
    // K = min(N, max(kmin, ceil(frac N))), the product in double (tests/sigma_ref.py)
    const double want = ceil((double)frac * (double)total);
    int k = want > (double)kmin ? (int)want : kmin;
    if (k > (int)total) k = (int)total;
    st.prefix = 0;
    st.krem = st.k = k;
    st.nblocks = (int)total;
  }
  __syncthreads();  // every thread has read state[c]
  if (st.krem > 0) {
    if (excl < (uint32_t)st.krem && (uint32_t)st.krem <= incl) {  // exactly one thread
      st.prefix |= (uint32_t)tid << (24 - 8 * level);
      st.krem -= (int)excl;
      state[c] = st;
    }
  } else if (tid == 0 && level == 0) {
    state[c] = st;  // no block: krem = 0 tells the later kernels
  }
}

// part[c][g][64]: the sums of Y[i][j]^2 over the selected blocks of workgroup g's share, count[c][g]: how many
__global__ __launch_bounds__(NLK_SIG_SUM_THREADS) void k_sigma_sums(double* part, int* count, const uint32_t* keys,
                                                                const NlkSigState* state, const float* img, int w,
                                                                int ch, int step, int nbx, size_t n, size_t share) {
  constexpr int WAVES = NLK_SIG_SUM_THREADS / 64;
  __shared__ double ws[NLK_SIG_SUM_THREADS];
  __shared__ int wn[WAVES];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, c = blockIdx.y;
  const NlkSigState st = state[c];
  const int li = lane >> 3, lj = lane & 7;
  float ci[8], cj[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    ci[k] = sigma_basis(li, k);
    cj[k] = sigma_basis(lj, k);
  }
  // the wavefront's keys: its part of the workgroup's share, in steps of 64
  const size_t per_wave = (share + WAVES - 1) / WAVES;
  size_t i0 = (size_t)blockIdx.x * share + wave * per_wave;
  size_t i1 = i0 + per_wave;
  const size_t end = (size_t)(blockIdx.x + 1) * share;
  if (i1 > end) i1 = end;
  if (i1 > n) i1 = n;
  const uint32_t* kc = keys + (size_t)c * n;
  double acc = 0.0;
  int nsel = 0;
  if (st.krem > 0) {
    uint32_t ahead = i0 + lane < i1 ? kc[i0 + lane] : NLK_SIG_SKIP;  // the keys of a step are loaded a step early
    for (size_t base = i0; base < i1; base += 64) {
      const uint32_t key = ahead;
      ahead = base + 64 + lane < i1 ? kc[base + 64 + lane] : NLK_SIG_SKIP;
      const bool sel = key <= st.prefix;  // (NLK_SIG_SKIP is above every key)
      uint64_t todo = __ballot(sel);
      nsel += __popcll(todo);
      while (todo) {  // the selected blocks of these 64, in order; the loop is uniform over the wavefront
        // lane (r, k) loads sample (r, k) of the next NLK_SIG_AHEAD selected blocks at once: a wavefront's time is the
        // latency of these loads, one after the other
        float s[NLK_SIG_AHEAD];
        uint64_t next = todo;
#pragma unroll
        for (int u = 0; u < NLK_SIG_AHEAD; ++u) {
          s[u] = 0.f;
          if (next) {
            const size_t blk = base + (size_t)__builtin_ctzll(next);
            next &= next - 1;
            const size_t by = blk / (size_t)nbx, bx = blk - by * (size_t)nbx;
            s[u] = img[((by * step + li) * (size_t)w + (bx * step + lj)) * ch + c];
          }
        }
#pragma unroll
        for (int u = 0; u < NLK_SIG_AHEAD; ++u) {
          if (!todo) break;
          todo &= todo - 1;
          // row pass: lane (r, j) = sum_k B[r][k] C[j][k]; column pass: lane (i, j) = sum_r C[i][r] T[r][j]
          float t = 0.f;
#pragma unroll
          for (int k = 0; k < 8; ++k) t = __builtin_fmaf(__shfl(s[u], (lane & ~7) + k), cj[k], t);
          float y = 0.f;
#pragma unroll
          for (int r = 0; r < 8; ++r) y = __builtin_fmaf(__shfl(t, r * 8 + lj), ci[r], y);
          acc += (double)y * (double)y;
        }
      }
    }
  }
  ws[tid] = acc;
  if (lane == 0) wn[wave] = nsel;
  __syncthreads();
  if (wave == 0) {  // the wavefronts' sums, added in their order
    double sum = ws[lane];
    int cnt = wn[0];
    for (int v = 1; v < WAVES; ++v) {
      sum += ws[v * 64 + lane];
      cnt += wn[v];
    }
    part[((size_t)c * gridDim.x + blockIdx.x) * 64 + lane] = sum;
    if (lane == 0) count[c * gridDim.x + blockIdx.x] = cnt;
  }
}

// one workgroup: per channel the partials added in order (thread (q, coefficient) takes the workgroups g = q mod 4,
// then the four are added), the means, their median over i + j >= high_min, the square roots
__global__ __launch_bounds__(NLK_SIG_THREADS) void k_sigma_final(float* sigma, int* counts, const double* part,
                                                                 const int* count, const NlkSigState* state, int ch,
                                                                 int groups, int high_min) {
  __shared__ double ws[NLK_SIG_THREADS];
  __shared__ double mean[64];
  __shared__ double mid[2];
  __shared__ int wn[NLK_SIG_THREADS];
  const int tid = threadIdx.x, lane = tid & 63, q = tid >> 6;
  const int li = lane >> 3, lj = lane & 7;
  const bool high = li + lj >= high_min;
  int nhigh = 0;
  for (int i = 0; i < 8; ++i)
    for (int j = 0; j < 8; ++j) nhigh += i + j >= high_min;
  double pooled = 0.0;
  for (int c = 0; c < ch; ++c) {
    const NlkSigState st = state[c];
    double acc = 0.0;
    for (int g0 = q; g0 < groups; g0 += 32) {  // eight loads in flight; the additions in the order of g
      double v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) v[u] = g0 + 4 * u < groups ? part[((size_t)c * groups + g0 + 4 * u) * 64 + lane] : 0.0;
#pragma unroll
      for (int u = 0; u < 8; ++u) acc += v[u];
    }
    int nacc = 0;
    for (int g = tid; g < groups; g += NLK_SIG_THREADS) nacc += count[c * groups + g];
    ws[tid] = acc;
    wn[tid] = nacc;
    __syncthreads();
    for (int half = NLK_SIG_THREADS / 2; half > 0; half >>= 1) {  // (integers: any order gives the same count)
      if (tid < half) wn[tid] += wn[tid + half];
      __syncthreads();
    }
    const int nsel = st.krem > 0 ? wn[0] : 0;
    if (q == 0) mean[lane] = (((ws[lane] + ws[64 + lane]) + ws[128 + lane]) + ws[192 + lane]) / (double)nsel;
    __syncthreads();
    if (q == 0 && high) {
      // the rank of this mean among the high-frequency ones (ties by coefficient index)
      const double v = mean[lane];
      int rank = 0;
      for (int m = 0; m < 64; ++m)
        if (((m >> 3) + (m & 7)) >= high_min && (mean[m] < v || (mean[m] == v && m < lane))) ++rank;
      if (rank == (nhigh - 1) / 2) mid[0] = v;
      if (rank == nhigh / 2) mid[1] = v;
    }
    __syncthreads();
    if (tid == 0) {
      // no block, or a NaN among the means (then no rank matches): NaN
      double var = 0.5 * (mid[0] + mid[1]);
      bool nan = nsel == 0;
      for (int m = 0; m < 64; ++m) nan = nan || (((m >> 3) + (m & 7)) >= high_min && mean[m] != mean[m]);
      if (nan) var = __longlong_as_double(0x7ff8000000000000ll);
      pooled += var;
      sigma[1 + c] = (float)sqrt(var);
      if (counts) {
        counts[2 * c] = st.nblocks;
        counts[2 * c + 1] = nsel;
      }
    }
    __syncthreads();
  }
  if (tid == 0) sigma[0] = (float)sqrt(pooled / (double)ch);
}
