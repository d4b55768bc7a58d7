// k_sigma.h — the block-DCT percentile estimator behind nlk_dev_estimate_sigma and nlk_dev_estimate_noise_curve
// (include/nlk_hip.h), stated once. Per slot — a channel, or with BINNED a (channel, bin of the block
// mean) pair — the 8 x 8 blocks on a grid of `step`, their orthonormal DCT Y, the low-frequency energy L of each, the
// K-th smallest L found exactly, and the median over the high-frequency coefficients of the mean of Y[i][j]^2 over the
// blocks with L <= that value. Unbinned is binned with one bin per channel, no range test and no block mean; its
// kernels touch no `bins` / `means` / `msum` array. The state and the histograms are [slot] and [slot][4][256].
//
//   k_sigma_keys   pass 1, one lane per block: the block from an LDS tile of the channel (or, where the tile of a
//   k_curve_keys   large step does not fit, straight from the image), 8 row + 8 column transforms on registers
//                  (k_dct8.h), L as a 32-bit key (the bits of a non-negative float order as the float does;
//                  NLK_SIG_SKIP for a block holding a non-finite sample) and the histogram of the keys' top byte.
//                  Binned: also the block mean (the 64 samples added in double in raster order) and its bin
//                  (NLK_CURVE_NOBIN: outside [lo, hi), or a skipped block), the histogram being that of the bin
//   k_sigma_pick   pass 2, one workgroup per slot: the digit of the K-th key in the current histogram; the first call
//   k_sigma_hist   also counts the blocks, fixes K and drops a slot with fewer than nmin blocks (krem = 0).
//   k_curve_hist   k_*_hist makes the next histogram, of the keys that share the digits found so far, for every bin
//                  at once. Integer atomics in LDS and HBM: their sums do not depend on order.
//   k_sigma_sums   pass 3, a workgroup per share (and bin): a wavefront walks its part of the keys in order and
//   k_curve_sums   transforms each selected block (of its bin) again, lane (i, j) holding Y[i][j] and adding its
//                  square to one double; binned, the block means are added too. The shares are a function of the
//                  sizes alone, so are the per-workgroup partials ...
//   k_sigma_final  ... which nlk_sig_slot_var adds in order per slot; lane (i, j) ranks its mean among the
//   k_curve_final  high-frequency ones and the two middle ranks give the median. k_sigma_final, one workgroup over
//                  the channels, pools the variances and writes the square roots; k_curve_final, one workgroup per
//                  channel over the bins, averages the block means and one thread fits the line var = a mean + b.
// The binned histograms live in LDS where nbins * 256 counters fit beside the tile (NLK_CURVE_LDS_BINS), else the
// kernels add straight to HBM.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "k_dct8.h"

#define NLK_SIG_THREADS 256
#define NLK_SIG_TBX 32             // k_*_keys: blocks per workgroup, across ...
#define NLK_SIG_TBY 8              // ... and down
#define NLK_SIG_LDS_MAX (48 << 10) // the tile is staged in LDS where it fits in this many bytes (step <= 6)
#define NLK_SIG_SKIP 0xffffffffu   // key of a skipped block
#define NLK_SIG_MAX_GROUPS 256     // k_sigma_hist / k_sigma_sums: workgroups per channel at most
#define NLK_SIG_SUM_THREADS 1024   // k_*_sums: 16 wavefronts, so that each walks a short run of keys
#define NLK_SIG_AHEAD 4            // k_*_sums: selected blocks whose samples are loaded together

#define NLK_CURVE_MAX_BINS 64
#define NLK_CURVE_MAX_GROUPS 64    // k_curve_hist / k_curve_sums: pass 3 runs one workgroup per share and bin
#define NLK_CURVE_NOBIN 0xffu
#define NLK_CURVE_LDS_BINS 16      // up to this many bins the per-workgroup histograms are kept in LDS (16 KiB)

struct NlkSigState {  // per slot, between the kernels of pass 2
  uint32_t prefix;    // the digits of the K-th key found so far (after the last pick: the key itself)
  int krem;           // its rank among the keys that share them, from 1; 0: the slot has no block, or too few
  int nblocks, k;     // N, K
};

struct NlkCurveBin {  // = struct nlk_curve_bin (include/nlk_hip.h)
  int nblocks, nsel;
  float mean, var;
};

// the LDS tile of a workgroup of pass 1: its size in pixels and its row pitch
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

// the counters of a workgroup's histograms in LDS: 256 per bin, none where the kernel adds straight to HBM
template <bool BINNED, bool LHIST>
constexpr int nlk_sig_lds_counters() {
  return !LHIST ? 1 : BINNED ? NLK_CURVE_LDS_BINS * 256 : 256;
}

// ---- pass 1. Unbinned: LHIST, and bins / means / nbins / lo / hi are not looked at.
template <bool STAGED, bool BINNED, bool LHIST>
__device__ __forceinline__ void nlk_sig_keys(uint32_t* keys, uint8_t* bins, double* means, uint32_t* hist0,
                                             const float* img, int w, int h, int ch, int step, int nbx, int nby,
                                             int low_max, int nbins, float lo, float hi) {
  extern __shared__ float tile[];
  __shared__ uint32_t lh[nlk_sig_lds_counters<BINNED, LHIST>()];
  if (!BINNED) nbins = 1;
  const int tid = threadIdx.x, c = blockIdx.z;
  const int tx = tid % NLK_SIG_TBX, ty = tid / NLK_SIG_TBX;
  const int bx = blockIdx.x * NLK_SIG_TBX + tx, by = blockIdx.y * NLK_SIG_TBY + ty;
  const int x0 = blockIdx.x * NLK_SIG_TBX * step, y0 = blockIdx.y * NLK_SIG_TBY * step;
  const int pitch = STAGED ? nlk_sig_pitch(step) : 0;
  if (LHIST)
    for (int i = tid; i < nbins * 256; i += NLK_SIG_THREADS) lh[i] = 0;
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
    bool take = true;  // the block is finite (and its mean in range)
    double sum = 0.0;
#pragma unroll
    for (int r = 0; r < 8; ++r)
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        b[r][k] = STAGED ? tile[(ty * step + r) * pitch + tx * step + k]
                         : img[((size_t)(by * step + r) * w + (bx * step + k)) * ch + c];
        take = take && fabsf(b[r][k]) <= 3.402823466e38f;  // false for NaN and the infinities
        if (BINNED) sum += (double)b[r][k];                // raster order
      }
    const double m = sum / 64.0;
    uint32_t key = NLK_SIG_SKIP;
    uint32_t bin = BINNED ? NLK_CURVE_NOBIN : 0;
    if (BINNED) take = take && m >= (double)lo && m < (double)hi;
    if (take) {
      if (BINNED) {
        int q = (int)floor((m - (double)lo) / ((double)hi - (double)lo) * (double)nbins);
        bin = (uint32_t)(q < nbins ? q : nbins - 1);
      }
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
      if (LHIST)
        atomicAdd(&lh[bin * 256 + (key >> 24)], 1u);
      else
        atomicAdd(&hist0[((size_t)c * nbins + bin) * 1024 + (key >> 24)], 1u);
    }
    const size_t at = ((size_t)c * nby + by) * nbx + bx;
    keys[at] = key;
    if (BINNED) {
      bins[at] = (uint8_t)bin;
      means[at] = m;
    }
  }
  if (LHIST) {
    __syncthreads();
    for (int i = tid; i < nbins * 256; i += NLK_SIG_THREADS)
      if (lh[i]) atomicAdd(&hist0[((size_t)c * nbins + (i >> 8)) * 1024 + (i & 255)], lh[i]);
  }
}

template <bool STAGED>
__global__ __launch_bounds__(NLK_SIG_THREADS) void k_sigma_keys(uint32_t* keys, uint32_t* hist0, const float* img,
                                                                int w, int h, int ch, int step, int nbx, int nby,
                                                                int low_max) {
  nlk_sig_keys<STAGED, false, true>(keys, nullptr, nullptr, hist0, img, w, h, ch, step, nbx, nby, low_max, 1, 0.f, 0.f);
}

template <bool STAGED, bool LHIST>
__global__ __launch_bounds__(NLK_SIG_THREADS) void k_curve_keys(uint32_t* keys, uint8_t* bins, double* means,
                                                                uint32_t* hist0, const float* img, int w, int h,
                                                                int ch, int step, int nbx, int nby, int low_max,
                                                                int nbins, float lo, float hi) {
  nlk_sig_keys<STAGED, true, LHIST>(keys, bins, means, hist0, img, w, h, ch, step, nbx, nby, low_max, nbins, lo, hi);
}

// ---- pass 2: histograms [slot][level] of the digit `level` (8 bits, from the top) of the keys of each slot whose
// higher digits are its prefix's
template <bool BINNED, bool LHIST>
__device__ __forceinline__ void nlk_sig_hist(uint32_t* hist, const uint32_t* keys, const uint8_t* bins,
                                             const NlkSigState* state, size_t n, int level, int nbins) {
  __shared__ uint32_t lh[nlk_sig_lds_counters<BINNED, LHIST>()];
  __shared__ uint32_t wants[BINNED ? NLK_CURVE_MAX_BINS : 1];  // the prefix of a bin, 0xffffffff: the bin takes no part
  if (!BINNED) nbins = 1;
  const int tid = threadIdx.x, c = blockIdx.y;
  const int shift = 24 - 8 * level;
  auto prefix_of = [&](int slot) {
    const NlkSigState st = state[slot];
    return st.krem > 0 ? st.prefix >> (shift + 8) : 0xffffffffu;
  };
  uint32_t want = 0;  // unbinned: the one prefix, in a register
  if (BINNED) {
    if (tid < nbins) wants[tid] = prefix_of(c * nbins + tid);
  } else {
    want = prefix_of(c);
    if (want == 0xffffffffu) return;  // (uniform over the workgroup)
  }
  if (LHIST)
    for (int i = tid; i < nbins * 256; i += NLK_SIG_THREADS) lh[i] = 0;
  __syncthreads();
  const uint32_t* kc = keys + (size_t)c * n;
  const uint8_t* bc = bins + (size_t)c * n;
  for (size_t i = (size_t)blockIdx.x * NLK_SIG_THREADS + tid; i < n; i += (size_t)gridDim.x * NLK_SIG_THREADS) {
    const uint32_t key = kc[i], bin = BINNED ? bc[i] : 0;
    if (key == NLK_SIG_SKIP) continue;  // (binned: just then bin == NLK_CURVE_NOBIN)
    if ((key >> (shift + 8)) != (BINNED ? wants[bin] : want)) continue;  // (level >= 1: the shifted key is below 0xffffffff)
    if (LHIST)
      atomicAdd(&lh[bin * 256 + ((key >> shift) & 255)], 1u);
    else
      atomicAdd(&hist[(((size_t)c * nbins + bin) * 4 + level) * 256 + ((key >> shift) & 255)], 1u);
  }
  if (LHIST) {
    __syncthreads();
    for (int i = tid; i < nbins * 256; i += NLK_SIG_THREADS)
      if (lh[i]) atomicAdd(&hist[(((size_t)c * nbins + (i >> 8)) * 4 + level) * 256 + (i & 255)], lh[i]);
  }
}

__global__ __launch_bounds__(NLK_SIG_THREADS) void k_sigma_hist(uint32_t* hist, const uint32_t* keys,
                                                                const NlkSigState* state, size_t n, int level) {
  nlk_sig_hist<false, true>(hist, keys, nullptr, state, n, level, 1);
}

template <bool LHIST>
__global__ __launch_bounds__(NLK_SIG_THREADS) void k_curve_hist(uint32_t* hist, const uint32_t* keys,
                                                                const uint8_t* bins, const NlkSigState* state,
                                                                size_t n, int level, int nbins) {
  nlk_sig_hist<true, LHIST>(hist, keys, bins, state, n, level, nbins);
}

// one workgroup per slot (grid: channels, or bins x channels): the digit `level` of the K-th key from histogram
// [slot][level]; a slot with fewer than nmin blocks is dropped (krem = 0, nblocks = N)
__global__ __launch_bounds__(NLK_SIG_THREADS) void k_sigma_pick(NlkSigState* state, const uint32_t* hist, int level,
                                                                float frac, int kmin, int nmin) {
  __shared__ uint32_t scan[2][256];
  const int tid = threadIdx.x, s = blockIdx.y * gridDim.x + blockIdx.x;
  const uint32_t cnt = hist[((size_t)s * 4 + level) * 256 + tid];
  int cur = 0;
  scan[0][tid] = cnt;
  __syncthreads();
  for (int d = 1; d < 256; d <<= 1) {  // inclusive sums
    scan[cur ^ 1][tid] = scan[cur][tid] + (tid >= d ? scan[cur][tid - d] : 0u);
    cur ^= 1;
    __syncthreads();
  }
  const uint32_t incl = scan[cur][tid], excl = incl - cnt, total = scan[cur][255];
  NlkSigState st = state[s];
  if (level == 0) {
    // K = min(N, max(kmin, ceil(frac N))), the product in double (tests/sigma_ref.py, tests/curve_ref.py)
    const double want = ceil((double)frac * (double)total);
    int k = want > (double)kmin ? (int)want : kmin;
    if (k > (int)total) k = (int)total;
    if ((int)total < nmin) k = 0;
    st.prefix = 0;
    st.krem = st.k = k;
    st.nblocks = (int)total;
  }
  __syncthreads();  // every thread has read state[s]
  if (st.krem > 0) {
    if (excl < (uint32_t)st.krem && (uint32_t)st.krem <= incl) {  // exactly one thread
      st.prefix |= (uint32_t)tid << (24 - 8 * level);
      st.krem -= (int)excl;
      state[s] = st;
    }
  } else if (tid == 0 && level == 0) {
    state[s] = st;  // no block, or too few: krem = 0 tells the later kernels
  }
}

// ---- pass 3. part[slot][g][64]: the sums of Y[i][j]^2 over the selected blocks of the slot in workgroup g's share,
// count[slot][g]: how many, binned msum[slot][g]: the sum of their means. Grid (shares, channels), binned
// (shares, bins, channels). The unbinned walk loads the keys of a step a step early.
template <bool BINNED>
__device__ __forceinline__ void nlk_sig_sums(double* part, int* count, double* msum, const uint32_t* keys,
                                             const uint8_t* bins, const double* means, const NlkSigState* state,
                                             const float* img, int w, int ch, int step, int nbx, size_t n,
                                             size_t share) {
  constexpr int WAVES = NLK_SIG_SUM_THREADS / 64;
  __shared__ double ws[NLK_SIG_SUM_THREADS];
  __shared__ double wm[BINNED ? WAVES : 1];
  __shared__ int wn[WAVES];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int q = BINNED ? blockIdx.y : 0, nbins = BINNED ? gridDim.y : 1, c = BINNED ? blockIdx.z : blockIdx.y;
  const NlkSigState st = state[c * nbins + q];
  const size_t slot = ((size_t)c * nbins + q) * gridDim.x + blockIdx.x;
  if (st.krem <= 0) {  // a slot without a selection: its partials are zero (uniform over the workgroup)
    if (tid < 64) part[slot * 64 + tid] = 0.0;
    if (tid == 0) {
      count[slot] = 0;
      if (BINNED) msum[slot] = 0.0;
    }
    return;
  }
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
  const uint8_t* bc = bins + (size_t)c * n;
  const double* mc = means + (size_t)c * n;
  double acc = 0.0, macc = 0.0;
  int nsel = 0;
  uint32_t ahead = !BINNED && i0 + lane < i1 ? kc[i0 + lane] : NLK_SIG_SKIP;
  for (size_t base = i0; base < i1; base += 64) {
    const size_t at = BINNED ? base : base + 64;  // unbinned: the keys of a step are loaded a step early
    const bool in = at + lane < i1;
    const uint32_t loaded = in ? kc[at + lane] : NLK_SIG_SKIP;
    const uint32_t bin = !BINNED ? 0 : in ? bc[at + lane] : NLK_CURVE_NOBIN;
    const uint32_t key = BINNED ? loaded : ahead;
    ahead = loaded;
    const bool sel = bin == (uint32_t)q && key <= st.prefix;  // (NLK_SIG_SKIP is above every key)
    uint64_t todo = __ballot(sel);
    nsel += __popcll(todo);
    while (todo) {  // the selected blocks of these 64, in order; the loop is uniform over the wavefront
      // lane (r, k) loads sample (r, k) of the next NLK_SIG_AHEAD selected blocks at once: a wavefront's time is the
      // latency of these loads, one after the other
      float s[NLK_SIG_AHEAD];
      double mu[NLK_SIG_AHEAD];
      uint64_t next = todo;
#pragma unroll
      for (int u = 0; u < NLK_SIG_AHEAD; ++u) {
        s[u] = 0.f;
        mu[u] = 0.0;
        if (next) {
          const size_t blk = base + (size_t)__builtin_ctzll(next);
          next &= next - 1;
          const size_t by = blk / (size_t)nbx, bx = blk - by * (size_t)nbx;
          s[u] = img[((by * step + li) * (size_t)w + (bx * step + lj)) * ch + c];
          if (BINNED) mu[u] = mc[blk];
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
        if (BINNED) macc += mu[u];
      }
    }
  }
  ws[tid] = acc;
  if (lane == 0) {
    wn[wave] = nsel;
    if (BINNED) wm[wave] = macc;
  }
  __syncthreads();
  if (wave == 0) {  // the wavefronts' sums, added in their order
    double sum = ws[lane], ms = BINNED ? wm[0] : 0.0;
    int cnt = wn[0];
    for (int v = 1; v < WAVES; ++v) {
      sum += ws[v * 64 + lane];
      cnt += wn[v];
      if (BINNED) ms += wm[v];
    }
    part[slot * 64 + lane] = sum;
    if (lane == 0) {
      count[slot] = cnt;
      if (BINNED) msum[slot] = ms;
    }
  }
}

__global__ __launch_bounds__(NLK_SIG_SUM_THREADS) void k_sigma_sums(double* part, int* count, const uint32_t* keys,
                                                                    const NlkSigState* state, const float* img, int w,
                                                                    int ch, int step, int nbx, size_t n, size_t share) {
  nlk_sig_sums<false>(part, count, nullptr, keys, nullptr, nullptr, state, img, w, ch, step, nbx, n, share);
}

__global__ __launch_bounds__(NLK_SIG_SUM_THREADS) void k_curve_sums(double* part, int* count, double* msum,
                                                                    const uint32_t* keys, const uint8_t* bins,
                                                                    const double* means, const NlkSigState* state,
                                                                    const float* img, int w, int ch, int step,
                                                                    int nbx, size_t n, size_t share) {
  nlk_sig_sums<true>(part, count, msum, keys, bins, means, state, img, w, ch, step, nbx, n, share);
}

// ---- the final kernels
struct NlkSigFinalLds {
  double ws[NLK_SIG_THREADS];
  double mean[64];
  double mid[2];
  int wn[NLK_SIG_THREADS];
};

// One workgroup on the partials part[groups][64], count[groups] of one slot that has a selection: the partials added
// in order (thread (p, coefficient) takes the workgroups g = p, p + 4, ..., then the four are added), the means, and
// their median over i + j >= high_min, which every thread returns with the number of selected blocks; NaN for a NaN
// among the means. On return the LDS is free again.
__device__ __forceinline__ double nlk_sig_slot_var(NlkSigFinalLds& s, int* nsel, const double* part, const int* count,
                                                   int groups, int high_min) {
  const int tid = threadIdx.x, lane = tid & 63, p = tid >> 6;
  int nhigh = 0;
  for (int i = 0; i < 8; ++i)
    for (int j = 0; j < 8; ++j) nhigh += i + j >= high_min;
  double acc = 0.0;
  for (int g0 = p; g0 < groups; g0 += 32) {  // eight loads in flight; the additions in the order of g
    double v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = g0 + 4 * u < groups ? part[((size_t)g0 + 4 * u) * 64 + lane] : 0.0;
#pragma unroll
    for (int u = 0; u < 8; ++u) acc += v[u];
  }
  int nacc = 0;
  for (int g = tid; g < groups; g += NLK_SIG_THREADS) nacc += count[g];
  s.ws[tid] = acc;
  s.wn[tid] = nacc;
  __syncthreads();
  for (int half = NLK_SIG_THREADS / 2; half > 0; half >>= 1) {  // (integers: any order gives the same count)
    if (tid < half) s.wn[tid] += s.wn[tid + half];
    __syncthreads();
  }
  const int n = s.wn[0];
  if (p == 0) s.mean[lane] = (((s.ws[lane] + s.ws[64 + lane]) + s.ws[128 + lane]) + s.ws[192 + lane]) / (double)n;
  __syncthreads();
  if (p == 0 && (lane >> 3) + (lane & 7) >= high_min) {
    // the rank of this mean among the high-frequency ones (ties by coefficient index)
    const double v = s.mean[lane];
    int rank = 0;
    for (int m = 0; m < 64; ++m)
      if (((m >> 3) + (m & 7)) >= high_min && (s.mean[m] < v || (s.mean[m] == v && m < lane))) ++rank;
    if (rank == (nhigh - 1) / 2) s.mid[0] = v;
    if (rank == nhigh / 2) s.mid[1] = v;
  }
  __syncthreads();
  double var = 0.5 * (s.mid[0] + s.mid[1]);
  for (int m = 0; m < 64; ++m)  // a NaN among the means (then no rank matches): NaN
    if (((m >> 3) + (m & 7)) >= high_min && s.mean[m] != s.mean[m]) var = __longlong_as_double(0x7ff8000000000000ll);
  __syncthreads();
  *nsel = n;
  return var;
}

// one workgroup over the channels: the variances pooled, the square roots written
__global__ __launch_bounds__(NLK_SIG_THREADS) void k_sigma_final(float* sigma, int* counts, const double* part,
                                                                 const int* count, const NlkSigState* state, int ch,
                                                                 int groups, int high_min) {
  __shared__ NlkSigFinalLds lds;
  double pooled = 0.0;
  for (int c = 0; c < ch; ++c) {
    const NlkSigState st = state[c];
    int nsel = 0;
    double var = __longlong_as_double(0x7ff8000000000000ll);  // no block: NaN
    if (st.krem > 0)  // (uniform over the workgroup)
      var = nlk_sig_slot_var(lds, &nsel, part + (size_t)c * groups * 64, count + (size_t)c * groups, groups, high_min);
    if (threadIdx.x == 0) {
      pooled += var;
      sigma[1 + c] = (float)sqrt(var);
      if (counts) {
        counts[2 * c] = st.nblocks;
        counts[2 * c + 1] = nsel;
      }
    }
  }
  if (threadIdx.x == 0) sigma[0] = (float)sqrt(pooled / (double)ch);
}

// one workgroup per channel over the bins: per bin the variance and the mean of the block means; then thread 0 fits
// var = a mean + b over the bins kept with weights n_q (the three rules of include/nlk_hip.h)
__global__ __launch_bounds__(NLK_SIG_THREADS) void k_curve_final(float* curve, NlkCurveBin* out_bins,
                                                                 const double* part, const int* count,
                                                                 const double* msum, const NlkSigState* state,
                                                                 int nbins, int groups, int high_min) {
  __shared__ NlkSigFinalLds lds;
  __shared__ double bm[NLK_CURVE_MAX_BINS], bv[NLK_CURVE_MAX_BINS];
  __shared__ int bn[NLK_CURVE_MAX_BINS];
  const int tid = threadIdx.x, c = blockIdx.x;
  const double qnan = __longlong_as_double(0x7ff8000000000000ll);
  for (int q = 0; q < nbins; ++q) {
    const NlkSigState st = state[c * nbins + q];
    const size_t slot0 = ((size_t)c * nbins + q) * groups;
    int nsel = 0;
    double var = qnan, mq = qnan;
    if (st.krem > 0) {  // (uniform over the workgroup)
      var = nlk_sig_slot_var(lds, &nsel, part + slot0 * 64, count + slot0, groups, high_min);
      double ms = 0.0;
      for (int g = 0; g < groups; ++g) ms += msum[slot0 + g];  // (every thread the same sum: nothing to share)
      mq = ms / (double)nsel;
    }
    if (tid == 0) {
      bn[q] = nsel;
      bm[q] = mq;
      bv[q] = var;
      if (out_bins) {
        NlkCurveBin o;
        o.nblocks = st.nblocks;
        o.nsel = nsel;
        o.mean = (float)mq;
        o.var = (float)var;
        out_bins[c * nbins + q] = o;
      }
    }
  }
  if (tid == 0) {
    int kept = 0;
    double sn = 0.0, snm = 0.0, snv = 0.0;
    for (int q = 0; q < nbins; ++q)
      if (bn[q] > 0) {
        ++kept;
        sn += (double)bn[q];
        snm += (double)bn[q] * bm[q];
        snv += (double)bn[q] * bv[q];
      }
    double a = qnan, b = qnan;
    if (kept > 0) {
      const double mbar = snm / sn, vbar = snv / sn;
      double sxx = 0.0, sxy = 0.0, smm = 0.0, smv = 0.0;
      for (int q = 0; q < nbins; ++q)
        if (bn[q] > 0) {
          const double d = bm[q] - mbar;
          sxx += (double)bn[q] * d * d;
          sxy += (double)bn[q] * d * (bv[q] - vbar);
          smm += (double)bn[q] * bm[q] * bm[q];
          smv += (double)bn[q] * bm[q] * bv[q];
        }
      a = kept >= 2 && sxx != 0.0 ? sxy / sxx : -1.0;
      b = vbar - a * mbar;
      if (!(a >= 0.0)) {  // fewer than two bins, no spread of the means, or a falling line: a constant
        a = 0.0;
        b = vbar;
      }
      if (b < 0.0) {  // a line through the origin
        a = smv / smm;
        b = 0.0;
      }
    }
    curve[2 * c] = (float)a;
    curve[2 * c + 1] = (float)b;
  }
}
