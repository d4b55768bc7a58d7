// k_sigma_curve.h — the noise-curve estimator of nlk_dev_estimate_noise_curve (include/nlk_hip.h):
// k_sigma.h's estimator run per bin of the block mean, then a weighted line var = a mean + b through the bins.
//
//   k_curve_keys   pass 1, one lane per block as k_sigma_keys: besides the key L it computes the block mean (the 64
//                  samples added in double in raster order), writes the mean and its bin (NLK_CURVE_NOBIN: outside
//                  [lo, hi), or a skipped block) and counts the top byte of the key in the histogram of that bin
//   k_curve_pick   pass 2, one workgroup per (channel, bin): the digit of the K_q-th key of the bin. The first call
//   k_curve_hist   fixes N_q and K_q and drops a bin with N_q < nmin (krem = 0). k_curve_hist makes the next
//                  histogram of every bin at once. Integer atomics: their sums do not depend on order.
//   k_curve_sums   pass 3, workgroup (share, bin, channel): k_sigma_sums' walk over the keys of the share, taking
//                  the blocks of its bin with L <= the bin's threshold; it also adds their means, in order
//   k_curve_final  one workgroup per channel: per bin the partials added in order, the means, their median over
//                  i + j >= high_min; then one thread fits the line over the bins kept, in double.
// The histograms live in LDS where nbins * 256 counters fit beside the tile (NLK_CURVE_LDS_BINS), else the kernels
// add straight to HBM.
#pragma once
#include "k_sigma_common.h"

#define NLK_CURVE_MAX_BINS 64
#define NLK_CURVE_NOBIN 0xffu
#define NLK_CURVE_LDS_BINS 16  // up to this many bins the per-workgroup histograms are kept in LDS (16 KiB)

struct NlkCurveBin {  // = struct nlk_curve_bin (include/nlk_hip.h)
  int nblocks, nsel;
  float mean, var;
};

template <bool STAGED, bool LHIST>
__global__ __launch_bounds__(NLK_SIG_THREADS) void k_curve_keys(uint32_t* keys, uint8_t* bins, double* means,
                                                                uint32_t* hist0, const float* img, int w, int h,
                                                                int ch, int step, int nbx, int nby, int low_max,
                                                                int nbins, float lo, float hi) {
  extern __shared__ float tile[];
  __shared__ uint32_t lh[LHIST ? NLK_CURVE_LDS_BINS * 256 : 1];
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
    bool finite = true;
    double sum = 0.0;
#pragma unroll
    for (int r = 0; r < 8; ++r)
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        b[r][k] = STAGED ? tile[(ty * step + r) * pitch + tx * step + k]
                         : img[((size_t)(by * step + r) * w + (bx * step + k)) * ch + c];
        finite = finite && fabsf(b[r][k]) <= 3.402823466e38f;  // false for NaN and the infinities
        sum += (double)b[r][k];                                 // raster order
      }
    const double m = sum / 64.0;
    uint32_t key = NLK_SIG_SKIP;
    uint32_t bin = NLK_CURVE_NOBIN;
    if (finite && m >= (double)lo && m < (double)hi) {
      int q = (int)floor((m - (double)lo) / ((double)hi - (double)lo) * (double)nbins);
      bin = (uint32_t)(q < nbins ? q : nbins - 1);
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
    bins[at] = (uint8_t)bin;
    means[at] = m;
  }
  if (LHIST) {
    __syncthreads();
    for (int i = tid; i < nbins * 256; i += NLK_SIG_THREADS)
      if (lh[i]) atomicAdd(&hist0[((size_t)c * nbins + (i >> 8)) * 1024 + (i & 255)], lh[i]);
  }
}

// histograms [c][bin][level] of the digit `level` of the keys of each bin whose higher digits are its prefix's
template <bool LHIST>
__global__ __launch_bounds__(NLK_SIG_THREADS) void k_curve_hist(uint32_t* hist, const uint32_t* keys,
                                                                const uint8_t* bins, const NlkSigState* state,
                                                                size_t n, int level, int nbins) {
  __shared__ uint32_t lh[LHIST ? NLK_CURVE_LDS_BINS * 256 : 1];
  __shared__ uint32_t want[NLK_CURVE_MAX_BINS];  // the prefix of a bin, 0xffffffff: the bin takes no part
  const int tid = threadIdx.x, c = blockIdx.y;
  const int shift = 24 - 8 * level;
  if (tid < nbins) {
    const NlkSigState st = state[c * nbins + tid];
    want[tid] = st.krem > 0 ? st.prefix >> (shift + 8) : 0xffffffffu;
  }
  if (LHIST)
    for (int i = tid; i < nbins * 256; i += NLK_SIG_THREADS) lh[i] = 0;
  __syncthreads();
  const uint32_t* kc = keys + (size_t)c * n;
  const uint8_t* bc = bins + (size_t)c * n;
  for (size_t i = (size_t)blockIdx.x * NLK_SIG_THREADS + tid; i < n; i += (size_t)gridDim.x * NLK_SIG_THREADS) {
    const uint32_t key = kc[i], bin = bc[i];
    if (bin == NLK_CURVE_NOBIN) continue;  // (then key == NLK_SIG_SKIP)
    if ((key >> (shift + 8)) != want[bin]) continue;  // (level >= 1: the shifted key is below 0xffffffff)
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

// one workgroup per (bin, channel): k_sigma_pick on the state and histogram of that pair; a bin with fewer than
// nmin blocks is dropped (krem = 0, nblocks = N_q)
__global__ __launch_bounds__(NLK_SIG_THREADS) void k_curve_pick(NlkSigState* state, const uint32_t* hist, int level,
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
    // K = min(N, max(kmin, ceil(frac N))), the product in double (tests/curve_ref.py)
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

// part[c][q][g][64]: the sums of Y[i][j]^2 over the selected blocks of bin q in workgroup g's share,
// count[c][q][g]: how many, msum[c][q][g]: the sum of their means
__global__ __launch_bounds__(NLK_SIG_SUM_THREADS) void k_curve_sums(double* part, int* count, double* msum,
                                                                    const uint32_t* keys, const uint8_t* bins,
                                                                    const double* means, const NlkSigState* state,
                                                                    const float* img, int w, int ch, int step,
                                                                    int nbx, size_t n, size_t share) {
  constexpr int WAVES = NLK_SIG_SUM_THREADS / 64;
  __shared__ double ws[NLK_SIG_SUM_THREADS];
  __shared__ double wm[WAVES];
  __shared__ int wn[WAVES];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int q = blockIdx.y, nbins = gridDim.y, c = blockIdx.z;
  const NlkSigState st = state[c * nbins + q];
  const size_t slot = ((size_t)c * nbins + q) * gridDim.x + blockIdx.x;
  if (st.krem <= 0) {  // a bin without a selection: its partials are zero (uniform over the workgroup)
    if (tid < 64) part[slot * 64 + tid] = 0.0;
    if (tid == 0) {
      count[slot] = 0;
      msum[slot] = 0.0;
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
  for (size_t base = i0; base < i1; base += 64) {
    const bool in = base + lane < i1;
    const uint32_t key = in ? kc[base + lane] : NLK_SIG_SKIP;
    const uint32_t bin = in ? bc[base + lane] : NLK_CURVE_NOBIN;
    const bool sel = bin == (uint32_t)q && key <= st.prefix;
    uint64_t todo = __ballot(sel);
    nsel += __popcll(todo);
    while (todo) {  // the selected blocks of these 64, in order; the loop is uniform over the wavefront
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
          mu[u] = mc[blk];
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
        macc += mu[u];
      }
    }
  }
  ws[tid] = acc;
  if (lane == 0) {
    wn[wave] = nsel;
    wm[wave] = macc;
  }
  __syncthreads();
  if (wave == 0) {  // the wavefronts' sums, added in their order
    double sum = ws[lane], ms = wm[0];
    int cnt = wn[0];
    for (int v = 1; v < WAVES; ++v) {
      sum += ws[v * 64 + lane];
      cnt += wn[v];
      ms += wm[v];
    }
    part[slot * 64 + lane] = sum;
    if (lane == 0) {
      count[slot] = cnt;
      msum[slot] = ms;
    }
  }
}

// one workgroup per channel. Per bin: the partials added in order (thread (p, coefficient) takes the workgroups
// g = p mod 4, then the four are added), the means, their median over i + j >= high_min, the mean of the block means.
// Then thread 0 fits var = a mean + b over the bins kept with weights n_q (the three rules of include/nlk_hip.h).
__global__ __launch_bounds__(NLK_SIG_THREADS) void k_curve_final(float* curve, NlkCurveBin* out_bins,
                                                                 const double* part, const int* count,
                                                                 const double* msum, const NlkSigState* state,
                                                                 int nbins, int groups, int high_min) {
  __shared__ double ws[NLK_SIG_THREADS];
  __shared__ double mean[64];
  __shared__ double mid[2];
  __shared__ double bm[NLK_CURVE_MAX_BINS], bv[NLK_CURVE_MAX_BINS];
  __shared__ int bn[NLK_CURVE_MAX_BINS];
  const int tid = threadIdx.x, lane = tid & 63, p = tid >> 6, c = blockIdx.x;
  const int li = lane >> 3, lj = lane & 7;
  const bool high = li + lj >= high_min;
  const double qnan = __longlong_as_double(0x7ff8000000000000ll);
  int nhigh = 0;
  for (int i = 0; i < 8; ++i)
    for (int j = 0; j < 8; ++j) nhigh += i + j >= high_min;
  for (int q = 0; q < nbins; ++q) {
    const NlkSigState st = state[c * nbins + q];
    const size_t slot0 = ((size_t)c * nbins + q) * groups;
    int nsel = 0;
    double var = qnan, mq = qnan;
    if (st.krem > 0) {  // (uniform over the workgroup)
      double acc = 0.0;
      for (int g = p; g < groups; g += 4) acc += part[(slot0 + g) * 64 + lane];
      ws[tid] = acc;
      __syncthreads();
      double ms = 0.0;
      for (int g = 0; g < groups; ++g) {  // (every thread the same sums: nothing to share)
        nsel += count[slot0 + g];
        ms += msum[slot0 + g];
      }
      if (p == 0) mean[lane] = (((ws[lane] + ws[64 + lane]) + ws[128 + lane]) + ws[192 + lane]) / (double)nsel;
      __syncthreads();
      if (p == 0 && high) {
        // the rank of this mean among the high-frequency ones (ties by coefficient index)
        const double v = mean[lane];
        int rank = 0;
        for (int m = 0; m < 64; ++m)
          if (((m >> 3) + (m & 7)) >= high_min && (mean[m] < v || (mean[m] == v && m < lane))) ++rank;
        if (rank == (nhigh - 1) / 2) mid[0] = v;
        if (rank == nhigh / 2) mid[1] = v;
      }
      __syncthreads();
      var = 0.5 * (mid[0] + mid[1]);
      for (int m = 0; m < 64; ++m)  // a NaN among the means (then no rank matches): NaN
        if (((m >> 3) + (m & 7)) >= high_min && mean[m] != mean[m]) var = qnan;
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
    __syncthreads();  // mean, mid and ws are free again
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
