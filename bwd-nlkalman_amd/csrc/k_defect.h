// k_defect.h — one step of the defect map learned over time: nlk_dev_defect_step (include/nlk_hip.h; the
// rule is stated in numpy by tests/defectmap_ref.py). despike's range test (k_despike.h) is read on the temporal mean
// `mean_in` of the frames before this one; where it hits, the sample of the frame `in` becomes the median of its own
// ring; the mean takes the raw sample either way.
//
// k_despike.h's lane layout and ring walk, by inclusion: lane l of a wave works on flat sample f0 + l of a row of w ch
// floats, a workgroup of 256 lanes walks down DESPIKE_ROWS rows, the ring's re-reads are L1 hits, a wave whose ring lies
// inside the frame (wave-uniform test) skips the index arithmetic. Per sample the kernel moves four planes (in, mean_in
// read; out, mean_out written) where despike moves two, plus one byte with a map. The ring of `in` (8 R more loads) and
// its sort run only in a wave that has a hit (a wave-uniform branch: hits are as rare as defects). The counts: one
// integer atomic per wave and channel with a replaced sample, after a ballot. No float atomics: every call gives the
// same bits.
#pragma once
#include "k_despike.h"

// what the lane's sample gives: p_v / p_m = the lane's sample of the frame and of the mean (FAST: in its row; general:
// the planes themselves, with the offsets yo[], xo[] of despike_ring). hit: the mean is outside its ring's range by more
// than thr; rep: ... and `out` is the median of the frame's ring (the frame and its ring are finite there)
template <int R, bool FAST>
__device__ __forceinline__ void defect_sample(const float* p_v, const float* p_m, ptrdiff_t W, int ch, const ptrdiff_t* yo,
                                              const int* xo, float thr, float gain, float& out, float& mean, bool& hit,
                                              bool& rep) {
#pragma clang fp contract(off)
  constexpr int N = 8 * R;
  float a[N];
  const float m = despike_ring<R, FAST>(a, p_m, W, ch, yo, xo);
  float mn, mx, nf;
  despike_range<N>(a, m, mn, mx, nf);
  hit = nf == 0.f && (m > mx + thr || m < mn - thr);
  const float v = FAST ? p_v[0] : p_v[yo[R] + xo[R]];
  out = v;
  rep = false;
  if (__builtin_amdgcn_ballot_w64(hit) != 0) {  // wave-uniform
    const float c = despike_ring<R, FAST>(a, p_v, W, ch, yo, xo);
    float lo, hi;
    despike_range<N>(a, c, lo, hi, nf);  // (lo, hi: not used; nf is)
    despike_middle<N>(a, lo, hi);
    rep = hit && nf == 0.f;
    if (rep) out = (lo + hi) * 0.5f;
  }
  const float d = (v - m) * gain;
  mean = v * 0.f == 0.f ? m + d : m;  // a non-finite sample leaves the mean as it is
}

// grid: as k_despike's. map: nullptr, or w h ch bytes (every one is written); count: nullptr, or ch words (zeroed)
template <int R>
__global__ __launch_bounds__(DESPIKE_THREADS) void k_defect_step(float* __restrict__ out, const float* __restrict__ in,
                                                                 float* __restrict__ mean_out,
                                                                 const float* __restrict__ mean_in, uint8_t* __restrict__ map,
                                                                 uint32_t* count, int w, int h, int ch, float thr, float gain,
                                                                 int nbx) {
  const int by = blockIdx.x / nbx, bx = blockIdx.x - by * nbx;  // (uniform)
  const int W = w * ch;
  const int f = bx * DESPIKE_THREADS + threadIdx.x;
  const bool live = f < W;
  const int fc = live ? f : W - 1;  // a lane past the row's end works on the last sample and stores nothing
  const int wave_f0 = bx * DESPIKE_THREADS + (threadIdx.x & ~63);
  const bool cols_in = wave_f0 >= R * ch && wave_f0 + 63 <= W - 1 - R * ch;  // (uniform in the wave; every lane live)
  const int x = fc / ch, c = fc - x * ch;
  int xo[2 * R + 1];
#pragma unroll
  for (int d = -R; d <= R; ++d) xo[d + R] = despike_reflect(x + d, w) * ch + c;
  const int y1 = min(h, (by + 1) * DESPIKE_ROWS);
  for (int y = by * DESPIKE_ROWS; y < y1; ++y) {
    bool hit, rep;
    float r, m;
    const size_t row = (size_t)y * W;
    if (cols_in && y >= R && y < h - R) {
      defect_sample<R, true>(in + row + fc, mean_in + row + fc, W, ch, nullptr, nullptr, thr, gain, r, m, hit, rep);
    } else {
      ptrdiff_t yo[2 * R + 1];
#pragma unroll
      for (int d = -R; d <= R; ++d) yo[d + R] = (ptrdiff_t)despike_reflect(y + d, h) * W;
      defect_sample<R, false>(in, mean_in, W, ch, yo, xo, thr, gain, r, m, hit, rep);
    }
    rep = rep && live;
    if (live) {
      out[row + f] = r;
      mean_out[row + f] = m;
      if (map) map[row + f] = hit ? 1 : 0;
    }
    if (count && __builtin_amdgcn_ballot_w64(rep) != 0) {  // (wave-uniform) one atomic per channel with a replaced sample
      for (int k = 0; k < ch; ++k) {
        const uint64_t b = __builtin_amdgcn_ballot_w64(rep && c == k);
        if (b != 0 && (threadIdx.x & 63) == 0) atomicAdd(count + k, (uint32_t)__popcll(b));
      }
    }
  }
}

// the first frame: nothing is known yet. out = in bit for bit, the mean starts as the frame (0 at a non-finite sample),
// the map is empty. n = w h ch samples, one per lane
__global__ __launch_bounds__(DESPIKE_THREADS) void k_defect_first(float* __restrict__ out, const float* __restrict__ in,
                                                                  float* __restrict__ mean_out, uint8_t* __restrict__ map,
                                                                  size_t n) {
  const size_t i = (size_t)blockIdx.x * DESPIKE_THREADS + threadIdx.x;
  if (i >= n) return;
  const float v = in[i];
  out[i] = v;
  mean_out[i] = v * 0.f == 0.f ? v : 0.f;
  if (map) map[i] = 0;
}
