// k_despike.h — the defective-pixel filter of nlk_dev_despike (include/nlk_hip.h; the rule is stated in
// numpy by tests/despike_ref.py): a sample that lies more than thr outside the range of its ring (the 8 R samples of
// its own channel at Chebyshev distance exactly R) becomes the ring's median, anything else is copied bit for bit.
//
// One read, one write, bound by memory traffic. A row is w ch flat floats: lane l of a wave works on flat sample
// f0 + l, so a ring neighbour (dx, dy) of every lane sits at the same distance dy W + dx ch and each of the 8 R + 1
// loads of a wave is one contiguous 256-byte segment, whatever ch is. The ring's rows overlap between neighbouring
// lanes and between the rows a workgroup walks down (DESPIKE_ROWS of them, one after the other): the re-reads are L1
// hits. Measured on a 1080p RGB frame (profiles/despike_time.txt): 15.2 us at R = 1 and 22.6 us at R = 2 this way, 21.7 and
// 28.6 us with the 2 R + DESPIKE_ROWS rows of a workgroup staged in LDS first (one path for every sample, the border
// indices resolved while staging): the staging adds a pass through LDS and a barrier to reads that L1 already serves,
// so the L1 form is the one kept. A wave whose samples all have their ring inside the frame (wave-uniform test) takes the path without index
// arithmetic; the waves on the border columns and rows reflect their indices (j = |i|, 2 (n - 1) - j past the end,
// then clamped).
//
// Per ring value: one v_min, one v_max and one FMA into `nf`, which stays 0 while the centre and the ring are finite
// and is NaN otherwise (x * 0 is NaN for an infinity and for a NaN; fminf / fmaxf would drop a NaN). The two middle
// order statistics come from Batcher's odd-even merge sort, unrolled, of which the compiler keeps the comparators that
// feed those two outputs; it runs only in a wave that has a hit (a wave-uniform branch: hits are rare). The counts:
// one integer atomic per wave and channel with a hit, after a ballot.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define DESPIKE_THREADS 256
#define DESPIKE_ROWS 8  // rows a workgroup walks down

__device__ __forceinline__ int despike_reflect(int i, int n) {
  int j = i < 0 ? -i : i;
  if (j >= n) j = 2 * (n - 1) - j;
  return min(max(j, 0), n - 1);
}

// (lo, hi) = the two middle order statistics of a[0 .. N), N = 8 or 16; the values are finite where the result is used
template <int N>
__device__ __forceinline__ void despike_middle(float (&a)[N], float& lo, float& hi) {
#pragma unroll
  for (int p = 1; p < N; p *= 2) {
#pragma unroll
    for (int k = p; k >= 1; k /= 2) {
#pragma unroll
      for (int j = k % p; j + k < N; j += 2 * k) {
#pragma unroll
        for (int i = 0; i < k; ++i) {
          const int u = i + j, v = i + j + k;
          if (v < N && u / (2 * p) == v / (2 * p)) {
            const float x = a[u], y = a[v];
            a[u] = fminf(x, y);
            a[v] = fmaxf(x, y);
          }
        }
      }
    }
  }
  lo = a[N / 2 - 1];
  hi = a[N / 2];
}

// the ring walk (k_defect.h walks the same way): a[] = the ring of the lane's sample, row by row, and the sample itself
// is returned. `p` = the lane's sample in its row (FAST) or the image (general: row offsets yo[], flat column offsets
// xo[])
template <int R, bool FAST>
__device__ __forceinline__ float despike_ring(float (&a)[8 * R], const float* p, ptrdiff_t W, int ch, const ptrdiff_t* yo,
                                              const int* xo) {
  int n = 0;
#pragma unroll
  for (int dy = -R; dy <= R; ++dy) {
#pragma unroll
    for (int dx = -R; dx <= R; ++dx) {
      if (dx != -R && dx != R && dy != -R && dy != R) continue;
      a[n++] = FAST ? p[dy * W + dx * ch] : p[yo[dy + R] + xo[dx + R]];
    }
  }
  return FAST ? p[0] : p[yo[R] + xo[R]];
}

// the ring's minimum and maximum, and nf: 0 while v and the ring are finite, NaN otherwise
template <int N>
__device__ __forceinline__ void despike_range(const float (&a)[N], float v, float& mn, float& mx, float& nf) {
  mn = a[0], mx = a[0], nf = __builtin_fmaf(v, 0.f, a[0] * 0.f);
#pragma unroll
  for (int k = 1; k < N; ++k) {
    mn = fminf(mn, a[k]);
    mx = fmaxf(mx, a[k]);
    nf = __builtin_fmaf(a[k], 0.f, nf);
  }
}

// one sample per lane (p, W, ch, yo, xo: as despike_ring's); returns what goes to out, hit = it was replaced
template <int R, bool FAST>
__device__ __forceinline__ float despike_sample(const float* p, ptrdiff_t W, int ch, const ptrdiff_t* yo, const int* xo,
                                                float thr, bool& hit) {
#pragma clang fp contract(off)
  constexpr int N = 8 * R;
  float a[N];
  const float v = despike_ring<R, FAST>(a, p, W, ch, yo, xo);
  float mn, mx, nf;
  despike_range<N>(a, v, mn, mx, nf);
  hit = nf == 0.f && (v > mx + thr || v < mn - thr);
  float r = v;
  if (__builtin_amdgcn_ballot_w64(hit) != 0) {  // wave-uniform
    float lo, hi;
    despike_middle<N>(a, lo, hi);
    if (hit) r = (lo + hi) * 0.5f;
  }
  return r;
}

// grid: nbx * ceil(h / DESPIKE_ROWS) workgroups, nbx = ceil(w ch / DESPIKE_THREADS); count: nullptr, or ch words (zeroed)
template <int R>
__global__ __launch_bounds__(DESPIKE_THREADS) void k_despike(float* __restrict__ out, const float* __restrict__ in,
                                                             uint32_t* count, int w, int h, int ch, float thr, int nbx) {
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
    bool hit;
    float r;
    if (cols_in && y >= R && y < h - R) {
      r = despike_sample<R, true>(in + (size_t)y * W + fc, W, ch, nullptr, nullptr, thr, hit);
    } else {
      ptrdiff_t yo[2 * R + 1];
#pragma unroll
      for (int d = -R; d <= R; ++d) yo[d + R] = (ptrdiff_t)despike_reflect(y + d, h) * W;
      r = despike_sample<R, false>(in, W, ch, yo, xo, thr, hit);
    }
    hit = hit && live;
    if (live) out[(size_t)y * W + f] = r;
    if (count && __builtin_amdgcn_ballot_w64(hit) != 0) {  // (wave-uniform) one atomic per channel with a hit
      for (int k = 0; k < ch; ++k) {
        const uint64_t m = __builtin_amdgcn_ballot_w64(hit && c == k);
        if (m != 0 && (threadIdx.x & 63) == 0) atomicAdd(count + k, (uint32_t)__popcll(m));
      }
    }
  }
}
