// k_group_lds.h — per-target group processing with the DCTs in LDS: gather the kept patches, 2-D DCT, Welford
// statistics, Kalman / Wiener (or RTS-smoother) gain, shrinkage of the group members, inverse DCT and weighted
// aggregation (reference: src/nlkalman.c:713-932 filter, :1603-1845 smoother; the model itself: k_group_math.h).
//
// One workgroup per active target. Thread `tid` owns the coefficients e = tid + NT * r of the ch * psz^2 coefficient
// vector for the whole call, so the running statistics, gains and shrinkage are thread-local register work; only
// the small separable DCTs cross threads, through LDS with the psz x psz basis resident in LDS (no FFTW). Group
// members are re-transformed in a second pass once the gains are known, so no per-group coefficient store is needed
// and the group size is unbounded (the smoother's 105 slots at sigma = 40 included). Slow next to k_groupp /
// k_group8m (no data reuse, one target per workgroup, atomics to HBM for every member pixel): the path of the
// lists of more than 128 entries and of the shapes the tuned kernels are not built for.
//
// The kernel body is written once; a shape policy says how big things are and how coefficient e splits into
// (channel c, row i, column j):
//   GroupFixed<PSZ, CH>  compile-time sizes, one wavefront, (c, i, j) recomputed by constant division where they are
//                        used, static LDS, the next candidate's pixels requested while this one is transformed
//   GroupAny             sizes from NlkGeom (patches up to 32 x 32, any channel count with ch * psz^2 <= 4096),
//                        four wavefronts, (c, i, j) kept in registers, dynamic LDS, no prefetch
// The fixed shapes sit next to occupancy steps (8 x 8 x 3: 66 VGPRs, 12 x 12 x 3: 157): what the policy hands the
// compiler decides on which side they land, so GroupFixed gives it constants and nothing to keep.
#pragma once
#include "k_group_math.h"

template <int PSZ, int CH>
struct GroupFixed {
  static constexpr int NT = 64, psz = PSZ, ch = CH, p2 = PSZ * PSZ, E = CH * p2, NR = (E + NT - 1) / NT;
  static constexpr bool PREFETCH = true;
  __device__ GroupFixed(const NlkGeom&, int) {}
  static __device__ __forceinline__ float* lds() {
    __shared__ __attribute__((aligned(16))) float buf[3 * p2 + 4 * E];
    return buf;
  }
  __device__ __forceinline__ void split(int e, int, int& c, int& i, int& j) const {
    const int rem = e % p2;
    c = e / p2, i = rem / PSZ, j = rem % PSZ;
  }
  __device__ __forceinline__ int win(int e, int) const { return e % p2; }    // index into the window
  __device__ __forceinline__ bool plane0(int e, int) const { return e < p2; }  // first channel: carries the weight
};

struct GroupAny {
  static constexpr int NT = 256, NR = 16;
  static constexpr bool PREFETCH = false;
  const int psz, ch, p2, E;
  int ec[NR], ei[NR], ej[NR];
  __device__ GroupAny(const NlkGeom& g, int tid) : psz(g.psz), ch(g.ch), p2(g.p2), E(g.E) {
#pragma unroll
    for (int r = 0; r < NR; ++r) {
      const int e = tid + NT * r, ee = e < E ? e : 0;
      ec[r] = ee / p2;
      const int rem = ee - ec[r] * p2;
      ei[r] = rem / psz;
      ej[r] = rem - ei[r] * psz;
    }
  }
  static __host__ __device__ size_t lds_bytes(const NlkGeom& g) {
    return sizeof(float) * (3 * (size_t)g.p2 + 4 * (size_t)g.E + NT / 64);
  }
  static __device__ __forceinline__ float* lds() {
    extern __shared__ __attribute__((aligned(16))) float dyn[];  // lds_bytes()
    return dyn;
  }
  __device__ __forceinline__ void split(int, int r, int& c, int& i, int& j) const { c = ec[r], i = ei[r], j = ej[r]; }
  __device__ __forceinline__ int win(int, int r) const { return ei[r] * psz + ej[r]; }
  __device__ __forceinline__ bool plane0(int, int r) const { return ec[r] == 0; }
};

constexpr int NLK_ANY_EMAX = GroupAny::NT * GroupAny::NR;  // largest ch * psz^2 of the run-time shape

// Separable 2-D transform of NSET coefficient sets held one element per (thread, r). tab = DCT basis C (forward) or
// its transpose (inverse):
//   pass 1: T[c][j][i] = sum_k X[c][i][k] * tab[j][k]
//   pass 2: Y[c][i][j] = sum_k tab[i][k] * T[c][j][k]
template <int NSET, class S>
__device__ inline void nlk_dct2d(const S& sh, const float* __restrict__ tab, float* __restrict__ X,
                                 float* __restrict__ T, float (&val)[NSET][S::NR], int tid) {
  const int psz = sh.psz, p2 = sh.p2, E = sh.E;
#pragma unroll
  for (int s = 0; s < NSET; ++s)
#pragma unroll
    for (int r = 0; r < S::NR; ++r) {
      const int e = tid + S::NT * r;
      if (e < E) X[s * E + e] = val[s][r];
    }
  __syncthreads();
#pragma unroll
  for (int s = 0; s < NSET; ++s)
#pragma unroll
    for (int r = 0; r < S::NR; ++r) {
      const int e = tid + S::NT * r;
      if (e < E) {
        int c, i, j;
        sh.split(e, r, c, i, j);
        const float* x = X + s * E + c * p2 + i * psz;
        const float* b = tab + j * psz;
        float acc = 0.f;
        for (int k = 0; k < psz; ++k) acc = fmaf(x[k], b[k], acc);
        T[s * E + c * p2 + j * psz + i] = acc;
      }
    }
  __syncthreads();
#pragma unroll
  for (int s = 0; s < NSET; ++s)
#pragma unroll
    for (int r = 0; r < S::NR; ++r) {
      const int e = tid + S::NT * r;
      if (e < E) {
        int c, i, j;
        sh.split(e, r, c, i, j);
        const float* b = tab + i * psz;
        const float* tt = T + s * E + c * p2 + j * psz;
        float acc = 0.f;
        for (int k = 0; k < psz; ++k) acc = fmaf(b[k], tt[k], acc);
        val[s][r] = acc;
      }
    }
  __syncthreads();
}

template <class S, bool SMO>
__global__ void __launch_bounds__(S::NT)
k_group_lds(const float* __restrict__ img,   // matching / statistics image (planar)
            const float* __restrict__ cur,   // image whose patches are filtered
            const float* __restrict__ prev,  // previous output or nullptr
            const uint8_t* __restrict__ vmap, NlkGeom g, const uint32_t* __restrict__ topk,
            const NlkTarget* __restrict__ tinfo, const uint32_t* __restrict__ gcoords,
            const uint8_t* __restrict__ active,
            const float* __restrict__ basis,   // [psz][psz] orthonormal DCT-II
            const float* __restrict__ window,  // [psz][psz] aggregation window
            float* __restrict__ acc) {
  constexpr int NR = S::NR, NT = S::NT;
  const int t = blockIdx.x;
  if (!active[t]) return;
  const NlkTarget info = tinfo[t];
  if (info.nagg == 0) return;
  const int tid = threadIdx.x;
  const S sh(g, tid);
  const int psz = sh.psz, p2 = sh.p2, E = sh.E;
  float* Cm = S::lds();    // C[k][j]
  float* Ct = Cm + p2;     // C^T
  float* Wn = Ct + p2;     // window
  float* X = Wn + p2;      // [2][E]
  float* T = X + 2 * E;    // [2][E]
  float* red = T + 2 * E;  // [NT / 64], only with more than one wavefront
  for (int i = tid; i < p2; i += NT) {
    const float b = basis[i];
    Cm[i] = b;
    Ct[(i % psz) * psz + i / psz] = b;
    Wn[i] = window[i];
  }
  __syncthreads();

  const size_t npix = (size_t)g.w * g.h;
  int poff[NR];   // offset of the element inside a planar image, relative to the patch origin
  bool live[NR];
#pragma unroll
  for (int r = 0; r < NR; ++r) {
    const int e = tid + NT * r;
    live[r] = e < E;
    int c, i, j;
    sh.split(live[r] ? e : 0, r, c, i, j);
    poff[r] = c * (int)npix + i * g.w + j;
  }
  const bool prev_p = info.flags & 1;
  const int k = info.nsel;
  const float s2 = g.sigma2;

  // ---------------- pass A: statistics over the k kept candidates
  NlkStat st[NR];
  int np0 = 0, np1 = 0;
  float val[2][NR], nxt[2][NR];
  bool vnext = false;
  auto gather = [&](int i, float (&dst)[2][NR], bool& v) {
    const uint32_t q = topk[(size_t)t * g.kmax + i];
    const int org = nlk_y(q) * g.w + nlk_x(q);
    v = prev_p && vmap[org];
#pragma unroll
    for (int r = 0; r < NR; ++r) {
      dst[0][r] = live[r] ? img[org + poff[r]] : 0.f;
      dst[1][r] = (live[r] && v) ? prev[org + poff[r]] : 0.f;
    }
  };
  if (S::PREFETCH && k > 0) gather(0, nxt, vnext);
  for (int i = 0; i < k; ++i) {
    bool v;
    if (S::PREFETCH) {
      v = vnext;
#pragma unroll
      for (int r = 0; r < NR; ++r) { val[0][r] = nxt[0][r]; val[1][r] = nxt[1][r]; }
      if (i + 1 < k) gather(i + 1, nxt, vnext);
    } else {
      gather(i, val, v);
    }
    if (v) nlk_dct2d<2>(sh, Cm, X, T, val, tid);
    else {
      float (&one)[1][NR] = reinterpret_cast<float (&)[1][NR]>(val);
      nlk_dct2d<1>(sh, Cm, X, T, one, tid);
    }
    np1++;
    const float inp1 = 1.f / (float)np1;
    float inp0 = 0.f;
    bool in_group = false;
    if (v) {
      np0++;
      inp0 = 1.f / (float)np0;
      in_group = np0 <= g.ntagg;
    }
#pragma unroll
    for (int r = 0; r < NR; ++r) nlk_welford<SMO>(st[r], val[0][r], val[1][r], v, in_group, inp1, inp0);
  }

  // ---------------- gains
  const int nagg = info.nagg;
  float gain[NR], mean[NR];
  float part = 0.f;
  {
    const float inp1 = np1 ? 1.f / (float)np1 : 0.f;
    const float inp0 = np0 ? 1.f / (float)np0 : 0.f;
#pragma unroll
    for (int r = 0; r < NR; ++r) {
      const float v1 = st[r].V1 * inp1;
      const float v0 = np0 ? st[r].V0 * inp0 : st[r].V0;
      const float v01 = np0 ? st[r].V01 * inp0 : st[r].V01;
      float a, term;
      if (SMO) {
        nlk_gain<2, false>(v1, v0, v01, g, s2, a, term);
        mean[r] = 0.f;
      } else if (np0 > 0) {
        nlk_gain<1, false>(v1, v0, v01, g, s2, a, term);
        mean[r] = st[r].M0;
      } else {
        nlk_gain<0, false>(v1, v0, v01, g, s2, a, term);
        mean[r] = st[r].M1;
      }
      gain[r] = a;
      if (live[r]) part += term;
    }
  }
  // sum of the terms over the workgroup: a butterfly inside the wavefront, then the wavefronts' sums in order
  for (int off = 32; off > 0; off >>= 1) part += __shfl_xor(part, off, 64);
  if (NT > 64) {
    if ((tid & 63) == 0) red[tid >> 6] = part;
    __syncthreads();
    part = 0.f;
    for (int i = 0; i < NT / 64; ++i) part += red[i];
  }
  const bool passthrough = SMO && np0 == 0;
  const float wgt = nlk_group_weight(part, nagg, passthrough);

  // ---------------- pass B: shrink, invert and aggregate the group members
  const float* src = g.have_basic ? cur : img;
  for (int n = 0; n < nagg; ++n) {
    const uint32_t q = gcoords[(size_t)t * g.gstride + n];
    const int org = nlk_y(q) * g.w + nlk_x(q);
    float out[NR];
    if (passthrough) {
#pragma unroll
      for (int r = 0; r < NR; ++r) out[r] = live[r] ? cur[org + poff[r]] : 0.f;
    } else {
#pragma unroll
      for (int r = 0; r < NR; ++r) {
        val[0][r] = live[r] ? src[org + poff[r]] : 0.f;
        val[1][r] = (SMO && live[r]) ? prev[org + poff[r]] : 0.f;
      }
      if (SMO) nlk_dct2d<2>(sh, Cm, X, T, val, tid);
      else {
        float (&one)[1][NR] = reinterpret_cast<float (&)[1][NR]>(val);
        nlk_dct2d<1>(sh, Cm, X, T, one, tid);
      }
      float y[1][NR];
#pragma unroll
      for (int r = 0; r < NR; ++r) y[0][r] = nlk_shrink<SMO>(gain[r], val[0][r], val[1][r], mean[r]);
      nlk_dct2d<1>(sh, Ct, X, T, y, tid);
#pragma unroll
      for (int r = 0; r < NR; ++r) out[r] = y[0][r];
    }
#pragma unroll
    for (int r = 0; r < NR; ++r) {
      if (live[r]) {
        const int e = tid + NT * r;
        const float ww = wgt * Wn[sh.win(e, r)];
        unsafeAtomicAdd(acc + org + poff[r], ww * out[r]);
        if (sh.plane0(e, r)) unsafeAtomicAdd(acc + (size_t)sh.ch * npix + org + poff[r], ww);
      }
    }
  }
}
