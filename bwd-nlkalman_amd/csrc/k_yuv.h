// k_yuv.h — planar Y'CbCr frames <-> the HWC float RGB image (nlk_dev_yuv_to_rgb / nlk_dev_rgb_to_yuv,
// include/nlk_hip.h; the arithmetic is written out in DESIGN.md §9 and restated in numpy by tests/yuv_ref.py).
//
// Both kernels are one pass, write-dominated in one direction and read-dominated in the other (1080p 4:2:0 8 bit:
// 3.1 MB of codes against 24.9 MB of floats). A thread owns 4 x 2 luma pixels: its RGB rows are three 16-byte
// accesses each (one for mono), its 8-bit luma rows one dword each, and the chroma samples it needs (4 x 3 per plane
// at 4:2:0) are converted once and shared by its 8 pixels. The code planes are small enough to stay in L2, so the
// chroma neighbours are read from there and not staged in LDS. Every index is clamped to its plane, which is all an
// image edge needs; a block that hangs over the right or bottom edge, and a code row that does not start on a dword,
// take element accesses with the same arithmetic.
//
// float32, one rounding per operation, in the order written: no contraction (this file's pragma), no division.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#pragma clang fp contract(off)

#define NLK_YUV_BX 64  // threads of a workgroup along x (4 luma pixels each) ...
#define NLK_YUV_BY 4   // ... and along y (2 luma rows each): 256 x 8 pixels

// made in double on the host, rounded to float once (tu_yuv.hip)
struct NlkYuvK {
  float y0, ky, c0, kc;        // code -> value: (code - y0) * ky, (code - c0) * kc
  float crr, cbu, cgu, cgv;    // R = y + crr v, B = y + cbu u, G = (y - cgu u) - cgv v
  float kr, kg, kb;            // y = (kr R + kg G) + kb B
  float icbu, icrr, iky, ikc;  // u = (B - y) icbu, v = (R - y) icrr; value -> code: rint(y iky + y0), rint(u ikc + c0)
  float maxc;                  // 2^depth - 1
};

// a float4 that only promises the alignment of a float: rows of an HWC image start anywhere (global 16-byte accesses
// need dword alignment only)
typedef float nlk_yuv_f4 __attribute__((ext_vector_type(4), aligned(4)));

__device__ __forceinline__ int nlk_yuv_clamp(int i, int n) { return i < 0 ? 0 : (i > n - 1 ? n - 1 : i); }

// samples x0 .. x0 + 3 of a code row as floats; `n` of them exist (the others come back as 0). Four of them on a
// dword boundary are one or two dword loads.
template <typename T>
__device__ __forceinline__ void nlk_yuv_load4(const T* p, int n, float (&v)[4]) {
  if (n == 4 && ((uintptr_t)p & 3) == 0) {
    if (sizeof(T) == 1) {
      const uint32_t q = *reinterpret_cast<const uint32_t*>(p);
      v[0] = (float)(q & 0xffu); v[1] = (float)((q >> 8) & 0xffu); v[2] = (float)((q >> 16) & 0xffu); v[3] = (float)(q >> 24);
    } else {
      const uint32_t q0 = reinterpret_cast<const uint32_t*>(p)[0], q1 = reinterpret_cast<const uint32_t*>(p)[1];
      v[0] = (float)(q0 & 0xffffu); v[1] = (float)(q0 >> 16); v[2] = (float)(q1 & 0xffffu); v[3] = (float)(q1 >> 16);
    }
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = k < n ? (float)p[k] : 0.f;
  }
}

template <typename T>
__device__ __forceinline__ void nlk_yuv_store4(T* p, int n, const uint32_t (&c)[4]) {
  if (n == 4 && ((uintptr_t)p & 3) == 0) {
    if (sizeof(T) == 1) {
      *reinterpret_cast<uint32_t*>(p) = c[0] | (c[1] << 8) | (c[2] << 16) | (c[3] << 24);
    } else {
      reinterpret_cast<uint32_t*>(p)[0] = c[0] | (c[1] << 16);
      reinterpret_cast<uint32_t*>(p)[1] = c[2] | (c[3] << 16);
    }
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (k < n) p[k] = (T)c[k];
  }
}

// the code of a value: round to nearest even, clamp to the code range; a NaN gives 0 (fmaxf returns the other operand)
__device__ __forceinline__ uint32_t nlk_yuv_code(float v, float ik, float off, float maxc) {
  const float t = rintf(v * ik + off);
  return (uint32_t)fminf(fmaxf(t, 0.f), maxc);
}

// one chroma row interpolated to the luma columns x0 .. x0 + 3 (x0 a multiple of 4): the samples are converted, then
// centred: 3/4 near + 1/4 far (far = i - 1 left of an even column, i + 1 right of an odd one); co-sited: the sample on
// an even column, the mean of two on an odd one
template <typename T, int SX, bool COS>
__device__ __forceinline__ void nlk_yuv_chroma_row(const T* row, int cw, int x0, float c0, float kc, float (&o)[4]) {
  if (SX == 1) {
#pragma unroll
    for (int k = 0; k < 4; ++k) o[k] = ((float)row[nlk_yuv_clamp(x0 + k, cw)] - c0) * kc;
    return;
  }
  const int i0 = x0 >> 1;
  float s[4];  // samples i0 - 1 .. i0 + 2
#pragma unroll
  for (int m = 0; m < 4; ++m) s[m] = ((float)row[nlk_yuv_clamp(i0 - 1 + m, cw)] - c0) * kc;
  if (COS) {
    o[0] = s[1];
    o[1] = (s[1] + s[2]) * 0.5f;
    o[2] = s[2];
    o[3] = (s[2] + s[3]) * 0.5f;
  } else {
    o[0] = 0.75f * s[1] + 0.25f * s[0];
    o[1] = 0.75f * s[1] + 0.25f * s[2];
    o[2] = 0.75f * s[2] + 0.25f * s[1];
    o[3] = 0.75f * s[2] + 0.25f * s[3];
  }
}

// one chroma plane at the 4 x 2 luma pixels from (x0, y0), y0 even: rows first, then (SY == 2) 3/4 of the near row
// + 1/4 of the far one (j - 1 above an even luma row, j + 1 below an odd one)
template <typename T, int SX, int SY, bool COS>
__device__ __forceinline__ void nlk_yuv_chroma_block(const T* plane, int cw, int chh, int x0, int y0, float c0, float kc,
                                                     float (&o)[2][4]) {
  if (SY == 1) {
    nlk_yuv_chroma_row<T, SX, COS>(plane + (size_t)nlk_yuv_clamp(y0, chh) * cw, cw, x0, c0, kc, o[0]);
    nlk_yuv_chroma_row<T, SX, COS>(plane + (size_t)nlk_yuv_clamp(y0 + 1, chh) * cw, cw, x0, c0, kc, o[1]);
    return;
  }
  const int j = y0 >> 1;
  float up[4], mid[4], dn[4];
  nlk_yuv_chroma_row<T, SX, COS>(plane + (size_t)nlk_yuv_clamp(j - 1, chh) * cw, cw, x0, c0, kc, up);
  nlk_yuv_chroma_row<T, SX, COS>(plane + (size_t)j * cw, cw, x0, c0, kc, mid);
  nlk_yuv_chroma_row<T, SX, COS>(plane + (size_t)nlk_yuv_clamp(j + 1, chh) * cw, cw, x0, c0, kc, dn);
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    o[0][k] = 0.75f * mid[k] + 0.25f * up[k];
    o[1][k] = 0.75f * mid[k] + 0.25f * dn[k];
  }
}

template <typename T, int SX, int SY, bool COS, bool MONO>
__global__ __launch_bounds__(NLK_YUV_BX * NLK_YUV_BY) void k_yuv_to_rgb(float* __restrict__ rgb, const T* __restrict__ yuv,
                                                                       int w, int h, NlkYuvK k) {
  const int x0 = (blockIdx.x * NLK_YUV_BX + threadIdx.x) * 4, y0 = (blockIdx.y * NLK_YUV_BY + threadIdx.y) * 2;
  if (x0 >= w || y0 >= h) return;
  const int nx = w - x0 < 4 ? w - x0 : 4, ny = h - y0 < 2 ? h - y0 : 2;
  float yy[2][4];
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    if (r >= ny) break;
    float c[4];
    nlk_yuv_load4<T>(yuv + (size_t)(y0 + r) * w + x0, nx, c);
#pragma unroll
    for (int i = 0; i < 4; ++i) yy[r][i] = (c[i] - k.y0) * k.ky;
  }
  if (MONO) {
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      if (r >= ny) break;
      float* o = rgb + (size_t)(y0 + r) * w + x0;
      if (nx == 4) {
        *reinterpret_cast<nlk_yuv_f4*>(o) = nlk_yuv_f4{yy[r][0], yy[r][1], yy[r][2], yy[r][3]};
      } else {
#pragma unroll
        for (int i = 0; i < 4; ++i)
          if (i < nx) o[i] = yy[r][i];
      }
    }
    return;
  }
  const int cw = (w + SX - 1) / SX, chh = (h + SY - 1) / SY;
  const T* cb = yuv + (size_t)w * h;
  const T* cr = cb + (size_t)cw * chh;
  float uu[2][4], vv[2][4];
  nlk_yuv_chroma_block<T, SX, SY, COS>(cb, cw, chh, x0, y0, k.c0, k.kc, uu);
  nlk_yuv_chroma_block<T, SX, SY, COS>(cr, cw, chh, x0, y0, k.c0, k.kc, vv);
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    if (r >= ny) break;
    float px[12];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float y = yy[r][i], u = uu[r][i], v = vv[r][i];
      px[3 * i] = y + k.crr * v;
      px[3 * i + 1] = (y - k.cgu * u) - k.cgv * v;
      px[3 * i + 2] = y + k.cbu * u;
    }
    float* o = rgb + ((size_t)(y0 + r) * w + x0) * 3;
    if (nx == 4) {
      nlk_yuv_f4* o4 = reinterpret_cast<nlk_yuv_f4*>(o);
      o4[0] = nlk_yuv_f4{px[0], px[1], px[2], px[3]};
      o4[1] = nlk_yuv_f4{px[4], px[5], px[6], px[7]};
      o4[2] = nlk_yuv_f4{px[8], px[9], px[10], px[11]};
    } else {
#pragma unroll
      for (int i = 0; i < 12; ++i)
        if (i < 3 * nx) o[i] = px[i];
    }
  }
}

// y, u, v of one RGB pixel
__device__ __forceinline__ void nlk_yuv_from_rgb(const NlkYuvK& k, float R, float G, float B, float& y, float& u, float& v) {
  y = (k.kr * R + k.kg * G) + k.kb * B;
  u = (B - y) * k.icbu;
  v = (R - y) * k.icrr;
}

template <typename T, int SX, int SY, bool COS, bool MONO>
__global__ __launch_bounds__(NLK_YUV_BX * NLK_YUV_BY) void k_rgb_to_yuv(T* __restrict__ yuv, const float* __restrict__ rgb,
                                                                       int w, int h, NlkYuvK k) {
  const int x0 = (blockIdx.x * NLK_YUV_BX + threadIdx.x) * 4, y0 = (blockIdx.y * NLK_YUV_BY + threadIdx.y) * 2;
  if (x0 >= w || y0 >= h) return;
  const int nx = w - x0 < 4 ? w - x0 : 4, ny = h - y0 < 2 ? h - y0 : 2;
  if (MONO) {
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      if (r >= ny) break;
      const float* in = rgb + (size_t)(y0 + r) * w + x0;
      float g[4];
      if (nx == 4) {
        const nlk_yuv_f4 q = *reinterpret_cast<const nlk_yuv_f4*>(in);
        g[0] = q.x; g[1] = q.y; g[2] = q.z; g[3] = q.w;
      } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) g[i] = i < nx ? in[i] : 0.f;
      }
      uint32_t c[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) c[i] = nlk_yuv_code(g[i], k.iky, k.y0, k.maxc);
      nlk_yuv_store4<T>(yuv + (size_t)(y0 + r) * w + x0, nx, c);
    }
    return;
  }
  // y, u, v of the columns x0 .. x0 + 3 on the rows y0 and min(y0 + 1, h - 1), columns clamped to the image (a
  // clamped column or row is the replicated sample the decimation asks for), and of the column left of the block
  // where the co-sited filter reaches it
  float yy[2][4], uu[2][4], vv[2][4], ul[2], vl[2];
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    const float* row = rgb + (size_t)nlk_yuv_clamp(y0 + r, h) * w * 3;
    float px[12];
    if (nx == 4) {
      const nlk_yuv_f4* in4 = reinterpret_cast<const nlk_yuv_f4*>(row + (size_t)x0 * 3);
      const nlk_yuv_f4 a = in4[0], b = in4[1], c = in4[2];
      px[0] = a.x; px[1] = a.y; px[2] = a.z; px[3] = a.w;
      px[4] = b.x; px[5] = b.y; px[6] = b.z; px[7] = b.w;
      px[8] = c.x; px[9] = c.y; px[10] = c.z; px[11] = c.w;
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float* p = row + (size_t)nlk_yuv_clamp(x0 + i, w) * 3;
        px[3 * i] = p[0]; px[3 * i + 1] = p[1]; px[3 * i + 2] = p[2];
      }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) nlk_yuv_from_rgb(k, px[3 * i], px[3 * i + 1], px[3 * i + 2], yy[r][i], uu[r][i], vv[r][i]);
    if (SX == 2 && COS) {
      const float* p = row + (size_t)nlk_yuv_clamp(x0 - 1, w) * 3;
      float yl;
      nlk_yuv_from_rgb(k, p[0], p[1], p[2], yl, ul[r], vl[r]);
    }
  }
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    if (r >= ny) break;
    uint32_t c[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) c[i] = nlk_yuv_code(yy[r][i], k.iky, k.y0, k.maxc);
    nlk_yuv_store4<T>(yuv + (size_t)(y0 + r) * w + x0, nx, c);
  }
  // chroma: decimated along the rows first, then across the two rows
  const int cw = (w + SX - 1) / SX, chh = (h + SY - 1) / SY;
  T* cb = yuv + (size_t)w * h;
  T* cr = cb + (size_t)cw * chh;
  constexpr int NC = 4 / SX;              // chroma samples of the block per row ...
  const int ncx = (nx + SX - 1) / SX;     // ... of which these exist
  float hu[2][NC], hv[2][NC];
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    if (SX == 1) {
#pragma unroll
      for (int i = 0; i < NC; ++i) { hu[r][i] = uu[r][i]; hv[r][i] = vv[r][i]; }
    } else if (COS) {
      hu[r][0] = (0.25f * ul[r] + 0.5f * uu[r][0]) + 0.25f * uu[r][1];
      hu[r][NC - 1] = (0.25f * uu[r][1] + 0.5f * uu[r][2]) + 0.25f * uu[r][3];
      hv[r][0] = (0.25f * vl[r] + 0.5f * vv[r][0]) + 0.25f * vv[r][1];
      hv[r][NC - 1] = (0.25f * vv[r][1] + 0.5f * vv[r][2]) + 0.25f * vv[r][3];
    } else {
      hu[r][0] = (uu[r][0] + uu[r][1]) * 0.5f;
      hu[r][NC - 1] = (uu[r][2] + uu[r][3]) * 0.5f;
      hv[r][0] = (vv[r][0] + vv[r][1]) * 0.5f;
      hv[r][NC - 1] = (vv[r][2] + vv[r][3]) * 0.5f;
    }
  }
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    if (SY == 2 ? r > 0 : r >= ny) break;
    uint32_t cu[4] = {0, 0, 0, 0}, cv[4] = {0, 0, 0, 0};
#pragma unroll
    for (int i = 0; i < NC; ++i) {
      const float u = SY == 2 ? (hu[0][i] + hu[1][i]) * 0.5f : hu[r][i];
      const float v = SY == 2 ? (hv[0][i] + hv[1][i]) * 0.5f : hv[r][i];
      cu[i] = nlk_yuv_code(u, k.ikc, k.c0, k.maxc);
      cv[i] = nlk_yuv_code(v, k.ikc, k.c0, k.maxc);
    }
    const size_t at = (size_t)(SY == 2 ? (y0 >> 1) : y0 + r) * cw + x0 / SX;
    nlk_yuv_store4<T>(cb + at, ncx, cu);  // (ncx <= 2 at SX == 2: element stores)
    nlk_yuv_store4<T>(cr + at, ncx, cv);
  }
}
