// k_group_math.h — the per-coefficient model of the group kernels, stated once: the three gains with the variance
// term that becomes the aggregation weight, the Welford step and the shrinkage of the LDS-DCT kernel, the weight.
// How a kernel forms v1 / v0 / v01n from its own sums, where it keeps the mean and how it exchanges the results
// between lanes is layout and stays in the kernel. The float expressions are the ones every kernel had; keep their
// operand order (contraction into FMAs follows the expression).
#pragma once
#include "nlk_common.h"

// Gain a of one coefficient and its share `term` of the group's variance (the weight is 1 / their sum).
//   MODE 0  Wiener, no valid previous patch   reference: src/nlkalman.c:799-811
//   MODE 1  Kalman                            reference: :859-904
//   MODE 2  RTS smoother                      reference: :1683-1776
// v1: variance of the image coefficients, v0: of the previous frame's, v01n: mean squared difference of the two.
// RCP: n * rcp(d) instead of n / d (k_group8m).
template <int MODE, bool RCP>
__device__ __forceinline__ void nlk_gain(float v1, float v0, float v01n, const NlkGeom& g, float s2, float& a,
                                         float& term) {
  auto ratio = [](float n, float d) { return RCP ? n * __builtin_amdgcn_rcpf(d) : n / d; };
  if (MODE == 2) {
    a = ratio(v1, v1 + g.beta_t * v01n);
    const float pv = v0 - g.beta_t * v01n;
    term = (1 - a * a) * v1 + a * a * (pv > 0.f ? pv : 0.f);
  } else if (MODE == 1) {
    const float d = v01n - (g.have_basic ? 0.f : s2);
    const float v = v0 + (0.f > d ? 0.f : d);
    a = ratio(v, v + g.beta_t * s2);
    term = (1 - a * a) * v + a * a * s2;
  } else {
    const float d = v1 - (g.have_basic ? 0.f : s2);
    const float v = 0.f > d ? 0.f : d;
    a = ratio(v, v + g.beta_x * s2);
    term = a * v;
  }
}

// Weight of a group from the sum of its coefficients' terms: the reference adds the same terms once per group
// member; a smoother group without a valid previous patch passes its pixels through (reference: :1795-1804).
__device__ __forceinline__ float nlk_group_weight(float term_sum, int nagg, bool passthrough) {
  float vp = term_sum * (float)nagg;
  if (passthrough) vp = 0.f;
  return 1.f / (vp > 1e-6f ? vp : 1e-6f);
}

// Running statistics of one coefficient in the LDS-DCT kernel (k_group_lds.h).
struct NlkStat {
  float M0 = 0.f, M0V = 0.f, V0 = 0.f, V01 = 0.f, M1 = 0.f, V1 = 0.f;
};

// Welford step for a candidate's image coefficient a and, where its previous patch is valid (v), previous-frame
// coefficient b; inp1 / inp0 = 1 / (candidates so far, with a valid previous patch). The filter keeps the mean of
// the group members (M0) apart from the mean of all candidates (M0V); the smoother has one.
template <bool SMO>
__device__ __forceinline__ void nlk_welford(NlkStat& s, float a, float b, bool v, bool in_group, float inp1,
                                            float inp0) {
  const float d1 = a - s.M1;
  s.M1 += d1 * inp1;
  s.V1 += d1 * (a - s.M1);
  if (v) {
    if (SMO) {  // reference: :1659-1667
      const float d0 = b - s.M0;
      s.M0 += d0 * inp0;
      s.V0 += d0 * (b - s.M0);
    } else {    // reference: :769-783
      const float d0 = b - s.M0V;
      s.M0V += d0 * inp0;
      s.V0 += d0 * (b - s.M0V);
      if (in_group) s.M0 += (b - s.M0) * inp0;
    }
    const float tt = b - a;
    s.V01 += tt * tt;
  }
}

// Shrinkage of a member's coefficient A: towards its previous-frame coefficient B in the smoother, towards the
// group mean in the filter (reference: :879, :902).
template <bool SMO>
__device__ __forceinline__ float nlk_shrink(float a, float A, float B, float mean) {
  return SMO ? (1 - a) * A + a * B : a * A + (1 - a) * mean;
}
