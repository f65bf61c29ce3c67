// The box rules of the refit (hgs.hierarchy.refit_boxes, the spec; hier_refit.hip runs them), each ONCE and for host and
// device alike: the two leaf rules, the union, the extent, the test a leaf box has to pass.  Plain C++ behind the
// qualifiers: tests/test_hier_refit_rule_on_host.py compiles this file with g++.
//
//   cube       s_k = exp(double(log_scales_k)), e = 3 max_k s_k (a NaN anywhere gives NaN), lo_a = f32(x_a - e),
//              hi_a = f32(x_a + e): the builder's leaf rule on the stored rows
//   ellipsoid  q^ = q / |q|, |q| = sqrt(((w w + x x) + y y) + z z); R = _rot_from_quat(q^);
//              h_a = 3 sqrt(((R_a0 R_a0) v_0 + (R_a1 R_a1) v_1) + (R_a2 R_a2) v_2), v_k = s_k s_k;
//              lo_a = f32(x_a - h_a), hi_a = f32(x_a + h_a): the AABB of the 3 sigma ellipsoid
//   union      min / max per coordinate (exact)
//   extent     max_a (hi_a - lo_a), a float32 subtraction on the rounded values
// Double arithmetic, every sum left to right, no contraction, one rounding to float32.  The one operation a host and the
// device may round differently is exp (sqrt and the division are correctly rounded on both).
#pragma once
#include "common.h"

#include <math.h>

namespace hgs {

constexpr int32_t kRefitKeep = 0, kRefitCube = 1, kRefitEllipsoid = 2;

// The largest of three; a NaN among them wins (comparisons alone would skip it).
__host__ __device__ __forceinline__ double refit_max3(double a, double b, double c) {
  double m = a;
  m = (b > m || b != b) ? b : m;
  m = (c > m || c != c) ? c : m;
  return m;
}

__host__ __device__ __forceinline__ void refit_leaf_cube(const double x[3], const double ls[3], float lo[3], float hi[3]) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const double e = 3.0 * refit_max3(exp(ls[0]), exp(ls[1]), exp(ls[2]));
  for (int a = 0; a < 3; ++a) {
    lo[a] = (float)(x[a] - e);
    hi[a] = (float)(x[a] + e);
  }
}

// q: (w, x, y, z) as stored, any norm; a zero quaternion gives NaN boxes
__host__ __device__ __forceinline__ void refit_leaf_ellipsoid(const double x[3], const double ls[3], const double q[4],
                                                              float lo[3], float hi[3]) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const double n = sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3]);
  const double r = q[0] / n, i = q[1] / n, j = q[2] / n, k = q[3] / n;
  const double R[9] = {1 - 2 * (j * j + k * k), 2 * (i * j - r * k), 2 * (i * k + r * j),
                       2 * (i * j + r * k), 1 - 2 * (i * i + k * k), 2 * (j * k - r * i),
                       2 * (i * k - r * j), 2 * (j * k + r * i), 1 - 2 * (i * i + j * j)};
  const double s0 = exp(ls[0]), s1 = exp(ls[1]), s2 = exp(ls[2]);
  const double v0 = s0 * s0, v1 = s1 * s1, v2 = s2 * s2;
  for (int a = 0; a < 3; ++a) {
    const double r0 = R[3 * a], r1 = R[3 * a + 1], r2 = R[3 * a + 2];
    const double h = 3.0 * sqrt(((r0 * r0) * v0 + (r1 * r1) * v1) + (r2 * r2) * v2);
    lo[a] = (float)(x[a] - h);
    hi[a] = (float)(x[a] + h);
  }
}

// What a leaf box has to be before anything is written: six finite coordinates, lo <= hi on every axis.
__host__ __device__ __forceinline__ bool refit_box_ok(const float lo[3], const float hi[3]) {
  bool ok = true;
  for (int a = 0; a < 3; ++a) ok = ok && (lo[a] - lo[a] == 0.0f) && (hi[a] - hi[a] == 0.0f) && lo[a] <= hi[a];
  return ok;
}

// (lo, hi) grown to hold (clo, chi); the boxes are finite, so min and max are exact
__host__ __device__ __forceinline__ void refit_union(float lo[3], float hi[3], const float clo[3], const float chi[3]) {
  for (int a = 0; a < 3; ++a) {
    lo[a] = clo[a] < lo[a] ? clo[a] : lo[a];
    hi[a] = chi[a] > hi[a] ? chi[a] : hi[a];
  }
}

// boxes[n,0,3]: the largest edge of the rounded box in float32, as the builder computes it
__host__ __device__ __forceinline__ float refit_extent(const float lo[3], const float hi[3]) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const float e0 = hi[0] - lo[0], e1 = hi[1] - lo[1], e2 = hi[2] - lo[2];
  const float m = e0 > e1 ? e0 : e1;
  return m > e2 ? m : e2;
}

}  // namespace hgs
