// The merge rule of an interior node ("Interior nodes"), each part ONCE and for host and device
// alike: a child's weight and covariance from its stored row, the w-weighted moment match over any number of children,
// and the eigen tail -- the cyclic Jacobi solve of the merged covariance, the one parametrisation of its (sign- and
// order-ambiguous) decomposition, covariance -> log-scales and quaternion.  hb_merge_kernel of hier_build.hip (two
// children, moments carried in double) and hp_remerge_kernel of hier_prune.hip (k children, moments taken from the
// children's float32 rows) call the same tail.  Plain C++ behind the qualifiers:
// tests/test_hier_merge_rule_on_host.py compiles this file with g++ and holds it against the float64 numpy spec.
//
// Double arithmetic throughout.  No function here sets the contraction mode: each runs under its includer's (the
// builder compiles its merge with the compiler's default, and its rows are the bits other tools were tested against;
// the host test compiles with contraction off).  The contract is the builder's own: mean, SH and opacity to 1e-5,
// covariance to 1e-5 Frobenius per node, unit quaternions, ascending eigenvalues -- not bits across compilers.
#pragma once
#include "common.h"

#include <math.h>

namespace hgs {

// One Jacobi rotation zeroing a[p][q] (r: the third index); v accumulates the rotations (columns = eigenvectors).
template <int p, int q, int r>
__host__ __device__ __forceinline__ void jacobi_rotate(double (&a)[3][3], double (&v)[3][3]) {
  const double apq = a[p][q];
  if (apq == 0.0) return;
  const double theta = (a[q][q] - a[p][p]) / (2.0 * apq);
  const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
  const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
  a[p][p] -= t * apq;
  a[q][q] += t * apq;
  a[p][q] = a[q][p] = 0.0;
  const double arp = a[r][p], arq = a[r][q];
  a[r][p] = a[p][r] = c * arp - s * arq;
  a[r][q] = a[q][r] = s * arp + c * arq;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const double vp = v[k][p], vq = v[k][q];
    v[k][p] = c * vp - s * vq;
    v[k][q] = s * vp + c * vq;
  }
}

// Eigen-pairs i < j in ascending order (a conditional swap of the values and of the columns of v).
template <int i, int j>
__host__ __device__ __forceinline__ void order_pair(double (&lam)[3], double (&v)[3][3]) {
  const bool sw = lam[j] < lam[i];
  const double li = lam[i], lj = lam[j];
  lam[i] = sw ? lj : li;
  lam[j] = sw ? li : lj;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const double a = v[k][i], b = v[k][j];
    v[k][i] = sw ? b : a;
    v[k][j] = sw ? a : b;
  }
}

// Column k of v with its largest-magnitude component (the first of equal ones) positive.
template <int k>
__host__ __device__ __forceinline__ void orient_column(double (&v)[3][3]) {
  const double a0 = fabs(v[0][k]), a1 = fabs(v[1][k]), a2 = fabs(v[2][k]);
  const double lead = (a0 >= a1 && a0 >= a2) ? v[0][k] : (a1 >= a2 ? v[1][k] : v[2][k]);
  if (lead < 0.0) {
#pragma unroll
    for (int r = 0; r < 3; ++r) v[r][k] = -v[r][k];
  }
}

// Unit quaternion (w, x, y, z) of the proper rotation m (the spec's _quat_from_rot), rounded to float32.
__host__ __device__ __forceinline__ void quat_from_rot(const double (&m)[3][3], float (&out)[4]) {
  const double tr = m[0][0] + m[1][1] + m[2][2];
  double q[4];
  if (tr > 0.0) {
    const double s = sqrt(fmax(tr + 1.0, 1e-20)) * 2.0;
    q[0] = 0.25 * s; q[1] = (m[2][1] - m[1][2]) / s; q[2] = (m[0][2] - m[2][0]) / s; q[3] = (m[1][0] - m[0][1]) / s;
  } else if (m[0][0] >= m[1][1] && m[0][0] >= m[2][2]) {
    const double s = sqrt(fmax(1.0 + m[0][0] - m[1][1] - m[2][2], 1e-20)) * 2.0;
    q[0] = (m[2][1] - m[1][2]) / s; q[1] = 0.25 * s; q[2] = (m[0][1] + m[1][0]) / s; q[3] = (m[0][2] + m[2][0]) / s;
  } else if (m[1][1] >= m[2][2]) {
    const double s = sqrt(fmax(1.0 + m[1][1] - m[0][0] - m[2][2], 1e-20)) * 2.0;
    q[0] = (m[0][2] - m[2][0]) / s; q[1] = (m[0][1] + m[1][0]) / s; q[2] = 0.25 * s; q[3] = (m[1][2] + m[2][1]) / s;
  } else {
    const double s = sqrt(fmax(1.0 + m[2][2] - m[0][0] - m[1][1], 1e-20)) * 2.0;
    q[0] = (m[1][0] - m[0][1]) / s; q[1] = (m[0][2] + m[2][0]) / s; q[2] = (m[1][2] + m[2][1]) / s; q[3] = 0.25 * s;
  }
  const double inv = 1.0 / sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
  out[0] = (float)(q[0] * inv); out[1] = (float)(q[1] * inv); out[2] = (float)(q[2] * inv); out[3] = (float)(q[3] * inv);
}

// The eigen tail: the symmetric covariance cv = (xx, xy, xz, yy, yz, zz) -> the row's log-scales and quaternion.  Cyclic
// Jacobi, at most 16 sweeps; one parametrisation of the decomposition: eigenvalues ascending, as numpy's eigh, clamped
// at 1e-12; every eigenvector's largest component positive; column 0 negated if that left an improper rotation.
__host__ __device__ __forceinline__ void merge_cov_to_row(const double (&cv)[6], float (&log_scales)[3], float (&quat)[4]) {
  double A[3][3] = {{cv[0], cv[1], cv[2]}, {cv[1], cv[3], cv[4]}, {cv[2], cv[4], cv[5]}};
  double V[3][3] = {{1.0, 0.0, 0.0}, {0.0, 1.0, 0.0}, {0.0, 0.0, 1.0}};
  for (int sweep = 0; sweep < 16; ++sweep) {
    const double off = fabs(A[0][1]) + fabs(A[0][2]) + fabs(A[1][2]);
    const double diag = fabs(A[0][0]) + fabs(A[1][1]) + fabs(A[2][2]);
    if (!(off > 1e-18 * diag)) break;
    jacobi_rotate<0, 1, 2>(A, V);
    jacobi_rotate<0, 2, 1>(A, V);
    jacobi_rotate<1, 2, 0>(A, V);
  }
  double lam[3] = {A[0][0], A[1][1], A[2][2]};
  order_pair<0, 1>(lam, V);
  order_pair<1, 2>(lam, V);
  order_pair<0, 1>(lam, V);
  orient_column<0>(V);
  orient_column<1>(V);
  orient_column<2>(V);
  const double det = V[0][0] * (V[1][1] * V[2][2] - V[1][2] * V[2][1]) - V[0][1] * (V[1][0] * V[2][2] - V[1][2] * V[2][0]) +
                     V[0][2] * (V[1][0] * V[2][1] - V[1][1] * V[2][0]);
  if (det < 0.0) {
#pragma unroll
    for (int r = 0; r < 3; ++r) V[r][0] = -V[r][0];
  }
#pragma unroll
  for (int a = 0; a < 3; ++a) log_scales[a] = (float)log(sqrt(fmax(lam[a], 1e-12)));
  quat_from_rot(V, quat);
}

// ---- a child from its stored float32 row (the re-merge; the builder carries its children's moments in double) ----------
// w = alpha * s0 * s1 * s2, s = exp(log_scales): the weight of a LEAF, from its row, as the builder gave it (the product
// the merger's root rule takes from finished rows; not clamped per child: the SUM is clamped, merge_weight_sum).  A node
// with children weighs merge_weight_sum of its children's weights -- what the builder carries up -- never the product of
// its own merged row, which is another number.
__host__ __device__ __forceinline__ double merge_child_weight(double alpha, const double (&ls)[3]) {
  return alpha * ((exp(ls[0]) * exp(ls[1])) * exp(ls[2]));
}

__host__ __device__ __forceinline__ double merge_weight_sum(double sum) { return fmax(sum, 1e-30); }

// R diag(s^2) R^T as (xx, xy, xz, yy, yz, zz), R = _rot_from_quat(q) of the quaternion AS STORED (w, x, y, z): the
// builder's leaf rule, which does not normalise.
__host__ __device__ __forceinline__ void merge_child_cov(const double (&q)[4], const double (&ls)[3], double (&cv)[6]) {
  const double r = q[0], x = q[1], y = q[2], z = q[3];
  const double R[3][3] = {{1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y)},
                          {2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x)},
                          {2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)}};
  const double s0 = exp(ls[0]), s1 = exp(ls[1]), s2 = exp(ls[2]);
  const double v[3] = {s0 * s0, s1 * s1, s2 * s2};
  constexpr int kRow[6] = {0, 0, 0, 1, 1, 2}, kCol[6] = {0, 1, 2, 1, 2, 2};
#pragma unroll
  for (int k = 0; k < 6; ++k) {
    const int a = kRow[k], b = kCol[k];
    cv[k] = (R[a][0] * v[0]) * R[b][0] + (R[a][1] * v[1]) * R[b][1] + (R[a][2] * v[2]) * R[b][2];
  }
}

// The moment match over k children in two walks, children in ascending order, sums left to right:
//   mu = sum_c f_c x_c              (merge_add_mean, from mu = 0)
//   cv = sum_c f_c (C_c + d_c d_c^T), d_c = x_c - mu   (merge_add_cov, from cv = 0)
// with f_c = w_c / merge_weight_sum(sum_c w_c).
__host__ __device__ __forceinline__ void merge_add_mean(double f, const double (&x)[3], double (&mu)[3]) {
#pragma unroll
  for (int a = 0; a < 3; ++a) mu[a] += f * x[a];
}

__host__ __device__ __forceinline__ void merge_add_cov(double f, const double (&x)[3], const double (&c)[6],
                                                       const double (&mu)[3], double (&cv)[6]) {
  const double d[3] = {x[0] - mu[0], x[1] - mu[1], x[2] - mu[2]};
  constexpr int kRow[6] = {0, 0, 0, 1, 1, 2}, kCol[6] = {0, 1, 2, 1, 2, 2};
#pragma unroll
  for (int k = 0; k < 6; ++k) cv[k] += f * (c[k] + d[kRow[k]] * d[kCol[k]]);
}

// the opacity of a merged node: the f-weighted average, clipped to [0, 1]
__host__ __device__ __forceinline__ float merge_alpha(double a) { return (float)fmin(fmax(a, 0.0), 1.0); }

}  // namespace hgs
