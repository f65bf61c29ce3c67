// The rules of TSDF fusion and of the surface-net extraction (tests/tsdf_spec.py, the spec; tsdf.hip runs them), each
// ONCE and for host and device alike.  Plain C++ behind the qualifiers: tests/test_tsdf_rule_on_host.py compiles this
// file with g++.  Everything is float32, every operation is written out in its order, contraction is off, and float
// division is correctly rounded on both sides: the numpy restatement matches bit for bit.
//
//   lattice    x_a = lo_a + voxel * float(i_a)
//   project    p_c = ((x_0 m[0][c] + x_1 m[1][c]) + x_2 m[2][c]) + m[3][c] (m: world_view_transform as stored, row
//              vectors; view[12] holds m[r][c] at 3 r + c), z = p_2 > z_min;
//              fx = ((p_0 / (z tanfovx) + 1) W - 1) 0.5, px = floor(fx + 0.5), 0 <= px < W tested on the floats; fy alike
//   update     d = depth[py, px] > 0, w = weight[py, px] (or 1) > 0, sdf = d - z >= -trunc, t = min(sdf / trunc, 1),
//              Wn = Wo + w, tsdf = (Wo tsdf + w t) / Wn, each colour channel alike, weight = min(Wn, max_weight)
//   cell       the 8 samples of a cell in the order 4 dk + 2 dj + di; the 12 edges: 4 along x, 4 along y, 4 along z,
//              each group by (k, j, i) of the edge's lower sample; an edge crosses where its ends differ in t < 0, at
//              tau = t_a / (t_a - t_b); vertex = sum of the crossing points in edge order / their count; normal = per
//              axis the sum over its 4 edges of t_b - t_a, normalised ((0,0,0) for a zero gradient); colour = the mean of
//              the 8 samples in sample order
//   quad       around the edge from sample s along axis a: the cells at (u - 1, v - 1), (u, v - 1), (u, v), (u - 1, v),
//              (u, v) = the two other axes in cyclic order (x: y z, y: z x, z: x y) -- the face normal then points along
//              +a; the order is reversed when the edge's LOWER sample is the outside one
// A failed test skips the view for the sample; a NaN fails every test (the comparisons are written so).
#pragma once
#include "common.h"

#include <math.h>

namespace hgs {

// the lower sample of edge e (0..11, edge order) of a cell: 0 2 4 6 | 0 1 4 5 | 0 1 2 3; the upper one is 1 << axis on
__host__ __device__ __forceinline__ int tsdf_edge_lo(int e) {
  const int axis = e >> 2, q = e & 3;
  return axis == 0 ? 2 * q : axis == 1 ? (q >> 1) * 4 + (q & 1) : q;
}

__host__ __device__ __forceinline__ float tsdf_lattice(float lo, float voxel, int32_t i) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  return lo + voxel * (float)i;
}

// Steps 1 and 2: the pixel a world point falls into and its view-space depth; false when the view does not see it.
__host__ __device__ __forceinline__ bool tsdf_project(float x0, float x1, float x2, const float* m, float tanfovx,
                                                      float tanfovy, int32_t W, int32_t H, float z_min, float* z_out,
                                                      int32_t* px_out, int32_t* py_out) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const float p0 = ((x0 * m[0] + x1 * m[3]) + x2 * m[6]) + m[9];
  const float p1 = ((x0 * m[1] + x1 * m[4]) + x2 * m[7]) + m[10];
  const float z = ((x0 * m[2] + x1 * m[5]) + x2 * m[8]) + m[11];
  if (!(z > z_min)) return false;
  const float fx = ((p0 / (z * tanfovx) + 1.0f) * (float)W - 1.0f) * 0.5f;
  const float fy = ((p1 / (z * tanfovy) + 1.0f) * (float)H - 1.0f) * 0.5f;
  const float px = floorf(fx + 0.5f), py = floorf(fy + 0.5f);
  if (!(px >= 0.0f && px < (float)W && py >= 0.0f && py < (float)H)) return false;
  *z_out = z;
  *px_out = (int32_t)px;
  *py_out = (int32_t)py;
  return true;
}

// Steps 3 to 6 on the values read at the pixel.  use_rgb: the view has colours (rgb[3]) and the volume takes them
// (colour[3]); neither pointer is followed otherwise.  false: nothing changed.
__host__ __device__ __forceinline__ bool tsdf_update(float d, float w, const float* rgb, bool use_rgb, float z,
                                                     float trunc, float max_weight, float* tsdf, float* weight,
                                                     float* colour) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  if (!(d > 0.0f) || !(w > 0.0f)) return false;
  const float sdf = d - z;
  if (!(sdf >= -trunc)) return false;
  const float q = sdf / trunc;
  const float t = q < 1.0f ? q : 1.0f;
  const float Wo = *weight, Wn = Wo + w;
  *tsdf = (Wo * *tsdf + w * t) / Wn;
  if (use_rgb) {
#pragma unroll
    for (int c = 0; c < 3; ++c) colour[c] = (Wo * colour[c] + w * rgb[c]) / Wn;
  }
  *weight = Wn < max_weight ? Wn : max_weight;
  return true;
}

__host__ __device__ __forceinline__ bool tsdf_observed(float weight, float min_weight) { return weight >= min_weight; }
__host__ __device__ __forceinline__ bool tsdf_inside(float t) { return t < 0.0f; }

// bit s = sample s of the cell is inside; the cell is active when all 8 are observed and the mask is neither 0 nor 255
__host__ __device__ __forceinline__ bool tsdf_cell_active(const float t[8], const float w[8], float min_weight) {
  bool observed = true;
  uint32_t in = 0;
#pragma unroll
  for (int s = 0; s < 8; ++s) {
    observed = observed && tsdf_observed(w[s], min_weight);
    in |= tsdf_inside(t[s]) ? (1u << s) : 0u;
  }
  return observed && in != 0u && in != 255u;
}

// The vertex of an active cell in cell-local units and its normal, from the cell's 8 samples.
__host__ __device__ __forceinline__ void tsdf_cell_vertex(const float t[8], float local[3], float normal[3]) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  float sum[3] = {0.0f, 0.0f, 0.0f}, grad[3] = {0.0f, 0.0f, 0.0f};
  int count = 0;
#pragma unroll
  for (int e = 0; e < 12; ++e) {
    const int axis = e >> 2, a = tsdf_edge_lo(e), b = a + (1 << axis);
    const float ta = t[a], tb = t[b];
    grad[axis] = (e & 3) ? grad[axis] + (tb - ta) : (tb - ta);
    if (tsdf_inside(ta) != tsdf_inside(tb)) {
      const float tau = ta / (ta - tb);
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const float base = (float)((a >> c) & 1);
        sum[c] = sum[c] + (c == axis ? base + tau : base);
      }
      ++count;
    }
  }
  for (int c = 0; c < 3; ++c) local[c] = sum[c] / (float)count;
  const float n = sqrtf((grad[0] * grad[0] + grad[1] * grad[1]) + grad[2] * grad[2]);
  for (int c = 0; c < 3; ++c) normal[c] = n > 0.0f ? grad[c] / n : 0.0f;
}

__host__ __device__ __forceinline__ float tsdf_vertex_world(float lo, float voxel, int32_t i, float local) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  return lo + voxel * ((float)i + local);
}

// the mean of one colour channel over the cell's 8 samples, in sample order
__host__ __device__ __forceinline__ float tsdf_cell_colour(const float c[8]) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  float s = c[0];
#pragma unroll
  for (int k = 1; k < 8; ++k) s = s + c[k];
  return s / 8.0f;
}

// The four cells around the edge from sample (i, j, k) along `axis`, as offsets (di, dj, dk) from the sample, in the
// order whose face normal points along +axis.
__host__ __device__ __forceinline__ void tsdf_quad_cells(int axis, int32_t cells[4][3]) {
  const int u = (axis + 1) % 3, v = (axis + 2) % 3;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    cells[q][axis] = 0;
    cells[q][u] = (q == 0 || q == 3) ? -1 : 0;
    cells[q][v] = q < 2 ? -1 : 0;
  }
}

// The quad's two triangles from its four vertex indices (in tsdf_quad_cells' order): kept when the lower sample is the
// inside one, reversed otherwise, so that the face normal points from the inside sample to the outside one.
__host__ __device__ __forceinline__ void tsdf_quad_faces(const int32_t v[4], bool lower_inside, int32_t faces[6]) {
  const int32_t v1 = lower_inside ? v[1] : v[3], v3 = lower_inside ? v[3] : v[1];
  faces[0] = v[0]; faces[1] = v1; faces[2] = v[2];
  faces[3] = v[0]; faces[4] = v[2]; faces[5] = v3;
}

}  // namespace hgs
