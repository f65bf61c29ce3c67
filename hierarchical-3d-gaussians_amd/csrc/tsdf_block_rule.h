// The rules of a SPARSE TSDF volume (tests/tsdf_sparse_spec.py, the spec; tsdf_sparse.hip
// runs them), each ONCE and for host and device alike, in the style of tsdf_rule.h: plain C++ behind the qualifiers
// (tests/test_tsdf_block_rule_on_host.py compiles this file with g++), float32, every operation written out in its order,
// contraction off: the numpy restatement matches bit for bit.
//
//   blocks     8 x 8 x 8 samples; block (bi, bj, bk) holds the lattice samples 8 b .. 8 b + 7 per axis; the block grid is
//              ceil(n / 8) per axis, x fastest; a sample's place in its block is 64 lk + 8 lj + li
//   marking    per pixel with d > 0 and w > 0 (a NaN fails) and d + trunc finite:
//              steps   S = max(1, ceil(trunc / voxel)), dz = (2 trunc) / S: a spacing of at most 2 voxels;
//                      z_s = (d - trunc) + s dz, s = 0 .. S; a z_s that is not > z_min is skipped
//              sub     M = max(1, ceil(max(((2 tanfovx) far) / W, ((2 tanfovy) far) / H) / (2 voxel))), far = d + trunc:
//                      the least M at which the pixel's footprint at the far end of the band, cut M x M, is at most 2
//                      voxels wide; more than kTsdfMaxSub: the pixel is not marched and the table's refusal word is set
//              point   sub-position (a, b), 0 <= a, b < M: fx = px + ((a + 0.5) / M - 0.5), fy alike;
//                      p_0 = ((2 fx + 1) / W - 1) (z tanfovx), p_1 alike, p_2 = z -- the inverse of tsdf_project's pixel
//                      formula --; q_c = p_c - m[3][c]; x_a = (q_0 m[a][0] + q_1 m[a][1]) + q_2 m[a][2] -- the transposed
//                      rotation --; g_a = (x_a - lo_a) / voxel; b_a = floor(g_a / 8); the point is dropped unless
//                      -1 <= b_a <= grid_a on all three axes, and the block marked is b_a CLAMPED to 0 .. grid_a - 1: a
//                      point up to one block outside the grid marks the border block next to it, because a near sample
//                      just inside the lattice may have its nearest marched point just outside it (a pixel ray that
//                      runs along the border; the pixels on the inner side holes)
//   dilation   a block is allocated when a block of its 3 x 3 x 3 neighbourhood, clipped to the grid, is marked
//   slots      the allocated blocks numbered by ascending linear block index
#pragma once
#include "tsdf_rule.h"

namespace hgs {

constexpr int kTsdfBlock = 8;                 // samples per block edge
constexpr int kTsdfBlockSamples = 512;
constexpr int kTsdfMaxSub = 16;               // the largest sub-pixel grid a pixel is marched with
constexpr int kTsdfMaxSteps = 4096;           // the largest S (trunc of at most 4096 voxels)
constexpr float kTsdfMaxTan = 1.5f;           // the accepted half field of view of a marked view, as a tangent

// blocks along an axis of n >= 1 samples (no n + 7: n may be 2^31 - 1)
__host__ __device__ __forceinline__ int32_t tsdf_block_grid(int32_t n) { return (n - 1) / kTsdfBlock + 1; }

// S; kTsdfMaxSteps + 1 where it would be more (or trunc / voxel is no number)
__host__ __device__ __forceinline__ int32_t tsdf_block_steps(float trunc, float voxel) {
  const float c = ceilf(trunc / voxel);
  if (!(c <= (float)kTsdfMaxSteps)) return kTsdfMaxSteps + 1;
  return c >= 1.0f ? (int32_t)c : 1;
}

__host__ __device__ __forceinline__ float tsdf_block_dz(float trunc, int32_t S) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  return (2.0f * trunc) / (float)S;
}

__host__ __device__ __forceinline__ float tsdf_block_depth(float d, float trunc, float dz, int32_t s) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  return (d - trunc) + (float)s * dz;
}

// Is the pixel marched at all?  (steps 3's tests of tsdf_update, and a band that ends at a finite depth)
__host__ __device__ __forceinline__ bool tsdf_block_pixel(float d, float w, float trunc) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  if (!(d > 0.0f) || !(w > 0.0f)) return false;
  const float far = d + trunc;
  return far - far == 0.0f;
}

// M of a marched pixel; 0 where it would be more than kTsdfMaxSub
__host__ __device__ __forceinline__ int32_t tsdf_block_sub(float d, float trunc, float tanfovx, float tanfovy, int32_t W,
                                                           int32_t H, float voxel) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const float far = d + trunc;
  const float fx = ((2.0f * tanfovx) * far) / (float)W, fy = ((2.0f * tanfovy) * far) / (float)H;
  const float m = ceilf((fx > fy ? fx : fy) / (2.0f * voxel));
  if (!(m <= (float)kTsdfMaxSub)) return 0;
  return m >= 1.0f ? (int32_t)m : 1;
}

// The block marked for the point at depth z on the ray through sub-position (a, b) of M x M of pixel (px, py): the
// point's own block, clamped onto the grid `grid` when the point lies up to one block outside it; false when it lies
// farther out (a NaN does).
__host__ __device__ __forceinline__ bool tsdf_block_point(int32_t px, int32_t py, int32_t a, int32_t b, int32_t M, float z,
                                                          const float* m, float tanfovx, float tanfovy, int32_t W,
                                                          int32_t H, const float* lo, float voxel, const int32_t* grid,
                                                          int32_t* block) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const float fx = (float)px + (((float)a + 0.5f) / (float)M - 0.5f);
  const float fy = (float)py + (((float)b + 0.5f) / (float)M - 0.5f);
  const float p0 = ((2.0f * fx + 1.0f) / (float)W - 1.0f) * (z * tanfovx);
  const float p1 = ((2.0f * fy + 1.0f) / (float)H - 1.0f) * (z * tanfovy);
  const float q0 = p0 - m[9], q1 = p1 - m[10], q2 = z - m[11];
  bool in = true;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float x = (q0 * m[3 * c] + q1 * m[3 * c + 1]) + q2 * m[3 * c + 2];
    const float g = (x - lo[c]) / voxel;
    const float bf = floorf(g * 0.125f);
    // (the float test first: a conversion out of int32's range is undefined; the integer test decides)
    const int32_t bi = (bf >= -1.0f && bf < 2147483648.0f) ? (int32_t)bf : -2;
    // up to one block outside the grid: the border block next to the point
    const bool ok = bi >= -1 && bi <= grid[c];
    in = in && ok;
    block[c] = !ok || bi < 0 ? 0 : bi < grid[c] ? bi : grid[c] - 1;
  }
  return in;
}

// The marking of one pixel: mark(bi, bj, bk) is called for the block tsdf_block_point gives every marched point.  false:
// the pixel asks for more than kTsdfMaxSub sub-positions and nothing was marched.
template <typename Mark>
__host__ __device__ __forceinline__ bool tsdf_block_march(int32_t px, int32_t py, float d, float w, const float* m,
                                                          float tanfovx, float tanfovy, int32_t W, int32_t H, float z_min,
                                                          const float* lo, float voxel, float trunc, int32_t S,
                                                          const int32_t* grid, Mark mark) {
  if (!tsdf_block_pixel(d, w, trunc)) return true;
  const int32_t M = tsdf_block_sub(d, trunc, tanfovx, tanfovy, W, H, voxel);
  if (M == 0) return false;
  const float dz = tsdf_block_dz(trunc, S);
  for (int32_t s = 0; s <= S; ++s) {
    const float z = tsdf_block_depth(d, trunc, dz, s);
    if (!(z > z_min)) continue;
    for (int32_t b = 0; b < M; ++b) {
      for (int32_t a = 0; a < M; ++a) {
        int32_t block[3];
        if (tsdf_block_point(px, py, a, b, M, z, m, tanfovx, tanfovy, W, H, lo, voxel, grid, block))
          mark(block[0], block[1], block[2]);
      }
    }
  }
  return true;
}

}  // namespace hgs
