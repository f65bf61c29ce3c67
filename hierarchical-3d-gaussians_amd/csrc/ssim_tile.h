// The SSIM tile, ONCE, for the two losses whose SSIM must agree bit for bit: hgs.loss.ssim (ssim.hip) and the fused
// training loss (photometric.hip).  Included by those two files only.  A workgroup of kThreads owns a kTW x kTH output
// tile: it stages the tile plus a kHalo-pixel halo (zeros outside the image) in LDS, filters the staged rows
// horizontally into LDS and finishes the filter vertically at each thread's own output pixels.  The forward filters the
// five moments of a pair of planes and evaluates S; the backward filters the three partial maps the forward wrote.
//
// Rounding is written down here, not left to the compiler: every tap of the four separable passes is ONE
// fmaf(w, x, acc) in tap order (the products a*a, b*b, a*b are single multiplies that feed it), the three (co)variances
// and the backward's F[A] + 2 x F[B] + gt F[Cc] are explicit fmaf, and the rest of the per-pixel formula is evaluated as
// written with contraction off.  No float multiply-add of this file is open to contraction or to the SLP vectoriser's
// choice between a fused and a split form, so photometric.hip's S, maps and SSIM gradient have ssim.hip's bits
// because they are this text instantiated twice, not because two compilations happened to decide alike.
#pragma once
#include "common.h"

#include <math.h>

namespace hgs {

constexpr int kTaps = 11;
constexpr int kHalo = kTaps / 2;
constexpr int kTW = 32;                 // output tile width (one column per lane of a half-wave)
constexpr int kTH = 16;                 // output tile height
constexpr int kIW = kTW + 2 * kHalo;    // staged width (42)
constexpr int kIH = kTH + 2 * kHalo;    // staged height (26)
constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kRowsPerPass = kThreads / kTW;   // 8 output rows per vertical step
constexpr int kRows = kTH / kRowsPerPass;      // output pixels per thread (2): rows tid / kTW + k * kRowsPerPass
constexpr int kReduceThreads = 1024;
constexpr float kC1 = 0.01f * 0.01f;
constexpr float kC2 = 0.03f * 0.03f;

// the 11-tap Gaussian window (sigma 1.5, normalised to sum 1 in double); passed by value: uniform across the grid
struct Window {
  float w[kTaps];
};

inline Window gaussian_window() {
  double g[kTaps], sum = 0.0;
  for (int k = 0; k < kTaps; ++k) {
    const double d = k - kHalo;
    g[k] = exp(-d * d / (2.0 * 1.5 * 1.5));
    sum += g[k];
  }
  Window w;
  for (int k = 0; k < kTaps; ++k) w.w[k] = (float)(g[k] / sum);
  return w;
}

// ---- workgroup sums in a fixed order -------------------------------------------------------------------------------
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// One workgroup's sum (every lane's value, then the wave sums in wave order), valid in thread 0.
__device__ __forceinline__ double block_sum(double v, double* wsum) {
  v = wave_sum(v);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) wsum[wave] = v;
  __syncthreads();
  double s = 0.0;
  if (threadIdx.x == 0)
    for (int i = 0; i < (int)(blockDim.x >> 6); ++i) s += wsum[i];
  return s;
}

// ---- staging -------------------------------------------------------------------------------------------------------
// The tile at (y0, x0) plus its halo of a pair of H x W planes.  load(o, a, b) gives the two values at pixel offset
// o = y * W + x; it is called inside the image only, outside both are 0.  The caller puts the barrier behind it.
template <typename Load>
__device__ __forceinline__ void stage_pair(float (&s1)[kIH][kIW], float (&s2)[kIH][kIW], int y0, int x0, int H, int W,
                                           Load load) {
  for (int i = threadIdx.x; i < kIH * kIW; i += kThreads) {
    const int r = i / kIW, c = i - r * kIW;
    const int gy = y0 - kHalo + r, gx = x0 - kHalo + c;
    float a = 0.f, b = 0.f;
    if (gy >= 0 && gy < H && gx >= 0 && gx < W) load((int64_t)gy * W + gx, a, b);
    s1[r][c] = a;
    s2[r][c] = b;
  }
}

// The same for the three partial maps A, B, Cc of one plane (`plane` points at its A; B and Cc lie `total` apart).
__device__ __forceinline__ void stage_maps(float (&sm)[3][kIH][kIW], const float* __restrict__ plane, int64_t total,
                                           int y0, int x0, int H, int W) {
  for (int i = threadIdx.x; i < kIH * kIW; i += kThreads) {
    const int r = i / kIW, c = i - r * kIW;
    const int gy = y0 - kHalo + r, gx = x0 - kHalo + c;
    const bool in = gy >= 0 && gy < H && gx >= 0 && gx < W;
    const int64_t o = (int64_t)gy * W + gx;
    sm[0][r][c] = in ? plane[o] : 0.f;
    sm[1][r][c] = in ? plane[total + o] : 0.f;
    sm[2][r][c] = in ? plane[2 * total + o] : 0.f;
  }
}

// ---- the four separable passes: one fmaf per tap, in tap order -----------------------------------------------------
// Horizontal, forward: F[a], F[b], F[a a], F[b b], F[a b] of every staged row at the tile's kTW columns.
__device__ __forceinline__ void filter_rows_moments(const float (&s1)[kIH][kIW], const float (&s2)[kIH][kIW],
                                                    float (&hm)[5][kIH][kTW], const Window& win) {
  for (int i = threadIdx.x; i < kIH * kTW; i += kThreads) {
    const int r = i / kTW, c = i - r * kTW;
    float m[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int k = 0; k < kTaps; ++k) {
      const float a = s1[r][c + k], b = s2[r][c + k], w = win.w[k];
      m[0] = fmaf(w, a, m[0]);
      m[1] = fmaf(w, b, m[1]);
      m[2] = fmaf(w, a * a, m[2]);
      m[3] = fmaf(w, b * b, m[3]);
      m[4] = fmaf(w, a * b, m[4]);
    }
#pragma unroll
    for (int q = 0; q < 5; ++q) hm[q][r][c] = m[q];
  }
}

// Horizontal, backward: F[A], F[B], F[Cc].
__device__ __forceinline__ void filter_rows_maps(const float (&sm)[3][kIH][kIW], float (&hm)[3][kIH][kTW],
                                                 const Window& win) {
  for (int i = threadIdx.x; i < kIH * kTW; i += kThreads) {
    const int r = i / kTW, c = i - r * kTW;
    float m[3] = {0.f, 0.f, 0.f};
#pragma unroll
    for (int k = 0; k < kTaps; ++k) {
      const float w = win.w[k];
#pragma unroll
      for (int q = 0; q < 3; ++q) m[q] = fmaf(w, sm[q][r][c + k], m[q]);
    }
#pragma unroll
    for (int q = 0; q < 3; ++q) hm[q][r][c] = m[q];
  }
}

// Vertical: the Q filtered quantities at output row rr, column c of the tile.
template <int Q>
__device__ __forceinline__ void filter_column(const float (&hm)[Q][kIH][kTW], int rr, int c, const Window& win,
                                              float (&f)[Q]) {
#pragma unroll
  for (int q = 0; q < Q; ++q) f[q] = 0.f;
#pragma unroll
  for (int k = 0; k < kTaps; ++k) {
    const float w = win.w[k];
#pragma unroll
    for (int q = 0; q < Q; ++q) f[q] = fmaf(w, hm[q][rr + k][c], f[q]);
  }
}

// ---- per pixel -----------------------------------------------------------------------------------------------------
// S from the five filtered moments f = mu1, mu2, F[x1 x1], F[x2 x2], F[x1 x2].  With map_a != nullptr it also stores
// the partials of S with respect to F[x1], F[x1^2], F[x1 x2] (map_a points at the pixel's A):
//   B = dS/dsigma1^2 = -S / D2,  Cc = dS/dsigma12 = 2 N1 / (D1 D2),
//   A = dS/dmu1 - 2 mu1 B - mu2 Cc,  dS/dmu1 = 2 mu2 N2 / (D1 D2) - 2 mu1 S / D1      (no division by S: S = 0 is safe)
// S does not depend on map_a.
__device__ __forceinline__ float ssim_pixel(const float (&f)[5], float* __restrict__ map_a, int64_t total) {
#pragma clang fp contract(off)
  const float mu1 = f[0], mu2 = f[1];
  // One fused multiply-add each, so that the three (co)variances round alike: with x1 == x2 they are equal and
  // N2 == D2 exactly (and N1 == D1: 2 mu mu and mu mu + mu mu are the same float).  Written as e - mu * mu, one
  // product could be rounded and another fused; in a flat region that difference, relative to C2, put S of identical
  // images 6e-6 from 1.
  const float sg1 = fmaf(-mu1, mu1, f[2]), sg2 = fmaf(-mu2, mu2, f[3]), sg12 = fmaf(-mu1, mu2, f[4]);
  const float n1 = 2.f * mu1 * mu2 + kC1, n2 = 2.f * sg12 + kC2;
  const float d1 = mu1 * mu1 + mu2 * mu2 + kC1, d2 = sg1 + sg2 + kC2;
  const float inv = 1.f / (d1 * d2);
  const float S = n1 * n2 * inv;
  if (map_a) {
    const float B = -S / d2;
    const float Cc = 2.f * n1 * inv;
    const float dmu1 = 2.f * mu2 * n2 * inv - 2.f * mu1 * S / d1;
    const float A = dmu1 - 2.f * mu1 * B - mu2 * Cc;
    map_a[0] = A;
    map_a[total] = B;
    map_a[2 * total] = Cc;
  }
  return S;
}

// dS/dx1 at a pixel before the factor g / count, from f = F[A], F[B], F[Cc]: F[A] + 2 x1 F[B] + x2 F[Cc].
__device__ __forceinline__ float ssim_pixel_grad(const float (&f)[3], float x1, float x2) {
  return fmaf(x2, f[2], fmaf(2.f * x1, f[1], f[0]));
}

}  // namespace hgs
