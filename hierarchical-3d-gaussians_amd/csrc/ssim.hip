// Fused SSIM loss (hgs.loss.ssim): the standard definition -- an 11-tap Gaussian window (sigma 1.5, normalised to sum
// 1) applied separably, zero padding, C1 = 0.01^2, C2 = 0.03^2 -- with its analytic backward.
//
//   forward    ssim_fwd_kernel: one workgroup per 32x16 output tile of one (image, channel) plane.  x1 and x2 of the
//              tile plus a 5-pixel halo (zeros outside the image) are staged in LDS; the horizontal pass writes the
//              five filtered moments of the 26 halo rows to LDS, the vertical pass finishes them per output pixel and
//              evaluates S in registers.  S is summed over the workgroup in double (wave shuffles, then the four wave
//              sums in order) into one partial per workgroup.  With maps != nullptr it also writes, per pixel, the
//              partials of S with respect to the filtered moments F[x1], F[x1^2], F[x1 x2]:
//                B = dS/dsigma1^2 = -S / D2,  Cc = dS/dsigma12 = 2 N1 / (D1 D2),
//                A = dS/dmu1 - 2 mu1 B - mu2 Cc,  dS/dmu1 = 2 mu2 N2 / (D1 D2) - 2 mu1 S / D1
//              (no division by S: S = 0 is safe).
//   reduce     ssim_reduce_kernel: one workgroup adds the partials image by image in a fixed order in double and writes
//              the per-image means and the overall mean (float).  No atomics: results are bit-reproducible.
//   backward   ssim_bwd_kernel: the same tiling.  grad_x1(q) = g (F[A](q) + 2 x1(q) F[B](q) + x2(q) F[Cc](q)), where
//              F is the same (symmetric) window and A, B, Cc are zero outside the image; g is the upstream gradient
//              over the number of pixels averaged.
#include "common.h"

namespace hgs {
namespace {

constexpr int kTaps = 11;
constexpr int kHalo = kTaps / 2;
constexpr int kTW = 32;                 // output tile width (one column per lane of a half-wave)
constexpr int kTH = 16;                 // output tile height
constexpr int kIW = kTW + 2 * kHalo;    // staged width (42)
constexpr int kIH = kTH + 2 * kHalo;    // staged height (26)
constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kRowsPerPass = kThreads / kTW;   // 8 output rows per vertical step
constexpr int kReduceThreads = 1024;
constexpr int64_t kMaxTiles = (int64_t)UINT32_MAX / kThreads;   // 16 777 215 workgroups of a 1-D grid
constexpr float kC1 = 0.01f * 0.01f;
constexpr float kC2 = 0.03f * 0.03f;

struct Window {
  float w[kTaps];
};

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// The block's partial in a fixed order: every lane's value, the wave sums in wave order.
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

struct TileCoords {
  int64_t plane;    // n * C + c
  int y0, x0;       // top-left output pixel of the tile
};

__device__ __forceinline__ TileCoords tile_of(int tiles_x, int tiles_per_plane) {
  TileCoords t;
  t.plane = blockIdx.x / tiles_per_plane;
  const int r = blockIdx.x - (int)t.plane * tiles_per_plane;
  t.y0 = (r / tiles_x) * kTH;
  t.x0 = (r % tiles_x) * kTW;
  return t;
}

__global__ __launch_bounds__(kThreads) void ssim_fwd_kernel(const float* __restrict__ x1, const float* __restrict__ x2,
                                                            int H, int W, int tiles_x, int tiles_per_plane, Window win,
                                                            int64_t total, float* __restrict__ maps,
                                                            double* __restrict__ partials) {
  __shared__ float s1[kIH][kIW];
  __shared__ float s2[kIH][kIW];
  __shared__ float hm[5][kIH][kTW];
  __shared__ double wsum[kWaves];
  const TileCoords t = tile_of(tiles_x, tiles_per_plane);
  const int64_t base = t.plane * (int64_t)H * W;
  const float* p1 = x1 + base;
  const float* p2 = x2 + base;
  const int tid = threadIdx.x;

  for (int i = tid; i < kIH * kIW; i += kThreads) {
    const int r = i / kIW, c = i - r * kIW;
    const int gy = t.y0 - kHalo + r, gx = t.x0 - kHalo + c;
    const bool in = gy >= 0 && gy < H && gx >= 0 && gx < W;
    const int64_t o = (int64_t)gy * W + gx;
    s1[r][c] = in ? p1[o] : 0.f;
    s2[r][c] = in ? p2[o] : 0.f;
  }
  __syncthreads();

  for (int i = tid; i < kIH * kTW; i += kThreads) {
    const int r = i / kTW, c = i - r * kTW;
    float m0 = 0.f, m1 = 0.f, m2 = 0.f, m3 = 0.f, m4 = 0.f;
#pragma unroll
    for (int k = 0; k < kTaps; ++k) {
      const float a = s1[r][c + k], b = s2[r][c + k], w = win.w[k];
      m0 += w * a;
      m1 += w * b;
      m2 += w * (a * a);
      m3 += w * (b * b);
      m4 += w * (a * b);
    }
    hm[0][r][c] = m0;
    hm[1][r][c] = m1;
    hm[2][r][c] = m2;
    hm[3][r][c] = m3;
    hm[4][r][c] = m4;
  }
  __syncthreads();

  const int c = tid % kTW;
  const int x = t.x0 + c;
  double acc = 0.0;
#pragma unroll
  for (int rr = tid / kTW; rr < kTH; rr += kRowsPerPass) {
    const int y = t.y0 + rr;
    float mu1 = 0.f, mu2 = 0.f, e11 = 0.f, e22 = 0.f, e12 = 0.f;
#pragma unroll
    for (int k = 0; k < kTaps; ++k) {
      const float w = win.w[k];
      mu1 += w * hm[0][rr + k][c];
      mu2 += w * hm[1][rr + k][c];
      e11 += w * hm[2][rr + k][c];
      e22 += w * hm[3][rr + k][c];
      e12 += w * hm[4][rr + k][c];
    }
    if (y < H && x < W) {
      // One fused multiply-add each, so that the three (co)variances round alike: with x1 == x2 they are equal and
      // N2 == D2 exactly.  Written as e - mu * mu, the compiler may round one product (mu1 * mu1 is shared with D1)
      // and fuse another; in a flat region that difference, relative to C2, put S of identical images 6e-6 from 1.
      const float sg1 = fmaf(-mu1, mu1, e11), sg2 = fmaf(-mu2, mu2, e22), sg12 = fmaf(-mu1, mu2, e12);
      const float n1 = 2.f * mu1 * mu2 + kC1, n2 = 2.f * sg12 + kC2;
      const float d1 = mu1 * mu1 + mu2 * mu2 + kC1, d2 = sg1 + sg2 + kC2;
      const float inv = 1.f / (d1 * d2);
      const float S = n1 * n2 * inv;
      acc += (double)S;
      if (maps) {
        const float B = -S / d2;
        const float Cc = 2.f * n1 * inv;
        const float dmu1 = 2.f * mu2 * n2 * inv - 2.f * mu1 * S / d1;
        const float A = dmu1 - 2.f * mu1 * B - mu2 * Cc;
        const int64_t o = base + (int64_t)y * W + x;
        maps[o] = A;
        maps[total + o] = B;
        maps[2 * total + o] = Cc;
      }
    }
  }
  const double s = block_sum(acc, wsum);
  if (tid == 0) partials[blockIdx.x] = s;
}

// One workgroup: image n's partials (C * tiles_per_plane of them, contiguous) summed in a fixed order.
__global__ __launch_bounds__(kReduceThreads) void ssim_reduce_kernel(const double* __restrict__ partials, int N,
                                                                     int64_t per_image, double inv_image_px,
                                                                     double inv_total_px, float* __restrict__ out_image,
                                                                     float* __restrict__ out_mean) {
  __shared__ double wsum[kReduceThreads / 64];
  double total = 0.0;
  for (int n = 0; n < N; ++n) {
    const double* p = partials + (int64_t)n * per_image;
    double v = 0.0;
    for (int64_t i = threadIdx.x; i < per_image; i += kReduceThreads) v += p[i];
    const double s = block_sum(v, wsum);
    if (threadIdx.x == 0) {
      out_image[n] = (float)(s * inv_image_px);
      total += s;
    }
    __syncthreads();   // wsum is reused by the next image
  }
  if (threadIdx.x == 0) *out_mean = (float)(total * inv_total_px);
}

__global__ __launch_bounds__(kThreads) void ssim_bwd_kernel(const float* __restrict__ x1, const float* __restrict__ x2,
                                                            const float* __restrict__ maps, const float* __restrict__ g,
                                                            int per_image, int C, double count, int H, int W,
                                                            int tiles_x, int tiles_per_plane, Window win, int64_t total,
                                                            float* __restrict__ grad) {
  __shared__ float sm[3][kIH][kIW];
  __shared__ float hm[3][kIH][kTW];
  const TileCoords t = tile_of(tiles_x, tiles_per_plane);
  const int64_t base = t.plane * (int64_t)H * W;
  const int tid = threadIdx.x;

  for (int i = tid; i < kIH * kIW; i += kThreads) {
    const int r = i / kIW, c = i - r * kIW;
    const int gy = t.y0 - kHalo + r, gx = t.x0 - kHalo + c;
    const bool in = gy >= 0 && gy < H && gx >= 0 && gx < W;
    const int64_t o = base + (int64_t)gy * W + gx;
    sm[0][r][c] = in ? maps[o] : 0.f;
    sm[1][r][c] = in ? maps[total + o] : 0.f;
    sm[2][r][c] = in ? maps[2 * total + o] : 0.f;
  }
  __syncthreads();

  for (int i = tid; i < kIH * kTW; i += kThreads) {
    const int r = i / kTW, c = i - r * kTW;
    float m0 = 0.f, m1 = 0.f, m2 = 0.f;
#pragma unroll
    for (int k = 0; k < kTaps; ++k) {
      const float w = win.w[k];
      m0 += w * sm[0][r][c + k];
      m1 += w * sm[1][r][c + k];
      m2 += w * sm[2][r][c + k];
    }
    hm[0][r][c] = m0;
    hm[1][r][c] = m1;
    hm[2][r][c] = m2;
  }
  __syncthreads();

  const int64_t n = t.plane / C;
  const float gs = (float)((double)g[per_image ? n : 0] / count);
  const int c = tid % kTW;
  const int x = t.x0 + c;
#pragma unroll
  for (int rr = tid / kTW; rr < kTH; rr += kRowsPerPass) {
    const int y = t.y0 + rr;
    if (y >= H || x >= W) continue;
    float fa = 0.f, fb = 0.f, fc = 0.f;
#pragma unroll
    for (int k = 0; k < kTaps; ++k) {
      const float w = win.w[k];
      fa += w * hm[0][rr + k][c];
      fb += w * hm[1][rr + k][c];
      fc += w * hm[2][rr + k][c];
    }
    const int64_t o = base + (int64_t)y * W + x;
    grad[o] = gs * (fa + 2.f * x1[o] * fb + x2[o] * fc);
  }
}

Window gaussian_window() {
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

struct Grid {
  int tiles_x, tiles_per_plane, blocks;
  int64_t total;
};

Grid grid_of(int32_t N, int32_t C, int32_t H, int32_t W) {
  Grid g;
  g.tiles_x = (W + kTW - 1) / kTW;
  g.tiles_per_plane = g.tiles_x * ((H + kTH - 1) / kTH);
  g.blocks = (int)((int64_t)N * C * g.tiles_per_plane);
  g.total = (int64_t)N * C * H * W;
  return g;
}

}  // namespace

bool ssim_sizes_ok(int32_t N, int32_t C, int32_t H, int32_t W) {
  if (N < 1 || C < 1 || H < 1 || W < 1) {
    set_error("bad sizes: N=%d C=%d H=%d W=%d (each must be >= 1)", N, C, H, W);
    return false;
  }
  int64_t px, bytes;
  if (__builtin_mul_overflow((int64_t)N * C, (int64_t)H, &px) || __builtin_mul_overflow(px, (int64_t)W, &px) ||
      __builtin_mul_overflow(px, (int64_t)(3 * sizeof(float)), &bytes)) {
    set_error("bad sizes: N=%d C=%d H=%d W=%d: N*C*H*W (x 12 bytes of maps) overflows int64", N, C, H, W);
    return false;
  }
  // One kThreads-thread workgroup per tile in a 1-D grid: the dispatch packet's grid_size_x counts work-items in 32 bits
  // (hsa_kernel_dispatch_packet_t), so at most (2^32 - 1) / kThreads = 16 777 215 tiles can be launched.
  const int64_t tiles = (int64_t)((W + (int64_t)kTW - 1) / kTW) * ((H + (int64_t)kTH - 1) / kTH);
  if (tiles > kMaxTiles || (int64_t)N * C > kMaxTiles / tiles) {
    set_error("bad sizes: N=%d C=%d H=%d W=%d: more than %lld tiles of %dx%d (one %d-thread workgroup per tile; a 1-D "
              "grid holds at most 2^32 - 1 work-items)", N, C, H, W, (long long)kMaxTiles, kTW, kTH, kThreads);
    return false;
  }
  return true;
}

size_t ssim_tmp_bytes(int32_t N, int32_t C, int32_t H, int32_t W) {
  return align_up((size_t)grid_of(N, C, H, W).blocks * sizeof(double));
}

int launch_ssim_fwd(const float* img1, const float* img2, int32_t N, int32_t C, int32_t H, int32_t W,
                    float* out_image, float* out_mean, float* maps, void* tmp, hipStream_t s) {
  const Grid g = grid_of(N, C, H, W);
  const Window win = gaussian_window();
  double* partials = static_cast<double*>(tmp);
  ssim_fwd_kernel<<<g.blocks, kThreads, 0, s>>>(img1, img2, H, W, g.tiles_x, g.tiles_per_plane, win, g.total, maps,
                                                 partials);
  HGS_LAUNCH_CHECK("ssim_fwd_kernel", s, false);
  const int64_t image_px = (int64_t)C * H * W;
  ssim_reduce_kernel<<<1, kReduceThreads, 0, s>>>(partials, N, (int64_t)C * g.tiles_per_plane, 1.0 / (double)image_px,
                                                  1.0 / (double)g.total, out_image, out_mean);
  HGS_LAUNCH_CHECK("ssim_reduce_kernel", s, false);
  return HGS_OK;
}

int launch_ssim_bwd(const float* img1, const float* img2, const float* maps, const float* grad_out, int32_t per_image,
                    int32_t N, int32_t C, int32_t H, int32_t W, float* grad_img1, hipStream_t s) {
  const Grid g = grid_of(N, C, H, W);
  const Window win = gaussian_window();
  const double count = per_image ? (double)((int64_t)C * H * W) : (double)g.total;
  ssim_bwd_kernel<<<g.blocks, kThreads, 0, s>>>(img1, img2, maps, grad_out, per_image ? 1 : 0, C, count, H, W,
                                                 g.tiles_x, g.tiles_per_plane, win, g.total, grad_img1);
  HGS_LAUNCH_CHECK("ssim_bwd_kernel", s, false);
  return HGS_OK;
}

}  // namespace hgs
