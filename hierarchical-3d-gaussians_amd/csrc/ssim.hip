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
// The tile itself (constants, window, staging, the filter passes, the per-pixel formula, the workgroup sums) is
// ssim_tile.h, shared with photometric.hip; this file holds the kernels around it, the reduction and the launchers.
#include "ssim_tile.h"

namespace hgs {
namespace {

constexpr int64_t kMaxTiles = (int64_t)UINT32_MAX / kThreads;   // 16 777 215 workgroups of a 1-D grid

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

  stage_pair(s1, s2, t.y0, t.x0, H, W, [&](int64_t o, float& a, float& b) { a = p1[o], b = p2[o]; });
  __syncthreads();
  filter_rows_moments(s1, s2, hm, win);
  __syncthreads();

  const int c = tid % kTW;
  const int x = t.x0 + c;
  double acc = 0.0;
#pragma unroll
  for (int rr = tid / kTW; rr < kTH; rr += kRowsPerPass) {
    const int y = t.y0 + rr;
    float f[5];
    filter_column(hm, rr, c, win, f);
    if (y < H && x < W) {
      const int64_t o = base + (int64_t)y * W + x;
      acc += (double)ssim_pixel(f, maps ? maps + o : nullptr, total);
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

  stage_maps(sm, maps + base, total, t.y0, t.x0, H, W);
  __syncthreads();
  filter_rows_maps(sm, hm, win);
  __syncthreads();

  const int64_t n = t.plane / C;
  const float gs = (float)((double)g[per_image ? n : 0] / count);
  const int c = tid % kTW;
  const int x = t.x0 + c;
#pragma unroll
  for (int rr = tid / kTW; rr < kTH; rr += kRowsPerPass) {
    const int y = t.y0 + rr;
    if (y >= H || x >= W) continue;
    float f[3];
    filter_column(hm, rr, c, win, f);
    const int64_t o = base + (int64_t)y * W + x;
    grad[o] = gs * ssim_pixel_grad(f, x1[o], x2[o]);
  }
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
