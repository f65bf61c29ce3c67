// Fused training loss (hgs.loss.photometric_loss): exposure, clamp, alpha mask, L1, D-SSIM and
// the inverse-depth L1 term of the reference's three training scripts, with the analytic backward.
//
//   per pixel p and output channel j      u_j = sum_i r_i E[i][j] + E[j][3]   (u = r without exposure)
//                                         v_j = min(max(u_j, 0), 1)           (clamp; gradient where 0 <= u <= 1)
//                                         x_j = v_j m
//   L1 = mean |x - gt|,  S = SSIM(x, gt) as ssim.hip,  D = mean |(d - d_mono) m_d|
//   loss = (1 - lambda) L1 + lambda (1 - S) + depth_weight D
//
// The SSIM tile -- staging, the four filter passes, S and its three maps, the workgroup sums -- is ssim_tile.h, the text
// ssim.hip instantiates: S, the maps and the SSIM part of the gradient have ssim.hip's bits.  This file holds what the
// fused loss adds: the exposure, the clamp and the mask while staging, the L1 and depth terms, the exposure partials.
//
//   forward    photo_fwd_kernel: one workgroup per 32x16 tile of one IMAGE (ssim.hip has one per plane): the exposure
//              mixes channels, so the workgroup loops over the output channels of its tile and re-stages ssim.hip's two
//              LDS buffers -- x_j, computed while staging from all channels of r, and gt_j -- per channel.  LDS stays at
//              ssim.hip's 25.4 KB (staging three x planes at once takes 34 KB and a workgroup per CU less); the extra
//              reads of r hit the cache.  Per workgroup three partials in double: the sums of |x - gt|, S and
//              |(d - d_mono) m_d|.
//   reduce     photo_reduce_kernel: one workgroup adds each of the three partial arrays in a fixed order and writes
//              loss, L1, S, D (four floats).
//   backward   photo_bwd_kernel: the same tiling and channel loop.  Filters ssim.hip's three partial maps, recomputes
//              u, v, x at the own pixel from r, forms dx_j = -lambda g/count (F[A] + 2 x F[B] + gt F[Cc]) +
//              (1 - lambda) g/count sign(x - gt), du_j = dx_j m [0 <= u_j <= 1], grad_r_i = sum_j E[i][j] du_j, and per
//              workgroup the 12 exposure partials sum r_i du_j, sum du_j in double; grad_d = depth_weight g/count_d
//              sign(q) m_d.
//   reduce     photo_exposure_reduce_kernel: workgroup (n, k) adds image n's partials of exposure entry k in a fixed
//              order.  No atomics anywhere: two calls give bit-identical results.
#include "ssim_tile.h"

namespace hgs {
namespace {

constexpr int kExp = 12;                       // entries of a 3x4 exposure

struct Images {
  const float* r;       // [N,C,H,W]
  const float* gt;      // [N,C,H,W]
  const float* E;       // [N,3,4] or nullptr
  const float* mask;    // [N,H,W] or nullptr
  const float* d;       // [N,H,W] or nullptr (then mono and md too)
  const float* mono;
  const float* md;
  int C, H, W, tiles_x, tiles_per_image, clamp;
};

// K sums of a kThreads workgroup at once: thread k < K adds the wave sums of value k in wave order and stores
// out[k * stride + blockIdx.x].
template <int K>
__device__ __forceinline__ void block_sums_store(double (&v)[K], double (*wsum)[kWaves], double* __restrict__ out,
                                                 int64_t stride) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const double s = wave_sum(v[k]);
    if (lane == 0) wsum[k][wave] = s;
  }
  __syncthreads();
  if (threadIdx.x < K) {
    double s = 0.0;
#pragma unroll
    for (int i = 0; i < kWaves; ++i) s += wsum[threadIdx.x][i];
    out[threadIdx.x * stride + blockIdx.x] = s;
  }
}

struct Tile {
  int64_t n;        // image
  int y0, x0;       // top-left output pixel of the tile
};

__device__ __forceinline__ Tile tile_of(const Images& im) {
  Tile t;
  t.n = blockIdx.x / im.tiles_per_image;
  const int r = blockIdx.x - (int)t.n * im.tiles_per_image;
  t.y0 = (r / im.tiles_x) * kTH;
  t.x0 = (r % im.tiles_x) * kTW;
  return t;
}

// Column j of the exposure: u_j = r0 e[0] + r1 e[1] + r2 e[2] + e[3].
struct ExpCol {
  float e[4];
};

template <bool EXP>
__device__ __forceinline__ ExpCol exp_col(const float* __restrict__ E, int j) {
  ExpCol c = {{0.f, 0.f, 0.f, 0.f}};
  if (EXP) {
    c.e[0] = E[j];
    c.e[1] = E[4 + j];
    c.e[2] = E[8 + j];
    c.e[3] = E[4 * j + 3];
  }
  return c;
}

// u_j at pixel offset o of image base rn (plane stride hw).  The forward and the backward share this expression, so
// that both see the same side of the clamp.
template <bool EXP>
__device__ __forceinline__ float exposed(const float* __restrict__ rn, int64_t hw, int64_t o, int j, const ExpCol& c) {
  if (!EXP) return rn[j * hw + o];
  return fmaf(rn[2 * hw + o], c.e[2], fmaf(rn[hw + o], c.e[1], rn[o] * c.e[0])) + c.e[3];
}

__device__ __forceinline__ float clamped(float u, int clamp) {
  if (!clamp) return u;
  return u < 0.f ? 0.f : (u > 1.f ? 1.f : u);       // NaN stays NaN, as torch.clamp
}

__device__ __forceinline__ float sign_of(float t) { return (float)(t > 0.f) - (float)(t < 0.f); }

template <bool EXP>
__global__ __launch_bounds__(kThreads) void photo_fwd_kernel(Images im, Window win, int64_t total,
                                                             float* __restrict__ maps, double* __restrict__ partials,
                                                             int64_t blocks) {
  __shared__ float s1[kIH][kIW];
  __shared__ float s2[kIH][kIW];
  __shared__ float hm[5][kIH][kTW];
  __shared__ double wsum[3][kWaves];
  const Tile t = tile_of(im);
  const int H = im.H, W = im.W;
  const int64_t hw = (int64_t)H * W;
  const float* rn = im.r + t.n * im.C * hw;
  const float* gn = im.gt + t.n * im.C * hw;
  const float* mn = im.mask ? im.mask + t.n * hw : nullptr;
  const float* En = EXP ? im.E + t.n * kExp : nullptr;
  const int tid = threadIdx.x;
  const int c = tid % kTW, r0 = tid / kTW;
  const int x = t.x0 + c;
  double acc[3] = {0.0, 0.0, 0.0};      // |x - gt|, S, |q|

  for (int j = 0; j < im.C; ++j) {
    const ExpCol ec = exp_col<EXP>(En, j);
    // every thread is past the previous channel's horizontal pass (the barrier behind it) and has taken its own
    // pixels of s1 / s2 into registers before that barrier: the buffers are free
    stage_pair(s1, s2, t.y0, t.x0, H, W, [&](int64_t o, float& xv, float& gv) {
      xv = clamped(exposed<EXP>(rn, hw, o, j, ec), im.clamp);
      if (mn) xv *= mn[o];
      gv = gn[j * hw + o];
    });
    __syncthreads();

    float own_x[kRows], own_g[kRows];
#pragma unroll
    for (int k = 0; k < kRows; ++k) {
      own_x[k] = s1[r0 + k * kRowsPerPass + kHalo][c + kHalo];
      own_g[k] = s2[r0 + k * kRowsPerPass + kHalo][c + kHalo];
    }
    filter_rows_moments(s1, s2, hm, win);
    __syncthreads();

    const int64_t base = (t.n * im.C + j) * hw;
#pragma unroll
    for (int k = 0; k < kRows; ++k) {
      const int rr = r0 + k * kRowsPerPass;
      const int y = t.y0 + rr;
      float f[5];
      filter_column(hm, rr, c, win, f);
      if (y < H && x < W) {
        const int64_t o = base + (int64_t)y * W + x;
        acc[0] += (double)fabsf(own_x[k] - own_g[k]);
        acc[1] += (double)ssim_pixel(f, maps ? maps + o : nullptr, total);
      }
    }
  }

  if (im.d) {
#pragma unroll
    for (int k = 0; k < kRows; ++k) {
      const int y = t.y0 + r0 + k * kRowsPerPass;
      if (y < H && x < W) {
        const int64_t o = t.n * hw + (int64_t)y * W + x;
        acc[2] += (double)fabsf((im.d[o] - im.mono[o]) * im.md[o]);
      }
    }
  }
  block_sums_store<3>(acc, wsum, partials, blocks);
}

// One workgroup: each of the three partial arrays summed in a fixed order; out = loss, L1, S, D.
__global__ __launch_bounds__(kReduceThreads) void photo_reduce_kernel(const double* __restrict__ partials,
                                                                      int64_t blocks, double inv_px, double inv_dpx,
                                                                      double lambda, double depth_weight,
                                                                      float* __restrict__ out) {
  __shared__ double wsum[kReduceThreads / 64];
  double s[3];
  for (int k = 0; k < 3; ++k) {
    const double* p = partials + k * blocks;
    double v = 0.0;
    for (int64_t i = threadIdx.x; i < blocks; i += kReduceThreads) v += p[i];
    s[k] = block_sum(v, wsum);
    __syncthreads();      // wsum is reused by the next sum
  }
  if (threadIdx.x == 0) {
    const double l1 = s[0] * inv_px, S = s[1] * inv_px, D = s[2] * inv_dpx;
    out[0] = (float)((1.0 - lambda) * l1 + lambda * (1.0 - S) + depth_weight * D);
    out[1] = (float)l1;
    out[2] = (float)S;
    out[3] = (float)D;
  }
}

template <bool EXP>
__global__ __launch_bounds__(kThreads) void photo_bwd_kernel(Images im, Window win, int64_t total,
                                                             const float* __restrict__ maps,
                                                             const float* __restrict__ g, double l1_scale,
                                                             double ssim_scale, double depth_scale,
                                                             float* __restrict__ grad_r, float* __restrict__ grad_d,
                                                             double* __restrict__ partials, int64_t blocks) {
  __shared__ float sm[3][kIH][kIW];
  __shared__ float hm[3][kIH][kTW];
  __shared__ double wsum[kExp][kWaves];
  const Tile t = tile_of(im);
  const int H = im.H, W = im.W;
  const int64_t hw = (int64_t)H * W;
  const float* rn = im.r + t.n * im.C * hw;
  const float* gn = im.gt + t.n * im.C * hw;
  const float* mn = im.mask ? im.mask + t.n * hw : nullptr;
  const float* En = EXP ? im.E + t.n * kExp : nullptr;
  float* grn = grad_r + t.n * im.C * hw;
  const int tid = threadIdx.x;
  const int c = tid % kTW, r0 = tid / kTW;
  const int x = t.x0 + c;
  const double up = (double)g[0];
  const float cl1 = (float)(l1_scale * up);        // (1 - lambda) g / count
  const float cs = (float)(ssim_scale * up);       // -lambda g / count

  bool own[kRows];
  int64_t off[kRows];
  float mk[kRows];
  float du[kRows][3];       // EXP only: the loop over j is unrolled, so these stay in registers
#pragma unroll
  for (int k = 0; k < kRows; ++k) {
    const int y = t.y0 + r0 + k * kRowsPerPass;
    own[k] = y < H && x < W;
    off[k] = own[k] ? (int64_t)y * W + x : 0;
    mk[k] = mn ? mn[off[k]] : 1.f;
#pragma unroll
    for (int j = 0; j < 3; ++j) du[k][j] = 0.f;
  }

  auto channel = [&](int j, float (&du_j)[kRows]) {
    const float* mj = maps + (t.n * im.C + j) * hw;
    // hm of the previous channel may still be read; sm is not (a barrier separates its last read from here)
    stage_maps(sm, mj, total, t.y0, t.x0, H, W);
    __syncthreads();
    filter_rows_maps(sm, hm, win);
    __syncthreads();
    const ExpCol ec = exp_col<EXP>(En, j);
#pragma unroll
    for (int k = 0; k < kRows; ++k) {
      const int rr = r0 + k * kRowsPerPass;
      float f[3];
      filter_column(hm, rr, c, win, f);
      du_j[k] = 0.f;
      if (own[k]) {
        const float u = exposed<EXP>(rn, hw, off[k], j, ec);
        const bool pass = !im.clamp || (u >= 0.f && u <= 1.f);
        const float xv = clamped(u, im.clamp) * mk[k];
        const float gv = gn[j * hw + off[k]];
        const float dx = cs * ssim_pixel_grad(f, xv, gv) + cl1 * sign_of(xv - gv);
        du_j[k] = pass ? dx * mk[k] : 0.f;
      }
    }
  };

  if (EXP) {
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      float d_j[kRows];
      channel(j, d_j);
#pragma unroll
      for (int k = 0; k < kRows; ++k) du[k][j] = d_j[k];
    }
    double acc[kExp];
#pragma unroll
    for (int e = 0; e < kExp; ++e) acc[e] = 0.0;
#pragma unroll
    for (int k = 0; k < kRows; ++k) {
      if (!own[k]) continue;
      float rv[3];
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        rv[i] = rn[i * hw + off[k]];
        grn[i * hw + off[k]] = fmaf(En[4 * i + 2], du[k][2], fmaf(En[4 * i + 1], du[k][1], En[4 * i] * du[k][0]));
      }
      if (partials) {
#pragma unroll
        for (int i = 0; i < 3; ++i) {
#pragma unroll
          for (int j = 0; j < 3; ++j) acc[4 * i + j] += (double)rv[i] * (double)du[k][j];
          acc[4 * i + 3] += (double)du[k][i];
        }
      }
    }
    if (partials) block_sums_store<kExp>(acc, wsum, partials, blocks);
  } else {
    for (int j = 0; j < im.C; ++j) {
      float d_j[kRows];
      channel(j, d_j);
#pragma unroll
      for (int k = 0; k < kRows; ++k)
        if (own[k]) grn[j * hw + off[k]] = d_j[k];
    }
  }

  if (grad_d) {
    const float gd = (float)(depth_scale * up);      // depth_weight g / count_d
#pragma unroll
    for (int k = 0; k < kRows; ++k) {
      if (!own[k]) continue;
      const int64_t o = t.n * hw + off[k];
      const float md = im.md[o];
      grad_d[o] = gd * sign_of((im.d[o] - im.mono[o]) * md) * md;
    }
  }
}

// Workgroup b = n * 12 + k: image n's partials of exposure entry k, in a fixed order.
__global__ __launch_bounds__(kThreads) void photo_exposure_reduce_kernel(const double* __restrict__ partials,
                                                                         int64_t blocks, int tiles_per_image,
                                                                         float* __restrict__ grad_E) {
  __shared__ double wsum[kWaves];
  const int n = blockIdx.x / kExp, k = blockIdx.x - n * kExp;
  const double* p = partials + k * blocks + (int64_t)n * tiles_per_image;
  double v = 0.0;
  for (int i = threadIdx.x; i < tiles_per_image; i += kThreads) v += p[i];
  const double s = block_sum(v, wsum);
  if (threadIdx.x == 0) grad_E[blockIdx.x] = (float)s;
}

struct Grid {
  Images im;
  int64_t blocks, total, depth_px;
};

Grid grid_of(const hgs_photo_args& a) {
  Grid g;
  g.im.r = a.rendered;
  g.im.gt = a.gt;
  g.im.E = a.exposure;
  g.im.mask = a.alpha_mask;
  g.im.d = a.invdepth;
  g.im.mono = a.mono_invdepth;
  g.im.md = a.depth_mask;
  g.im.C = a.C;
  g.im.H = a.H;
  g.im.W = a.W;
  g.im.tiles_x = (a.W + kTW - 1) / kTW;
  g.im.tiles_per_image = g.im.tiles_x * ((a.H + kTH - 1) / kTH);
  g.im.clamp = a.clamp ? 1 : 0;
  g.blocks = (int64_t)a.N * g.im.tiles_per_image;
  g.total = (int64_t)a.N * a.C * a.H * a.W;
  g.depth_px = (int64_t)a.N * a.H * a.W;
  return g;
}

}  // namespace

size_t photo_tmp_bytes(int32_t N, int32_t C, int32_t H, int32_t W) {
  hgs_photo_args a = {};
  a.N = N, a.C = C, a.H = H, a.W = W;
  return align_up((size_t)grid_of(a).blocks * kExp * sizeof(double));
}

int launch_photo_fwd(const hgs_photo_args& a, float* out, float* maps, void* tmp, hipStream_t s) {
  const Grid g = grid_of(a);
  const Window win = gaussian_window();
  double* partials = static_cast<double*>(tmp);
  if (a.exposure)
    photo_fwd_kernel<true><<<(unsigned)g.blocks, kThreads, 0, s>>>(g.im, win, g.total, maps, partials, g.blocks);
  else
    photo_fwd_kernel<false><<<(unsigned)g.blocks, kThreads, 0, s>>>(g.im, win, g.total, maps, partials, g.blocks);
  HGS_LAUNCH_CHECK("photo_fwd_kernel", s, false);
  photo_reduce_kernel<<<1, kReduceThreads, 0, s>>>(partials, g.blocks, 1.0 / (double)g.total, 1.0 / (double)g.depth_px,
                                                   a.lambda_dssim, a.invdepth ? a.depth_weight : 0.0, out);
  HGS_LAUNCH_CHECK("photo_reduce_kernel", s, false);
  return HGS_OK;
}

int launch_photo_bwd(const hgs_photo_args& a, const float* maps, const float* grad_out, float* grad_rendered,
                     float* grad_exposure, float* grad_invdepth, void* tmp, hipStream_t s) {
  const Grid g = grid_of(a);
  const Window win = gaussian_window();
  double* partials = grad_exposure ? static_cast<double*>(tmp) : nullptr;
  const double l1_scale = (1.0 - a.lambda_dssim) / (double)g.total, ssim_scale = -a.lambda_dssim / (double)g.total;
  const double depth_scale = a.depth_weight / (double)g.depth_px;
  if (a.exposure)
    photo_bwd_kernel<true><<<(unsigned)g.blocks, kThreads, 0, s>>>(g.im, win, g.total, maps, grad_out, l1_scale,
                                                                    ssim_scale, depth_scale, grad_rendered,
                                                                    grad_invdepth, partials, g.blocks);
  else
    photo_bwd_kernel<false><<<(unsigned)g.blocks, kThreads, 0, s>>>(g.im, win, g.total, maps, grad_out, l1_scale,
                                                                     ssim_scale, depth_scale, grad_rendered,
                                                                     grad_invdepth, partials, g.blocks);
  HGS_LAUNCH_CHECK("photo_bwd_kernel", s, false);
  if (grad_exposure) {
    photo_exposure_reduce_kernel<<<(unsigned)(a.N * kExp), kThreads, 0, s>>>(partials, g.blocks, g.im.tiles_per_image,
                                                                             grad_exposure);
    HGS_LAUNCH_CHECK("photo_exposure_reduce_kernel", s, false);
  }
  return HGS_OK;
}

}  // namespace hgs
