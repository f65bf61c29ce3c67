// Attribution of a per-pixel image to the Gaussians that blend it: for every row i of one
// forward and every channel c < C of a planar float32 image f [C, H, W],
//     A[i, c] = sum over the counted pixels p at which K6 blends row i of  w_i(p) * f_c(p),     w = alpha * T_before,
// and the sum of the weights themselves.  This is dL / d colors_precomp of a backward seeded with f -- the whole of K7 and
// K8 for C numbers per row, refused on the in-op LOD route and without a slot map -- computed on the forward's side.
//
// Two kernels in the shape of contrib.hip (f-22), both instances of tile_walk.h; no atomics anywhere, bit-reproducible:
//  * attribute_tile_kernel<C>: the tile walk with per-instance records (A0, A1, A2, sum of weights; unused channels
//    zero).  Each lane loads f_c of its four pixels once (4 C registers; a pixel that is outside the image or masked out
//    is never read).  Per (instance, quadrant) pair and pixel it forms t_c = w * f_c, ONE rounded product, and w; a pixel
//    that is not counted, or at which the row is not blended, contributes a SELECTED 0.0f, never 0 * f: a NaN or an
//    infinity there reaches no output.  The pair's 64 pixel slots are reduced in f-22's one fixed order -- (t0 + t1) +
//    (t2 + t3), then the DPP butterfly over the row.  The fourth component goes through exactly the operations of
//    f-22's `wsum`, so the two are equal bit for bit, and so is a channel of ones (w * 1.0f is w).
//  * attribute_sum_kernel<C>: the run sum with float64 accumulators and a plain read-modify-write into
//    out[slot * C + c] and, when given, wsum[slot].  A row whose summed wsum is zero (blended at no counted pixel: a
//    weight is at least 1e-4 / 255) writes nothing.
//  Measured: profiles/f23_attribute_kernels.md.
#include "tile_walk.h"

#pragma clang fp contract(off)

namespace hgs {
namespace {

template <int C>
__global__ __launch_bounds__(64) void attribute_tile_kernel(
    const uint32_t* __restrict__ ranges, const uint32_t* __restrict__ point_list, const float4* __restrict__ records,
    int W, int H, int gx, int T, const uint32_t* __restrict__ order, const uint32_t* __restrict__ offsets,
    const float* __restrict__ image, const uint8_t* __restrict__ pixel_mask, float4* __restrict__ inst, uint32_t L) {
  __shared__ float4 lrec[(kBatch + 1) * 2];       // the staged instances (tile_walk.h)
  __shared__ uint16_t qlist[(kBatch + 1) * 4];    // the quadrants' lists
  __shared__ float4 acc[(kBatch + 1) * 4];        // (A0, A1, A2, sum of weights) of every pair

  const int tile = block_tile(T, order);
  if ((uint32_t)tile >= (uint32_t)T) return;
  const TileLane t(tile, gx);
  const int lane = t.lane;
  const size_t plane = (size_t)W * (size_t)H;

  float fly[4], Tp[4], f[C][4];
  bool counted[4];
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    const bool inside = t.inside(s, W, H);
    fly[s] = t.fly0(s, inside);
    Tp[s] = 1.0f;
    count_pixel(t, s, inside, W, pixel_mask, counted);
    // the image is read at counted pixels only
#pragma unroll
    for (int c = 0; c < C; ++c) f[c][s] = counted[s] ? image[(size_t)c * plane + (size_t)t.py(s) * W + t.px] : 0.0f;
  }
  t.open(lrec);
  const bool leader = (lane & 15) == 0;

  const uint32_t r0 = ranges[tile * 2 + 0], r1 = ranges[tile * 2 + 1];
  uint64_t alive = alive_lanes(fly);
  uint32_t base = r0;
  for (; base < r1 && alive != 0; base += kBatch) {
    const int n = __builtin_amdgcn_readfirstlane((int)min((uint32_t)kBatch, r1 - base));
    __syncthreads();
    uint32_t my_e = 0xffffffffu;
    bool hit[4] = {false, false, false, false};
    if (lane < n) {
      float4 a0, a1, a2;
      const uint32_t gid = t.stage(point_list, records, base + lane, alive, a0, a1, a2, hit);
      lrec[lane * 2 + 0] = a0;
      lrec[lane * 2 + 1] = a1;
      my_e = emission_slot(offsets[gid], __float_as_uint(a2.w), t.tx, t.ty);
    }
    const int nmax = t.file(qlist, hit);
    __syncthreads();
    for (int it = 0; it < nmax; ++it) {
      const uint32_t j = qlist[it * 4 + t.q];
      const float4 q0 = lrec[j * 2 + 0], q1 = lrec[j * 2 + 1];
      const float dx = q0.x - t.flx;
      const float ax = q0.z * dx * dx;
      const float bx = q0.w * dx;
      float w[4], tc[C][4];
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        const Blend b = blend_pixel(q0, q1, ax, bx, fly[s], Tp[s]);
        const bool use = b.blend && counted[s];
        const float ws = b.w;
        w[s] = use ? ws : 0.0f;
        // one rounded product per channel; elsewhere a selected zero, never 0 * f
#pragma unroll
        for (int c = 0; c < C; ++c) tc[c][s] = use ? ws * f[c][s] : 0.0f;
        Tp[s] = b.T_after(Tp[s]);
        fly[s] = b.fly_after(fly[s]);
      }
      // the pair's 64 pixel slots in a fixed order: the lane's four, then a butterfly over the row
      float4 sums = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
      sums.x = row_sum((tc[0][0] + tc[0][1]) + (tc[0][2] + tc[0][3]));
      if constexpr (C > 1) sums.y = row_sum((tc[1][0] + tc[1][1]) + (tc[1][2] + tc[1][3]));
      if constexpr (C > 2) sums.z = row_sum((tc[2][0] + tc[2][1]) + (tc[2][2] + tc[2][3]));
      sums.w = row_sum((w[0] + w[1]) + (w[2] + w[3]));
      if (leader) acc[j * 4 + t.q] = sums;
    }
    __syncthreads();
    // lane i adds up instance i's pairs in quadrant order and stores the record to its emission slot: every staged
    // instance is written, reached or not
    if (my_e < L) {
      float4 rs = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if (hit[k]) {
          const float4 p = acc[lane * 4 + k];
          rs.x += p.x;
          rs.y += p.y;
          rs.z += p.z;
          rs.w += p.w;
        }
      }
      inst[my_e] = rs;
    }
    alive = alive_lanes(fly);
  }
  zero_tail(t, base, r1, point_list, records, offsets, inst, L);
}

template <int C>
struct AttributeSum {
  double a0, a1, a2, sw;
  __device__ __forceinline__ void add(const float4& r) {
    a0 += (double)r.x;
    if (C > 1) a1 += (double)r.y;
    if (C > 2) a2 += (double)r.z;
    sw += (double)r.w;
  }
  __device__ __forceinline__ void add_lane(int d) {
    a0 += __shfl_xor(a0, d, 64);
    if (C > 1) a1 += __shfl_xor(a1, d, 64);
    if (C > 2) a2 += __shfl_xor(a2, d, 64);
    sw += __shfl_xor(sw, d, 64);
  }
  __device__ __forceinline__ bool nowhere() const { return sw == 0.0; }
};

template <int C>
__global__ __launch_bounds__(kSumBlock) void attribute_sum_kernel(
    int P, const uint32_t* __restrict__ tiles_touched, const uint32_t* __restrict__ offsets,
    const float4* __restrict__ inst, uint32_t L, const int32_t* __restrict__ slot_of_row, long long n_slots,
    double* __restrict__ out, double* __restrict__ wsum) {
  long long s;
  AttributeSum<C> a{};
  if (!run_sum(P, tiles_touched, offsets, inst, L, slot_of_row, n_slots, s, a)) return;
  double* o = out + (size_t)s * C;
  o[0] += a.a0;
  if (C > 1) o[1] += a.a1;
  if (C > 2) o[2] += a.a2;
  if (wsum) wsum[s] += a.sw;
}

template <int C>
int launch_c(const hgs_raster_args& a, const GeomWs& g, const BinWs& b, const AttributeWs& w, uint32_t L,
             const float* image, const uint8_t* pixel_mask, const int32_t* slot_of_row, int64_t n_slots, double* out,
             double* wsum, hipStream_t s) {
  const int gxx = grid_x(a.width), T = gxx * grid_y(a.height);
  const int nblk = ((T + 7) / 8) * 8;
  float4* inst = reinterpret_cast<float4*>(w.inst);
  hipLaunchKernelGGL(attribute_tile_kernel<C>, dim3(nblk), dim3(64), 0, s, b.ranges, b.vals_out,
                     reinterpret_cast<const float4*>(g.records), a.width, a.height, gxx, T, b.tile_order, g.offsets,
                     image, pixel_mask, inst, L);
  HGS_LAUNCH_CHECK("attribute_tile", s, a.debug);
  hipLaunchKernelGGL(attribute_sum_kernel<C>, dim3((a.P + kSumBlock - 1) / kSumBlock), dim3(kSumBlock), 0, s, a.P,
                     g.tiles_touched, g.offsets, inst, L, slot_of_row, (long long)n_slots, out, wsum);
  HGS_LAUNCH_CHECK("attribute_sum", s, a.debug);
  return HGS_OK;
}

}  // namespace

int launch_raster_attribute(const hgs_raster_args& a, const GeomWs& g, const BinWs& b, const AttributeWs& w, uint32_t L,
                            const float* image, int channels, const uint8_t* pixel_mask, const int32_t* slot_of_row,
                            int64_t n_slots, double* out, double* wsum, hipStream_t s) {
  switch (channels) {
    case 1: return launch_c<1>(a, g, b, w, L, image, pixel_mask, slot_of_row, n_slots, out, wsum, s);
    case 2: return launch_c<2>(a, g, b, w, L, image, pixel_mask, slot_of_row, n_slots, out, wsum, s);
    default: return launch_c<3>(a, g, b, w, L, image, pixel_mask, slot_of_row, n_slots, out, wsum, s);
  }
}

}  // namespace hgs
