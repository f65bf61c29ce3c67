// Per-Gaussian blending statistics of one forward: for every row the largest weight
// w = alpha * T it reaches at a pixel, the sum of its weights and the number of pixels it is blended into.  Nothing
// upstream computes these; the sum alone could be had here as d(sum of an image channel) / d colors_precomp through
// K7 and K8 -- the whole backward for one number.
//
// Two kernels in the shape of K7 / K8 (no atomics anywhere, bit-reproducible), both instances of tile_walk.h:
//  * contrib_tile_kernel: the tile walk with per-instance records (largest weight, sum of weights, pixel count as bits,
//    0).  A pixel the mask does not count, or at which the row is not blended, adds a selected zero; the count is
//    carried as a float (at most 64 per pair, 256 per record: exact).
//  * contrib_sum_kernel: the run sum with (max, float64 sum, integer count) and a plain read-modify-write into the
//    row's slot.
//  Measured: profiles/f22_contrib_kernels.md.
#include "tile_walk.h"

#pragma clang fp contract(off)

namespace hgs {
namespace {

__global__ __launch_bounds__(64) void contrib_tile_kernel(
    const uint32_t* __restrict__ ranges, const uint32_t* __restrict__ point_list, const float4* __restrict__ records,
    int W, int H, int gx, int T, const uint32_t* __restrict__ order, const uint32_t* __restrict__ offsets,
    const uint8_t* __restrict__ pixel_mask, float4* __restrict__ inst, uint32_t L) {
  __shared__ float4 lrec[(kBatch + 1) * 2];       // the staged instances (tile_walk.h)
  __shared__ uint16_t qlist[(kBatch + 1) * 4];    // the quadrants' lists
  __shared__ float4 acc[(kBatch + 1) * 4];        // (largest weight, sum, pixel count, -) of every pair

  const int tile = block_tile(T, order);
  if ((uint32_t)tile >= (uint32_t)T) return;
  const TileLane t(tile, gx);
  const int lane = t.lane;

  float fly[4], Tp[4];
  bool counted[4];
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    const bool inside = t.inside(s, W, H);
    fly[s] = t.fly0(s, inside);
    Tp[s] = 1.0f;
    count_pixel(t, s, inside, W, pixel_mask, counted);
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
      float w[4], c = 0.0f;
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        const Blend b = blend_pixel(q0, q1, ax, bx, fly[s], Tp[s]);
        w[s] = (b.blend && counted[s]) ? b.w : 0.0f;
        c += (b.blend && counted[s]) ? 1.0f : 0.0f;
        Tp[s] = b.T_after(Tp[s]);
        fly[s] = b.fly_after(fly[s]);
      }
      // the pair's 64 pixel slots in a fixed order: the lane's four, then a butterfly over the row (the count as a
      // float: at most 64, exact)
      const float tmax = row_max(fmaxf(fmaxf(w[0], w[1]), fmaxf(w[2], w[3])));
      const float tsum = row_sum((w[0] + w[1]) + (w[2] + w[3]));
      const float tcnt = row_sum(c);
      if (leader) acc[j * 4 + t.q] = make_float4(tmax, tsum, tcnt, 0.0f);
    }
    __syncthreads();
    // lane i adds up instance i's pairs in quadrant order and stores the record to its emission slot: every staged
    // instance is written, reached or not
    if (my_e < L) {
      float rmax = 0.0f, rsum = 0.0f, rcnt = 0.0f;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if (hit[k]) {
          const float4 p = acc[lane * 4 + k];
          rmax = fmaxf(rmax, p.x);
          rsum += p.y;
          rcnt += p.z;
        }
      }
      inst[my_e] = make_float4(rmax, rsum, __uint_as_float((uint32_t)rcnt), 0.0f);
    }
    alive = alive_lanes(fly);
  }
  zero_tail(t, base, r1, point_list, records, offsets, inst, L);
}

struct ContribSum {
  float m;
  double sum;
  long long c;
  __device__ __forceinline__ void add(const float4& r) {
    m = fmaxf(m, r.x);
    sum += (double)r.y;
    c += (long long)__float_as_uint(r.z);
  }
  __device__ __forceinline__ void add_lane(int d) {
    m = fmaxf(m, __shfl_xor(m, d, 64));
    sum += __shfl_xor(sum, d, 64);
    c += __shfl_xor(c, d, 64);
  }
  __device__ __forceinline__ bool nowhere() const { return c == 0; }
};

__global__ __launch_bounds__(kSumBlock) void contrib_sum_kernel(
    int P, const uint32_t* __restrict__ tiles_touched, const uint32_t* __restrict__ offsets,
    const float4* __restrict__ inst, uint32_t L, const int32_t* __restrict__ slot_of_row, long long n_slots,
    float* __restrict__ wmax, double* __restrict__ wsum, long long* __restrict__ count) {
  long long s;
  ContribSum a{};
  if (!run_sum(P, tiles_touched, offsets, inst, L, slot_of_row, n_slots, s, a)) return;
  wmax[s] = fmaxf(wmax[s], a.m);
  wsum[s] += a.sum;
  count[s] += a.c;
}

}  // namespace

int launch_raster_contrib(const hgs_raster_args& a, const GeomWs& g, const BinWs& b, const ContribWs& w, uint32_t L,
                          const uint8_t* pixel_mask, const int32_t* slot_of_row, int64_t n_slots, float* wmax,
                          double* wsum, int64_t* count, hipStream_t s) {
  const int gxx = grid_x(a.width), T = gxx * grid_y(a.height);
  const int nblk = ((T + 7) / 8) * 8;
  float4* inst = reinterpret_cast<float4*>(w.inst);
  hipLaunchKernelGGL(contrib_tile_kernel, dim3(nblk), dim3(64), 0, s, b.ranges, b.vals_out,
                     reinterpret_cast<const float4*>(g.records), a.width, a.height, gxx, T, b.tile_order, g.offsets,
                     pixel_mask, inst, L);
  HGS_LAUNCH_CHECK("contrib_tile", s, a.debug);
  hipLaunchKernelGGL(contrib_sum_kernel, dim3((a.P + kSumBlock - 1) / kSumBlock), dim3(kSumBlock), 0, s, a.P,
                     g.tiles_touched, g.offsets, inst, L, slot_of_row, (long long)n_slots, wmax, wsum,
                     reinterpret_cast<long long*>(count));
  HGS_LAUNCH_CHECK("contrib_sum", s, a.debug);
  return HGS_OK;
}

}  // namespace hgs
