// Per-pixel readout of one forward: for every pixel the rows K6 blended there, front to
// back, reduced to eight planes -- the covered share 1 - T, the number of rows, the first and the last row, the row of
// the largest weight w = alpha * T_before with that weight, and the first row after which T falls below one half with
// the view-space depth K1 stored for it.  f-22 and f-23 (contrib.hip, attribute.hip) read a forward from the rows'
// side and end in per-row arrays; this file answers the opposite question, what a pixel shows.
//
// One kernel, no atomics, no scratch, bit-reproducible:
//  * pixels_tile_kernel: the tile walk of tile_walk.h.  The staged record carries, in the two words that hold K6's
//    colour in the other walks, the row's ID AFTER THE SLOT MAP and its DEPTH BITS: the map and GeomWs::depths are read
//    once per instance by the staging lane, the map's entry is bounded there, and the visit reads nothing from global
//    memory.
//    A pixel's answer lives in ONE LANE's registers (per pixel: T, the row coordinate, count, front, back, best weight
//    and its id, median id and its depth): no cross-lane reduction, no LDS accumulator, no barrier after the visits, no
//    second kernel.  Updates are selects: `front` while count == 0, the heaviest on a strict > (the front-most row wins
//    equal bits), the median while it is unset and T after the row < 0.5f.  An ignored row (id -2) still occludes and
//    counts; it only cannot be named.  Every pixel inside the image is stored to every non-NULL plane by plain vector
//    stores, so the caller need not pre-fill; with `empty` (L == 0 or P == 0) no workspace is read and the planes take
//    the "nothing" values.
//  Measured: profiles/f24_pixels_kernels.md.
#include "tile_walk.h"

#pragma clang fp contract(off)

namespace hgs {
namespace {

constexpr int kNoRow = -1;        // id where no row answers
constexpr int kIgnoredRow = -2;   // id of a row the slot map does not name

__global__ __launch_bounds__(64) void pixels_tile_kernel(
    const uint32_t* __restrict__ ranges, const uint32_t* __restrict__ point_list, const float4* __restrict__ records,
    const float* __restrict__ depths, int W, int H, int gx, int T, const uint32_t* __restrict__ order,
    const int32_t* __restrict__ slot_of_row, long long n_slots, hgs_raster_pixel_planes out, int empty) {
  __shared__ float4 lrec[(kBatch + 1) * 2];       // the staged instances (tile_walk.h): (.., .., id bits, depth bits)
  __shared__ uint16_t qlist[(kBatch + 1) * 4];    // the quadrants' lists

  const int tile = block_tile(T, order);
  if ((uint32_t)tile >= (uint32_t)T) return;
  const TileLane t(tile, gx);
  const int lane = t.lane;

  float fly[4], Tp[4], best[4], mdepth[4];
  int cnt[4], front[4], back[4], heavy[4], med[4];
  bool inside[4];
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    inside[s] = t.inside(s, W, H);
    fly[s] = t.fly0(s, inside[s]);
    Tp[s] = 1.0f;
    best[s] = 0.0f;
    mdepth[s] = 0.0f;
    cnt[s] = 0;
    front[s] = back[s] = heavy[s] = med[s] = kNoRow;
  }
  t.open(lrec);

  uint32_t r0 = 0, r1 = 0;
  if (!empty) { r0 = ranges[tile * 2 + 0]; r1 = ranges[tile * 2 + 1]; }
  uint64_t alive = alive_lanes(fly);
  for (uint32_t base = r0; base < r1 && alive != 0; base += kBatch) {
    const int n = __builtin_amdgcn_readfirstlane((int)min((uint32_t)kBatch, r1 - base));
    __syncthreads();
    bool hit[4] = {false, false, false, false};
    if (lane < n) {
      float4 a0, a1, a2;
      const uint32_t gid = t.stage(point_list, records, base + lane, alive, a0, a1, a2, hit);
      // the row's id after the slot map, bounded here; its depth as K1 stored it
      int id = (int)gid;
      if (slot_of_row) {
        const long long sl = (long long)slot_of_row[gid];
        id = (sl >= 0 && sl < n_slots) ? (int)sl : kIgnoredRow;
      }
      a1.z = __int_as_float(id);
      a1.w = depths[gid];
      lrec[lane * 2 + 0] = a0;
      lrec[lane * 2 + 1] = a1;
    }
    const int nmax = t.file(qlist, hit);
    __syncthreads();
    for (int it = 0; it < nmax; ++it) {
      const uint32_t j = qlist[it * 4 + t.q];
      const float4 q0 = lrec[j * 2 + 0], q1 = lrec[j * 2 + 1];
      const int id = __float_as_int(q1.z);
      const float dx = q0.x - t.flx;
      const float ax = q0.z * dx * dx;
      const float bx = q0.w * dx;
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        const Blend b = blend_pixel(q0, q1, ax, bx, fly[s], Tp[s]);
        const bool blend = b.blend;
        const float w = b.w, Tn = b.Tn;
        front[s] = (blend && cnt[s] == 0) ? id : front[s];
        back[s] = blend ? id : back[s];
        cnt[s] += blend ? 1 : 0;
        const bool heavier = blend && w > best[s];      // strict: the front-most row keeps equal bits
        heavy[s] = heavier ? id : heavy[s];
        best[s] = heavier ? w : best[s];
        const bool half = blend && med[s] == kNoRow && Tn < 0.5f;
        med[s] = half ? id : med[s];
        mdepth[s] = half ? q1.w : mdepth[s];
        Tp[s] = b.T_after(Tp[s]);
        fly[s] = b.fly_after(fly[s]);
      }
    }
    alive = alive_lanes(fly);
  }
  // a median row the map ignores is named -2 and keeps its depth; where there is no median the depth is 0
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    if (!inside[s]) continue;
    const size_t p = (size_t)t.py(s) * (size_t)W + (size_t)t.px;
    if (out.alpha) out.alpha[p] = 1.0f - Tp[s];
    if (out.count) out.count[p] = cnt[s];
    if (out.front) out.front[p] = front[s];
    if (out.back) out.back[p] = back[s];
    if (out.heaviest) out.heaviest[p] = heavy[s];
    if (out.wmax) out.wmax[p] = best[s];
    if (out.median) out.median[p] = med[s];
    if (out.median_depth) out.median_depth[p] = mdepth[s];
  }
}

}  // namespace

int launch_raster_pixels(const hgs_raster_args& a, const GeomWs& g, const BinWs& b, bool empty,
                         const int32_t* slot_of_row, int64_t n_slots, const hgs_raster_pixel_planes& out, hipStream_t s) {
  const int gxx = grid_x(a.width), T = gxx * grid_y(a.height);
  const int nblk = ((T + 7) / 8) * 8;
  hipLaunchKernelGGL(pixels_tile_kernel, dim3(nblk), dim3(64), 0, s, b.ranges, b.vals_out,
                     reinterpret_cast<const float4*>(g.records), g.depths, a.width, a.height, gxx, T,
                     empty ? nullptr : b.tile_order, slot_of_row, (long long)n_slots, out, empty ? 1 : 0);
  HGS_LAUNCH_CHECK("pixels_tile", s, a.debug);
  return HGS_OK;
}

}  // namespace hgs
