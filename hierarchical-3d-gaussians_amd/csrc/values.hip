// Per-row values painted into the picture with the forward's blend weights: for every pixel
// p inside the image and every channel c < C,
//     out[c][p] = sum over the rows K6 blended at p, front to back, of  w(p) * values[slot(row)][c]  +  T_final(p) * bg[c],
// with w = alpha * T_before as K6 added it to the colour, and optionally the plane of the weights of the NAMED rows
// themselves.  This is the dual of f-23 (attribute.hip scatters a per-pixel image onto rows; this file gathers a
// per-row table into a per-pixel image) and what a second forward with colors_precomp would render -- without K1, the
// binning and the sort, with up to four channels per launch, and with the table indexed through a slot map (the
// render_indices of a cut: values per hierarchy node).
//
// One kernel, no atomics, no scratch, bit-reproducible:
//  * values_tile_kernel<C, WSUM>: the tile walk of tile_walk.h in the shape of pixels_tile_kernel.  The staging lane
//    resolves the row's slot (slot_of_row[gid] when that lies in [0, n_slots); gid itself without a map), loads the
//    slot's C floats ONCE per instance and stores them as one float4 to a third LDS array beside the records (`lval`,
//    zeros at the dummy index kBatch); the word of the record that holds K6's red in the other walks carries whether
//    the row is NAMED.  A row the map ignores stages zeros and its values are never read: it still occludes, it adds
//    nothing to `out` or `wsum`.  The visit reads nothing from global memory.
//    A pixel's sums live in ONE LANE's registers (per pixel: T, the row coordinate, C accumulators, the weight sum): no
//    cross-lane reduction, no LDS accumulator, no barrier after the visits, no second kernel.  Per channel
//    acc = blend ? fmaf(w, v, acc) : acc  in list order -- a SELECT, not a zero weight: with finite values these are
//    K6's bits (fma2(w, colour, C) with w = 0 off the blend set: x + 0 is x, and no accumulator is ever -0), and a NaN
//    or an infinity in a row's value reaches exactly the pixels the row is blended at.
//    The epilogue rounds as K6's does: there  C + T * bg  is contracted, one fused multiply-add, and here it is written
//    as one.  Without a background the accumulator's bits are stored.  Every pixel inside the image is stored to every
//    given plane by plain vector stores, so the caller need not pre-fill; with `empty` (L == 0 or P == 0) no workspace
//    and no value is read, `out` takes the background and `wsum` zeros.
//  Measured: profiles/f26_values_kernels.md.
#include "tile_walk.h"

#pragma clang fp contract(off)

namespace hgs {
namespace {

template <int C, bool WSUM>
__global__ __launch_bounds__(64) void values_tile_kernel(
    const uint32_t* __restrict__ ranges, const uint32_t* __restrict__ point_list, const float4* __restrict__ records,
    int W, int H, int gx, int T, const uint32_t* __restrict__ order, const int32_t* __restrict__ slot_of_row,
    long long n_slots, const float* __restrict__ values, long long stride, const float* __restrict__ bg,
    float* __restrict__ out, float* __restrict__ wsum, int empty) {
  __shared__ float4 lrec[(kBatch + 1) * 2];       // the staged instances (tile_walk.h): (.., .., named, -)
  __shared__ uint16_t qlist[(kBatch + 1) * 4];    // the quadrants' lists
  __shared__ float4 lval[kBatch + 1];             // the staged instances' values (unused channels zero)

  const int tile = block_tile(T, order);
  if ((uint32_t)tile >= (uint32_t)T) return;
  const TileLane t(tile, gx);
  const int lane = t.lane;

  float fly[4], Tp[4], acc[C][4], ws[4];
  bool inside[4];
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    inside[s] = t.inside(s, W, H);
    fly[s] = t.fly0(s, inside[s]);
    Tp[s] = 1.0f;
    ws[s] = 0.0f;
#pragma unroll
    for (int c = 0; c < C; ++c) acc[c][s] = 0.0f;
  }
  t.open(lrec);
  if (lane == 0) lval[kBatch] = make_float4(0.f, 0.f, 0.f, 0.f);

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
      // the row's slot, bounded here; the slot's values, read once per instance
      const long long sl = slot_of_row ? (long long)slot_of_row[gid] : (long long)gid;
      const bool named = sl >= 0 && sl < n_slots;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (named) {
        const float* r = values + sl * stride;
        v.x = r[0];
        if constexpr (C > 1) v.y = r[1];
        if constexpr (C > 2) v.z = r[2];
        if constexpr (C > 3) v.w = r[3];
      }
      a1.z = __int_as_float(named ? 1 : 0);
      lrec[lane * 2 + 0] = a0;
      lrec[lane * 2 + 1] = a1;
      lval[lane] = v;
    }
    const int nmax = t.file(qlist, hit);
    __syncthreads();
    for (int it = 0; it < nmax; ++it) {
      const uint32_t j = qlist[it * 4 + t.q];
      const float4 q0 = lrec[j * 2 + 0], q1 = lrec[j * 2 + 1];
      const float4 v = lval[j];
      const bool named = __float_as_int(q1.z) != 0;
      const float dx = q0.x - t.flx;
      const float ax = q0.z * dx * dx;
      const float bx = q0.w * dx;
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        const Blend b = blend_pixel(q0, q1, ax, bx, fly[s], Tp[s]);
        const bool blend = b.blend;
        const float w = b.w;
        acc[0][s] = blend ? fmaf(w, v.x, acc[0][s]) : acc[0][s];
        if constexpr (C > 1) acc[1][s] = blend ? fmaf(w, v.y, acc[1][s]) : acc[1][s];
        if constexpr (C > 2) acc[2][s] = blend ? fmaf(w, v.z, acc[2][s]) : acc[2][s];
        if constexpr (C > 3) acc[3][s] = blend ? fmaf(w, v.w, acc[3][s]) : acc[3][s];
        if constexpr (WSUM) ws[s] = (blend && named) ? ws[s] + w : ws[s];
        Tp[s] = b.T_after(Tp[s]);
        fly[s] = b.fly_after(fly[s]);
      }
    }
    alive = alive_lanes(fly);
  }

  float b[C];
#pragma unroll
  for (int c = 0; c < C; ++c) b[c] = bg ? bg[c] : 0.0f;
  const size_t plane = (size_t)W * (size_t)H;
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    if (!inside[s]) continue;
    const size_t p = (size_t)t.py(s) * (size_t)W + (size_t)t.px;
    // K6's epilogue: one fused multiply-add; without a background the accumulator's own bits
#pragma unroll
    for (int c = 0; c < C; ++c) out[(size_t)c * plane + p] = bg ? fmaf(Tp[s], b[c], acc[c][s]) : acc[c][s];
    if constexpr (WSUM) wsum[p] = ws[s];
  }
}

template <int C, bool WSUM>
void launch_cw(const hgs_raster_args& a, const GeomWs& g, const BinWs& b, bool empty, const float* values,
               int64_t value_stride, const int32_t* slot_of_row, int64_t n_slots, const float* background, float* out,
               float* wsum, hipStream_t s) {
  const int gxx = grid_x(a.width), T = gxx * grid_y(a.height);
  const int nblk = ((T + 7) / 8) * 8;
  hipLaunchKernelGGL((values_tile_kernel<C, WSUM>), dim3(nblk), dim3(64), 0, s, b.ranges, b.vals_out,
                     reinterpret_cast<const float4*>(g.records), a.width, a.height, gxx, T,
                     empty ? nullptr : b.tile_order, slot_of_row, (long long)n_slots, values, (long long)value_stride,
                     background, out, wsum, empty ? 1 : 0);
}

template <int C>
void launch_c(const hgs_raster_args& a, const GeomWs& g, const BinWs& b, bool empty, const float* values,
              int64_t value_stride, const int32_t* slot_of_row, int64_t n_slots, const float* background, float* out,
              float* wsum, hipStream_t s) {
  if (wsum) launch_cw<C, true>(a, g, b, empty, values, value_stride, slot_of_row, n_slots, background, out, wsum, s);
  else launch_cw<C, false>(a, g, b, empty, values, value_stride, slot_of_row, n_slots, background, out, wsum, s);
}

}  // namespace

int launch_raster_values(const hgs_raster_args& a, const GeomWs& g, const BinWs& b, bool empty, const float* values,
                         int64_t value_stride, int channels, const int32_t* slot_of_row, int64_t n_slots,
                         const float* background, float* out, float* wsum, hipStream_t s) {
  switch (channels) {
    case 1: launch_c<1>(a, g, b, empty, values, value_stride, slot_of_row, n_slots, background, out, wsum, s); break;
    case 2: launch_c<2>(a, g, b, empty, values, value_stride, slot_of_row, n_slots, background, out, wsum, s); break;
    case 3: launch_c<3>(a, g, b, empty, values, value_stride, slot_of_row, n_slots, background, out, wsum, s); break;
    default: launch_c<4>(a, g, b, empty, values, value_stride, slot_of_row, n_slots, background, out, wsum, s); break;
  }
  HGS_LAUNCH_CHECK("values_tile", s, a.debug);
  return HGS_OK;
}

}  // namespace hgs
