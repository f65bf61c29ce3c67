// Per-pixel readout of one forward: for every pixel the rows K6 blended there, front to
// back, reduced to eight planes -- the covered share 1 - T, the number of rows, the first and the last row, the row of
// the largest weight w = alpha * T_before with that weight, and the first row after which T falls below one half with
// the view-space depth K1 stored for it.  f-22 and f-23 (contrib.hip, attribute.hip) read a forward from the rows'
// side and end in per-row arrays; this file answers the opposite question, what a pixel shows.
//
// One kernel, no atomics, no scratch, bit-reproducible:
//  * pixels_tile_kernel: ONE WAVE PER 16x16 TILE in K6's XCD-aware tile order.  The wave re-walks the tile's
//    depth-sorted list front to back in batches of 64 records staged through LDS and repeats K6's per-pixel decisions on
//    the same 64-byte records with the same float32 expressions (exp2_le1, the 0.99 cap, alpha >= 1/255,
//    T (1 - alpha) < 1e-4 stops the pixel; contraction is off for the file), four QUADRANT STREAMS as in K7, f-22 and
//    f-23: the staging lane tests K1's alpha >= 1/255 box against the quadrants, four ballots file the instance into the
//    lists by rank, one (instance, quadrant) pair per DPP row and iteration.  The staged record carries, in the two
//    words that hold K6's colour in contrib.hip, the row's ID AFTER THE SLOT MAP and its DEPTH BITS: the map and
//    GeomWs::depths are read once per instance by the staging lane, the map's entry is bounded there, and the visit
//    reads nothing from global memory.
//    A pixel's answer lives in ONE LANE's registers (per pixel: T, the row coordinate, count, front, back, best weight
//    and its id, median id and its depth): no cross-lane reduction, no LDS accumulator, no second kernel.  Updates are
//    selects: `front` while count == 0, the heaviest on a strict > (the front-most row wins equal bits), the median
//    while it is unset and T after the row < 0.5f.  An ignored row (id -2) still occludes and counts; it only cannot be
//    named.  Every pixel inside the image is stored to every non-NULL plane by plain vector stores, so the caller need
//    not pre-fill; with `empty` (L == 0 or P == 0) no workspace is read and the planes take the "nothing" values.
//  block_tile, exp2_le1, rank_below and the staging / quadrant-list loop stand here a third time (contrib.hip and
//  attribute.hip keep theirs, so that their kernels compile to what they did before this file existed); DESIGN.md
//  section 8 lists folding the three walks into one text.
//  Measured: profiles/f24_pixels_kernels.md.
#include "common.h"

#pragma clang fp contract(off)

namespace hgs {
namespace {

constexpr float kAlphaMin = 1.0f / 255.0f;
constexpr float kAlphaMax = 0.99f;
constexpr float kTEps = 0.0001f;
constexpr float kBig = 1.0e18f;   // y coordinate of a finished / outside pixel (K6's convention)
constexpr int kBatch = 64;        // instances staged per batch, one per lane
constexpr int kNoRow = -1;        // id where no row answers
constexpr int kIgnoredRow = -2;   // id of a row the slot map does not name

// exp2(min(x, 0)) through the [0, 1] output clamp of v_exp_f32: K6's expression
__device__ __forceinline__ float exp2_le1(float x) { return __builtin_amdgcn_fmed3f(__builtin_amdgcn_exp2f(x), 0.0f, 1.0f); }

// K6's block -> tile map (render.hip: block_to_tile)
__device__ __forceinline__ int block_tile(int T, const uint32_t* __restrict__ order) {
  const int per = (T + 7) >> 3;
  const int b = blockIdx.x;
  return order ? (int)order[b] : (b & 7) * per + (b >> 3);
}

// number of set bits of `m` below this lane
__device__ __forceinline__ uint32_t rank_below(uint64_t m) {
  return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}

__global__ __launch_bounds__(64) void pixels_tile_kernel(
    const uint32_t* __restrict__ ranges, const uint32_t* __restrict__ point_list, const float4* __restrict__ records,
    const float* __restrict__ depths, int W, int H, int gx, int T, const uint32_t* __restrict__ order,
    const int32_t* __restrict__ slot_of_row, long long n_slots, hgs_raster_pixel_planes out, int empty) {
  // float4 per staged instance: (gxt, gyt, A2, B2) (C2, opacity, id bits, depth bits); instance kBatch is a dummy of
  // opacity 0 that the rows whose list has run out fetch
  __shared__ float4 lrec[(kBatch + 1) * 2];
  // entry `it`: the it-th instance of each quadrant's list (kBatch: none)
  __shared__ uint16_t qlist[(kBatch + 1) * 4];

  const int tile = block_tile(T, order);
  if ((uint32_t)tile >= (uint32_t)T) return;
  const int ty = tile / gx, tx = tile - ty * gx;
  const int lane = threadIdx.x;
  // K7's lane -> pixel map: the DPP row (16 lanes) is the 8x8 quadrant q (bit 0: right, bit 1: lower half); lane l of
  // the row owns the column x = l & 7, pixels at rows ((l >> 3) & 1) + 2 s of the quadrant
  const int q = lane >> 4;
  const int lx = (lane & 7) + ((q & 1) << 3), ly0 = ((lane >> 3) & 1) + ((q >> 1) << 3);
  const int px = tx * kTile + lx;
  const float flx = (float)lx;
  const float tile_x0 = (float)(tx * kTile), tile_y0 = (float)(ty * kTile);

  float fly[4], Tp[4], best[4], mdepth[4];
  int cnt[4], front[4], back[4], heavy[4], med[4];
  bool inside[4];
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    const int py = ty * kTile + ly0 + 2 * s;
    inside[s] = px < W && py < H;
    fly[s] = inside[s] ? (float)(ly0 + 2 * s) : kBig;
    Tp[s] = 1.0f;
    best[s] = 0.0f;
    mdepth[s] = 0.0f;
    cnt[s] = 0;
    front[s] = back[s] = heavy[s] = med[s] = kNoRow;
  }
  if (lane == 0) {
    lrec[kBatch * 2 + 0] = make_float4(0.f, 0.f, 0.f, 0.f);
    lrec[kBatch * 2 + 1] = make_float4(0.f, 0.f, 0.f, 0.f);
  }

  uint32_t r0 = 0, r1 = 0;
  if (!empty) { r0 = ranges[tile * 2 + 0]; r1 = ranges[tile * 2 + 1]; }
  uint64_t alive = __ballot(fminf(fminf(fly[0], fly[1]), fminf(fly[2], fly[3])) < kBig);
  for (uint32_t base = r0; base < r1 && alive != 0; base += kBatch) {
    const int n = __builtin_amdgcn_readfirstlane((int)min((uint32_t)kBatch, r1 - base));
    __syncthreads();
    bool hit[4] = {false, false, false, false};
    if (lane < n) {
      const uint32_t gid = point_list[base + lane];
      const float4* r = records + (size_t)gid * kRecVec;
      float4 a0 = r[0];
      float4 a1 = r[1];
      const float4 a2 = r[2], a3 = r[3];
      a0.x = (a0.x - tile_x0) + a3.x;       // tile-relative pixel centre (K6's expression)
      a0.y = (a0.y - tile_y0) + a3.y;
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
      // K1's alpha >= 1/255 box (the one K6's cell lists are cut from) against the quadrants' pixel ranges; a quadrant
      // all of whose pixels have stopped takes no more instances
      const float ex = a2.z, ey = a3.w;
      const bool xl = (a0.x - ex <= 7.0f) && (a0.x + ex >= 0.0f), xr = (a0.x - ex <= 15.0f) && (a0.x + ex >= 8.0f);
      const bool yt = (a0.y - ey <= 7.0f) && (a0.y + ey >= 0.0f), yb = (a0.y - ey <= 15.0f) && (a0.y + ey >= 8.0f);
      hit[0] = xl && yt && (alive & 0xffffull) != 0;
      hit[1] = xr && yt && (alive & 0xffff0000ull) != 0;
      hit[2] = xl && yb && (alive & 0xffff00000000ull) != 0;
      hit[3] = xr && yb && (alive & 0xffff000000000000ull) != 0;
    }
    // the quadrants' lists, front to back: entry = rank of the instance inside its quadrant's mask.  (DS operations of
    // one wave execute in order: the fill is complete before the entries' stores.)
    for (int i = lane; i < (kBatch + 1) * 4; i += 64) qlist[i] = (uint16_t)kBatch;
    int nmax = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const uint64_t m = __ballot(hit[k]);
      if (hit[k]) qlist[rank_below(m) * 4 + k] = (uint16_t)lane;
      nmax = max(nmax, __builtin_popcountll(m));
    }
    __syncthreads();
    // one (instance, quadrant) pair per row of the wave and iteration
    for (int it = 0; it < nmax; ++it) {
      const uint32_t j = qlist[it * 4 + q];
      const float4 q0 = lrec[j * 2 + 0], q1 = lrec[j * 2 + 1];
      const int id = __float_as_int(q1.z);
      const float dx = q0.x - flx;
      const float ax = q0.z * dx * dx;
      const float bx = q0.w * dx;
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        const float dy = q0.y - fly[s];
        const float pw = fmaf(dy, fmaf(q1.x, dy, bx), ax);
        const float alpha = fminf(kAlphaMax, q1.y * exp2_le1(pw));
        const bool live = alpha >= kAlphaMin;
        const float Tn = Tp[s] * (1.0f - alpha);
        const bool go = !(Tn < kTEps);
        const bool blend = live && go;
        const float w = alpha * Tp[s];
        front[s] = (blend && cnt[s] == 0) ? id : front[s];
        back[s] = blend ? id : back[s];
        cnt[s] += blend ? 1 : 0;
        const bool heavier = blend && w > best[s];      // strict: the front-most row keeps equal bits
        heavy[s] = heavier ? id : heavy[s];
        best[s] = heavier ? w : best[s];
        const bool half = blend && med[s] == kNoRow && Tn < 0.5f;
        med[s] = half ? id : med[s];
        mdepth[s] = half ? q1.w : mdepth[s];
        Tp[s] = blend ? Tn : Tp[s];
        fly[s] = (live && !go) ? kBig : fly[s];     // a saturated pixel leaves the tile
      }
    }
    alive = __ballot(fminf(fminf(fly[0], fly[1]), fminf(fly[2], fly[3])) < kBig);
  }
  // a median row the map ignores is named -2 and keeps its depth; where there is no median the depth is 0
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    if (!inside[s]) continue;
    const size_t p = (size_t)(ty * kTile + ly0 + 2 * s) * (size_t)W + (size_t)px;
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
