// The forward-side tile walk, ONCE, for the four files that read a finished forward without running the backward:
// contrib.hip (f-22), attribute.hip (f-23), pixels.hip (f-24) and values.hip (f-26).  Device only; included by those
// four files and by nothing else (render.hip keeps its own K6 and K7).  The walk is a contract: a row counts at a pixel exactly when K6
// blended it there, with the weight K6 added to the colour -- so K6's decision stands here in one text, not three.
//
//  * ONE WAVE PER 16x16 TILE in K6's XCD-aware tile order (block_tile), so no barrier beyond those of a one-wave
//    workgroup.  The wave re-walks the tile's depth-sorted list front to back in batches of 64 records staged through LDS
//    and repeats K6's per-pixel decisions on the same 64-byte records with the same float32 expressions (exp2_le1, the
//    0.99 cap, alpha >= 1/255, T (1 - alpha) < 1e-4 stops the pixel; K6's expressions have no product feeding a sum).
//  * QUADRANT STREAMS, as in K7: the four DPP rows of the wave own the four 8x8 quadrants of the tile and each walks ITS
//    OWN list -- the staging lane tests K1's alpha >= 1/255 box (the one K6's cell lists are cut from: outside it K6
//    visits nothing) against the quadrants, four ballots file the instance into the lists by rank -- so one iteration
//    serves up to four (instance, quadrant) pairs and a batch costs max(list lengths) iterations instead of 64 passes
//    over the tile (the wave-uniform walk measured 429 us on the metric frame, this one 227).  A quadrant all of whose
//    pixels have stopped takes no more instances; the walk ends when no pixel is alive.
//  * DS operations of one wave execute in order: the fill of the lists is complete before the entries' stores, and the
//    two barriers of a batch only separate the staging lanes' stores from the rows' loads.
//
// The walk is handed out as FORCE-INLINED PIECES, not as one loop template: the lane map (TileLane), a pixel's start
// (inside, fly0), the staging of one record with the quadrant box test (stage), the filing into the lists (file), the
// liveness ballot (alive_lanes) and the blend step for one pixel (blend_pixel).  A kernel keeps its own skeleton -- its
// LDS arrays, the batch loop, the barriers, the loop over a batch's pairs -- and its per-pixel state as plain local
// arrays, and says between the pieces what only it does: what the staging lane adds, what a visit keeps, what follows a
// batch and the loop.  The one-function form (a loop template over a policy struct) was tried and compiles to other
// kernels: a member array is split into scalars where a local float[4] becomes one vector value, and hooks that write
// through references are simplified before they are inlined (contrib_tile_kernel: 49 registers for 46; the readout
// kernel 71 for 82, another occupancy class).  With these pieces -- the per-pixel ones take and return VALUES -- every
// kernel keeps its register row (profiles/f25_tile_walk.md).
//
// Rounding is written down here, not left to the includer: contraction is off from this line on, and the one fused
// operation of the blend step is an explicit fmaf (the rule ssim_tile.h set).
//
// Below the walk: the per-instance records of f-22 and f-23 (the DPP row butterfly, the emission slot, the mask test, the
// zero-record tail) and ONE text of the run sum that adds a row's records up.
#pragma once
#include "common.h"

#pragma clang fp contract(off)

namespace hgs {

constexpr float kAlphaMin = 1.0f / 255.0f;
constexpr float kAlphaMax = 0.99f;
constexpr float kTEps = 0.0001f;
constexpr float kBig = 1.0e18f;   // y coordinate of a finished / outside pixel (K6's convention)
constexpr int kBatch = 64;        // instances staged per batch, one per lane
constexpr int kSumBlock = 256;
constexpr uint32_t kLongRun = 64; // records of a run that one thread still adds up alone

// exp2(min(x, 0)) through the [0, 1] output clamp of v_exp_f32: K6's expression
__device__ __forceinline__ float exp2_le1(float x) { return __builtin_amdgcn_fmed3f(__builtin_amdgcn_exp2f(x), 0.0f, 1.0f); }

// K6's block -> tile map (render.hip: block_to_tile)
__device__ __forceinline__ int block_tile(int T, const uint32_t* __restrict__ order) {
  const int per = (T + 7) >> 3;
  const int b = blockIdx.x;
  return order ? (int)order[b] : (b & 7) * per + (b >> 3);
}

template <int CTRL>
__device__ __forceinline__ float dpp(float v) {
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xf, 0xf, true));
}
constexpr int kQuadSwap1 = 0xB1, kQuadSwap2 = 0x4E, kRowHalfMirror = 0x141, kRowMirror = 0x140;

// totals over a DPP row (16 lanes) by a butterfly; every lane of the row ends with the same bits
__device__ __forceinline__ float row_sum(float v) {
  v += dpp<kQuadSwap1>(v);
  v += dpp<kQuadSwap2>(v);
  v += dpp<kRowHalfMirror>(v);
  v += dpp<kRowMirror>(v);
  return v;
}
__device__ __forceinline__ float row_max(float v) {
  v = fmaxf(v, dpp<kQuadSwap1>(v));
  v = fmaxf(v, dpp<kQuadSwap2>(v));
  v = fmaxf(v, dpp<kRowHalfMirror>(v));
  v = fmaxf(v, dpp<kRowMirror>(v));
  return v;
}
// number of set bits of `m` below this lane
__device__ __forceinline__ uint32_t rank_below(uint64_t m) {
  return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}

// slot of the (tile, Gaussian) instance in emission order (found through `offsets` and the record's tile rectangle, as
// K7 finds it)
__device__ __forceinline__ uint32_t emission_slot(uint32_t off, uint32_t rectbits, int tx, int ty) {
  const uint32_t minx = rectbits & 1023u, miny = (rectbits >> 10) & 1023u, rw = rectbits >> 20;
  return off + ((uint32_t)ty - miny) * rw + ((uint32_t)tx - minx);
}

// One lane's share of a tile: K7's lane -> pixel map.  The DPP row (16 lanes) is the 8x8 quadrant q (bit 0: right, bit
// 1: lower half); lane l of the row owns the column x = l & 7, pixels at rows ((l >> 3) & 1) + 2 s of the quadrant.
struct TileLane {
  int tx, ty, lane, q, lx, ly0, px;
  float flx, tile_x0, tile_y0;

  __device__ __forceinline__ TileLane(int tile, int gx) {
    ty = tile / gx;
    tx = tile - ty * gx;
    lane = threadIdx.x;
    q = lane >> 4;
    lx = (lane & 7) + ((q & 1) << 3);
    ly0 = ((lane >> 3) & 1) + ((q >> 1) << 3);
    px = tx * kTile + lx;
    flx = (float)lx;
    tile_x0 = (float)(tx * kTile);
    tile_y0 = (float)(ty * kTile);
  }
  __device__ __forceinline__ int py(int s) const { return ty * kTile + ly0 + 2 * s; }

  // pixel s before the first row: whether it is inside the image, and its row coordinate `fly` (kBig: finished or
  // outside); its transmittance starts at 1
  __device__ __forceinline__ bool inside(int s, int W, int H) const { return px < W && py(s) < H; }
  __device__ __forceinline__ float fly0(int s, bool in) const { return in ? (float)(ly0 + 2 * s) : kBig; }

  // the dummy record at index kBatch
  __device__ __forceinline__ void open(float4* lrec) const {
    if (lane == 0) {
      lrec[kBatch * 2 + 0] = make_float4(0.f, 0.f, 0.f, 0.f);
      lrec[kBatch * 2 + 1] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
  }

  // STAGING, by lane `lane` of a batch for list entry i: the instance's record with K6's tile-relative centre, and its
  // hits -- K1's alpha >= 1/255 box (the one K6's cell lists are cut from) against the quadrants' pixel ranges; a
  // quadrant all of whose pixels have stopped takes no more instances.  The caller stores a0 and a1 (whose last two
  // words are its own) to lrec[lane * 2].  Returns the instance's row.
  __device__ __forceinline__ uint32_t stage(const uint32_t* __restrict__ point_list, const float4* __restrict__ records,
                                            uint32_t i, uint64_t alive, float4& a0, float4& a1, float4& a2,
                                            bool (&hit)[4]) const {
    const uint32_t gid = point_list[i];
    const float4* r = records + (size_t)gid * kRecVec;
    a0 = r[0];
    a1 = r[1];
    a2 = r[2];
    const float4 a3 = r[3];
    a0.x = (a0.x - tile_x0) + a3.x;       // tile-relative pixel centre (K6's expression)
    a0.y = (a0.y - tile_y0) + a3.y;
    const float ex = a2.z, ey = a3.w;
    const bool xl = (a0.x - ex <= 7.0f) && (a0.x + ex >= 0.0f), xr = (a0.x - ex <= 15.0f) && (a0.x + ex >= 8.0f);
    const bool yt = (a0.y - ey <= 7.0f) && (a0.y + ey >= 0.0f), yb = (a0.y - ey <= 15.0f) && (a0.y + ey >= 8.0f);
    hit[0] = xl && yt && (alive & 0xffffull) != 0;
    hit[1] = xr && yt && (alive & 0xffff0000ull) != 0;
    hit[2] = xl && yb && (alive & 0xffff00000000ull) != 0;
    hit[3] = xr && yb && (alive & 0xffff000000000000ull) != 0;
    return gid;
  }

  // FILING: the quadrants' lists, front to back: entry = rank of the instance inside its quadrant's mask.  (DS
  // operations of one wave execute in order: the fill is complete before the entries' stores.)  Returns the length of
  // the longest list: the iterations of the batch, one (instance, quadrant) pair per row of the wave and iteration.
  __device__ __forceinline__ int file(uint16_t* qlist, const bool (&hit)[4]) const {
    for (int i = lane; i < (kBatch + 1) * 4; i += 64) qlist[i] = (uint16_t)kBatch;
    int nmax = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const uint64_t m = __ballot(hit[k]);
      if (hit[k]) qlist[rank_below(m) * 4 + k] = (uint16_t)lane;
      nmax = max(nmax, __builtin_popcountll(m));
    }
    return nmax;
  }
};

// lanes with a pixel that can still take a row
__device__ __forceinline__ uint64_t alive_lanes(const float (&fly)[4]) {
  return __ballot(fminf(fminf(fly[0], fly[1]), fminf(fly[2], fly[3])) < kBig);
}

// THE BLEND STEP for one pixel (row coordinate fly, transmittance Tp so far) and one staged instance (q0, q1; ax = A2
// dx^2 and bx = B2 dx are the pair's): K6's decision.  `blend`: the row is blended here, with weight w = alpha * T_before
// and Tn the transmittance after it; T_after and fly_after are the pixel's state behind the row.
struct Blend {
  bool blend, live, go;
  float w, Tn;
  __device__ __forceinline__ float T_after(float Tp) const { return blend ? Tn : Tp; }
  __device__ __forceinline__ float fly_after(float fly) const { return (live && !go) ? kBig : fly; }   // a saturated pixel leaves the tile
};
__device__ __forceinline__ Blend blend_pixel(const float4& q0, const float4& q1, float ax, float bx, float fly,
                                             float Tp) {
  Blend b;
  const float dy = q0.y - fly;
  const float pw = fmaf(dy, fmaf(q1.x, dy, bx), ax);
  const float alpha = fminf(kAlphaMax, q1.y * exp2_le1(pw));
  b.live = alpha >= kAlphaMin;
  b.Tn = Tp * (1.0f - alpha);
  b.go = !(b.Tn < kTEps);
  b.blend = b.live && b.go;
  b.w = alpha * Tp;
  return b;
}

// ---- per-instance records (f-22, f-23) ------------------------------------------------------------------------------
// One 16-byte record per (tile, Gaussian) instance in the scratch, at the instance's EMISSION slot.  A pair's 64 pixel
// slots are reduced in ONE FIXED ORDER (the lane's four pixels, a DPP butterfly inside the row) and stored by the row's
// leader to the pair's own LDS slot in `acc` ([(kBatch + 1) * 4] float4, written by the pair's one visit; row kBatch is
// the sink of the rows that have run out).  At the end of the batch lane j adds up instance j's pairs in quadrant order
// and stores the record (in each file: the sums are its own, and the fold behind a shared template costs
// contrib_tile_kernel two registers): the result does not depend on what else is in the list.  Instances the tile never
// reaches (every pixel stopped) store zeros: the scratch needs no zero fill.

// a pixel is counted when it is inside the image and the caller's mask, if there is one, is non-zero there
__device__ __forceinline__ void count_pixel(const TileLane& t, int s, bool inside, int W,
                                            const uint8_t* __restrict__ pixel_mask, bool (&counted)[4]) {
  counted[s] = inside;
  if (inside && pixel_mask) counted[s] = pixel_mask[(size_t)t.py(s) * W + t.px] != 0;
}

// instances behind the stop of every pixel: zero records
__device__ __forceinline__ void zero_tail(const TileLane& t, uint32_t base, uint32_t r1,
                                          const uint32_t* __restrict__ point_list, const float4* __restrict__ records,
                                          const uint32_t* __restrict__ offsets, float4* __restrict__ inst, uint32_t L) {
  for (uint32_t i = base + (uint32_t)t.lane; i < r1; i += 64) {
    const uint32_t gid = point_list[i];
    const uint32_t rb = __float_as_uint(reinterpret_cast<const float*>(records + (size_t)gid * kRecVec + 2)[3]);
    const uint32_t e = emission_slot(offsets[gid], rb, t.tx, t.ty);
    if (e < L) inst[e] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  }
}

// ---- the run sum (f-22, f-23) ---------------------------------------------------------------------------------------
// One thread per row adds up the row's contiguous run of records in run order -- runs of more than kLongRun records by
// the whole wave -- into an accumulator Acc{}: Acc::add(record), Acc::add_lane(d) (the accumulator of lane ^ d joins this
// one) and Acc::nowhere() (the row is blended at no counted pixel).  False: the row writes nothing; else `s` is its
// slot, for the caller's plain read-modify-write (distinct slots are the caller's precondition, so no two threads touch
// the same entry).
template <class Acc>
__device__ __forceinline__ bool run_sum(int P, const uint32_t* __restrict__ tiles_touched,
                                        const uint32_t* __restrict__ offsets, const float4* __restrict__ inst, uint32_t L,
                                        const int32_t* __restrict__ slot_of_row, long long n_slots, long long& s, Acc& a) {
  const int i = blockIdx.x * kSumBlock + threadIdx.x;
  const int lane = threadIdx.x & 63;
  s = -1;
  uint32_t n = 0, off = 0;
  if (i < P) {
    n = tiles_touched[i];
    s = slot_of_row ? (long long)slot_of_row[i] : (long long)i;
    if (n) off = offsets[i];
  }
  // an ignored row (negative slot); a slot beyond the arrays is never written through; a run outside the scratch is not read
  const bool use = n != 0 && s >= 0 && s < n_slots && off <= L && n <= L - off;
  if (use && n <= kLongRun) {                       // a short run: this thread, in run order
    for (uint32_t k = 0; k < n; ++k) a.add(inst[(size_t)off + k]);
  }
  // Long runs (a Gaussian of a trained scene covers thousands of tiles): the wave takes them one after the other, lane l
  // adds records l, l + 64, ... in that order and a butterfly adds the 64 partial sums -- an order that depends on the
  // run's length alone, so the bits do not depend on which rows share the wave.  (Both operands of every butterfly step
  // are the same two values in either lane: all lanes end with the same bits.)
  for (uint64_t longs = __ballot(use && n > kLongRun); longs != 0; longs &= longs - 1) {
    const int src = __builtin_ctzll(longs);
    const uint32_t o = (uint32_t)__shfl((int)off, src, 64), nn = (uint32_t)__shfl((int)n, src, 64);
    Acc p{};
    for (uint32_t k = (uint32_t)lane; k < nn; k += 64) p.add(inst[(size_t)o + k]);
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) p.add_lane(d);
    if (lane == src) a = p;
  }
  return use && !a.nowhere();                       // blended nowhere: the slot keeps its bits
}

}  // namespace hgs
