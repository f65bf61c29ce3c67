// Attribution of a per-pixel image to the Gaussians that blend it: for every row i of one
// forward and every channel c < C of a planar float32 image f [C, H, W],
//     A[i, c] = sum over the counted pixels p at which K6 blends row i of  w_i(p) * f_c(p),     w = alpha * T_before,
// and the sum of the weights themselves.  This is dL / d colors_precomp of a backward seeded with f -- the whole of K7 and
// K8 for C numbers per row, refused on the in-op LOD route and without a slot map -- computed on the forward's side.
//
// Two kernels in the shape of contrib.hip (f-22), whose walk this file repeats; no atomics anywhere, bit-reproducible:
//  * attribute_tile_kernel<C>: ONE WAVE PER 16x16 TILE in K6's XCD-aware tile order.  Each lane loads f_c of its four
//    pixels once (4 C registers; a pixel that is outside the image or masked out is never read).  The wave re-walks the
//    tile's depth-sorted list in batches of 64 records staged through LDS, four QUADRANT STREAMS as in K7 and f-22, and
//    repeats K6's per-pixel decisions on the same 64-byte records with the same float32 expressions (exp2_le1, the 0.99
//    cap, alpha >= 1/255, T (1 - alpha) < 1e-4 stops the pixel; contraction is off for the file).  Per (instance,
//    quadrant) pair and pixel it forms t_c = w * f_c, ONE rounded product, and w; a pixel that is not counted, or at
//    which the row is not blended, contributes a SELECTED 0.0f, never 0 * f: a NaN or an infinity there reaches no
//    output.  The pair's 64 pixel slots are reduced in f-22's one fixed order -- (t0 + t1) + (t2 + t3), then the DPP
//    butterfly over the row -- into the pair's own LDS slot; at the end of the batch lane j adds instance j's pairs in
//    quadrant order and stores one 16-byte record (A0, A1, A2, wsum; unused channels zero) to the instance's EMISSION
//    slot.  Instances the tile never reaches store zeros: the scratch needs no zero fill.  The fourth component goes
//    through exactly the operations of f-22's `wsum`, so the two are equal bit for bit, and so is a channel of ones
//    (w * 1.0f is w).
//  * attribute_sum_kernel<C>: one thread per row adds the row's contiguous run of records in run order with float64
//    accumulators -- runs of more than 64 records by the whole wave in f-22's length-only order -- and does a plain
//    read-modify-write into out[slot * C + c] and, when given, wsum[slot].  A row whose summed wsum is zero (blended at
//    no counted pixel: a weight is at least 1e-4 / 255) writes nothing.  Distinct slots are the caller's precondition.
//  The DPP sums, emission_slot and block_tile stand here a second time (contrib.hip keeps its own, so that its kernels
//  compile to what they did before this file existed); DESIGN.md section 8 lists folding the two walks into one text.
//  Measured: profiles/f23_attribute_kernels.md.
#include "common.h"

#pragma clang fp contract(off)

namespace hgs {
namespace {

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
// number of set bits of `m` below this lane
__device__ __forceinline__ uint32_t rank_below(uint64_t m) {
  return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}

// record of one (tile, Gaussian) instance in the scratch: (A0, A1, A2, sum of weights)
__device__ __forceinline__ uint32_t emission_slot(uint32_t off, uint32_t rectbits, int tx, int ty) {
  const uint32_t minx = rectbits & 1023u, miny = (rectbits >> 10) & 1023u, rw = rectbits >> 20;
  return off + ((uint32_t)ty - miny) * rw + ((uint32_t)tx - minx);
}

template <int C>
__global__ __launch_bounds__(64) void attribute_tile_kernel(
    const uint32_t* __restrict__ ranges, const uint32_t* __restrict__ point_list, const float4* __restrict__ records,
    int W, int H, int gx, int T, const uint32_t* __restrict__ order, const uint32_t* __restrict__ offsets,
    const float* __restrict__ image, const uint8_t* __restrict__ pixel_mask, float4* __restrict__ inst, uint32_t L) {
  // float4 per staged instance: (gxt, gyt, A2, B2) (C2, opacity, -, -); instance kBatch is a dummy of opacity 0 that
  // the rows whose list has run out fetch
  __shared__ float4 lrec[(kBatch + 1) * 2];
  // entry `it`: the it-th instance of each quadrant's list (kBatch: none)
  __shared__ uint16_t qlist[(kBatch + 1) * 4];
  // (A0, A1, A2, sum of weights) of every (instance, quadrant) pair, written by the pair's one visit; row kBatch is the
  // sink of the rows that have run out
  __shared__ float4 acc[(kBatch + 1) * 4];

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
  const size_t plane = (size_t)W * (size_t)H;

  float fly[4], Tp[4], f[C][4];
  bool counted[4];
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    const int py = ty * kTile + ly0 + 2 * s;
    const bool inside = px < W && py < H;
    fly[s] = inside ? (float)(ly0 + 2 * s) : kBig;
    Tp[s] = 1.0f;
    counted[s] = inside;
    if (inside && pixel_mask) counted[s] = pixel_mask[(size_t)py * W + px] != 0;
    // the image is read at counted pixels only
#pragma unroll
    for (int c = 0; c < C; ++c) f[c][s] = counted[s] ? image[(size_t)c * plane + (size_t)py * W + px] : 0.0f;
  }
  if (lane == 0) {
    lrec[kBatch * 2 + 0] = make_float4(0.f, 0.f, 0.f, 0.f);
    lrec[kBatch * 2 + 1] = make_float4(0.f, 0.f, 0.f, 0.f);
  }
  const bool leader = (lane & 15) == 0;

  const uint32_t r0 = ranges[tile * 2 + 0], r1 = ranges[tile * 2 + 1];
  uint64_t alive = __ballot(fminf(fminf(fly[0], fly[1]), fminf(fly[2], fly[3])) < kBig);
  uint32_t base = r0;
  for (; base < r1 && alive != 0; base += kBatch) {
    const int n = __builtin_amdgcn_readfirstlane((int)min((uint32_t)kBatch, r1 - base));
    __syncthreads();
    uint32_t my_e = 0xffffffffu;
    bool hit[4] = {false, false, false, false};
    if (lane < n) {
      const uint32_t gid = point_list[base + lane];
      const float4* r = records + (size_t)gid * kRecVec;
      float4 a0 = r[0];
      const float4 a1 = r[1], a2 = r[2], a3 = r[3];
      a0.x = (a0.x - tile_x0) + a3.x;       // tile-relative pixel centre (K6's expression)
      a0.y = (a0.y - tile_y0) + a3.y;
      lrec[lane * 2 + 0] = a0;
      lrec[lane * 2 + 1] = a1;
      my_e = emission_slot(offsets[gid], __float_as_uint(a2.w), tx, ty);
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
      const float dx = q0.x - flx;
      const float ax = q0.z * dx * dx;
      const float bx = q0.w * dx;
      float w[4], t[C][4];
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        const float dy = q0.y - fly[s];
        const float pw = fmaf(dy, fmaf(q1.x, dy, bx), ax);
        const float alpha = fminf(kAlphaMax, q1.y * exp2_le1(pw));
        const bool live = alpha >= kAlphaMin;
        const float Tn = Tp[s] * (1.0f - alpha);
        const bool go = !(Tn < kTEps);
        const bool blend = live && go;
        const bool use = blend && counted[s];
        const float ws = alpha * Tp[s];
        w[s] = use ? ws : 0.0f;
        // one rounded product per channel; elsewhere a selected zero, never 0 * f
#pragma unroll
        for (int c = 0; c < C; ++c) t[c][s] = use ? ws * f[c][s] : 0.0f;
        Tp[s] = blend ? Tn : Tp[s];
        fly[s] = (live && !go) ? kBig : fly[s];     // a saturated pixel leaves the tile
      }
      // the pair's 64 pixel slots in a fixed order: the lane's four, then a butterfly over the row
      float4 sums = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
      sums.x = row_sum((t[0][0] + t[0][1]) + (t[0][2] + t[0][3]));
      if constexpr (C > 1) sums.y = row_sum((t[1][0] + t[1][1]) + (t[1][2] + t[1][3]));
      if constexpr (C > 2) sums.z = row_sum((t[2][0] + t[2][1]) + (t[2][2] + t[2][3]));
      sums.w = row_sum((w[0] + w[1]) + (w[2] + w[3]));
      if (leader) acc[j * 4 + q] = sums;
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
    alive = __ballot(fminf(fminf(fly[0], fly[1]), fminf(fly[2], fly[3])) < kBig);
  }
  // instances behind the stop of every pixel: zero records
  for (uint32_t i = base + (uint32_t)lane; i < r1; i += 64) {
    const uint32_t gid = point_list[i];
    const uint32_t rb = __float_as_uint(reinterpret_cast<const float*>(records + (size_t)gid * kRecVec + 2)[3]);
    const uint32_t e = emission_slot(offsets[gid], rb, tx, ty);
    if (e < L) inst[e] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  }
}

template <int C>
__global__ __launch_bounds__(kSumBlock) void attribute_sum_kernel(
    int P, const uint32_t* __restrict__ tiles_touched, const uint32_t* __restrict__ offsets,
    const float4* __restrict__ inst, uint32_t L, const int32_t* __restrict__ slot_of_row, long long n_slots,
    double* __restrict__ out, double* __restrict__ wsum) {
  const int i = blockIdx.x * kSumBlock + threadIdx.x;
  const int lane = threadIdx.x & 63;
  long long s = -1;
  uint32_t n = 0, off = 0;
  if (i < P) {
    n = tiles_touched[i];
    s = slot_of_row ? (long long)slot_of_row[i] : (long long)i;
    if (n) off = offsets[i];
  }
  // an ignored row (negative slot); a slot beyond the arrays is never written through; a run outside the scratch is not read
  const bool use = n != 0 && s >= 0 && s < n_slots && off <= L && n <= L - off;
  double a0 = 0.0, a1 = 0.0, a2 = 0.0, sw = 0.0;
  if (use && n <= kLongRun) {                       // a short run: this thread, in run order
    for (uint32_t k = 0; k < n; ++k) {
      const float4 r = inst[(size_t)off + k];
      a0 += (double)r.x;
      if (C > 1) a1 += (double)r.y;
      if (C > 2) a2 += (double)r.z;
      sw += (double)r.w;
    }
  }
  // Long runs: the wave takes them one after the other, lane l adds records l, l + 64, ... in that order and a butterfly
  // adds the 64 partial sums -- f-22's order, which depends on the run's length alone, so the bits do not depend on which
  // rows share the wave.  (Both operands of every butterfly step are the same two values in either lane.)
  for (uint64_t longs = __ballot(use && n > kLongRun); longs != 0; longs &= longs - 1) {
    const int src = __builtin_ctzll(longs);
    const uint32_t o = (uint32_t)__shfl((int)off, src, 64), nn = (uint32_t)__shfl((int)n, src, 64);
    double p0 = 0.0, p1 = 0.0, p2 = 0.0, pw = 0.0;
    for (uint32_t k = (uint32_t)lane; k < nn; k += 64) {
      const float4 r = inst[(size_t)o + k];
      p0 += (double)r.x;
      if (C > 1) p1 += (double)r.y;
      if (C > 2) p2 += (double)r.z;
      pw += (double)r.w;
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
      p0 += __shfl_xor(p0, d, 64);
      if (C > 1) p1 += __shfl_xor(p1, d, 64);
      if (C > 2) p2 += __shfl_xor(p2, d, 64);
      pw += __shfl_xor(pw, d, 64);
    }
    if (lane == src) { a0 = p0; a1 = p1; a2 = p2; sw = pw; }
  }
  if (!use || sw == 0.0) return;                    // blended nowhere: the slots keep their bits
  double* o = out + (size_t)s * C;
  o[0] += a0;
  if (C > 1) o[1] += a1;
  if (C > 2) o[2] += a2;
  if (wsum) wsum[s] += sw;
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

AttributeWs AttributeWs::layout(Carver& c, uint32_t L) { return {c.take<float>((size_t)(L ? L : 1) * 4)}; }

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
