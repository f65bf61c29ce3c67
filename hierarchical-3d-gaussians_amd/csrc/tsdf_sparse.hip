// A SPARSE TSDF volume: 8 x 8 x 8 blocks allocated near the observed surface over a virtual lattice, the fusion and the
// surface-net rules of tsdf_rule.h on them, the allocation rule of tsdf_block_rule.h (tests/tsdf_sparse_spec.py, the
// spec); hgs/meshing.py is the Python side.  On every lattice that a dense volume can hold,
// the allocated samples and the mesh carry the bits of csrc/tsdf.hip's.
//
//   table      dense over the block grid (ceil(n / 8) per axis, x fastest, at most 2^31 - 1 blocks): slots int32 [G]
//              (-1: none), marks uint8 [G], and a refusal word; ONE allocation laid out by carve_table.  Linear SAMPLE
//              indices of the virtual lattice exist nowhere: a sample is (block, place in the block), its lattice
//              coordinates 8 b + l per axis are 32-bit, its storage index 512 slot + place is 64-bit.
//   mark       tsdf_sparse_mark_kernel: one thread per pixel of up to 8 views (blockIdx.y = the view) marches the pixel's
//              band (tsdf_block_rule.h) and stores 1 at the mark of every block a marched point falls into: plain
//              idempotent stores of one value, no atomics; marks accumulate over calls.
//   commit     plan: tsdf_sparse_dilate_kernel, one thread per block of the GRID (never per sample of the lattice): slot =
//              0 where a block of the 3 x 3 x 3 neighbourhood is marked, else -1, and the workgroup's count;
//              tsdf_sparse_scan_kernel: common.h's chained scan; ONE host wait reads B and the refusal word.
//              apply: tsdf_sparse_assign_kernel: slot = the workgroup's offset + the block's rank -- ascending linear block
//              index --, block_of_slot[slot] = the block.
//   integrate  tsdf_sparse_integrate_kernel: one workgroup of 128 threads per allocated block, a thread owns 4 consecutive
//              x samples (16-byte loads and stores: a block's rows are 32 bytes and the arrays 16-byte aligned).  The
//              lattice indices are 8 block + place; every float is then tsdf.hip's, through the same tsdf_rule.h calls:
//              all views project first (a 32-bit mask), a thread nobody sees returns before any volume access, the views
//              are applied in array order on registers, an unchanged group is not stored.  Samples beyond the lattice
//              are skipped (they keep 1 / 0 / 0).  There is NO whole-block early reject: a block's bounding sphere
//              against a view's frustum would have to reproduce the float32 rounding of tsdf_project's pixel test to
//              provably never skip a sample the dense rule updates, and the projection mask already spares the unseen
//              block its memory traffic.
//   extract    plan: tsdf_sparse_class_kernel, one workgroup of 512 threads per allocated block: the block's 9 x 9 x 9
//              halo of tsdf and weight is staged in LDS (5832 bytes), the +1 faces from the neighbouring blocks through
//              the table; a sample that is beyond the lattice or in no allocated block is staged with weight -1, so no
//              cell or edge that needs it passes tsdf_observed.  A thread writes its sample's word -- class bits 0..2,
//              the rank of its cell among the block's active cells in bits 3..11 (9 bits) -- and the block's count.
//              tsdf_sparse_quads_kernel: per sample the quads of its three edges from the words of its neighbours (the
//              lower-side blocks too, through the table), the block's count.  The chained scan over both; ONE host wait.
//              apply: tsdf_sparse_emit_kernel: vertices by (slot, place of the cell), faces by (slot, place of the edge's
//              lower sample, axis), and cells [V,3], the lattice cell of every vertex.
// No kernel here uses atomics or scratch.
#include "lod_cut.h"    // the launcher of the chained scan, block_exclusive_offset (the cut rules in it are not used)
#include "tsdf_block_rule.h"

#include <mutex>
#include <vector>

#pragma clang fp contract(off)

namespace hgs {
namespace {

constexpr int kMaxViews = 8;
constexpr int64_t kMaxGridBlocks = 0x7fffffff;
// the quad offsets are 32-bit and a sample has at most three quads
constexpr int64_t kMaxExtractBlocks = 0xffffffffll / 3 / kTsdfBlockSamples;
constexpr uint32_t kCellActive = 1u, kObserved = 2u, kInside = 4u;
constexpr int kRankShift = 3;
constexpr int kStateWords = 64;        // state[0]: the refusal word of the marking

struct Views { hgs_tsdf_view v[kMaxViews]; };

struct Table {
  int32_t* slots;     // [G]
  uint8_t* marks;     // [G]
  uint32_t* state;    // [kStateWords]
};
Table carve_table(Carver& c, int64_t G) {
  Table t;
  t.slots = c.take<int32_t>((size_t)G);
  t.marks = c.take<uint8_t>((size_t)G);
  t.state = c.take<uint32_t>(kStateWords);
  return t;
}

// the block grid and the lattice, as the kernels take them
struct Grid {
  int32_t gb[3];
  int32_t n[3];
};
__host__ __device__ inline int64_t grid_index(const Grid& g, int32_t bi, int32_t bj, int32_t bk) {
  return ((int64_t)bk * g.gb[1] + bj) * g.gb[0] + bi;
}
__device__ __forceinline__ void block_of(const Grid& g, int64_t b, int32_t* bi, int32_t* bj, int32_t* bk) {
  const int64_t row = b / g.gb[0];
  *bi = (int32_t)(b - row * g.gb[0]);
  *bk = (int32_t)(row / g.gb[1]);
  *bj = (int32_t)(row - (int64_t)*bk * g.gb[1]);
}

// The storage index of the sample at place (li, lj, lk), each in -1 .. 15, relative to block (bi, bj, bk); -1 where the
// sample lies beyond the lattice or in no allocated block.
__device__ __forceinline__ int64_t storage_index(const Grid& g, const int32_t* __restrict__ slots, int32_t bi, int32_t bj,
                                                 int32_t bk, int li, int lj, int lk) {
  const int32_t ci = bi + (li >> 3), cj = bj + (lj >> 3), ck = bk + (lk >> 3);
  const int pi = li & 7, pj = lj & 7, pk = lk & 7;
  if (ci < 0 || cj < 0 || ck < 0 || ci >= g.gb[0] || cj >= g.gb[1] || ck >= g.gb[2]) return -1;
  // (8 c + p < n without the product: n may be 2^31 - 1)
  if (pi > g.n[0] - 1 - 8 * (int64_t)ci || pj > g.n[1] - 1 - 8 * (int64_t)cj || pk > g.n[2] - 1 - 8 * (int64_t)ck) return -1;
  const int32_t slot = slots[grid_index(g, ci, cj, ck)];
  if (slot < 0) return -1;
  return (int64_t)slot * kTsdfBlockSamples + (pk * 64 + pj * 8 + pi);
}

// ---- marking ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void tsdf_sparse_mark_kernel(Views views, Grid g, float lo0, float lo1, float lo2,
                                                               float voxel, float trunc, int32_t S,
                                                               uint8_t* __restrict__ marks, uint32_t* __restrict__ state) {
  const hgs_tsdf_view& a = views.v[blockIdx.y];
  const int64_t pix = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (pix >= (int64_t)a.W * a.H) return;
  const int32_t py = (int32_t)(pix / a.W), px = (int32_t)(pix - (int64_t)py * a.W);
  const float d = a.depth[pix];
  const float w = a.weight ? a.weight[pix] : 1.0f;
  const float lo[3] = {lo0, lo1, lo2};
  const bool marched = tsdf_block_march(px, py, d, w, a.view, a.tanfovx, a.tanfovy, a.W, a.H, a.z_min, lo, voxel, trunc, S,
                                        g.gb, [&](int32_t bi, int32_t bj, int32_t bk) {
                                          marks[grid_index(g, bi, bj, bk)] = (uint8_t)1;
                                        });
  if (!marched) state[0] = 1u;
}

// ---- commit ----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void tsdf_sparse_dilate_kernel(const uint8_t* __restrict__ marks, Grid g, int64_t G,
                                                                 int32_t* __restrict__ slots, uint32_t* __restrict__ sums,
                                                                 unsigned long long* __restrict__ chain) {
  clear_scan_chain(chain);
  const int64_t b = (int64_t)blockIdx.x * 256 + threadIdx.x;
  uint32_t any = 0;
  if (b < G) {
    int32_t bi, bj, bk;
    block_of(g, b, &bi, &bj, &bk);
    const int32_t i0 = max(bi - 1, 0), i1 = min(bi + 1, g.gb[0] - 1), j0 = max(bj - 1, 0), j1 = min(bj + 1, g.gb[1] - 1),
                  k0 = max(bk - 1, 0), k1 = min(bk + 1, g.gb[2] - 1);
    for (int32_t k = k0; k <= k1; ++k)
      for (int32_t j = j0; j <= j1; ++j)
        for (int32_t i = i0; i <= i1; ++i) any |= marks[grid_index(g, i, j, k)];
    any = any ? 1u : 0u;
    slots[b] = any ? 0 : -1;
  }
  const uint32_t off = block_exclusive_offset(any);
  if (threadIdx.x == 255) sums[blockIdx.x] = off + any;
}

__global__ __launch_bounds__(1024) void tsdf_sparse_scan_kernel(uint32_t* __restrict__ sums, int n,
                                                                unsigned long long* __restrict__ chain, int c_off,
                                                                int chunks) {
  (void)chained_scan_inplace(sums, n, chain, c_off, chunks);
}

__global__ __launch_bounds__(256) void tsdf_sparse_assign_kernel(int64_t G, int32_t B, int32_t* __restrict__ slots,
                                                                 const uint32_t* __restrict__ sums,
                                                                 int32_t* __restrict__ block_of_slot) {
  const int64_t b = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const uint32_t any = (b < G && slots[b] >= 0) ? 1u : 0u;
  const uint32_t off = block_exclusive_offset(any);
  if (!any) return;
  const uint32_t slot = sums[blockIdx.x] + off;
  if (slot >= (uint32_t)B) return;        // (never behind this table's plan: B is its total)
  slots[b] = (int32_t)slot;
  block_of_slot[slot] = (int32_t)b;
}

// ---- integrate -------------------------------------------------------------------------------------------------------
struct Arrays {
  float* tsdf;
  float* weight;
  float* colour;
  const int32_t* block_of_slot;
  float lo[3];
  float voxel, trunc, max_weight;
};

template <bool kColour>
__global__ __launch_bounds__(128) void tsdf_sparse_integrate_kernel(Arrays vol, Grid g, Views views, int n_views) {
  int32_t bi, bj, bk;
  block_of(g, (int64_t)vol.block_of_slot[blockIdx.x], &bi, &bj, &bk);
  const int li = (threadIdx.x & 1) * 4, lj = (threadIdx.x >> 1) & 7, lk = threadIdx.x >> 4;
  // the lattice indices: 64-bit until they are known to lie inside the lattice
  const int64_t i0w = 8 * (int64_t)bi + li, jw = 8 * (int64_t)bj + lj, kw = 8 * (int64_t)bk + lk;
  if (jw >= g.n[1] || kw >= g.n[2] || i0w >= g.n[0]) return;
  const int32_t i0 = (int32_t)i0w, j = (int32_t)jw, k = (int32_t)kw;
  const int count = (int)min((int64_t)4, (int64_t)g.n[0] - i0w);
  const float x1 = tsdf_lattice(vol.lo[1], vol.voxel, j), x2 = tsdf_lattice(vol.lo[2], vol.voxel, k);
  float x0[4];
#pragma unroll
  for (int s = 0; s < 4; ++s) x0[s] = tsdf_lattice(vol.lo[0], vol.voxel, s < count ? i0 + s : i0);
  // ---- which view sees which sample: before any volume access
  uint32_t mask = 0;
  for (int v = 0; v < n_views; ++v) {
    const hgs_tsdf_view& a = views.v[v];
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      float z;
      int32_t px, py;
      if (s < count && tsdf_project(x0[s], x1, x2, a.view, a.tanfovx, a.tanfovy, a.W, a.H, a.z_min, &z, &px, &py))
        mask |= 1u << (4 * v + s);
    }
  }
  if (mask == 0u) return;
  // ---- the samples, once: a group of 4 is 16 bytes at a 16-byte aligned address
  const int64_t base = (int64_t)blockIdx.x * kTsdfBlockSamples + (lk * 64 + lj * 8 + li);
  float* const tp = vol.tsdf + base;
  float* const wp = vol.weight + base;
  float* const cp = kColour ? vol.colour + base * 3 : nullptr;
  float T[4], Wt[4], Cl[4][3];
  {
    const float4 t4 = *reinterpret_cast<const float4*>(tp), w4 = *reinterpret_cast<const float4*>(wp);
    T[0] = t4.x; T[1] = t4.y; T[2] = t4.z; T[3] = t4.w;
    Wt[0] = w4.x; Wt[1] = w4.y; Wt[2] = w4.z; Wt[3] = w4.w;
    if constexpr (kColour) {
      const float4 c0 = reinterpret_cast<const float4*>(cp)[0], c1 = reinterpret_cast<const float4*>(cp)[1],
                   c2 = reinterpret_cast<const float4*>(cp)[2];
      Cl[0][0] = c0.x; Cl[0][1] = c0.y; Cl[0][2] = c0.z; Cl[1][0] = c0.w;
      Cl[1][1] = c1.x; Cl[1][2] = c1.y; Cl[2][0] = c1.z; Cl[2][1] = c1.w;
      Cl[2][2] = c2.x; Cl[3][0] = c2.y; Cl[3][1] = c2.z; Cl[3][2] = c2.w;
    }
  }
  // ---- the views in array order, on registers
  bool changed = false;
  for (int v = 0; v < n_views; ++v) {
    const hgs_tsdf_view& a = views.v[v];
    const size_t plane = (size_t)a.W * (size_t)a.H;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      if (!((mask >> (4 * v + s)) & 1u)) continue;
      float z;
      int32_t px, py;
      if (!tsdf_project(x0[s], x1, x2, a.view, a.tanfovx, a.tanfovy, a.W, a.H, a.z_min, &z, &px, &py)) continue;
      const size_t pix = (size_t)py * (size_t)a.W + (size_t)px;
      const float d = a.depth[pix];
      const float w = a.weight ? a.weight[pix] : 1.0f;
      if constexpr (kColour) {
        float rgb[3] = {0.0f, 0.0f, 0.0f};
        if (a.rgb) {
#pragma unroll
          for (int c = 0; c < 3; ++c) rgb[c] = a.rgb[(size_t)c * plane + pix];
        }
        changed |= tsdf_update(d, w, rgb, a.rgb != nullptr, z, vol.trunc, vol.max_weight, &T[s], &Wt[s], Cl[s]);
      } else {
        changed |= tsdf_update(d, w, nullptr, false, z, vol.trunc, vol.max_weight, &T[s], &Wt[s], nullptr);
      }
    }
  }
  if (!changed) return;
  *reinterpret_cast<float4*>(tp) = make_float4(T[0], T[1], T[2], T[3]);
  *reinterpret_cast<float4*>(wp) = make_float4(Wt[0], Wt[1], Wt[2], Wt[3]);
  if constexpr (kColour) {
    reinterpret_cast<float4*>(cp)[0] = make_float4(Cl[0][0], Cl[0][1], Cl[0][2], Cl[1][0]);
    reinterpret_cast<float4*>(cp)[1] = make_float4(Cl[1][1], Cl[1][2], Cl[2][0], Cl[2][1]);
    reinterpret_cast<float4*>(cp)[2] = make_float4(Cl[2][2], Cl[3][0], Cl[3][1], Cl[3][2]);
  }
}

// ---- extraction ------------------------------------------------------------------------------------------------------
// exclusive offset of this thread's count among the counts of its 512-thread workgroup, in thread order
__device__ __forceinline__ uint32_t block512_exclusive_offset(uint32_t cnt, uint32_t* total) {
  __shared__ uint32_t wave_tot512[8];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint32_t inc = cnt;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const uint32_t t = __shfl_up(inc, off, 64);
    if (lane >= off) inc += t;
  }
  if (lane == 63) wave_tot512[wave] = inc;
  __syncthreads();
  uint32_t wbase = 0, all = 0;
#pragma unroll
  for (int w = 0; w < 8; ++w) {
    const uint32_t t = wave_tot512[w];
    wbase += (w < wave) ? t : 0u;
    all += t;
  }
  *total = all;
  return wbase + inc - cnt;
}

// the first workgroup clears the chains of the two scans that follow (gridDim.x = the sums they scan)
__device__ __forceinline__ void clear_chains(unsigned long long* __restrict__ vchain, unsigned long long* __restrict__ qchain) {
  if (blockIdx.x == 0)
    for (int t = threadIdx.x; t < scan_chunks(gridDim.x); t += blockDim.x) {
      vchain[t] = 0ull;
      qchain[t] = 0ull;
    }
}

__global__ __launch_bounds__(512) void tsdf_sparse_class_kernel(const float* __restrict__ tsdf,
                                                                const float* __restrict__ weight,
                                                                const int32_t* __restrict__ block_of_slot,
                                                                const int32_t* __restrict__ slots, Grid g, float min_weight,
                                                                uint16_t* __restrict__ words, uint32_t* __restrict__ vsum,
                                                                unsigned long long* __restrict__ vchain,
                                                                unsigned long long* __restrict__ qchain) {
  __shared__ float halo_t[729], halo_w[729];
  clear_chains(vchain, qchain);
  int32_t bi, bj, bk;
  block_of(g, (int64_t)block_of_slot[blockIdx.x], &bi, &bj, &bk);
  for (int h = threadIdx.x; h < 729; h += 512) {
    const int hk = h / 81, hj = (h - hk * 81) / 9, hi = h - hk * 81 - hj * 9;
    const int64_t at = storage_index(g, slots, bi, bj, bk, hi, hj, hk);
    halo_t[h] = at >= 0 ? tsdf[at] : 1.0f;
    halo_w[h] = at >= 0 ? weight[at] : -1.0f;
  }
  __syncthreads();
  const int li = threadIdx.x & 7, lj = (threadIdx.x >> 3) & 7, lk = threadIdx.x >> 6;
  const int h0 = lk * 81 + lj * 9 + li;
  uint32_t c = (tsdf_observed(halo_w[h0], min_weight) ? kObserved : 0u) | (tsdf_inside(halo_t[h0]) ? kInside : 0u);
  if (c & kObserved) {
    float t[8], w[8];
#pragma unroll
    for (int s = 0; s < 8; ++s) {
      const int h = h0 + (s & 1) + ((s >> 1) & 1) * 9 + (s >> 2) * 81;
      t[s] = halo_t[h];
      w[s] = halo_w[h];
    }
    if (tsdf_cell_active(t, w, min_weight)) c |= kCellActive;
  }
  const uint32_t active = c & kCellActive;
  uint32_t total;
  const uint32_t off = block512_exclusive_offset(active, &total);
  words[(int64_t)blockIdx.x * kTsdfBlockSamples + threadIdx.x] = (uint16_t)(c | (off << kRankShift));
  if (threadIdx.x == 0) vsum[blockIdx.x] = total;
}

// the word of the sample at place (li, lj, lk) relative to the block; 0 where there is no such sample
__device__ __forceinline__ uint32_t word_at(const Grid& g, const int32_t* __restrict__ slots,
                                            const uint16_t* __restrict__ words, int32_t bi, int32_t bj, int32_t bk, int li,
                                            int lj, int lk, int64_t* at_out = nullptr) {
  const int64_t at = storage_index(g, slots, bi, bj, bk, li, lj, lk);
  if (at_out) *at_out = at;
  return at >= 0 ? (uint32_t)words[at] : 0u;
}

__global__ __launch_bounds__(512) void tsdf_sparse_quads_kernel(const uint16_t* __restrict__ words,
                                                                const int32_t* __restrict__ block_of_slot,
                                                                const int32_t* __restrict__ slots, Grid g,
                                                                uint8_t* __restrict__ quads, uint32_t* __restrict__ qsum) {
  int32_t bi, bj, bk;
  block_of(g, (int64_t)block_of_slot[blockIdx.x], &bi, &bj, &bk);
  const int at[3] = {(int)(threadIdx.x & 7), (int)((threadIdx.x >> 3) & 7), (int)(threadIdx.x >> 6)};
  const int64_t n = (int64_t)blockIdx.x * kTsdfBlockSamples + threadIdx.x;
  const uint32_t c = words[n];
  uint32_t bits = 0;
  if (c & kObserved) {
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      int up[3] = {at[0], at[1], at[2]};
      up[a] += 1;
      const uint32_t cu = word_at(g, slots, words, bi, bj, bk, up[0], up[1], up[2]);
      if (!(cu & kObserved) || ((cu ^ c) & kInside) == 0u) continue;
      int32_t cells[4][3];
      tsdf_quad_cells(a, cells);
      bool all = true;
#pragma unroll
      for (int q = 0; q < 4; ++q)
        all = all && (word_at(g, slots, words, bi, bj, bk, at[0] + cells[q][0], at[1] + cells[q][1], at[2] + cells[q][2]) &
                      kCellActive) != 0u;
      bits |= all ? (1u << a) : 0u;
    }
  }
  quads[n] = (uint8_t)bits;
  uint32_t total;
  (void)block512_exclusive_offset((uint32_t)__popc(bits), &total);
  if (threadIdx.x == 0) qsum[blockIdx.x] = total;
}

// both sums scanned in place; sums[n] = the total
__global__ __launch_bounds__(1024) void tsdf_sparse_scan2_kernel(uint32_t* __restrict__ vsum, uint32_t* __restrict__ qsum,
                                                                 int n, unsigned long long* __restrict__ vchain,
                                                                 unsigned long long* __restrict__ qchain, int c_off,
                                                                 int chunks) {
  (void)chained_scan_inplace(vsum, n, vchain, c_off, chunks);
  __syncthreads();      // the scan's shared words are written again
  (void)chained_scan_inplace(qsum, n, qchain, c_off, chunks);
}

template <bool kColour>
__global__ __launch_bounds__(512) void tsdf_sparse_emit_kernel(Arrays vol, Grid g, const int32_t* __restrict__ slots,
                                                               const uint16_t* __restrict__ words,
                                                               const uint8_t* __restrict__ quads,
                                                               const uint32_t* __restrict__ vsum,
                                                               const uint32_t* __restrict__ qsum,
                                                               float* __restrict__ vertices, float* __restrict__ normals,
                                                               float* __restrict__ colours, int32_t* __restrict__ faces,
                                                               int32_t* __restrict__ cells_out) {
  int32_t bi, bj, bk;
  block_of(g, (int64_t)vol.block_of_slot[blockIdx.x], &bi, &bj, &bk);
  const int at[3] = {(int)(threadIdx.x & 7), (int)((threadIdx.x >> 3) & 7), (int)(threadIdx.x >> 6)};
  const int64_t n = (int64_t)blockIdx.x * kTsdfBlockSamples + threadIdx.x;
  const uint32_t c = words[n], bits = quads[n];
  if (c & kCellActive) {
    int64_t corner[8];
    float t[8];
#pragma unroll
    for (int s = 0; s < 8; ++s) {
      // (an active cell has all 8; the clamp keeps a plan that the table no longer matches inside the arrays)
      corner[s] = max(storage_index(g, slots, bi, bj, bk, at[0] + (s & 1), at[1] + ((s >> 1) & 1), at[2] + (s >> 2)),
                      (int64_t)0);
      t[s] = vol.tsdf[corner[s]];
    }
    float local[3], normal[3];
    tsdf_cell_vertex(t, local, normal);
    const size_t vi = (size_t)vsum[blockIdx.x] + ((c >> kRankShift) & 511u);
    const int32_t cell[3] = {8 * bi + at[0], 8 * bj + at[1], 8 * bk + at[2]};
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      vertices[vi * 3 + a] = tsdf_vertex_world(vol.lo[a], vol.voxel, cell[a], local[a]);
      normals[vi * 3 + a] = normal[a];
      cells_out[vi * 3 + a] = cell[a];
    }
    if constexpr (kColour) {
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) {
        float v[8];
#pragma unroll
        for (int s = 0; s < 8; ++s) v[s] = vol.colour[corner[s] * 3 + ch];
        colours[vi * 3 + ch] = tsdf_cell_colour(v);
      }
    }
  }
  const uint32_t cnt = (uint32_t)__popc(bits);
  uint32_t total;
  size_t q = (size_t)qsum[blockIdx.x] + block512_exclusive_offset(cnt, &total);
  if (bits) {
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      if (!((bits >> a) & 1u)) continue;
      int32_t cells[4][3], v[4], f[6];
      tsdf_quad_cells(a, cells);
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        int64_t m;
        const uint32_t cw = word_at(g, slots, words, bi, bj, bk, at[0] + cells[u][0], at[1] + cells[u][1],
                                    at[2] + cells[u][2], &m);
        v[u] = (int32_t)(vsum[max(m, (int64_t)0) / kTsdfBlockSamples] + ((cw >> kRankShift) & 511u));    // (a quad has all four)
      }
      tsdf_quad_faces(v, (c & kInside) != 0u, f);
#pragma unroll
      for (int u = 0; u < 6; ++u) faces[q * 6 + u] = f[u];
      ++q;
    }
  }
}

// ---- workspaces ------------------------------------------------------------------------------------------------------
struct CommitTmp {
  uint32_t* sums;                // [nblk + 1] allocated blocks per workgroup of the grid, scanned in place; [nblk] = B
  unsigned long long* chain;     // [scan_chunks(nblk)]
};
CommitTmp carve_commit_tmp(Carver& c, int64_t G) {
  const size_t nblk = (size_t)((G + 255) / 256);
  CommitTmp t;
  t.sums = c.take<uint32_t>(nblk + 1);
  t.chain = c.take<unsigned long long>((size_t)scan_chunks(nblk));
  return t;
}

struct ExtractTmp {
  uint16_t* words;   // [B,512] class bits and cell ranks
  uint8_t* quads;    // [B,512] quad bits
  uint32_t* vsum;    // [B + 1] active cells per block, scanned in place; [B] = the vertices
  uint32_t* qsum;    // [B + 1] quads per block, likewise
  unsigned long long* vchain;   // [scan_chunks(B)] each
  unsigned long long* qchain;
};
ExtractTmp carve_extract_tmp(Carver& c, int64_t B) {
  const size_t b = (size_t)(B > 0 ? B : 1);
  ExtractTmp t;
  t.words = c.take<uint16_t>(b * kTsdfBlockSamples);
  t.quads = c.take<uint8_t>(b * kTsdfBlockSamples);
  t.vsum = c.take<uint32_t>(b + 1);
  t.qsum = c.take<uint32_t>(b + 1);
  t.vchain = c.take<unsigned long long>((size_t)scan_chunks(b));
  t.qchain = c.take<unsigned long long>((size_t)scan_chunks(b));
  return t;
}

// The successful plans by (device, tmp): an apply follows indices out of tmp, so it runs only behind a plan of its kind
// and sizes.
enum PlanKind { kCommitPlan, kExtractPlan };
struct Plan { int device; const void* tmp; PlanKind kind; int32_t nx, ny, nz; int64_t B; };
std::mutex g_plan_mutex;
std::vector<Plan> g_plans;

void forget_plan(int device, const void* tmp) {
  std::lock_guard<std::mutex> lock(g_plan_mutex);
  for (size_t k = 0; k < g_plans.size(); ++k)
    if (g_plans[k].device == device && g_plans[k].tmp == tmp) { g_plans.erase(g_plans.begin() + k); break; }
}
void add_plan(const Plan& p) {
  std::lock_guard<std::mutex> lock(g_plan_mutex);
  if (g_plans.size() >= 64) g_plans.erase(g_plans.begin());
  g_plans.push_back(p);
}
bool planned(int device, const void* tmp, PlanKind kind, const hgs_tsdf_sparse* v) {
  std::lock_guard<std::mutex> lock(g_plan_mutex);
  for (const Plan& p : g_plans)
    if (p.device == device && p.tmp == tmp)
      return p.kind == kind && p.nx == v->nx && p.ny == v->ny && p.nz == v->nz && p.B == (int64_t)v->n_blocks;
  return false;
}

bool positive_finite(float x) { return x > 0.0f && x - x == 0.0f; }

int refuse(const char* why) {
  set_error("%s", why);
  return HGS_ERR_INVALID;
}

// the block grid of a lattice; 0 where the lattice or the grid is refused (hgs_last_error names it)
int64_t grid_blocks(int32_t nx, int32_t ny, int32_t nz, Grid* g) {
  if (nx < 1 || ny < 1 || nz < 1) {
    set_error("bad sizes: a lattice of %d x %d x %d samples; every dimension >= 1 expected", nx, ny, nz);
    return 0;
  }
  const int64_t gx = tsdf_block_grid(nx), gy = tsdf_block_grid(ny), gz = tsdf_block_grid(nz);
  if (gx * gy > kMaxGridBlocks || gx * gy * gz > kMaxGridBlocks) {
    set_error("bad sizes: a block grid of %lld x %lld x %lld; at most 2^31 - 1 blocks expected", (long long)gx, (long long)gy,
              (long long)gz);
    return 0;
  }
  if (g) *g = Grid{{(int32_t)gx, (int32_t)gy, (int32_t)gz}, {nx, ny, nz}};
  return gx * gy * gz;
}

enum Stage { kBeforeCommit, kCommitApply, kAfterCommit };

// what every call asks of the volume
int check_sparse(const hgs_tsdf_sparse* v, Stage stage, Grid* g, int64_t* G) {
  if (!v) return refuse("null argument: the volume");
  *G = grid_blocks(v->nx, v->ny, v->nz, g);
  if (*G == 0) return HGS_ERR_INVALID;
  if (!positive_finite(v->voxel)) return refuse("voxel must be positive and finite");
  if (!positive_finite(v->trunc)) return refuse("trunc must be positive and finite");
  if (!(v->max_weight > 0.0f)) return refuse("max_weight must be positive");
  if (!v->table) return refuse("null argument: table");
  if ((uintptr_t)v->table & (kAlign - 1)) { set_error("table must be %d-byte aligned", (int)kAlign); return HGS_ERR_INVALID; }
  if (stage == kBeforeCommit) {
    if (v->n_blocks != -1) return refuse("the volume is committed (n_blocks != -1): its table is final, no mark or commit plan");
    return HGS_OK;
  }
  if (v->n_blocks < 0) return refuse("the volume is not committed (n_blocks < 0): commit it first");
  if ((int64_t)v->n_blocks > *G) return refuse("bad sizes: n_blocks exceeds the block grid");
  if (v->capacity < v->n_blocks) {
    set_error("bad sizes: slot arrays of %d blocks for n_blocks = %d", v->capacity, v->n_blocks);
    return HGS_ERR_INVALID;
  }
  if (!v->block_of_slot) return refuse("null argument: block_of_slot");
  if ((uintptr_t)v->block_of_slot & 3u) return refuse("block_of_slot must be 4-byte aligned");
  if (stage == kCommitApply) return HGS_OK;
  if (!v->tsdf || !v->weight) return refuse("null argument: tsdf / weight");
  if (((uintptr_t)v->tsdf | (uintptr_t)v->weight | (uintptr_t)v->colour) & 15u)
    return refuse("tsdf / weight / colour must be 16-byte aligned");
  return HGS_OK;
}

int check_views(const hgs_tsdf_view* views, int32_t n_views, bool colour, bool marking) {
  if (n_views < 1 || n_views > kMaxViews) {
    set_error("bad sizes: n_views=%d not in [1, %d]", n_views, kMaxViews);
    return HGS_ERR_INVALID;
  }
  if (!views) return refuse("null argument: views");
  for (int v = 0; v < n_views; ++v) {
    const hgs_tsdf_view& a = views[v];
    if (a.W < 1 || a.H < 1 || (int64_t)a.W * a.H > 0x7fffffff) {
      set_error("bad sizes: view %d is %d x %d pixels; W, H >= 1 and at most 2^31 - 1 pixels expected", v, a.W, a.H);
      return HGS_ERR_INVALID;
    }
    if (!a.depth) { set_error("null argument: the depth of view %d", v); return HGS_ERR_INVALID; }
    if (a.rgb && !colour) { set_error("view %d has rgb but the volume has no colour", v); return HGS_ERR_INVALID; }
    if (((uintptr_t)a.depth | (uintptr_t)a.weight | (uintptr_t)a.rgb) & 3u) {
      set_error("the planes of view %d must be 4-byte aligned", v);
      return HGS_ERR_INVALID;
    }
    if (marking && !(positive_finite(a.tanfovx) && positive_finite(a.tanfovy) && a.tanfovx <= kTsdfMaxTan &&
                     a.tanfovy <= kTsdfMaxTan)) {
      set_error("field of view: view %d has tangents %g, %g; positive and at most %g expected of a marked view", v,
                (double)a.tanfovx, (double)a.tanfovy, (double)kTsdfMaxTan);
      return HGS_ERR_INVALID;
    }
  }
  return HGS_OK;
}

int check_tmp(const void* tmp) {
  if (!tmp) return refuse("null argument: tmp");
  if ((uintptr_t)tmp & (kAlign - 1)) { set_error("tmp must be %d-byte aligned", (int)kAlign); return HGS_ERR_INVALID; }
  return HGS_OK;
}

int check_extract(const hgs_tsdf_sparse* v, const void* tmp, Grid* g, int64_t* G) {
  if (int rc = check_sparse(v, kAfterCommit, g, G)) return rc;
  if ((int64_t)v->n_blocks > kMaxExtractBlocks) {
    set_error("bad sizes: %d blocks; an extraction takes at most %lld (its quad offsets are 32-bit)", v->n_blocks,
              (long long)kMaxExtractBlocks);
    return HGS_ERR_INVALID;
  }
  return check_tmp(tmp);
}

Arrays arrays_of(const hgs_tsdf_sparse* v) {
  return Arrays{v->tsdf, v->weight, v->colour, v->block_of_slot, {v->lo[0], v->lo[1], v->lo[2]}, v->voxel, v->trunc,
                v->max_weight};
}

Views views_of(const hgs_tsdf_view* views, int32_t n_views) {
  Views va;
  for (int v = 0; v < kMaxViews; ++v) va.v[v] = views[v < n_views ? v : 0];
  return va;
}

}  // namespace
}  // namespace hgs

using namespace hgs;

extern "C" {

int hgs_tsdf_sparse_table_layout(int32_t nx, int32_t ny, int32_t nz, int64_t layout[4]) {
  if (!layout) return refuse("null argument: layout");
  const int64_t G = grid_blocks(nx, ny, nz, nullptr);
  if (G == 0) return HGS_ERR_INVALID;
  Carver c(nullptr);
  (void)c.take<int32_t>((size_t)G);
  layout[0] = G;
  layout[1] = (int64_t)c.offset;
  (void)c.take<uint8_t>((size_t)G);
  layout[2] = (int64_t)c.offset;
  Carver whole(nullptr);
  carve_table(whole, G);
  layout[3] = (int64_t)whole.bytes(0);   // the table is required to be kAlign-aligned: no slack
  return HGS_OK;
}

size_t hgs_tsdf_sparse_commit_tmp_bytes(int32_t nx, int32_t ny, int32_t nz) {
  const int64_t G = grid_blocks(nx, ny, nz, nullptr);
  if (G == 0) return 0;
  Carver c(nullptr);
  carve_commit_tmp(c, G);
  return c.bytes(0);
}

size_t hgs_tsdf_sparse_extract_tmp_bytes(int32_t n_blocks) {
  if (n_blocks < 0 || (int64_t)n_blocks > kMaxExtractBlocks) return 0;
  Carver c(nullptr);
  carve_extract_tmp(c, n_blocks);
  return c.bytes(0);
}

int hgs_tsdf_sparse_mark(const hgs_tsdf_sparse* volume, const hgs_tsdf_view* views, int32_t n_views, hgs_stream_t stream,
                         int device) {
  Grid g;
  int64_t G;
  if (int rc = check_sparse(volume, kBeforeCommit, &g, &G)) return rc;
  if (int rc = check_views(views, n_views, true, true)) return rc;
  const int32_t S = tsdf_block_steps(volume->trunc, volume->voxel);
  if (S > kTsdfMaxSteps) {
    set_error("bad sizes: trunc is more than %d voxels", kTsdfMaxSteps);
    return HGS_ERR_INVALID;
  }
  HGS_HIP(hipSetDevice(device));
  hipStream_t s = static_cast<hipStream_t>(stream);
  Carver c(volume->table);
  const Table t = carve_table(c, G);
  int64_t pixels = 0;
  for (int v = 0; v < n_views; ++v) pixels = max(pixels, (int64_t)views[v].W * views[v].H);
  const dim3 grid((unsigned)((pixels + 255) / 256), (unsigned)n_views), block(256);
  hipLaunchKernelGGL(tsdf_sparse_mark_kernel, grid, block, 0, s, views_of(views, n_views), g, volume->lo[0], volume->lo[1],
                     volume->lo[2], volume->voxel, volume->trunc, S, t.marks, t.state);
  HGS_LAUNCH_CHECK("tsdf_sparse_mark", s, false);
  return HGS_OK;
}

int hgs_tsdf_sparse_commit_plan(const hgs_tsdf_sparse* volume, void* tmp, int64_t* n_blocks_host, hgs_stream_t stream,
                                int device) {
  Grid g;
  int64_t G;
  if (int rc = check_sparse(volume, kBeforeCommit, &g, &G)) return rc;
  if (int rc = check_tmp(tmp)) return rc;
  if (!n_blocks_host) return refuse("null argument: n_blocks_host");
  forget_plan(device, tmp);
  HGS_HIP(hipSetDevice(device));
  hipStream_t s = static_cast<hipStream_t>(stream);
  Carver ct(volume->table), cw(tmp);
  const Table t = carve_table(ct, G);
  const CommitTmp w = carve_commit_tmp(cw, G);
  const int nblk = (int)((G + 255) / 256);
  hipLaunchKernelGGL(tsdf_sparse_dilate_kernel, dim3((unsigned)nblk), dim3(256), 0, s, t.marks, g, G, t.slots, w.sums,
                     w.chain);
  HGS_LAUNCH_CHECK("tsdf_sparse_dilate", s, false);
  if (int rc = launch_scan_chunks(tsdf_sparse_scan_kernel, "tsdf_sparse_scan", nblk, s, w.sums, nblk, w.chain)) return rc;
  // ---- the one host wait
  uint32_t total = 0, refusal = 0;
  HGS_HIP(hipMemcpyAsync(&total, w.sums + nblk, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
  HGS_HIP(hipMemcpyAsync(&refusal, t.state, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
  HGS_HIP(wait_stream(s));
  if (refusal != 0u) {
    set_error("sub-pixel grid: a marked pixel's footprint at the far end of its band is more than %d x 2 voxels wide",
              kTsdfMaxSub);
    return HGS_ERR_INVALID;
  }
  *n_blocks_host = (int64_t)total;
  Plan p{device, tmp, kCommitPlan, volume->nx, volume->ny, volume->nz, (int64_t)total};
  add_plan(p);
  return HGS_OK;
}

int hgs_tsdf_sparse_commit_apply(const hgs_tsdf_sparse* volume, const void* tmp, hgs_stream_t stream, int device) {
  Grid g;
  int64_t G;
  if (int rc = check_sparse(volume, kCommitApply, &g, &G)) return rc;
  if (int rc = check_tmp(tmp)) return rc;
  if (!planned(device, tmp, kCommitPlan, volume))
    return refuse("no successful hgs_tsdf_sparse_commit_plan of these dimensions and this n_blocks on this (device, tmp)");
  HGS_HIP(hipSetDevice(device));
  hipStream_t s = static_cast<hipStream_t>(stream);
  Carver ct(volume->table), cw(const_cast<void*>(tmp));
  const Table t = carve_table(ct, G);
  const CommitTmp w = carve_commit_tmp(cw, G);
  const int nblk = (int)((G + 255) / 256);
  hipLaunchKernelGGL(tsdf_sparse_assign_kernel, dim3((unsigned)nblk), dim3(256), 0, s, G, volume->n_blocks, t.slots, w.sums,
                     volume->block_of_slot);
  HGS_LAUNCH_CHECK("tsdf_sparse_assign", s, false);
  return HGS_OK;
}

int hgs_tsdf_sparse_integrate(const hgs_tsdf_sparse* volume, const hgs_tsdf_view* views, int32_t n_views,
                              hgs_stream_t stream, int device) {
  Grid g;
  int64_t G;
  if (int rc = check_sparse(volume, kAfterCommit, &g, &G)) return rc;
  if (int rc = check_views(views, n_views, volume->colour != nullptr, false)) return rc;
  if (volume->n_blocks == 0) return HGS_OK;
  HGS_HIP(hipSetDevice(device));
  hipStream_t s = static_cast<hipStream_t>(stream);
  const dim3 grid((unsigned)volume->n_blocks), block(128);
  if (volume->colour) {
    hipLaunchKernelGGL(tsdf_sparse_integrate_kernel<true>, grid, block, 0, s, arrays_of(volume), g, views_of(views, n_views),
                       (int)n_views);
  } else {
    hipLaunchKernelGGL(tsdf_sparse_integrate_kernel<false>, grid, block, 0, s, arrays_of(volume), g,
                       views_of(views, n_views), (int)n_views);
  }
  HGS_LAUNCH_CHECK("tsdf_sparse_integrate", s, false);
  return HGS_OK;
}

int hgs_tsdf_sparse_extract_plan(const hgs_tsdf_sparse* volume, float min_weight, void* tmp, int64_t totals_host[2],
                                 hgs_stream_t stream, int device) {
  Grid g;
  int64_t G;
  if (int rc = check_extract(volume, tmp, &g, &G)) return rc;
  if (!positive_finite(min_weight)) return refuse("min_weight must be positive and finite");
  if (!totals_host) return refuse("null argument: totals_host");
  forget_plan(device, tmp);
  const int32_t B = volume->n_blocks;
  if (B > 0) {
    HGS_HIP(hipSetDevice(device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    Carver ct(volume->table), cw(tmp);
    const Table t = carve_table(ct, G);
    const ExtractTmp w = carve_extract_tmp(cw, B);
    const dim3 grid((unsigned)B), block(512);
    hipLaunchKernelGGL(tsdf_sparse_class_kernel, grid, block, 0, s, volume->tsdf, volume->weight, volume->block_of_slot,
                       t.slots, g, min_weight, w.words, w.vsum, w.vchain, w.qchain);
    HGS_LAUNCH_CHECK("tsdf_sparse_class", s, false);
    hipLaunchKernelGGL(tsdf_sparse_quads_kernel, grid, block, 0, s, w.words, volume->block_of_slot, t.slots, g, w.quads,
                       w.qsum);
    HGS_LAUNCH_CHECK("tsdf_sparse_quads", s, false);
    if (int rc = launch_scan_chunks(tsdf_sparse_scan2_kernel, "tsdf_sparse_scan2", B, s, w.vsum, w.qsum, B, w.vchain,
                                    w.qchain))
      return rc;
    // ---- the one host wait
    uint32_t totals[2];
    HGS_HIP(hipMemcpyAsync(&totals[0], w.vsum + B, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    HGS_HIP(hipMemcpyAsync(&totals[1], w.qsum + B, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    HGS_HIP(wait_stream(s));
    totals_host[0] = (int64_t)totals[0];
    totals_host[1] = (int64_t)totals[1];
  } else {
    totals_host[0] = totals_host[1] = 0;
  }
  Plan p{device, tmp, kExtractPlan, volume->nx, volume->ny, volume->nz, (int64_t)B};
  add_plan(p);
  return HGS_OK;
}

int hgs_tsdf_sparse_extract_apply(const hgs_tsdf_sparse* volume, const void* tmp, float* vertices, float* normals,
                                  float* colours, int32_t* faces, int32_t* cells, hgs_stream_t stream, int device) {
  Grid g;
  int64_t G;
  if (int rc = check_extract(volume, tmp, &g, &G)) return rc;
  if (colours && !volume->colour) return refuse("colours asked of a volume that has no colour");
  if (!vertices || !normals || !faces || !cells) return refuse("null argument: vertices / normals / faces / cells");
  if (((uintptr_t)vertices | (uintptr_t)normals | (uintptr_t)colours | (uintptr_t)faces | (uintptr_t)cells) & 3u)
    return refuse("vertices / normals / colours / faces / cells must be 4-byte aligned");
  if (!planned(device, tmp, kExtractPlan, volume))
    return refuse("no successful hgs_tsdf_sparse_extract_plan of these dimensions and this n_blocks on this (device, tmp)");
  const int32_t B = volume->n_blocks;
  if (B == 0) return HGS_OK;
  HGS_HIP(hipSetDevice(device));
  hipStream_t s = static_cast<hipStream_t>(stream);
  Carver ct(volume->table), cw(const_cast<void*>(tmp));
  const Table t = carve_table(ct, G);
  const ExtractTmp w = carve_extract_tmp(cw, B);
  const dim3 grid((unsigned)B), block(512);
  if (colours) {
    hipLaunchKernelGGL(tsdf_sparse_emit_kernel<true>, grid, block, 0, s, arrays_of(volume), g, t.slots, w.words, w.quads,
                       w.vsum, w.qsum, vertices, normals, colours, faces, cells);
  } else {
    hipLaunchKernelGGL(tsdf_sparse_emit_kernel<false>, grid, block, 0, s, arrays_of(volume), g, t.slots, w.words, w.quads,
                       w.vsum, w.qsum, vertices, normals, colours, faces, cells);
  }
  HGS_LAUNCH_CHECK("tsdf_sparse_emit", s, false);
  return HGS_OK;
}

}  // extern "C"
