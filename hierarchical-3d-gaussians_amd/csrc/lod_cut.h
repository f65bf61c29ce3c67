// The rules of the hierarchy cut, each ONCE, for the four calls that must agree bit for bit: expand_to_size +
// get_interpolation_weights (lod.hip), the frustum-culled cut (lod_frustum.hip), the budget-exact cut (lod_budget.hip)
// and the cut for several views (lod_views.hip); hier_trim.hip takes the workgroup sums and the scan launcher from here,
// hier_reach.hip the squared distance of node_size widened to a box of viewpoints (box_d2).
// The node record is hier_nodes.h's.  What decides -- the size of a node, the cull, the weight -- is float32 in a fixed
// operation order with contraction off (oracle/lod_oracle.py, tests/frustum_spec.py and tests/budget_cut_spec.py restate
// it); the rest is the shape the calls share: per-node emission counts, workgroup sums, the chained scan of common.h, an
// emit pass in ascending node order.
#pragma once
#include "hier_nodes.h"   // the node record

namespace hgs {

// boxes: 8 floats per node = min.xyz+extent, max.xyz+pad
constexpr int kMaxLevels = 64;
constexpr float kFltMax = 3.4028234663852886e38f;

struct Vec3 { float x, y, z; };
// five planes (a, d), a . x + d >= 0 inside, and the factor on the radii; passed by value: uniform across the grid
struct Frustum { float4 p[5]; float rs; };

// ---- the rules -----------------------------------------------------------------------------------------------------
__device__ __forceinline__ float node_size(const float* __restrict__ boxes, int n, Vec3 v) {
#pragma clang fp contract(off)
  const float4 mn = reinterpret_cast<const float4*>(boxes)[(size_t)n * 2 + 0];
  const float4 mx = reinterpret_cast<const float4*>(boxes)[(size_t)n * 2 + 1];
  const float dx = fmaxf(fmaxf(mn.x - v.x, v.x - mx.x), 0.0f);
  const float dy = fmaxf(fmaxf(mn.y - v.y, v.y - mx.y), 0.0f);
  const float dz = fmaxf(fmaxf(mn.z - v.z, v.z - mx.z), 0.0f);
  const float d2 = (dx * dx + dy * dy) + dz * dz;
  const float dist = sqrtf(d2);
  const float s = mn.w / dist;
  return d2 > 0.0f ? s : kFltMax;
}

__device__ __forceinline__ bool ball_outside(float4 b, float4 pl, float rs) {
#pragma clang fp contract(off)
  const float t = ((pl.x * b.x + pl.y * b.y) + pl.z * b.z) + pl.w;
  return t + rs * b.w < 0.0f;       // (NaN compares false: such a ball is never outside)
}

// is an entry of node n (parent par, < 0 at the root) dropped?  The parent's ball -- a second 16-byte gather -- is read
// only when the node's own ball is outside some plane.
__device__ __forceinline__ bool entry_culled(const float4* __restrict__ bounds, int n, int par, const Frustum& f) {
  const float4 bn = bounds[n];
  uint32_t out = 0;
#pragma unroll
  for (int k = 0; k < 5; ++k) out |= ball_outside(bn, f.p[k], f.rs) ? (1u << k) : 0u;
  if (out == 0) return false;
  const float4 bp = bounds[par >= 0 ? par : n];
  bool both = false;
#pragma unroll
  for (int k = 0; k < 5; ++k) both |= ((out >> k) & 1u) && ball_outside(bp, f.p[k], f.rs);
  return both;
}

// The interpolation weight of a node of size sn under a parent of size sp at granularity tau.  Restated from the public
// gaussian-hierarchy source (not vendored in the reference checkout): the transition runs while the parent's size falls
// from 2 tau to tau.
__device__ __forceinline__ float interp_weight(float sp, float sn, float tau) {
#pragma clang fp contract(off)
  const float two_tau = 2.0f * tau;
  if (sp > two_tau) sp = two_tau;
  const float s0 = fmaxf(0.5f * sp, sn);
  const float diff = sp - s0;
  float w = 1.0f;
  if (diff > 0.0f) {
    const float tdiff = fmaxf(0.0f, tau - s0);
    w = fmaxf(1.0f - tdiff / diff, 0.0f);
  }
  return w;
}

// Entries of the node with record nd.  reached: every ancestor is too coarse for this view; coarse: so is the node.
// Too coarse: only the Gaussians no child stands for (the children follow); fine enough: the node as a whole.  The
// callers bring the "size >= tau" verdicts, on floats or on their bit patterns.
__device__ __forceinline__ uint32_t cut_count(bool reached, bool coarse, const int32_t* __restrict__ nd) {
  if (!reached) return 0u;
  return coarse ? (uint32_t)nd[3] : (uint32_t)(nd[3] + nd[4]);
}

// ---- the same rules on operands that are already in registers ------------------------------------------------------
// For the call that loads a node once and judges it for several views (lod_views.hip).  Each is the body of the rule
// above it, word for word, behind another way in; the rules above stay as they are so that the three single-view calls
// compile to what they always did.  tests/test_cut_views_gpu.py holds the two texts together bit for bit.
__device__ __forceinline__ float box_size(float4 mn, float4 mx, Vec3 v) {          // node_size
#pragma clang fp contract(off)
  const float dx = fmaxf(fmaxf(mn.x - v.x, v.x - mx.x), 0.0f);
  const float dy = fmaxf(fmaxf(mn.y - v.y, v.y - mx.y), 0.0f);
  const float dz = fmaxf(fmaxf(mn.z - v.z, v.z - mx.z), 0.0f);
  const float d2 = (dx * dx + dy * dy) + dz * dz;
  const float dist = sqrtf(d2);
  const float s = mn.w / dist;
  return d2 > 0.0f ? s : kFltMax;
}
// box_size with the viewpoint widened to the closed box [lo, hi] (hier_reach.hip), up to its squared distance: the
// caller takes the minimum over its boxes and ends with extent / sqrtf(d2) as box_size does.  lo == hi == v gives
// box_size's d2 bit for bit; the fmaxf chain makes d2 a non-negative number whatever the operands (never NaN).
__device__ __forceinline__ float box_d2(float4 mn, float4 mx, Vec3 lo, Vec3 hi) {
#pragma clang fp contract(off)
  const float dx = fmaxf(fmaxf(mn.x - hi.x, lo.x - mx.x), 0.0f);
  const float dy = fmaxf(fmaxf(mn.y - hi.y, lo.y - mx.y), 0.0f);
  const float dz = fmaxf(fmaxf(mn.z - hi.z, lo.z - mx.z), 0.0f);
  return (dx * dx + dy * dy) + dz * dz;
}
// entry_culled in its two halves: bit k = the ball is outside plane k ...
__device__ __forceinline__ uint32_t planes_outside(float4 b, const Frustum& f) {
  uint32_t out = 0;
#pragma unroll
  for (int k = 0; k < 5; ++k) out |= ball_outside(b, f.p[k], f.rs) ? (1u << k) : 0u;
  return out;
}
// ... and: is the parent's ball outside one of the planes in `out` as well?
__device__ __forceinline__ bool parent_outside_too(uint32_t out, float4 bp, const Frustum& f) {
  bool both = false;
#pragma unroll
  for (int k = 0; k < 5; ++k) both |= ((out >> k) & 1u) && ball_outside(bp, f.p[k], f.rs);
  return both;
}
__device__ __forceinline__ uint32_t cut_count(bool reached, bool coarse, int32_t leafs, int32_t merged) {
  if (!reached) return 0u;
  return coarse ? (uint32_t)leafs : (uint32_t)(leafs + merged);
}

// ---- workgroup sums, their scan, the emit pass (workgroups of 256 threads = 256 nodes) -------------------------------
// For the scan launch behind a kernel that writes workgroup sums: the scan's chain has to be zero when it starts.
__device__ __forceinline__ void clear_scan_chain(unsigned long long* __restrict__ chain) {
  if (blockIdx.x == 0)
    for (int t = threadIdx.x; t < scan_chunks(gridDim.x); t += 256) chain[t] = 0ull;
}
// ... and so has the unculled total the scan adds up behind the kept total, where there is a cull
__device__ __forceinline__ void clear_scan_chain(unsigned long long* __restrict__ chain,
                                                 uint32_t* __restrict__ block_sums) {
  clear_scan_chain(chain);
  if (blockIdx.x == 0 && threadIdx.x == 0) block_sums[gridDim.x + 1] = 0u;
}

// sums of one workgroup's K counts -> out[k][blockIdx.x] (K = 1: the emission counts; K = 2: kept and unculled)
template <int K>
__device__ __forceinline__ void block_totals(const uint32_t (&cnt)[K], uint32_t* const (&out)[K]) {
  __shared__ uint32_t wave_tot[K][4];
  uint32_t v[K];
#pragma unroll
  for (int k = 0; k < K; ++k) v[k] = cnt[k];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] += __shfl_xor(v[k], off, 64);
  }
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int k = 0; k < K; ++k) wave_tot[k][threadIdx.x >> 6] = v[k];
  }
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int k = 0; k < K; ++k) out[k][blockIdx.x] = wave_tot[k][0] + wave_tot[k][1] + wave_tot[k][2] + wave_tot[k][3];
  }
}

// Body of a 1024-thread scan kernel where there is a cull: the chained scan of the kept sums (total -> sums[n]); every
// chunk also adds its share of the unculled sums to sums[n + 1] (zeroed by the kernel in front): one integer add per
// 8192 workgroups of the mark pass, any order.
__device__ __forceinline__ void scan_sums_and_unculled_total(uint32_t* __restrict__ sums,
                                                             const uint32_t* __restrict__ block_all, int n,
                                                             unsigned long long* __restrict__ chain, int c_off,
                                                             int chunks) {
  __shared__ uint32_t all_wave[16];
  const int i0 = ((int)blockIdx.x + c_off) * kScanChunk + (int)threadIdx.x * kScanPer;
  uint32_t a = 0;
#pragma unroll
  for (int k = 0; k < kScanPer; ++k) a += (i0 + k < n) ? block_all[i0 + k] : 0u;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) a += __shfl_xor(a, off, 64);
  if ((threadIdx.x & 63) == 0) all_wave[threadIdx.x >> 6] = a;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t t = 0;
#pragma unroll
    for (int w = 0; w < 16; ++w) t += all_wave[w];
    if (t) atomicAdd(sums + n + 1, t);
  }
  (void)chained_scan_inplace(sums, n, chain, c_off, chunks);
}

// exclusive offset of this thread's count among the counts of its workgroup, in thread order
__device__ __forceinline__ uint32_t block_exclusive_offset(uint32_t cnt) {
  __shared__ uint32_t wave_tot[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint32_t inc = cnt;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const uint32_t t = __shfl_up(inc, off, 64);
    if (lane >= off) inc += t;
  }
  if (lane == 63) wave_tot[wave] = inc;
  __syncthreads();
  uint32_t wbase = 0;
  for (int w = 0; w < wave; ++w) wbase += wave_tot[w];
  return wbase + inc - cnt;
}

// The cnt entries of node n at pos, pos + 1, ...: its rows from `start` on, the parent's row (pstart < 0 at the root:
// the row itself), the node; nothing at or past `capacity`.  kWeights: every entry also gets the node's weight w and
// sibling count kids.
template <bool kWeights>
__device__ __forceinline__ void write_entries(uint32_t pos, uint32_t cnt, int capacity, int n, int start, int pstart,
                                              int32_t* __restrict__ render_indices,
                                              int32_t* __restrict__ parent_indices, int32_t* __restrict__ node_indices,
                                              float* __restrict__ weights = nullptr, float w = 1.0f,
                                              int32_t* __restrict__ num_siblings = nullptr, int kids = 1) {
  for (uint32_t k = 0; k < cnt; ++k) {
    const uint32_t o = pos + k;
    if (o < (uint32_t)capacity) {
      render_indices[o] = start + (int)k;
      parent_indices[o] = pstart >= 0 ? pstart : start + (int)k;
      node_indices[o] = n;
      if constexpr (kWeights) {
        weights[o] = w;
        num_siblings[o] = kids;
      }
    }
  }
}

// ---- host side -----------------------------------------------------------------------------------------------------
// The part of a cut workspace behind the per-node arrays: the workgroup sums and what scans them.
struct SumsTmp {
  uint32_t* block_sums;  // [nblk + 1] sums, scanned in place; [nblk] = total.  With a cull [nblk + 2]: the kept sums,
                         // [nblk] = kept total, [nblk + 1] = unculled total
  uint32_t* block_all;   // [nblk] unculled sums (with a cull)
  unsigned long long* chain;  // [scan_chunks(nblk)] published chunk totals of the scan (cleared by the kernel before it)
};
inline SumsTmp carve_sums(Carver& c, size_t n, bool cull) {
  const size_t nblk = (n + 255) / 256;
  SumsTmp t;
  t.block_sums = c.take<uint32_t>(nblk + (cull ? 2 : 1));
  t.block_all = cull ? c.take<uint32_t>(nblk) : nullptr;
  t.chain = c.take<unsigned long long>((size_t)scan_chunks(nblk));
  return t;
}

// Workspace of the two calls that have a level-by-level route.
struct LevelTmp : SumsTmp {
  uint32_t* emit_cnt;    // [N]
  int32_t* frontier_a;   // [N]  (level route only)
  int32_t* frontier_b;   // [N]
  uint32_t* counts;      // [kMaxLevels + 2] frontier sizes of the levels
};
constexpr int kCountWords = kMaxLevels + 2;
// (a *_tmp_bytes call lays the workspace out on a null Carver and answers c.bytes(kAlign): common.h)
inline LevelTmp carve_levels(Carver& c, int32_t N, bool cull) {
  const size_t n = (size_t)(N > 0 ? N : 1);
  LevelTmp t;
  t.emit_cnt = c.take<uint32_t>(n);
  t.frontier_a = c.take<int32_t>(n);
  t.frontier_b = c.take<int32_t>(n);
  t.counts = c.take<uint32_t>(kCountWords);
  static_cast<SumsTmp&>(t) = carve_sums(c, n, cull);
  return t;
}

// Level-by-level marking (lod.hip): t.emit_cnt = the count of every node the cut reaches, 0 elsewhere.  One launch per
// tree level; the host looks at the frontier size every 8 levels; a hierarchy deeper than kMaxLevels is refused.
int launch_level_marking(const int32_t* nodes, const float* boxes, int32_t N, float tau, Vec3 vp, const LevelTmp& t,
                         hipStream_t s);

// The chained scan over nblk workgroup sums in launches of at most `resident` chunk workgroups (common.h,
// chained_scan_inplace).  kernel(args..., c_off, chunks) is a 1024-thread scan kernel.
template <typename Kernel, typename... Args>
inline int launch_scan_chunks(Kernel kernel, const char* name, int nblk, hipStream_t s, Args... args) {
  const int chunks = scan_chunks(nblk), resident = scan_resident_workgroups();
  for (int c0 = 0; c0 < chunks; c0 += resident) {
    hipLaunchKernelGGL(kernel, dim3(min(resident, chunks - c0)), dim3(1024), 0, s, args..., c0, chunks);
    HGS_LAUNCH_CHECK(name, s, false);
  }
  return HGS_OK;
}

}  // namespace hgs
