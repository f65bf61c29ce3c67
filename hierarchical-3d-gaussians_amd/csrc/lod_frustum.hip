// Frustum-culled hierarchy cut (opt-in, beside K9 / K10 of lod.hip, which stay as they are): the LOD cut, the frustum
// test on view-independent bounding spheres, the interpolation weights and the sibling counts in ONE call.
//
// The rule (include/hgs.h): node n carries a ball (c_n, R_n) around its own rows; an entry of node
// n with parent p is dropped iff one of the five planes has BOTH balls, their radii scaled by radius_scale, outside.
// Everything that decides is float32 in a fixed order with contraction off (tests/frustum_spec.py restates it), so a
// culled cut is exactly the unculled cut minus the dropped entries: order, parents, weights and sibling counts of the
// kept ones do not change.
//
// Layout as lod.hip: per-node emission counts, workgroup sums, the chained scan of common.h, an emit pass in ascending
// node order, one host wait for the two counts.  The weights are computed where an entry is emitted (the node's and the
// parent's box are in cache from the mark pass), which saves the separate pass over the cut that K10 is.
#include "common.h"

namespace hgs {
namespace {

constexpr int kNodeInts = 7;   // depth,parent,start,count_leafs,count_merged,start_children,count_children
constexpr int kMaxLevels = 64;
constexpr float kFltMax = 3.4028234663852886e38f;

struct Vec3 { float x, y, z; };
// five planes (a, d), a . x + d >= 0 inside, and the factor on the radii; passed by value: uniform across the grid
struct Frustum { float4 p[5]; float rs; };

// lod.hip's node_size, restated (that file keeps its kernels untouched)
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

// One thread per node: the ball around the node's own rows.  bad[0] = 1 + the first-seen node whose rows leave [0, G).
__global__ __launch_bounds__(256) void frustum_bounds_kernel(const int32_t* __restrict__ nodes, int N,
                                                             const float* __restrict__ means,
                                                             const float* __restrict__ scales, int G,
                                                             float4* __restrict__ bounds, uint32_t* __restrict__ bad) {
#pragma clang fp contract(off)
  const int n = blockIdx.x * 256 + threadIdx.x;
  if (n >= N) return;
  const int32_t* nd = nodes + (size_t)n * kNodeInts;
  const long long start = nd[2];
  const long long cnt = (long long)nd[3] + (long long)nd[4];
  float4 b = make_float4(0.0f, 0.0f, 0.0f, __builtin_inff());      // no rows: never outside a plane
  if (nd[3] < 0 || nd[4] < 0 || (cnt > 0 && (start < 0 || start + cnt > (long long)G))) {
    atomicCAS(bad, 0u, (uint32_t)n + 1u);
  } else if (cnt > 0) {
    float sx = 0.0f, sy = 0.0f, sz = 0.0f;
    for (long long i = start; i < start + cnt; ++i) {
      sx += means[i * 3 + 0];
      sy += means[i * 3 + 1];
      sz += means[i * 3 + 2];
    }
    const float fc = (float)cnt;
    const float cx = sx / fc, cy = sy / fc, cz = sz / fc;
    float R = 0.0f;
    for (long long i = start; i < start + cnt; ++i) {
      const float dx = means[i * 3 + 0] - cx, dy = means[i * 3 + 1] - cy, dz = means[i * 3 + 2] - cz;
      const float d2 = (dx * dx + dy * dy) + dz * dz;
      const float smax = fmaxf(fmaxf(scales[i * 3 + 0], scales[i * 3 + 1]), scales[i * 3 + 2]);
      R = fmaxf(R, sqrtf(d2) + 3.0f * smax);
    }
    b = make_float4(cx, cy, cz, R);
  }
  bounds[n] = b;
}

// sums of one workgroup's kept and unculled counts -> block_sums[blockIdx.x], block_all[blockIdx.x]
__device__ __forceinline__ void block_totals(uint32_t kept, uint32_t all, uint32_t* __restrict__ block_sums,
                                             uint32_t* __restrict__ block_all) {
  __shared__ uint32_t wave_kept[4], wave_all[4];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    kept += __shfl_xor(kept, off, 64);
    all += __shfl_xor(all, off, 64);
  }
  if ((threadIdx.x & 63) == 0) { wave_kept[threadIdx.x >> 6] = kept; wave_all[threadIdx.x >> 6] = all; }
  __syncthreads();
  if (threadIdx.x == 0) {
    block_sums[blockIdx.x] = wave_kept[0] + wave_kept[1] + wave_kept[2] + wave_kept[3];
    block_all[blockIdx.x] = wave_all[0] + wave_all[1] + wave_all[2] + wave_all[3];
  }
}

// Single-pass route (boxes nest: lod.hip, lod_mark_kernel): cut decision and cull per node, one launch over the N nodes.
__global__ __launch_bounds__(256) void frustum_mark_kernel(const int32_t* __restrict__ nodes,
                                                           const float* __restrict__ boxes,
                                                           const float4* __restrict__ bounds, int N, float tau, Vec3 vp,
                                                           Frustum f, uint32_t* __restrict__ emit_cnt,
                                                           uint32_t* __restrict__ block_sums,
                                                           uint32_t* __restrict__ block_all,
                                                           unsigned long long* __restrict__ chain) {
  if (blockIdx.x == 0) {      // for the scan launch behind this one: its chain, and the unculled total it adds up
    for (int t = threadIdx.x; t < scan_chunks(gridDim.x); t += 256) chain[t] = 0ull;
    if (threadIdx.x == 0) block_sums[gridDim.x + 1] = 0u;
  }
  const int n = blockIdx.x * 256 + threadIdx.x;
  uint32_t cnt = 0, kept = 0;
  if (n < N) {
    const int32_t* nd = nodes + (size_t)n * kNodeInts;
    const int par = nd[1];
    const float sn = node_size(boxes, n, vp);
    const bool coarse = sn >= tau;
    const bool reached = coarse || par < 0 || node_size(boxes, par, vp) >= tau;
    if (reached) cnt = coarse ? (uint32_t)nd[3] : (uint32_t)(nd[3] + nd[4]);
    kept = (cnt && !entry_culled(bounds, n, par, f)) ? cnt : 0u;
    emit_cnt[n] = kept;
  }
  block_totals(kept, cnt, block_sums, block_all);
}

// Level-by-level route, restated from lod.hip (lod_init_kernel / lod_expand_level_kernel): the unculled counts ...
__global__ void frustum_init_kernel(uint32_t* counts, int32_t* frontier, int N) {
  if (threadIdx.x == 0) {
    counts[0] = N > 0 ? 1u : 0u;
    frontier[0] = 0;
  }
}

__global__ __launch_bounds__(256) void frustum_expand_level_kernel(const int32_t* __restrict__ nodes,
                                                                   const float* __restrict__ boxes, float tau, Vec3 vp,
                                                                   const int32_t* __restrict__ fin,
                                                                   const uint32_t* __restrict__ count_in,
                                                                   int32_t* __restrict__ fout,
                                                                   uint32_t* __restrict__ count_out,
                                                                   uint32_t* __restrict__ emit_cnt) {
  const uint32_t n_in = *count_in;
  for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < n_in; i += gridDim.x * 256u) {
    const int n = fin[i];
    const int32_t* nd = nodes + (size_t)n * kNodeInts;
    const int nch = nd[6];
    const float s = node_size(boxes, n, vp);
    if (s >= tau) {
      emit_cnt[n] = (uint32_t)nd[3];
      if (nch > 0) {
        const uint32_t base = atomicAdd(count_out, (uint32_t)nch);
        const int c0 = nd[5];
        for (int k = 0; k < nch; ++k) fout[base + k] = c0 + k;
      }
    } else {
      emit_cnt[n] = (uint32_t)(nd[3] + nd[4]);
    }
  }
}

// ... then the cull over the marked nodes (emit_cnt: unculled in, kept out) and the workgroup sums
__global__ __launch_bounds__(256) void frustum_cull_kernel(const int32_t* __restrict__ nodes,
                                                           const float4* __restrict__ bounds, int N, Frustum f,
                                                           uint32_t* __restrict__ emit_cnt,
                                                           uint32_t* __restrict__ block_sums,
                                                           uint32_t* __restrict__ block_all,
                                                           unsigned long long* __restrict__ chain) {
  if (blockIdx.x == 0) {      // for the scan launch behind this one: its chain, and the unculled total it adds up
    for (int t = threadIdx.x; t < scan_chunks(gridDim.x); t += 256) chain[t] = 0ull;
    if (threadIdx.x == 0) block_sums[gridDim.x + 1] = 0u;
  }
  const int n = blockIdx.x * 256 + threadIdx.x;
  uint32_t cnt = 0, kept = 0;
  if (n < N) {
    cnt = emit_cnt[n];
    if (cnt) {
      kept = entry_culled(bounds, n, nodes[(size_t)n * kNodeInts + 1], f) ? 0u : cnt;
      if (!kept) emit_cnt[n] = 0u;
    }
  }
  block_totals(kept, cnt, block_sums, block_all);
}

// the chained scan of the kept sums (total -> sums[n]); every chunk also adds its share of the unculled sums to
// sums[n + 1] (zeroed by the kernel in front): one integer add per 8192 workgroups of the mark pass, any order
__global__ __launch_bounds__(1024) void frustum_scan_sums_kernel(uint32_t* __restrict__ sums,
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

// lod.hip's emit pass plus, per emitted node, lod_weights_kernel's expressions
__global__ __launch_bounds__(256) void frustum_emit_kernel(const int32_t* __restrict__ nodes,
                                                           const float* __restrict__ boxes,
                                                           const uint32_t* __restrict__ emit_cnt, int N, float tau,
                                                           Vec3 vp, const uint32_t* __restrict__ block_sums,
                                                           int32_t* __restrict__ render_indices,
                                                           int32_t* __restrict__ parent_indices,
                                                           int32_t* __restrict__ node_indices,
                                                           float* __restrict__ weights,
                                                           int32_t* __restrict__ num_siblings, int capacity) {
#pragma clang fp contract(off)
  __shared__ uint32_t wave_tot[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n = blockIdx.x * 256 + tid;
  const uint32_t cnt = (n < N) ? emit_cnt[n] : 0u;
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
  if (cnt == 0) return;
  const uint32_t pos = block_sums[blockIdx.x] + wbase + inc - cnt;
  const int32_t* nd = nodes + (size_t)n * kNodeInts;
  const int start = nd[2];
  const int par = nd[1];
  int pstart = -1;
  float w = 1.0f;
  int kids = 1;
  if (par >= 0) {
    pstart = nodes[(size_t)par * kNodeInts + 2];
    const float two_tau = 2.0f * tau;
    float sp = node_size(boxes, par, vp);
    if (sp > two_tau) sp = two_tau;
    const float sn = node_size(boxes, n, vp);
    kids = nodes[(size_t)par * kNodeInts + 6];
    const float s0 = fmaxf(0.5f * sp, sn);
    const float diff = sp - s0;
    if (diff > 0.0f) {
      const float tdiff = fmaxf(0.0f, tau - s0);
      w = fmaxf(1.0f - tdiff / diff, 0.0f);
    }
  }
  for (uint32_t k = 0; k < cnt; ++k) {
    const uint32_t o = pos + k;
    if (o < (uint32_t)capacity) {
      render_indices[o] = start + (int)k;
      parent_indices[o] = pstart >= 0 ? pstart : start + (int)k;
      node_indices[o] = n;
      weights[o] = w;
      num_siblings[o] = kids;
    }
  }
}

struct CutViewTmp {
  uint32_t* emit_cnt;    // [N]
  int32_t* frontier_a;   // [N]  (level route only)
  int32_t* frontier_b;   // [N]
  uint32_t* counts;      // [kMaxLevels + 2] frontier sizes of the levels
  uint32_t* block_sums;  // [nblk + 2] kept sums, scanned in place; [nblk] = kept total, [nblk + 1] = unculled total
  uint32_t* block_all;   // [nblk] unculled sums
  unsigned long long* chain;  // [scan_chunks(nblk)]
};
constexpr int kCountWords = kMaxLevels + 2;

inline CutViewTmp carve_cut_view(void* tmp, int32_t N) {
  const size_t n = (size_t)(N > 0 ? N : 1);
  char* p = static_cast<char*>(tmp);
  CutViewTmp t;
  t.emit_cnt = carve<uint32_t>(p, n);
  t.frontier_a = carve<int32_t>(p, n);
  t.frontier_b = carve<int32_t>(p, n);
  t.counts = carve<uint32_t>(p, kCountWords);
  t.block_sums = carve<uint32_t>(p, (n + 255) / 256 + 2);
  t.block_all = carve<uint32_t>(p, (n + 255) / 256);
  t.chain = carve<unsigned long long>(p, (size_t)scan_chunks((n + 255) / 256));
  return t;
}

}  // namespace
}  // namespace hgs

using namespace hgs;

extern "C" {

int hgs_hier_cull_bounds(const int32_t* nodes, int32_t N, const float* means, const float* scales, int32_t G,
                         float* bounds, hgs_stream_t stream, int device) {
  if (N <= 0) return HGS_OK;
  if (!nodes || !means || !scales || !bounds) { set_error("hier_cull_bounds: null argument"); return HGS_ERR_INVALID; }
  if (G < 0) { set_error("hier_cull_bounds: G = %d", G); return HGS_ERR_INVALID; }
  HGS_HIP(hipSetDevice(device));
  hipStream_t s = static_cast<hipStream_t>(stream);
  // the one word the row check reports through: allocated and released here (a bounds build happens once per
  // hierarchy, or when its rows change), so that the call needs no workspace argument
  uint32_t* bad = nullptr;
  HGS_HIP(hipMalloc(&bad, sizeof(uint32_t)));
  hipError_t e = hipMemsetAsync(bad, 0, sizeof(uint32_t), s);
  uint32_t first = 0;
  if (e == hipSuccess) {
    hipLaunchKernelGGL(frustum_bounds_kernel, dim3((N + 255) / 256), dim3(256), 0, s, nodes, N, means, scales, G,
                       reinterpret_cast<float4*>(bounds), bad);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpyAsync(&first, bad, sizeof(uint32_t), hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = wait_stream(s);
  (void)hipFree(bad);
  if (e != hipSuccess) { set_error("hier_cull_bounds: %s", hipGetErrorString(e)); return HGS_ERR_HIP; }
  if (first) {
    set_error("hier_cull_bounds: the rows of node %u lie outside [0, %d)", first - 1u, G);
    return HGS_ERR_INVALID;
  }
  return HGS_OK;
}

size_t hgs_lod_cut_view_tmp_bytes(int32_t N) {
  const size_t n = (size_t)(N > 0 ? N : 1);
  return 3 * align_up(n * 4) + align_up(kCountWords * 4) + align_up(((n + 255) / 256 + 2) * 4) +
         align_up(((n + 255) / 256) * 4) + align_up((size_t)scan_chunks((n + 255) / 256) * 8) + kAlign;
}

int hgs_lod_cut_view(const int32_t* nodes, const float* boxes, const float* bounds, int32_t N, float size,
                     const float viewpoint[3], const float planes[20], float radius_scale, int32_t nested,
                     int32_t* render_indices, int32_t* parent_indices, int32_t* nodes_for_render_indices,
                     float* weights, int32_t* num_siblings, int32_t capacity, void* tmp, int32_t* count_out_host,
                     int32_t* unculled_out_host, hgs_stream_t stream, int device) {
  if (!count_out_host || !unculled_out_host) { set_error("lod_cut_view: null count pointer"); return HGS_ERR_INVALID; }
  *count_out_host = 0;
  *unculled_out_host = 0;
  if (N <= 0) return HGS_OK;
  if (!nodes || !boxes || !bounds || !viewpoint || !planes || !render_indices || !parent_indices ||
      !nodes_for_render_indices || !weights || !num_siblings || !tmp) {
    set_error("lod_cut_view: null argument");
    return HGS_ERR_INVALID;
  }
  if (capacity < 0) { set_error("lod_cut_view: capacity = %d", capacity); return HGS_ERR_INVALID; }
  HGS_HIP(hipSetDevice(device));
  hipStream_t s = static_cast<hipStream_t>(stream);
  const CutViewTmp t = carve_cut_view(tmp, N);
  const Vec3 vp = {viewpoint[0], viewpoint[1], viewpoint[2]};
  Frustum f;
  for (int k = 0; k < 5; ++k) f.p[k] = make_float4(planes[4 * k], planes[4 * k + 1], planes[4 * k + 2], planes[4 * k + 3]);
  f.rs = radius_scale;
  const int nblk = (N + 255) / 256;
  const float4* bnd = reinterpret_cast<const float4*>(bounds);
  if (nested) {
    hipLaunchKernelGGL(frustum_mark_kernel, dim3(nblk), dim3(256), 0, s, nodes, boxes, bnd, N, size, vp, f, t.emit_cnt,
                       t.block_sums, t.block_all, t.chain);
    HGS_LAUNCH_CHECK("frustum_mark", s, false);
  } else {
    HGS_HIP(hipMemsetAsync(t.emit_cnt, 0, (size_t)N * 4, s));
    HGS_HIP(hipMemsetAsync(t.counts, 0, kCountWords * 4, s));
    hipLaunchKernelGGL(frustum_init_kernel, dim3(1), dim3(64), 0, s, t.counts, t.frontier_a, N);
    HGS_LAUNCH_CHECK("frustum_init", s, false);
    // level-synchronous expansion as hgs_expand_to_size: the host looks at the frontier size every 8 levels
    int32_t* fin = t.frontier_a;
    int32_t* fout = t.frontier_b;
    int level = 0;
    bool finished = false;
    while (!finished) {
      const int stop = level + 8;
      for (; level < stop && level < kMaxLevels; ++level) {
        hipLaunchKernelGGL(frustum_expand_level_kernel, dim3(1024), dim3(256), 0, s, nodes, boxes, size, vp, fin,
                           t.counts + level, fout, t.counts + level + 1, t.emit_cnt);
        HGS_LAUNCH_CHECK("frustum_expand_level", s, false);
        int32_t* sw = fin; fin = fout; fout = sw;
      }
      uint32_t next = 0;
      HGS_HIP(hipMemcpyAsync(&next, t.counts + level, 4, hipMemcpyDeviceToHost, s));
      HGS_HIP(wait_stream(s));
      if (next == 0) finished = true;
      else if (level >= kMaxLevels) { set_error("hierarchy deeper than %d levels", kMaxLevels); return HGS_ERR_INVALID; }
    }
    hipLaunchKernelGGL(frustum_cull_kernel, dim3(nblk), dim3(256), 0, s, nodes, bnd, N, f, t.emit_cnt, t.block_sums,
                       t.block_all, t.chain);
    HGS_LAUNCH_CHECK("frustum_cull", s, false);
  }
  const int chunks = scan_chunks(nblk), resident = scan_resident_workgroups();
  for (int c0 = 0; c0 < chunks; c0 += resident) {
    hipLaunchKernelGGL(frustum_scan_sums_kernel, dim3(min(resident, chunks - c0)), dim3(1024), 0, s, t.block_sums,
                       t.block_all, nblk, t.chain, c0, chunks);
    HGS_LAUNCH_CHECK("frustum_scan_sums", s, false);
  }
  // (a grid over the nodes, not over the entries: an empty cut launches nothing of size zero)
  hipLaunchKernelGGL(frustum_emit_kernel, dim3(nblk), dim3(256), 0, s, nodes, boxes, t.emit_cnt, N, size, vp,
                     t.block_sums, render_indices, parent_indices, nodes_for_render_indices, weights, num_siblings,
                     capacity);
  HGS_LAUNCH_CHECK("frustum_emit", s, false);
  uint32_t totals[2] = {0, 0};            // kept, unculled: neighbours, one copy
  HGS_HIP(hipMemcpyAsync(totals, t.block_sums + nblk, 8, hipMemcpyDeviceToHost, s));
  HGS_HIP(wait_stream(s));
  const uint32_t total = totals[0], all = totals[1];
  *unculled_out_host = (int32_t)all;
  if (total > (uint32_t)capacity) {
    *count_out_host = (int32_t)total;     // (the count a retry needs; nothing past `capacity` was written)
    set_error("lod_cut_view: %u entries exceed the output capacity %d", total, capacity);
    return HGS_ERR_INVALID;
  }
  *count_out_host = (int32_t)total;
  return HGS_OK;
}

}  // extern "C"
