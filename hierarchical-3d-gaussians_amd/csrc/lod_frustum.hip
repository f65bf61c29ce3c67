// Frustum-culled hierarchy cut (opt-in, beside K9 / K10 of lod.hip): the LOD cut, the frustum test on view-independent
// bounding spheres, the interpolation weights and the sibling counts in ONE call.
//
// The rule (include/hgs.h): node n carries a ball (c_n, R_n) around its own rows; an entry of node
// n with parent p is dropped iff one of the five planes has BOTH balls, their radii scaled by radius_scale, outside.
// Everything that decides is float32 in a fixed order with contraction off (lod_cut.h holds it, tests/frustum_spec.py
// restates it), so a culled cut is exactly the unculled cut minus the dropped entries: order, parents, weights and
// sibling counts of the kept ones do not change.
//
// Layout as lod.hip, from the same parts of lod_cut.h: per-node emission counts, workgroup sums, the chained scan of
// common.h, an emit pass in ascending node order, one host wait for the two counts.  The weights are computed where an
// entry is emitted (the node's and the parent's box are in cache from the mark pass), which saves the separate pass
// over the cut that K10 is.
#include "lod_cut.h"

namespace hgs {
namespace {

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

// Single-pass route (boxes nest: lod.hip, lod_mark_kernel): cut decision and cull per node, one launch over the N nodes.
__global__ __launch_bounds__(256) void frustum_mark_kernel(const int32_t* __restrict__ nodes,
                                                           const float* __restrict__ boxes,
                                                           const float4* __restrict__ bounds, int N, float tau, Vec3 vp,
                                                           Frustum f, uint32_t* __restrict__ emit_cnt,
                                                           uint32_t* __restrict__ block_sums,
                                                           uint32_t* __restrict__ block_all,
                                                           unsigned long long* __restrict__ chain) {
  clear_scan_chain(chain, block_sums);
  const int n = blockIdx.x * 256 + threadIdx.x;
  uint32_t cnt = 0, kept = 0;
  if (n < N) {
    const int32_t* nd = nodes + (size_t)n * kNodeInts;
    const int par = nd[1];
    const float sn = node_size(boxes, n, vp);
    const bool coarse = sn >= tau;
    const bool reached = coarse || par < 0 || node_size(boxes, par, vp) >= tau;
    cnt = cut_count(reached, coarse, nd);
    kept = (cnt && !entry_culled(bounds, n, par, f)) ? cnt : 0u;
    emit_cnt[n] = kept;
  }
  block_totals<2>({kept, cnt}, {block_sums, block_all});
}

// Level-by-level route: the unculled counts by launch_level_marking (lod.hip), then the cull over the marked nodes
// (emit_cnt: unculled in, kept out) and the workgroup sums
__global__ __launch_bounds__(256) void frustum_cull_kernel(const int32_t* __restrict__ nodes,
                                                           const float4* __restrict__ bounds, int N, Frustum f,
                                                           uint32_t* __restrict__ emit_cnt,
                                                           uint32_t* __restrict__ block_sums,
                                                           uint32_t* __restrict__ block_all,
                                                           unsigned long long* __restrict__ chain) {
  clear_scan_chain(chain, block_sums);
  const int n = blockIdx.x * 256 + threadIdx.x;
  uint32_t cnt = 0, kept = 0;
  if (n < N) {
    cnt = emit_cnt[n];
    if (cnt) {
      kept = entry_culled(bounds, n, nodes[(size_t)n * kNodeInts + 1], f) ? 0u : cnt;
      if (!kept) emit_cnt[n] = 0u;
    }
  }
  block_totals<2>({kept, cnt}, {block_sums, block_all});
}

__global__ __launch_bounds__(1024) void frustum_scan_sums_kernel(uint32_t* __restrict__ sums,
                                                                 const uint32_t* __restrict__ block_all, int n,
                                                                 unsigned long long* __restrict__ chain, int c_off,
                                                                 int chunks) {
  scan_sums_and_unculled_total(sums, block_all, n, chain, c_off, chunks);
}

// lod.hip's emit pass plus, per emitted node, lod_weights_kernel's weight
__global__ __launch_bounds__(256) void frustum_emit_kernel(const int32_t* __restrict__ nodes,
                                                           const float* __restrict__ boxes,
                                                           const uint32_t* __restrict__ emit_cnt, int N, float tau,
                                                           Vec3 vp, const uint32_t* __restrict__ block_sums,
                                                           int32_t* __restrict__ render_indices,
                                                           int32_t* __restrict__ parent_indices,
                                                           int32_t* __restrict__ node_indices,
                                                           float* __restrict__ weights,
                                                           int32_t* __restrict__ num_siblings, int capacity) {
  const int n = blockIdx.x * 256 + threadIdx.x;
  const uint32_t cnt = (n < N) ? emit_cnt[n] : 0u;
  const uint32_t off = block_exclusive_offset(cnt);
  if (cnt == 0) return;
  const int32_t* nd = nodes + (size_t)n * kNodeInts;
  const int start = nd[2];
  const int par = nd[1];
  int pstart = -1;
  float w = 1.0f;
  int kids = 1;
  if (par >= 0) {
    pstart = nodes[(size_t)par * kNodeInts + 2];
    w = interp_weight(node_size(boxes, par, vp), node_size(boxes, n, vp), tau);
    kids = nodes[(size_t)par * kNodeInts + 6];
  }
  write_entries<true>(block_sums[blockIdx.x] + off, cnt, capacity, n, start, pstart, render_indices, parent_indices,
                      node_indices, weights, w, num_siblings, kids);
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
  Carver c(nullptr);
  carve_levels(c, N, true);
  return c.bytes(kAlign);
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
  Carver c(tmp);
  const LevelTmp t = carve_levels(c, N, true);
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
    const int rc = launch_level_marking(nodes, boxes, N, size, vp, t, s);
    if (rc != HGS_OK) return rc;
    hipLaunchKernelGGL(frustum_cull_kernel, dim3(nblk), dim3(256), 0, s, nodes, bnd, N, f, t.emit_cnt, t.block_sums,
                       t.block_all, t.chain);
    HGS_LAUNCH_CHECK("frustum_cull", s, false);
  }
  const int rc = launch_scan_chunks(frustum_scan_sums_kernel, "frustum_scan_sums", nblk, s, t.block_sums, t.block_all,
                                    nblk, t.chain);
  if (rc != HGS_OK) return rc;
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
