// K9 (expand_to_size) and K10 (get_interpolation_weights): the per-view hierarchy LOD cut.
//
// Replaces gaussian_hierarchy._C.expand_to_size / get_interpolation_weights
// (train_post.py:91-113, render_hierarchy.py:58-80; the reference checkout does not vendor the submodule that
// implements them -- semantics restated in include/hgs.h, oracle/lod_oracle.py and DESIGN.md section 4).
// Top-down frontier expansion: work is
// proportional to the nodes ABOVE the cut, not to the hierarchy size; the only
// full-size pass is the flag compaction (4 B per node), which also makes the output
// order deterministic (ascending node index) despite the atomic frontier appends.
#include "lod_cut.h"

namespace hgs {
namespace {

__global__ void lod_init_kernel(uint32_t* counts, int32_t* frontier, int N) {
  if (threadIdx.x == 0) {
    counts[0] = N > 0 ? 1u : 0u;
    frontier[0] = 0;
  }
}

__global__ __launch_bounds__(256) void lod_expand_level_kernel(const int32_t* __restrict__ nodes,
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
    const bool coarse = node_size(boxes, n, vp) >= tau;
    emit_cnt[n] = cut_count(true, coarse, nd);      // (on the frontier: its parent was too coarse)
    if (coarse && nch > 0) {                        // the children are next
      const uint32_t base = atomicAdd(count_out, (uint32_t)nch);
      const int c0 = nd[5];
      for (int k = 0; k < nch; ++k) fout[base + k] = c0 + k;
    }
  }
}

// Single-pass cut for hierarchies whose boxes NEST (child AABB inside the parent's, child extent <= parent extent --
// checked once per hierarchy by lod_nested_kernel): then size(parent) >= size(child) from every viewpoint, "all
// ancestors are too coarse" collapses to "the parent is too coarse", and every node decides for itself -- one launch
// over the N nodes instead of one launch per tree level (24 levels x ~8 us at 1 M nodes).
__global__ __launch_bounds__(256) void lod_mark_kernel(const int32_t* __restrict__ nodes, const float* __restrict__ boxes,
                                                       int N, float tau, Vec3 vp, uint32_t* __restrict__ emit_cnt,
                                                       uint32_t* __restrict__ block_sums,
                                                       unsigned long long* __restrict__ chain) {
  clear_scan_chain(chain);
  const int n = blockIdx.x * 256 + threadIdx.x;
  uint32_t cnt = 0;
  if (n < N) {
    const int32_t* nd = nodes + (size_t)n * kNodeInts;
    const int par = nd[1];
    // size(parent) >= size(n) in float32 too when the boxes nest (smaller numerator, larger denominator, every
    // operation of node_size monotone under rounding): a node that is too coarse itself has been reached, and its
    // parent's box -- a second 32-byte gather -- is only read for the nodes that are fine enough
    const float sn = node_size(boxes, n, vp);
    const bool coarse = sn >= tau;
    const bool reached = coarse || par < 0 || node_size(boxes, par, vp) >= tau;
    cnt = cut_count(reached, coarse, nd);
    emit_cnt[n] = cnt;
  }
  block_totals<1>({cnt}, {block_sums});
}

// flag[0] = 1 if some node's box is not inside its parent's or has a larger extent (view independent)
__global__ __launch_bounds__(256) void lod_nested_kernel(const int32_t* __restrict__ nodes, const float* __restrict__ boxes,
                                                         int N, uint32_t* __restrict__ flag) {
  const int n = blockIdx.x * 256 + threadIdx.x;
  if (n >= N) return;
  const int par = nodes[(size_t)n * kNodeInts + 1];
  if (par < 0) return;
  if (par >= N) { *flag = 1u; return; }
  const float4 cmn = reinterpret_cast<const float4*>(boxes)[(size_t)n * 2 + 0];
  const float4 cmx = reinterpret_cast<const float4*>(boxes)[(size_t)n * 2 + 1];
  const float4 pmn = reinterpret_cast<const float4*>(boxes)[(size_t)par * 2 + 0];
  const float4 pmx = reinterpret_cast<const float4*>(boxes)[(size_t)par * 2 + 1];
  const bool ok = cmn.x >= pmn.x && cmn.y >= pmn.y && cmn.z >= pmn.z && cmx.x <= pmx.x && cmx.y <= pmx.y &&
                  cmx.z <= pmx.z && cmn.w <= pmn.w && cmn.x <= cmx.x && cmn.y <= cmx.y && cmn.z <= cmx.z;
  if (!ok) *flag = 1u;      // benign race: every writer stores 1 (NaNs fail the comparisons and land here too)
}

// per-workgroup sums of emit_cnt (256 nodes per workgroup)
__global__ __launch_bounds__(256) void lod_block_sums_kernel(const uint32_t* __restrict__ emit_cnt, int N,
                                                             uint32_t* __restrict__ block_sums,
                                                             unsigned long long* __restrict__ chain) {
  clear_scan_chain(chain);
  const int i = blockIdx.x * 256 + threadIdx.x;
  block_totals<1>({(i < N) ? emit_cnt[i] : 0u}, {block_sums});
}

__global__ __launch_bounds__(1024) void lod_scan_sums_kernel(uint32_t* __restrict__ sums, int n,
                                                             unsigned long long* __restrict__ chain, int c_off,
                                                             int chunks) {
  (void)chained_scan_inplace(sums, n, chain, c_off, chunks);
}

__global__ __launch_bounds__(256) void lod_emit_kernel(const int32_t* __restrict__ nodes,
                                                       const uint32_t* __restrict__ emit_cnt, int N,
                                                       const uint32_t* __restrict__ block_sums,
                                                       int32_t* __restrict__ render_indices,
                                                       int32_t* __restrict__ parent_indices,
                                                       int32_t* __restrict__ node_indices, int capacity) {
  const int n = blockIdx.x * 256 + threadIdx.x;
  const uint32_t cnt = (n < N) ? emit_cnt[n] : 0u;
  const uint32_t off = block_exclusive_offset(cnt);
  if (cnt == 0) return;
  const int32_t* nd = nodes + (size_t)n * kNodeInts;
  const int start = nd[2];
  const int par = nd[1];
  const int pstart = par >= 0 ? nodes[(size_t)par * kNodeInts + 2] : -1;
  write_entries<false>(block_sums[blockIdx.x] + off, cnt, capacity, n, start, pstart, render_indices, parent_indices,
                       node_indices);
}

__global__ __launch_bounds__(256) void lod_weights_kernel(const int32_t* __restrict__ node_indices, int n, float tau,
                                                          const int32_t* __restrict__ nodes,
                                                          const float* __restrict__ boxes, Vec3 vp,
                                                          float* __restrict__ weights,
                                                          int32_t* __restrict__ num_siblings) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int nd = node_indices[i];
  const int par = nodes[(size_t)nd * kNodeInts + 1];
  float w = 1.0f;
  int kids = 1;
  if (par >= 0) {
    w = interp_weight(node_size(boxes, par, vp), node_size(boxes, nd, vp), tau);
    kids = nodes[(size_t)par * kNodeInts + 6];
  }
  weights[i] = w;
  num_siblings[i] = kids;
}

}  // namespace

int launch_level_marking(const int32_t* nodes, const float* boxes, int32_t N, float tau, Vec3 vp, const LevelTmp& t,
                         hipStream_t s) {
  HGS_HIP(hipMemsetAsync(t.emit_cnt, 0, (size_t)N * 4, s));
  HGS_HIP(hipMemsetAsync(t.counts, 0, kCountWords * 4, s));
  hipLaunchKernelGGL(lod_init_kernel, dim3(1), dim3(64), 0, s, t.counts, t.frontier_a, N);
  HGS_LAUNCH_CHECK("lod_init", s, false);
  // Level-synchronous expansion.  The frontier size of a level is only known on the device, so
  // every level is launched with a grid-stride kernel; the host polls the level counters every
  // 8 levels to stop early (a hierarchy deeper than kMaxLevels is rejected).
  int32_t* fin = t.frontier_a;
  int32_t* fout = t.frontier_b;
  const int grid = 1024;
  int level = 0;
  bool finished = false;
  while (!finished) {
    const int stop = level + 8;
    for (; level < stop && level < kMaxLevels; ++level) {
      hipLaunchKernelGGL(lod_expand_level_kernel, dim3(grid), dim3(256), 0, s, nodes, boxes, tau, vp, fin,
                         t.counts + level, fout, t.counts + level + 1, t.emit_cnt);
      HGS_LAUNCH_CHECK("lod_expand_level", s, false);
      int32_t* sw = fin; fin = fout; fout = sw;
    }
    uint32_t next = 0;
    HGS_HIP(hipMemcpyAsync(&next, t.counts + level, 4, hipMemcpyDeviceToHost, s));
    HGS_HIP(wait_stream(s));
    if (next == 0) finished = true;
    else if (level >= kMaxLevels) { set_error("hierarchy deeper than %d levels", kMaxLevels); return HGS_ERR_INVALID; }
  }
  return HGS_OK;
}

}  // namespace hgs

using namespace hgs;

extern "C" {

size_t hgs_expand_tmp_bytes(int32_t N) {
  Carver c(nullptr);
  carve_levels(c, N, false);
  return c.bytes(kAlign);
}

static int expand_finish(const int32_t* nodes, const LevelTmp& t, int32_t N, int32_t* render_indices,
                         int32_t* parent_indices, int32_t* nodes_for_render_indices, int32_t capacity,
                         int32_t* count_out_host, hipStream_t s) {
  const int nblk = (N + 255) / 256;
  const int rc = launch_scan_chunks(lod_scan_sums_kernel, "lod_scan_sums", nblk, s, t.block_sums, nblk, t.chain);
  if (rc != HGS_OK) return rc;
  hipLaunchKernelGGL(lod_emit_kernel, dim3(nblk), dim3(256), 0, s, nodes, t.emit_cnt, N, t.block_sums,
                     render_indices, parent_indices, nodes_for_render_indices, capacity);
  HGS_LAUNCH_CHECK("lod_emit", s, false);
  uint32_t total = 0;
  HGS_HIP(hipMemcpyAsync(&total, t.block_sums + nblk, 4, hipMemcpyDeviceToHost, s));
  HGS_HIP(wait_stream(s));
  if (total > (uint32_t)capacity) {
    set_error("expand_to_size: %u entries exceed the output capacity %d", total, capacity);
    return HGS_ERR_INVALID;
  }
  *count_out_host = (int32_t)total;
  return HGS_OK;
}

int hgs_expand_to_size(const int32_t* nodes, const float* boxes, int32_t N, float size, const float viewpoint[3],
                       const float viewdir[3], int32_t* render_indices, int32_t* parent_indices,
                       int32_t* nodes_for_render_indices, int32_t capacity, void* tmp, int32_t* count_out_host,
                       hgs_stream_t stream, int device) {
  (void)viewdir;  // always zeros at the reference's call sites (train_post.py:96, render_hierarchy.py:63)
  if (!count_out_host) { set_error("null count_out_host"); return HGS_ERR_INVALID; }
  *count_out_host = 0;
  if (N <= 0) return HGS_OK;
  if (!nodes || !boxes || !viewpoint || !render_indices || !parent_indices || !nodes_for_render_indices || !tmp) {
    set_error("null argument");
    return HGS_ERR_INVALID;
  }
  HGS_HIP(hipSetDevice(device));
  hipStream_t s = static_cast<hipStream_t>(stream);
  Carver c(tmp);
  const LevelTmp t = carve_levels(c, N, false);
  const Vec3 vp = {viewpoint[0], viewpoint[1], viewpoint[2]};
  const int rc = launch_level_marking(nodes, boxes, N, size, vp, t, s);
  if (rc != HGS_OK) return rc;
  const int nblk = (N + 255) / 256;
  hipLaunchKernelGGL(lod_block_sums_kernel, dim3(nblk), dim3(256), 0, s, t.emit_cnt, N, t.block_sums, t.chain);
  HGS_LAUNCH_CHECK("lod_block_sums", s, false);
  return expand_finish(nodes, t, N, render_indices, parent_indices, nodes_for_render_indices, capacity, count_out_host, s);
}

int hgs_expand_to_size_nested(const int32_t* nodes, const float* boxes, int32_t N, float size, const float viewpoint[3],
                              const float viewdir[3], int32_t* render_indices, int32_t* parent_indices,
                              int32_t* nodes_for_render_indices, int32_t capacity, void* tmp, int32_t* count_out_host,
                              hgs_stream_t stream, int device) {
  (void)viewdir;
  if (!count_out_host) { set_error("null count_out_host"); return HGS_ERR_INVALID; }
  *count_out_host = 0;
  if (N <= 0) return HGS_OK;
  if (!nodes || !boxes || !viewpoint || !render_indices || !parent_indices || !nodes_for_render_indices || !tmp) {
    set_error("null argument");
    return HGS_ERR_INVALID;
  }
  HGS_HIP(hipSetDevice(device));
  hipStream_t s = static_cast<hipStream_t>(stream);
  Carver c(tmp);
  const LevelTmp t = carve_levels(c, N, false);
  const Vec3 vp = {viewpoint[0], viewpoint[1], viewpoint[2]};
  hipLaunchKernelGGL(lod_mark_kernel, dim3((N + 255) / 256), dim3(256), 0, s, nodes, boxes, N, size, vp, t.emit_cnt,
                     t.block_sums, t.chain);
  HGS_LAUNCH_CHECK("lod_mark", s, false);
  return expand_finish(nodes, t, N, render_indices, parent_indices, nodes_for_render_indices, capacity, count_out_host, s);
}

int hgs_hier_boxes_nested(const int32_t* nodes, const float* boxes, int32_t N, void* tmp, int32_t* nested_out_host,
                          hgs_stream_t stream, int device) {
  if (!nested_out_host) { set_error("null nested_out_host"); return HGS_ERR_INVALID; }
  *nested_out_host = 1;
  if (N <= 0) return HGS_OK;
  if (!nodes || !boxes || !tmp) { set_error("null argument"); return HGS_ERR_INVALID; }
  HGS_HIP(hipSetDevice(device));
  hipStream_t s = static_cast<hipStream_t>(stream);
  uint32_t* flag = static_cast<uint32_t*>(tmp);
  HGS_HIP(hipMemsetAsync(flag, 0, 4, s));
  hipLaunchKernelGGL(lod_nested_kernel, dim3((N + 255) / 256), dim3(256), 0, s, nodes, boxes, N, flag);
  HGS_LAUNCH_CHECK("lod_nested", s, false);
  uint32_t bad = 0;
  HGS_HIP(hipMemcpyAsync(&bad, flag, 4, hipMemcpyDeviceToHost, s));
  HGS_HIP(wait_stream(s));
  *nested_out_host = bad ? 0 : 1;
  return HGS_OK;
}

int hgs_interp_weights(const int32_t* node_indices, int32_t n, float size, const int32_t* nodes, const float* boxes,
                       int32_t N, const float viewpoint[3], const float viewdir[3], float* interpolation_weights,
                       int32_t* num_siblings, hgs_stream_t stream, int device) {
  (void)viewdir; (void)N;
  if (n <= 0) return HGS_OK;
  if (!node_indices || !nodes || !boxes || !viewpoint || !interpolation_weights || !num_siblings) {
    set_error("null argument");
    return HGS_ERR_INVALID;
  }
  HGS_HIP(hipSetDevice(device));
  hipStream_t s = static_cast<hipStream_t>(stream);
  const Vec3 vp = {viewpoint[0], viewpoint[1], viewpoint[2]};
  hipLaunchKernelGGL(lod_weights_kernel, dim3((n + 255) / 256), dim3(256), 0, s, node_indices, n, size, nodes, boxes,
                     vp, interpolation_weights, num_siblings);
  HGS_LAUNCH_CHECK("lod_weights", s, false);
  return HGS_OK;
}

}  // extern "C"
