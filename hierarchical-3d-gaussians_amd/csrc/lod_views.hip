// Hierarchy cut for several views in one call (opt-in, beside hgs_lod_cut_view of lod_frustum.hip): what the
// single-pass route of that call gives for each of V <= HGS_CUT_MAX_VIEWS views, bit for bit, from ONE pass over the
// nodes and one host wait.
//
// Almost every byte the single-pass cut moves does not depend on the view: the node record, the node's box, the
// parent's box and the culling ball.  Only the viewpoint, the granularity, five planes and a radius scale differ, and
// those are wave-uniform kernel arguments (100 bytes per view, by value).  So the mark pass loads a node once and
// judges it for every view with the very expressions of frustum_mark_kernel (the rules are lod_cut.h's), writes one
// emission count per view and the workgroup's sums per view; the sums of each view are scanned by the chained scan of
// common.h; ONE emit launch (grid: workgroups of nodes x views) writes all views into packed outputs: view v starts
// at the sum of the earlier views' counts, each rounded up to 4 entries, so that every slice starts on 16 bytes.
// The boxes must nest (there is no level-by-level route here).
#include "lod_cut.h"

namespace hgs {
namespace {

constexpr int kMaxViews = HGS_CUT_MAX_VIEWS;

// what differs between views; plain floats so that 16 of them are 1600 bytes of kernel arguments
struct ViewArgs {
  float vp[3];
  float tau;
  float pl[20];
  float rs;
};
struct ViewsArgs { ViewArgs v[kMaxViews]; };
static_assert(sizeof(ViewsArgs) == 1600, "100 bytes per view");

__device__ __forceinline__ Vec3 viewpoint_of(const ViewArgs& a) { return Vec3{a.vp[0], a.vp[1], a.vp[2]}; }
__device__ __forceinline__ Frustum frustum_of(const ViewArgs& a) {
  Frustum f;
#pragma unroll
  for (int k = 0; k < 5; ++k) f.p[k] = make_float4(a.pl[4 * k], a.pl[4 * k + 1], a.pl[4 * k + 2], a.pl[4 * k + 3]);
  f.rs = a.rs;
  return f;
}

// the workgroup sums of view v: every view has a SumsTmp of its own, `stride` bytes after the one before
template <typename T>
__device__ __forceinline__ T* of_view(T* view0, size_t stride, int v) {
  return (T*)((const char*)view0 + stride * (size_t)v);
}

// frustum_mark_kernel for V views: one thread per node, everything that does not depend on the view loaded once.
// kCull false: no planes -- kept = unculled, one sum per view.
template <bool kCull>
__global__ __launch_bounds__(256) void views_mark_kernel(const int32_t* __restrict__ nodes,
                                                         const float* __restrict__ boxes,
                                                         const float4* __restrict__ bounds, int N, int V, ViewsArgs va,
                                                         uint32_t* __restrict__ emit_cnt, size_t cnt_stride,
                                                         uint32_t* __restrict__ block_sums0,
                                                         uint32_t* __restrict__ block_all0,
                                                         unsigned long long* __restrict__ chain0, size_t sums_stride) {
  for (int v = 0; v < V; ++v) {
    if constexpr (kCull) clear_scan_chain(of_view(chain0, sums_stride, v), of_view(block_sums0, sums_stride, v));
    else clear_scan_chain(of_view(chain0, sums_stride, v));
  }
  const int n = blockIdx.x * 256 + threadIdx.x;
  const bool live = n < N;
  int par = -1;
  int32_t leafs = 0, merged = 0;
  float4 mn = make_float4(0.0f, 0.0f, 0.0f, 0.0f), mx = mn, pmn = mn, pmx = mn, bn = mn, bp = mn;
  bool have_bp = false;
  if (live) {
    const int32_t* nd = nodes + (size_t)n * kNodeInts;
    par = nd[1];
    leafs = nd[3];
    merged = nd[4];
    const float4* bx = reinterpret_cast<const float4*>(boxes);
    mn = bx[(size_t)n * 2 + 0];
    mx = bx[(size_t)n * 2 + 1];
    if (par >= 0) {
      pmn = bx[(size_t)par * 2 + 0];
      pmx = bx[(size_t)par * 2 + 1];
    }
    if constexpr (kCull) bn = bounds[n];
  }
  for (int v = 0; v < V; ++v) {
    uint32_t cnt = 0, kept = 0;
    if (live) {
      const Vec3 vp = viewpoint_of(va.v[v]);
      const float tau = va.v[v].tau;
      const float sn = box_size(mn, mx, vp);
      const bool coarse = sn >= tau;
      const bool reached = coarse || par < 0 || box_size(pmn, pmx, vp) >= tau;
      cnt = cut_count(reached, coarse, leafs, merged);
      kept = cnt;
      if constexpr (kCull) {
        if (cnt) {
          const Frustum f = frustum_of(va.v[v]);
          const uint32_t out = planes_outside(bn, f);
          if (out) {
            // the parent's ball: gathered once, and only by a node whose own ball is outside a plane of some view
            if (!have_bp) {
              bp = bounds[par >= 0 ? par : n];
              have_bp = true;
            }
            if (parent_outside_too(out, bp, f)) kept = 0u;
          }
        }
      }
      emit_cnt[(size_t)v * cnt_stride + n] = kept;
    }
    if constexpr (kCull)
      block_totals<2>({kept, cnt}, {of_view(block_sums0, sums_stride, v), of_view(block_all0, sums_stride, v)});
    else
      block_totals<1>({kept}, {of_view(block_sums0, sums_stride, v)});
    __syncthreads();      // block_totals' shared words are read by thread 0 and written again for the next view
  }
}

__global__ __launch_bounds__(1024) void views_scan_cull_kernel(uint32_t* __restrict__ sums,
                                                               const uint32_t* __restrict__ block_all, int n,
                                                               unsigned long long* __restrict__ chain, int c_off,
                                                               int chunks) {
  scan_sums_and_unculled_total(sums, block_all, n, chain, c_off, chunks);
}

__global__ __launch_bounds__(1024) void views_scan_kernel(uint32_t* __restrict__ sums, int n,
                                                          unsigned long long* __restrict__ chain, int c_off,
                                                          int chunks) {
  (void)chained_scan_inplace(sums, n, chain, c_off, chunks);
}

// frustum_emit_kernel for view blockIdx.y, its entries behind those of the views before it: base = the sum of their
// scanned totals, each rounded up to 4 entries (64-bit: a sum past 2^32 must not wrap back into the buffers).  The
// first thread of every view leaves the view's two totals in res[2 v], res[2 v + 1]: one copy brings all of them back.
__global__ __launch_bounds__(256) void views_emit_kernel(const int32_t* __restrict__ nodes,
                                                         const float* __restrict__ boxes,
                                                         const uint32_t* __restrict__ emit_cnt, size_t cnt_stride,
                                                         int N, ViewsArgs va, const uint32_t* __restrict__ block_sums0,
                                                         size_t sums_stride, int cull,
                                                         int32_t* __restrict__ render_indices,
                                                         int32_t* __restrict__ parent_indices,
                                                         int32_t* __restrict__ node_indices,
                                                         float* __restrict__ weights,
                                                         int32_t* __restrict__ num_siblings, int capacity,
                                                         uint32_t* __restrict__ res) {
  const int v = blockIdx.y;
  const int nblk = gridDim.x;
  const uint32_t* block_sums = of_view(block_sums0, sums_stride, v);
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    res[2 * v + 0] = block_sums[nblk];
    res[2 * v + 1] = block_sums[cull ? nblk + 1 : nblk];
  }
  const uint32_t first = block_sums[blockIdx.x];
  if (first == block_sums[blockIdx.x + 1]) return;        // nothing to emit here ([nblk] = the total): no loads
  unsigned long long base = 0ull;
  for (int u = 0; u < v; ++u)
    base += ((unsigned long long)of_view(block_sums0, sums_stride, u)[nblk] + 3ull) & ~3ull;
  const int n = blockIdx.x * 256 + threadIdx.x;
  const uint32_t cnt = (n < N) ? emit_cnt[(size_t)v * cnt_stride + n] : 0u;
  const uint32_t off = block_exclusive_offset(cnt);
  if (cnt == 0) return;
  const unsigned long long pos = base + (unsigned long long)first + (unsigned long long)off;
  if (pos >= (unsigned long long)capacity) return;        // (so pos fits the 32 bits write_entries counts in)
  const Vec3 vp = viewpoint_of(va.v[v]);
  const float tau = va.v[v].tau;
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
  write_entries<true>((uint32_t)pos, cnt, capacity, n, start, pstart, render_indices, parent_indices, node_indices,
                      weights, w, num_siblings, kids);
}

struct ViewsTmp {
  uint32_t* emit_cnt;    // [V][n] emission counts, view by view
  size_t cnt_stride;     // n
  SumsTmp sums0;         // view 0's workgroup sums; view v's lie sums_stride bytes * v further on
  size_t sums_stride;
  uint32_t* res;         // [2 * kMaxViews] kept and unculled total of every view: what the host reads
};

inline int clamp_views(int32_t V) { return V < 1 ? 1 : (V > kMaxViews ? kMaxViews : V); }

inline ViewsTmp carve_views(Carver& c, int32_t N, int32_t V) {
  const size_t n = (size_t)(N > 0 ? N : 1);
  const int views = clamp_views(V);
  ViewsTmp t;
  t.emit_cnt = c.take<uint32_t>((size_t)views * n);
  t.cnt_stride = n;
  const size_t before = c.offset;
  t.sums0 = carve_sums(c, n, true);
  t.sums_stride = c.offset - before;
  for (int v = 1; v < views; ++v) (void)carve_sums(c, n, true);
  t.res = c.take<uint32_t>(2 * kMaxViews);
  return t;
}

}  // namespace
}  // namespace hgs

using namespace hgs;

extern "C" {

// (V outside [1, HGS_CUT_MAX_VIEWS] is answered as the nearest valid V: a size query has no error to return)
size_t hgs_lod_cut_views_tmp_bytes(int32_t N, int32_t V) {
  Carver c(nullptr);
  carve_views(c, N, V);
  return c.bytes(kAlign);
}

int hgs_lod_cut_views(const int32_t* nodes, const float* boxes, const float* bounds, int32_t N, int32_t V,
                      const float* sizes, const float* viewpoints, const float* planes, const float* radius_scales,
                      int32_t* render_indices, int32_t* parent_indices, int32_t* nodes_for_render_indices,
                      float* weights, int32_t* num_siblings, int32_t capacity, void* tmp, int32_t* counts_out_host,
                      int32_t* unculled_out_host, int32_t* offsets_out_host, int64_t* needed_out_host,
                      hgs_stream_t stream, int device) {
  if (V < 1 || V > kMaxViews) {
    set_error("lod_cut_views: V = %d views, one call takes 1 to %d", V, kMaxViews);
    return HGS_ERR_INVALID;
  }
  if (!counts_out_host || !unculled_out_host || !offsets_out_host || !needed_out_host) {
    set_error("lod_cut_views: null result pointer");
    return HGS_ERR_INVALID;
  }
  for (int v = 0; v < V; ++v) counts_out_host[v] = unculled_out_host[v] = offsets_out_host[v] = 0;
  *needed_out_host = 0;
  if (N <= 0) return HGS_OK;
  if (!nodes || !boxes || !sizes || !viewpoints || !radius_scales || !render_indices || !parent_indices ||
      !nodes_for_render_indices || !weights || !num_siblings || !tmp) {
    set_error("lod_cut_views: null argument");
    return HGS_ERR_INVALID;
  }
  if ((bounds == nullptr) != (planes == nullptr)) {
    set_error("lod_cut_views: bounds and planes go together (both or neither)");
    return HGS_ERR_INVALID;
  }
  if (capacity < 0) { set_error("lod_cut_views: capacity = %d", capacity); return HGS_ERR_INVALID; }
  HGS_HIP(hipSetDevice(device));
  hipStream_t s = static_cast<hipStream_t>(stream);
  Carver c(tmp);
  const ViewsTmp t = carve_views(c, N, V);
  const bool cull = bounds != nullptr;
  ViewsArgs va;
  for (int v = 0; v < kMaxViews; ++v) {
    const int u = v < V ? v : 0;              // (the unused slots repeat view 0: no uninitialised kernel arguments)
    ViewArgs& a = va.v[v];
    for (int k = 0; k < 3; ++k) a.vp[k] = viewpoints[3 * u + k];
    a.tau = sizes[u];
    for (int k = 0; k < 20; ++k) a.pl[k] = cull ? planes[20 * u + k] : 0.0f;
    a.rs = radius_scales[u];
  }
  const int nblk = (N + 255) / 256;
  const SumsTmp& s0 = t.sums0;
  if (cull) {
    hipLaunchKernelGGL(views_mark_kernel<true>, dim3(nblk), dim3(256), 0, s, nodes, boxes,
                       reinterpret_cast<const float4*>(bounds), N, V, va, t.emit_cnt, t.cnt_stride, s0.block_sums,
                       s0.block_all, s0.chain, t.sums_stride);
  } else {
    hipLaunchKernelGGL(views_mark_kernel<false>, dim3(nblk), dim3(256), 0, s, nodes, boxes,
                       static_cast<const float4*>(nullptr), N, V, va, t.emit_cnt, t.cnt_stride, s0.block_sums,
                       s0.block_all, s0.chain, t.sums_stride);
  }
  HGS_LAUNCH_CHECK("views_mark", s, false);
  for (int v = 0; v < V; ++v) {
    const size_t shift = t.sums_stride * (size_t)v;
    uint32_t* sums = reinterpret_cast<uint32_t*>(reinterpret_cast<char*>(s0.block_sums) + shift);
    const uint32_t* all = reinterpret_cast<const uint32_t*>(reinterpret_cast<char*>(s0.block_all) + shift);
    unsigned long long* chain = reinterpret_cast<unsigned long long*>(reinterpret_cast<char*>(s0.chain) + shift);
    const int rc = cull ? launch_scan_chunks(views_scan_cull_kernel, "views_scan_cull", nblk, s, sums, all, nblk,
                                             chain)
                        : launch_scan_chunks(views_scan_kernel, "views_scan", nblk, s, sums, nblk, chain);
    if (rc != HGS_OK) return rc;
  }
  // (a grid over the nodes, not over the entries: empty cuts launch nothing of size zero)
  hipLaunchKernelGGL(views_emit_kernel, dim3(nblk, V), dim3(256), 0, s, nodes, boxes, t.emit_cnt, t.cnt_stride, N, va,
                     s0.block_sums, t.sums_stride, cull ? 1 : 0, render_indices, parent_indices,
                     nodes_for_render_indices, weights, num_siblings, capacity, t.res);
  HGS_LAUNCH_CHECK("views_emit", s, false);
  uint32_t res[2 * kMaxViews] = {};           // (kept, unculled) of every view: neighbours, one copy
  HGS_HIP(hipMemcpyAsync(res, t.res, (size_t)V * 8, hipMemcpyDeviceToHost, s));
  HGS_HIP(wait_stream(s));
  const unsigned long long int_max = 0x7FFFFFFFull;
  unsigned long long offset = 0ull, needed = 0ull;
  for (int v = 0; v < V; ++v) {
    const unsigned long long kept = res[2 * v];
    counts_out_host[v] = (int32_t)(kept < int_max ? kept : int_max);
    unculled_out_host[v] = (int32_t)(res[2 * v + 1] < int_max ? res[2 * v + 1] : int_max);
    offsets_out_host[v] = (int32_t)(offset < int_max ? offset : int_max);
    needed = offset + kept;
    offset += (kept + 3ull) & ~3ull;
  }
  *needed_out_host = (int64_t)needed;
  if (needed > int_max) {
    set_error("lod_cut_views: %llu entries are more than the 2^31 - 1 one set of outputs can index", needed);
    return HGS_ERR_INVALID;
  }
  if (needed > (unsigned long long)capacity) {
    set_error("lod_cut_views: %llu entries exceed the output capacity %d", needed, capacity);
    return HGS_ERR_INVALID;
  }
  return HGS_OK;
}

}  // extern "C"
