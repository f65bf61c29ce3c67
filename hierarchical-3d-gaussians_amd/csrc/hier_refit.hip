// Refitting a hierarchy's boxes: the rule of hgs.hierarchy.refit_boxes (the spec) on the device.
//
//   rule       only boxes change.  A leaf (count_children == 0) keeps its box, or takes the cube / the ellipsoid box of
//              its own row (hier_refit_rule.h); a node with children takes the union of its children's FINAL boxes, its
//              own Gaussian not included (the builder's and the merger's rule); every written box gets the extent of
//              its rounded coordinates, boxes[n,1,3] is copied.  Children before parents.
//   plan       hr_plan_kernel: one thread per node (a capped grid walks the nodes) runs the three layout checks
//              (node_layout of hier_nodes.h) and the depth checks of the aligner (restated here: hier_align.hip is not
//              touched), evaluates a leaf's box into registers for the test it has to pass (nothing is stored), writes
//              the depth as a sort key, counts the nodes per depth (LDS bins per workgroup), the leaves and the sum of
//              count_children; sort_pairs32 (8 bits, stable) turns the keys into the level lists, ascending ids inside
//              a level; ONE host wait reads the counts and the checks.  Nothing has been written to boxes_out then.
//   apply      asynchronous.  hr_leaf_kernel: one thread per node, the leaves write (or, kept and out of place, copy)
//              their boxes; then hr_level_kernel, one launch per depth from the deepest level with children up to 0:
//              one thread per node of the level list reads its children's boxes as two float4 each -- contiguous
//              children, neighbouring lanes on neighbouring ids: the reads coalesce without LDS -- and writes its own.
//
// Every index followed has passed the checks: a children range lies in [1, N), every node lies in the range of its own
// parent and the ranges hold N - 1 slots in all, so each range is exactly the node's children, one level down.  A single
// thread walks a wide node (the merged root).  In place (boxes_out == boxes) or out of place (no overlap).
#include "hier_nodes.h"
#include "hier_refit_rule.h"

#pragma clang fp contract(off)

namespace hgs {
namespace {

constexpr int kHrThreads = 256;
constexpr int kMaxDepth = 255;
constexpr int kLevels = kMaxDepth + 1;
constexpr int kHrChecks = 7;
constexpr int kHrPlanBlocks = 2048;   // 8 workgroups of 256 threads on each of 256 compute units: the plan's grid at most

// Device half of the report, read back with the level counts in one copy.
struct HrResult {
  uint32_t counts[kLevels];          // nodes per depth (one with a depth outside [0, 255] is not counted)
  uint32_t leaves;
  uint32_t pad;
  unsigned long long children_sum;   // over the nodes whose children range passed its check
  uint32_t minima[kHrChecks + 1];    // unsigned minima, kNone = none: the checks in the report's order ([5] = the second
                                     // smallest node of depth 0), [7] = the smallest node of depth 0
};
constexpr size_t kHrZeroBytes = offsetof(HrResult, minima);

struct LeafBox { float lo[3], hi[3]; };

// A leaf's box by `mode`, from its row (or, kept, from the input box).
__device__ __forceinline__ LeafBox hr_leaf_box(int64_t i, int32_t mode, const float* __restrict__ xyz,
                                               const float* __restrict__ log_scales, const float* __restrict__ rots,
                                               const float* boxes) {
  LeafBox b;
  if (mode == kRefitKeep) {
    const float4 mn = reinterpret_cast<const float4*>(boxes)[i * 2 + 0];
    const float4 mx = reinterpret_cast<const float4*>(boxes)[i * 2 + 1];
    b.lo[0] = mn.x; b.lo[1] = mn.y; b.lo[2] = mn.z;
    b.hi[0] = mx.x; b.hi[1] = mx.y; b.hi[2] = mx.z;
    return b;
  }
  const double x[3] = {xyz[i * 3 + 0], xyz[i * 3 + 1], xyz[i * 3 + 2]};
  const double ls[3] = {log_scales[i * 3 + 0], log_scales[i * 3 + 1], log_scales[i * 3 + 2]};
  if (mode == kRefitCube) {
    refit_leaf_cube(x, ls, b.lo, b.hi);
  } else {
    const float4 qf = reinterpret_cast<const float4*>(rots)[i];
    const double q[4] = {qf.x, qf.y, qf.z, qf.w};
    refit_leaf_ellipsoid(x, ls, q, b.lo, b.hi);
  }
  return b;
}

// One thread per node, kHrPlanBlocks workgroups at most that walk the nodes in strides: the checks, the depth as the sort
// key, the per-depth counts, the leaf count, the children sum.  The sums are kept in registers and LDS over the whole
// walk and reach the global words once per workgroup, and a wave whose nodes share a depth -- nearly every wave of a BFS
// numbering -- counts them with one LDS atomic (with one workgroup per 256 nodes, each flushing its sums and every lane
// adding to its LDS bin, this kernel took 3.1 ms at 50 M nodes; 0.9 ms this way).
__global__ __launch_bounds__(kHrThreads) void hr_plan_kernel(const int32_t* __restrict__ nodes,
                                                             const float* __restrict__ xyz,
                                                             const float* __restrict__ log_scales,
                                                             const float* __restrict__ rots,
                                                             const float* __restrict__ boxes, int32_t N, int32_t mode,
                                                             uint32_t* __restrict__ keys, HrResult* __restrict__ res) {
  __shared__ uint32_t bins[kLevels];
  __shared__ uint32_t s_leaves;
  __shared__ unsigned long long s_children;
  bins[threadIdx.x] = 0;            // kHrThreads == kLevels
  if (threadIdx.x == 0) { s_leaves = 0; s_children = 0; }
  __syncthreads();
  const int lane = threadIdx.x & 63;
  unsigned long long children = 0;
  uint32_t leaves = 0;
  for (int64_t base = (int64_t)blockIdx.x * kHrThreads; base < N; base += (int64_t)gridDim.x * kHrThreads) {
    const int64_t i = base + threadIdx.x;
    uint32_t key = 0;
    bool counted = false;
    if (i < N) {
      const int32_t* nd = nodes + i * kNodeInts;
      const int32_t depth = nd[0], parent = nd[1];
      const int64_t cc = nd[6];
      // ---- the three layout checks
      const uint32_t v = node_layout(nodes, i, N);
      if (v & kBadRow) atomicMin(&res->minima[0], (uint32_t)i);
      if (v & kBadChildren) atomicMin(&res->minima[1], (uint32_t)i);
      if (v & kBadParent) atomicMin(&res->minima[2], (uint32_t)i);
      if (!(v & kBadChildren)) children += (unsigned long long)cc;
      // ---- the depth checks
      const bool bad_depth = depth < 0 || depth > kMaxDepth;
      if (bad_depth) atomicMin(&res->minima[3], (uint32_t)i);
      if (depth != 0) {
        if (parent < 0 || parent >= N || nodes[(int64_t)parent * kNodeInts] != depth - 1) atomicMin(&res->minima[4], (uint32_t)i);
      } else {
        // the two smallest nodes of depth 0: the second one is the smallest max(a, b) over pairs of them, and the pair
        // of the two smallest meets here whichever of them arrives first
        const uint32_t old = atomicMin(&res->minima[7], (uint32_t)i);
        if (old != kNone) atomicMin(&res->minima[5], max(old, (uint32_t)i));
      }
      // ---- a leaf: its box, for the test alone
      if (cc == 0) {
        ++leaves;
        const LeafBox b = hr_leaf_box(i, mode, xyz, log_scales, rots, boxes);
        if (!refit_box_ok(b.lo, b.hi)) atomicMin(&res->minima[6], (uint32_t)i);
      }
      key = bad_depth ? 0u : (uint32_t)depth;
      keys[i] = key;
      counted = !bad_depth;
    }
    // ---- the per-depth count (every lane of the workgroup is here: the trip count is the workgroup's)
    const unsigned long long m = __ballot(counted);
    if (m) {
      const int first = __ffsll((long long)m) - 1;
      const uint32_t k0 = __shfl(key, first);
      if (__ballot(counted && key != k0) == 0) {
        if (lane == first) atomicAdd(&bins[k0], (uint32_t)__popcll(m));
      } else if (counted) {
        atomicAdd(&bins[key], 1u);
      }
    }
  }
  for (int o = 32; o > 0; o >>= 1) {
    children += __shfl_down(children, o);
    leaves += __shfl_down(leaves, o);
  }
  if (lane == 0) {
    if (children) atomicAdd(&s_children, children);
    if (leaves) atomicAdd(&s_leaves, leaves);
  }
  __syncthreads();
  const uint32_t c = bins[threadIdx.x];
  if (c) atomicAdd(&res->counts[threadIdx.x], c);
  if (threadIdx.x == 0) {
    if (s_leaves) atomicAdd(&res->leaves, s_leaves);
    if (s_children) atomicAdd(&res->children_sum, s_children);
  }
}
static_assert(kHrThreads == kLevels, "one thread per depth bin");

// One thread per node: a leaf writes its box (kept: copies it; the launch is skipped in place).
__global__ __launch_bounds__(kHrThreads) void hr_leaf_kernel(const int32_t* __restrict__ nodes,
                                                             const float* __restrict__ xyz,
                                                             const float* __restrict__ log_scales,
                                                             const float* __restrict__ rots, const float* boxes,
                                                             float* boxes_out, int32_t N, int32_t mode) {
  const int64_t i = (int64_t)blockIdx.x * kHrThreads + threadIdx.x;
  if (i >= N || nodes[i * kNodeInts + 6] != 0) return;
  if (mode == kRefitKeep) {
    const float4 mn = reinterpret_cast<const float4*>(boxes)[i * 2 + 0];
    const float4 mx = reinterpret_cast<const float4*>(boxes)[i * 2 + 1];
    reinterpret_cast<float4*>(boxes_out)[i * 2 + 0] = mn;
    reinterpret_cast<float4*>(boxes_out)[i * 2 + 1] = mx;
    return;
  }
  const float own = boxes[i * 8 + 7];      // boxes[n,1,3]: copied
  const LeafBox b = hr_leaf_box(i, mode, xyz, log_scales, rots, boxes);
  reinterpret_cast<float4*>(boxes_out)[i * 2 + 0] = make_float4(b.lo[0], b.lo[1], b.lo[2], refit_extent(b.lo, b.hi));
  reinterpret_cast<float4*>(boxes_out)[i * 2 + 1] = make_float4(b.hi[0], b.hi[1], b.hi[2], own);
}

// One thread per node of one depth: the union of its children's boxes.  `level` = this depth's slice of the depth-sorted
// node ids; the children were written by the leaf pass or by the previous launch.
__global__ __launch_bounds__(kHrThreads) void hr_level_kernel(const uint32_t* __restrict__ level, int32_t count,
                                                              const int32_t* __restrict__ nodes, const float* boxes,
                                                              float* boxes_out) {
  const int32_t t = (int32_t)(blockIdx.x * kHrThreads + threadIdx.x);
  if (t >= count) return;
  const int64_t id = level[t];
  const int64_t sc = nodes[id * kNodeInts + 5];
  const int32_t cc = nodes[id * kNodeInts + 6];
  if (cc <= 0) return;
  const float4* kids = reinterpret_cast<const float4*>(boxes_out) + sc * 2;
  float4 mn = kids[0], mx = kids[1];
  float lo[3] = {mn.x, mn.y, mn.z}, hi[3] = {mx.x, mx.y, mx.z};
  for (int32_t c = 1; c < cc; ++c) {
    mn = kids[2 * c];
    mx = kids[2 * c + 1];
    const float clo[3] = {mn.x, mn.y, mn.z}, chi[3] = {mx.x, mx.y, mx.z};
    refit_union(lo, hi, clo, chi);
  }
  const float own = reinterpret_cast<const float4*>(boxes)[id * 2 + 1].w;
  reinterpret_cast<float4*>(boxes_out)[id * 2 + 0] = make_float4(lo[0], lo[1], lo[2], refit_extent(lo, hi));
  reinterpret_cast<float4*>(boxes_out)[id * 2 + 1] = make_float4(hi[0], hi[1], hi[2], own);
}

struct HrTmp {
  HrResult* res;
  uint32_t* keys;
  uint32_t* keys_sorted;
  uint32_t* order;
  void* sort_tmp;
};

HrTmp carve_hr_tmp(Carver& c, int64_t N) {
  HrTmp t;
  t.res = c.take<HrResult>(1);
  t.keys = c.take<uint32_t>((size_t)N);
  t.keys_sorted = c.take<uint32_t>((size_t)N);
  t.order = c.take<uint32_t>((size_t)N);
  t.sort_tmp = c.take<char>(sort_tmp_bytes((uint32_t)N));   // nested: the sort's own slack included
  return t;
}

}  // namespace

size_t hier_refit_tmp_bytes(int64_t N) {
  Carver c(nullptr);
  carve_hr_tmp(c, N);
  return c.bytes(0);   // tmp is required to be kAlign-aligned: no slack
}

int launch_hier_refit(const hgs_hier_view& in, float* boxes_out, int32_t mode, void* tmp, hgs_hier_refit_report* report,
                      hipStream_t s) {
  const int64_t N = in.N;
  Carver c(tmp);
  const HrTmp t = carve_hr_tmp(c, N);
  // ---- checks, keys, counts; the level lists
  HGS_HIP(hipMemsetAsync(t.res, 0, kHrZeroBytes, s));
  HGS_HIP(hipMemsetAsync(t.res->minima, 0xff, sizeof(t.res->minima), s));
  const dim3 grid((unsigned)((N + kHrThreads - 1) / kHrThreads)), block(kHrThreads);
  const dim3 plan_grid(grid.x < (unsigned)kHrPlanBlocks ? grid.x : (unsigned)kHrPlanBlocks);
  hipLaunchKernelGGL(hr_plan_kernel, plan_grid, block, 0, s, in.nodes, in.xyz, in.log_scales, in.rots, in.boxes, (int32_t)N, mode,
                     t.keys, t.res);
  HGS_LAUNCH_CHECK("hr_plan", s, false);
  int rc = sort_pairs32(t.keys, nullptr, t.keys_sorted, t.order, t.sort_tmp, (uint32_t)N, nullptr, 8, s, false);
  if (rc) return rc;
  // ---- the one host wait
  HrResult host;
  HGS_HIP(hipMemcpyAsync(&host, t.res, sizeof(host), hipMemcpyDeviceToHost, s));
  HGS_HIP(wait_stream(s));
  first_bad_from_minima(host.minima, kHrChecks, report->first_bad);
  int levels = 0;
  while (levels < kLevels && host.counts[levels]) ++levels;
  report->levels = levels;
  report->leaves = (int64_t)host.leaves;
  report->children_sum = (int64_t)host.children_sum;
  static const char* const what[kHrChecks] = {
      "start != node index or count_leafs + count_merged != 1", "children range outside [1, N)",
      "parent outside [0, N) or not claiming the node (node 0: parent != -1)", "depth outside [0, 255]",
      "depth is not the parent's depth + 1 (without a parent in [0, N): depth != 0)", "more than one node of depth 0",
      "a leaf whose box is not finite or has lo > hi"};
  if (fail_on_first_bad(report->first_bad, what, kHrChecks,
                        "not a hierarchy that can be refit: %s (first offending node %d); nothing was written"))
    return HGS_ERR_INVALID;
  if (report->children_sum != N - 1) {
    set_error("not a hierarchy that can be refit: count_children sums to %lld over %lld nodes, N - 1 expected (two nodes "
              "claim the same children); nothing was written", (long long)report->children_sum, (long long)N);
    return HGS_ERR_INVALID;
  }
  // (node 0 has no parent, so it passed with depth 0; every other node lies one level under its parent: the depths in use
  //  are 0 .. levels - 1 without a gap)
  // ---- the leaves, then one launch per level, bottom-up
  if (!(mode == kRefitKeep && boxes_out == in.boxes)) {
    hipLaunchKernelGGL(hr_leaf_kernel, grid, block, 0, s, in.nodes, in.xyz, in.log_scales, in.rots, in.boxes, boxes_out,
                       (int32_t)N, mode);
    HGS_LAUNCH_CHECK("hr_leaf", s, false);
  }
  int64_t first = N - host.counts[levels - 1];   // the deepest level holds leaves alone
  for (int d = levels - 2; d >= 0; --d) {
    const int64_t count = host.counts[d];
    first -= count;
    hipLaunchKernelGGL(hr_level_kernel, dim3((unsigned)((count + kHrThreads - 1) / kHrThreads)), block, 0, s,
                       t.order + first, (int32_t)count, in.nodes, in.boxes, boxes_out);
    HGS_LAUNCH_CHECK("hr_level", s, false);
  }
  return HGS_OK;
}

}  // namespace hgs
