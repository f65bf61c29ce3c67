// Refitting a hierarchy's boxes: the rule of hgs.hierarchy.refit_boxes (the spec) on the device.
//
//   rule       only boxes change.  A leaf (count_children == 0) keeps its box, or takes the cube / the ellipsoid box of
//              its own row (hier_refit_rule.h); a node with children takes the union of its children's FINAL boxes, its
//              own Gaussian not included (the builder's and the merger's rule); every written box gets the extent of
//              its rounded coordinates, boxes[n,1,3] is copied.  Children before parents.
//   plan       hr_plan_kernel: the plan walk of hier_levels.h, shared with hier_prune.hip -- one thread per node (a
//              capped grid walks the nodes) runs the three layout checks and the three depth checks, writes the depth as
//              a sort key, counts the nodes per depth (LDS bins per workgroup), the leaves and the sum of count_children
//              -- and at a leaf evaluates its box into registers for the test it has to pass (nothing is stored);
//              sort_pairs32 (8 bits, stable) turns the keys into the level lists, ascending ids inside a level; ONE
//              host wait reads the counts and the checks.  Nothing has been written to boxes_out then.
//   apply      asynchronous.  hr_leaf_kernel: one thread per node, the leaves write (or, kept and out of place, copy)
//              their boxes; then hr_level_kernel, one launch per depth from the deepest level with children up to 0:
//              one thread per node of the level list reads its children's boxes as two float4 each -- contiguous
//              children, neighbouring lanes on neighbouring ids: the reads coalesce without LDS -- and writes its own.
//
// Every index followed has passed the checks: a children range lies in [1, N), every node lies in the range of its own
// parent and the ranges hold N - 1 slots in all, so each range is exactly the node's children, one level down.  A single
// thread walks a wide node (the merged root).  In place (boxes_out == boxes) or out of place (no overlap).
#include "hier_levels.h"
#include "hier_nodes.h"
#include "hier_refit_rule.h"

#pragma clang fp contract(off)

namespace hgs {
namespace {

constexpr int kHrThreads = kLevelThreads;
using HrResult = LevelResult;   // tally: the leaves; minima[kLevelOwnCheck]: a leaf whose box fails its test

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

// One thread per node, kLevelPlanBlocks workgroups at most that walk the nodes in strides: the plan walk of hier_levels.h
// (the checks, the depth as the sort key, the per-depth counts, the children sum) with the leaf count as its tally and,
// at a leaf, the test of its box.
__global__ __launch_bounds__(kHrThreads) void hr_plan_kernel(const int32_t* __restrict__ nodes,
                                                             const float* __restrict__ xyz,
                                                             const float* __restrict__ log_scales,
                                                             const float* __restrict__ rots,
                                                             const float* __restrict__ boxes, int32_t N, int32_t mode,
                                                             uint32_t* __restrict__ keys, HrResult* __restrict__ res) {
  __shared__ LevelPlanLds lds;
  level_plan_begin(lds);
  const int lane = threadIdx.x & 63;
  unsigned long long children = 0;
  uint32_t leaves = 0;
  for (int64_t base = (int64_t)blockIdx.x * kHrThreads; base < N; base += (int64_t)gridDim.x * kHrThreads) {
    const int64_t i = base + threadIdx.x;
    uint32_t key = 0;
    bool counted = false;
    if (i < N) {
      int64_t cc;
      key = level_check_node(nodes, i, N, res->minima, children, &counted, &cc);
      // ---- a leaf: its box, for the test alone
      if (cc == 0) {
        ++leaves;
        const LeafBox b = hr_leaf_box(i, mode, xyz, log_scales, rots, boxes);
        if (!refit_box_ok(b.lo, b.hi)) atomicMin(&res->minima[kLevelOwnCheck], (uint32_t)i);
      }
      keys[i] = key;
    }
    level_count_depths(lds.bins, key, counted, lane);
  }
  level_plan_end(lds, children, leaves, lane, res);
}

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
  level_box_from_children(boxes_out, id, sc, cc, boxes);
}

using HrTmp = LevelListsTmp<HrResult>;

}  // namespace

size_t hier_refit_tmp_bytes(int64_t N) {
  Carver c(nullptr);
  HrTmp t;
  carve_level_lists(c, N, t);
  return c.bytes(0);   // tmp is required to be kAlign-aligned: no slack
}

int launch_hier_refit(const hgs_hier_view& in, float* boxes_out, int32_t mode, void* tmp, hgs_hier_refit_report* report,
                      hipStream_t s) {
  const int64_t N = in.N;
  Carver c(tmp);
  HrTmp t;
  carve_level_lists(c, N, t);
  // ---- checks, keys, counts; the level lists
  int rc = clear_level_result(t.res, s);
  if (rc) return rc;
  const dim3 grid((unsigned)((N + kHrThreads - 1) / kHrThreads)), block(kHrThreads);
  hipLaunchKernelGGL(hr_plan_kernel, level_plan_grid(N), block, 0, s, in.nodes, in.xyz, in.log_scales, in.rots, in.boxes,
                     (int32_t)N, mode, t.keys, t.res);
  HGS_LAUNCH_CHECK("hr_plan", s, false);
  if ((rc = sort_level_lists(t, N, s))) return rc;
  // ---- the one host wait
  HrResult host;
  HGS_HIP(hipMemcpyAsync(&host, t.res, sizeof(host), hipMemcpyDeviceToHost, s));
  HGS_HIP(wait_stream(s));
  first_bad_from_minima(host.minima, kLevelChecks + 1, report->first_bad);
  const int levels = level_count(host.counts);
  report->levels = levels;
  report->leaves = (int64_t)host.tally;
  report->children_sum = (int64_t)host.children_sum;
  if ((rc = level_plan_verdict(report->first_bad, "a leaf whose box is not finite or has lo > hi", report->children_sum, N,
                               "refit")))
    return rc;
  // ---- the leaves, then one launch per level, bottom-up
  if (!(mode == kRefitKeep && boxes_out == in.boxes)) {
    hipLaunchKernelGGL(hr_leaf_kernel, grid, block, 0, s, in.nodes, in.xyz, in.log_scales, in.rots, in.boxes, boxes_out,
                       (int32_t)N, mode);
    HGS_LAUNCH_CHECK("hr_leaf", s, false);
  }
  return launch_levels_up(hr_level_kernel, "hr_level", s, t.order, host.counts, levels, N, in.nodes, in.boxes, boxes_out);
}

}  // namespace hgs
