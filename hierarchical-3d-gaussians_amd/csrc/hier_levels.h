// The level-ordered walk, for a tool that goes through a hierarchy one depth at a time, ONCE: device half and host half.
//
//   device     the plan of hier_refit.hip and hier_prune.hip: the six checks a node has to pass -- the three layout checks
//              of hier_nodes.h and the three depth checks -- its depth as an 8-bit sort key, the count of nodes per depth,
//              one tally of the tool's own and the sum of count_children.  A plan kernel calls level_plan_begin, then
//              level_check_node for each of its nodes and level_count_depths once per trip of its workgroup, then
//              level_plan_end.  And the box of a node with children: the union of its children's boxes.
//   host       the workspace of the level lists and its carve, the stable 8-bit sort of the keys into the lists (ascending
//              ids inside a level), the number of levels from the counts, one launch per depth bottom-up or top-down, and
//              the error text of a failed plan.  hier_align.hip runs the host half under its own check kernel: its rule
//              reads depth and parent alone and accepts any numbering.
#pragma once
#include "hier_nodes.h"
#include "hier_refit_rule.h"   // the union and the extent of a box

#include <cstdio>

namespace hgs {
namespace {

constexpr int kMaxDepth = 255;
constexpr int kLevels = kMaxDepth + 1;
constexpr int kLevelThreads = kLevels;    // a workgroup of every kernel here: one thread per depth bin
constexpr int kLevelPlanBlocks = 2048;    // 8 workgroups of 256 threads on each of 256 compute units: a plan's grid at most
constexpr int kLevelChecks = 6;           // minima[0 .. 6): the checks in the reports' order
constexpr int kLevelOwnCheck = 6;         // minima[6]: a check of the tool's own (refit: the leaf box)
constexpr int kLevelRoot = 7;             // minima[7]: the smallest node of depth 0

// Device half of a plan's report, read back in one copy.  A tool with more to count derives from it.
struct LevelResult {
  uint32_t counts[kLevels];          // nodes per depth (one with a depth outside [0, 255] is not counted)
  uint32_t tally;                    // the tool's own count: refit's leaves, prune's removed leaves
  uint32_t pad;
  unsigned long long children_sum;   // over the nodes whose children range passed its check
  uint32_t minima[kLevelRoot + 1];   // unsigned minima, kNone = none ([5] = the second smallest node of depth 0)
};

// What a plan kernel's workgroup keeps in LDS over its whole walk.
struct LevelPlanLds {
  uint32_t bins[kLevels];
  uint32_t tally;
  unsigned long long children;
};

__device__ __forceinline__ void level_plan_begin(LevelPlanLds& lds) {
  lds.bins[threadIdx.x] = 0;
  if (threadIdx.x == 0) { lds.tally = 0; lds.children = 0; }
  __syncthreads();
}

// The checks of node i (< N).  minima: those of a LevelResult.  children += count_children where the children range
// passed its check.  -> the sort key; *counted: the node takes part in the per-depth count; *cc_out: its count_children.
__device__ __forceinline__ uint32_t level_check_node(const int32_t* __restrict__ nodes, int64_t i, int32_t N,
                                                     uint32_t* __restrict__ minima, unsigned long long& children,
                                                     bool* counted, int64_t* cc_out) {
  const int32_t* nd = nodes + i * kNodeInts;
  const int32_t depth = nd[0], parent = nd[1];
  const int64_t cc = nd[6];
  // ---- the three layout checks
  const uint32_t v = node_layout(nodes, i, N);
  if (v & kBadRow) atomicMin(&minima[0], (uint32_t)i);
  if (v & kBadChildren) atomicMin(&minima[1], (uint32_t)i);
  if (v & kBadParent) atomicMin(&minima[2], (uint32_t)i);
  if (!(v & kBadChildren)) children += (unsigned long long)cc;
  // ---- the depth checks
  const bool bad_depth = depth < 0 || depth > kMaxDepth;
  if (bad_depth) atomicMin(&minima[3], (uint32_t)i);
  if (depth != 0) {
    if (parent < 0 || parent >= N || nodes[(int64_t)parent * kNodeInts] != depth - 1) atomicMin(&minima[4], (uint32_t)i);
  } else {
    // the two smallest nodes of depth 0: the second one is the smallest max(a, b) over pairs of them, and the pair
    // of the two smallest meets here whichever of them arrives first
    const uint32_t old = atomicMin(&minima[kLevelRoot], (uint32_t)i);
    if (old != kNone) atomicMin(&minima[5], max(old, (uint32_t)i));
  }
  *counted = !bad_depth;
  *cc_out = cc;
  return bad_depth ? 0u : (uint32_t)depth;
}

// The per-depth count of one trip (every lane of the workgroup is here: the trip count is the workgroup's): a wave whose
// nodes share a depth -- nearly every wave of a BFS numbering -- counts them with one LDS atomic (with one workgroup per
// 256 nodes, each flushing its sums and every lane adding to its LDS bin, refit's plan took 3.1 ms at 50 M nodes; 0.9 ms
// with a capped grid, the sums in registers and LDS over the whole walk, and this).
__device__ __forceinline__ void level_count_depths(uint32_t* bins, uint32_t key, bool counted, int lane) {
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

// The end of a plan kernel: the lanes' sums into LDS, and the workgroup's bins and sums into the global words, once.
__device__ __forceinline__ void level_plan_end(LevelPlanLds& lds, unsigned long long children, uint32_t tally, int lane,
                                               LevelResult* __restrict__ res) {
  for (int o = 32; o > 0; o >>= 1) {
    children += __shfl_down(children, o);
    tally += __shfl_down(tally, o);
  }
  if (lane == 0) {
    if (children) atomicAdd(&lds.children, children);
    if (tally) atomicAdd(&lds.tally, tally);
  }
  __syncthreads();
  const uint32_t c = lds.bins[threadIdx.x];
  if (c) atomicAdd(&res->counts[threadIdx.x], c);
  if (threadIdx.x == 0) {
    if (lds.tally) atomicAdd(&res->tally, lds.tally);
    if (lds.children) atomicAdd(&res->children_sum, lds.children);
  }
}

// Node id's box in boxes_out <- the union of the boxes of its cc >= 1 children from row sc of boxes_out, two float4 per
// child, with the extent of its rounded coordinates; boxes[id,1,3] is carried over (boxes may be boxes_out).
__device__ __forceinline__ void level_box_from_children(float* boxes_out, int64_t id, int64_t sc, int32_t cc,
                                                        const float* boxes) {
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

// ---- the host half

// The workspace of the level lists, Result = the tool's device report; a tool with more arrays takes them behind these.
template <typename Result>
struct LevelListsTmp {
  Result* res;
  uint32_t* keys;          // [N] the depth keys
  uint32_t* keys_sorted;   // [N]
  uint32_t* order;         // [N] the level lists: the node ids by depth, ascending inside a depth
  void* sort_tmp;
};

template <typename Result>
void carve_level_lists(Carver& c, int64_t N, LevelListsTmp<Result>& t) {
  t.res = c.take<Result>(1);
  t.keys = c.take<uint32_t>((size_t)N);
  t.keys_sorted = c.take<uint32_t>((size_t)N);
  t.order = c.take<uint32_t>((size_t)N);
  t.sort_tmp = c.take<char>(sort_tmp_bytes((uint32_t)N));   // nested: the sort's own slack included
}

// A LevelResult (or one derived from it) before its plan kernel: zeros, the minima kNone.
template <typename Result>
int clear_level_result(Result* res, hipStream_t s) {
  HGS_HIP(hipMemsetAsync(res, 0, sizeof(Result), s));
  HGS_HIP(hipMemsetAsync(res->minima, 0xff, sizeof(res->minima), s));
  return HGS_OK;
}

inline dim3 level_plan_grid(int64_t N) {
  const int64_t blocks = (N + kLevelThreads - 1) / kLevelThreads;
  return dim3((unsigned)(blocks < kLevelPlanBlocks ? blocks : kLevelPlanBlocks));
}

// t.keys -> t.order: the level lists
template <typename Result>
int sort_level_lists(const LevelListsTmp<Result>& t, int64_t N, hipStream_t s) {
  return sort_pairs32(t.keys, nullptr, t.keys_sorted, t.order, t.sort_tmp, (uint32_t)N, nullptr, 8, s, false);
}

// The depths in use are 0 .. levels - 1 without a gap once the depth checks have passed.
inline int level_count(const uint32_t* counts) {
  int levels = 0;
  while (levels < kLevels && counts[levels]) ++levels;
  return levels;
}

// kernel(list, count, args...) over the list of every depth with children, deepest first: levels - 2 .. 0 (the deepest
// level holds leaves alone).  counts: the nodes per depth of the N nodes in `order`.
template <typename Kernel, typename... Args>
int launch_levels_up(Kernel kernel, const char* name, hipStream_t s, const uint32_t* order, const uint32_t* counts,
                     int levels, int64_t N, Args... args) {
  int64_t first = N - counts[levels - 1];
  for (int d = levels - 2; d >= 0; --d) {
    const int64_t count = counts[d];
    first -= count;
    hipLaunchKernelGGL(kernel, dim3((unsigned)((count + kLevelThreads - 1) / kLevelThreads)), dim3(kLevelThreads), 0, s,
                       order + first, (int32_t)count, args...);
    HGS_LAUNCH_CHECK(name, s, false);
  }
  return HGS_OK;
}

// Its twin: the list of every depth with a parent, 1 .. levels - 1.
template <typename Kernel, typename... Args>
int launch_levels_down(Kernel kernel, const char* name, hipStream_t s, const uint32_t* order, const uint32_t* counts,
                       int levels, Args... args) {
  int64_t first = counts[0];
  for (int d = 1; d < levels; ++d) {
    const int64_t count = counts[d];
    hipLaunchKernelGGL(kernel, dim3((unsigned)((count + kLevelThreads - 1) / kLevelThreads)), dim3(kLevelThreads), 0, s,
                       order + first, (int32_t)count, args...);
    HGS_LAUNCH_CHECK(name, s, false);
    first += count;
  }
  return HGS_OK;
}

// The verdict on a plan's report: the first failing check of first_bad -- the six of this header, then the tool's own
// (own_check; nullptr: none) -- or a children sum that is not N - 1 -> the error text and HGS_ERR_INVALID.  verb: what
// the hierarchy cannot be ("refit", "pruned").
inline int level_plan_verdict(const int32_t* first_bad, const char* own_check, int64_t children_sum, int64_t N,
                              const char* verb) {
  const char* const what[kLevelChecks + 1] = {
      kLayoutChecks[0], kLayoutChecks[1], kLayoutChecks[2], "depth outside [0, 255]",
      "depth is not the parent's depth + 1 (without a parent in [0, N): depth != 0)", "more than one node of depth 0",
      own_check};
  char frame[128];
  snprintf(frame, sizeof(frame), "not a hierarchy that can be %s: %%s (first offending node %%d); nothing was written", verb);
  if (fail_on_first_bad(first_bad, what, kLevelChecks + (own_check ? 1 : 0), frame)) return HGS_ERR_INVALID;
  if (children_sum != N - 1) {
    set_error("not a hierarchy that can be %s: count_children sums to %lld over %lld nodes, N - 1 expected (two nodes "
              "claim the same children); nothing was written", verb, (long long)children_sum, (long long)N);
    return HGS_ERR_INVALID;
  }
  // (node 0 has no parent, so it passed with depth 0; every other node lies one level under its parent: the depths in use
  //  are 0 .. levels - 1 without a gap)
  return HGS_OK;
}

}  // namespace
}  // namespace hgs
