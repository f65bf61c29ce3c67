// The plan of a level-ordered walk, for a tool that goes through a hierarchy one depth at a time from the deepest level
// up: the six checks a node has to pass -- the three layout checks of hier_nodes.h and the three depth checks -- its depth
// as an 8-bit sort key, and the count of nodes per depth.  A plan kernel calls level_check_node for each of its nodes and
// level_count_depths once per trip of its workgroup; a stable 8-bit sort of the keys then gives the level lists,
// ascending ids inside a level.  hier_prune.hip runs it.  It RESTATES the walk of hr_plan_kernel (hier_refit.hip), which
// keeps its own text: routed through these functions that kernel compiled to other code (three instructions more, other
// registers), and the refit is not this header's to change.  tests/test_hier_prune_gpu.py holds the two together: every
// corruption refit names, prune names with the same node.
#pragma once
#include "hier_nodes.h"

namespace hgs {
namespace {

constexpr int kMaxDepth = 255;
constexpr int kLevels = kMaxDepth + 1;
constexpr int kLevelChecks = 6;   // minima[0 .. 6): the checks in the reports' order; minima[kLevelRoot]: scratch

// The checks of node i (< N).  minima: unsigned minima, kNone = none, [0..2] the layout checks, [3] a depth outside
// [0, 255], [4] a depth that is not the parent's + 1, [5] the second smallest node of depth 0, [root_slot] the smallest
// node of depth 0.  children += count_children where the children range passed its check.  -> the sort key; *counted:
// the node takes part in the per-depth count; *cc_out: its count_children.
__device__ __forceinline__ uint32_t level_check_node(const int32_t* __restrict__ nodes, int64_t i, int32_t N,
                                                     uint32_t* __restrict__ minima, int root_slot,
                                                     unsigned long long& children, bool* counted, int64_t* cc_out) {
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
    const uint32_t old = atomicMin(&minima[root_slot], (uint32_t)i);
    if (old != kNone) atomicMin(&minima[5], max(old, (uint32_t)i));
  }
  *counted = !bad_depth;
  *cc_out = cc;
  return bad_depth ? 0u : (uint32_t)depth;
}

// The per-depth count of one trip (every lane of the workgroup is here): a wave whose nodes share a depth -- nearly
// every wave of a BFS numbering -- counts them with one LDS atomic.
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

}  // namespace
}  // namespace hgs
