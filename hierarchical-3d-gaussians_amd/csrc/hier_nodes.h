// What the hierarchy tools share, each ONCE: the node record, the merger's three layout checks (run by hier_merge.hip,
// hier_trim.hip and, through hier_levels.h, hier_refit.hip and hier_prune.hip; restated in numpy by
// hgs.hierarchy.layout_check_masks) and their sentences, the seven row pointers of a hierarchy, the host half of a
// "first offending node per check" report.  Plain C++: tests/test_hier_nodes_on_host.py compiles it with g++.
#pragma once
#include "common.h"

namespace hgs {

void set_error(const char* fmt, ...);   // (common.h's; repeated for the stand-in)

constexpr int kNodeInts = 7;   // depth, parent, start, count_leafs, count_merged, start_children, count_children

// The verdict on node i of nodes[N][kNodeInts], one bit per check in the order the reports list them: a bad row, a bad
// children range, a parent that does not claim the node; and kParentInRange: i > 0 and 0 <= parent < N (the parent's
// record and box may be read: trim's rule needs it).  The three sums are 64-bit: the columns are an unchecked file's.
constexpr uint32_t kBadRow = 1u, kBadChildren = 2u, kBadParent = 4u, kParentInRange = 8u;

__host__ __device__ __forceinline__ uint32_t node_layout(const int32_t* __restrict__ nodes, int64_t i, int32_t N) {
  const int32_t* nd = nodes + i * kNodeInts;
  const int32_t parent = nd[1], start = nd[2], leafs = nd[3], merged = nd[4], sc = nd[5];
  const int64_t cc = nd[6];
  const bool bad_row = start != i || (int64_t)leafs + merged != 1;
  const bool parent_in_range = i > 0 && parent >= 0 && parent < N;
  bool bad_parent;
  if (i == 0) {
    bad_parent = parent != -1;
  } else if (!parent_in_range) {
    bad_parent = true;
  } else {
    const int32_t* pn = nodes + (int64_t)parent * kNodeInts;
    const int64_t ps = pn[5], pc = pn[6];
    bad_parent = !(i >= ps && i < ps + pc);
  }
  const bool bad_children = cc < 0 || (cc > 0 && (sc < 1 || (int64_t)sc + cc > N));
  return (bad_row ? kBadRow : 0u) | (bad_children ? kBadChildren : 0u) | (bad_parent ? kBadParent : 0u) |
         (parent_in_range ? kParentInRange : 0u);
}
// What the three checks say in an error text (hier_trim.hip, and hier_levels.h for hier_refit.hip and hier_prune.hip).
constexpr const char* kLayoutChecks[3] = {"start != node index or count_leafs + count_merged != 1",
                                          "children range outside [1, N)",
                                          "parent outside [0, N) or not claiming the node (node 0: parent != -1)"};

// The seven arrays of an hgs_hier_view as kernel arguments: read-only (HierRowsIn) and writable (HierRows).
template <typename F, typename I>
struct HierRowsOf {
  F* xyz; F* shs; F* alpha; F* log_scales; F* rots; I* nodes; F* boxes;
  static HierRowsOf of(const hgs_hier_view& v) { return {v.xyz, v.shs, v.alpha, v.log_scales, v.rots, v.nodes, v.boxes}; }
};
using HierRowsIn = HierRowsOf<const float, const int32_t>;
using HierRows = HierRowsOf<float, int32_t>;

// The report.  On the device a check's slot is an unsigned minimum: filled with 0xff bytes (= kNone) before the launch,
// lowered with atomicMin(&slot, (uint32_t)i) by every offender.  Read back, -1 stands for "nobody".
constexpr uint32_t kNone = 0xffffffffu;
inline void first_bad_from_minima(const uint32_t* minima, int n, int32_t* first_bad) {
  for (int c = 0; c < n; ++c) first_bad[c] = minima[c] == kNone ? -1 : (int32_t)minima[c];
}
// The first check of first_bad[0 .. n) with an offender -> the error text and HGS_ERR_INVALID; HGS_OK if there is none.
// frame: the caller's sentence with a %s for what[check] and a %d for the node, in that order.
inline int fail_on_first_bad(const int32_t* first_bad, const char* const* what, int n, const char* frame) {
  for (int c = 0; c < n; ++c)
    if (first_bad[c] >= 0) { set_error(frame, what[c], first_bad[c]); return HGS_ERR_INVALID; }
  return HGS_OK;
}

}  // namespace hgs
