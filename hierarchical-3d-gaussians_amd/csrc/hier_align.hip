// Rotation alignment of a hierarchy: the rule of hgs.hierarchy.align_hierarchy (the spec) in place on the device.
//
//   rule       a node's (rotation, scales) pair has 24 equivalent parametrisations: the frame's axes permuted and negated by
//              a proper signed permutation matrix M, R(q (x) g) = R(q) M, the log-scales permuted with the axes.  Every node
//              of depth > 0 takes the one whose quaternion is closest to its parent's FINAL quaternion: the first j that
//              maximises |<q (x) g_j, q'_parent>|, the sign of the dot folded in.  Parents before children.
//   levels     ha_check_kernel: one thread per node validates the row's depth / parent columns (first offending node per
//              check), writes the depth as a sort key and counts the nodes per depth; sort_pairs32 (8 bits, stable) turns
//              the keys into the level lists; ONE host wait reads the counts and the checks.  Nothing has been written
//              to the hierarchy at that point: an invalid one is returned untouched.  The workspace, the sort, the number
//              of levels and the launch per depth are the host half of hier_levels.h; the checks are this rule's own.
//   align      ha_level_kernel, one launch per depth 1, 2, ..: one thread per node reads its parent column, its 7 floats
//              and the parent's quaternion (written by the previous launch), and writes its 7 floats if they change.
//              Arithmetic in double, contraction off, every sum in the spec's order: the choice and the bits are the spec's.
//
// Any numbering works (the builder's BFS, the merger's chunks side by side): only depth and parent are read.
#include "hier_levels.h"   // the host half of the level walk; the check kernel here is this rule's own
#include "hier_nodes.h"

#pragma clang fp contract(off)

namespace hgs {
namespace {

constexpr int kHaThreads = kLevelThreads;

// Device half of the report, read back with the level counts in one copy.
struct HaResult {
  uint32_t counts[kLevels];   // nodes per depth (one with a depth outside [0, 255] is not counted)
  uint32_t first_bad[3];      // unsigned minima, kNone = none
  uint32_t first_root;        // the smallest node index of depth 0
  uint32_t second_root;       // the second smallest
  uint32_t pad[3];
};

struct GroupElement {
  double q[4];   // (w, x, y, z) of the signed permutation matrix
  int perm[3];   // new axis k = +- old axis perm[k]
};

// hgs.hierarchy.align_group(): permutations of (0,1,2) outermost, signs (1,-1)^3 inside, det > 0 kept; the quaternions
// are _quat_from_rot's float64 values (its two roundings of sqrt(1/2) included)
constexpr double kA = 0x1.6a09e667f3bcdp-1, kB = 0x1.6a09e667f3bccp-1;
constexpr int kGroup = 24;
__device__ constexpr GroupElement kG[kGroup] = {
    {{1.0, 0.0, 0.0, 0.0}, {0, 1, 2}},
    {{0.0, 1.0, 0.0, 0.0}, {0, 1, 2}},
    {{0.0, 0.0, 1.0, 0.0}, {0, 1, 2}},
    {{0.0, 0.0, 0.0, 1.0}, {0, 1, 2}},
    {{kA, kB, 0.0, 0.0}, {0, 2, 1}},
    {{kA, -kB, 0.0, 0.0}, {0, 2, 1}},
    {{0.0, 0.0, kA, kB}, {0, 2, 1}},
    {{0.0, 0.0, kA, -kB}, {0, 2, 1}},
    {{0.0, kA, kB, 0.0}, {1, 0, 2}},
    {{kA, 0.0, 0.0, kB}, {1, 0, 2}},
    {{kA, 0.0, 0.0, -kB}, {1, 0, 2}},
    {{0.0, kA, -kB, 0.0}, {1, 0, 2}},
    {{0.5, 0.5, 0.5, 0.5}, {1, 2, 0}},
    {{-0.5, 0.5, 0.5, -0.5}, {1, 2, 0}},
    {{0.5, 0.5, -0.5, -0.5}, {1, 2, 0}},
    {{-0.5, 0.5, -0.5, 0.5}, {1, 2, 0}},
    {{-0.5, 0.5, 0.5, 0.5}, {2, 0, 1}},
    {{0.5, 0.5, -0.5, 0.5}, {2, 0, 1}},
    {{0.5, 0.5, 0.5, -0.5}, {2, 0, 1}},
    {{-0.5, 0.5, -0.5, -0.5}, {2, 0, 1}},
    {{kA, 0.0, -kB, 0.0}, {2, 1, 0}},
    {{0.0, kA, 0.0, kB}, {2, 1, 0}},
    {{kA, 0.0, kB, 0.0}, {2, 1, 0}},
    {{0.0, kA, 0.0, -kB}, {2, 1, 0}},
};

// One thread per node: the checks of the row, its depth as the sort key, the per-depth counts (LDS bins per workgroup).
__global__ __launch_bounds__(kHaThreads) void ha_check_kernel(const int32_t* __restrict__ nodes, int32_t N,
                                                              uint32_t* __restrict__ keys, HaResult* __restrict__ res) {
  __shared__ uint32_t bins[kLevels];
  bins[threadIdx.x] = 0;            // kHaThreads == kLevels
  __syncthreads();
  const int64_t i = (int64_t)blockIdx.x * kHaThreads + threadIdx.x;
  if (i < N) {
    const int32_t depth = nodes[i * kNodeInts + 0], parent = nodes[i * kNodeInts + 1];
    const bool bad_depth = depth < 0 || depth > kMaxDepth;
    if (bad_depth) atomicMin(&res->first_bad[0], (uint32_t)i);
    if (depth != 0) {
      if (parent < 0 || parent >= N) atomicMin(&res->first_bad[1], (uint32_t)i);
      else if (nodes[(int64_t)parent * kNodeInts] != depth - 1) atomicMin(&res->first_bad[2], (uint32_t)i);
    } else {
      // the two smallest roots: the second one is the smallest max(a, b) over pairs of roots, and the pair of the two
      // smallest meets here whichever of them arrives first
      const uint32_t old = atomicMin(&res->first_root, (uint32_t)i);
      if (old != kNone) atomicMin(&res->second_root, max(old, (uint32_t)i));
    }
    const uint32_t key = bad_depth ? 0u : (uint32_t)depth;
    keys[i] = key;
    if (!bad_depth) atomicAdd(&bins[key], 1u);
  }
  __syncthreads();
  const uint32_t c = bins[threadIdx.x];
  if (c) atomicAdd(&res->counts[threadIdx.x], c);
}

// One thread per node of one depth: the rule.  `level` = this depth's slice of the depth-sorted node ids.
__global__ __launch_bounds__(kHaThreads) void ha_level_kernel(const uint32_t* __restrict__ level, int32_t count,
                                                              const int32_t* __restrict__ nodes,
                                                              float* __restrict__ log_scales, float* __restrict__ rots) {
  const int32_t t = (int32_t)(blockIdx.x * kHaThreads + threadIdx.x);
  if (t >= count) return;
  const int64_t id = level[t];
  const int64_t parent = nodes[id * kNodeInts + 1];
  const float4 qf = reinterpret_cast<const float4*>(rots)[id];
  const float4 pf = reinterpret_cast<const float4*>(rots)[parent];
  const double a0 = qf.x, a1 = qf.y, a2 = qf.z, a3 = qf.w;
  const double p0 = pf.x, p1 = pf.y, p2 = pf.z, p3 = pf.w;
  int best_j = 0;
  double best_abs = 0.0, best_d = 0.0, b0 = a0, b1 = a1, b2 = a2, b3 = a3;
#pragma unroll
  for (int j = 0; j < kGroup; ++j) {
    const double g0 = kG[j].q[0], g1 = kG[j].q[1], g2 = kG[j].q[2], g3 = kG[j].q[3];
    const double c0 = a0 * g0 - a1 * g1 - a2 * g2 - a3 * g3;
    const double c1 = a0 * g1 + a1 * g0 + a2 * g3 - a3 * g2;
    const double c2 = a0 * g2 - a1 * g3 + a2 * g0 + a3 * g1;
    const double c3 = a0 * g3 + a1 * g2 - a2 * g1 + a3 * g0;
    const double d = c0 * p0 + c1 * p1 + c2 * p2 + c3 * p3;
    const double ad = fabs(d);
    if (j == 0 || ad > best_abs) {      // the first maximum
      best_j = j; best_abs = ad; best_d = d;
      b0 = c0; b1 = c1; b2 = c2; b3 = c3;
    }
  }
  const bool neg = best_d < 0.0;        // sign(0) = +
  if (best_j == 0) {
    if (neg) reinterpret_cast<float4*>(rots)[id] = make_float4(-qf.x, -qf.y, -qf.z, -qf.w);   // exact negation
    return;
  }
  reinterpret_cast<float4*>(rots)[id] = neg ? make_float4((float)-b0, (float)-b1, (float)-b2, (float)-b3)
                                            : make_float4((float)b0, (float)b1, (float)b2, (float)b3);
  const float l0 = log_scales[id * 3 + 0], l1 = log_scales[id * 3 + 1], l2 = log_scales[id * 3 + 2];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int p = kG[best_j].perm[k];
    log_scales[id * 3 + k] = p == 0 ? l0 : (p == 1 ? l1 : l2);
  }
}

using HaTmp = LevelListsTmp<HaResult>;

}  // namespace

size_t hier_align_tmp_bytes(int64_t N) {
  Carver c(nullptr);
  HaTmp t;
  carve_level_lists(c, N, t);
  return c.bytes(0);   // this workspace never had a slack block of its own (the nested sort's is its last)
}

int launch_hier_align(const int32_t* nodes, int64_t N, float* log_scales, float* rots, void* tmp,
                      hgs_hier_align_report* report, hipStream_t s) {
  Carver c(tmp);
  HaTmp t;
  carve_level_lists(c, N, t);
  // ---- checks, keys and level counts; the level lists
  HGS_HIP(hipMemsetAsync(t.res->counts, 0, sizeof(t.res->counts), s));
  HGS_HIP(hipMemsetAsync(t.res->first_bad, 0xff, sizeof(HaResult) - sizeof(t.res->counts), s));
  const unsigned blocks = (unsigned)((N + kHaThreads - 1) / kHaThreads);
  hipLaunchKernelGGL(ha_check_kernel, dim3(blocks), dim3(kHaThreads), 0, s, nodes, (int32_t)N, t.keys, t.res);
  HGS_LAUNCH_CHECK("ha_check", s, false);
  if (int rc = sort_level_lists(t, N, s)) return rc;
  // ---- the one host wait
  HaResult host;
  HGS_HIP(hipMemcpyAsync(&host, t.res, sizeof(host), hipMemcpyDeviceToHost, s));
  HGS_HIP(wait_stream(s));
  first_bad_from_minima(host.first_bad, 3, report->first_bad);
  first_bad_from_minima(&host.second_root, 1, &report->first_bad[3]);
  report->roots = (int32_t)host.counts[0];
  const int levels = level_count(host.counts);
  report->levels = levels;
  report->reserved[0] = report->reserved[1] = 0;
  static const char* const what[4] = {"depth outside [0, 255]", "parent outside [0, N) at a node of depth > 0",
                                      "parent's depth is not the node's depth - 1", "more than one node of depth 0"};
  if (fail_on_first_bad(report->first_bad, what, 4,
                        "not a valid hierarchy: %s (first offending node %d); nothing was changed"))
    return HGS_ERR_INVALID;
  if (host.first_root == kNone) {
    report->roots = 0;
    set_error("not a valid hierarchy: no node of depth 0; nothing was changed");
    return HGS_ERR_INVALID;
  }
  // (every node of depth d > 0 has a parent of depth d - 1, so the depths in use are 0 .. levels - 1 without a gap)
  // ---- one launch per level, top-down
  return launch_levels_down(ha_level_kernel, "ha_level", s, t.order, host.counts, levels, nodes, log_scales, rots);
}

}  // namespace hgs
