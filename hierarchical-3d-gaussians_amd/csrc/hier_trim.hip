// Trimming a hierarchy: the rule of hgs.hierarchy.trim_hierarchy (the spec) on the device, in two calls.
//
//   rule       test(p) = extent(p) >= min_extent, and with a region: box(p) meets the closed box [lo, hi] (float32
//              comparisons only).  Node 0 is kept; node n > 0 is kept iff test(parent(n)): siblings stay or go together.
//              A kept node with children whose own test fails becomes a STUB: it takes a leaf's record.  Rows and boxes of
//              the kept nodes are copied in ascending old order, node records renumbered.
//   plan       ht_plan_kernel: one thread per node reads its record, its own box and its parent's (the grandparent's only
//              for the closure check of a kept node), evaluates test, the keep flag, the three layout checks of the merger
//              (node_layout of hier_nodes.h, the text hier_merge.hip runs) and the closure check (first offending node
//              per check), and writes the workgroup's keep sum and stub sum; ht_scan_kernel: the chained scan of
//              common.h over the keep sums, the stub sums added up beside it (one atomic per scan chunk: one per stub
//              wave on a single word cost 4 ms at 4.2 M stubs); ONE host wait reads back the kept count, the stub count
//              and the checks.  Nothing has been written to any output at that point.
//   keyed      hgs_hier_trim_plan_keyed: the same plan with one more conjunct in test, key[p] >= key_floor, key a device
//              float per node (hgs.hierarchy.trim_to_views: the view reach of hier_reach.hip against a granularity).
//              ht_plan_kernel<true> beside ht_plan_kernel<false>; the same tmp layout and plan record, so apply takes
//              either plan.
//   apply      asynchronous.  ht_maps_kernel: new_of_old and old_of_new from the flags and the scanned sums;
//              ht_gather_kernel: one workgroup per kHtRows OUTPUT rows stages their source rows in LDS, then copies tensor
//              by tensor, one thread per 16-byte piece (shs where 12 M is a multiple of 16 and both bases are aligned,
//              rots, boxes) or 4-byte piece (xyz, alpha, log_scales, the rewritten node records, shs otherwise): stores
//              are contiguous over the workgroup's rows, reads contiguous within a row, and across rows wherever the kept
//              set is a run of the old order (under an extent floor it is nearly a prefix of the BFS order).
//
// Rows at index >= N of the input (a skybox tail) are not read; rows at index >= N' of the output are not written.
#include "hier_gather.h"   // the maps kernel, the row copy and the plan book, shared with hier_prune.hip
#include "hier_nodes.h"
#include "lod_cut.h"   // the workgroup sums and the launcher of the chained scan (the cut rules in it are not used here)

namespace hgs {
namespace {

constexpr uint32_t kTest = 2u;   // bit 1 of a node's flag byte (bit 0: kKeep of hier_gather.h)

// Device half of the report (the kept and stub counts are the two words behind the scanned workgroup sums).
struct HtResult {
  uint32_t first_bad[4];   // unsigned minima, kNone = none
};

// kKeyed: one more conjunct, key[n] >= key_floor (hgs_hier_trim_plan_keyed; a NaN key never passes)
template <bool kKeyed>
__device__ __forceinline__ bool ht_test(const float* __restrict__ boxes, int64_t n, const hgs_hier_trim_args& a,
                                        const float* __restrict__ key, float key_floor) {
  const float4 mn = reinterpret_cast<const float4*>(boxes)[n * 2 + 0];
  bool ok = mn.w >= a.min_extent;                 // (a NaN extent never passes)
  if constexpr (kKeyed) ok = ok && key[n] >= key_floor;
  if (a.use_roi) {
    const float4 mx = reinterpret_cast<const float4*>(boxes)[n * 2 + 1];
    ok = ok && mn.x <= a.roi_hi[0] && mx.x >= a.roi_lo[0] && mn.y <= a.roi_hi[1] && mx.y >= a.roi_lo[1] &&
         mn.z <= a.roi_hi[2] && mx.z >= a.roi_lo[2];
  }
  return ok;
}

// One thread per node: the checks of the row, its flags, the workgroup's keep sum and stub sum.  <false>: the plan of
// hgs_hier_trim_plan (key and key_floor are not looked at); <true>: the keyed plan.
template <bool kKeyed>
__global__ __launch_bounds__(kHtThreads) void ht_plan_kernel(const int32_t* __restrict__ nodes,
                                                             const float* __restrict__ boxes, int32_t N,
                                                             hgs_hier_trim_args a, uint8_t* __restrict__ flags,
                                                             uint32_t* __restrict__ block_sums,
                                                             uint32_t* __restrict__ block_stubs,
                                                             unsigned long long* __restrict__ chain,
                                                             HtResult* __restrict__ res, const float* __restrict__ key,
                                                             float key_floor) {
  clear_scan_chain(chain, block_sums);
  const int64_t i = (int64_t)blockIdx.x * kHtThreads + threadIdx.x;
  uint32_t keep = 0, stub = 0;
  if (i < N) {
    const int32_t* nd = nodes + i * kNodeInts;
    const int32_t parent = nd[1];
    const int64_t cc = nd[6];
    // ---- the merger's three checks
    const uint32_t v = node_layout(nodes, i, N);
    if (v & kBadRow) atomicMin(&res->first_bad[0], (uint32_t)i);
    if (v & kBadChildren) atomicMin(&res->first_bad[1], (uint32_t)i);
    if (v & kBadParent) atomicMin(&res->first_bad[2], (uint32_t)i);
    // ---- the rule
    const bool test_self = ht_test<kKeyed>(boxes, i, a, key, key_floor);
    bool k = i == 0;
    if (v & kParentInRange) {
      k = ht_test<kKeyed>(boxes, parent, a, key, key_floor);
      if (k && parent != 0) {          // closure: a kept node's parent is kept (a bad grandparent index is check [2]'s)
        const int32_t pp = nodes[(int64_t)parent * kNodeInts + 1];
        if (pp >= 0 && pp < N && !ht_test<kKeyed>(boxes, pp, a, key, key_floor)) atomicMin(&res->first_bad[3], (uint32_t)i);
      }
    }
    keep = k ? 1u : 0u;
    stub = (k && cc > 0 && !test_self) ? 1u : 0u;
    flags[i] = (uint8_t)((k ? kKeep : 0u) | (test_self ? kTest : 0u));
  }
  const uint32_t cnt[2] = {keep, stub};
  uint32_t* const out[2] = {block_sums, block_stubs};
  block_totals<2>(cnt, out);
}

// sums[0 .. n) scanned in place, sums[n] = the kept count, sums[n + 1] = the stub count
__global__ __launch_bounds__(1024) void ht_scan_kernel(uint32_t* __restrict__ sums,
                                                       const uint32_t* __restrict__ block_stubs, int n,
                                                       unsigned long long* __restrict__ chain, int c_off, int chunks) {
  scan_sums_and_unculled_total(sums, block_stubs, n, chain, c_off, chunks);
}

// One workgroup per kHtRows output rows.  S: 16-byte pieces of an shs row (0: shs goes in W 4-byte pieces).
__global__ __launch_bounds__(kHtThreads) void ht_gather_kernel(HierRowsIn in, HierRows out,
                                                               const int32_t* __restrict__ old_of_new,
                                                               const int32_t* __restrict__ new_of_old,
                                                               const uint8_t* __restrict__ flags, int32_t kept,
                                                               uint32_t S, uint32_t W) {
  __shared__ int32_t src[kHtRows];
  const int64_t r0 = (int64_t)blockIdx.x * kHtRows;
  const uint32_t rows = ht_stage_rows(src, old_of_new, r0, kept);
  ht_copy_tensors(in, out, src, r0, rows, S, W);
  // the node records, one thread per int: depth kept, parent / start / start_children renumbered, a stub takes a
  // leaf's record, a leaf keeps its own
  int32_t* o = out.nodes + r0 * kNodeInts;
  const uint32_t L = rows * kNodeInts;
  for (uint32_t u = threadIdx.x; u < L; u += kHtThreads) {
    const uint32_t jl = u / kNodeInts, k = u - jl * kNodeInts;
    const int64_t i = src[jl];
    const int32_t* nd = in.nodes + i * kNodeInts;
    const int32_t cc = nd[6];
    const bool stub = cc > 0 && (flags[i] & kTest) == 0u;
    int32_t v;
    switch (k) {
      case 0: v = nd[0]; break;
      case 1: v = i == 0 ? -1 : new_of_old[nd[1]]; break;
      case 2: v = (int32_t)(r0 + jl); break;
      case 3: v = stub ? 1 : nd[3]; break;
      case 4: v = stub ? 0 : nd[4]; break;
      case 5: v = stub ? 0 : (cc > 0 ? new_of_old[nd[5]] : nd[5]); break;
      default: v = stub ? 0 : cc; break;
    }
    o[u] = v;
  }
}

struct HtTmp : SumsTmp {
  HtResult* res;
  uint8_t* flags;   // [N]
};

HtTmp carve_ht_tmp(Carver& c, int64_t N) {
  HtTmp t;
  t.res = c.take<HtResult>(1);
  t.flags = c.take<uint8_t>((size_t)N);
  static_cast<SumsTmp&>(t) = carve_sums(c, (size_t)N, true);   // block_all: the workgroups' stub sums
  return t;
}

// What the last successful plan on (device, tmp) found: the apply call checks its sizes against it on the host.
struct HtPlan { int device; const void* tmp; int64_t N; int64_t kept; };
PlanBook<HtPlan> g_ht_plans;

}  // namespace

size_t hier_trim_tmp_bytes(int64_t N) {
  Carver c(nullptr);
  carve_ht_tmp(c, N);
  return c.bytes(0);   // tmp is required to be kAlign-aligned: no slack
}

bool hier_trim_planned(int device, const void* tmp, int64_t* N, int64_t* kept) {
  HtPlan p;
  if (!g_ht_plans.find(device, tmp, &p)) return false;
  *N = p.N;
  *kept = p.kept;
  return true;
}

// key == nullptr: the plain plan; else the keyed one (key float [N] on the device, key_floor)
int launch_hier_trim_plan(const hgs_hier_view& in, const hgs_hier_trim_args& args, const float* key, float key_floor,
                          void* tmp, hgs_hier_trim_report* report, hipStream_t s, int device) {
  g_ht_plans.forget(device, tmp);
  const int64_t N = in.N;
  Carver c(tmp);
  const HtTmp t = carve_ht_tmp(c, N);
  HGS_HIP(hipMemsetAsync(t.res, 0xff, sizeof(HtResult), s));
  const int nblk = (int)((N + kHtThreads - 1) / kHtThreads);
  if (key) {
    hipLaunchKernelGGL(ht_plan_kernel<true>, dim3((unsigned)nblk), dim3(kHtThreads), 0, s, in.nodes, in.boxes, (int32_t)N,
                       args, t.flags, t.block_sums, t.block_all, t.chain, t.res, key, key_floor);
    HGS_LAUNCH_CHECK("ht_plan_keyed", s, false);
  } else {
    hipLaunchKernelGGL(ht_plan_kernel<false>, dim3((unsigned)nblk), dim3(kHtThreads), 0, s, in.nodes, in.boxes, (int32_t)N,
                       args, t.flags, t.block_sums, t.block_all, t.chain, t.res, key, key_floor);
    HGS_LAUNCH_CHECK("ht_plan", s, false);
  }
  const int rc = launch_scan_chunks(ht_scan_kernel, "ht_scan", nblk, s, t.block_sums, t.block_all, nblk, t.chain);
  if (rc) return rc;
  // ---- the one host wait
  HtResult host;
  uint32_t totals[2];      // kept, stubs
  HGS_HIP(hipMemcpyAsync(&host, t.res, sizeof(host), hipMemcpyDeviceToHost, s));
  HGS_HIP(hipMemcpyAsync(totals, t.block_sums + nblk, sizeof(totals), hipMemcpyDeviceToHost, s));
  HGS_HIP(wait_stream(s));
  first_bad_from_minima(host.first_bad, 4, report->first_bad);
  report->kept = (int64_t)totals[0];
  report->stubs = (int64_t)totals[1];
  static const char* const what[4] = {
      kLayoutChecks[0], kLayoutChecks[1], kLayoutChecks[2],
      "a kept node under a dropped parent (the boxes do not nest, or the extents grow downwards)"};
  if (fail_on_first_bad(report->first_bad, what, 4,
                        key ? "not a hierarchy that can be trimmed to views: %s (first offending node %d; "
                              "hgs.refit_hierarchy makes the boxes nest); nothing was written"
                            : "not a hierarchy that can be trimmed: %s (first offending node %d); nothing was written"))
    return HGS_ERR_INVALID;
  g_ht_plans.add(HtPlan{device, tmp, N, (int64_t)totals[0]});
  return HGS_OK;
}

int launch_hier_trim_apply(const hgs_hier_view& in, const hgs_hier_view& out, const void* tmp, int32_t* old_of_new,
                           int32_t* new_of_old, bool shs16, hipStream_t s) {
  const int64_t N = in.N, kept = out.N;
  Carver c(const_cast<void*>(tmp));
  const HtTmp t = carve_ht_tmp(c, N);
  const unsigned nblk = (unsigned)((N + kHtThreads - 1) / kHtThreads);
  hipLaunchKernelGGL(ht_maps_kernel, dim3(nblk), dim3(kHtThreads), 0, s, t.flags, t.block_sums, (int32_t)N, (int32_t)kept,
                     old_of_new, new_of_old);
  HGS_LAUNCH_CHECK("ht_maps", s, false);
  const uint32_t W = 3u * (uint32_t)in.M, S = shs16 ? W / 4u : 0u;
  hipLaunchKernelGGL(ht_gather_kernel, dim3((unsigned)((kept + kHtRows - 1) / kHtRows)), dim3(kHtThreads), 0, s,
                     HierRowsIn::of(in), HierRows::of(out), old_of_new, new_of_old, t.flags, (int32_t)kept, S, W);
  HGS_LAUNCH_CHECK("ht_gather", s, false);
  return HGS_OK;
}

}  // namespace hgs
