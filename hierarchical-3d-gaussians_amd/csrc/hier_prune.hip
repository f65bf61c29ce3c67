// Removing leaves from a hierarchy and re-merging their ancestors: the rule of hgs.hierarchy.prune_hierarchy (the spec)
// on the device, in two calls.  This project's own rule.
//
//   rule       a leaf (count_children == 0) is REMOVED iff a criterion holds (float32 comparisons: its mean inside one
//              of up to 16 closed boxes, outside a keep box, alpha not >= a floor, a log-scale not <= a ceiling, a mask
//              byte); a leaf is ALIVE iff it is not removed, a node with children iff one of its children is; an alive
//              node with children is DIRTY iff one of its children is dead or dirty.  The alive nodes are written in
//              ascending old order, records renumbered, count_children = the surviving children (they stay contiguous);
//              leaves and clean nodes are bit copies; a dirty node's box is the union of its surviving children's final
//              boxes and its row the w-weighted moment match of their final float32 rows, deepest level first
//              (hier_merge_rule.h: the builder's merge generalised to k children); w is the weight the builder carries:
//              alpha s0 s1 s2 of a leaf's row, at a node with children the sum of its surviving children's weights.
//   plan       hp_plan_kernel: the plan walk of hier_levels.h, the one text hier_refit.hip runs too (the six checks, the
//              depth keys, the per-depth counts, the reduce tail), with the removal test at every leaf, whose verdict is
//              the leaf's flag byte; the host half of that header for what follows: sort_pairs32 (8 bits, stable)
//              gives the level lists; the FIRST host wait reads the checks and the level counts.  hp_mark_kernel, one
//              launch per depth from the deepest level with children up: one thread per node walks its children's flag
//              bytes and leaves its own, its first surviving child and the surviving count (in the sort's key arrays,
//              free by then).  hp_count_kernel: workgroup sums of the alive flags, the dirty and single-child counts;
//              hp_scan_kernel: the chained scan of common.h.  The SECOND host wait reads the kept count, the other
//              counts and the root's verdict.  Nothing has been written to any output at that point.
//   apply      asynchronous.  ht_maps_kernel and the row copy of hier_gather.h (the trimmer's, shared), with this rule's
//              record rewrite in hp_gather_kernel; then hp_remerge_kernel, one launch per depth, deepest first, over
//              that level's list: one thread per node, a dirty one unions its children's boxes and -- by the re-merge
//              mode -- recomputes its row: three walks over its k children (weights; mean and opacity; covariance),
//              moments in double, the eigen tail, then the SH row coefficient by coefficient.  Every alive node with
//              children, clean or dirty, sums its children's weights and leaves its own in tmp for its parent's launch;
//              a child's share waits in tmp between the walks (two doubles per output row in all).
//
// Every index followed has passed the checks (see hier_refit.hip).  A node's k scattered child rows are read by one
// thread: acceptable while the dirty set is the ancestors of what was removed; DESIGN.md section 7 f-21 has the cost
// when nearly every interior node is dirty.  Rows at index >= N of the input are not read; rows at index >= N' of the
// output are not written.
#include "hier_gather.h"
#include "hier_levels.h"
#include "hier_merge_rule.h"
#include "hier_nodes.h"
#include "lod_cut.h"           // the workgroup sums and the launcher of the chained scan

namespace hgs {
namespace {

constexpr int kHpThreads = kLevelThreads;
constexpr uint32_t kDirty = 2u;         // bit 1 of a node's flag byte (bit 0: kKeep of hier_gather.h = alive)

// Device half of the report, read back in one copy at each of the two waits.  tally: the leaves a criterion removed.
struct HpResult : LevelResult {
  uint32_t dirty;                    // alive nodes with a dead or dirty child
  uint32_t single;                   // alive nodes left with one child
};

// is the point x inside the closed box [lo, hi]?  (a NaN coordinate is never inside)
__device__ __forceinline__ bool hp_inside(const float x[3], const float lo[3], const float hi[3]) {
  return x[0] >= lo[0] && x[0] <= hi[0] && x[1] >= lo[1] && x[1] <= hi[1] && x[2] >= lo[2] && x[2] <= hi[2];
}

// The removal test of leaf i: float32 comparisons only.
__device__ __forceinline__ bool hp_removed(const HierRowsIn& in, int64_t i, const hgs_hier_prune_args& a,
                                           const uint8_t* __restrict__ remove) {
  bool r = remove != nullptr && remove[i] != 0;
  if (a.remove_boxes > 0 || a.use_keep_box) {
    const float x[3] = {in.xyz[i * 3 + 0], in.xyz[i * 3 + 1], in.xyz[i * 3 + 2]};
    for (int b = 0; b < a.remove_boxes; ++b) r = r || hp_inside(x, a.remove_lo[b], a.remove_hi[b]);
    if (a.use_keep_box) r = r || !hp_inside(x, a.keep_lo, a.keep_hi);
  }
  if (a.use_min_opacity) r = r || !(in.alpha[i] >= a.min_opacity);
  if (a.use_max_scale) {
    const float L = a.log_max_scale;    // not (max_k ls_k <= L), a NaN log-scale included
    r = r || !(in.log_scales[i * 3 + 0] <= L && in.log_scales[i * 3 + 1] <= L && in.log_scales[i * 3 + 2] <= L);
  }
  return r;
}

// One thread per node, kLevelPlanBlocks workgroups at most that walk the nodes in strides: the plan walk of hier_levels.h
// (the checks, the depth as the sort key, the per-depth counts, the children sum) with the removed leaves as its tally:
// at a leaf the removal test, flags[i] = alive.  A node with children gets its flag from hp_mark_kernel.
__global__ __launch_bounds__(kHpThreads) void hp_plan_kernel(HierRowsIn in, int32_t N, hgs_hier_prune_args a,
                                                             const uint8_t* __restrict__ remove,
                                                             uint32_t* __restrict__ keys, uint8_t* __restrict__ flags,
                                                             HpResult* __restrict__ res) {
  __shared__ LevelPlanLds lds;
  level_plan_begin(lds);
  const int lane = threadIdx.x & 63;
  unsigned long long children = 0;
  uint32_t removed = 0;
  for (int64_t base = (int64_t)blockIdx.x * kHpThreads; base < N; base += (int64_t)gridDim.x * kHpThreads) {
    const int64_t i = base + threadIdx.x;
    uint32_t key = 0;
    bool counted = false;
    if (i < N) {
      int64_t cc;
      key = level_check_node(in.nodes, i, N, res->minima, children, &counted, &cc);
      uint8_t f = 0;
      if (cc == 0) {
        const bool r = hp_removed(in, i, a, remove);
        removed += r ? 1u : 0u;
        f = r ? 0 : (uint8_t)kKeep;
      }
      flags[i] = f;
      keys[i] = key;
    }
    level_count_depths(lds.bins, key, counted, lane);
  }
  level_plan_end(lds, children, removed, lane, res);
}

// One thread per node of one depth: alive and dirty from its children's flag bytes (written by the plan at leaves, by
// the previous launch at nodes with children), its first surviving child and the surviving count.
__global__ __launch_bounds__(kHpThreads) void hp_mark_kernel(const uint32_t* __restrict__ level, int32_t count,
                                                             const int32_t* __restrict__ nodes, uint8_t* flags,
                                                             int32_t* __restrict__ first_alive,
                                                             int32_t* __restrict__ surviving) {
  const int32_t t = (int32_t)(blockIdx.x * kHpThreads + threadIdx.x);
  if (t >= count) return;
  const int64_t id = level[t];
  const int64_t sc = nodes[id * kNodeInts + 5];
  const int32_t cc = nodes[id * kNodeInts + 6];
  if (cc <= 0) return;
  int32_t n = 0, first = 0;
  bool dirty = false;
  for (int32_t c = 0; c < cc; ++c) {
    const uint32_t f = flags[sc + c];
    const bool alive = (f & kKeep) != 0u;
    if (alive && n == 0) first = (int32_t)(sc + c);
    n += alive ? 1 : 0;
    dirty = dirty || !alive || (f & kDirty) != 0u;
  }
  flags[id] = (uint8_t)(n > 0 ? (kKeep | (dirty ? kDirty : 0u)) : 0u);
  first_alive[id] = first;
  surviving[id] = n;
}

// One thread per node: the workgroup's alive sum (for the scan), the dirty and the single-child counts.
__global__ __launch_bounds__(kHpThreads) void hp_count_kernel(const int32_t* __restrict__ nodes, int32_t N,
                                                              const uint8_t* __restrict__ flags,
                                                              const int32_t* __restrict__ surviving,
                                                              uint32_t* __restrict__ block_sums,
                                                              unsigned long long* __restrict__ chain,
                                                              HpResult* __restrict__ res) {
  __shared__ uint32_t s_cnt[2];
  clear_scan_chain(chain);
  if (threadIdx.x < 2) s_cnt[threadIdx.x] = 0;
  __syncthreads();
  const int64_t i = (int64_t)blockIdx.x * kHpThreads + threadIdx.x;
  uint32_t alive = 0, dirty = 0, single = 0;
  if (i < N) {
    const uint32_t f = flags[i];
    alive = (f & kKeep) ? 1u : 0u;
    dirty = (alive && (f & kDirty)) ? 1u : 0u;
    single = (alive && nodes[i * kNodeInts + 6] > 0 && surviving[i] == 1) ? 1u : 0u;
  }
  uint32_t d = dirty, g = single;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    d += __shfl_xor(d, off, 64);
    g += __shfl_xor(g, off, 64);
  }
  if ((threadIdx.x & 63) == 0) {
    if (d) atomicAdd(&s_cnt[0], d);
    if (g) atomicAdd(&s_cnt[1], g);
  }
  const uint32_t cnt[1] = {alive};
  uint32_t* const out[1] = {block_sums};
  block_totals<1>(cnt, out);          // (its barrier also orders the two LDS counts)
  if (threadIdx.x == 0) {
    if (s_cnt[0]) atomicAdd(&res->dirty, s_cnt[0]);
    if (s_cnt[1]) atomicAdd(&res->single, s_cnt[1]);
  }
}

// sums[0 .. n) scanned in place, sums[n] = the kept count
__global__ __launch_bounds__(1024) void hp_scan_kernel(uint32_t* __restrict__ sums, int n,
                                                       unsigned long long* __restrict__ chain, int c_off, int chunks) {
  (void)chained_scan_inplace(sums, n, chain, c_off, chunks);
}

// One workgroup per kHtRows output rows: the trimmer's row copy, and this rule's record rewrite.
__global__ __launch_bounds__(kHtThreads) void hp_gather_kernel(HierRowsIn in, HierRows out,
                                                               const int32_t* __restrict__ old_of_new,
                                                               const int32_t* __restrict__ new_of_old,
                                                               const int32_t* __restrict__ first_alive,
                                                               const int32_t* __restrict__ surviving, int32_t kept,
                                                               uint32_t S, uint32_t W) {
  __shared__ int32_t src[kHtRows];
  const int64_t r0 = (int64_t)blockIdx.x * kHtRows;
  const uint32_t rows = ht_stage_rows(src, old_of_new, r0, kept);
  ht_copy_tensors(in, out, src, r0, rows, S, W);
  // the node records, one thread per int: depth, count_leafs and count_merged kept; parent, start and start_children
  // renumbered (the first SURVIVING child); count_children = the surviving children; a leaf keeps its own
  int32_t* o = out.nodes + r0 * kNodeInts;
  const uint32_t L = rows * kNodeInts;
  for (uint32_t u = threadIdx.x; u < L; u += kHtThreads) {
    const uint32_t jl = u / kNodeInts, k = u - jl * kNodeInts;
    const int64_t i = src[jl];
    const int32_t* nd = in.nodes + i * kNodeInts;
    const int32_t cc = nd[6];
    int32_t v;
    switch (k) {
      case 1: v = i == 0 ? -1 : new_of_old[nd[1]]; break;
      case 2: v = (int32_t)(r0 + jl); break;
      case 5: v = cc > 0 ? new_of_old[first_alive[i]] : nd[5]; break;
      case 6: v = cc > 0 ? surviving[i] : cc; break;
      default: v = nd[k]; break;
    }
    o[u] = v;
  }
}

// One thread per node of one depth of the INPUT's level list (old ids; a dead node and a leaf leave at once): a dirty
// node's box, and by `mode` its row, from its children in the output -- copied by the gather or written by the previous
// launch.  W = 3 M floats per SH row.
__global__ __launch_bounds__(kHpThreads) void hp_remerge_kernel(const uint32_t* __restrict__ level, int32_t count,
                                                                const uint8_t* __restrict__ flags,
                                                                const int32_t* __restrict__ new_of_old, HierRows out,
                                                                uint32_t W, int32_t mode, double* __restrict__ wts,
                                                                double* __restrict__ shr) {
  const int32_t t = (int32_t)(blockIdx.x * kHpThreads + threadIdx.x);
  if (t >= count) return;
  const int64_t old = level[t];
  const uint32_t fl = flags[old];
  if (!(fl & kKeep)) return;
  const int64_t id = new_of_old[old];
  const int32_t cc = out.nodes[id * kNodeInts + 6];
  if (cc <= 0) return;
  const int64_t sc = out.nodes[id * kNodeInts + 5];
  const bool dirty = (fl & kDirty) != 0u;
  // the union of the children's final boxes; boxes[n,1,3] stays (the gather copied it)
  if (dirty) level_box_from_children(out.boxes, id, sc, cc, out.boxes);
  if (mode == HGS_HIER_PRUNE_REMERGE_NONE) return;
  // ---- walk 1, at clean nodes too: the weights the builder carries.  A leaf weighs alpha s0 s1 s2 of its row, a node
  // with children the clamped sum of its surviving children's weights (its own thread left it in wts one launch ago).
  double sum = 0.0;
  for (int32_t c = 0; c < cc; ++c) {
    const int64_t r = sc + c;
    double w;
    if (out.nodes[r * kNodeInts + 6] == 0) {
      const double ls[3] = {out.log_scales[r * 3 + 0], out.log_scales[r * 3 + 1], out.log_scales[r * 3 + 2]};
      w = merge_child_weight((double)out.alpha[r], ls);
      wts[r] = w;
    } else {
      w = wts[r];
    }
    sum += w;
  }
  const double ws = merge_weight_sum(sum);
  wts[id] = ws;
  if (!(mode == HGS_HIER_PRUNE_REMERGE_ALL || dirty)) return;
  // ---- walk 2: the mean and the opacity
  double mu[3] = {0.0, 0.0, 0.0}, al = 0.0;
  for (int32_t c = 0; c < cc; ++c) {
    const int64_t r = sc + c;
    const double f = wts[r] / ws;
    shr[r] = f;
    const double x[3] = {out.xyz[r * 3 + 0], out.xyz[r * 3 + 1], out.xyz[r * 3 + 2]};
    merge_add_mean(f, x, mu);
    al += f * (double)out.alpha[r];
  }
  // ---- walk 3: the covariance
  double cv[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int32_t c = 0; c < cc; ++c) {
    const int64_t r = sc + c;
    const double x[3] = {out.xyz[r * 3 + 0], out.xyz[r * 3 + 1], out.xyz[r * 3 + 2]};
    const double ls[3] = {out.log_scales[r * 3 + 0], out.log_scales[r * 3 + 1], out.log_scales[r * 3 + 2]};
    const float4 qf = reinterpret_cast<const float4*>(out.rots)[r];
    const double q[4] = {qf.x, qf.y, qf.z, qf.w};
    double cc6[6];
    merge_child_cov(q, ls, cc6);
    merge_add_cov(shr[r], x, cc6, mu, cv);
  }
#pragma unroll
  for (int a = 0; a < 3; ++a) out.xyz[id * 3 + a] = (float)mu[a];
  out.alpha[id] = merge_alpha(al);
  float ls[3], q[4];
  merge_cov_to_row(cv, ls, q);
#pragma unroll
  for (int a = 0; a < 3; ++a) out.log_scales[id * 3 + a] = ls[a];
  reinterpret_cast<float4*>(out.rots)[id] = make_float4(q[0], q[1], q[2], q[3]);
  // ---- the SH row: f-weighted averages, coefficient by coefficient (4-byte pieces: any alignment of the base)
  const float* ksh = out.shs + sc * W;
  float* osh = out.shs + id * W;
  for (uint32_t j = 0; j < W; ++j) {
    double acc = 0.0;
    for (int32_t c = 0; c < cc; ++c) acc += shr[sc + c] * (double)ksh[(int64_t)c * W + j];
    osh[j] = (float)acc;
  }
}

// The level lists, and behind them this tool's own.  After the sort `keys` holds every node's first surviving child and
// `keys_sorted` its count of surviving children.
struct HpTmp : SumsTmp, LevelListsTmp<HpResult> {
  uint8_t* flags;          // [N]
  double* wts;             // [N] the weight a node carries: the sum over its surviving leaves (apply; by OUTPUT row)
  double* shr;             // [N] a child's share of its parent's weight (apply; by OUTPUT row)
};

HpTmp carve_hp_tmp(Carver& c, int64_t N) {
  HpTmp t;
  carve_level_lists(c, N, t);
  t.flags = c.take<uint8_t>((size_t)N);
  t.wts = c.take<double>((size_t)N);
  t.shr = c.take<double>((size_t)N);
  static_cast<SumsTmp&>(t) = carve_sums(c, (size_t)N, false);
  return t;
}

// What the last successful plan on (device, tmp) found: apply checks its sizes against it on the host and takes the
// level sizes from it.
struct HpPlan {
  int device;
  const void* tmp;
  int64_t N, kept;
  int levels;
  uint32_t counts[kLevels];
};
PlanBook<HpPlan> g_hp_plans;

}  // namespace

size_t hier_prune_tmp_bytes(int64_t N) {
  Carver c(nullptr);
  carve_hp_tmp(c, N);
  return c.bytes(0);   // tmp is required to be kAlign-aligned: no slack
}

bool hier_prune_planned(int device, const void* tmp, int64_t* N, int64_t* kept) {
  HpPlan p;
  if (!g_hp_plans.find(device, tmp, &p)) return false;
  *N = p.N;
  *kept = p.kept;
  return true;
}

int launch_hier_prune_plan(const hgs_hier_view& in, const hgs_hier_prune_args& args, const uint8_t* remove, void* tmp,
                           hgs_hier_prune_report* report, hipStream_t s, int device) {
  g_hp_plans.forget(device, tmp);
  const int64_t N = in.N;
  Carver c(tmp);
  const HpTmp t = carve_hp_tmp(c, N);
  int32_t* const first_alive = reinterpret_cast<int32_t*>(t.keys);
  int32_t* const surviving = reinterpret_cast<int32_t*>(t.keys_sorted);
  // ---- checks, keys, counts, the leaves' verdicts; the level lists
  int rc = clear_level_result(t.res, s);
  if (rc) return rc;
  const dim3 grid((unsigned)((N + kHpThreads - 1) / kHpThreads)), block(kHpThreads);
  hipLaunchKernelGGL(hp_plan_kernel, level_plan_grid(N), block, 0, s, HierRowsIn::of(in), (int32_t)N, args, remove, t.keys,
                     t.flags, t.res);
  HGS_LAUNCH_CHECK("hp_plan", s, false);
  if ((rc = sort_level_lists(t, N, s))) return rc;
  // ---- the first host wait
  HpResult host;
  HGS_HIP(hipMemcpyAsync(&host, t.res, sizeof(host), hipMemcpyDeviceToHost, s));
  HGS_HIP(wait_stream(s));
  first_bad_from_minima(host.minima, kLevelChecks, report->first_bad);
  const int levels = level_count(host.counts);
  report->levels = levels;
  report->children_sum = (int64_t)host.children_sum;
  report->removed_leaves = (int64_t)host.tally;
  if ((rc = level_plan_verdict(report->first_bad, nullptr, report->children_sum, N, "pruned"))) return rc;
  // ---- alive and dirty, one launch per level, bottom-up
  rc = launch_levels_up(hp_mark_kernel, "hp_mark", s, t.order, host.counts, levels, N, in.nodes, t.flags, first_alive, surviving);
  if (rc) return rc;
  // ---- the alive sums and their scan, the counts
  const int nblk = (int)grid.x;
  hipLaunchKernelGGL(hp_count_kernel, grid, block, 0, s, in.nodes, (int32_t)N, t.flags, surviving, t.block_sums, t.chain,
                     t.res);
  HGS_LAUNCH_CHECK("hp_count", s, false);
  rc = launch_scan_chunks(hp_scan_kernel, "hp_scan", nblk, s, t.block_sums, nblk, t.chain);
  if (rc) return rc;
  // ---- the second host wait
  uint32_t kept = 0;
  uint8_t root = 0;
  HGS_HIP(hipMemcpyAsync(&host, t.res, sizeof(host), hipMemcpyDeviceToHost, s));
  HGS_HIP(hipMemcpyAsync(&kept, t.block_sums + nblk, sizeof(kept), hipMemcpyDeviceToHost, s));
  HGS_HIP(hipMemcpyAsync(&root, t.flags, sizeof(root), hipMemcpyDeviceToHost, s));
  HGS_HIP(wait_stream(s));
  report->kept = (int64_t)kept;
  report->dead = N - (int64_t)kept;
  report->dirty = (int64_t)host.dirty;
  report->single_child = (int64_t)host.single;
  report->root_dead = (root & kKeep) ? 0 : 1;
  if (report->root_dead) {
    set_error("every leaf would be removed (%lld of %lld nodes are leaves a criterion removes); nothing was written",
              (long long)report->removed_leaves, (long long)N);
    return HGS_ERR_INVALID;
  }
  HpPlan p;
  p.device = device;
  p.tmp = tmp;
  p.N = N;
  p.kept = (int64_t)kept;
  p.levels = levels;
  for (int d = 0; d < kLevels; ++d) p.counts[d] = host.counts[d];
  g_hp_plans.add(p);
  return HGS_OK;
}

int launch_hier_prune_apply(const hgs_hier_view& in, const hgs_hier_view& out, const void* tmp, int32_t remerge,
                            int32_t* old_of_new, int32_t* new_of_old, bool shs16, hipStream_t s, int device) {
  HpPlan p;
  if (!g_hp_plans.find(device, tmp, &p)) { set_error("no successful hgs_hier_prune_plan on this device and tmp"); return HGS_ERR_INVALID; }
  const int64_t N = in.N, kept = out.N;
  Carver c(const_cast<void*>(tmp));
  const HpTmp t = carve_hp_tmp(c, N);
  const int32_t* const first_alive = reinterpret_cast<const int32_t*>(t.keys);
  const int32_t* const surviving = reinterpret_cast<const int32_t*>(t.keys_sorted);
  const unsigned nblk = (unsigned)((N + kHtThreads - 1) / kHtThreads);
  hipLaunchKernelGGL(ht_maps_kernel, dim3(nblk), dim3(kHtThreads), 0, s, t.flags, t.block_sums, (int32_t)N, (int32_t)kept,
                     old_of_new, new_of_old);
  HGS_LAUNCH_CHECK("hp_maps", s, false);
  const uint32_t W = 3u * (uint32_t)in.M, S = shs16 ? W / 4u : 0u;
  hipLaunchKernelGGL(hp_gather_kernel, dim3((unsigned)((kept + kHtRows - 1) / kHtRows)), dim3(kHtThreads), 0, s,
                     HierRowsIn::of(in), HierRows::of(out), old_of_new, new_of_old, first_alive, surviving, (int32_t)kept, S, W);
  HGS_LAUNCH_CHECK("hp_gather", s, false);
  // ---- boxes and rows of the dirty nodes, one launch per level, bottom-up.  Nothing to do where nothing died and no row
  // is asked for again.
  if (kept == N && remerge != HGS_HIER_PRUNE_REMERGE_ALL) return HGS_OK;
  return launch_levels_up(hp_remerge_kernel, "hp_remerge", s, t.order, p.counts, p.levels, N, t.flags, new_of_old,
                          HierRows::of(out), W, remerge, t.wts, t.shr);
}

}  // namespace hgs
