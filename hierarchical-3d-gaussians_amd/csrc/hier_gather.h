// What the two tools that make a smaller copy of a hierarchy share (hier_trim.hip, hier_prune.hip), each ONCE: the maps
// from a per-node keep bit and the scanned workgroup sums, the staging of a gather workgroup's source rows, the copy of
// the six tensors' rows in pieces of 16 or 4 bytes, and the book of successful plans that the apply calls look up.
// The record rewrite is each rule's own and stays with its gather kernel.
#pragma once
#include "hier_nodes.h"
#include "lod_cut.h"   // block_exclusive_offset

#include <mutex>
#include <vector>

namespace hgs {
namespace {

constexpr int kHtThreads = 256;
constexpr int kHtRows = 128;            // output rows per workgroup of a gather
constexpr uint32_t kKeep = 1u;          // bit 0 of a node's flag byte: the node is in the output

// One thread per old node: its new index from the scanned workgroup sums, both maps.
__global__ __launch_bounds__(kHtThreads) void ht_maps_kernel(const uint8_t* __restrict__ flags,
                                                             const uint32_t* __restrict__ block_sums, int32_t N,
                                                             int32_t kept, int32_t* __restrict__ old_of_new,
                                                             int32_t* __restrict__ new_of_old) {
  const int64_t i = (int64_t)blockIdx.x * kHtThreads + threadIdx.x;
  const bool keep = i < N && (flags[i] & kKeep) != 0u;
  const uint32_t pos = block_sums[blockIdx.x] + block_exclusive_offset(keep ? 1u : 0u);
  if (i < N) {
    new_of_old[i] = keep ? (int32_t)pos : -1;
    if (keep && pos < (uint32_t)kept) old_of_new[pos] = (int32_t)i;
  }
}

// rows [r0, r0 + rows) of a tensor of `ppr` pieces of type T per row <- the rows src[0 .. rows) of `in`
template <typename T>
__device__ __forceinline__ void ht_copy_rows(T* __restrict__ out, const T* __restrict__ in, const int32_t* src,
                                             int64_t r0, uint32_t rows, uint32_t ppr) {
  T* o = out + r0 * ppr;
  const uint32_t L = rows * ppr;
#pragma unroll 4
  for (uint32_t u = threadIdx.x; u < L; u += kHtThreads) {
    const uint32_t jl = u / ppr, k = u - jl * ppr;
    o[u] = in[(int64_t)src[jl] * ppr + k];
  }
}

// A gather workgroup's output rows are [r0, r0 + rows), rows <= kHtRows (fewer at the end of the `kept` rows): their
// source rows from old_of_new into src[kHtRows] (LDS), behind a barrier.  -> rows
__device__ __forceinline__ uint32_t ht_stage_rows(int32_t* src, const int32_t* __restrict__ old_of_new, int64_t r0,
                                                  int32_t kept) {
  const uint32_t rows = (uint32_t)min((int64_t)kHtRows, (int64_t)kept - r0);
  if (threadIdx.x < rows) src[threadIdx.x] = old_of_new[r0 + threadIdx.x];
  __syncthreads();
  return rows;
}

// The six tensors that are copied bit for bit, for the rows src[0 .. rows) staged in LDS.  S: 16-byte pieces of an shs
// row (0: shs goes in W 4-byte pieces).
__device__ __forceinline__ void ht_copy_tensors(HierRowsIn in, HierRows out, const int32_t* src, int64_t r0,
                                                uint32_t rows, uint32_t S, uint32_t W) {
  if (S) ht_copy_rows(reinterpret_cast<float4*>(out.shs), reinterpret_cast<const float4*>(in.shs), src, r0, rows, S);
  else ht_copy_rows(out.shs, in.shs, src, r0, rows, W);
  ht_copy_rows(reinterpret_cast<float4*>(out.boxes), reinterpret_cast<const float4*>(in.boxes), src, r0, rows, 2u);
  ht_copy_rows(reinterpret_cast<float4*>(out.rots), reinterpret_cast<const float4*>(in.rots), src, r0, rows, 1u);
  ht_copy_rows(out.xyz, in.xyz, src, r0, rows, 3u);
  ht_copy_rows(out.log_scales, in.log_scales, src, r0, rows, 3u);
  ht_copy_rows(out.alpha, in.alpha, src, r0, rows, 1u);
}

// What the last successful plan on each (device, tmp) found: the apply call checks its sizes against it on the host.
// Plan: a record that begins with `int device; const void* tmp;`.  At most 64 records, oldest first.
template <typename Plan>
struct PlanBook {
  std::mutex mutex;
  std::vector<Plan> plans;

  // a plan call begins with it: whatever it finds, the plan before it on this (device, tmp) no longer holds
  void forget(int device, const void* tmp) {
    std::lock_guard<std::mutex> lock(mutex);
    for (size_t k = 0; k < plans.size(); ++k)
      if (plans[k].device == device && plans[k].tmp == tmp) { plans.erase(plans.begin() + k); break; }
  }
  bool find(int device, const void* tmp, Plan* out) {
    std::lock_guard<std::mutex> lock(mutex);
    for (const Plan& p : plans)
      if (p.device == device && p.tmp == tmp) { *out = p; return true; }
    return false;
  }
  void add(const Plan& p) {
    std::lock_guard<std::mutex> lock(mutex);
    if (plans.size() >= 64) plans.erase(plans.begin());
    plans.push_back(p);
  }
};

}  // namespace
}  // namespace hgs
