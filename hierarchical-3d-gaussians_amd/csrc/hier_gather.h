// What the two tools that make a smaller copy of a hierarchy share (hier_trim.hip, hier_prune.hip), each ONCE: the maps
// from a per-node keep bit and the scanned workgroup sums, and the copy of one tensor's rows in pieces of 16 or 4 bytes.
// The record rewrite is each rule's own and stays with its gather kernel.
#pragma once
#include "hier_nodes.h"
#include "lod_cut.h"   // block_exclusive_offset

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

}  // namespace
}  // namespace hgs
