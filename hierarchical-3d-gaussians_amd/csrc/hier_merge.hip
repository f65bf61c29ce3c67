// Consolidation of chunk hierarchies: the rule of hgs.hierarchy.merge_hierarchies (the spec) applied to chunks trimmed
// to their first N rows, on the device, one chunk at a time.
//
//   layout     node 0 = a new root whose k children are the chunk roots (nodes 1..k); chunk c's node 0 lands at 1 + c,
//              its nodes 1..N-1 at base_c .. base_c + N - 2 (base_0 = 1 + k, base_{c+1} = base_c + N_c - 1)
//   rows       attribute rows and boxes are copied into place (hipMemcpyAsync, host or device source): no kernel
//   nodes      hm_nodes_kernel: one thread per node remaps depth / parent / start / start_children and validates the
//              chunk in the same pass (hier_nodes.h's checks: first offending node per check, the children counts summed)
//   root       hm_root_kernel: one wave computes the root row and box from rows 1..k in double, as the spec
//
// Rows at index >= N of a chunk (a skybox tail appended after the node rows) are not read.
#include "hier_nodes.h"

namespace hgs {
namespace {

constexpr int kHmThreads = 256;
constexpr int kHmWaves = kHmThreads / 64;
constexpr int kChecks = 3;

// Device half of the report: the first offending node per check as an unsigned minimum (kNone = none), and the sum of
// the children counts.
struct HmResult {
  uint32_t first_bad[4];
  unsigned long long children_sum;
};

__device__ __forceinline__ int64_t wave_sum(int64_t v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// One thread per chunk node: the remapped row into the merged array, and the checks of the row.
__global__ __launch_bounds__(kHmThreads) void hm_nodes_kernel(const int32_t* __restrict__ nodes, int32_t N,
                                                              int32_t root_slot, int64_t base,
                                                              int32_t* __restrict__ out, HmResult* __restrict__ res) {
  __shared__ int64_t part[kHmWaves];
  const int64_t i = (int64_t)blockIdx.x * kHmThreads + threadIdx.x;
  int64_t cc = 0;
  if (i < N) {
    const int32_t* nd = nodes + i * kNodeInts;
    const int32_t depth = nd[0], parent = nd[1], leafs = nd[3], merged = nd[4], sc = nd[5];
    cc = nd[6];
    const uint32_t v = node_layout(nodes, i, N);
    if (v & kBadRow) atomicMin(&res->first_bad[0], (uint32_t)i);
    if (v & kBadChildren) atomicMin(&res->first_bad[1], (uint32_t)i);
    if (v & kBadParent) atomicMin(&res->first_bad[2], (uint32_t)i);
    auto remap = [&](int64_t id) { return (int32_t)(id == 0 ? (int64_t)root_slot : base + id - 1); };
    const int64_t id = remap(i);
    int32_t* o = out + id * kNodeInts;
    o[0] = (int32_t)((int64_t)depth + 1);
    o[1] = parent < 0 ? 0 : remap(parent);
    o[2] = (int32_t)id;
    o[3] = leafs;
    o[4] = merged;
    o[5] = cc > 0 ? remap(sc) : 0;
    o[6] = (int32_t)cc;
  }
  cc = wave_sum(cc);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = cc;
  __syncthreads();
  if (threadIdx.x == 0) {
    int64_t s = 0;
#pragma unroll
    for (int w = 0; w < kHmWaves; ++w) s += part[w];
    if (s != 0) atomicAdd(&res->children_sum, (unsigned long long)s);
  }
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}
__device__ __forceinline__ float wave_min(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = fminf(v, __shfl_xor(v, off, 64));
  return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, 64));
  return v;
}

// the spec's weight of chunk root r: clamp_min(alpha * s0 * s1 * s2, 1e-30), s = exp(log_scales) in double
__device__ __forceinline__ double root_weight(const HierRows& m, int64_t r) {
  const double s0 = exp((double)m.log_scales[r * 3 + 0]), s1 = exp((double)m.log_scales[r * 3 + 1]),
               s2 = exp((double)m.log_scales[r * 3 + 2]);
  return fmax((double)m.alpha[r] * ((s0 * s1) * s2), 1e-30);
}

// One wave: node 0's row and box from the chunk roots at rows 1..k (merge_hierarchies' formulas, in double; the sums
// run in another order than torch's, so the row agrees to float32 rounding).
__global__ __launch_bounds__(64) void hm_root_kernel(HierRows m, int32_t k, int32_t M) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x;
  double W = 0.0;
  for (int c = lane; c < k; c += 64) W += root_weight(m, 1 + c);
  W = wave_sum(W);
  // mean and opacity: f-weighted sums, f = w / W
  double mu[3] = {0.0, 0.0, 0.0}, al = 0.0;
  for (int c = lane; c < k; c += 64) {
    const int64_t r = 1 + c;
    const double f = root_weight(m, r) / W;
#pragma unroll
    for (int a = 0; a < 3; ++a) mu[a] += f * (double)m.xyz[r * 3 + a];
    al += f * (double)m.alpha[r];
  }
#pragma unroll
  for (int a = 0; a < 3; ++a) mu[a] = wave_sum(mu[a]);
  al = wave_sum(al);
  // axis-aligned second moments: diag(R diag(s^2) R^T) of the normalised quaternion + the spread of the means; box union
  double var[3] = {0.0, 0.0, 0.0};
  float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
  for (int c = lane; c < k; c += 64) {
    const int64_t r = 1 + c;
    const double f = root_weight(m, r) / W;
    double q[4] = {m.rots[r * 4 + 0], m.rots[r * 4 + 1], m.rots[r * 4 + 2], m.rots[r * 4 + 3]};
    const double qn = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
#pragma unroll
    for (int j = 0; j < 4; ++j) q[j] /= qn;
    const double qr = q[0], qx = q[1], qy = q[2], qz = q[3];
    const double R[3][3] = {{1 - 2 * (qy * qy + qz * qz), 2 * (qx * qy - qr * qz), 2 * (qx * qz + qr * qy)},
                            {2 * (qx * qy + qr * qz), 1 - 2 * (qx * qx + qz * qz), 2 * (qy * qz - qr * qx)},
                            {2 * (qx * qz - qr * qy), 2 * (qy * qz + qr * qx), 1 - 2 * (qx * qx + qy * qy)}};
    double s2[3];
#pragma unroll
    for (int b = 0; b < 3; ++b) {
      const double s = exp((double)m.log_scales[r * 3 + b]);
      s2[b] = s * s;
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const double v = R[a][0] * R[a][0] * s2[0] + R[a][1] * R[a][1] * s2[1] + R[a][2] * R[a][2] * s2[2];
      const double d = (double)m.xyz[r * 3 + a] - mu[a];
      var[a] += f * (v + d * d);
      mn[a] = fminf(mn[a], m.boxes[r * 8 + a]);
      mx[a] = fmaxf(mx[a], m.boxes[r * 8 + 4 + a]);
    }
  }
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    var[a] = wave_sum(var[a]);
    mn[a] = wave_min(mn[a]);
    mx[a] = wave_max(mx[a]);
  }
  // SH: one lane per coefficient, the chunks in order
  for (int j = lane; j < 3 * M; j += 64) {
    double s = 0.0;
    for (int c = 0; c < k; ++c) {
      const int64_t r = 1 + c;
      s += (root_weight(m, r) / W) * (double)m.shs[r * 3 * M + j];
    }
    m.shs[j] = (float)s;
  }
  if (lane == 0) {
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      m.xyz[a] = (float)mu[a];
      m.log_scales[a] = (float)log(sqrt(fmax(var[a], 1e-12)));
    }
    reinterpret_cast<float4*>(m.rots)[0] = make_float4(1.0f, 0.0f, 0.0f, 0.0f);
    m.alpha[0] = (float)fmin(fmax(al, 0.0), 1.0);
    const float e = fmaxf(fmaxf(mx[0] - mn[0], mx[1] - mn[1]), mx[2] - mn[2]);
    reinterpret_cast<float4*>(m.boxes)[0] = make_float4(mn[0], mn[1], mn[2], e);
    reinterpret_cast<float4*>(m.boxes)[1] = make_float4(mx[0], mx[1], mx[2], 0.0f);
    const int32_t root[kNodeInts] = {0, -1, 0, 0, 1, 1, k};
#pragma unroll
    for (int j = 0; j < kNodeInts; ++j) m.nodes[j] = root[j];
  }
}

// merged rows [dst, dst + n) <- chunk rows [src, src + n), `bytes` per row (any memory on either side)
int copy_rows(void* merged, const void* chunk, int64_t dst, int64_t src, int64_t n, size_t bytes, hipStream_t s) {
  if (n <= 0) return HGS_OK;
  HGS_HIP(hipMemcpyAsync(static_cast<char*>(merged) + dst * bytes, static_cast<const char*>(chunk) + src * bytes,
                         n * bytes, hipMemcpyDefault, s));
  return HGS_OK;
}

}  // namespace

int launch_hier_merge_place(const hgs_hier_view& chunk, int32_t index, int64_t base, const hgs_hier_view& merged,
                            void* tmp, hgs_hier_merge_report* report, hipStream_t s) {
  const int64_t N = chunk.N;
  const size_t M = (size_t)chunk.M;
  const int64_t slot = 1 + (int64_t)index;
  // ---- attribute rows and boxes: row 0 -> the root's child slot, rows 1..N-1 -> base ..
  struct { void* dst; const void* src; size_t bytes; } parts[] = {
      {merged.xyz, chunk.xyz, 12}, {merged.shs, chunk.shs, 12 * M}, {merged.alpha, chunk.alpha, 4},
      {merged.log_scales, chunk.log_scales, 12}, {merged.rots, chunk.rots, 16}, {merged.boxes, chunk.boxes, 32}};
  for (auto& p : parts) {
    int rc = copy_rows(p.dst, p.src, slot, 0, 1, p.bytes, s);
    if (!rc) rc = copy_rows(p.dst, p.src, base, 1, N - 1, p.bytes, s);
    if (rc) return rc;
  }
  // ---- nodes: remap + validate
  HmResult* res = static_cast<HmResult*>(tmp);
  HGS_HIP(hipMemsetAsync(res->first_bad, 0xff, sizeof(res->first_bad), s));
  HGS_HIP(hipMemsetAsync(&res->children_sum, 0, sizeof(res->children_sum), s));
  const unsigned blocks = (unsigned)((N + kHmThreads - 1) / kHmThreads);
  hipLaunchKernelGGL(hm_nodes_kernel, dim3(blocks), dim3(kHmThreads), 0, s, chunk.nodes, (int32_t)N, (int32_t)slot, base,
                     merged.nodes, res);
  HGS_LAUNCH_CHECK("hm_nodes", s, false);
  // ---- the report: one read per chunk
  HmResult host;
  HGS_HIP(hipMemcpyAsync(&host, res, sizeof(host), hipMemcpyDeviceToHost, s));
  HGS_HIP(hipStreamSynchronize(s));
  first_bad_from_minima(host.first_bad, kChecks, report->first_bad);   // (a chunk that fails is the caller's to refuse)
  report->reserved = 0;
  report->children_sum = (int64_t)host.children_sum;
  return HGS_OK;
}

int launch_hier_merge_root(const hgs_hier_view& merged, int32_t k, hipStream_t s) {
  hipLaunchKernelGGL(hm_root_kernel, dim3(1), dim3(64), 0, s, HierRows::of(merged), k, merged.M);
  HGS_LAUNCH_CHECK("hm_root", s, false);
  return HGS_OK;
}

}  // namespace hgs
