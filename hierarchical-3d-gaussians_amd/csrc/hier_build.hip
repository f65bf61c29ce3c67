// Hierarchy construction: a balanced binary BVH over Morton-sorted leaves, interior nodes holding the moment-matched
// merge of their two children -- the rule of hgs.hierarchy.build_hierarchy (the spec), built on the device.
//
//   bounds     scene min / max (order-preserving integer atomics on the float bits: exact)
//   morton     10 bits per axis, computed in double with numpy's operation sequence (bit-identical codes)
//   sort       the library's stable LSD radix sort (radix_sort.hip), value = row index: numpy's stable argsort
//   topology   top-down, one launch per level: the threads of level d - 1 write the rows of their children
//   merge      bottom-up, one launch per level: moments in double, SH / opacity as weighted averages, box union,
//              3x3 symmetric Jacobi eigen-solve for the interior rotation and scales (one canonical parametrisation
//              of the eigen-frame: ascending eigenvalues, each axis' largest component positive, proper rotation)
//
// Level sizes are host arithmetic (no device round trip).  A range [l, h) splits at (l + h) / 2, so the ranges of one
// level take two lengths {k, k + 1} with k = P >> d.  With D = floor(log2 P): levels 0 .. D - 1 are all interior
// (2^d nodes), level D has 2^D nodes of length 1 or 2 (c = P - 2^D of length 2) and level D + 1 the 2c leaves under
// them.  On level D the ranges tile [0, P) in order, so the number of length-2 nodes in front of node i is l_i - i:
// its children's place, no prefix sum.
#include "hier_merge_rule.h"   // the eigen tail of the merge, shared with hier_prune.hip
#include "hier_nodes.h"

namespace hgs {
namespace {

constexpr int kMomDoubles = 10;     // mean xyz, covariance xx xy xz yy yz zz, weight w = alpha * s0 * s1 * s2
constexpr int kShFloats = 48;       // output SH rows are padded to 16 coefficients
constexpr int kHbThreads = 256;

__device__ __forceinline__ uint32_t ordered_bits(float f) {
  const uint32_t u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float from_ordered_bits(uint32_t e) {
  return __uint_as_float((e & 0x80000000u) ? (e & 0x7fffffffu) : ~e);
}

// words[0..2] = ordered bits of the minimum per axis, words[3..5] = complement of those of the maximum (both atomicMin;
// the caller fills the six words with 0xff first)
__global__ __launch_bounds__(kHbThreads) void hb_bounds_kernel(const float* __restrict__ xyz, int32_t P,
                                                               uint32_t* __restrict__ words) {
  uint32_t lo[3] = {~0u, ~0u, ~0u}, nhi[3] = {~0u, ~0u, ~0u};
  for (int64_t i = (int64_t)blockIdx.x * kHbThreads + threadIdx.x; i < P; i += (int64_t)gridDim.x * kHbThreads) {
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const uint32_t e = ordered_bits(xyz[i * 3 + a]);
      lo[a] = min(lo[a], e);
      nhi[a] = min(nhi[a], ~e);
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      lo[a] = min(lo[a], (uint32_t)__shfl_xor((int)lo[a], off, 64));
      nhi[a] = min(nhi[a], (uint32_t)__shfl_xor((int)nhi[a], off, 64));
    }
  }
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      atomicMin(&words[a], lo[a]);
      atomicMin(&words[3 + a], nhi[a]);
    }
  }
}

__device__ __forceinline__ uint32_t spread10(uint32_t v) {
  v = (v | (v << 16)) & 0x030000FFu;
  v = (v | (v << 8)) & 0x0300F00Fu;
  v = (v | (v << 4)) & 0x030C30C3u;
  v = (v | (v << 2)) & 0x09249249u;
  return v;
}

// numpy: clip((x - lo) / maximum(hi - lo, 1e-12) * 1023, 0, 1023).astype(uint64), every step a rounded double op
__device__ __forceinline__ uint32_t quantise(float x, float lo, float hi) {
#pragma clang fp contract(off)
  const double den = fmax((double)hi - (double)lo, 1e-12);
  double q = ((double)x - (double)lo) / den * 1023.0;
  q = fmin(fmax(q, 0.0), 1023.0);
  return (uint32_t)q;
}

__global__ __launch_bounds__(kHbThreads) void hb_morton_kernel(const float* __restrict__ xyz, int32_t P,
                                                               const uint32_t* __restrict__ words,
                                                               uint32_t* __restrict__ keys) {
  const int64_t i = (int64_t)blockIdx.x * kHbThreads + threadIdx.x;
  if (i >= P) return;
  uint32_t code = 0;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const float lo = from_ordered_bits(words[a]), hi = from_ordered_bits(~words[3 + a]);
    code |= spread10(quantise(xyz[i * 3 + a], lo, hi)) << a;
  }
  keys[i] = code;
}

struct BuildIn {
  const float* xyz;
  const float* scales;
  const float* rots;
  const float* opacity;
  const float* shs;
  const uint32_t* order;      // sorted position -> input row
  int32_t P, M;
};

struct BuildOut : HierRows {
  int2* range;                // [l, h) of the sorted leaves under each node
  double* mom;                // [N, kMomDoubles]
};

// numpy: bmin / bmax = x -+ 3 * max(s) in double, then rounded to float32; extent = max edge as a float32 subtraction
__device__ __forceinline__ void leaf_box(const float x[3], const float s[3], float* __restrict__ box) {
#pragma clang fp contract(off)
  const double ext = 3.0 * (double)fmaxf(fmaxf(s[0], s[1]), s[2]);
  float mn[3], mx[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    mn[a] = (float)((double)x[a] - ext);
    mx[a] = (float)((double)x[a] + ext);
  }
  const float e = fmaxf(fmaxf(mx[0] - mn[0], mx[1] - mn[1]), mx[2] - mn[2]);
  reinterpret_cast<float4*>(box)[0] = make_float4(mn[0], mn[1], mn[2], e);
  reinterpret_cast<float4*>(box)[1] = make_float4(mx[0], mx[1], mx[2], 0.0f);
}

// A leaf: the input row at sorted position l, in its input parametrisation; moments for the merge above it.
__device__ void init_leaf(const BuildIn& in, const BuildOut& out, int64_t id, int32_t l) {
  const int64_t src = in.order[l];
  const float x[3] = {in.xyz[src * 3 + 0], in.xyz[src * 3 + 1], in.xyz[src * 3 + 2]};
  const float s[3] = {in.scales[src * 3 + 0], in.scales[src * 3 + 1], in.scales[src * 3 + 2]};
  const float4 q = make_float4(in.rots[src * 4 + 0], in.rots[src * 4 + 1], in.rots[src * 4 + 2], in.rots[src * 4 + 3]);
  const float op = in.opacity[src];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    out.xyz[id * 3 + a] = x[a];
    out.log_scales[id * 3 + a] = (float)log((double)s[a]);
  }
  reinterpret_cast<float4*>(out.rots)[id] = q;
  out.alpha[id] = op;
  const float* sh_in = in.shs + src * in.M * 3;
  float4* sh_out = reinterpret_cast<float4*>(out.shs + id * kShFloats);
  const int n_in = in.M * 3;
#pragma unroll
  for (int j = 0; j < kShFloats / 4; ++j) {
    float v[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = (4 * j + k < n_in) ? sh_in[4 * j + k] : 0.0f;
    sh_out[j] = make_float4(v[0], v[1], v[2], v[3]);
  }
  leaf_box(x, s, out.boxes + id * 8);
  // covariance R diag(s^2) R^T of the (unnormalised, as the spec) quaternion, in double
  const double r = q.x, qx = q.y, qy = q.z, qz = q.w;
  const double R[3][3] = {{1 - 2 * (qy * qy + qz * qz), 2 * (qx * qy - r * qz), 2 * (qx * qz + r * qy)},
                          {2 * (qx * qy + r * qz), 1 - 2 * (qx * qx + qz * qz), 2 * (qy * qz - r * qx)},
                          {2 * (qx * qz - r * qy), 2 * (qy * qz + r * qx), 1 - 2 * (qx * qx + qy * qy)}};
  const double ds[3] = {s[0], s[1], s[2]};
  double L[3][3];
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int b = 0; b < 3; ++b) L[a][b] = R[a][b] * ds[b];
  auto cov = [&](int a, int b) { return L[a][0] * L[b][0] + L[a][1] * L[b][1] + L[a][2] * L[b][2]; };
  double* m = out.mom + id * kMomDoubles;
  m[0] = x[0]; m[1] = x[1]; m[2] = x[2];
  m[3] = cov(0, 0); m[4] = cov(0, 1); m[5] = cov(0, 2); m[6] = cov(1, 1); m[7] = cov(1, 2); m[8] = cov(2, 2);
  m[9] = (double)op * ((ds[0] * ds[1]) * ds[2]);
}

// Row of node `id` (index `idx` in its level) over the sorted leaves [l, h).  Interior: its children are the k-th pair
// of the next level (first id `next_first`), k = idx on a level without leaves, l - idx on the mixed level.
__device__ void write_node(const BuildIn& in, const BuildOut& out, int64_t id, int32_t depth, int32_t parent, int32_t l,
                           int32_t h, int64_t idx, bool mixed, int64_t next_first) {
  int32_t* nd = out.nodes + id * kNodeInts;
  nd[0] = depth;
  nd[1] = parent;
  nd[2] = (int32_t)id;
  out.range[id] = make_int2(l, h);
  if (h - l == 1) {
    nd[3] = 1; nd[4] = 0; nd[5] = 0; nd[6] = 0;
    init_leaf(in, out, id, l);
  } else {
    const int64_t k = mixed ? (int64_t)l - idx : idx;
    nd[3] = 0; nd[4] = 1; nd[5] = (int32_t)(next_first + 2 * k); nd[6] = 2;
  }
}

__global__ void hb_root_kernel(BuildIn in, BuildOut out, bool mixed) {
  if (threadIdx.x == 0) write_node(in, out, 0, 0, -1, 0, in.P, 0, mixed, 1);
}

// One thread per node of level d - 1 (first id parent_first): an interior node writes the rows of its two children.
__global__ __launch_bounds__(kHbThreads) void hb_level_kernel(BuildIn in, BuildOut out, int64_t parent_first,
                                                              int64_t n_parents, int32_t depth, int64_t child_first,
                                                              bool mixed, int64_t next_first) {
  const int64_t i = (int64_t)blockIdx.x * kHbThreads + threadIdx.x;
  if (i >= n_parents) return;
  const int64_t pid = parent_first + i;
  const int2 r = out.range[pid];
  if (r.y - r.x < 2) return;
  const int64_t c0 = out.nodes[pid * kNodeInts + 5];
  const int32_t mid = (int32_t)(((int64_t)r.x + r.y) / 2);
  write_node(in, out, c0, depth, (int32_t)pid, r.x, mid, c0 - child_first, mixed, next_first);
  write_node(in, out, c0 + 1, depth, (int32_t)pid, mid, r.y, c0 + 1 - child_first, mixed, next_first);
}

// One thread per node of level d: an interior node merges its two children (already final).
__global__ __launch_bounds__(kHbThreads) void hb_merge_kernel(BuildOut out, int64_t first, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * kHbThreads + threadIdx.x;
  if (i >= n) return;
  const int64_t id = first + i;
  const int32_t* nd = out.nodes + id * kNodeInts;
  if (nd[6] == 0) return;
  const int64_t c0 = nd[5], c1 = c0 + 1;
  const double* m0 = out.mom + c0 * kMomDoubles;
  const double* m1 = m0 + kMomDoubles;
  const double w0 = m0[9], w1 = m1[9];
  const double ws = fmax(w0 + w1, 1e-30);
  const double f0 = w0 / ws, f1 = w1 / ws;
  double mu[3], d0[3], d1[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    mu[a] = f0 * m0[a] + f1 * m1[a];
    d0[a] = m0[a] - mu[a];
    d1[a] = m1[a] - mu[a];
  }
  constexpr int kRow[6] = {0, 0, 0, 1, 1, 2}, kCol[6] = {0, 1, 2, 1, 2, 2};
  double cv[6];
#pragma unroll
  for (int k = 0; k < 6; ++k)
    cv[k] = f0 * (m0[3 + k] + d0[kRow[k]] * d0[kCol[k]]) + f1 * (m1[3 + k] + d1[kRow[k]] * d1[kCol[k]]);
  double* m = out.mom + id * kMomDoubles;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    m[a] = mu[a];
    out.xyz[id * 3 + a] = (float)mu[a];
  }
#pragma unroll
  for (int k = 0; k < 6; ++k) m[3 + k] = cv[k];
  m[9] = ws;
  // SH and opacity: weighted averages of the children's rows
  const float4* s0 = reinterpret_cast<const float4*>(out.shs + c0 * kShFloats);
  const float4* s1 = s0 + kShFloats / 4;
  float4* so = reinterpret_cast<float4*>(out.shs + id * kShFloats);
#pragma unroll 4
  for (int j = 0; j < kShFloats / 4; ++j) {
    const float4 a = s0[j], b = s1[j];
    so[j] = make_float4((float)(f0 * a.x + f1 * b.x), (float)(f0 * a.y + f1 * b.y), (float)(f0 * a.z + f1 * b.z),
                        (float)(f0 * a.w + f1 * b.w));
  }
  out.alpha[id] = (float)fmin(fmax(f0 * out.alpha[c0] + f1 * out.alpha[c1], 0.0), 1.0);
  // box: union of the children's (monotone rounding: the float union is the rounded double union)
  {
    const float4* b0 = reinterpret_cast<const float4*>(out.boxes + c0 * 8);
    const float4* b1 = b0 + 2;
    const float4 mn0 = b0[0], mx0 = b0[1], mn1 = b1[0], mx1 = b1[1];
    const float mn[3] = {fminf(mn0.x, mn1.x), fminf(mn0.y, mn1.y), fminf(mn0.z, mn1.z)};
    const float mx[3] = {fmaxf(mx0.x, mx1.x), fmaxf(mx0.y, mx1.y), fmaxf(mx0.z, mx1.z)};
    const float e = fmaxf(fmaxf(mx[0] - mn[0], mx[1] - mn[1]), mx[2] - mn[2]);
    float4* bo = reinterpret_cast<float4*>(out.boxes + id * 8);
    bo[0] = make_float4(mn[0], mn[1], mn[2], e);
    bo[1] = make_float4(mx[0], mx[1], mx[2], 0.0f);
  }
  // rotation and scales: the eigen tail of hier_merge_rule.h (cyclic Jacobi, one parametrisation of the decomposition)
  float ls[3], q[4];
  merge_cov_to_row(cv, ls, q);
#pragma unroll
  for (int a = 0; a < 3; ++a) out.log_scales[id * 3 + a] = ls[a];
  reinterpret_cast<float4*>(out.rots)[id] = make_float4(q[0], q[1], q[2], q[3]);
}

inline unsigned blocks_for(int64_t n) { return (unsigned)((n + kHbThreads - 1) / kHbThreads); }

struct HbTmp {
  uint32_t* words;
  uint32_t* keys;
  uint32_t* keys_sorted;
  uint32_t* order;
  int2* range;
  double* mom;
  void* sort_tmp;
};

HbTmp carve_hb_tmp(Carver& c, int32_t P) {
  const size_t N = 2 * (size_t)P - 1;
  HbTmp t;
  t.words = c.take<uint32_t>(8);
  t.keys = c.take<uint32_t>(P);
  t.keys_sorted = c.take<uint32_t>(P);
  t.order = c.take<uint32_t>(P);
  t.range = c.take<int2>(N);
  t.mom = c.take<double>(N * kMomDoubles);
  t.sort_tmp = c.take<char>(sort_tmp_bytes((uint32_t)P));   // nested: the sort's own slack included
  return t;
}

}  // namespace

size_t hier_build_tmp_bytes(int32_t P) {
  Carver c(nullptr);
  carve_hb_tmp(c, P);
  return c.bytes(kAlign);
}

int launch_hier_build(const float* xyz, const float* scales, const float* rots, const float* opacity, const float* shs,
                      int32_t P, int32_t M, float* out_xyz, float* out_shs, float* out_alpha, float* out_log_scales,
                      float* out_rots, int32_t* out_nodes, float* out_boxes, void* tmp, hipStream_t s) {
  Carver ws(tmp);
  const HbTmp t = carve_hb_tmp(ws, P);
  // ---- Morton order of the leaves
  HGS_HIP(hipMemsetAsync(t.words, 0xff, 8 * 4, s));
  hipLaunchKernelGGL(hb_bounds_kernel, dim3(min(blocks_for(P), 2048u)), dim3(kHbThreads), 0, s, xyz, P, t.words);
  HGS_LAUNCH_CHECK("hb_bounds", s, false);
  hipLaunchKernelGGL(hb_morton_kernel, dim3(blocks_for(P)), dim3(kHbThreads), 0, s, xyz, P, t.words, t.keys);
  HGS_LAUNCH_CHECK("hb_morton", s, false);
  int rc = sort_pairs32(t.keys, nullptr, t.keys_sorted, t.order, t.sort_tmp, (uint32_t)P, nullptr, 30, s, false);
  if (rc) return rc;
  // ---- level sizes (host arithmetic)
  int D = 0;
  while (((int64_t)2 << D) <= P) ++D;                  // D = floor(log2 P)
  const int64_t c = (int64_t)P - ((int64_t)1 << D);     // length-2 nodes of level D
  int64_t first[33], count[33];
  int levels = 0;
  for (int d = 0; d <= D; ++d, ++levels) {
    first[d] = ((int64_t)1 << d) - 1;
    count[d] = (int64_t)1 << d;
  }
  if (c > 0) {
    first[levels] = ((int64_t)2 << D) - 1;
    count[levels] = 2 * c;
    ++levels;
  }
  const BuildIn in{xyz, scales, rots, opacity, shs, t.order, P, M};
  const BuildOut out{{out_xyz, out_shs, out_alpha, out_log_scales, out_rots, out_nodes, out_boxes}, t.range, t.mom};
  // ---- topology and leaves, top-down
  hipLaunchKernelGGL(hb_root_kernel, dim3(1), dim3(64), 0, s, in, out, D == 0);
  HGS_LAUNCH_CHECK("hb_root", s, false);
  for (int d = 1; d < levels; ++d) {
    const int64_t next_first = d + 1 < levels ? first[d + 1] : 0;
    hipLaunchKernelGGL(hb_level_kernel, dim3(blocks_for(count[d - 1])), dim3(kHbThreads), 0, s, in, out, first[d - 1],
                       count[d - 1], (int32_t)d, first[d], d == D, next_first);
    HGS_LAUNCH_CHECK("hb_level", s, false);
  }
  // ---- merge, bottom-up (the last level holds leaves only)
  for (int d = levels - 2; d >= 0; --d) {
    hipLaunchKernelGGL(hb_merge_kernel, dim3(blocks_for(count[d])), dim3(kHbThreads), 0, s, out, first[d], count[d]);
    HGS_LAUNCH_CHECK("hb_merge", s, false);
  }
  return HGS_OK;
}

}  // namespace hgs
