// A surface from depth maps: TSDF fusion over views and a surface-net extraction, the rules of tsdf_rule.h
// (tests/tsdf_spec.py, the spec) on the device; hgs/meshing.py is the Python side.
//
//   integrate  tsdf_integrate_kernel: ONE pass over the volume for up to kTsdfMaxViews views.  A thread owns 4
//              consecutive x samples of a row.  The per-view parameters (12 matrix words, two tangents, W, H, z_min,
//              three plane pointers: 96 bytes) are kernel arguments read at wave-uniform addresses, so they sit in
//              scalar registers.  First every view projects the thread's samples (steps 1 and 2 of the rule) into a
//              32-bit mask, bit 4 v + s = view v sees sample s; a thread whose mask is empty returns before any volume
//              access, so the part of a volume that lies outside every frustum costs no traffic.  Then the 4 samples
//              are loaded once -- 16-byte loads where the group is whole and its address is 16-byte aligned in every
//              array, scalar loads for ragged rows and tails --, the views are applied in array order on registers,
//              and the samples are stored once, only if some view changed one.  The projection is recomputed for
//              the set bits: keeping the pixel and the depth of all 32 (view, sample) pairs instead (64 registers, the
//              view loop unrolled) was measured and is no faster -- 3.38 against 3.66 ms for 8 views at 512^3, but
//              0.75 against 0.61 ms for one view and 3.96 against 2.86 ms with colour on a half-seen volume, at 3-4
//              waves per SIMD instead of 8 (profiles/f27_tsdf_kernels.md).  No atomics, no LDS, no scratch.
//   plan       tsdf_mark_kernel: one thread per sample writes the sample's class byte (cell active, observed, inside),
//              the rank of its cell among the active cells of its workgroup (a byte: 256 threads) and the workgroup's
//              count; tsdf_count_kernel: per sample the quads of its three edges (three bits) from the class bytes of
//              its neighbours, and the workgroup's count; tsdf_scan_kernel: common.h's chained scan over both sums;
//              ONE host wait reads the two totals.
//   apply      asynchronous.  tsdf_emit_kernel: an active cell writes its vertex, normal and colour at
//              sums[workgroup] + rank -- ascending linear cell index --, a sample writes the two triangles of each of
//              its quads at the scanned quad offset, the vertex indices from the same sums and ranks.  Every index it
//              writes at comes from the workspace, which a plan on the same (device, tmp, dimensions) has filled whole.
#include "lod_cut.h"    // the workgroup offsets and the launcher of the chained scan (the cut rules in it are not used)
#include "tsdf_rule.h"

#include <mutex>
#include <vector>

#pragma clang fp contract(off)

namespace hgs {
namespace {

constexpr int kTsdfThreads = 256;
constexpr int kTsdfMaxViews = 8;
constexpr int64_t kTsdfMaxSamples = 0x7fffffff;
// the quad offsets are 32-bit and a sample has at most three quads
constexpr int64_t kTsdfMaxExtractSamples = 0xffffffffll / 3;
constexpr uint32_t kCellActive = 1u, kObserved = 2u, kInside = 4u;

struct TsdfViews { hgs_tsdf_view v[kTsdfMaxViews]; };
static_assert(sizeof(hgs_tsdf_view) == 96, "96 bytes per view");

template <bool kColour>
__global__ __launch_bounds__(kTsdfThreads) void tsdf_integrate_kernel(hgs_tsdf_volume vol, TsdfViews views, int n_views,
                                                                      int32_t groups_x, int64_t n_threads) {
  const int64_t tid = (int64_t)blockIdx.x * kTsdfThreads + threadIdx.x;
  if (tid >= n_threads) return;
  const int64_t row = tid / groups_x;
  const int32_t i0 = (int32_t)(tid - row * groups_x) * 4;
  const int32_t k = (int32_t)(row / vol.ny), j = (int32_t)(row - (int64_t)k * vol.ny);
  const int count = min(4, vol.nx - i0);
  const float x1 = tsdf_lattice(vol.lo[1], vol.voxel, j), x2 = tsdf_lattice(vol.lo[2], vol.voxel, k);
  float x0[4];
#pragma unroll
  for (int s = 0; s < 4; ++s) x0[s] = tsdf_lattice(vol.lo[0], vol.voxel, i0 + s);
  // ---- which view sees which sample: before any volume access
  uint32_t mask = 0;
  for (int v = 0; v < n_views; ++v) {
    const hgs_tsdf_view& a = views.v[v];
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      float z;
      int32_t px, py;
      if (s < count && tsdf_project(x0[s], x1, x2, a.view, a.tanfovx, a.tanfovy, a.W, a.H, a.z_min, &z, &px, &py))
        mask |= 1u << (4 * v + s);
    }
  }
  if (mask == 0u) return;
  // ---- the samples, once
  const int64_t base = row * vol.nx + i0;
  float* const tp = vol.tsdf + base;
  float* const wp = vol.weight + base;
  float* const cp = kColour ? vol.colour + base * 3 : nullptr;
  const bool vec = count == 4 && (((uintptr_t)tp | (uintptr_t)wp | (uintptr_t)cp) & 15u) == 0u;
  float T[4], Wt[4], Cl[4][3];
  if (vec) {
    const float4 t4 = *reinterpret_cast<const float4*>(tp), w4 = *reinterpret_cast<const float4*>(wp);
    T[0] = t4.x; T[1] = t4.y; T[2] = t4.z; T[3] = t4.w;
    Wt[0] = w4.x; Wt[1] = w4.y; Wt[2] = w4.z; Wt[3] = w4.w;
    if constexpr (kColour) {
      const float4 c0 = reinterpret_cast<const float4*>(cp)[0], c1 = reinterpret_cast<const float4*>(cp)[1],
                   c2 = reinterpret_cast<const float4*>(cp)[2];
      Cl[0][0] = c0.x; Cl[0][1] = c0.y; Cl[0][2] = c0.z; Cl[1][0] = c0.w;
      Cl[1][1] = c1.x; Cl[1][2] = c1.y; Cl[2][0] = c1.z; Cl[2][1] = c1.w;
      Cl[2][2] = c2.x; Cl[3][0] = c2.y; Cl[3][1] = c2.z; Cl[3][2] = c2.w;
    }
  } else {
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      T[s] = s < count ? tp[s] : 0.0f;
      Wt[s] = s < count ? wp[s] : 0.0f;
      if constexpr (kColour) {
#pragma unroll
        for (int c = 0; c < 3; ++c) Cl[s][c] = s < count ? cp[s * 3 + c] : 0.0f;
      }
    }
  }
  // ---- the views in array order, on registers
  bool changed = false;
  for (int v = 0; v < n_views; ++v) {
    const hgs_tsdf_view& a = views.v[v];
    const size_t plane = (size_t)a.W * (size_t)a.H;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      if (!((mask >> (4 * v + s)) & 1u)) continue;
      float z;
      int32_t px, py;
      if (!tsdf_project(x0[s], x1, x2, a.view, a.tanfovx, a.tanfovy, a.W, a.H, a.z_min, &z, &px, &py)) continue;
      const size_t pix = (size_t)py * (size_t)a.W + (size_t)px;
      const float d = a.depth[pix];
      const float w = a.weight ? a.weight[pix] : 1.0f;
      if constexpr (kColour) {
        float rgb[3] = {0.0f, 0.0f, 0.0f};
        if (a.rgb) {
#pragma unroll
          for (int c = 0; c < 3; ++c) rgb[c] = a.rgb[(size_t)c * plane + pix];
        }
        changed |= tsdf_update(d, w, rgb, a.rgb != nullptr, z, vol.trunc, vol.max_weight, &T[s], &Wt[s], Cl[s]);
      } else {
        changed |= tsdf_update(d, w, nullptr, false, z, vol.trunc, vol.max_weight, &T[s], &Wt[s], nullptr);
      }
    }
  }
  if (!changed) return;
  if (vec) {
    *reinterpret_cast<float4*>(tp) = make_float4(T[0], T[1], T[2], T[3]);
    *reinterpret_cast<float4*>(wp) = make_float4(Wt[0], Wt[1], Wt[2], Wt[3]);
    if constexpr (kColour) {
      reinterpret_cast<float4*>(cp)[0] = make_float4(Cl[0][0], Cl[0][1], Cl[0][2], Cl[1][0]);
      reinterpret_cast<float4*>(cp)[1] = make_float4(Cl[1][1], Cl[1][2], Cl[2][0], Cl[2][1]);
      reinterpret_cast<float4*>(cp)[2] = make_float4(Cl[2][2], Cl[3][0], Cl[3][1], Cl[3][2]);
    }
  } else {
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      if (s < count) {
        tp[s] = T[s];
        wp[s] = Wt[s];
        if constexpr (kColour) {
#pragma unroll
          for (int c = 0; c < 3; ++c) cp[s * 3 + c] = Cl[s][c];
        }
      }
    }
  }
}

// ---- extraction ------------------------------------------------------------------------------------------------------
struct Dims { int32_t nx, ny, nz; };
__device__ __forceinline__ void sample_of(int64_t n, Dims d, int32_t* i, int32_t* j, int32_t* k) {
  const int64_t row = n / d.nx;
  *i = (int32_t)(n - row * d.nx);
  *k = (int32_t)(row / d.ny);
  *j = (int32_t)(row - (int64_t)*k * d.ny);
}
// the linear offsets of a cell's 8 samples from its lower corner, in sample order
__device__ __forceinline__ int64_t corner_offset(int s, Dims d) {
  return (int64_t)(s & 1) + (int64_t)((s >> 1) & 1) * d.nx + (int64_t)(s >> 2) * d.nx * d.ny;
}

// One thread per sample: its class byte, the rank of its cell among the workgroup's active cells, the workgroup's count.
__global__ __launch_bounds__(kTsdfThreads) void tsdf_mark_kernel(const float* __restrict__ tsdf,
                                                                 const float* __restrict__ weight, Dims d, int64_t N,
                                                                 float min_weight, uint8_t* __restrict__ cls,
                                                                 uint8_t* __restrict__ rank, uint32_t* __restrict__ vsum,
                                                                 unsigned long long* __restrict__ vchain,
                                                                 unsigned long long* __restrict__ qchain) {
  clear_scan_chain(vchain);
  clear_scan_chain(qchain);
  const int64_t n = (int64_t)blockIdx.x * kTsdfThreads + threadIdx.x;
  uint32_t c = 0;
  if (n < N) {
    int32_t i, j, k;
    sample_of(n, d, &i, &j, &k);
    const float t0 = tsdf[n], w0 = weight[n];
    c = (tsdf_observed(w0, min_weight) ? kObserved : 0u) | (tsdf_inside(t0) ? kInside : 0u);
    if ((c & kObserved) && i < d.nx - 1 && j < d.ny - 1 && k < d.nz - 1) {
      float t[8], w[8];
#pragma unroll
      for (int s = 0; s < 8; ++s) {
        t[s] = tsdf[n + corner_offset(s, d)];
        w[s] = weight[n + corner_offset(s, d)];
      }
      if (tsdf_cell_active(t, w, min_weight)) c |= kCellActive;
    }
  }
  const uint32_t active = c & kCellActive;
  const uint32_t off = block_exclusive_offset(active);
  if (n < N) {
    cls[n] = (uint8_t)c;
    rank[n] = (uint8_t)off;
  }
  if (threadIdx.x == kTsdfThreads - 1) vsum[blockIdx.x] = off + active;
}

// Is the cell at sample (i, j, k) + o in range and active?
__device__ __forceinline__ bool cell_active_at(const uint8_t* __restrict__ cls, int64_t n, Dims d, int32_t i, int32_t j,
                                               int32_t k, const int32_t o[3]) {
  const int32_t ci = i + o[0], cj = j + o[1], ck = k + o[2];
  if (ci < 0 || cj < 0 || ck < 0 || ci > d.nx - 2 || cj > d.ny - 2 || ck > d.nz - 2) return false;
  const int64_t m = n + o[0] + (int64_t)o[1] * d.nx + (int64_t)o[2] * d.nx * d.ny;
  return (cls[m] & kCellActive) != 0u;
}

// One thread per sample: bit a of its quad byte = the edge from the sample along axis a emits a quad.
__global__ __launch_bounds__(kTsdfThreads) void tsdf_count_kernel(const uint8_t* __restrict__ cls, Dims d, int64_t N,
                                                                  uint8_t* __restrict__ quads,
                                                                  uint32_t* __restrict__ qsum) {
  const int64_t n = (int64_t)blockIdx.x * kTsdfThreads + threadIdx.x;
  uint32_t bits = 0;
  if (n < N) {
    int32_t i, j, k;
    sample_of(n, d, &i, &j, &k);
    const uint32_t c = cls[n];
    if (c & kObserved) {
      const int32_t at[3] = {i, j, k}, dim[3] = {d.nx, d.ny, d.nz};
      const int64_t step[3] = {1, d.nx, (int64_t)d.nx * d.ny};
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        if (at[a] + 1 >= dim[a]) continue;
        const uint32_t cu = cls[n + step[a]];
        if (!(cu & kObserved) || ((cu ^ c) & kInside) == 0u) continue;
        int32_t cells[4][3];
        tsdf_quad_cells(a, cells);
        bool all = true;
#pragma unroll
        for (int q = 0; q < 4; ++q) all = all && cell_active_at(cls, n, d, i, j, k, cells[q]);
        bits |= all ? (1u << a) : 0u;
      }
    }
    quads[n] = (uint8_t)bits;
  }
  const uint32_t cnt = (uint32_t)__popc(bits);
  const uint32_t off = block_exclusive_offset(cnt);
  if (threadIdx.x == kTsdfThreads - 1) qsum[blockIdx.x] = off + cnt;
}

// both sums scanned in place; sums[n] = the total
__global__ __launch_bounds__(1024) void tsdf_scan_kernel(uint32_t* __restrict__ vsum, uint32_t* __restrict__ qsum, int n,
                                                         unsigned long long* __restrict__ vchain,
                                                         unsigned long long* __restrict__ qchain, int c_off, int chunks) {
  (void)chained_scan_inplace(vsum, n, vchain, c_off, chunks);
  __syncthreads();      // the scan's shared words are written again
  (void)chained_scan_inplace(qsum, n, qchain, c_off, chunks);
}

__device__ __forceinline__ int32_t vertex_of_cell(int64_t m, const uint8_t* __restrict__ rank,
                                                  const uint32_t* __restrict__ vsum) {
  return (int32_t)(vsum[m / kTsdfThreads] + rank[m]);
}

// One thread per sample: the vertex of its cell, the triangles of its quads.
template <bool kColour>
__global__ __launch_bounds__(kTsdfThreads) void tsdf_emit_kernel(hgs_tsdf_volume vol, int64_t N,
                                                                 const uint8_t* __restrict__ cls,
                                                                 const uint8_t* __restrict__ rank,
                                                                 const uint8_t* __restrict__ quads,
                                                                 const uint32_t* __restrict__ vsum,
                                                                 const uint32_t* __restrict__ qsum,
                                                                 float* __restrict__ vertices, float* __restrict__ normals,
                                                                 float* __restrict__ colours, int32_t* __restrict__ faces) {
  const Dims d{vol.nx, vol.ny, vol.nz};
  const int64_t n = (int64_t)blockIdx.x * kTsdfThreads + threadIdx.x;
  uint32_t c = 0, bits = 0;
  int32_t i = 0, j = 0, k = 0;
  if (n < N) {
    c = cls[n];
    bits = quads[n];
    sample_of(n, d, &i, &j, &k);
  }
  if (c & kCellActive) {
    float t[8];
#pragma unroll
    for (int s = 0; s < 8; ++s) t[s] = vol.tsdf[n + corner_offset(s, d)];
    float local[3], normal[3];
    tsdf_cell_vertex(t, local, normal);
    const size_t vi = (size_t)vertex_of_cell(n, rank, vsum);
    const int32_t at[3] = {i, j, k};
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      vertices[vi * 3 + a] = tsdf_vertex_world(vol.lo[a], vol.voxel, at[a], local[a]);
      normals[vi * 3 + a] = normal[a];
    }
    if constexpr (kColour) {
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) {
        float v[8];
#pragma unroll
        for (int s = 0; s < 8; ++s) v[s] = vol.colour[(n + corner_offset(s, d)) * 3 + ch];
        colours[vi * 3 + ch] = tsdf_cell_colour(v);
      }
    }
  }
  const uint32_t cnt = (uint32_t)__popc(bits);
  size_t q = (size_t)qsum[blockIdx.x] + block_exclusive_offset(cnt);
  if (bits) {
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      if (!((bits >> a) & 1u)) continue;
      int32_t cells[4][3], v[4], f[6];
      tsdf_quad_cells(a, cells);
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int64_t m = n + cells[u][0] + (int64_t)cells[u][1] * d.nx + (int64_t)cells[u][2] * d.nx * d.ny;
        v[u] = vertex_of_cell(m, rank, vsum);
      }
      tsdf_quad_faces(v, (c & kInside) != 0u, f);
#pragma unroll
      for (int u = 0; u < 6; ++u) faces[q * 6 + u] = f[u];
      ++q;
    }
  }
}

struct TsdfTmp {
  uint8_t* cls;     // [N] class bytes
  uint8_t* rank;    // [N] rank of the sample's cell among its workgroup's active cells
  uint8_t* quads;   // [N] quad bits
  uint32_t* vsum;   // [nblk + 1] active cells per workgroup, scanned in place; [nblk] = the vertices
  uint32_t* qsum;   // [nblk + 1] quads per workgroup, likewise
  unsigned long long* vchain;   // [scan_chunks(nblk)] each
  unsigned long long* qchain;
};

TsdfTmp carve_tsdf_tmp(Carver& c, int64_t N) {
  const size_t nblk = (size_t)((N + kTsdfThreads - 1) / kTsdfThreads);
  TsdfTmp t;
  t.cls = c.take<uint8_t>((size_t)N);
  t.rank = c.take<uint8_t>((size_t)N);
  t.quads = c.take<uint8_t>((size_t)N);
  t.vsum = c.take<uint32_t>(nblk + 1);
  t.qsum = c.take<uint32_t>(nblk + 1);
  t.vchain = c.take<unsigned long long>((size_t)scan_chunks(nblk));
  t.qchain = c.take<unsigned long long>((size_t)scan_chunks(nblk));
  return t;
}

// The successful plans by (device, tmp): apply follows indices out of tmp, so it runs only behind a plan of its sizes.
struct TsdfPlan { int device; const void* tmp; int32_t nx, ny, nz; };
std::mutex g_plan_mutex;
std::vector<TsdfPlan> g_plans;

void forget_plan(int device, const void* tmp) {
  std::lock_guard<std::mutex> lock(g_plan_mutex);
  for (size_t k = 0; k < g_plans.size(); ++k)
    if (g_plans[k].device == device && g_plans[k].tmp == tmp) { g_plans.erase(g_plans.begin() + k); break; }
}
void add_plan(const TsdfPlan& p) {
  std::lock_guard<std::mutex> lock(g_plan_mutex);
  if (g_plans.size() >= 64) g_plans.erase(g_plans.begin());
  g_plans.push_back(p);
}
bool planned(int device, const void* tmp, const hgs_tsdf_volume* v) {
  std::lock_guard<std::mutex> lock(g_plan_mutex);
  for (const TsdfPlan& p : g_plans)
    if (p.device == device && p.tmp == tmp) return p.nx == v->nx && p.ny == v->ny && p.nz == v->nz;
  return false;
}

bool positive_finite(float x) { return x > 0.0f && x - x == 0.0f; }

int refuse(const char* why) {
  set_error("%s", why);
  return HGS_ERR_INVALID;
}

// what every call asks of the volume
int check_volume(const hgs_tsdf_volume* v) {
  if (!v) return refuse("null argument: the volume");
  if (v->nx < 1 || v->ny < 1 || v->nz < 1 || (int64_t)v->nx * v->ny > kTsdfMaxSamples ||
      (int64_t)v->nx * v->ny * v->nz > kTsdfMaxSamples) {
    set_error("bad sizes: a volume of %d x %d x %d samples; every dimension >= 1 and at most 2^31 - 1 samples expected",
              v->nx, v->ny, v->nz);
    return HGS_ERR_INVALID;
  }
  if (!positive_finite(v->voxel)) return refuse("voxel must be positive and finite");
  if (!positive_finite(v->trunc)) return refuse("trunc must be positive and finite");
  if (!(v->max_weight > 0.0f)) return refuse("max_weight must be positive");
  if (!v->tsdf || !v->weight) return refuse("null argument: tsdf / weight");
  if (((uintptr_t)v->tsdf | (uintptr_t)v->weight | (uintptr_t)v->colour) & 3u)
    return refuse("tsdf / weight / colour must be 4-byte aligned");
  return HGS_OK;
}

int check_extract(const hgs_tsdf_volume* v, const void* tmp) {
  if (int rc = check_volume(v)) return rc;
  if ((int64_t)v->nx * v->ny * v->nz > kTsdfMaxExtractSamples) {
    set_error("bad sizes: %lld samples; an extraction takes at most (2^32 - 1) / 3 (its quad offsets are 32-bit)",
              (long long)((int64_t)v->nx * v->ny * v->nz));
    return HGS_ERR_INVALID;
  }
  if (!tmp) return refuse("null argument: tmp");
  if ((uintptr_t)tmp & (kAlign - 1)) { set_error("tmp must be %d-byte aligned", (int)kAlign); return HGS_ERR_INVALID; }
  return HGS_OK;
}

}  // namespace
}  // namespace hgs

using namespace hgs;

extern "C" {

int hgs_tsdf_integrate(const hgs_tsdf_volume* volume, const hgs_tsdf_view* views, int32_t n_views, hgs_stream_t stream,
                       int device) {
  if (n_views < 1 || n_views > kTsdfMaxViews) {
    set_error("bad sizes: n_views=%d not in [1, %d]", n_views, kTsdfMaxViews);
    return HGS_ERR_INVALID;
  }
  if (int rc = check_volume(volume)) return rc;
  if (!views) return refuse("null argument: views");
  TsdfViews va;
  for (int v = 0; v < kTsdfMaxViews; ++v) va.v[v] = views[v < n_views ? v : 0];
  for (int v = 0; v < n_views; ++v) {
    const hgs_tsdf_view& a = views[v];
    if (a.W < 1 || a.H < 1 || (int64_t)a.W * a.H > 0x7fffffff) {
      set_error("bad sizes: view %d is %d x %d pixels; W, H >= 1 and at most 2^31 - 1 pixels expected", v, a.W, a.H);
      return HGS_ERR_INVALID;
    }
    if (!a.depth) { set_error("null argument: the depth of view %d", v); return HGS_ERR_INVALID; }
    if (a.rgb && !volume->colour) { set_error("view %d has rgb but the volume has no colour", v); return HGS_ERR_INVALID; }
    if (((uintptr_t)a.depth | (uintptr_t)a.weight | (uintptr_t)a.rgb) & 3u) {
      set_error("the planes of view %d must be 4-byte aligned", v);
      return HGS_ERR_INVALID;
    }
  }
  HGS_HIP(hipSetDevice(device));
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int32_t groups_x = (volume->nx + 3) / 4;
  const int64_t n_threads = (int64_t)groups_x * volume->ny * volume->nz;
  const dim3 grid((unsigned)((n_threads + kTsdfThreads - 1) / kTsdfThreads)), block(kTsdfThreads);
  if (volume->colour) {
    hipLaunchKernelGGL(tsdf_integrate_kernel<true>, grid, block, 0, s, *volume, va, (int)n_views, groups_x, n_threads);
  } else {
    hipLaunchKernelGGL(tsdf_integrate_kernel<false>, grid, block, 0, s, *volume, va, (int)n_views, groups_x, n_threads);
  }
  HGS_LAUNCH_CHECK("tsdf_integrate", s, false);
  return HGS_OK;
}

size_t hgs_tsdf_extract_tmp_bytes(int32_t nx, int32_t ny, int32_t nz) {
  if (nx < 1 || ny < 1 || nz < 1 || (int64_t)nx * ny > kTsdfMaxSamples ||
      (int64_t)nx * ny * nz > kTsdfMaxExtractSamples)
    return 0;
  Carver c(nullptr);
  carve_tsdf_tmp(c, (int64_t)nx * ny * nz);
  return c.bytes(0);   // tmp is required to be kAlign-aligned: no slack
}

int hgs_tsdf_extract_plan(const hgs_tsdf_volume* volume, float min_weight, void* tmp, int64_t totals_host[2],
                          hgs_stream_t stream, int device) {
  if (int rc = check_extract(volume, tmp)) return rc;
  if (!positive_finite(min_weight)) return refuse("min_weight must be positive and finite");
  if (!totals_host) return refuse("null argument: totals_host");
  forget_plan(device, tmp);
  HGS_HIP(hipSetDevice(device));
  hipStream_t s = static_cast<hipStream_t>(stream);
  const Dims d{volume->nx, volume->ny, volume->nz};
  const int64_t N = (int64_t)d.nx * d.ny * d.nz;
  Carver c(tmp);
  const TsdfTmp t = carve_tsdf_tmp(c, N);
  const int nblk = (int)((N + kTsdfThreads - 1) / kTsdfThreads);
  const dim3 grid((unsigned)nblk), block(kTsdfThreads);
  hipLaunchKernelGGL(tsdf_mark_kernel, grid, block, 0, s, volume->tsdf, volume->weight, d, N, min_weight, t.cls, t.rank,
                     t.vsum, t.vchain, t.qchain);
  HGS_LAUNCH_CHECK("tsdf_mark", s, false);
  hipLaunchKernelGGL(tsdf_count_kernel, grid, block, 0, s, t.cls, d, N, t.quads, t.qsum);
  HGS_LAUNCH_CHECK("tsdf_count", s, false);
  if (int rc = launch_scan_chunks(tsdf_scan_kernel, "tsdf_scan", nblk, s, t.vsum, t.qsum, nblk, t.vchain, t.qchain))
    return rc;
  // ---- the one host wait
  uint32_t totals[2];
  HGS_HIP(hipMemcpyAsync(&totals[0], t.vsum + nblk, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
  HGS_HIP(hipMemcpyAsync(&totals[1], t.qsum + nblk, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
  HGS_HIP(wait_stream(s));
  totals_host[0] = (int64_t)totals[0];
  totals_host[1] = (int64_t)totals[1];
  add_plan(TsdfPlan{device, tmp, d.nx, d.ny, d.nz});
  return HGS_OK;
}

int hgs_tsdf_extract_apply(const hgs_tsdf_volume* volume, const void* tmp, float* vertices, float* normals,
                           float* colours, int32_t* faces, hgs_stream_t stream, int device) {
  if (int rc = check_extract(volume, tmp)) return rc;
  if (colours && !volume->colour) return refuse("colours asked of a volume that has no colour");
  if (!vertices || !normals || !faces) return refuse("null argument: vertices / normals / faces");
  if (((uintptr_t)vertices | (uintptr_t)normals | (uintptr_t)colours | (uintptr_t)faces) & 3u)
    return refuse("vertices / normals / colours / faces must be 4-byte aligned");
  if (!planned(device, tmp, volume))
    return refuse("no successful hgs_tsdf_extract_plan of these dimensions on this (device, tmp)");
  HGS_HIP(hipSetDevice(device));
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int64_t N = (int64_t)volume->nx * volume->ny * volume->nz;
  Carver c(const_cast<void*>(tmp));
  const TsdfTmp t = carve_tsdf_tmp(c, N);
  const dim3 grid((unsigned)((N + kTsdfThreads - 1) / kTsdfThreads)), block(kTsdfThreads);
  if (colours) {
    hipLaunchKernelGGL(tsdf_emit_kernel<true>, grid, block, 0, s, *volume, N, t.cls, t.rank, t.quads, t.vsum, t.qsum,
                       vertices, normals, colours, faces);
  } else {
    hipLaunchKernelGGL(tsdf_emit_kernel<false>, grid, block, 0, s, *volume, N, t.cls, t.rank, t.quads, t.vsum, t.qsum,
                       vertices, normals, colours, faces);
  }
  HGS_LAUNCH_CHECK("tsdf_emit", s, false);
  return HGS_OK;
}

}  // extern "C"
