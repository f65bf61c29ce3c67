// K11: simple_knn._C.distCUDA2 replacement (scene/gaussian_model.py:190): for every point,
// the mean of the squared distances to its 3 nearest neighbours.  Exact:
//   1. bounding box, 30-bit Morton codes, radix sort (reuses the rasterizer's sort),
//   2. AABB of every run of 256 Morton-consecutive points,
//   3. per point: seed the best-3 list from its Morton neighbours, then visit only the
//      runs whose AABB is closer than the current 3rd-best distance.
// One-off initialisation work, not part of the per-frame path.
#include "common.h"

namespace hgs {
namespace {

constexpr int kRun = 256;

__device__ __forceinline__ uint32_t f2ord(float f) {
  const uint32_t u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float ord2f(uint32_t u) {
  return __uint_as_float((u & 0x80000000u) ? (u & 0x7fffffffu) : ~u);
}

__global__ void knn_init_kernel(uint32_t* mm) {
  if (threadIdx.x < 3) mm[threadIdx.x] = 0xffffffffu;        // min
  else if (threadIdx.x < 6) mm[threadIdx.x] = 0u;            // max
}

__global__ __launch_bounds__(256) void knn_bbox_kernel(const float* __restrict__ xyz, int P, uint32_t* mm) {
  float mn[3] = {3.0e38f, 3.0e38f, 3.0e38f}, mx[3] = {-3.0e38f, -3.0e38f, -3.0e38f};
  for (int i = blockIdx.x * 256 + threadIdx.x; i < P; i += gridDim.x * 256) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const float v = xyz[(size_t)i * 3 + k];
      mn[k] = fminf(mn[k], v);
      mx[k] = fmaxf(mx[k], v);
    }
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      mn[k] = fminf(mn[k], __shfl_xor(mn[k], off, 64));
      mx[k] = fmaxf(mx[k], __shfl_xor(mx[k], off, 64));
    }
  }
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      atomicMin(&mm[k], f2ord(mn[k]));
      atomicMax(&mm[3 + k], f2ord(mx[k]));
    }
  }
}

__device__ __forceinline__ uint32_t spread10(uint32_t x) {
  x &= 0x3ffu;
  x = (x | (x << 16)) & 0x030000ffu;
  x = (x | (x << 8)) & 0x0300f00fu;
  x = (x | (x << 4)) & 0x030c30c3u;
  x = (x | (x << 2)) & 0x09249249u;
  return x;
}

__global__ __launch_bounds__(256) void knn_morton_kernel(const float* __restrict__ xyz, int P,
                                                         const uint32_t* __restrict__ mm,
                                                         uint64_t* __restrict__ keys, uint32_t* __restrict__ vals) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= P) return;
  uint32_t code = 0;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const float lo = ord2f(mm[k]), hi = ord2f(mm[3 + k]);
    const float ext = fmaxf(hi - lo, 1e-30f);
    float t = (xyz[(size_t)i * 3 + k] - lo) / ext;
    t = fminf(fmaxf(t, 0.0f), 1.0f);
    const uint32_t q = (uint32_t)(t * 1023.0f);
    code |= spread10(q) << k;
  }
  keys[i] = (uint64_t)code;
  vals[i] = (uint32_t)i;
}

__global__ __launch_bounds__(kRun) void knn_gather_boxes_kernel(const float* __restrict__ xyz, int P,
                                                                const uint32_t* __restrict__ order,
                                                                float4* __restrict__ sorted,
                                                                float* __restrict__ boxes) {
  __shared__ float red[6][kRun / 64];
  const int i = blockIdx.x * kRun + threadIdx.x;
  float p[3] = {0.f, 0.f, 0.f};
  const bool ok = i < P;
  if (ok) {
    const uint32_t src = order[i];
    p[0] = xyz[(size_t)src * 3 + 0];
    p[1] = xyz[(size_t)src * 3 + 1];
    p[2] = xyz[(size_t)src * 3 + 2];
    sorted[i] = make_float4(p[0], p[1], p[2], __uint_as_float(src));
  }
  float mn[3], mx[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    mn[k] = ok ? p[k] : 3.0e38f;
    mx[k] = ok ? p[k] : -3.0e38f;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      mn[k] = fminf(mn[k], __shfl_xor(mn[k], off, 64));
      mx[k] = fmaxf(mx[k], __shfl_xor(mx[k], off, 64));
    }
    if ((threadIdx.x & 63) == 0) {
      red[k][threadIdx.x >> 6] = mn[k];
      red[3 + k][threadIdx.x >> 6] = mx[k];
    }
  }
  __syncthreads();
  if (threadIdx.x < 6) {
    float v = red[threadIdx.x][0];
    for (int w = 1; w < kRun / 64; ++w)
      v = threadIdx.x < 3 ? fminf(v, red[threadIdx.x][w]) : fmaxf(v, red[threadIdx.x][w]);
    boxes[(size_t)blockIdx.x * 6 + threadIdx.x] = v;
  }
}

__device__ __forceinline__ void push3(float d, float best[3]) {
  if (d < best[2]) {
    if (d < best[1]) {
      best[2] = best[1];
      if (d < best[0]) { best[1] = best[0]; best[0] = d; } else { best[1] = d; }
    } else {
      best[2] = d;
    }
  }
}

__global__ __launch_bounds__(256) void knn_search_kernel(const float4* __restrict__ sorted, int P,
                                                         const float* __restrict__ boxes, int nbox,
                                                         float* __restrict__ out) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= P) return;
  const float4 me = sorted[i];
  float best[3] = {3.0e38f, 3.0e38f, 3.0e38f};
  for (int j = max(0, i - 3); j <= min(P - 1, i + 3); ++j) {
    if (j == i) continue;
    const float4 q = sorted[j];
    const float dx = q.x - me.x, dy = q.y - me.y, dz = q.z - me.z;
    push3(dx * dx + dy * dy + dz * dz, best);
  }
  for (int b = 0; b < nbox; ++b) {
    const float* bx = boxes + (size_t)b * 6;
    const float dx = fmaxf(fmaxf(bx[0] - me.x, me.x - bx[3]), 0.f);
    const float dy = fmaxf(fmaxf(bx[1] - me.y, me.y - bx[4]), 0.f);
    const float dz = fmaxf(fmaxf(bx[2] - me.z, me.z - bx[5]), 0.f);
    if (dx * dx + dy * dy + dz * dz >= best[2]) continue;
    const int j0 = b * kRun, j1 = min(P, j0 + kRun);
    for (int j = j0; j < j1; ++j) {
      if (j == i || (j >= i - 3 && j <= i + 3)) continue;
      const float4 q = sorted[j];
      const float ex = q.x - me.x, ey = q.y - me.y, ez = q.z - me.z;
      push3(ex * ex + ey * ey + ez * ez, best);
    }
  }
  float sum = 0.f;
  int cnt = 0;
#pragma unroll
  for (int k = 0; k < 3; ++k)
    if (best[k] < 3.0e38f) { sum += best[k]; ++cnt; }
  // same convention as the 3-neighbour mean: divide by 3 (fewer than 4 points -> partial sum / 3)
  (void)cnt;
  out[__float_as_uint(me.w)] = sum / 3.0f;
}

struct KnnTmp {
  uint32_t* mm;
  uint64_t* keys_in;
  uint32_t* vals_in;
  uint64_t* keys_out;
  uint32_t* vals_out;
  float4* sorted;
  float* boxes;
  void* sort_tmp;
};

inline KnnTmp carve_knn(Carver& c, int32_t P) {
  const size_t p = (size_t)(P > 0 ? P : 1);
  KnnTmp t;
  t.mm = c.take<uint32_t>(8);
  t.keys_in = c.take<uint64_t>(p);
  t.vals_in = c.take<uint32_t>(p);
  t.keys_out = c.take<uint64_t>(p);
  t.vals_out = c.take<uint32_t>(p);
  t.sorted = c.take<float4>(p);
  t.boxes = c.take<float>(((p + kRun - 1) / kRun) * 6);
  t.sort_tmp = c.take<char>(sort_tmp_bytes((uint32_t)p));   // nested: the sort's own slack included
  return t;
}

}  // namespace
}  // namespace hgs

using namespace hgs;

extern "C" {

size_t hgs_knn_tmp_bytes(int32_t P) {
  Carver c(nullptr);
  carve_knn(c, P);
  return c.bytes(kAlign);
}

int hgs_dist2_knn3(const float* xyz, int32_t P, float* out_mean_d2, void* tmp, hgs_stream_t stream, int device) {
  if (P <= 0) return HGS_OK;
  if (!xyz || !out_mean_d2 || !tmp) { set_error("null argument"); return HGS_ERR_INVALID; }
  HGS_HIP(hipSetDevice(device));
  hipStream_t s = static_cast<hipStream_t>(stream);
  Carver c(tmp);
  const KnnTmp t = carve_knn(c, P);
  const int nblk = (P + 255) / 256;
  hipLaunchKernelGGL(knn_init_kernel, dim3(1), dim3(64), 0, s, t.mm);
  HGS_LAUNCH_CHECK("knn_init", s, false);
  hipLaunchKernelGGL(knn_bbox_kernel, dim3(nblk < 1024 ? nblk : 1024), dim3(256), 0, s, xyz, P, t.mm);
  HGS_LAUNCH_CHECK("knn_bbox", s, false);
  hipLaunchKernelGGL(knn_morton_kernel, dim3(nblk), dim3(256), 0, s, xyz, P, t.mm, t.keys_in, t.vals_in);
  HGS_LAUNCH_CHECK("knn_morton", s, false);
  int rc = sort_pairs(t.keys_in, t.vals_in, t.keys_out, t.vals_out, t.sort_tmp, (uint32_t)P, 30, s, false);
  if (rc) return rc;
  const int nbox = (P + kRun - 1) / kRun;
  hipLaunchKernelGGL(knn_gather_boxes_kernel, dim3(nbox), dim3(kRun), 0, s, xyz, P, t.vals_out, t.sorted, t.boxes);
  HGS_LAUNCH_CHECK("knn_gather_boxes", s, false);
  hipLaunchKernelGGL(knn_search_kernel, dim3(nblk), dim3(256), 0, s, t.sorted, P, t.boxes, nbox, out_mean_d2);
  HGS_LAUNCH_CHECK("knn_search", s, false);
  return HGS_OK;
}

}  // extern "C"
