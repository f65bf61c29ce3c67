// Budgeted residency of a hierarchy's attribute rows (include/hgs.h: hgs_resid_*, hgs_host_alloc): the "VRAM-budgeted
// streaming LOD" that BASELINE configs[4] names and the reference's hierarchy viewer offers as `--budget <MB>`
// (README.md:233-235; implemented in the un-vendored SIBR viewer -- nothing to restate, the mechanism here is this
// library's own).  The full attribute arrays live in pinned host memory mapped into the device's address space; the GPU
// keeps B rows in slot arrays and an int32 per Gaussian saying where (or that not).  Misses of a view are fetched by a
// kernel that READS THE HOST ROWS ITSELF (one packed 256-byte row per Gaussian, sixteen lanes per row, one float4 each:
// resid_fetch_kernel below) -- PCIe carries exactly the rows that are needed, there is no host-side gather and no
// staging copy.  Slots are recycled by age (frames since the last use) when the free list runs out.
#include "common.h"
#include "half_widen.h"

namespace hgs {
namespace {

constexpr int kAges = 64;

// `weights` (nullable): interpolation weight of every entry of the cut.  The rasterizer's in-op LOD gather does not read
// the parent row of an entry whose weight is exactly 1 (gaussian_math.h: lod_row_gather -- 82 % of the entries of the
// 50 M-node render loop), so that parent need not be resident for this entry: its slot is reported as the node's own.
__global__ __launch_bounds__(256) void resid_mark_kernel(const int32_t* __restrict__ ri, const int32_t* __restrict__ pi,
                                                         const float* __restrict__ weights, int n, int G,
                                                         int32_t* __restrict__ slot_of, uint32_t* __restrict__ stamp,
                                                         uint32_t frame, int32_t* __restrict__ miss_ids,
                                                         uint32_t* __restrict__ counters, int32_t* __restrict__ ro,
                                                         int32_t* __restrict__ po) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const bool need_parent = !weights || weights[i] != 1.0f;
  const int32_t ids[2] = {ri[i], pi[i]};
  int32_t out[2];
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const int32_t id = ids[k];
    if (id < 0 || id >= G) { counters[2] = 1u; out[k] = -1; continue; }     // (benign race: every writer stores 1)
    if (k == 1 && !need_parent) { out[1] = out[0]; continue; }
    int32_t s = slot_of[id];
    if (s == -1) {                               // absent: exactly one lane of the launch queues it
      const int32_t old = atomicCAS(&slot_of[id], -1, -2);
      if (old == -1) miss_ids[atomicAdd(&counters[0], 1u)] = id;
      s = old >= 0 ? old : -2;
    }
    if (s >= 0) stamp[s] = frame;                // (same value from every writer)
    out[k] = s;
  }
  ro[i] = out[0];
  po[i] = out[1];
}

__global__ __launch_bounds__(256) void resid_remap_kernel(const int32_t* __restrict__ ri, const int32_t* __restrict__ pi,
                                                          const float* __restrict__ weights, int n,
                                                          const int32_t* __restrict__ slot_of,
                                                          int32_t* __restrict__ ro, int32_t* __restrict__ po) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int32_t r = slot_of[ri[i]];
  ro[i] = r;
  po[i] = (!weights || weights[i] != 1.0f) ? slot_of[pi[i]] : r;
}

// occupied slots by age = min(frame - stamp, kAges - 1)
__global__ __launch_bounds__(256) void resid_age_hist_kernel(const uint32_t* __restrict__ stamp,
                                                             const int32_t* __restrict__ id_of_slot, int B, uint32_t frame,
                                                             uint32_t* __restrict__ hist) {
  __shared__ uint32_t h[kAges];
  if (threadIdx.x < kAges) h[threadIdx.x] = 0u;
  __syncthreads();
  for (int s = blockIdx.x * 256 + threadIdx.x; s < B; s += gridDim.x * 256)
    if (id_of_slot[s] >= 0) atomicAdd(&h[min(frame - stamp[s], (uint32_t)(kAges - 1))], 1u);
  __syncthreads();
  if (threadIdx.x < kAges && h[threadIdx.x]) atomicAdd(&hist[threadIdx.x], h[threadIdx.x]);
}

// frees every occupied slot of age >= min_age (>= 1: a row used this frame stays); counters[1] = top of the free stack
__global__ __launch_bounds__(256) void resid_evict_kernel(const uint32_t* __restrict__ stamp, int32_t* __restrict__ id_of_slot,
                                                          int32_t* __restrict__ slot_of, int B, uint32_t frame,
                                                          uint32_t min_age, int32_t* __restrict__ free_list,
                                                          uint32_t* __restrict__ counters) {
  const int s = blockIdx.x * 256 + threadIdx.x;
  if (s >= B) return;
  const int32_t id = id_of_slot[s];
  if (id < 0 || min(frame - stamp[s], (uint32_t)(kAges - 1)) < min_age) return;
  slot_of[id] = -1;
  id_of_slot[s] = -1;
  free_list[atomicAdd(&counters[1], 1u)] = s;
}

// Host layout: ONE PACKED ROW of HGS_RESID_HOST_ROW_FLOATS = 64 floats (256 B, four PCIe read requests of 64 B) per
// Gaussian --
//   [0, 3 M) SH coefficients   [48, 52) rotation   [52, 55) mean   [55, 58) scale   [58] opacity   rest: padding
// -- instead of the five attribute arrays: a row fetched from five arrays costs seven 64-byte requests for 236 useful
// bytes (measured: 21 GB/s of rows over a link that moves twice that in requests).  Sixteen lanes per missing row, four
// rows per wave: every lane loads ONE float4 of the packed row (one fully coalesced 256-byte read per row), lanes 0..11
// store the SH block, lane 12 the quaternion, lanes 13 / 14 mean, scale and opacity; the slot comes from the top of the
// free stack.  The miss list is sorted for bulk fetches (hgs/residency.py), so a wave's four rows are usually
// neighbours in host memory.
template <bool kVec>
__global__ __launch_bounds__(256) void resid_fetch_kernel(const int32_t* __restrict__ miss_ids, uint32_t m,
                                                          const int32_t* __restrict__ free_list, uint32_t free_top,
                                                          int32_t* __restrict__ slot_of, int32_t* __restrict__ id_of_slot,
                                                          uint32_t* __restrict__ stamp, uint32_t frame,
                                                          const float4* __restrict__ src, hgs_resid_rows dst, int nsh) {
  const uint32_t j = blockIdx.x * 16u + (threadIdx.x >> 4);
  const int sub = threadIdx.x & 15;
  if (j >= m) return;
  const size_t id = (size_t)miss_ids[j];
  const size_t s = (size_t)free_list[free_top - 1u - j];
  const float4 v = src[id * (HGS_RESID_HOST_ROW_FLOATS / 4) + sub];
  if (sub < 12) {
    if (kVec) {                                    // nsh % 4 == 0: slot rows of the SH array are 16-byte aligned
      if (sub * 4 < nsh) reinterpret_cast<float4*>(dst.shs + s * nsh)[sub] = v;
    } else {
      const float c[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (int t = 0; t < 4; ++t)
        if (sub * 4 + t < nsh) dst.shs[s * nsh + sub * 4 + t] = c[t];
    }
  } else if (sub == 12) {
    reinterpret_cast<float4*>(dst.rotations)[s] = v;
  } else if (sub == 13) {                          // floats 52..55: mean, scale.x
    dst.means3D[s * 3 + 0] = v.x; dst.means3D[s * 3 + 1] = v.y; dst.means3D[s * 3 + 2] = v.z;
    dst.scales[s * 3 + 0] = v.w;
  } else if (sub == 14) {                          // floats 56..59: scale.y, scale.z, opacity, pad
    dst.scales[s * 3 + 1] = v.x; dst.scales[s * 3 + 2] = v.y;
    dst.opacities[s] = v.z;
    slot_of[id] = (int32_t)s;
    id_of_slot[s] = (int32_t)id;
    stamp[s] = frame;
  }
}

// ---- half-precision host rows (HGS_RESID_HOST_ROW_BYTES_HALF, include/hgs.h) ---------------------------------------
// A row is eight 16-byte chunks: chunks 0..5 hold 48 halves of SH, chunk 6 rotation (4 halves), scale (3) and opacity
// (1), chunk 7 the mean as three float32 and four bytes of padding.

// (widen_half / widen8, IEEE half bits -> float, exact: half_widen.h -- one text with K1's half-row LOD route)

// float -> IEEE half (bits), the narrowing rule of include/hgs.h: round to nearest even with subnormal halves kept, a
// finite value beyond +-65504 becomes +-65504 (narrowing never makes an infinity), NaN stays NaN (0x7e00 under its sign),
// an infinity stays one
__device__ __forceinline__ uint32_t narrow_half(float x) {
  if (x != x) return (__float_as_uint(x) >> 16 & 0x8000u) | 0x7e00u;
  if (fabsf(x) <= 3.402823466e+38f) x = fminf(fmaxf(x, -65504.0f), 65504.0f);       // (false for infinities)
  const _Float16 h = (_Float16)x;
  uint16_t b;
  __builtin_memcpy(&b, &h, 2);
  return b;
}

__device__ __forceinline__ uint32_t narrow2(float lo, float hi) { return narrow_half(lo) | narrow_half(hi) << 16; }

// Eight lanes per missing row, eight rows per wave, 32 rows per workgroup: every lane loads ONE 16-byte chunk of the
// packed half row (one fully coalesced 128-byte read per row = two 64-byte PCIe requests), widens it and stores floats
// into the slot arrays the float kernel fills: lanes 0..5 the SH block, lane 6 rotation, scale and opacity, lane 7 the
// mean and the bookkeeping.  Slot assignment as in resid_fetch_kernel: miss j takes free_list[free_top - 1 - j].
template <bool kVec>
__global__ __launch_bounds__(256) void resid_fetch_half_kernel(const int32_t* __restrict__ miss_ids, uint32_t m,
                                                               const int32_t* __restrict__ free_list, uint32_t free_top,
                                                               int32_t* __restrict__ slot_of, int32_t* __restrict__ id_of_slot,
                                                               uint32_t* __restrict__ stamp, uint32_t frame,
                                                               const uint4* __restrict__ src, hgs_resid_rows dst, int nsh) {
  const uint32_t j = blockIdx.x * 32u + (threadIdx.x >> 3);
  const int sub = threadIdx.x & 7;
  if (j >= m) return;
  const size_t id = (size_t)miss_ids[j];
  const size_t s = (size_t)free_list[free_top - 1u - j];
  const uint4 v = src[id * (HGS_RESID_HOST_ROW_BYTES_HALF / 16) + sub];
  if (sub < 6) {
    float f[8];
    widen8(v, f);
    if (kVec) {                                    // nsh % 4 == 0: slot rows of the SH array are 16-byte aligned
      float4* row = reinterpret_cast<float4*>(dst.shs + s * nsh);
      if (sub * 8 < nsh) row[sub * 2] = make_float4(f[0], f[1], f[2], f[3]);
      if (sub * 8 + 4 < nsh) row[sub * 2 + 1] = make_float4(f[4], f[5], f[6], f[7]);
    } else {
#pragma unroll
      for (int t = 0; t < 8; ++t)
        if (sub * 8 + t < nsh) dst.shs[s * nsh + sub * 8 + t] = f[t];
    }
  } else if (sub == 6) {                           // halves 48..55: rotation, scale, opacity
    float f[8];
    widen8(v, f);
    reinterpret_cast<float4*>(dst.rotations)[s] = make_float4(f[0], f[1], f[2], f[3]);
    dst.scales[s * 3 + 0] = f[4]; dst.scales[s * 3 + 1] = f[5]; dst.scales[s * 3 + 2] = f[6];
    dst.opacities[s] = f[7];
  } else {                                         // bytes 112..127: mean (float32), padding
    dst.means3D[s * 3 + 0] = __uint_as_float(v.x);
    dst.means3D[s * 3 + 1] = __uint_as_float(v.y);
    dst.means3D[s * 3 + 2] = __uint_as_float(v.z);
    slot_of[id] = (int32_t)s;
    id_of_slot[s] = (int32_t)id;
    stamp[s] = frame;
  }
}

// Half SLOTS (hgs_resid_fetch_half_slots): the slot arrays hold the rows as they arrive -- SH, rotation, scale and opacity
// as IEEE half, the mean as float32 -- so a slot costs 6 M + 28 bytes instead of 4 (3 M + 11).  The read is that of
// resid_fetch_half_kernel (eight lanes per row, one 16-byte chunk each); the BITS are copied, nothing is converted:
// lanes 0..5 store the first 6 M bytes of the SH block (kVec: 6 M % 16 == 0 and the array 16-byte aligned -- whole
// chunks; else 2-byte stores, since a slot's row then starts off a 16-byte boundary), lane 6 the rotation (8 bytes),
// the scale (rows are 6 bytes apart: three 2-byte stores) and the opacity (2 bytes), lane 7 the mean and the bookkeeping.
// No store is wider than what it writes: the last slot of a [B] half array may end 2 bytes past a 4-byte boundary.
template <bool kVec>
__global__ __launch_bounds__(256) void resid_fetch_half_slots_kernel(const int32_t* __restrict__ miss_ids, uint32_t m,
                                                                     const int32_t* __restrict__ free_list, uint32_t free_top,
                                                                     int32_t* __restrict__ slot_of, int32_t* __restrict__ id_of_slot,
                                                                     uint32_t* __restrict__ stamp, uint32_t frame,
                                                                     const uint4* __restrict__ src, hgs_resid_rows_half dst,
                                                                     int nsh) {
  const uint32_t j = blockIdx.x * 32u + (threadIdx.x >> 3);
  const int sub = threadIdx.x & 7;
  if (j >= m) return;
  const size_t id = (size_t)miss_ids[j];
  const size_t s = (size_t)free_list[free_top - 1u - j];
  const uint4 v = src[id * (HGS_RESID_HOST_ROW_BYTES_HALF / 16) + sub];
  if (sub < 6) {
    uint16_t* row = static_cast<uint16_t*>(dst.shs) + s * nsh;
    if (kVec) {
      if (sub * 8 < nsh) reinterpret_cast<uint4*>(row)[sub] = v;
    } else {
      const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (int t = 0; t < 8; ++t)
        if (sub * 8 + t < nsh) row[sub * 8 + t] = (uint16_t)(w[t >> 1] >> ((t & 1) * 16));
    }
  } else if (sub == 6) {                           // halves 48..55: rotation, scale, opacity
    static_cast<uint2*>(dst.rotations)[s] = make_uint2(v.x, v.y);
    uint16_t* sc = static_cast<uint16_t*>(dst.scales) + s * 3;
    sc[0] = (uint16_t)v.z; sc[1] = (uint16_t)(v.z >> 16); sc[2] = (uint16_t)v.w;
    static_cast<uint16_t*>(dst.opacities)[s] = (uint16_t)(v.w >> 16);
  } else {                                         // bytes 112..127: mean (float32), padding
    float* mean = static_cast<float*>(dst.means3D) + s * 3;
    mean[0] = __uint_as_float(v.x);
    mean[1] = __uint_as_float(v.y);
    mean[2] = __uint_as_float(v.z);
    slot_of[id] = (int32_t)s;
    id_of_slot[s] = (int32_t)id;
    stamp[s] = frame;
  }
}

// Device attribute arrays -> packed rows in pinned, device-mapped host memory, written by the kernel itself with plain
// 16-byte vector stores (one per lane, a row's lanes adjacent: whole rows leave as 128- / 256-byte writes).  kHalf: eight
// lanes per row in the half layout above; else sixteen lanes per row in the float layout resid_fetch_kernel reads.
// Padding is written as zeros in both.  A row's lanes read consecutive floats of the SH array.
template <bool kHalf>
__global__ __launch_bounds__(256) void resid_pack_kernel(hgs_resid_rows src, size_t G, int nsh, uint4* __restrict__ out) {
  constexpr int kLanes = kHalf ? 8 : 16;
  const size_t g = (size_t)blockIdx.x * (256 / kLanes) + threadIdx.x / kLanes;
  const int sub = threadIdx.x % kLanes;
  if (g >= G) return;
  uint4 v = make_uint4(0u, 0u, 0u, 0u);
  if (kHalf) {
    if (sub < 6) {
      float f[8];
#pragma unroll
      for (int t = 0; t < 8; ++t) f[t] = sub * 8 + t < nsh ? src.shs[g * nsh + sub * 8 + t] : 0.0f;
      v = make_uint4(narrow2(f[0], f[1]), narrow2(f[2], f[3]), narrow2(f[4], f[5]), narrow2(f[6], f[7]));
    } else if (sub == 6) {
      const float* q = src.rotations + g * 4;
      v = make_uint4(narrow2(q[0], q[1]), narrow2(q[2], q[3]), narrow2(src.scales[g * 3 + 0], src.scales[g * 3 + 1]),
                     narrow2(src.scales[g * 3 + 2], src.opacities[g]));
    } else {
      v = make_uint4(__float_as_uint(src.means3D[g * 3 + 0]), __float_as_uint(src.means3D[g * 3 + 1]),
                     __float_as_uint(src.means3D[g * 3 + 2]), 0u);
    }
  } else {
    if (sub < 12) {
      uint32_t w[4];
#pragma unroll
      for (int t = 0; t < 4; ++t) w[t] = sub * 4 + t < nsh ? __float_as_uint(src.shs[g * nsh + sub * 4 + t]) : 0u;
      v = make_uint4(w[0], w[1], w[2], w[3]);
    } else if (sub == 12) {
      const float* q = src.rotations + g * 4;
      v = make_uint4(__float_as_uint(q[0]), __float_as_uint(q[1]), __float_as_uint(q[2]), __float_as_uint(q[3]));
    } else if (sub == 13) {                        // floats 52..55: mean, scale.x
      v = make_uint4(__float_as_uint(src.means3D[g * 3 + 0]), __float_as_uint(src.means3D[g * 3 + 1]),
                     __float_as_uint(src.means3D[g * 3 + 2]), __float_as_uint(src.scales[g * 3 + 0]));
    } else if (sub == 14) {                        // floats 56..59: scale.y, scale.z, opacity, padding
      v = make_uint4(__float_as_uint(src.scales[g * 3 + 1]), __float_as_uint(src.scales[g * 3 + 2]),
                     __float_as_uint(src.opacities[g]), 0u);
    }
  }
  out[g * kLanes + sub] = v;
}

}  // namespace
}  // namespace hgs

using namespace hgs;

extern "C" {

void* hgs_host_alloc(size_t bytes) {
  void* p = nullptr;
  if (hipHostMalloc(&p, bytes ? bytes : 1, hipHostMallocPortable | hipHostMallocMapped) != hipSuccess) {
    (void)hipGetLastError();
    return nullptr;
  }
  return p;
}

void hgs_host_free(void* p) {
  if (p) (void)hipHostFree(p);
}

static int read_words(uint32_t* dst_host, const uint32_t* src_dev, int words, hipStream_t s) {
  HGS_HIP(hipMemcpyAsync(dst_host, src_dev, sizeof(uint32_t) * words, hipMemcpyDeviceToHost, s));
  HGS_HIP(wait_stream(s));
  return HGS_OK;
}

int hgs_resid_mark(const int32_t* render_indices, const int32_t* parent_indices, const float* weights, int32_t n, int32_t G,
                   int32_t* slot_of, uint32_t* stamp, uint32_t frame, int32_t* miss_ids, uint32_t* counters,
                   int32_t* ro, int32_t* po, uint32_t* miss_count_host, hgs_stream_t stream, int device) {
  if (!miss_count_host) { set_error("null miss_count_host"); return HGS_ERR_INVALID; }
  *miss_count_host = 0;
  if (n <= 0) return HGS_OK;
  if (!render_indices || !parent_indices || !slot_of || !stamp || !miss_ids || !counters || !ro || !po || G <= 0) {
    set_error("null argument");
    return HGS_ERR_INVALID;
  }
  HGS_HIP(hipSetDevice(device));
  hipStream_t s = static_cast<hipStream_t>(stream);
  HGS_HIP(hipMemsetAsync(counters, 0, 4 * sizeof(uint32_t), s));
  hipLaunchKernelGGL(resid_mark_kernel, dim3((n + 255) / 256), dim3(256), 0, s, render_indices, parent_indices, weights, n, G,
                     slot_of, stamp, frame, miss_ids, counters, ro, po);
  HGS_LAUNCH_CHECK("resid_mark", s, false);
  uint32_t w[4] = {0, 0, 0, 0};
  int rc = read_words(w, counters, 4, s);
  if (rc) return rc;
  // the misses queued so far are reported on the error path too: the caller has to take them back out of the queue
  *miss_count_host = w[0];
  if (w[2]) { set_error("a render / parent index lies outside [0, %d)", G); return HGS_ERR_INVALID; }
  return HGS_OK;
}

int hgs_resid_evict(uint32_t* stamp, int32_t* id_of_slot, int32_t* slot_of, int32_t B, uint32_t frame, uint32_t need,
                    int32_t* free_list, uint32_t* counters, uint32_t* free_top_inout_host, hgs_stream_t stream,
                    int device) {
  if (!stamp || !id_of_slot || !slot_of || !free_list || !counters || !free_top_inout_host || B <= 0) {
    set_error("null argument");
    return HGS_ERR_INVALID;
  }
  if (*free_top_inout_host >= need) return HGS_OK;
  HGS_HIP(hipSetDevice(device));
  hipStream_t s = static_cast<hipStream_t>(stream);
  uint32_t* hist_dev = counters + 4;              // counters: [0] misses [1] free-stack top [2] error [4 .. 4 + kAges) ages
  HGS_HIP(hipMemsetAsync(hist_dev, 0, kAges * sizeof(uint32_t), s));
  const int grid = B < 256 * 1024 ? (B + 255) / 256 : 1024;
  hipLaunchKernelGGL(resid_age_hist_kernel, dim3(grid), dim3(256), 0, s, stamp, id_of_slot, B, frame, hist_dev);
  HGS_LAUNCH_CHECK("resid_age_hist", s, false);
  uint32_t hist[kAges];
  int rc = read_words(hist, hist_dev, kAges, s);
  if (rc) return rc;
  const uint32_t missing = need - *free_top_inout_host;
  uint64_t acc = 0;
  int min_age = 0;
  for (int a = kAges - 1; a >= 1; --a) {
    acc += hist[a];
    if (acc >= missing) { min_age = a; break; }
  }
  if (min_age == 0) {
    set_error("the view needs %u more rows than the budget of %d rows can free (rows unused this frame: %llu)", missing, B,
              (unsigned long long)acc);
    return HGS_ERR_CAPACITY;
  }
  HGS_HIP(hipMemcpyAsync(counters + 1, free_top_inout_host, sizeof(uint32_t), hipMemcpyHostToDevice, s));
  hipLaunchKernelGGL(resid_evict_kernel, dim3((B + 255) / 256), dim3(256), 0, s, stamp, id_of_slot, slot_of, B, frame,
                     (uint32_t)min_age, free_list, counters);
  HGS_LAUNCH_CHECK("resid_evict", s, false);
  uint32_t top = 0;
  rc = read_words(&top, counters + 1, 1, s);
  if (rc) return rc;
  *free_top_inout_host = top;
  return HGS_OK;
}

// what every fetch call checks before its launch (m > 0); *d receives the device-side address of the packed host rows
static int resid_fetch_checks(const int32_t* miss_ids, uint32_t m, const int32_t* free_list, uint32_t free_top,
                              const int32_t* slot_of, const int32_t* id_of_slot, const uint32_t* stamp,
                              const void* host_rows_packed, const void* slot_rows, int32_t M, int device, void** d) {
  if (!miss_ids || !free_list || !slot_of || !id_of_slot || !stamp || !host_rows_packed || !slot_rows) {
    set_error("null argument");
    return HGS_ERR_INVALID;
  }
  if (M < 1 || M > 16) { set_error("M = %d SH coefficients per channel: 1..16", M); return HGS_ERR_INVALID; }
  if (free_top < m) { set_error("%u free slots for %u missing rows", free_top, m); return HGS_ERR_CAPACITY; }
  HGS_HIP(hipSetDevice(device));
  // the packed host rows by their device-side address
  *d = nullptr;
  if (hipHostGetDevicePointer(d, const_cast<void*>(host_rows_packed), 0) != hipSuccess) {
    (void)hipGetLastError();
    set_error("the packed host rows must come from hgs_host_alloc (pinned, device-mapped)");
    return HGS_ERR_INVALID;
  }
  return HGS_OK;
}

// the two fetch calls into float slots: the checks, one launch
static int resid_fetch(bool half, const int32_t* miss_ids, uint32_t m, const int32_t* free_list, uint32_t free_top,
                       int32_t* slot_of, int32_t* id_of_slot, uint32_t* stamp, uint32_t frame, const void* host_rows_packed,
                       const hgs_resid_rows* slot_rows, int32_t M, hgs_stream_t stream, int device) {
  if (m == 0) return HGS_OK;
  void* d = nullptr;
  const int rc = resid_fetch_checks(miss_ids, m, free_list, free_top, slot_of, id_of_slot, stamp, host_rows_packed, slot_rows,
                                    M, device, &d);
  if (rc) return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (((uintptr_t)d | (uintptr_t)slot_rows->rotations) & 15u) {
    set_error("packed host rows / slot rotations must be 16-byte aligned");
    return HGS_ERR_INVALID;
  }
  const bool vec = ((M * 3) & 3) == 0 && (((uintptr_t)slot_rows->shs & 15u) == 0);
  if (half) {
    const uint4* src = static_cast<const uint4*>(d);
    if (vec)
      hipLaunchKernelGGL(resid_fetch_half_kernel<true>, dim3((m + 31) / 32), dim3(256), 0, s, miss_ids, m, free_list,
                         free_top, slot_of, id_of_slot, stamp, frame, src, *slot_rows, M * 3);
    else
      hipLaunchKernelGGL(resid_fetch_half_kernel<false>, dim3((m + 31) / 32), dim3(256), 0, s, miss_ids, m, free_list,
                         free_top, slot_of, id_of_slot, stamp, frame, src, *slot_rows, M * 3);
    HGS_LAUNCH_CHECK("resid_fetch_half", s, false);
    return HGS_OK;
  }
  const float4* src = static_cast<const float4*>(d);
  if (vec)
    hipLaunchKernelGGL(resid_fetch_kernel<true>, dim3((m + 15) / 16), dim3(256), 0, s, miss_ids, m, free_list, free_top,
                       slot_of, id_of_slot, stamp, frame, src, *slot_rows, M * 3);
  else
    hipLaunchKernelGGL(resid_fetch_kernel<false>, dim3((m + 15) / 16), dim3(256), 0, s, miss_ids, m, free_list, free_top,
                       slot_of, id_of_slot, stamp, frame, src, *slot_rows, M * 3);
  HGS_LAUNCH_CHECK("resid_fetch", s, false);
  return HGS_OK;
}

int hgs_resid_fetch(const int32_t* miss_ids, uint32_t m, const int32_t* free_list, uint32_t free_top, int32_t* slot_of,
                    int32_t* id_of_slot, uint32_t* stamp, uint32_t frame, const float* host_rows_packed,
                    const hgs_resid_rows* slot_rows, int32_t M, hgs_stream_t stream, int device) {
  return resid_fetch(false, miss_ids, m, free_list, free_top, slot_of, id_of_slot, stamp, frame, host_rows_packed, slot_rows,
                     M, stream, device);
}

int hgs_resid_fetch_half(const int32_t* miss_ids, uint32_t m, const int32_t* free_list, uint32_t free_top, int32_t* slot_of,
                         int32_t* id_of_slot, uint32_t* stamp, uint32_t frame, const void* host_rows_packed,
                         const hgs_resid_rows* slot_rows, int32_t M, hgs_stream_t stream, int device) {
  return resid_fetch(true, miss_ids, m, free_list, free_top, slot_of, id_of_slot, stamp, frame, host_rows_packed, slot_rows,
                     M, stream, device);
}

int hgs_resid_fetch_half_slots(const int32_t* miss_ids, uint32_t m, const int32_t* free_list, uint32_t free_top,
                               int32_t* slot_of, int32_t* id_of_slot, uint32_t* stamp, uint32_t frame,
                               const void* host_rows_packed, const hgs_resid_rows_half* slot_rows, int32_t M,
                               hgs_stream_t stream, int device) {
  if (m == 0) return HGS_OK;
  void* d = nullptr;
  const int rc = resid_fetch_checks(miss_ids, m, free_list, free_top, slot_of, id_of_slot, stamp, host_rows_packed, slot_rows,
                                    M, device, &d);
  if (rc) return rc;
  if (!slot_rows->means3D || !slot_rows->shs || !slot_rows->opacities || !slot_rows->scales || !slot_rows->rotations) {
    set_error("null argument");
    return HGS_ERR_INVALID;
  }
  // the rotation of a slot is stored with one 8-byte access, the mean as floats, everything else as halves
  if (((uintptr_t)d & 15u) || ((uintptr_t)slot_rows->rotations & 7u) || ((uintptr_t)slot_rows->means3D & 3u) ||
      (((uintptr_t)slot_rows->shs | (uintptr_t)slot_rows->scales | (uintptr_t)slot_rows->opacities) & 1u)) {
    set_error("packed host rows must be 16-byte aligned, half slot rotations 8-byte aligned (means 4, the other arrays 2)");
    return HGS_ERR_INVALID;
  }
  hipStream_t s = static_cast<hipStream_t>(stream);
  const uint4* src = static_cast<const uint4*>(d);
  const bool vec = ((M * 3) & 7) == 0 && (((uintptr_t)slot_rows->shs & 15u) == 0);      // 6 M % 16 == 0
  if (vec)
    hipLaunchKernelGGL(resid_fetch_half_slots_kernel<true>, dim3((m + 31) / 32), dim3(256), 0, s, miss_ids, m, free_list,
                       free_top, slot_of, id_of_slot, stamp, frame, src, *slot_rows, M * 3);
  else
    hipLaunchKernelGGL(resid_fetch_half_slots_kernel<false>, dim3((m + 31) / 32), dim3(256), 0, s, miss_ids, m, free_list,
                       free_top, slot_of, id_of_slot, stamp, frame, src, *slot_rows, M * 3);
  HGS_LAUNCH_CHECK("resid_fetch_half_slots", s, false);
  return HGS_OK;
}

int hgs_resid_pack_rows(const hgs_resid_rows* src, int64_t G, int32_t M, int32_t half, void* host_rows_packed,
                        hgs_stream_t stream, int device) {
  if (!src || !host_rows_packed || !src->means3D || !src->shs || !src->opacities || !src->scales || !src->rotations) {
    set_error("null argument");
    return HGS_ERR_INVALID;
  }
  if (G < 0 || G > 0x7fffffffLL) { set_error("G = %lld rows: 0..2^31-1", (long long)G); return HGS_ERR_INVALID; }
  if (M < 1 || M > 16) { set_error("M = %d SH coefficients per channel: 1..16", M); return HGS_ERR_INVALID; }
  if (half != 0 && half != 1) { set_error("half = %d: 0 (float rows) or 1 (half rows)", half); return HGS_ERR_INVALID; }
  if (G == 0) return HGS_OK;
  HGS_HIP(hipSetDevice(device));
  hipStream_t s = static_cast<hipStream_t>(stream);
  void* d = nullptr;
  if (hipHostGetDevicePointer(&d, host_rows_packed, 0) != hipSuccess) {
    (void)hipGetLastError();
    set_error("the packed host rows must come from hgs_host_alloc (pinned, device-mapped)");
    return HGS_ERR_INVALID;
  }
  if ((uintptr_t)d & 15u) { set_error("packed host rows must be 16-byte aligned"); return HGS_ERR_INVALID; }
  uint4* out = static_cast<uint4*>(d);
  if (half)
    hipLaunchKernelGGL(resid_pack_kernel<true>, dim3((unsigned)((G + 31) / 32)), dim3(256), 0, s, *src, (size_t)G, M * 3, out);
  else
    hipLaunchKernelGGL(resid_pack_kernel<false>, dim3((unsigned)((G + 15) / 16)), dim3(256), 0, s, *src, (size_t)G, M * 3, out);
  HGS_LAUNCH_CHECK("resid_pack", s, false);
  return HGS_OK;
}

int hgs_resid_remap(const int32_t* render_indices, const int32_t* parent_indices, const float* weights, int32_t n,
                    const int32_t* slot_of, int32_t* ro, int32_t* po, hgs_stream_t stream, int device) {
  if (n <= 0) return HGS_OK;
  if (!render_indices || !parent_indices || !slot_of || !ro || !po) { set_error("null argument"); return HGS_ERR_INVALID; }
  HGS_HIP(hipSetDevice(device));
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(resid_remap_kernel, dim3((n + 255) / 256), dim3(256), 0, s, render_indices, parent_indices, weights,
                     n, slot_of, ro, po);
  HGS_LAUNCH_CHECK("resid_remap", s, false);
  return HGS_OK;
}

}  // extern "C"
