// The view reach of every node of a hierarchy: the rule of hgs.hierarchy.view_reach (the spec) on the device.
//
//   rule       a view set is C closed boxes [lo_c, hi_c] of camera positions (a single position: lo == hi).  For node p
//              D2(p) = min over c of box_d2(box(p), lo_c, hi_c) (lod_cut.h: node_size's squared distance with the
//              viewpoint widened to a box) and reach(p) = D2 > 0 ? extent(p) / sqrtf(D2) : FLT_MAX: the largest
//              node_size any viewpoint of the set can see the node at.  sqrt and the division are monotone, so one of
//              each per node, behind the minimum, gives the bits of max over c of extent / sqrtf(d2(p, c)).
//   pass       hr_reach_kernel: one thread per node holds its two box words in registers and walks a range of regions.
//              A region's six floats are read at a wave-uniform address, so they arrive in scalar registers and feed the
//              vector subtractions directly: no LDS, no barrier, 13.5 vector instructions per (node, region) pair (6 sub,
//              3 max3, a mul and a pk_mul, 2 add, half a min3) and nothing else in the loop.  The pass is bound by their
//              issue, not by bytes: 0.97 of the calibrated issue rate at 50 M nodes under 4 096 views.
//   split      blockIdx.y takes a slice of whole slabs of kReachSlab regions.  One slice where the node workgroups
//              alone fill the GPU: the thread then writes reach itself.  Several where they do not (few nodes, many
//              views): the slices fold into D2's BIT PATTERN with atomicMin -- d2 is a non-negative float, so unsigned
//              order is float order, and a minimum is exact in any order: deterministic -- and hr_finish_kernel turns
//              D2 into reach.  No float atomics, no host wait: the call is asynchronous on the caller's stream.
#include "lod_cut.h"

namespace hgs {
namespace {

constexpr int kHrThreads = 256;
constexpr int kReachSlab = 256;          // regions: the unit a slice of the region range is made of
constexpr int64_t kHrTargetWgs = 2048;   // workgroups wanted in flight (256 CUs x 8) before the region range is split
constexpr int64_t kHrMaxSlices = 4096;

__device__ __forceinline__ float reach_of(float extent, float d2) {
#pragma clang fp contract(off)
  const float s = extent / sqrtf(d2);
  return d2 > 0.0f ? s : kFltMax;
}

// grid (node workgroups, slices).  kSplit: fold into d2_bits (preset to all ones); else write reach.
template <bool kSplit>
__global__ __launch_bounds__(kHrThreads) void hr_reach_kernel(const float* __restrict__ boxes, int32_t N,
                                                              const float* __restrict__ regions, int32_t C,
                                                              int32_t per_slice, float* __restrict__ reach,
                                                              uint32_t* __restrict__ d2_bits) {
  const int64_t i = (int64_t)blockIdx.x * kHrThreads + threadIdx.x;
  if (i >= N) return;
  const float4 mn = reinterpret_cast<const float4*>(boxes)[i * 2 + 0];
  const float4 mx = reinterpret_cast<const float4*>(boxes)[i * 2 + 1];
  const int32_t c0 = (int32_t)blockIdx.y * per_slice;
  const int32_t c1 = min(C, c0 + per_slice);
  float best = __builtin_inff();
#pragma unroll 4
  for (int32_t c = c0; c < c1; ++c) {
    const float* r = regions + (int64_t)c * 6;       // wave-uniform: scalar loads
    best = fminf(best, box_d2(mn, mx, Vec3{r[0], r[1], r[2]}, Vec3{r[3], r[4], r[5]}));
  }
  if constexpr (kSplit) atomicMin(d2_bits + i, __float_as_uint(best));
  else reach[i] = reach_of(mn.w, best);
}

__global__ __launch_bounds__(kHrThreads) void hr_finish_kernel(const float* __restrict__ boxes, int32_t N,
                                                               const uint32_t* __restrict__ d2_bits,
                                                               float* __restrict__ reach) {
  const int64_t i = (int64_t)blockIdx.x * kHrThreads + threadIdx.x;
  if (i < N) reach[i] = reach_of(boxes[i * 8 + 3], __uint_as_float(d2_bits[i]));
}

struct HrTmp { uint32_t* d2_bits; };   // [N]

HrTmp carve_hr_tmp(Carver& c, int64_t N) {
  HrTmp t;
  t.d2_bits = c.take<uint32_t>((size_t)N);
  return t;
}

// regions per slice (a multiple of kReachSlab) -> the slices are ceil(C / that)
int32_t hr_per_slice(int64_t N, int32_t C) {
  const int64_t nblk = (N + kHrThreads - 1) / kHrThreads, slabs = ((int64_t)C + kReachSlab - 1) / kReachSlab;
  int64_t slices = (kHrTargetWgs + nblk - 1) / nblk;
  slices = slices < slabs ? slices : slabs;
  slices = slices < kHrMaxSlices ? slices : kHrMaxSlices;
  const int64_t slabs_per = (slabs + slices - 1) / slices;
  return (int32_t)(slabs_per * kReachSlab);
}

}  // namespace

size_t hier_reach_tmp_bytes(int64_t N, int32_t C) {
  (void)C;                 // the workspace is D2's bit patterns whatever the split
  Carver c(nullptr);
  carve_hr_tmp(c, N);
  return c.bytes(0);       // tmp is required to be kAlign-aligned: no slack
}

int launch_hier_reach(const float* boxes, int64_t N, const float* regions, int32_t C, float* reach, void* tmp,
                      hipStream_t s) {
  Carver c(tmp);
  const HrTmp t = carve_hr_tmp(c, N);
  const int32_t per = hr_per_slice(N, C);
  const unsigned nblk = (unsigned)((N + kHrThreads - 1) / kHrThreads), slices = (unsigned)((C + per - 1) / per);
  if (slices == 1) {
    hipLaunchKernelGGL(hr_reach_kernel<false>, dim3(nblk, 1), dim3(kHrThreads), 0, s, boxes, (int32_t)N, regions, C, per,
                       reach, t.d2_bits);
    HGS_LAUNCH_CHECK("hr_reach", s, false);
    return HGS_OK;
  }
  HGS_HIP(hipMemsetAsync(t.d2_bits, 0xff, (size_t)N * sizeof(uint32_t), s));
  hipLaunchKernelGGL(hr_reach_kernel<true>, dim3(nblk, slices), dim3(kHrThreads), 0, s, boxes, (int32_t)N, regions, C, per,
                     reach, t.d2_bits);
  HGS_LAUNCH_CHECK("hr_reach_split", s, false);
  hipLaunchKernelGGL(hr_finish_kernel, dim3(nblk), dim3(kHrThreads), 0, s, boxes, (int32_t)N, t.d2_bits, reach);
  HGS_LAUNCH_CHECK("hr_finish", s, false);
  return HGS_OK;
}

}  // namespace hgs
