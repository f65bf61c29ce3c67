// Similarity transform of a hierarchy: the rule of hgs.hierarchy.transform_hierarchy (the spec) on the device.
//
//   rule       x' = s R x + t.  Per row: xyz'_a = ((R_a0 x_0 + R_a1 x_1) + R_a2 x_2) s + t_a; rots' = q_R (x) rots (Hamilton,
//              norms kept); log_scales' = log_scales + log s; SH band 0 keeps its bits, band l: c'_m = sum_m' D_l[m][m'] c_m'
//              per channel; alpha and the node records are copied.  Per box: lo'_a = (sum_b (R_ab >= 0 ? R_ab lo_b :
//              R_ab hi_b)) s + t_a, hi' with lo and hi swapped, the extent = the largest edge of the rounded box in
//              float32.  Arithmetic in double, contraction off, every sum in the spec's order, one rounding to float32:
//              the bits are the spec's.  The SH blocks are consumed as given (the host derives them).
//   rows       tf_rows_kernel<M>: one workgroup per kTfRows rows (all G: the tail behind the nodes included).  The rows'
//              SH block is contiguous in memory: it is staged in LDS in 16-byte pieces (12 M a multiple of 16 and both
//              bases aligned) or 4-byte pieces, at a row stride of 3 M | 1 words (odd: the 48-word stride of M = 16 would
//              put rows r and r + 2 on one bank of the 32 a 4-byte access sees); one thread per (row, channel) --
//              channel-major, so a wave walks consecutive rows, conflict free -- rotates bands 1.. in place in LDS; the block is
//              written back in the pieces it came in.  The first kTfRows threads carry one row's xyz, log_scales, rots
//              and alpha through registers meanwhile.  The 101 doubles of the parameter block are kernel arguments.
//   boxes      tf_boxes_kernel: one thread per node, both float4 of the box read, both written; the workgroup copies its
//              nodes' records when the output is another array.
//
// In place (an output array == the input array) or out of place (no overlap): a workgroup reads its rows before it
// writes them, and no workgroup touches another's rows.  No workspace, no host wait.
#include "hier_nodes.h"

#pragma clang fp contract(off)

namespace hgs {
namespace {

constexpr int kTfThreads = 256;
constexpr int kTfRows = 128;          // rows per workgroup of the row kernel

// Band L of one (row, channel) column in LDS, in place: p -> coefficient 0 of the channel, 3 words between coefficients.
template <int L>
__device__ __forceinline__ void tf_band(float* p, const double* D) {
  constexpr int n = 2 * L + 1, o = L * L;
  double c[n];
#pragma unroll
  for (int k = 0; k < n; ++k) c[k] = (double)p[(o + k) * 3];
#pragma unroll
  for (int m = 0; m < n; ++m) {
    double acc = D[m * n] * c[0];
#pragma unroll
    for (int k = 1; k < n; ++k) acc = acc + D[m * n + k] * c[k];
    p[(o + m) * 3] = (float)acc;
  }
}

template <int M>
__global__ __launch_bounds__(kTfThreads) void tf_rows_kernel(HierRowsIn in, HierRows out, int64_t G,
                                                             hgs_hier_transform_args a, int shs16) {
  constexpr int W = 3 * M, kStride = W | 1;
  __shared__ float sh[M == 1 ? 1 : kTfRows * kStride];
  const int64_t r0 = (int64_t)blockIdx.x * kTfRows;
  const int rows = (int)min((int64_t)kTfRows, G - r0);
  const float* src = in.shs + r0 * W;
  float* dst = out.shs + r0 * W;
  const int tid = threadIdx.x;

  // ---- the SH block: global -> LDS
  if constexpr (M == 1) {
    if (src != dst)
      for (int u = tid; u < rows * W; u += kTfThreads) dst[u] = src[u];
  } else if (shs16) {
    const int L = rows * (W / 4);
    for (int u = tid; u < L; u += kTfThreads) {
      const float4 v = reinterpret_cast<const float4*>(src)[u];
      const int f = 4 * u, row = f / W, k = f - row * W;
      float* p = &sh[row * kStride + k];
      p[0] = v.x; p[1] = v.y; p[2] = v.z; p[3] = v.w;
    }
  } else {
    for (int u = tid; u < rows * W; u += kTfThreads) {
      const int row = u / W, k = u - row * W;
      sh[row * kStride + k] = src[u];
    }
  }

  // ---- one row's xyz, log_scales, rots, alpha: read, computed and written by one thread
  if (tid < rows) {
    const int64_t r = r0 + tid;
    const double x0 = in.xyz[r * 3 + 0], x1 = in.xyz[r * 3 + 1], x2 = in.xyz[r * 3 + 2];
    const double l0 = in.log_scales[r * 3 + 0], l1 = in.log_scales[r * 3 + 1], l2 = in.log_scales[r * 3 + 2];
    const float4 qf = reinterpret_cast<const float4*>(in.rots)[r];
    const double b0 = qf.x, b1 = qf.y, b2 = qf.z, b3 = qf.w;
    const double a0 = a.q[0], a1 = a.q[1], a2 = a.q[2], a3 = a.q[3];
    if (in.alpha != out.alpha) out.alpha[r] = in.alpha[r];
    out.xyz[r * 3 + 0] = (float)(((a.R[0] * x0 + a.R[1] * x1) + a.R[2] * x2) * a.s + a.t[0]);
    out.xyz[r * 3 + 1] = (float)(((a.R[3] * x0 + a.R[4] * x1) + a.R[5] * x2) * a.s + a.t[1]);
    out.xyz[r * 3 + 2] = (float)(((a.R[6] * x0 + a.R[7] * x1) + a.R[8] * x2) * a.s + a.t[2]);
    out.log_scales[r * 3 + 0] = (float)(l0 + a.log_s);
    out.log_scales[r * 3 + 1] = (float)(l1 + a.log_s);
    out.log_scales[r * 3 + 2] = (float)(l2 + a.log_s);
    float4 o;
    o.x = (float)(a0 * b0 - a1 * b1 - a2 * b2 - a3 * b3);
    o.y = (float)(a0 * b1 + a1 * b0 + a2 * b3 - a3 * b2);
    o.z = (float)(a0 * b2 - a1 * b3 + a2 * b0 + a3 * b1);
    o.w = (float)(a0 * b3 + a1 * b2 - a2 * b1 + a3 * b0);
    reinterpret_cast<float4*>(out.rots)[r] = o;
  }

  if constexpr (M > 1) {
    __syncthreads();
    // ---- bands 1.. of every (row, channel), channel-major
    for (int item = tid; item < 3 * kTfRows; item += kTfThreads) {
      const int ch = item / kTfRows, row = item - ch * kTfRows;
      if (row < rows) {
        float* p = &sh[row * kStride + ch];
        tf_band<1>(p, a.D1);
        if constexpr (M >= 9) tf_band<2>(p, a.D2);
        if constexpr (M >= 16) tf_band<3>(p, a.D3);
      }
    }
    __syncthreads();
    // ---- LDS -> global
    if (shs16) {
      const int L = rows * (W / 4);
      for (int u = tid; u < L; u += kTfThreads) {
        const int f = 4 * u, row = f / W, k = f - row * W;
        const float* p = &sh[row * kStride + k];
        reinterpret_cast<float4*>(dst)[u] = make_float4(p[0], p[1], p[2], p[3]);
      }
    } else {
      for (int u = tid; u < rows * W; u += kTfThreads) {
        const int row = u / W, k = u - row * W;
        dst[u] = sh[row * kStride + k];
      }
    }
  }
}

__global__ __launch_bounds__(kTfThreads) void tf_boxes_kernel(HierRowsIn in, HierRows out, int64_t N, hgs_hier_transform_args a) {
  const int64_t n0 = (int64_t)blockIdx.x * kTfThreads;
  const int64_t i = n0 + threadIdx.x;
  if (i < N) {
    const float4 mn = reinterpret_cast<const float4*>(in.boxes)[i * 2 + 0];
    const float4 mx = reinterpret_cast<const float4*>(in.boxes)[i * 2 + 1];
    const double lo[3] = {mn.x, mn.y, mn.z}, hi[3] = {mx.x, mx.y, mx.z};
    float l[3], h[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const double r0 = a.R[3 * k], r1 = a.R[3 * k + 1], r2 = a.R[3 * k + 2];
      const double tl0 = r0 * (r0 >= 0.0 ? lo[0] : hi[0]), tl1 = r1 * (r1 >= 0.0 ? lo[1] : hi[1]),
                   tl2 = r2 * (r2 >= 0.0 ? lo[2] : hi[2]);
      const double th0 = r0 * (r0 >= 0.0 ? hi[0] : lo[0]), th1 = r1 * (r1 >= 0.0 ? hi[1] : lo[1]),
                   th2 = r2 * (r2 >= 0.0 ? hi[2] : lo[2]);
      l[k] = (float)(((tl0 + tl1) + tl2) * a.s + a.t[k]);
      h[k] = (float)(((th0 + th1) + th2) * a.s + a.t[k]);
    }
    const float e = fmaxf(fmaxf(h[0] - l[0], h[1] - l[1]), h[2] - l[2]);
    reinterpret_cast<float4*>(out.boxes)[i * 2 + 0] = make_float4(l[0], l[1], l[2], e);
    reinterpret_cast<float4*>(out.boxes)[i * 2 + 1] = make_float4(h[0], h[1], h[2], mx.w);
  }
  if (in.nodes != out.nodes) {
    const int L = (int)min((int64_t)kTfThreads, N - n0) * kNodeInts;
    for (int u = threadIdx.x; u < L; u += kTfThreads) out.nodes[n0 * kNodeInts + u] = in.nodes[n0 * kNodeInts + u];
  }
}

}  // namespace

int launch_hier_transform(const hgs_hier_view& in, const hgs_hier_view& out, const hgs_hier_transform_args& a, bool shs16,
                          hipStream_t s) {
  const HierRowsIn i = HierRowsIn::of(in);
  const HierRows o = HierRows::of(out);
  const int64_t G = in.G, N = in.N;
  const dim3 grid((unsigned)((G + kTfRows - 1) / kTfRows)), block(kTfThreads);
  const int s16 = shs16 ? 1 : 0;
  switch (in.M) {
    case 1: hipLaunchKernelGGL(tf_rows_kernel<1>, grid, block, 0, s, i, o, G, a, s16); break;
    case 4: hipLaunchKernelGGL(tf_rows_kernel<4>, grid, block, 0, s, i, o, G, a, s16); break;
    case 9: hipLaunchKernelGGL(tf_rows_kernel<9>, grid, block, 0, s, i, o, G, a, s16); break;
    default: hipLaunchKernelGGL(tf_rows_kernel<16>, grid, block, 0, s, i, o, G, a, s16); break;
  }
  HGS_LAUNCH_CHECK("tf_rows", s, false);
  hipLaunchKernelGGL(tf_boxes_kernel, dim3((unsigned)((N + kTfThreads - 1) / kTfThreads)), block, 0, s, i, o, N, a);
  HGS_LAUNCH_CHECK("tf_boxes", s, false);
  return HGS_OK;
}

}  // namespace hgs
