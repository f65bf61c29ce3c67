// K1 (preprocess forward) and K8 (preprocess backward): one lane per Gaussian.
//
// Restates the per-Gaussian stage of the op called at
// gaussian_renderer/__init__.py:105-113 (reference source absent; algorithm per
// SURVEY.md App. A 1-6, 9-10).  HBM-bound streaming kernels: 236 B in per Gaussian
// at SH degree 3 (fwd), 236 B in + 248 B out (bwd).
#include "gaussian_math.h"
#include "half_widen.h"

#include <stdlib.h>

#include <mutex>

namespace hgs {

namespace {

struct CamLds {
  float vm[16];
  float pm[16];
  float cam[3];
};

__device__ __forceinline__ void load_camera(const hgs_raster_args& a, CamLds& c) {
  // 35 floats, wave-uniform addresses -> scalar loads.
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    c.vm[i] = a.viewmatrix[i];
    c.pm[i] = a.projmatrix[i];
  }
  c.cam[0] = a.campos[0];
  c.cam[1] = a.campos[1];
  c.cam[2] = a.campos[2];
}

__device__ __forceinline__ uint32_t wave_sum_u32(uint32_t v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

__device__ __forceinline__ void load_sh(const float* __restrict__ shs, int idx, int M, float sh[48]) {
  const int n = M * 3;
  const float* src = shs + (size_t)idx * n;
  if ((n & 3) == 0) {
    const float4* s4 = reinterpret_cast<const float4*>(src);
#pragma unroll
    for (int i = 0; i < 12; ++i) {
      if (i * 4 < n) {
        const float4 v = s4[i];
        sh[i * 4 + 0] = v.x;
        sh[i * 4 + 1] = v.y;
        sh[i * 4 + 2] = v.z;
        sh[i * 4 + 3] = v.w;
      }
    }
  } else {
#pragma unroll
    for (int i = 0; i < 48; ++i)
      if (i < n) sh[i] = src[i];
  }
}

// 16-byte stores of a Gaussian's M*3 SH gradients (12 x dwordx4 per lane at M = 16)
__device__ __forceinline__ void store_sh(float* __restrict__ dshs, int idx, int M, const float v[48]) {
  const int n = M * 3;
  float* dst = dshs + (size_t)idx * n;
  if ((n & 3) == 0) {
    float4* d4 = reinterpret_cast<float4*>(dst);
#pragma unroll
    for (int i = 0; i < 12; ++i)
      if (i * 4 < n) d4[i] = make_float4(v[i * 4 + 0], v[i * 4 + 1], v[i * 4 + 2], v[i * 4 + 3]);
  } else {
#pragma unroll
    for (int i = 0; i < 48; ++i)
      if (i < n) dst[i] = v[i];
  }
}

// ---- cooperative (coalesced) access to the [P, M, 3] SH arrays --------------------------------------
// One lane per Gaussian wants 12*M contiguous bytes (192 B at M = 16): issued per lane, every dwordx4
// instruction touches 64 different cache lines (measured 2.6 TB/s).  Instead the workgroup streams its
// 256 Gaussians' coefficients as one contiguous block (lane i <-> 16 bytes i) through LDS, rows padded
// by 4 floats so that the per-lane ds_read_b128 / ds_write_b128 are bank-conflict free.
__device__ __forceinline__ int sh_row_stride(int n) { return n + 4; }   // floats

__device__ __forceinline__ void coop_load_sh(const float* __restrict__ shs, int block_first, int P, int n,
                                             float* lds) {
  const int count = min(kPreBlock, P - block_first);           // Gaussians in this workgroup
  const int vecs = count * n / 4;
  const float4* src = reinterpret_cast<const float4*>(shs + (size_t)block_first * n);
  const int stride = sh_row_stride(n);
  for (int v = threadIdx.x; v < vecs; v += kPreBlock) {
    const int e = v * 4;
    const int gsn = e / n, off = e - gsn * n;
    *reinterpret_cast<float4*>(lds + gsn * stride + off) = src[v];
  }
}

// The same block load split in two: ISSUE the workgroup's coalesced 16-byte loads into registers (up to 12 per lane),
// COMMIT them to the padded LDS rows later -- whatever the kernel computes in between runs under the loads' latency.
__device__ __forceinline__ void coop_issue_sh(const float* __restrict__ shs, int block_first, int P, int n,
                                              float4 (&reg)[12]) {
  const int vecs = min(kPreBlock, P - block_first) * n / 4;
  const float4* src = reinterpret_cast<const float4*>(shs + (size_t)block_first * n);
#pragma unroll
  for (int k = 0; k < 12; ++k) {
    const int v = (int)threadIdx.x + k * kPreBlock;
    reg[k] = v < vecs ? src[v] : make_float4(0.f, 0.f, 0.f, 0.f);
  }
}
__device__ __forceinline__ void coop_commit_sh(const float4 (&reg)[12], int block_first, int P, int n, float* lds) {
  const int vecs = min(kPreBlock, P - block_first) * n / 4;
  const int stride = sh_row_stride(n);
#pragma unroll
  for (int k = 0; k < 12; ++k) {
    const int v = (int)threadIdx.x + k * kPreBlock;
    if (v < vecs) {
      const int e = v * 4;
      const int gsn = n == 48 ? e / 48 : e / n, off = e - gsn * n;
      *reinterpret_cast<float4*>(lds + gsn * stride + off) = reg[k];
    }
  }
}

template <bool ACC>
__device__ __forceinline__ void coop_store_sh(float* __restrict__ dst_all, int block_first, int P, int n,
                                              const float* lds) {
  const int count = min(kPreBlock, P - block_first);
  const int vecs = count * n / 4;
  float4* dst = reinterpret_cast<float4*>(dst_all + (size_t)block_first * n);
  const int stride = sh_row_stride(n);
  if (ACC) {
    // accumulate: reads of the old gradients are issued four at a time ahead of the adds and stores -- a
    // load/add/store chain per 16 bytes would serialise on memory latency, twelve in flight spill registers
    constexpr int kGroup = 4;
    for (int base = 0; base < vecs; base += kGroup * kPreBlock) {
      float4 old[kGroup];
#pragma unroll
      for (int it = 0; it < kGroup; ++it) {
        const int v = base + it * kPreBlock + (int)threadIdx.x;
        old[it] = v < vecs ? dst[v] : make_float4(0.f, 0.f, 0.f, 0.f);
      }
#pragma unroll
      for (int it = 0; it < kGroup; ++it) {
        const int v = base + it * kPreBlock + (int)threadIdx.x;
        if (v < vecs) {
          const int e = v * 4;
          const int gsn = e / n, off = e - gsn * n;
          const float4 val = *reinterpret_cast<const float4*>(lds + gsn * stride + off);
          dst[v] = make_float4(val.x + old[it].x, val.y + old[it].y, val.z + old[it].z, val.w + old[it].w);
        }
      }
    }
  } else {
    for (int v = threadIdx.x; v < vecs; v += kPreBlock) {
      const int e = v * 4;
      const int gsn = e / n, off = e - gsn * n;
      dst[v] = *reinterpret_cast<const float4*>(lds + gsn * stride + off);
    }
  }
}

__device__ __forceinline__ void lds_row_read(const float* lds, int n, float v[48]) {
  const float* row = lds + threadIdx.x * sh_row_stride(n);
#pragma unroll
  for (int i = 0; i < 12; ++i) {
    if (i * 4 < n) {
      const float4 t = *reinterpret_cast<const float4*>(row + i * 4);
      v[i * 4 + 0] = t.x; v[i * 4 + 1] = t.y; v[i * 4 + 2] = t.z; v[i * 4 + 3] = t.w;
    }
  }
}
__device__ __forceinline__ void lds_row_write(float* lds, int n, const float v[48]) {
  float* row = lds + threadIdx.x * sh_row_stride(n);
#pragma unroll
  for (int i = 0; i < 12; ++i)
    if (i * 4 < n) *reinterpret_cast<float4*>(row + i * 4) = make_float4(v[i * 4 + 0], v[i * 4 + 1], v[i * 4 + 2], v[i * 4 + 3]);
}

// ---- split SH storage (hgs_raster_args.shs_rest): features_dc [P,1,3] and features_rest [P,M-1,3] ----------
// Same LDS row layout as above ([dc | rest], stride 3M + 4), filled from / drained to two contiguous global
// blocks.  3 and 45 floats per Gaussian are not multiples of 4, so the 16-byte global accesses straddle rows and
// the LDS side is done per float; a workgroup's block starts 16-byte aligned (256 Gaussians x 12 / 180 bytes).
__device__ __forceinline__ void coop_load_seg(const float* __restrict__ src_all, int block_first, int P, int nseg,
                                              int col0, int stride, float* lds) {
  const int count = min(kPreBlock, P - block_first);
  const int total = count * nseg;
  const float* src = src_all + (size_t)block_first * nseg;
  const int vecs = total >> 2;
  for (int v = threadIdx.x; v < vecs; v += kPreBlock) {
    const float4 t = reinterpret_cast<const float4*>(src)[v];
    const float tv[4] = {t.x, t.y, t.z, t.w};
    int gsn = (v * 4) / nseg, off = v * 4 - gsn * nseg;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      lds[gsn * stride + col0 + off] = tv[c];
      if (++off == nseg) { off = 0; ++gsn; }
    }
  }
  for (int e = vecs * 4 + threadIdx.x; e < total; e += kPreBlock) {
    const int gsn = e / nseg, off = e - gsn * nseg;
    lds[gsn * stride + col0 + off] = src[e];
  }
}

template <bool ACC>
__device__ __forceinline__ void coop_store_seg(float* __restrict__ dst_all, int block_first, int P, int nseg,
                                               int col0, int stride, const float* lds) {
  const int count = min(kPreBlock, P - block_first);
  const int total = count * nseg;
  float* dst = dst_all + (size_t)block_first * nseg;
  const int vecs = total >> 2;
  for (int v = threadIdx.x; v < vecs; v += kPreBlock) {
    float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
    if (ACC) o = reinterpret_cast<const float4*>(dst)[v];
    float tv[4];
    int gsn = (v * 4) / nseg, off = v * 4 - gsn * nseg;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      tv[c] = lds[gsn * stride + col0 + off];
      if (++off == nseg) { off = 0; ++gsn; }
    }
    reinterpret_cast<float4*>(dst)[v] = make_float4(tv[0] + o.x, tv[1] + o.y, tv[2] + o.z, tv[3] + o.w);
  }
  for (int e = vecs * 4 + threadIdx.x; e < total; e += kPreBlock) {
    const int gsn = e / nseg, off = e - gsn * nseg;
    const float v = lds[gsn * stride + col0 + off];
    dst[e] = ACC ? dst[e] + v : v;
  }
}

// per-lane access to the split layout (mostly-culled workgroups of K1)
__device__ __forceinline__ void load_sh_split(const float* __restrict__ dc, const float* __restrict__ rest, int idx,
                                              int M, float sh[48]) {
  sh[0] = dc[(size_t)idx * 3 + 0]; sh[1] = dc[(size_t)idx * 3 + 1]; sh[2] = dc[(size_t)idx * 3 + 2];
  const int nr = (M - 1) * 3;
  const float* src = rest + (size_t)idx * nr;
#pragma unroll
  for (int i = 0; i < 45; ++i)
    if (i < nr) sh[3 + i] = src[i];
}

// In-kernel LOD interpolation: the workgroup's rows are gathered (node row, parent row) and lerped on their way into
// LDS, one lane per 16-byte chunk so that every 192-byte row is read as contiguous segments.  (node, parent, weight) of
// row i sit in the pad floats of its LDS slot (written by lane i before the barrier that precedes this call).
__device__ __forceinline__ void coop_gather_sh(const float* __restrict__ shs, int block_first, int P, int n, float* lds) {
  const int count = min(kPreBlock, P - block_first);
  const int cpr = n / 4;                                        // 16-byte chunks per row
  const int stride = sh_row_stride(n);
  const float4* src = reinterpret_cast<const float4*>(shs);
  for (int v = threadIdx.x; v < count * cpr; v += kPreBlock) {
    const int row = v / cpr, c = v - row * cpr;
    const float* pad = lds + row * stride + n;
    const size_t r = (size_t)__float_as_uint(pad[0]), p = (size_t)__float_as_uint(pad[1]);
    const float w = pad[2], u = 1.0f - w;
    const float4 x = src[r * cpr + c], y = src[p * cpr + c];     // (weight 1: p = r, see lod_row_gather)
    *reinterpret_cast<float4*>(lds + row * stride + c * 4) =
        make_float4(lod_lerp(x.x, y.x, w, u), lod_lerp(x.y, y.y, w, u), lod_lerp(x.z, y.z, w, u), lod_lerp(x.w, y.w, w, u));
  }
}
__device__ __forceinline__ void load_sh_lod(const hgs_raster_args& a, int idx, float sh[48]) {
  const LodRow l = lod_row_gather<true>(a, idx);
  const int n = a.M * 3;
  const float* x = a.shs + l.r * n;
  const float* y = a.shs + l.p * n;
#pragma unroll
  for (int i = 0; i < 48; ++i)
    if (i < n) sh[i] = lod_lerp(x[i], y[i], l.w, l.u);
}

// ---- half-precision attribute rows (hgs_raster_args.lod_half_rows: the half SLOTS of the budgeted residency) ----------------
// The forms of the LOD loaders above (gaussian_math.h: load_scale_rot / load_opacity; coop_gather_sh, load_sh_lod) for
// arrays of IEEE half: every value is widened as it is loaded (half_widen.h: exact) and then takes the float32 path -- the
// same lod_row_gather (weight 1: p = r, the loads stay unconditional), the same separately rounded lod_lerp, the same
// hemisphere flip -- so the row is bit for bit the one float32 arrays holding the widened values give.  The mean stays
// float32 (load_mean).  A gathered row is 6 M + 28 bytes instead of 4 (3 M + 11).
//
// The cooperative SH gather, one lane per 16-byte chunk = eight halves, which become two float4 of the row's LDS slot
// (the layout coop_gather_sh writes; at M = 16 a row is six chunks).  Needs n % 8 == 0 (6 M % 16 == 0: rows start on
// 16-byte boundaries, and so do the LDS slots at a stride of n + 4 floats).
__device__ __forceinline__ void coop_gather_sh_half(const void* __restrict__ shs, int block_first, int P, int n, float* lds) {
  const int count = min(kPreBlock, P - block_first);
  const int cpr = n / 8;                                        // 16-byte chunks per row
  const int stride = sh_row_stride(n);
  const uint4* src = static_cast<const uint4*>(shs);
  for (int v = threadIdx.x; v < count * cpr; v += kPreBlock) {
    const int row = v / cpr, c = v - row * cpr;
    const float* pad = lds + row * stride + n;
    const size_t r = (size_t)__float_as_uint(pad[0]), p = (size_t)__float_as_uint(pad[1]);
    const float w = pad[2], u = 1.0f - w;
    const uint4 xb = src[r * cpr + c], yb = src[p * cpr + c];   // (weight 1: p = r, see lod_row_gather)
    float x[8], y[8];
    widen8(xb, x);
    widen8(yb, y);
    float4* dst = reinterpret_cast<float4*>(lds + row * stride + c * 8);
    dst[0] = make_float4(lod_lerp(x[0], y[0], w, u), lod_lerp(x[1], y[1], w, u), lod_lerp(x[2], y[2], w, u), lod_lerp(x[3], y[3], w, u));
    dst[1] = make_float4(lod_lerp(x[4], y[4], w, u), lod_lerp(x[5], y[5], w, u), lod_lerp(x[6], y[6], w, u), lod_lerp(x[7], y[7], w, u));
  }
}
// per lane, 2-byte loads: the route of every other M (a row of 6 M bytes then starts off a 16-byte boundary)
__device__ __forceinline__ void load_sh_lod_half(const hgs_raster_args& a, int idx, float sh[48]) {
  const LodRow l = lod_row_gather<true>(a, idx);
  const int n = a.M * 3;
  const uint16_t* x = reinterpret_cast<const uint16_t*>(a.shs) + l.r * n;
  const uint16_t* y = reinterpret_cast<const uint16_t*>(a.shs) + l.p * n;
#pragma unroll
  for (int i = 0; i < 48; ++i)
    if (i < n) sh[i] = lod_lerp(widen_half(x[i]), widen_half(y[i]), l.w, l.u);
}
// scales: three 2-byte loads (rows are 6 bytes apart); rotation: one 8-byte load
__device__ __forceinline__ void load_scale_rot_half(const hgs_raster_args& a, int idx, float sc[3], float q[4]) {
  const LodRow l = lod_row_gather<true>(a, idx);
  const uint16_t* s16 = reinterpret_cast<const uint16_t*>(a.scales);
#pragma unroll
  for (int k = 0; k < 3; ++k) sc[k] = lod_lerp(widen_half(s16[l.r * 3 + k]), widen_half(s16[l.p * 3 + k]), l.w, l.u);
  const uint2 ra = reinterpret_cast<const uint2*>(a.rotations)[l.r], rb = reinterpret_cast<const uint2*>(a.rotations)[l.p];
  const float4 qa = make_float4(widen_half(ra.x & 0xffffu), widen_half(ra.x >> 16), widen_half(ra.y & 0xffffu), widen_half(ra.y >> 16));
  const float4 qb = make_float4(widen_half(rb.x & 0xffffu), widen_half(rb.x >> 16), widen_half(rb.y & 0xffffu), widen_half(rb.y >> 16));
  const float sgn = (qa.x * qb.x + qa.y * qb.y + qa.z * qb.z + qa.w * qb.w) < 0.0f ? -1.0f : 1.0f;
  q[0] = lod_lerp(qa.x, sgn * qb.x, l.w, l.u); q[1] = lod_lerp(qa.y, sgn * qb.y, l.w, l.u);
  q[2] = lod_lerp(qa.z, sgn * qb.z, l.w, l.u); q[3] = lod_lerp(qa.w, sgn * qb.w, l.w, l.u);
}
__device__ __forceinline__ float load_opacity_half(const hgs_raster_args& a, int idx) {
  const LodRow l = lod_row_gather<true>(a, idx);
  const uint16_t* o16 = reinterpret_cast<const uint16_t*>(a.opacities);
  return lod_lerp(widen_half(o16[l.r]), widen_half(o16[l.p]), l.w, l.u);
}


// ---- M = 16, plain [P, 16, 3] layout: the coefficient block straight into LDS ----------------------------------------------
// K1 at M = 16 used to stage the workgroup's whole block (256 rows x 52 floats = 53 KB) through LDS and to hold its
// twelve 16-byte loads per lane in registers across the double-precision chain: 53 KB and 144 registers both capped the
// kernel at 3 waves per SIMD.  `global_load_lds_dwordx4` writes the rows into LDS without passing through registers
// (nothing to hold across the chain); the image is UNPADDED (the DMA's destination is the wave's base + 16 * lane: no
// room for pad), so the bank swizzle is applied on the SOURCE address of the DMA and on the read, never on the
// destination (cdna_hip_programming.md rule 21).  (Round 5 also built the block as two half rows -- every line requested
// twice -- and as two row groups, and K1 as a geometry kernel + a colour kernel on a second stream: all measured slower,
// profiles/r05_k1_layouts.txt, r05_k1_split_ab.txt; removed in round 6.)
typedef const void __attribute__((address_space(1))) * gptr_t;
typedef void __attribute__((address_space(3))) * lptr_t;

// rgb and (JAC) d(rgb)/d(direction) sums over the four coefficients [K0, K0 + 4); same order of additions as the
// one-block loop (k ascending), so the two routes give the same bits
template <bool JAC, int K0>
__device__ __forceinline__ void sh48_accumulate4(int deg, float dx, float dy, float dz, const float sh[12], float rgb[3],
                                                 float J[9]) {
  const int nb = (deg + 1) * (deg + 1);
  float b[16];
  sh_basis(deg, dx, dy, dz, b);
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    if (K0 + k < nb) {                                     // (explicit FMAs: the same bits in every instantiation)
      rgb[0] = __builtin_fmaf(b[K0 + k], sh[k * 3 + 0], rgb[0]);
      rgb[1] = __builtin_fmaf(b[K0 + k], sh[k * 3 + 1], rgb[1]);
      rgb[2] = __builtin_fmaf(b[K0 + k], sh[k * 3 + 2], rgb[2]);
    }
  }
  if constexpr (JAC) {
    float dbx[16], dby[16], dbz[16];
    sh_basis_grad(deg, dx, dy, dz, dbx, dby, dbz);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (K0 + k < nb) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          J[0 + c] = __builtin_fmaf(dbx[K0 + k], sh[k * 3 + c], J[0 + c]);
          J[3 + c] = __builtin_fmaf(dby[K0 + k], sh[k * 3 + c], J[3 + c]);
          J[6 + c] = __builtin_fmaf(dbz[K0 + k], sh[k * 3 + c], J[6 + c]);
        }
      }
    }
  }
}
// the same from global memory (mostly-culled workgroups: visible lanes only), 48 bytes at a time
template <bool JAC>
__device__ __forceinline__ void sh48_row_from_global(const float* __restrict__ shs, int idx, int deg, float dx, float dy,
                                                     float dz, float rgb[3], float J[9]) {
  const float4* src = reinterpret_cast<const float4*>(shs + (size_t)idx * 48);
  const int nb = (deg + 1) * (deg + 1);
  float sh[12];
#define HGS_SH48_Q(Q)                                                                         \
  if (Q * 4 < nb) {                                                                           \
    _Pragma("unroll") for (int c = 0; c < 3; ++c) {                                           \
      const float4 t = src[Q * 3 + c];                                                        \
      sh[c * 4 + 0] = t.x; sh[c * 4 + 1] = t.y; sh[c * 4 + 2] = t.z; sh[c * 4 + 3] = t.w;     \
    }                                                                                         \
    sh48_accumulate4<JAC, Q * 4>(deg, dx, dy, dz, sh, rgb, J);                                \
  }
  HGS_SH48_Q(0) HGS_SH48_Q(1) HGS_SH48_Q(2) HGS_SH48_Q(3)
#undef HGS_SH48_Q
}

// All 256 rows at once (48 KB: three workgroups per compute unit -- enough, because the DMA keeps 48 KB per workgroup in
// flight without a register).  A row = 12 chunks of 16 bytes at row * 192; row r keeps chunk c in slot (c + f(r)) mod 12,
// f(r) = bits 2..3 of r: the 16 rows of a ds_read_b128 lane group then cover all 16 bank groups (192 r mod 256 takes four
// values).  Only the chunks the active degree needs are fetched.
constexpr int kK1ImageBytes = kPreBlock * 192;

__device__ __forceinline__ void sh48_issue_rows(const float* __restrict__ shs, int block_first, int P, int nchunks,
                                                float* lds) {
  const int count = min(kPreBlock, P - block_first);
  const char* src = reinterpret_cast<const char*>(shs + (size_t)block_first * 48);
  const int wave_base = (int)(threadIdx.x & ~63u);
  constexpr int kPer = 12;                                      // DMA instructions per lane
#pragma unroll
  for (int k = 0; k < kPer; ++k) {
    const int slot = k * kPreBlock + (int)threadIdx.x;          // linear 16-byte slot of the LDS image
    const int row_l = slot / 12, cs = slot - row_l * 12;
    int c = cs - ((row_l >> 2) & 3);                             // the logical chunk this slot keeps
    c = c < 0 ? c + 12 : c;
    const int row = row_l;
    char* dst = reinterpret_cast<char*>(lds) + (size_t)(k * kPreBlock + wave_base) * 16;   // wave-uniform
    if (row < count && c < nchunks)
      __builtin_amdgcn_global_load_lds((gptr_t)(src + (size_t)row * 192 + c * 16), (lptr_t)dst, 16, 0, 0);
  }
}
// row `row_l` of the image, coefficients [4 Q, 4 Q + 4): 12 floats
template <int Q>
__device__ __forceinline__ void sh48_read_row_quarter(const float* lds, int row_l, float v[12]) {
  const int f = (row_l >> 2) & 3;
  const float* row = lds + row_l * 48;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    int sl = Q * 3 + c + f;
    sl = sl >= 12 ? sl - 12 : sl;
    const float4 t = *reinterpret_cast<const float4*>(row + sl * 4);
    v[c * 4 + 0] = t.x; v[c * 4 + 1] = t.y; v[c * 4 + 2] = t.z; v[c * 4 + 3] = t.w;
  }
}
template <bool JAC>
__device__ __forceinline__ void sh48_row_from_lds(const float* lds, int row_l, bool vis, int deg, float dx, float dy,
                                                  float dz, float rgb[3], float J[9]) {
  const int nb = (deg + 1) * (deg + 1);
  float sh[12];
  sh48_read_row_quarter<0>(lds, row_l, sh);
  if (vis) sh48_accumulate4<JAC, 0>(deg, dx, dy, dz, sh, rgb, J);
  if (nb > 4) {                                                  // (uniform)
    sh48_read_row_quarter<1>(lds, row_l, sh);
    if (vis) sh48_accumulate4<JAC, 4>(deg, dx, dy, dz, sh, rgb, J);
    if (nb > 8) {
      sh48_read_row_quarter<2>(lds, row_l, sh);
      if (vis) sh48_accumulate4<JAC, 8>(deg, dx, dy, dz, sh, rgb, J);
      sh48_read_row_quarter<3>(lds, row_l, sh);
      if (vis) sh48_accumulate4<JAC, 12>(deg, dx, dy, dz, sh, rgb, J);
    }
  }
}

// ---- the per-workgroup sums of K1 and their scan -----------------------------------------------------------------------
// Every workgroup of K1 leaves nine sums (its instances, and its instances per tile band); K3 needs their exclusive scans
// over the workgroups.  Rounds 1-4 ran a scan launch between K1 and K3 (6.6 us + a kernel boundary for 140 KB).  With
// `super` given, that launch is gone: K1 also ADDS its sums (fire-and-forget atomics, nobody waits for an answer) to the
// totals of its SUPERBLOCK of kSuper consecutive workgroups, and workgroup b of K3 puts its nine prefixes together
// itself -- the superblock totals before b's superblock plus the raw sums of the workgroups before b inside it: two
// 64-lane loads and two wave reductions per array (binning.hip).  Integer adds commute, the consumer runs behind a
// kernel boundary: no hand-off inside a launch, no assumption about dispatch order, residency or placement.
// The superblock totals must be ZERO when K1 starts; they live in a block owned by the library per (device, stream),
// zeroed when it is created and zeroed again by the counting kernel that follows K3 (tile_bin.hip) -- a workspace carved
// from the caller's memory is fresh on every call and would need a memset launch in front of K1, the launch this is
// there to save.
// instances per tile band of one rectangle, added to the workgroup's LDS counters.  Almost every rectangle lies inside ONE
// band (first and last tile in the same band: seven compares each, no division); one that straddles boundaries counts
// (# of its tiles with id < x) at the boundaries x = b * per it spans, in closed form.
__device__ __forceinline__ void k1_band_count(const Proj& pr, uint32_t touched, int gx, int gy, uint32_t* band_cnt) {
  const int T = gx * gy, per = band_tiles(T), w = pr.maxx - pr.minx;
  const int t_first = pr.miny * gx + pr.minx, t_last = (pr.maxy - 1) * gx + pr.maxx - 1;
  int b_first = 0, b_last = 0;
#pragma unroll
  for (int b = 1; b < kBands; ++b) {
    b_first += (t_first >= b * per) ? 1 : 0;
    b_last += (t_last >= b * per) ? 1 : 0;
  }
  if (b_first == b_last) {
    atomicAdd(&band_cnt[b_first], touched);
  } else {
    int prev = 0;
    for (int b = b_first; b <= b_last; ++b) {
      const int x = min((b + 1) * per, T);
      const int xr = x / gx, xc = x - xr * gx;
      int cnt = (min(max(xr, pr.miny), pr.maxy) - pr.miny) * w;
      if (xr >= pr.miny && xr < pr.maxy) cnt += min(max(xc - pr.minx, 0), w);
      if (cnt > prev) atomicAdd(&band_cnt[b], (uint32_t)(cnt - prev));
      prev = cnt;
    }
  }
}

// The continuous quantities of a visible Gaussian's 2D record (double-precision chain, gaussian_math.h).
struct K1Rec {
  float opac, thr, ext_x, ext_y, invz;
  float gx_hi, gy_hi, gx_lo, gy_lo, A2, B2, C2;
};
__device__ __forceinline__ void k1_continuous(const hgs_raster_args& a, const CamLds& cam, const Proj& pr,
                                              const float p[3], const float sc_act[3], const float q_act[4],
                                              float opac, K1Rec& o) {
  o.opac = opac;
  ProjD pd;
  if (a.cov3D_precomp) {
#pragma unroll
    for (int i = 0; i < 6; ++i) pd.c3[i] = (double)pr.c3[i];
  } else {
    cov3d_from_scale_rot_d(sc_act, a.scale_modifier, q_act, pd);
  }
  project_gaussian_d(p, cam.vm, cam.pm, a.width, a.height, a.tanfovx, a.tanfovy, pr.clampx, pr.clampy, pd);
  // pixel centre as hi + lo floats: the render kernels make it tile-relative before use
  o.gx_hi = (float)pd.px; o.gy_hi = (float)pd.py;
  o.gx_lo = (float)(pd.px - (double)o.gx_hi); o.gy_lo = (float)(pd.py - (double)o.gy_hi);
  // conic pre-scaled to a base-2 exponent: power2 = A2*dx^2 + C2*dy^2 + B2*dx*dy
  const double kLog2e = 1.4426950408889634;
  o.A2 = (float)(-0.5 * kLog2e * pd.conA);
  o.B2 = (float)(-kLog2e * pd.conB);
  o.C2 = (float)(-0.5 * kLog2e * pd.conC);
  // The compositing kernels clamp the exponent at 0 instead of testing its sign ("power > 0 -> skip" never fires
  // for a positive definite conic).  Rounding the three coefficients to float32 must therefore not make an extremely
  // elongated conic indefinite (relative determinant below ~1e-7: sigma of thousands of pixels): if it does, the
  // mixed term is pulled back inside by one part in a million.
  {
    const double lim = 4.0 * (double)o.A2 * (double)o.C2;
    if (!((double)o.B2 * (double)o.B2 < lim)) o.B2 = (float)copysign(sqrt(fmax(lim, 0.0)) * (1.0 - 1.0e-6), (double)o.B2);
  }
  // log-domain skip threshold of the compositing kernels: alpha >= 1/255 <=> power2 >= log2(1/255) - log2(o);
  // 1e-3 guard band so the exact alpha test keeps every borderline decision (opacity <= 0 -> +inf / NaN:
  // never a candidate, exactly like the exact test)
  o.thr = (-7.994353436858858f - 1.0e-3f) - __builtin_amdgcn_logf(opac);
  // Half extents (pixels) of the axis-aligned box around the region where alpha can reach 1/255:
  //   d^T conic d <= T2 = 2 (ln(255 o) + guard)  =>  |dx| <= sqrt(T2 Sigma'_xx), |dy| <= sqrt(T2 Sigma'_yy)
  // (the extent of an ellipse along an axis is set by the COVARIANCE's diagonal: no determinant, no cancellation, so
  // float32 is enough).  T2 = -2 ln 2 * thr: the same logarithm as the skip threshold.  The compositing kernels
  // use the box to decide, once per (tile, Gaussian), which quadrants can be touched at all; it is inflated (the 1e-3
  // guard in the base-2 exponent, 1e-4 relative, 5e-3 px) so that it contains every pixel the exact alpha test could
  // accept.  -1: no pixel ever (o <= ~1/255).
  o.ext_x = -1.0f; o.ext_y = -1.0f;
  {
    const float T2 = -1.3862943611198906f * o.thr;
    const float sxx = (float)pd.a, syy = (float)pd.c;
    if (T2 > 0.0f) {
      const bool sane = sxx < 3.0e38f && syy < 3.0e38f;      // (NaN / inf covariance: never skip on the box)
      o.ext_x = sane ? sqrtf(T2 * sxx) * 1.0001f + 5.0e-3f : 1.0e9f;
      o.ext_y = sane ? sqrtf(T2 * syy) * 1.0001f + 5.0e-3f : 1.0e9f;
    }
  }
  o.invz = (float)pd.itz;
}

// How the M = 16 K1 stores its 64-byte records and 48-byte Jacobian rows: through the wave's own part of the LDS image
// (free once the wave has read its rows; a lane's row of NV 16-byte pieces goes to LDS as it will lie in memory, then
// every store instruction of the wave writes 1 KB of consecutive bytes).  Straight from the lane -- NV instructions
// that each touch 64 different cache lines -- a row-per-lane store pattern is bound by the rate at which the memory
// pipeline takes partial lines, not by bandwidth (8 us more; what each part of K1 costs: profiles/r05_k1_anatomy.txt).
// v[NV] of lane l = the NV consecutive float4 of row (row0 + l) of a [rows, NV] float4 array at dst; rows whose bit in
// `mask` is clear are not written.  wave_lds: >= 64 * NV * 16 bytes private to the calling wave.
template <int NV>
__device__ __forceinline__ void wave_store_rows(float4* __restrict__ dst, size_t row0, const float4 (&v)[NV],
                                                unsigned long long mask, float4* wave_lds) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int q = 0; q < NV; ++q) wave_lds[lane * NV + q] = v[q];
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
  for (int j = 0; j < NV; ++j) {
    const int i = j * 64 + lane;                 // float4 index inside the wave's block of rows
    const int r = i / NV;
    const float4 t = wave_lds[i];
    if ((mask >> r) & 1ull) dst[row0 * NV + i] = t;
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();               // (the next use of wave_lds overwrites it)
}

// The 36-byte Jacobian rows of the wave's 64 Gaussians the same way: nine words per lane at a stride of nine (odd: no
// bank conflict), read back as the 144 consecutive 16-byte pieces they are in memory.  A wave with no visible row
// stores nothing; otherwise all 64 rows are written (the rows of culled Gaussians are never read) -- in the last wave
// also the rows from P up to the next multiple of 64, which is why GeomWs sizes shjac for ceil(P / 64) * 64 rows.
__device__ __forceinline__ void wave_store_jac(float* __restrict__ dst, size_t row0, const float (&J)[9],
                                               unsigned long long mask, float4* wave_lds) {
  const int lane = threadIdx.x & 63;
  float* wl = reinterpret_cast<float*>(wave_lds);
#pragma unroll
  for (int k = 0; k < 9; ++k) wl[lane * 9 + k] = J[k];
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  float4* d4 = reinterpret_cast<float4*>(dst + row0 * kJacStride);      // row0 is a multiple of 64: 16-byte aligned
  if (mask) {
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const int i = j * 64 + lane;
      if (i < 64 * 9 / 4) d4[i] = wave_lds[i];
    }
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();               // (the next use of wave_lds overwrites it)
}

template <bool JAC, bool LOD, bool DEFER, bool H48, bool HALF = false>
                                // JAC: also store d(rgb)/d(direction) for the backward; LOD: in-kernel LOD
                                // interpolation; DEFER: the plain [P, M, 3] coefficient block is loaded into registers
                                // ahead of the double-precision chain (their own instantiations: the extra state
                                // would cost every other caller of K1 its occupancy); H48: plain [P, 16, 3] block
                                // straight into LDS by DMA (above; DEFER and LOD do not apply); HALF: the LOD route
                                // on arrays of IEEE half (lod_half_rows), widened on load -- forward only
__device__ __forceinline__ void preprocess_fwd_body(const hgs_raster_args& a, const GeomWs& g,
                                                    int32_t* __restrict__ radii, uint32_t* __restrict__ super, uint32_t heavy_thr) {
  static_assert(!(H48 && (LOD || DEFER)), "the DMA route is the plain layout's");
  static_assert(!HALF || (LOD && !JAC && !DEFER), "half rows: the in-kernel LOD route, forward only");
  constexpr int kShMask = HALF ? 7 : 3;          // the cooperative SH route moves 16-byte chunks: four floats, eight halves
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  float* lds_sh = reinterpret_cast<float*>(smem_raw);
  __shared__ uint32_t wave_tot[kPreBlock / 64];
  __shared__ uint32_t band_cnt[kBands];          // this workgroup's instances per tile band (binning: band streams)
  if (threadIdx.x < kBands) band_cnt[threadIdx.x] = 0u;
  if (!super && blockIdx.x == 0)        // the scan launch that follows publishes its chunk totals here (common.h)
    for (int t = threadIdx.x; t < (1 + kBands) * scan_chunks(gridDim.x); t += kPreBlock) g.scan_chain[t] = 0ull;
  __syncthreads();
  const int idx = blockIdx.x * kPreBlock + threadIdx.x;
  const int gx = (a.width + kTile - 1) / kTile;
  const int gy = (a.height + kTile - 1) / kTile;
  CamLds cam;
  load_camera(a, cam);

  uint32_t touched = 0;
  Proj pr;
  pr.visible = false;
  float p[3] = {0.f, 0.f, 0.f};
  float sc_act[3] = {0.f, 0.f, 0.f}, q_act[4] = {1.f, 0.f, 0.f, 0.f};   // activated scale / rotation
  float opac = 0.f;
  constexpr bool lod = LOD;
  const int shn = a.M * 3;
  if (idx < a.P) {
    const LodRow lr = lod_row_gather<LOD>(a, idx);     // (its node / parent / weight also steer the cooperative SH gather)
    load_mean<LOD>(a, lr, p);
    if (lod && a.shs && (shn & kShMask) == 0) {
      // the cooperative SH gather below needs every row's (node row, parent row, weight): they ride in the four pad
      // floats at the end of the row's LDS slot
      float* pad = lds_sh + threadIdx.x * sh_row_stride(shn) + shn;
      pad[0] = __uint_as_float((uint32_t)lr.r); pad[1] = __uint_as_float((uint32_t)lr.p); pad[2] = lr.w;
    }
    if constexpr (H48) {
      // every ordinary load of the kernel is issued up here: while the LDS DMA below is in flight the compiler waits
      // for ALL outstanding memory operations at the first use of any load's result
      opac = load_opacity<LOD>(a, idx, nullptr);
      if (a.interpolation_weights && a.num_node_kids && !a.lod_per_pixel)     // (per pixel: the compositing kernels remap alpha)
        opac = lod_opacity(opac, a.interpolation_weights[idx], a.num_node_kids[idx], nullptr);
    }
    if (a.cov3D_precomp) {
#pragma unroll
      for (int i = 0; i < 6; ++i) pr.c3[i] = a.cov3D_precomp[(size_t)idx * 6 + i];
    } else {
      if constexpr (HALF) load_scale_rot_half(a, idx, sc_act, q_act);
      else load_scale_rot<LOD>(a, idx, sc_act, q_act, nullptr);
      float R[9], s[3];
      cov3d_from_scale_rot(sc_act, a.scale_modifier, q_act, pr.c3, R, s);
    }
    project_gaussian(p, cam.vm, cam.pm, a.width, a.height, a.tanfovx, a.tanfovy, gx, gy, pr);
  }
  // ---- the workgroup's sums: instances, and instances per tile band (feed the offsets scans) -----------------------------
  if (idx < a.P && pr.visible) {
    touched = (uint32_t)((pr.maxx - pr.minx) * (pr.maxy - pr.miny));
    k1_band_count(pr, touched, gx, gy, band_cnt);
  }
  {
    const uint32_t ws = wave_sum_u32(touched);
    if ((threadIdx.x & 63) == 0) wave_tot[threadIdx.x >> 6] = ws;
  }
  // SH coefficients: stream the workgroup's block through LDS when most of it is visible (coalesced),
  // fall back to per-lane loads (visible lanes only) when most of the block is culled.
  bool coop = false, deferred = false;
  const bool sh_lds = a.shs && (shn & kShMask) == 0;
  const int nvis = __syncthreads_count(pr.visible);        // (also orders wave_tot / band_cnt)
  if (threadIdx.x < 64) {                                  // (wave 0) raw sums; with `super` also into the superblock totals
    uint32_t mine = 0;
    if (threadIdx.x == 0) {
#pragma unroll
      for (int w = 0; w < kPreBlock / 64; ++w) mine += wave_tot[w];
      g.block_sums[blockIdx.x] = mine;
    } else if (threadIdx.x <= kBands) {
      mine = band_cnt[threadIdx.x - 1];
      g.block_band[(size_t)(threadIdx.x - 1) * (gridDim.x + 1) + blockIdx.x] = mine;
    }
    if (super && threadIdx.x <= kBands && mine)
      __hip_atomic_fetch_add(&super[threadIdx.x * kMaxSuper + (blockIdx.x / kSuper)], mine, __ATOMIC_RELAXED,
                             __HIP_MEMORY_SCOPE_AGENT);
    // ... and an outlier files itself into the heavy list: K3 shares out its emission (binning.hip)
    if (super && threadIdx.x == 0 && heavy_thr != 0u && mine > heavy_thr) {
      const uint32_t slot = __hip_atomic_fetch_add(&super[kHeavyRow], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (slot < (uint32_t)kMaxHeavy) {
        super[kHeavyRow + 1 + 2 * slot] = blockIdx.x;
        super[kHeavyRow + 2 + 2 * slot] = mine;
      }
    }
  }
  // Plain layout: the block's loads are ISSUED here and land while the double-precision chain below runs -- K1 is
  // bound by latency, not by its arithmetic or by HBM.
  float4 shreg[DEFER ? 12 : 1];
  if (sh_lds) {
    coop = nvis * 2 >= kPreBlock;
    if (coop) {
      if constexpr (H48) {
        sh48_issue_rows(a.shs, blockIdx.x * kPreBlock, a.P, ((a.sh_degree + 1) * (a.sh_degree + 1) * 3 + 3) / 4, lds_sh);
      } else if (lod) {
        if constexpr (HALF) coop_gather_sh_half(a.shs, blockIdx.x * kPreBlock, a.P, shn, lds_sh);
        else coop_gather_sh(a.shs, blockIdx.x * kPreBlock, a.P, shn, lds_sh);
      } else if (a.shs_rest) {
        coop_load_seg(a.shs, blockIdx.x * kPreBlock, a.P, 3, 0, sh_row_stride(shn), lds_sh);
        coop_load_seg(a.shs_rest, blockIdx.x * kPreBlock, a.P, shn - 3, 3, sh_row_stride(shn), lds_sh);
      } else if constexpr (DEFER) {
        coop_issue_sh(a.shs, blockIdx.x * kPreBlock, a.P, shn, shreg);
        deferred = true;
      } else {
        coop_load_sh(a.shs, blockIdx.x * kPreBlock, a.P, shn, lds_sh);
      }
    }
  }
  // ---- everything that does not need the coefficients: the double-precision chain, the record's geometry ----------
  int32_t rad = 0;
  uint32_t flags = 0;
  K1Rec rec;
  rec.opac = 0.f; rec.thr = 0.f; rec.ext_x = -1.0f; rec.ext_y = -1.0f; rec.invz = 0.f;
  rec.gx_hi = 0.f; rec.gy_hi = 0.f; rec.gx_lo = 0.f; rec.gy_lo = 0.f; rec.A2 = 0.f; rec.B2 = 0.f; rec.C2 = 0.f;
  if (idx < a.P && pr.visible) {
    rad = (int32_t)pr.rad_f;
    if (pr.clampx) flags |= 8u;
    if (pr.clampy) flags |= 16u;
    if constexpr (!H48) {
      if constexpr (HALF) opac = load_opacity_half(a, idx);
      else opac = load_opacity<LOD>(a, idx, nullptr);
      if (a.interpolation_weights && a.num_node_kids && !a.lod_per_pixel)     // (per pixel: the compositing kernels remap alpha)
        opac = lod_opacity(opac, a.interpolation_weights[idx], a.num_node_kids[idx], nullptr);
    }
    k1_continuous(a, cam, pr, p, sc_act, q_act, opac, rec);
  }
  if constexpr (DEFER) {
    if (deferred) coop_commit_sh(shreg, blockIdx.x * kPreBlock, a.P, shn, lds_sh);
  }
  if constexpr (H48) {      // the DMA has landed before any wave passes the barrier
    if (coop) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  }
  if (coop) __syncthreads();
  // ---- colour ---------------------------------------------------------------------------------------------------------
  float rgb[3] = {0.f, 0.f, 0.f};
  const bool vis = idx < a.P && pr.visible;
  float J[JAC ? 9 : 1];
  if constexpr (H48) {     // (launched with a.shs only)
    float dx, dy, dz;
    unit_dir(p, cam.cam, dx, dy, dz);
    float Jt[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (coop) {                                          // (the barrier above waited for the DMA)
      sh48_row_from_lds<JAC>(lds_sh, (int)threadIdx.x, vis, a.sh_degree, dx, dy, dz, rgb, Jt);
    } else if (vis) {
      sh48_row_from_global<JAC>(a.shs, idx, a.sh_degree, dx, dy, dz, rgb, Jt);
    }
    if constexpr (JAC) {
#pragma unroll
      for (int i = 0; i < 9; ++i) J[i] = Jt[i];
    }
    if (vis) {
      rgb[0] += 0.5f; rgb[1] += 0.5f; rgb[2] += 0.5f;
      if (rgb[0] < 0.f) { rgb[0] = 0.f; flags |= 1u; }
      if (rgb[1] < 0.f) { rgb[1] = 0.f; flags |= 2u; }
      if (rgb[2] < 0.f) { rgb[2] = 0.f; flags |= 4u; }
    }
  } else if (vis) {
    if (a.colors_precomp) {
      rgb[0] = a.colors_precomp[idx * 3 + 0];
      rgb[1] = a.colors_precomp[idx * 3 + 1];
      rgb[2] = a.colors_precomp[idx * 3 + 2];
    } else {
      float sh[48];
      if (coop) lds_row_read(lds_sh, shn, sh);
      else if (lod && HALF) load_sh_lod_half(a, idx, sh);
      else if (lod) load_sh_lod(a, idx, sh);
      else if (a.shs_rest) load_sh_split(a.shs, a.shs_rest, idx, a.M, sh);
      else load_sh(a.shs, idx, a.M, sh);
      float dx, dy, dz;
      unit_dir(p, cam.cam, dx, dy, dz);
      // (the same four-coefficient steps as the half-row route: one piece of code, one rounding behaviour -- the in-kernel
      // LOD interpolation must give the bits of the Python glue's rows rendered by the plain call)
      float Jt[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
      sh48_accumulate4<JAC, 0>(a.sh_degree, dx, dy, dz, sh, rgb, Jt);
      sh48_accumulate4<JAC, 4>(a.sh_degree, dx, dy, dz, sh + 12, rgb, Jt);
      sh48_accumulate4<JAC, 8>(a.sh_degree, dx, dy, dz, sh + 24, rgb, Jt);
      sh48_accumulate4<JAC, 12>(a.sh_degree, dx, dy, dz, sh + 36, rgb, Jt);
      if constexpr (JAC) {
        // (row-per-lane stores: the routes off the M = 16 plain layout; that one stores whole lines, below)
        float* jd = g.shjac + (size_t)idx * kJacStride;
#pragma unroll
        for (int k = 0; k < 9; ++k) jd[k] = Jt[k];
      }
      float r0 = rgb[0], r1 = rgb[1], r2 = rgb[2];
      r0 += 0.5f; r1 += 0.5f; r2 += 0.5f;
      if (r0 < 0.f) { r0 = 0.f; flags |= 1u; }
      if (r1 < 0.f) { r1 = 0.f; flags |= 2u; }
      if (r2 < 0.f) { r2 = 0.f; flags |= 4u; }
      rgb[0] = r0; rgb[1] = r1; rgb[2] = r2;
    }
  }
  // ---- the record and the per-Gaussian arrays ----------------------------------------------------------------------------
  const uint32_t rectbits = (uint32_t)pr.minx | ((uint32_t)pr.miny << 10) | ((uint32_t)(pr.maxx - pr.minx) << 20);
  bool rows_stored = false;
  if constexpr (H48) {
    if (coop) {                            // (uniform; the wave's own part of the image is free by now)
      rows_stored = true;
      float4* wl = reinterpret_cast<float4*>(reinterpret_cast<char*>(lds_sh) +
                                             (threadIdx.x >> 6) * (kK1ImageBytes / (kPreBlock / 64)));
      const unsigned long long vmask = __ballot(vis);
      const size_t row0 = (size_t)blockIdx.x * kPreBlock + (threadIdx.x & ~63u);
      const float4 r4[4] = {make_float4(rec.gx_hi, rec.gy_hi, rec.A2, rec.B2), make_float4(rec.C2, rec.opac, rgb[0], rgb[1]),
                            make_float4(rgb[2], rec.invz, rec.ext_x, __uint_as_float(rectbits)),
                            make_float4(rec.gx_lo, rec.gy_lo, rec.thr, rec.ext_y)};
      wave_store_rows<4>(reinterpret_cast<float4*>(g.records), row0, r4, vmask, wl);
      if constexpr (JAC) {
        wave_store_jac(g.shjac, row0, J, vmask, wl);
      }
    }
  }
  if (idx < a.P) {
    if (pr.visible && !rows_stored) {
      float4* recp = reinterpret_cast<float4*>(g.records) + (size_t)idx * kRecVec;
      recp[0] = make_float4(rec.gx_hi, rec.gy_hi, rec.A2, rec.B2);
      recp[1] = make_float4(rec.C2, rec.opac, rgb[0], rgb[1]);
      recp[2] = make_float4(rgb[2], rec.invz, rec.ext_x, __uint_as_float(rectbits));
      recp[3] = make_float4(rec.gx_lo, rec.gy_lo, rec.thr, rec.ext_y);
      if constexpr (H48 && JAC) {
        float* jd = g.shjac + (size_t)idx * kJacStride;
#pragma unroll
        for (int k = 0; k < 9; ++k) jd[k] = J[k];
      }
    }
    // zero rectangle (= zero instances) for culled Gaussians: the binning kernels derive counts from it
    reinterpret_cast<uint2*>(g.rects)[idx] =
        pr.visible ? make_uint2((uint32_t)pr.minx | ((uint32_t)pr.miny << 16), (uint32_t)pr.maxx | ((uint32_t)pr.maxy << 16))
                   : make_uint2(0u, 0u);
    radii[idx] = rad;
    g.depths[idx] = pr.tz;            // every Gaussian: the depth sort runs over all P keys
    g.tiles_touched[idx] = touched;
    g.flags[idx] = flags;
  }
}

template <bool JAC, bool LOD, bool DEFER>
__global__ __launch_bounds__(kPreBlock) void preprocess_fwd_kernel(hgs_raster_args a, GeomWs g,
                                                                   int32_t* __restrict__ radii, uint32_t* __restrict__ super, uint32_t heavy_thr) {
  preprocess_fwd_body<JAC, LOD, DEFER, false>(a, g, radii, super, heavy_thr);
}
// In-kernel LOD interpolation on half-precision rows (hgs_raster_args.lod_half_rows): forward only, no Jacobian.
__global__ __launch_bounds__(kPreBlock) void preprocess_fwd_lod_half_kernel(hgs_raster_args a, GeomWs g,
                                                                            int32_t* __restrict__ radii,
                                                                            uint32_t* __restrict__ super, uint32_t heavy_thr) {
  preprocess_fwd_body<false, true, false, false, true>(a, g, radii, super, heavy_thr);
}
// The M = 16 DMA route: 48 KB of LDS per workgroup (three workgroups per compute unit), the registers held to what four
// waves per SIMD leave (128).
template <bool JAC>
__global__ __launch_bounds__(kPreBlock, 4) void preprocess_fwd_h48_kernel(hgs_raster_args a, GeomWs g,
                                                                          int32_t* __restrict__ radii,
                                                                          uint32_t* __restrict__ super, uint32_t heavy_thr) {
  preprocess_fwd_body<JAC, false, false, true>(a, g, radii, super, heavy_thr);
}

// Exclusive scan of the per-workgroup sums (nblk = P/256): grid row 0 scans block_sums, rows 1..kBands the columns of
// block_band (common.h: chained_scan_inplace, one workgroup per 8192 entries); every array has n + 1 entries, the total
// lands in entry n.
// `total_mirror` (may be null): a second home for the grand total -- mapped host memory, so that the host learns the
// instance count without a copy command in the stream (under the profiler a 4-byte D2H copy + its barriers showed as
// ~10 us of stream time; free-running frames measure the same either way).
__global__ __launch_bounds__(1024) void scan_block_sums_kernel(uint32_t* __restrict__ sums0,
                                                               uint32_t* __restrict__ bands, int n,
                                                               unsigned long long* __restrict__ chain,
                                                               uint32_t* __restrict__ total_mirror, int c_off,
                                                               int chunks) {
  uint32_t* __restrict__ sums = blockIdx.y == 0 ? sums0 : bands + (size_t)(blockIdx.y - 1) * (n + 1);
  const uint32_t total = chained_scan_inplace(sums, n, chain + (size_t)blockIdx.y * chunks, c_off, chunks);
  if (threadIdx.x == 0 && blockIdx.y == 0 && (int)blockIdx.x + c_off == chunks - 1 && total_mirror) *total_mirror = total;
}

// ---------------------------------------------------------------------------
// K8: chain rule from the per-instance sums of the render backward to the op's
// inputs.  Instance sums (12 floats each, see render.hip):
//   0: sum X*dx   1: sum X*dy   2: sum X*dx^2   3: sum X*dx*dy   4: sum X*dy^2
//   5: sum G*dL/dalpha          6..8: sum w*dL/dC_k              9: sum w*dL/dD
// with X = dL/dpower, w = alpha*T.
// ---------------------------------------------------------------------------
// ---- in-kernel LOD scatter (hgs_raster_args.lod_scatter) ----------------------------------------------------------
// Row i of the op is w_i * attr[r_i] + (1 - w_i) * attr[p_i]; its gradient g_i goes to the node row (w_i g_i: the node
// rows of a cut are unique -> plain stores) and to the parent row ((1 - w_i) g_i, summed over the siblings).  Siblings
// are CONSECUTIVE rows when the parent indices are non-decreasing (expand_to_size emits them so): the first lane of a
// run sums it from LDS in row order and stores once.  Runs cut by a workgroup boundary (at most two per workgroup) and
// every run of an order that is not non-decreasing (flag word, launch_lod_monotone) use atomic adds instead; two
// partial sums added to a zero-filled row give the same bits in either order.
__device__ __forceinline__ int lod_parent_at(const hgs_raster_args& a, int i) {   // parent row of op row i, any i < P
  return i < a.lod_n ? a.lod_parent_indices[i] : a.lod_rows - (a.P - a.lod_n) + (i - a.lod_n);
}
struct LodRun {
  bool leader;    // first row of its run within this workgroup
  bool atomic;    // the run continues in a neighbouring workgroup, or the order is not monotone
  int end;        // one past the run's last row (workgroup-relative)
};
__device__ __forceinline__ LodRun lod_run(const hgs_raster_args& a, const int* lds_par, int t, int count, int block_first,
                                          bool nonmono) {
  LodRun r;
  const int p = lds_par[t];
  r.leader = (t == 0) || lds_par[t - 1] != p;
  r.end = t + 1;
  r.atomic = nonmono;
  if (r.leader) {
    while (r.end < count && lds_par[r.end] == p) ++r.end;
    if (t == 0 && block_first > 0 && lod_parent_at(a, block_first - 1) == p) r.atomic = true;
    if (r.end == count && block_first + count < a.P && lod_parent_at(a, block_first + count) == p) r.atomic = true;
  }
  return r;
}
__device__ __forceinline__ void lod_add(float* dst, float v, bool atomic) {
  if (atomic) atomicAdd(dst, v); else *dst = v;
}

// ---- long runs of instance records (K8a) ------------------------------------------------------------------------------
// K8a sums each Gaussian's run of instance records (one lane per Gaussian).  Benchmark scenes have 2.7 records per
// Gaussian; a TRAINED scene at 1080p has 28 on average and Gaussians that cover thousands of tiles (the 1080p run of
// profiles/r05_config2_config3_scripts_run1.log: K8 1.9 ms of a 3.6 ms frame, 11.7 ms on a hierarchy cut -- one lane
// walking 3 000 records while 63 wait).  When the frame's mean run is long (launch_preprocess_bwd) two kernels run in
// front of K8a.  Round 5 gave a wave 8 consecutive Gaussians whatever their runs; a hierarchy cut lists its big nodes side
// by side (4 096 rows holding a third of the frame's records), so a few hundred waves on a few compute units did all the
// work: 0.47 ms.  Now the RECORDS are dealt out:
//   k8_worklist_kernel   every run of more than kK8LongRun records is cut into segments of kK8Seg records and one
//                        (Gaussian, segment) pair per segment goes onto a worklist (a workgroup reserves its pairs' places
//                        with one atomic add: the ORDER of the list is not deterministic, what a pair stands for is);
//   k8_presum_work_kernel a fixed grid of waves takes the pairs in turn: lane i sums records i, i + 64, ... of the segment
//                        (consecutive 40-byte records, coalesced; double-precision partial sums), the 64 partials of each of
//                        the ten components are folded in a fixed order and the ten sums are stored, as doubles, OVER THE
//                        SEGMENT'S FIRST TWO RECORDS -- the segment is consumed, nobody else reads it.
// K8a then adds a long run's segment sums in segment order.  Every sum is a fixed tree: bit-reproducible.
__device__ __forceinline__ uint32_t k8_nseg(uint32_t n) {        // n > kK8LongRun; the last segment holds >= 2 records
  uint32_t c = (n + kK8Seg - 1u) / kK8Seg;
  if (c > 1u && n - (c - 1u) * kK8Seg < 2u) --c;
  return c;
}
// (at most kWorklistGrid workgroups, each over a contiguous share of the 256-Gaussian blocks: one workgroup per block had
// 1 465 workgroups queue up on the one counter -- 20 us of a 2 us job on the trained-scale frame)
constexpr int kWorklistGrid = 256;
__global__ __launch_bounds__(kPreBlock) void k8_worklist_kernel(int P, const uint32_t* __restrict__ tiles_touched,
                                                                uint2* __restrict__ work, uint32_t* __restrict__ counter) {
  __shared__ uint32_t wave_tot[kPreBlock / 64];
  __shared__ uint32_t base_s;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int nblk = (P + kPreBlock - 1) / kPreBlock;
  const int per = (nblk + (int)gridDim.x - 1) / (int)gridDim.x;
  const int b0 = (int)blockIdx.x * per, b1 = min(b0 + per, nblk);
  // pass 1: this workgroup's pairs, one reservation
  uint32_t mine = 0;
  for (int b = b0; b < b1; ++b) {
    const int idx = b * kPreBlock + (int)threadIdx.x;
    const uint32_t n = idx < P ? tiles_touched[idx] : 0u;
    mine += n > kK8LongRun ? k8_nseg(n) : 0u;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) mine += __shfl_xor(mine, off, 64);
  if (lane == 0) wave_tot[wave] = mine;
  __syncthreads();
  uint32_t total = 0;
#pragma unroll
  for (int w = 0; w < kPreBlock / 64; ++w) total += wave_tot[w];
  if (total == 0u) return;                                               // (workgroup-uniform)
  if (threadIdx.x == 0) base_s = atomicAdd(counter, total);
  __syncthreads();
  uint32_t run = base_s;
  // pass 2: block by block, the pairs in Gaussian order
  for (int b = b0; b < b1; ++b) {
    const int idx = b * kPreBlock + (int)threadIdx.x;
    const uint32_t n = idx < P ? tiles_touched[idx] : 0u;
    const uint32_t c = n > kK8LongRun ? k8_nseg(n) : 0u;
    uint32_t inc = c;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const uint32_t t = __shfl_up(inc, off, 64);
      if (lane >= off) inc += t;
    }
    __syncthreads();                                                     // (the previous block's totals have been read)
    if (lane == 63) wave_tot[wave] = inc;
    __syncthreads();
    uint32_t before = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < kPreBlock / 64; ++w) {
      const uint32_t t = wave_tot[w];
      before += w < wave ? t : 0u;
      tot += t;
    }
    uint2* dst = work + run + before + inc - c;
    for (uint32_t j = 0; j < c; ++j) dst[j] = make_uint2((uint32_t)idx, j);
    run += tot;
  }
}

constexpr int kPresumGrid = 2048;        // workgroups of four waves: every wave takes pairs w, w + 8192, ...
__global__ __launch_bounds__(kPreBlock) void k8_presum_work_kernel(const uint2* __restrict__ work,
                                                                   const uint32_t* __restrict__ counter,
                                                                   const uint32_t* __restrict__ tiles_touched,
                                                                   const uint32_t* __restrict__ offsets,
                                                                   float* __restrict__ inst) {
  __shared__ double red_all[kPreBlock / 64][640 + 40];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint32_t n_work = *counter;
  double* red = red_all[wave];
  for (uint32_t item = blockIdx.x * (kPreBlock / 64) + wave; item < n_work; item += gridDim.x * (kPreBlock / 64)) {   // (wave-uniform)
    const uint2 w = work[item];
    const uint32_t n = tiles_touched[w.x];
    const uint32_t r0 = w.y * kK8Seg;
    const uint32_t r1 = (w.y + 1u == k8_nseg(n)) ? n : r0 + kK8Seg;
    const size_t rbase = (size_t)offsets[w.x] + r0;
    const float2* ip = reinterpret_cast<const float2*>(inst) + rbase * 5;
    double t[10];
#pragma unroll
    for (int i = 0; i < 10; ++i) t[i] = 0.0;
#pragma unroll 4
    for (uint32_t k = (uint32_t)lane; k < r1 - r0; k += 64u) {
      const float2 v0 = ip[k * 5 + 0], v1 = ip[k * 5 + 1], v2 = ip[k * 5 + 2], v3 = ip[k * 5 + 3], v4 = ip[k * 5 + 4];
      t[0] += v0.x; t[1] += v0.y; t[2] += v1.x; t[3] += v1.y;
      t[4] += v2.x; t[5] += v2.y; t[6] += v3.x; t[7] += v3.y;
      t[8] += v4.x; t[9] += v4.y;
    }
#pragma unroll
    for (int i = 0; i < 10; ++i) red[i * 64 + lane] = t[i];
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    // fold in two fixed stages: lane 4 c + q sums partials 16 q .. 16 q + 15 of component c, lane c the four quarter sums
    if (lane < 40) {
      double acc = 0.0;
      const double* src = red + (lane >> 2) * 64 + (lane & 3) * 16;
#pragma unroll
      for (int j = 0; j < 16; ++j) acc += src[j];
      red[640 + lane] = acc;
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    if (lane < 10) {
      const double* q = red + 640 + lane * 4;
      reinterpret_cast<double*>(inst + rbase * kInstStride)[lane] = ((q[0] + q[1]) + q[2]) + q[3];   // (40-byte records: 8-byte aligned)
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();                                     // (the next pair overwrites the scratch)
  }
}

// ---- K8a, phase 1: sum the instance partials (one contiguous run per Gaussian, emission order) -------------------------
// The runs of a wave's 64 Gaussians lie BACK TO BACK in the scratch (emission order = Gaussian order), ~170 records of
// 40 bytes: the wave streams that range through LDS with all lanes loading (coalesced; by LDS DMA the whole pass in
// flight, through registers -- HGS_K8_STAGE=0 -- four loads per lane at a time) and every lane then sums its own run
// out of LDS -- in the same order as before, so the sums keep their bits.
// Round 3 had each lane walk its run in global memory: 2.7 dependent round trips per Gaussian on average, the longest
// run of the wave for everybody, at 3 waves per SIMD (160 registers) to hide them.
// Two routes per wave:
//   * (always in frames of short runs, launch_preprocess_bwd) the wave streams its contiguous range of records through
//     LDS, each lane sums its own run from there;
//   * `presummed` and a run of more than kK8LongRun records in the wave: k8_presum_work_kernel left every segment's ten
//     sums at the segment's start; the other lanes walk their short runs in global memory (the wave's range is mostly
//     the long run).
// `st` is the calling wave's stage (kK8StageRec records).  Every lane of the wave calls (out-of-range lanes with n = 0).
//
// Staged (kK8ModeStage, the default): the pass goes into the stage by LDS DMA, every 16-byte piece of it in flight at
// once and no register in between -- one round trip per pass where the register route takes one per four loads of a
// lane.  A record is 40 bytes, so a pass starts 8-byte aligned: the DMA starts at the 16-byte boundary at or below it
// (never in front of `inst`, whose base is 16-byte aligned -- the launcher checks) and the sums read the stage `shift`
// bytes further in.  A pass is kK8DmaRec records, so that the shift and the last, partial piece fit the stage; the last
// piece of the last run may reach 8 bytes past the records, inside the extent the workspace's size query rounds up to.
// A pass boundary changes no bit: each lane still adds its own run in run order.  `off` is offsets[idx], loaded at
// kernel entry next to tiles_touched (a culled row's word is uninitialised and never used).
constexpr uint32_t kK8StageRec = 256;                                 // records per wave and pass: 10 KB
constexpr uint32_t kK8StageBytes = kK8StageRec * kInstStride * 4;
constexpr uint32_t kK8DmaRec = 254;                                   // 8 + 254 x 40 = 10 168 bytes: 636 pieces of 640
static_assert((8 + kK8DmaRec * kInstStride * 4 + 15) / 16 <= kK8StageBytes / 16,
              "a DMA pass, shifted, fits the stage in whole 16-byte pieces");
constexpr int kK8ModePresum = 1, kK8ModeStage = 2, kK8ModeStageIn = 4;   // `mode` of the K8 kernels (launch_preprocess_bwd)
// what the waves of a workgroup keep behind the four stages: the 64 rows of mean, scales, rotation, opacity and flags
constexpr uint32_t kK8InWave = 64 * (12 + 12 + 16 + 4 + 4);           // 3 072 bytes per wave
constexpr uint32_t kK8InMean = 0, kK8InScale = 768, kK8InRot = 1536, kK8InOp = 2560, kK8InFlags = 2816;
constexpr uint32_t kK8LdsBytes = (kPreBlock / 64) * (kK8StageBytes + kK8InWave);   // 53 248: K8b's output stage at M = 16

// number of 16-byte pieces and the shift of a pass of `cnt` records that starts at record `first` of the scratch
__host__ __device__ __forceinline__ uint32_t k8_pass_shift(size_t first) { return (uint32_t)((first * (kInstStride * 4)) & 15u); }
__host__ __device__ __forceinline__ uint32_t k8_pass_pieces(size_t first, uint32_t cnt) {
  return (k8_pass_shift(first) + cnt * (kInstStride * 4) + 15u) >> 4;
}

// The wave's 64 rows of every per-Gaussian input into its block `in` of LDS, at kernel entry; k8_chain reads them there.
// By LDS DMA (five wave-instructions; a wave's slice of a tensor is contiguous and 16-byte aligned when the tensor is),
// waited for together with the first pass of the records: full waves of aligned tensors (kK8ModeStageIn), so that no
// piece reaches past row P.  Every other wave -- the last one of a P off the wave grid, a torch view with a storage
// offset -- loads its rows lane by lane, as the chain would, and every lane writes the row it will read back itself.
// With a precomputed covariance the scales and rotations are absent and their slots stay unread.
__device__ __forceinline__ void k8_stage_inputs(const hgs_raster_args& a, const GeomWs& g, int idx, int mode, unsigned char* in) {
  const int lane = threadIdx.x & 63, wave_first = idx & ~63;
  const bool sr = !a.cov3D_precomp;
  if ((mode & kK8ModeStageIn) && wave_first + 64 <= a.P) {             // (wave-uniform)
    const char* m = reinterpret_cast<const char*>(a.means3D + (size_t)wave_first * 3);
    const char* o = reinterpret_cast<const char*>(a.opacities + wave_first);
    const char* f = reinterpret_cast<const char*>(g.flags + wave_first);
    if (lane < 48) __builtin_amdgcn_global_load_lds((gptr_t)(m + lane * 16), (lptr_t)(in + kK8InMean), 16, 0, 0);
    if (sr) {
      const char* sc = reinterpret_cast<const char*>(a.scales + (size_t)wave_first * 3);
      const char* r = reinterpret_cast<const char*>(a.rotations + (size_t)wave_first * 4);
      if (lane < 48) __builtin_amdgcn_global_load_lds((gptr_t)(sc + lane * 16), (lptr_t)(in + kK8InScale), 16, 0, 0);
      __builtin_amdgcn_global_load_lds((gptr_t)(r + lane * 16), (lptr_t)(in + kK8InRot), 16, 0, 0);
    }
    if (lane < 16) {
      __builtin_amdgcn_global_load_lds((gptr_t)(o + lane * 16), (lptr_t)(in + kK8InOp), 16, 0, 0);
      __builtin_amdgcn_global_load_lds((gptr_t)(f + lane * 16), (lptr_t)(in + kK8InFlags), 16, 0, 0);
    }
  } else if (idx < a.P) {
    float* m = reinterpret_cast<float*>(in + kK8InMean) + lane * 3;
    m[0] = a.means3D[idx * 3 + 0]; m[1] = a.means3D[idx * 3 + 1]; m[2] = a.means3D[idx * 3 + 2];
    if (sr) {
      float* sc = reinterpret_cast<float*>(in + kK8InScale) + lane * 3;
      sc[0] = a.scales[idx * 3 + 0]; sc[1] = a.scales[idx * 3 + 1]; sc[2] = a.scales[idx * 3 + 2];
      reinterpret_cast<float4*>(in + kK8InRot)[lane] = reinterpret_cast<const float4*>(a.rotations)[idx];
    }
    reinterpret_cast<float*>(in + kK8InOp)[lane] = a.opacities[idx];
    reinterpret_cast<uint32_t*>(in + kK8InFlags)[lane] = g.flags[idx];
  }
}

template <bool STG>   // STG: the passes by LDS DMA
__device__ __forceinline__ void k8_sum_runs(const float* __restrict__ inst, uint32_t off, uint32_t n,
                                            int mode, float2* st, double (&s)[10]) {
  const int lane = threadIdx.x & 63;
  const int presummed = mode & kK8ModePresum;
  constexpr bool dma = STG;
  const unsigned long long long_mask = presummed ? __ballot(n > kK8LongRun) : 0ull;
  if (long_mask == 0ull) {
    uint32_t incl = n;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const uint32_t t = __shfl_up(incl, off, 64);
      if (lane >= off) incl += t;
    }
    const uint32_t my0 = incl - n, my1 = incl;                         // this lane's run, in records of the wave's range
    const uint32_t total = __shfl(incl, 63, 64);
    if (total) {                                                       // (wave-uniform)
      const unsigned long long nz = __ballot(n != 0u);
      const int first = __ffsll((long long)nz) - 1;
      const size_t base = (size_t)__shfl(n ? off : 0u, first, 64);     // (no instances before the first non-empty lane)
      const uint32_t pass = dma ? kK8DmaRec : kK8StageRec;
      for (uint32_t c0 = 0; c0 < total; c0 += pass) {
        const uint32_t cnt = min(pass, total - c0);
        uint32_t shift2 = 0;                                           // where record c0 lies in the stage, in float2
        if (dma) {
          const uint32_t shift = k8_pass_shift(base + c0), pieces = k8_pass_pieces(base + c0, cnt);
          const char* src = reinterpret_cast<const char*>(inst) + ((base + c0) * (kInstStride * 4) - shift);
#pragma unroll
          for (uint32_t j = 0; j < kK8StageBytes / 1024; ++j) {        // (a wave-instruction fills 1 KB)
            const uint32_t piece = j * 64u + (uint32_t)lane;
            if (piece < pieces)
              __builtin_amdgcn_global_load_lds((gptr_t)(src + (size_t)piece * 16), (lptr_t)(reinterpret_cast<char*>(st) + j * 1024), 16, 0, 0);
          }
          asm volatile("s_waitcnt vmcnt(0)" ::: "memory");             // (retires the kernel-entry input DMA as well)
          shift2 = shift >> 3;
        } else {
          const uint32_t cn = cnt * 5u;                                // float2 words of this pass
          const float2* src = reinterpret_cast<const float2*>(inst) + (base + c0) * 5;
          for (uint32_t t0 = 0; t0 < cn; t0 += 64u * 4u) {             // four loads in flight per lane
            float2 v[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              const uint32_t t = t0 + (uint32_t)j * 64u + (uint32_t)lane;
              v[j] = src[min(t, cn - 1u)];
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              const uint32_t t = t0 + (uint32_t)j * 64u + (uint32_t)lane;
              if (t < cn) st[t] = v[j];
            }
          }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        const uint32_t k0 = max(my0, c0), k1 = min(my1, c0 + pass);
        for (uint32_t k = k0; k < k1; ++k) {
          const float2* r = st + shift2 + (k - c0) * 5u;
          const float2 v0 = r[0], v1 = r[1], v2 = r[2], v3 = r[3], v4 = r[4];
          s[0] += v0.x; s[1] += v0.y; s[2] += v1.x; s[3] += v1.y;
          s[4] += v2.x; s[5] += v2.y; s[6] += v3.x; s[7] += v3.y;
          s[8] += v4.x; s[9] += v4.y;
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();                               // (the next pass overwrites the stage)
      }
    }
  } else if (n != 0u) {
    if (n > kK8LongRun) {
      const uint32_t nseg = k8_nseg(n);
      for (uint32_t j = 0; j < nseg; ++j) {                              // segment sums, in segment order
        const double* ps = reinterpret_cast<const double*>(inst + ((size_t)off + (size_t)j * kK8Seg) * kInstStride);
#pragma unroll
        for (int i = 0; i < 10; ++i) s[i] += ps[i];
      }
    } else {
      const float2* ip = reinterpret_cast<const float2*>(inst) + (size_t)off * 5;
#pragma unroll 2
      for (uint32_t k = 0; k < n; ++k) {
        const float2 v0 = ip[k * 5 + 0], v1 = ip[k * 5 + 1], v2 = ip[k * 5 + 2], v3 = ip[k * 5 + 3], v4 = ip[k * 5 + 4];
        s[0] += v0.x; s[1] += v0.y; s[2] += v1.x; s[3] += v1.y;
        s[4] += v2.x; s[5] += v2.y; s[6] += v3.x; s[7] += v3.y;
        s[8] += v4.x; s[9] += v4.y;
      }
    }
  }
}

// ---- K8a, phase 2: recompute the forward projection and walk the chain rule back (one visible Gaussian per lane) --------
// s: the ten sums of the Gaussian's run.  p: its mean, as loaded.  gr: dL/drgb, clamp-masked (K1's flags) for SH colours,
// the plain sums for precomputed colours.  The gradients arrive zeroed (cov3D_precomp leaves d_scale and d_rot alone).
// (separate arrays, not a struct: with a struct K8a took 178 registers instead of 158)
// STG: the raw inputs come from `in`, the wave's staged block (k8_stage_inputs, landed); else every value is loaded here,
// lane by lane.  The staged route applies the activations with the text of load_scale_rot / load_opacity
// (gaussian_math.h) to the same raw values; tests/test_k8_staged_gpu.py holds the two routes to the same bits.
template <bool LOD, bool STG>
__device__ __forceinline__ void k8_chain(const hgs_raster_args& a, const GeomWs& g, int idx, const double (&s)[10],
                                         float (&p)[3], float (&d_mean)[3], float (&d_m2)[3], float& d_op,
                                         float (&d_scale)[3], float (&d_rot)[4], float (&d_c3)[6], float (&gr)[3],
                                         const unsigned char* in, const CamLds* cam_entry) {
  // (STG: the camera was loaded at kernel entry, in front of the DMA -- behind a write to memory the compiler would no
  // longer take its 35 uniform words by scalar loads, and they would sit in 35 vector registers through the chain)
  CamLds cam_here;
  if constexpr (!STG) load_camera(a, cam_here);
  const CamLds& cam = STG ? *cam_entry : cam_here;
  gr[0] = (float)s[6]; gr[1] = (float)s[7]; gr[2] = (float)s[8];
  const int lane = threadIdx.x & 63;
  static_assert(!(LOD && STG), "the LOD route gathers rows by index");
  constexpr bool staged = STG;
  // ---- recompute the forward projection (double chain; clamp decisions from K1's flags) ----
  uint32_t flags;
  if (staged) {
    flags = reinterpret_cast<const uint32_t*>(in + kK8InFlags)[lane];
    const float* m = reinterpret_cast<const float*>(in + kK8InMean) + lane * 3;
    p[0] = m[0]; p[1] = m[1]; p[2] = m[2];
  } else {
    flags = g.flags[idx];
    load_mean<LOD>(a, lod_row_gather<LOD>(a, idx), p);
  }
  float q[4] = {1.f, 0.f, 0.f, 0.f};
  float sc[3] = {1.f, 1.f, 1.f};
  double qnorm = 1.0;
  ProjD pd;
  if (a.cov3D_precomp) {
#pragma unroll
    for (int i = 0; i < 6; ++i) pd.c3[i] = (double)a.cov3D_precomp[(size_t)idx * 6 + i];
  } else {
    if (staged) {
      const float* sr = reinterpret_cast<const float*>(in + kK8InScale) + lane * 3;
      sc[0] = sr[0]; sc[1] = sr[1]; sc[2] = sr[2];
      if (a.activations & HGS_ACT_SCALE_EXP) {
#pragma unroll
        for (int i = 0; i < 3; ++i) sc[i] = (float)exp((double)sc[i]);
      }
      const float4 qv = reinterpret_cast<const float4*>(in + kK8InRot)[lane];
      q[0] = qv.x; q[1] = qv.y; q[2] = qv.z; q[3] = qv.w;
      if (a.activations & HGS_ACT_ROT_NORMALIZE) {
        const double w = q[0], x = q[1], y = q[2], z = q[3];
        qnorm = fmax(sqrt(((w * w + x * x) + y * y) + z * z), 1e-12);
        q[0] = (float)(w / qnorm); q[1] = (float)(x / qnorm); q[2] = (float)(y / qnorm); q[3] = (float)(z / qnorm);
      }
    } else {
      load_scale_rot<LOD>(a, idx, sc, q, &qnorm);
    }
    cov3d_from_scale_rot_d(sc, a.scale_modifier, q, pd);
  }
  project_gaussian_d(p, cam.vm, cam.pm, a.width, a.height, a.tanfovx, a.tanfovy, (flags & 8u) != 0,
                     (flags & 16u) != 0, pd);

  const double A = pd.conA, B = pd.conB, C = pd.conC;
  const double gA = -0.5 * s[2], gB = -s[3], gC = -0.5 * s[4];
  const double ggx = -(A * s[0] + B * s[1]);
  const double ggy = -(C * s[1] + B * s[0]);
  const double dm2x = ggx * 0.5 * (double)a.width, dm2y = ggy * 0.5 * (double)a.height;
  d_m2[0] = (float)dm2x;
  d_m2[1] = (float)dm2y;
  double dmean[3] = {0.0, 0.0, 0.0};

  // screen position -> clip space -> world
  const double dhx = dm2x * pd.pw, dhy = dm2y * pd.pw;
  const double dhw = -(dm2x * pd.hx + dm2y * pd.hy) * pd.pw * pd.pw;
#pragma unroll
  for (int j = 0; j < 3; ++j)
    dmean[j] += (double)cam.pm[j * 4 + 0] * dhx + (double)cam.pm[j * 4 + 1] * dhy + (double)cam.pm[j * 4 + 3] * dhw;

  // conic -> 2D covariance
  const double a2 = pd.a, b2 = pd.b, c2 = pd.c;
  const double di2 = pd.di * pd.di;
  const double ga = (-c2 * c2 * gA + b2 * c2 * gB - b2 * b2 * gC) * di2;
  const double gb = (2.0 * b2 * c2 * gA - (a2 * c2 + b2 * b2) * gB + 2.0 * a2 * b2 * gC) * di2;
  const double gc = (-b2 * b2 * gA + a2 * b2 * gB - a2 * a2 * gC) * di2;
  const double hb = 0.5 * gb;
  // dL/dSigma (full symmetric matrix) = T^T G2 T; the lower triangle is the upper one mirrored, so that Gs is
  // symmetric to the bit: evaluated on its own it rounds differently, and that antisymmetric rounding noise reaches
  // the rotation gradient even where the exact one is zero (an isotropic Gaussian, whose rotation cannot matter)
  double Gs[3][3];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = i; j < 3; ++j)
      Gs[i][j] = Gs[j][i] = pd.T0[i] * (ga * pd.T0[j] + hb * pd.T1[j]) + pd.T1[i] * (hb * pd.T0[j] + gc * pd.T1[j]);
  d_c3[0] = (float)Gs[0][0];
  d_c3[1] = (float)(2.0 * Gs[0][1]);
  d_c3[2] = (float)(2.0 * Gs[0][2]);
  d_c3[3] = (float)Gs[1][1];
  d_c3[4] = (float)(2.0 * Gs[1][2]);
  d_c3[5] = (float)Gs[2][2];
  // dL/dT = 2 G2 T Sigma = 2 G2 U
  double dT0[3], dT1[3];
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    dT0[j] = 2.0 * ga * pd.U0[j] + gb * pd.U1[j];
    dT1[j] = gb * pd.U0[j] + 2.0 * gc * pd.U1[j];
  }
  double gJ00 = 0.0, gJ02 = 0.0, gJ11 = 0.0, gJ12 = 0.0;
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    gJ00 += dT0[j] * (double)cam.vm[j * 4 + 0];
    gJ02 += dT0[j] * (double)cam.vm[j * 4 + 2];
    gJ11 += dT1[j] * (double)cam.vm[j * 4 + 1];
    gJ12 += dT1[j] * (double)cam.vm[j * 4 + 2];
  }
  const double itz = pd.itz, itz2 = itz * itz, itz3 = itz2 * itz;
  const double g_txc = -pd.fx * itz2 * gJ02;
  const double g_tyc = -pd.fy * itz2 * gJ12;
  double g_tz = -pd.fx * itz2 * gJ00 + 2.0 * pd.fx * pd.txc * itz3 * gJ02 - pd.fy * itz2 * gJ11 +
                2.0 * pd.fy * pd.tyc * itz3 * gJ12;
  double g_tx = 0.0, g_ty = 0.0;
  if (flags & 8u) g_tz += g_txc * (pd.txc * itz); else g_tx = g_txc;
  if (flags & 16u) g_tz += g_tyc * (pd.tyc * itz); else g_ty = g_tyc;
  // inverse depth
  g_tz += -s[9] * itz2;
#pragma unroll
  for (int j = 0; j < 3; ++j)
    dmean[j] += (double)cam.vm[j * 4 + 0] * g_tx + (double)cam.vm[j * 4 + 1] * g_ty + (double)cam.vm[j * 4 + 2] * g_tz;
  d_mean[0] = (float)dmean[0]; d_mean[1] = (float)dmean[1]; d_mean[2] = (float)dmean[2];

  // Sigma -> scale / rotation
  if (!a.cov3D_precomp) {
    const double* R = pd.R;
    const double* sv = pd.s;
    double dM[3][3];   // dL/dM, M_ik = R_ik s_k ; dL/dM = 2 Gs M
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        double acc = 0.0;
#pragma unroll
        for (int j = 0; j < 3; ++j) acc += Gs[i][j] * (R[j * 3 + k] * sv[k]);
        dM[i][k] = 2.0 * acc;
      }
    double gR[3][3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      double acc = 0.0;
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        acc += R[i * 3 + k] * dM[i][k];
        gR[i][k] = dM[i][k] * sv[k];
      }
      double dsk = (double)a.scale_modifier * acc;
      if (a.activations & HGS_ACT_SCALE_EXP) dsk *= (double)sc[k];          // d exp(raw) / d raw = exp(raw)
      d_scale[k] = (float)dsk;
    }
    const double r = q[0], x = q[1], y = q[2], z = q[3];
    double dq[4];
    dq[0] = 2.0 * (-z * gR[0][1] + y * gR[0][2] + z * gR[1][0] - x * gR[1][2] - y * gR[2][0] + x * gR[2][1]);
    dq[1] = 2.0 * (y * gR[0][1] + z * gR[0][2] + y * gR[1][0] - 2.0 * x * gR[1][1] - r * gR[1][2] +
                   z * gR[2][0] + r * gR[2][1] - 2.0 * x * gR[2][2]);
    dq[2] = 2.0 * (-2.0 * y * gR[0][0] + x * gR[0][1] + r * gR[0][2] + x * gR[1][0] + z * gR[1][2] -
                   r * gR[2][0] + z * gR[2][1] - 2.0 * y * gR[2][2]);
    dq[3] = 2.0 * (-2.0 * z * gR[0][0] - r * gR[0][1] + x * gR[0][2] + r * gR[1][0] - 2.0 * z * gR[1][1] +
                   y * gR[1][2] + x * gR[2][0] + y * gR[2][1]);
    if (a.activations & HGS_ACT_ROT_NORMALIZE) {     // through q = raw / |raw|: (I - q q^T) / |raw|
      const double dot = r * dq[0] + x * dq[1] + y * dq[2] + z * dq[3];
      const double inv = 1.0 / qnorm;
      dq[0] = (dq[0] - r * dot) * inv; dq[1] = (dq[1] - x * dot) * inv;
      dq[2] = (dq[2] - y * dot) * inv; dq[3] = (dq[3] - z * dot) * inv;
    }
    d_rot[0] = (float)dq[0]; d_rot[1] = (float)dq[1]; d_rot[2] = (float)dq[2]; d_rot[3] = (float)dq[3];
  }

  // opacity (through the LOD remap)
  {
    float dod = 1.0f;
    double dact = 1.0;
    float o_act;
    if (staged) {
      const float raw = reinterpret_cast<const float*>(in + kK8InOp)[lane];
      o_act = raw;
      if (a.activations & HGS_ACT_OPACITY_SIGMOID) {
        const double o = 1.0 / (1.0 + exp(-(double)raw));
        dact = o * (1.0 - o);
        o_act = (float)o;
      } else if (a.activations & HGS_ACT_OPACITY_ABS) {
        dact = raw > 0.f ? 1.0 : (raw < 0.f ? -1.0 : 0.0);
        o_act = fabsf(raw);
      }
    } else {
      o_act = load_opacity<LOD>(a, idx, &dact);
    }
    float o_rec = o_act;      // the opacity K1 put into the record (same functions, same float)
    if (a.interpolation_weights && a.num_node_kids && !a.lod_per_pixel)
      o_rec = lod_opacity(o_act, a.interpolation_weights[idx], a.num_node_kids[idx], &dod);
    // the instance records carry sum X = sum (o G) dL/dalpha; dL/do = sum G dL/dalpha = (sum X) / o.  o <= 0: never
    // blended, sum X = 0
    // (exact division, once per Gaussian: rcp_d seeds from v_rcp_f32, which overflows for a denormal opacity -- the
    // Newton step would then turn 0 x inf into a NaN that poisons the optimizer state)
    const float sums5 = o_rec > 0.0f ? (float)(s[5] / (double)o_rec) : 0.0f;
    d_op = a.activations ? (float)((double)sums5 * (double)dod * dact) : sums5 * dod;
  }

  if (!a.colors_precomp) {
    if (flags & 1u) gr[0] = 0.f;
    if (flags & 2u) gr[1] = 0.f;
    if (flags & 4u) gr[2] = 0.f;
  }
}

// One row of every per-Gaussian gradient but dL/dmeans3D (which K8b adds the view-direction term to).
// accumulate_grads: add to what the buffers hold (gradient accumulation over several views of one optimizer
// step); dL/dmeans2D (a per-view statistic) and dL/dcolors_precomp (the gradient of a view's colours) are always
// overwritten
template <bool ACC>
__device__ __forceinline__ void k8_store_row(const hgs_raster_grads& out, int idx, const float (&d_m2)[3], float d_op,
                                             const float (&d_scale)[3], const float (&d_rot)[4], const float (&d_c3)[6],
                                             const float (&d_col)[3]) {
  constexpr bool acc = ACC;
#pragma unroll
  for (int j = 0; j < 3; ++j) out.dL_dmeans2D[idx * 3 + j] = d_m2[j];
  out.dL_dopacity[idx] = d_op + (acc ? out.dL_dopacity[idx] : 0.f);
  if (out.dL_dcolors) {
#pragma unroll
    for (int j = 0; j < 3; ++j) out.dL_dcolors[idx * 3 + j] = d_col[j];   // per view, like dL/dmeans2D: never accumulated
  }
  if (out.dL_dscales) {
#pragma unroll
    for (int j = 0; j < 3; ++j) out.dL_dscales[idx * 3 + j] = d_scale[j] + (acc ? out.dL_dscales[idx * 3 + j] : 0.f);
  }
  if (out.dL_drotations) {
    float4* dst = reinterpret_cast<float4*>(out.dL_drotations) + idx;
    float4 v = make_float4(d_rot[0], d_rot[1], d_rot[2], d_rot[3]);
    if (acc) { const float4 o = *dst; v.x += o.x; v.y += o.y; v.z += o.z; v.w += o.w; }
    *dst = v;
  }
  if (out.dL_dcov3D) {
#pragma unroll
    for (int j = 0; j < 6; ++j) out.dL_dcov3D[(size_t)idx * 6 + j] = d_c3[j] + (acc ? out.dL_dcov3D[(size_t)idx * 6 + j] : 0.f);
  }
}

// ACC: add into the gradient buffers (accumulation over the views of one optimizer step).  STG: records and inputs staged
// by LDS DMA (k8_sum_runs, k8_stage_inputs), the inputs in 12 KB of LDS next to the four stages -- 53 248 bytes together,
// still three workgroups per compute unit; never with LOD, whose rows are gathered by index.
// Two kernels over one body (k8a_body.h): preprocess_bwd_kernel<ACC, LOD> (registers) and preprocess_bwd_staged_kernel<ACC>.
template <bool ACC, bool LOD>
__global__ __launch_bounds__(kPreBlock) void preprocess_bwd_kernel(hgs_raster_args a, GeomWs g,
                                                                   const float* __restrict__ inst,
                                                                   float* __restrict__ drgb,
                                                                   float* __restrict__ dmean_rows,
                                                                   const uint32_t* __restrict__ lod_flag,
                                                                   hgs_raster_grads out, int mode) {
  constexpr bool STG = false;
#include "k8a_body.h"
}
template <bool ACC>
__global__ __launch_bounds__(kPreBlock) void preprocess_bwd_staged_kernel(hgs_raster_args a, GeomWs g,
                                                                          const float* __restrict__ inst,
                                                                          float* __restrict__ drgb,
                                                                          float* __restrict__ dmean_rows,
                                                                          const uint32_t* __restrict__ lod_flag,
                                                                          hgs_raster_grads out, int mode) {
  constexpr bool LOD = false, STG = true;
#include "k8a_body.h"
}


// K8b: SH part of the backward.  Pure streaming kernel (192 B of coefficients in, 192 B of gradients out
// per Gaussian at M = 16), split from the double-precision geometry chain of K8a so that it runs at high
// occupancy.  Adds the view-direction term to dL/dmeans3D written by K8a.
template <bool ACC, bool JAC, bool LOD>   // JAC: d(rgb)/d(direction) was stored by K1 (prepare_backward): the coefficients are not read
__global__ __launch_bounds__(kPreBlock) void sh_bwd_kernel(hgs_raster_args a, GeomWs g,
                                                           const float* __restrict__ drgb,
                                                           const float* __restrict__ dmean_rows,
                                                           const uint32_t* __restrict__ lod_flag, hgs_raster_grads out) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  float* lds = reinterpret_cast<float*>(smem_raw);
  const int n = a.M * 3;
  const bool split = a.shs_rest != nullptr;       // features_dc / features_rest as two tensors
  const bool coop = (n & 3) == 0;                 // 16-byte granules (M = 16, 4, ...); else per-lane access
  const int block_first = blockIdx.x * kPreBlock;
  const int idx = block_first + threadIdx.x;
  const bool valid = idx < a.P;
  const bool active = valid && g.tiles_touched[idx] != 0;
  if (!JAC && coop) {
    if (split) {
      coop_load_seg(a.shs, block_first, a.P, 3, 0, sh_row_stride(n), lds);
      coop_load_seg(a.shs_rest, block_first, a.P, n - 3, 3, sh_row_stride(n), lds);
    } else {
      coop_load_sh(a.shs, block_first, a.P, n, lds);
    }
    __syncthreads();
  }
  float dsh[48];
#pragma unroll
  for (int i = 0; i < 48; ++i) dsh[i] = 0.f;
  float sh[JAC ? 1 : 48];
  if constexpr (!JAC) {
    if (active) {
      if (coop) lds_row_read(lds, n, sh);
      else if (split) load_sh_split(a.shs, a.shs_rest, idx, a.M, sh);
      else load_sh(a.shs, idx, a.M, sh);
    }
  }
  if (!JAC && coop) __syncthreads();              // every row has been read: the buffer becomes the output stage
  float vdir[3] = {0.f, 0.f, 0.f};                // view-direction term of dL/dmean
  if (active) {
    const float gr[3] = {drgb[idx * 3 + 0], drgb[idx * 3 + 1], drgb[idx * 3 + 2]};
    float pm[3];
    load_mean<LOD>(a, lod_row_gather<LOD>(a, idx), pm);
    float ux, uy, uz;
    const float inv = unit_dir(pm, a.campos, ux, uy, uz);
    float b[16];
    sh_basis(a.sh_degree, ux, uy, uz, b);
    const int nb = (a.sh_degree + 1) * (a.sh_degree + 1);
    float gdx = 0.f, gdy = 0.f, gdz = 0.f;
    if constexpr (JAC) {
      const float* jp = g.shjac + (size_t)idx * kJacStride;
      float J[9];
#pragma unroll
      for (int k = 0; k < 9; ++k) J[k] = jp[k];
      gdx = gr[0] * J[0] + gr[1] * J[1] + gr[2] * J[2];
      gdy = gr[0] * J[3] + gr[1] * J[4] + gr[2] * J[5];
      gdz = gr[0] * J[6] + gr[1] * J[7] + gr[2] * J[8];
#pragma unroll
      for (int k = 0; k < 16; ++k) {
        if (k < nb) { dsh[k * 3 + 0] = b[k] * gr[0]; dsh[k * 3 + 1] = b[k] * gr[1]; dsh[k * 3 + 2] = b[k] * gr[2]; }
      }
    } else {
      float dbx[16], dby[16], dbz[16];
      sh_basis_grad(a.sh_degree, ux, uy, uz, dbx, dby, dbz);
#pragma unroll
      for (int k = 0; k < 16; ++k) {
        if (k < nb) {
          dsh[k * 3 + 0] = b[k] * gr[0]; dsh[k * 3 + 1] = b[k] * gr[1]; dsh[k * 3 + 2] = b[k] * gr[2];
          const float dotc = gr[0] * sh[k * 3 + 0] + gr[1] * sh[k * 3 + 1] + gr[2] * sh[k * 3 + 2];
          gdx += dbx[k] * dotc; gdy += dby[k] * dotc; gdz += dbz[k] * dotc;
        }
      }
    }
    // through the normalisation dir = d/|d|
    const float dot = ux * gdx + uy * gdy + uz * gdz;
    vdir[0] = (gdx - ux * dot) * inv; vdir[1] = (gdy - uy * dot) * inv; vdir[2] = (gdz - uz * dot) * inv;
    if (!(LOD && a.lod_scatter)) {
      out.dL_dmeans3D[idx * 3 + 0] += vdir[0];
      out.dL_dmeans3D[idx * 3 + 1] += vdir[1];
      out.dL_dmeans3D[idx * 3 + 2] += vdir[2];
    }
  }
  if constexpr (LOD) {
    if (a.lod_scatter) {
      // scatter of the SH and mean gradients (see lod_run): rows staged in LDS (the four pad floats of a row carry its
      // node row, parent row, weight and "on screen"), every 16 bytes of a row handled by one lane
      __shared__ float lds_m[3 * kPreBlock];
      __shared__ int lds_par[kPreBlock];
      const int t = threadIdx.x;
      const int count = min(kPreBlock, a.P - block_first);
      const int stride = sh_row_stride(n), cpr = n >> 2;
      LodRow l;
      l.r = l.p = 0; l.w = 1.0f; l.u = 0.0f;
      if (valid) l = lod_row<true>(a, idx);
      if (valid) {
        lds_row_write(lds, n, dsh);
        float* pad = lds + t * stride + n;
        pad[0] = __uint_as_float((uint32_t)l.r); pad[1] = __uint_as_float((uint32_t)l.p); pad[2] = l.w;
        pad[3] = __uint_as_float(active ? 1u : 0u);
#pragma unroll
        for (int j = 0; j < 3; ++j) lds_m[j * kPreBlock + t] = active ? dmean_rows[idx * 3 + j] + vdir[j] : 0.0f;
      }
      lds_par[t] = valid ? (int)l.p : -1;
      __syncthreads();
      const bool nonmono = *lod_flag != 0u;
      float4* dsh_full = reinterpret_cast<float4*>(out.dL_dshs);
      for (int v = t; v < count * cpr; v += kPreBlock) {
        const int row = v / cpr, c = v - row * cpr;
        const float* rp = lds + row * stride;
        const uint32_t r = __float_as_uint(rp[n]), pr = __float_as_uint(rp[n + 1]);
        const bool self = r == pr;
        if (__float_as_uint(rp[n + 3])) {                         // node row: plain store
          const float wn = self ? 1.0f : rp[n + 2];
          const float4 g4 = *reinterpret_cast<const float4*>(rp + c * 4);
          dsh_full[(size_t)r * cpr + c] = make_float4(wn * g4.x, wn * g4.y, wn * g4.z, wn * g4.w);
        }
        const LodRun run = lod_run(a, lds_par, row, count, block_first, nonmono);
        if (run.leader) {
          float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
          bool any = false;
          for (int j = row; j < run.end; ++j) {
            const float* rj = lds + j * stride;
            if (!__float_as_uint(rj[n + 3]) || __float_as_uint(rj[n]) == __float_as_uint(rj[n + 1])) continue;
            any = true;
            const float uj = 1.0f - rj[n + 2];
            const float4 g4 = *reinterpret_cast<const float4*>(rj + c * 4);
            acc.x += uj * g4.x; acc.y += uj * g4.y; acc.z += uj * g4.z; acc.w += uj * g4.w;
          }
          if (any) {
            float* dst = reinterpret_cast<float*>(dsh_full + (size_t)pr * cpr + c);
            if (run.atomic) {
              atomicAdd(dst + 0, acc.x); atomicAdd(dst + 1, acc.y); atomicAdd(dst + 2, acc.z); atomicAdd(dst + 3, acc.w);
            } else {
              *reinterpret_cast<float4*>(dst) = acc;
            }
          }
        }
      }
      if (t < count) {                                            // the mean: one lane per row
        const float* rp = lds + t * stride;
        const uint32_t r = __float_as_uint(rp[n]), pr = __float_as_uint(rp[n + 1]);
        const bool self = r == pr;
        if (__float_as_uint(rp[n + 3])) {
          const float wn = self ? 1.0f : rp[n + 2];
#pragma unroll
          for (int j = 0; j < 3; ++j) out.dL_dmeans3D[(size_t)r * 3 + j] = wn * lds_m[j * kPreBlock + t];
        }
        const LodRun run = lod_run(a, lds_par, t, count, block_first, nonmono);
        if (run.leader) {
          float acc3[3] = {0.f, 0.f, 0.f};
          bool any = false;
          for (int j = t; j < run.end; ++j) {
            const float* rj = lds + j * stride;
            if (!__float_as_uint(rj[n + 3]) || __float_as_uint(rj[n]) == __float_as_uint(rj[n + 1])) continue;
            any = true;
            const float uj = 1.0f - rj[n + 2];
#pragma unroll
            for (int k = 0; k < 3; ++k) acc3[k] += uj * lds_m[k * kPreBlock + j];
          }
          if (any) {
#pragma unroll
            for (int k = 0; k < 3; ++k) lod_add(out.dL_dmeans3D + (size_t)pr * 3 + k, acc3[k], run.atomic);
          }
        }
      }
      return;
    }
  }
  if (coop) {
    if (valid) lds_row_write(lds, n, dsh);
    __syncthreads();
    if (split) {
      coop_store_seg<ACC>(out.dL_dshs, block_first, a.P, 3, 0, sh_row_stride(n), lds);
      coop_store_seg<ACC>(out.dL_dshs_rest, block_first, a.P, n - 3, 3, sh_row_stride(n), lds);
    } else {
      coop_store_sh<ACC>(out.dL_dshs, block_first, a.P, n, lds);
    }
  } else if (valid && split) {
    float* d0 = out.dL_dshs + (size_t)idx * 3;
    float* d1 = out.dL_dshs_rest + (size_t)idx * (n - 3);
#pragma unroll
    for (int i = 0; i < 48; ++i) {       // static indices keep dsh[] in registers
      if (i < 3) d0[i] = dsh[i] + (ACC ? d0[i] : 0.f);
      else if (i < n) d1[i - 3] = dsh[i] + (ACC ? d1[i - 3] : 0.f);
    }
  } else if (valid) {
    if (ACC) {
      const float* old = out.dL_dshs + (size_t)idx * n;
#pragma unroll
      for (int i = 0; i < 48; ++i)       // static indices keep dsh[] in registers
        if (i < n) dsh[i] += old[i];
    }
    store_sh(out.dL_dshs, idx, a.M, dsh);
  }
}

// d_mean += the view-direction term of dL/dmean, rounded as preprocess_bwd_kernel<false, false> followed by
// sh_bwd_kernel<false, true, false> round it: there the compiler contracts  x0 y0 + x1 y1 + x2 y2  into
// fma(x2, y2, fma(x0, y0, x1 y1)),  g - u dot  into  fma(-u, dot, g),  and K8b's  dL/dmean += v inv  into  fma(v, inv, .)
// on what K8a stored,  d_mean + 0.f  (a -0.f becomes +0.f).  Written out, with contraction off, so that the fused
// kernel does not depend on what the compiler makes of the same expressions in other surroundings.
__device__ __forceinline__ float k8_dot3(float x0, float y0, float x1, float y1, float x2, float y2) {
#pragma clang fp contract(off)
  return __fmaf_rn(x2, y2, __fmaf_rn(x0, y0, x1 * y1));
}
__device__ __forceinline__ void k8_add_view_term(const float (&gr)[3], const float (&J)[9], float ux, float uy, float uz,
                                                 float inv, float (&d_mean)[3]) {
#pragma clang fp contract(off)
  const float gdx = k8_dot3(gr[0], J[0], gr[1], J[1], gr[2], J[2]);
  const float gdy = k8_dot3(gr[0], J[3], gr[1], J[4], gr[2], J[5]);
  const float gdz = k8_dot3(gr[0], J[6], gr[1], J[7], gr[2], J[8]);
  const float dot = k8_dot3(ux, gdx, uy, gdy, uz, gdz);       // through the normalisation dir = d/|d|
  d_mean[0] = __fmaf_rn(__fmaf_rn(-ux, dot, gdx), inv, d_mean[0] + 0.f);
  d_mean[1] = __fmaf_rn(__fmaf_rn(-uy, dot, gdy), inv, d_mean[1] + 0.f);
  d_mean[2] = __fmaf_rn(__fmaf_rn(-uz, dot, gdz), inv, d_mean[2] + 0.f);
}

// K8a and K8b in one kernel, for the drop-in training call (launch_preprocess_bwd says when): what
// preprocess_bwd_kernel<false, false> and sh_bwd_kernel<false, true, false> compute together, to the bit, without the
// 64 bytes per Gaussian that only pass between the two (drgb out and in, dL/dmeans3D out, in and out again, the mean and
// tiles_touched a second time) and without the second launch.
//   entry    tiles_touched and offsets; each full wave's 64 rows of inputs by LDS DMA into the 12 KB behind the stages
//   phase 1  the run sums (k8_sum_runs); the waves' stages are the first 40 KB of the dynamic buffer
//   phase 2  the double chain (k8_chain) on the staged inputs, the wave's Jacobian rows landing in its stage meanwhile;
//            every gradient but the SH block is stored from registers
//   phase 3  K8b's JAC body on the mean and the masked dL/drgb still in registers (k8_add_view_term); dL/dmeans3D is
//            written once; then the buffer becomes the [256][3M + 4] output stage (every lane fills its row from b[] and
//            dL/drgb: no dsh[48] next to the chain) and the SH block leaves as whole lines (coop_store_sh)
// 160 registers like K8a (the double chain): three waves per SIMD, which three 53 KB buffers per compute unit also allow.
// No waves-per-SIMD hint: with its 168-register cap the compiler spills 32 bytes, without it it needs 160 and none.
template <bool STG>   // STG: records, inputs and Jacobians staged by LDS DMA (HGS_K8_STAGE=0: the loads through registers)
__global__ __launch_bounds__(kPreBlock) void preprocess_bwd_sh_kernel(hgs_raster_args a, GeomWs g,
                                                                         const float* __restrict__ inst,
                                                                         hgs_raster_grads out, int mode) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  const int block_first = blockIdx.x * kPreBlock;
  const int idx = block_first + threadIdx.x;
  const bool in_range = idx < a.P;                           // (out-of-range lanes stay: wave-wide staging, barriers)
  const int wave = threadIdx.x >> 6, wave_first = idx & ~63;
  unsigned char* st = smem_raw + wave * kK8StageBytes;       // the wave's stage; its inputs lie behind the four stages
  unsigned char* in = smem_raw + (kPreBlock / 64) * kK8StageBytes + wave * kK8InWave;
  CamLds cam;                                                // (once, in front of every write to memory: scalar loads)
  if constexpr (STG) {
    load_camera(a, cam);
    k8_stage_inputs(a, g, idx, mode, in);
  }
  const uint32_t n = in_range ? g.tiles_touched[idx] : 0u;
  uint32_t off = 0u;
  if constexpr (STG) { if (in_range) off = g.offsets[idx]; }
  else { if (n) off = g.offsets[idx]; }

  double s[10];
#pragma unroll
  for (int i = 0; i < 10; ++i) s[i] = 0.0;
  k8_sum_runs<STG>(inst, off, n, mode, reinterpret_cast<float2*>(st), s);
  // the wave's stage is free: its 64 Jacobian rows (2 304 contiguous bytes, 16-byte aligned; shjac holds whole waves)
  // land in it during the double chain
  const bool jac_staged = STG && wave_first < a.P;           // (wave-uniform)
  if constexpr (STG) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");         // (a wave that staged no records: the inputs have landed)
    if (jac_staged) {
      const int lane = threadIdx.x & 63;
      const char* src = reinterpret_cast<const char*>(g.shjac + (size_t)wave_first * kJacStride);
      static_assert(64 * kJacStride * 4 == 2304, "64 Jacobian rows = 144 pieces of 16 bytes");
      __builtin_amdgcn_global_load_lds((gptr_t)(src + lane * 16), (lptr_t)st, 16, 0, 0);
      __builtin_amdgcn_global_load_lds((gptr_t)(src + 1024 + lane * 16), (lptr_t)(st + 1024), 16, 0, 0);
      if (lane < 16) __builtin_amdgcn_global_load_lds((gptr_t)(src + 2048 + lane * 16), (lptr_t)(st + 2048), 16, 0, 0);
    }
  }

  float d_mean[3] = {0.f, 0.f, 0.f};
  float d_m2[3] = {0.f, 0.f, 0.f};
  float d_op = 0.f;
  float d_scale[3] = {0.f, 0.f, 0.f};
  float d_rot[4] = {0.f, 0.f, 0.f, 0.f};
  float d_c3[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  float gr[3] = {0.f, 0.f, 0.f};                             // clamp-masked dL/drgb
  float b[16];
  const int nb = (a.sh_degree + 1) * (a.sh_degree + 1);
  float p[3];
  if (n != 0) k8_chain<false, STG>(a, g, idx, s, p, d_mean, d_m2, d_op, d_scale, d_rot, d_c3, gr, in, &cam);
  // Staged, the rows are stored behind phase 3's arithmetic: a wait for the Jacobian DMA in front of them costs nothing
  // (it landed during the chain), behind them it would wait for the stores as well -- as the Jacobian loads of the
  // register route do.
  constexpr bool stores_last = STG;
  if (in_range && !stores_last) {
    const float d_col[3] = {0.f, 0.f, 0.f};
    k8_store_row<false>(out, idx, d_m2, d_op, d_scale, d_rot, d_c3, d_col);
  }
  __builtin_amdgcn_sched_barrier(0);                         // (phase 3's loads stay out of the double chain's registers)
  // every DMA of this wave has landed before its Jacobians are read and before the buffer becomes the output stage
  if constexpr (STG) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  if (n != 0) {
    float ux, uy, uz;
    const float inv = unit_dir(p, STG ? cam.cam : a.campos, ux, uy, uz);
    sh_basis(a.sh_degree, ux, uy, uz, b);
    float J[9];
    if (jac_staged) {
      const float* jl = reinterpret_cast<const float*>(st) + (threadIdx.x & 63) * kJacStride;
#pragma unroll
      for (int k = 0; k < 9; ++k) J[k] = jl[k];
    } else {
      const float* jp = g.shjac + (size_t)idx * kJacStride;
#pragma unroll
      for (int k = 0; k < 9; ++k) J[k] = jp[k];
    }
    k8_add_view_term(gr, J, ux, uy, uz, inv, d_mean);
  } else {
#pragma unroll
    for (int j = 0; j < 3; ++j) d_mean[j] = 0.f;             // (culled: K8a stores 0, K8b leaves it)
  }
  if (in_range) {
#pragma unroll
    for (int j = 0; j < 3; ++j) out.dL_dmeans3D[idx * 3 + j] = d_mean[j];
    if (stores_last) {
      const float d_col[3] = {0.f, 0.f, 0.f};
      k8_store_row<false>(out, idx, d_m2, d_op, d_scale, d_rot, d_c3, d_col);
    }
  }

  float* lds = reinterpret_cast<float*>(smem_raw);
  const int nc = a.M * 3, stride = sh_row_stride(nc);
  __syncthreads();                                           // (every wave has summed its runs: the stages are dead)
  if (in_range) {
    float* row = lds + threadIdx.x * stride;
#pragma unroll
    for (int i = 0; i < 12; ++i) {
      if (i * 4 < nc) {
        float v[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const int k = (i * 4 + c) / 3, ch = (i * 4 + c) % 3;
          v[c] = (n != 0 && k < nb) ? b[k] * gr[ch] : 0.f;     // (culled rows and the degrees above sh_degree: zeros)
        }
        *reinterpret_cast<float4*>(row + i * 4) = make_float4(v[0], v[1], v[2], v[3]);
      }
    }
  }
  __syncthreads();
  coop_store_sh<false>(out.dL_dshs, block_first, a.P, nc, lds);
}

// K8b for several views of the same Gaussians at once (hgs_raster_sh_bwd_batched): the SH block is read once and
// the gradient block written once for all views -- per view this kernel's traffic is otherwise the largest of the
// streaming kernels (384 B per Gaussian).
// COOP: 3M % 4 == 0, the SH block goes through LDS, else per-lane access.  COLOR: the views come from the batched
// colour route (gradient w.r.t. the clamped colour + clamp mask) instead of deferred raster backwards (masked
// gradient + visibility).
template <bool ACC, bool COOP, bool COLOR>
__device__ __forceinline__ void sh_bwd_batched_body(const ShBwdViews& v, int P, int M, int sh_degree,
                                                    const float* __restrict__ means3D, const float* __restrict__ shs,
                                                    float* __restrict__ dL_dshs, float* __restrict__ dL_dmeans3D) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  float* lds = reinterpret_cast<float*>(smem_raw);
  const int n = M * 3;
  constexpr bool coop = COOP;
  const int block_first = blockIdx.x * kPreBlock;
  const int idx = block_first + threadIdx.x;
  const bool valid = idx < P;
  if (coop) {
    coop_load_sh(shs, block_first, P, n, lds);
    __syncthreads();
  }
  // the coefficients stay in this lane's LDS row and are re-read per view (keeping them in registers next to the
  // 48 accumulators and the basis arrays costs a wave of occupancy)
  float sh_reg[COOP ? 1 : 48];
  if constexpr (!COOP) { if (valid) load_sh(shs, idx, M, sh_reg); }
  float dsh[48];
#pragma unroll
  for (int i = 0; i < 48; ++i) dsh[i] = 0.f;
  float gm0 = 0.f, gm1 = 0.f, gm2 = 0.f;
  if (valid) {
    const float px = means3D[idx * 3 + 0], py = means3D[idx * 3 + 1], pz = means3D[idx * 3 + 2];
    const int nb = (sh_degree + 1) * (sh_degree + 1);
    for (int w = 0; w < v.n; ++w) {
      if (!COLOR && static_cast<const uint32_t*>(v.mask[w])[idx] == 0) continue;
      float gr0 = v.drgb[w][idx * 3 + 0], gr1 = v.drgb[w][idx * 3 + 1], gr2 = v.drgb[w][idx * 3 + 2];
      if (COLOR) {            // the incoming gradient is w.r.t. the clamped colour
        const uint32_t m = static_cast<const uint8_t*>(v.mask[w])[idx];
        if (m & 1u) gr0 = 0.f;
        if (m & 2u) gr1 = 0.f;
        if (m & 4u) gr2 = 0.f;
        if (gr0 == 0.f && gr1 == 0.f && gr2 == 0.f) continue;      // culled / not contributing in this view
      }
      // dotc[k] = gr . c_k straight from the LDS row (or the registers of the per-lane path): no 48-float copy
      float dotc[16];
#pragma unroll
      for (int k = 0; k < 16; ++k) dotc[k] = 0.f;
      if constexpr (COOP) {
        const float4* row4 = reinterpret_cast<const float4*>(lds + threadIdx.x * sh_row_stride(n));
#pragma unroll
        for (int i = 0; i < 12; ++i) {
          if (i * 4 < n) {
            const float4 t = row4[i];
            const float tv[4] = {t.x, t.y, t.z, t.w};
#pragma unroll
            for (int c = 0; c < 4; ++c) {
              const int ch = (i * 4 + c) % 3;
              dotc[(i * 4 + c) / 3] += (ch == 0 ? gr0 : ch == 1 ? gr1 : gr2) * tv[c];
            }
          }
        }
      } else {
#pragma unroll
        for (int i = 0; i < 48; ++i) dotc[i / 3] += (i % 3 == 0 ? gr0 : i % 3 == 1 ? gr1 : gr2) * sh_reg[i];
      }
      const float pxyz[3] = {px, py, pz};
      float ux, uy, uz;
      const float inv = unit_dir(pxyz, v.campos[w], ux, uy, uz);
      {
        float b[16];
        sh_basis(sh_degree, ux, uy, uz, b);
#pragma unroll
        for (int k = 0; k < 16; ++k) {
          if (k < nb) { dsh[k * 3 + 0] += b[k] * gr0; dsh[k * 3 + 1] += b[k] * gr1; dsh[k * 3 + 2] += b[k] * gr2; }
        }
      }
      float gdx = 0.f, gdy = 0.f, gdz = 0.f;
      {
        float dbx[16], dby[16], dbz[16];
        sh_basis_grad(sh_degree, ux, uy, uz, dbx, dby, dbz);
#pragma unroll
        for (int k = 0; k < 16; ++k) {
          if (k < nb) { gdx += dbx[k] * dotc[k]; gdy += dby[k] * dotc[k]; gdz += dbz[k] * dotc[k]; }
        }
      }
      const float dot = ux * gdx + uy * gdy + uz * gdz;
      gm0 += (gdx - ux * dot) * inv;
      gm1 += (gdy - uy * dot) * inv;
      gm2 += (gdz - uz * dot) * inv;
    }
    dL_dmeans3D[idx * 3 + 0] += gm0;
    dL_dmeans3D[idx * 3 + 1] += gm1;
    dL_dmeans3D[idx * 3 + 2] += gm2;
  }
  if (coop) {
    __syncthreads();            // every lane is done reading its coefficients: the buffer becomes the output stage
    if (valid) lds_row_write(lds, n, dsh);
    __syncthreads();
    coop_store_sh<ACC>(dL_dshs, block_first, P, n, lds);
  } else if (valid) {
    if (ACC) {
      const float* old = dL_dshs + (size_t)idx * n;
#pragma unroll
      for (int i = 0; i < 48; ++i)
        if (i < n) dsh[i] += old[i];
    }
    store_sh(dL_dshs, idx, M, dsh);
  }
}

}  // namespace

template <bool ACC, bool COOP>
__global__ __launch_bounds__(kPreBlock) void sh_bwd_batched_kernel(ShBwdViews v, int P, int M, int sh_degree,
                                                                   const float* __restrict__ means3D,
                                                                   const float* __restrict__ shs,
                                                                   float* __restrict__ dL_dshs,
                                                                   float* __restrict__ dL_dmeans3D) {
  sh_bwd_batched_body<ACC, COOP, false>(v, P, M, sh_degree, means3D, shs, dL_dshs, dL_dmeans3D);
}
template <bool ACC, bool COOP>     // 3 workgroups per CU = what the LDS stage allows: keeps the registers under 170
__global__ __launch_bounds__(kPreBlock, 3) void sh_bwd_batched_color_kernel(ShBwdViews v, int P, int M, int sh_degree,
                                                                            const float* __restrict__ means3D,
                                                                            const float* __restrict__ shs,
                                                                            float* __restrict__ dL_dshs,
                                                                            float* __restrict__ dL_dmeans3D) {
  sh_bwd_batched_body<ACC, COOP, true>(v, P, M, sh_degree, means3D, shs, dL_dshs, dL_dmeans3D);
}

// Colours of one block of Gaussians for every view: SH block through LDS once, basis per view.
__global__ __launch_bounds__(kPreBlock) void sh_colors_batched_kernel(ShFwdViews v, int P, int M, int sh_degree,
                                                                      const float* __restrict__ means3D,
                                                                      const float* __restrict__ shs) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  float* lds = reinterpret_cast<float*>(smem_raw);
  const int n = M * 3;
  const bool coop = (n & 3) == 0;
  const int block_first = blockIdx.x * kPreBlock;
  const int idx = block_first + threadIdx.x;
  if (coop) {
    coop_load_sh(shs, block_first, P, n, lds);
    __syncthreads();
  }
  if (idx >= P) return;
  float sh[48];
  if (coop) lds_row_read(lds, n, sh); else load_sh(shs, idx, M, sh);
  const float px = means3D[idx * 3 + 0], py = means3D[idx * 3 + 1], pz = means3D[idx * 3 + 2];
  const int nb = (sh_degree + 1) * (sh_degree + 1);
  for (int w = 0; w < v.n; ++w) {
    const float pxyz[3] = {px, py, pz};
    float dx, dy, dz;
    unit_dir(pxyz, v.campos[w], dx, dy, dz);
    float b[16];
    sh_basis(sh_degree, dx, dy, dz, b);
    float r0 = 0.f, r1 = 0.f, r2 = 0.f;
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      if (k < nb) {
        r0 += b[k] * sh[k * 3 + 0];
        r1 += b[k] * sh[k * 3 + 1];
        r2 += b[k] * sh[k * 3 + 2];
      }
    }
    r0 += 0.5f; r1 += 0.5f; r2 += 0.5f;
    uint32_t m = 0;
    if (r0 < 0.f) { r0 = 0.f; m |= 1u; }
    if (r1 < 0.f) { r1 = 0.f; m |= 2u; }
    if (r2 < 0.f) { r2 = 0.f; m |= 4u; }
    v.rgb_out[w][idx * 3 + 0] = r0;
    v.rgb_out[w][idx * 3 + 1] = r1;
    v.rgb_out[w][idx * 3 + 2] = r2;
    v.clamp_out[w][idx] = (uint8_t)m;
  }
}

int launch_sh_colors_batched(const ShFwdViews& v, int32_t P, int32_t M, int32_t sh_degree, const float* means3D,
                             const float* shs, hipStream_t s) {
  const int nblk = (P + kPreBlock - 1) / kPreBlock;
  if (nblk <= 0) return HGS_OK;
  const size_t lds_bytes = (size_t)kPreBlock * (M * 3 + 4) * sizeof(float);
  hipLaunchKernelGGL(sh_colors_batched_kernel, dim3(nblk), dim3(kPreBlock), lds_bytes, s, v, P, M, sh_degree, means3D, shs);
  HGS_LAUNCH_CHECK("sh_colors_batched", s, false);
  return HGS_OK;
}

int launch_sh_bwd_batched(const ShBwdViews& v, int32_t P, int32_t M, int32_t sh_degree, const float* means3D,
                          const float* shs, float* dL_dshs, float* dL_dmeans3D, bool accumulate, hipStream_t s) {
  const int nblk = (P + kPreBlock - 1) / kPreBlock;
  if (nblk <= 0) return HGS_OK;
  const size_t lds_bytes = (size_t)kPreBlock * (M * 3 + 4) * sizeof(float);
  const bool coop = ((M * 3) & 3) == 0;
  const bool color = v.color != 0;
  auto kern = color ? (coop ? (accumulate ? sh_bwd_batched_color_kernel<true, true> : sh_bwd_batched_color_kernel<false, true>)
                            : (accumulate ? sh_bwd_batched_color_kernel<true, false> : sh_bwd_batched_color_kernel<false, false>))
                    : (coop ? (accumulate ? sh_bwd_batched_kernel<true, true> : sh_bwd_batched_kernel<false, true>)
                            : (accumulate ? sh_bwd_batched_kernel<true, false> : sh_bwd_batched_kernel<false, false>));
  hipLaunchKernelGGL(kern, dim3(nblk), dim3(kPreBlock), lds_bytes, s, v, P, M, sh_degree, means3D, shs, dL_dshs,
                     dL_dmeans3D);
  HGS_LAUNCH_CHECK("sh_bwd_batched", s, false);
  return HGS_OK;
}

// Zeroed superblock totals of K1 (above), one block per (device, stream): launches on one stream run one after the other
// and the counting kernel behind K3 leaves the block at zero, so it is zeroed by the host only when it is created -- or
// when an error return between K1 and that kernel left it `dirty`.  At most kMaxSyncBlocks distinct streams are served;
// further ones (and HGS_SCAN_LAUNCH=1) take the separate scan launch.
namespace {
constexpr int kMaxSyncBlocks = 64;
struct SyncBlock { int device; hipStream_t stream; uint32_t* words; bool dirty; };
std::mutex g_sync_mu;
SyncBlock g_sync[kMaxSyncBlocks];
int g_sync_n = 0;
}  // namespace
size_t super_block_bytes() { return (size_t)(2 + kBands) * kMaxSuper * sizeof(uint32_t); }   // 9 rows of totals + the heavy list
uint32_t* super_block_acquire(hipStream_t s) {
  static const bool off = getenv("HGS_SCAN_LAUNCH") != nullptr;
  if (off) return nullptr;
  // hipStreamPerThread is ONE handle for a different stream in every host thread: two threads' frames would share a block
  // and interleave their sums.  A capturing stream must not see the allocation / memset of a first use.  Both take the
  // scan launch.
  if (s == hipStreamPerThread) return nullptr;
  hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(s, &cap) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
  if (cap != hipStreamCaptureStatusNone) return nullptr;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
  std::lock_guard<std::mutex> lk(g_sync_mu);
  for (int i = 0; i < g_sync_n; ++i) {
    SyncBlock& b = g_sync[i];
    if (b.device != dev || b.stream != s) continue;
    if (b.dirty) {
      if (hipMemsetAsync(b.words, 0, super_block_bytes(), s) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
      b.dirty = false;
    }
    return b.words;
  }
  if (g_sync_n == kMaxSyncBlocks) return nullptr;
  uint32_t* w = nullptr;
  if (hipMalloc(reinterpret_cast<void**>(&w), super_block_bytes()) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
  if (hipMemsetAsync(w, 0, super_block_bytes(), s) != hipSuccess) { (void)hipGetLastError(); (void)hipFree(w); return nullptr; }
  g_sync[g_sync_n++] = {dev, s, w, false};
  return w;
}
// Frees the blocks of `device` (all devices: < 0).  The caller guarantees that no call of this library is in flight there.
int super_block_release(int device) {
  std::lock_guard<std::mutex> lk(g_sync_mu);
  int kept = 0, freed = 0;
  for (int i = 0; i < g_sync_n; ++i) {
    if (device < 0 || g_sync[i].device == device) {
      int cur = 0;
      const bool sw = hipGetDevice(&cur) == hipSuccess && cur != g_sync[i].device && hipSetDevice(g_sync[i].device) == hipSuccess;
      (void)hipFree(g_sync[i].words);
      if (sw) (void)hipSetDevice(cur);
      ++freed;
    } else {
      g_sync[kept++] = g_sync[i];
    }
  }
  g_sync_n = kept;
  return freed;
}
void super_block_mark_dirty(const uint32_t* words) {
  std::lock_guard<std::mutex> lk(g_sync_mu);
  for (int i = 0; i < g_sync_n; ++i)
    if (g_sync[i].words == words) g_sync[i].dirty = true;
}

int launch_preprocess_fwd(const hgs_raster_args& a, const GeomWs& g, int32_t* radii, hipStream_t s, uint32_t* super,
                          uint32_t heavy_thr) {
  const int nblk = (a.P + kPreBlock - 1) / kPreBlock;
  if (nblk > 0) {
    const bool jac = a.prepare_backward && a.shs;
    const bool plain = a.shs && !a.shs_rest && !a.lod_render_indices && ((a.M * 3) & 3) == 0;
    const bool h48 = plain && a.M == 16;
    const bool defer = plain && !h48;
    const size_t lds_bytes = !a.shs ? 0 : h48 ? (size_t)kK1ImageBytes : (size_t)kPreBlock * (a.M * 3 + 4) * sizeof(float);
    auto k1 = a.lod_half_rows      ? preprocess_fwd_lod_half_kernel     // (only with lod_render_indices, never jac: abi.cpp)
              : a.lod_render_indices ? (jac ? preprocess_fwd_kernel<true, true, false> : preprocess_fwd_kernel<false, true, false>)
              : h48   ? (jac ? preprocess_fwd_h48_kernel<true> : preprocess_fwd_h48_kernel<false>)
              : defer ? (jac ? preprocess_fwd_kernel<true, false, true> : preprocess_fwd_kernel<false, false, true>)
                      : (jac ? preprocess_fwd_kernel<true, false, false> : preprocess_fwd_kernel<false, false, false>);
    hipLaunchKernelGGL(k1, dim3(nblk), dim3(kPreBlock), lds_bytes, s, a, g, radii, super, heavy_thr);
    HGS_LAUNCH_CHECK("preprocess_fwd", s, a.debug);
  }
  return HGS_OK;
}

int launch_scan_block_sums(const GeomWs& g, int32_t P, hipStream_t s, bool debug, uint32_t* total_mirror) {
  const int nblk = (P + kPreBlock - 1) / kPreBlock;
  const int chunks = scan_chunks(nblk), resident = scan_resident_workgroups();
  if (chunks * (1 + kBands) <= resident && !scan_split_forced()) {
    hipLaunchKernelGGL(scan_block_sums_kernel, dim3(chunks, 1 + kBands), dim3(1024), 0, s, g.block_sums, g.block_band,
                       nblk, g.scan_chain, total_mirror, 0, chunks);
    HGS_LAUNCH_CHECK("scan_block_sums", s, debug);
    return HGS_OK;
  }
  // one launch per array (the kernel's row 0 scans its first pointer) and per `resident` chunks of it: a chunk only looks
  // back at chunks of its own launch -- resident together with it -- or of launches that have completed.  (A CU mask in
  // the environment makes `resident` 1: one launch per chunk, slow and correct.)
  for (int y = 0; y < 1 + kBands; ++y) {
    uint32_t* sums = y == 0 ? g.block_sums : g.block_band + (size_t)(y - 1) * (nblk + 1);
    for (int c0 = 0; c0 < chunks; c0 += resident) {
      hipLaunchKernelGGL(scan_block_sums_kernel, dim3(min(resident, chunks - c0), 1), dim3(1024), 0, s, sums, g.block_band,
                         nblk, g.scan_chain + (size_t)y * chunks, y == 0 ? total_mirror : nullptr, c0, chunks);
      HGS_LAUNCH_CHECK("scan_block_sums", s, debug);
    }
  }
  return HGS_OK;
}

int launch_preprocess_bwd(const hgs_raster_args& a, const GeomWs& g, const BwdWs& w, const hgs_raster_grads& out, uint32_t L,
                          hipStream_t s) {
  const int nblk = (a.P + kPreBlock - 1) / kPreBlock;
  if (nblk > 0) {
    // long runs first, when the frame has them: mean run above 6 records (L > 6 P; HGS_K8_PRESUM=0 / 1 forces; read on
    // every call, like the two switches below)
    const char* force = getenv("HGS_K8_PRESUM");
    const bool presum = force ? force[0] == '1' : (uint64_t)L > 6ull * (uint64_t)a.P;
    if (presum) {
      HGS_HIP(hipMemsetAsync(w.work_counter, 0, sizeof(uint32_t), s));
      hipLaunchKernelGGL(k8_worklist_kernel, dim3(nblk < kWorklistGrid ? nblk : kWorklistGrid), dim3(kPreBlock), 0, s, a.P,
                         g.tiles_touched, w.work, w.work_counter);
      HGS_LAUNCH_CHECK("preprocess_bwd_worklist", s, a.debug);
      const int want = (int)(((size_t)L / 64 + 3) / 4);                   // no more workgroups than a pair each could use
      hipLaunchKernelGGL(k8_presum_work_kernel, dim3(want < 1 ? 1 : (want < kPresumGrid ? want : kPresumGrid)), dim3(kPreBlock), 0,
                         s, w.work, w.work_counter, g.tiles_touched, g.offsets, w.inst_grads);
      HGS_LAUNCH_CHECK("preprocess_bwd_long_runs", s, a.debug);
    }
    // LDS DMA staging (k8_sum_runs, k8_stage_inputs; HGS_K8_STAGE=0 keeps the loads through registers; read on every
    // call): the kernels' STG forms when the scratch and the Jacobians are 16-byte aligned and the rows are not gathered
    // by index; in them the per-Gaussian inputs by DMA when every one of their tensors is aligned (a torch view with a
    // storage offset is not; scales and rotations are absent with a precomputed covariance)
    const char* stage_env = getenv("HGS_K8_STAGE");
    const auto al16 = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; };
    int mode = presum ? kK8ModePresum : 0;
    if (!(stage_env && stage_env[0] == '0') && !a.lod_render_indices && al16(w.inst_grads) && al16(g.shjac)) {
      mode |= kK8ModeStage;
      if (al16(a.means3D) && al16(a.scales) && al16(a.rotations) && al16(a.opacities) && al16(g.flags)) mode |= kK8ModeStageIn;
    }
    const bool stg = (mode & kK8ModeStage) != 0;
    // the drop-in training call: K8a and K8b as one kernel (HGS_K8_FUSE=0 keeps them apart; read on every call)
    const char* fuse_env = getenv("HGS_K8_FUSE");
    const bool fused = !(fuse_env && fuse_env[0] == '0') && !a.lod_render_indices && !a.accumulate_grads &&
                       !a.defer_sh_bwd && a.shs && !a.shs_rest && out.dL_dshs && a.prepare_backward && !a.colors_precomp &&
                       ((a.M * 3) & 3) == 0;
    if (fused) {       // one dynamic LDS buffer: the four waves' run stages and staged inputs, then the output stage
      const size_t stage_bytes = kK8LdsBytes;
      const size_t rows_bytes = (size_t)kPreBlock * (a.M * 3 + 4) * sizeof(float);
      hipLaunchKernelGGL(stg ? preprocess_bwd_sh_kernel<true> : preprocess_bwd_sh_kernel<false>, dim3(nblk), dim3(kPreBlock),
                         stage_bytes > rows_bytes ? stage_bytes : rows_bytes, s, a, g, w.inst_grads, out, mode);
      HGS_LAUNCH_CHECK("preprocess_bwd_sh", s, a.debug);
      return HGS_OK;
    }
    auto k8a = a.lod_render_indices ? preprocess_bwd_kernel<false, true>      // (accumulation is refused with lod, abi.cpp)
               : stg ? (a.accumulate_grads ? preprocess_bwd_staged_kernel<true> : preprocess_bwd_staged_kernel<false>)
                     : (a.accumulate_grads ? preprocess_bwd_kernel<true, false> : preprocess_bwd_kernel<false, false>);
    hipLaunchKernelGGL(k8a, dim3(nblk), dim3(kPreBlock), 0, s, a, g, w.inst_grads, w.drgb, w.dmean_rows, w.lod_flag, out,
                       mode);
    HGS_LAUNCH_CHECK("preprocess_bwd", s, a.debug);
    if (a.shs && out.dL_dshs && !a.defer_sh_bwd) {
      const size_t lds_bytes = (size_t)kPreBlock * (a.M * 3 + 4) * sizeof(float);
      auto k8b = a.lod_render_indices ? sh_bwd_kernel<false, true, true>
                 : (a.prepare_backward && a.shs) ? (a.accumulate_grads ? sh_bwd_kernel<true, true, false> : sh_bwd_kernel<false, true, false>)
                                                 : (a.accumulate_grads ? sh_bwd_kernel<true, false, false> : sh_bwd_kernel<false, false, false>);
      hipLaunchKernelGGL(k8b, dim3(nblk), dim3(kPreBlock), lds_bytes, s, a, g, w.drgb, w.dmean_rows, w.lod_flag, out);
      HGS_LAUNCH_CHECK("sh_bwd", s, a.debug);
    }
  }
  return HGS_OK;
}

}  // namespace hgs
