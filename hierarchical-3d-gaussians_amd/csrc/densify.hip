// K14 / K15: adaptive density control as one stream compaction.  Replaces the torch chain of
// the reference's GaussianModel.densify_and_prune (scene/gaussian_model.py:528-685, called from train_single.py:150-151:
// clone, split, two prunes -- three passes of boolean-mask indexing and torch.cat over six parameter tensors and their
// twelve Adam moment tensors) by a PLAN (class and rank of every row) and an APPLY (every output row written once).
//
// The rule, per row r of P (F protected leading rows = scaffold_points, tau = max_grad, d = percent_dense * extent):
//     g = accum, NaN -> 0;  o = sigmoid(opacity);  m = max_k exp(scaling_k);  w = max_radii2D * o^(1/5)
//     clone = (|g| w >= tau) and (o > 0.15) and (m <= d) and (r >= F)
//     split = ( g  w >= tau) and (o > 0.15) and (m >  d) and (r >= F)      (no absolute value: gaussian_model.py:625)
//     low   = o < min_opacity
// Output rows, each block in ascending r:  [originals with not split and not (low and r >= F)] [clones with not low]
// [child 0 of splits with not low] [child 1 of the same rows].  The k-th split row (ascending r, pruned ones counted)
// owns the noise rows z[k] and z[S + k].  Child j:  xyz' = xyz + R(q / |q|) (exp(scaling) * z_j),
// scaling' = log(exp(scaling) / 1.6), everything else copied; moments of every new row are zero.
//
// plan:  24 B read and 8 B written per row (+ four sums per 256 rows); apply: every element of a source row is read once
// with its two moments and stored to its destinations.  Destinations are monotone in r, so consecutive threads store
// contiguous runs; a thread carries four elements 256 apart so that four rounds of loads are in flight.  No atomics anywhere: the order of the output rows is a function of the inputs alone.
#include "common.h"

namespace hgs {
namespace {

constexpr int kMaxTensors = HGS_ADAM_MAX_TENSORS;
constexpr int kRows = 256;                       // rows per plan workgroup = one entry of each of the four sum arrays
constexpr uint32_t kKeepOrig = 1u, kKeepClone = 2u, kSplit = 4u, kKeepSplit = 8u;

// per source row: x = its four exclusive ranks inside its workgroup, one byte each (kept originals, kept clones, split
// rows, kept split rows: at most 255), y = the class bits
__host__ __device__ inline size_t plan_blocks(int64_t P) { return (size_t)((P + kRows - 1) / kRows); }
inline size_t sums_stride(int64_t P) { return align_up((plan_blocks(P) + 1) * sizeof(uint32_t)) / sizeof(uint32_t); }

__device__ __forceinline__ uint32_t lanes_below(uint64_t b) {
  return __builtin_amdgcn_mbcnt_hi((uint32_t)(b >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)b, 0u));
}

__global__ __launch_bounds__(kRows) void densify_plan_kernel(const float* __restrict__ accum, const float* __restrict__ radii,
                                                             const float* __restrict__ opacity,
                                                             const float* __restrict__ scaling, int64_t P, int64_t F,
                                                             float tau, float min_opacity, float d,
                                                             uint2* __restrict__ rec, uint32_t* __restrict__ sums,
                                                             uint32_t stride) {
  __shared__ uint32_t wave_cnt[kRows / 64][4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t r = (int64_t)blockIdx.x * kRows + tid;
  uint32_t cls = 0;
  if (r < P) {
    float g = accum[r];
    g = (g != g) ? 0.0f : g;
    const float o = 1.0f / (1.0f + expf(-opacity[r]));
    const float m = fmaxf(fmaxf(expf(scaling[3 * r]), expf(scaling[3 * r + 1])), expf(scaling[3 * r + 2]));
    const float rad = radii[r], pw = powf(o, 0.2f);
    const bool open = r >= F, solid = o > 0.15f;
    const bool clone = (fabsf(g) * rad * pw >= tau) && solid && (m <= d) && open;
    const bool split = (g * rad * pw >= tau) && solid && (m > d) && open;
    const bool low = o < min_opacity;
    if (!split && !(low && open)) cls |= kKeepOrig;
    if (clone && !low) cls |= kKeepClone;
    if (split) cls |= kSplit;
    if (split && !low) cls |= kKeepSplit;
  }
  uint32_t rank[4], tot[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const uint64_t b = __ballot((cls >> k) & 1u);
    rank[k] = lanes_below(b);
    tot[k] = (uint32_t)__popcll(b);
    if (lane == 0) wave_cnt[wave][k] = tot[k];
  }
  __syncthreads();
  uint32_t packed = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    uint32_t base = 0, all = 0;
#pragma unroll
    for (int w = 0; w < kRows / 64; ++w) {
      const uint32_t c = wave_cnt[w][k];
      base += (w < wave) ? c : 0u;
      all += c;
    }
    packed |= ((base + rank[k]) & 255u) << (8 * k);     // a set bit's exclusive rank is at most 255
    if (tid == 0) sums[(size_t)k * stride + blockIdx.x] = all;
  }
  if (r < P) rec[r] = make_uint2(packed, cls);
}

// In-place exclusive scan of the four sum arrays, one 1024-thread workgroup per array walking it 1024 entries per round
// (32 rounds at 8 M rows); totals as int64 to `totals` (device-visible memory: plain vector stores).
__global__ __launch_bounds__(1024) void densify_scan_kernel(uint32_t* __restrict__ sums, uint32_t stride, uint32_t n,
                                                            int64_t* __restrict__ totals) {
  __shared__ uint32_t wave_tot[16];
  uint32_t* a = sums + (size_t)blockIdx.x * stride;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  uint64_t carry = 0;
  for (uint32_t i0 = 0; i0 < n; i0 += 1024) {
    const uint32_t i = i0 + tid;
    const uint32_t v = i < n ? a[i] : 0u;
    uint32_t inc = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const uint32_t t = __shfl_up(inc, off, 64);
      if (lane >= off) inc += t;
    }
    if (lane == 63) wave_tot[wave] = inc;
    __syncthreads();
    uint32_t wbase = 0, all = 0;
#pragma unroll
    for (int w = 0; w < 16; ++w) {
      const uint32_t t = wave_tot[w];
      wbase += (w < wave) ? t : 0u;
      all += t;
    }
    if (i < n) a[i] = (uint32_t)carry + wbase + inc - v;
    carry += all;
    __syncthreads();
  }
  if (tid == 0) totals[blockIdx.x] = (int64_t)carry;
}

struct DensifyLaunch {
  hgs_densify_tensor t[kMaxTensors];
  uint32_t first_block[kMaxTensors + 1];   // block range of every tensor
};

struct DensifyCounts {
  int64_t n_orig, n_clone, n_split, n_kept_split, n_out;
};

constexpr int kPerThread = 4;                    // elements per apply thread, 256 apart: four rounds of loads in flight

// Every element of a source row is handled by one thread: kPerThread elements per thread, all of their loads issued
// before the first is waited for (the stores could alias the sources as far as the compiler knows, so the phases are
// written out: records and values, then moments and block offsets, then the stores).  One element per thread kept
// half as many bytes in flight and reached 47 % of the byte floor (profiles/f8_densify_kernels.md).
template <typename IDX>
__global__ __launch_bounds__(256) void densify_apply_kernel(DensifyLaunch L, int n_tensors, int64_t P, DensifyCounts N,
                                                            const uint2* __restrict__ rec,
                                                            const uint32_t* __restrict__ sums, uint32_t stride,
                                                            const float* __restrict__ scaling,
                                                            const float* __restrict__ rotation,
                                                            const float* __restrict__ noise) {
  int ti = 0;
#pragma unroll
  for (int k = 1; k < kMaxTensors; ++k)
    if (k < n_tensors && blockIdx.x >= L.first_block[k]) ti = k;
  const hgs_densify_tensor& T = L.t[ti];
  const IDX len = (IDX)T.row_len;
  const IDX total = (IDX)P * len;
  const IDX e0 = (IDX)(blockIdx.x - L.first_block[ti]) * (256 * kPerThread) + threadIdx.x;
  const bool moments = T.exp_avg != nullptr;
  IDX e[kPerThread], r[kPerThread];
  uint2 rc[kPerThread];
  float v[kPerThread], m1[kPerThread], m2[kPerThread];
  uint32_t off[kPerThread][4];
#pragma unroll
  for (int u = 0; u < kPerThread; ++u) {
    e[u] = e0 + (IDX)(u * 256);
    const IDX ee = e[u] < total ? e[u] : (IDX)0;        // clamped index + select, no branch per load
    r[u] = ee / len;
    rc[u] = rec[r[u]];
    v[u] = T.src[ee];
  }
#pragma unroll
  for (int u = 0; u < kPerThread; ++u) {
    if (e[u] >= total) rc[u].y = 0u;
    const uint32_t cls = rc[u].y;
    const size_t blk = (size_t)(r[u] / kRows);
    m1[u] = m2[u] = 0.0f;
    if (moments && (cls & kKeepOrig)) {
      m1[u] = T.exp_avg[e[u]];
      m2[u] = T.exp_avg_sq[e[u]];
    }
    off[u][0] = (cls & kKeepOrig) ? sums[blk] : 0u;
    off[u][1] = (cls & kKeepClone) ? sums[stride + blk] : 0u;
    off[u][2] = (cls & kKeepSplit) ? sums[2 * (size_t)stride + blk] : 0u;
    off[u][3] = (cls & kKeepSplit) ? sums[3 * (size_t)stride + blk] : 0u;
  }
#pragma unroll
  for (int u = 0; u < kPerThread; ++u) {
    const uint32_t cls = rc[u].y, ranks = rc[u].x;
    const int c = (int)(e[u] - r[u] * len);
    if (cls & kKeepOrig) {
      const int64_t row = (int64_t)off[u][0] + (ranks & 255u);
      if (row < N.n_out) {
        const int64_t o = row * T.row_len + c;
        T.dst[o] = v[u];
        if (moments) {
          T.dst_exp_avg[o] = m1[u];
          T.dst_exp_avg_sq[o] = m2[u];
        }
      }
    }
    if (cls & kKeepClone) {
      const int64_t row = N.n_orig + (int64_t)off[u][1] + ((ranks >> 8) & 255u);
      if (row < N.n_out) {
        const int64_t o = row * T.row_len + c;
        T.dst[o] = v[u];
        if (moments) {
          T.dst_exp_avg[o] = 0.0f;
          T.dst_exp_avg_sq[o] = 0.0f;
        }
      }
    }
    if (cls & kKeepSplit) {
      const int64_t k = (int64_t)off[u][2] + ((ranks >> 16) & 255u);       // noise rank
      const int64_t row0 = N.n_orig + N.n_clone + (int64_t)off[u][3] + ((ranks >> 24) & 255u);
      const int64_t row1 = row0 + N.n_kept_split;
      if (row1 < N.n_out && k < N.n_split) {
        float c0 = v[u], c1 = v[u];
        if (T.kind == HGS_DENSIFY_XYZ) {
          const float* s = scaling + (int64_t)r[u] * 3;
          const float* q = rotation + (int64_t)r[u] * 4;
          const float s0 = expf(s[0]), s1 = expf(s[1]), s2 = expf(s[2]);
          const float qr = q[0], qx = q[1], qy = q[2], qz = q[3];
          const float norm = sqrtf(qr * qr + qx * qx + qy * qy + qz * qz);
          const float w = qr / norm, x = qx / norm, y = qy / norm, z = qz / norm;
          float R0, R1, R2;                                  // row c of utils/general_utils.py:82-103
          if (c == 0) { R0 = 1.0f - 2.0f * (y * y + z * z); R1 = 2.0f * (x * y - w * z); R2 = 2.0f * (x * z + w * y); }
          else if (c == 1) { R0 = 2.0f * (x * y + w * z); R1 = 1.0f - 2.0f * (x * x + z * z); R2 = 2.0f * (y * z - w * x); }
          else { R0 = 2.0f * (x * z - w * y); R1 = 2.0f * (y * z + w * x); R2 = 1.0f - 2.0f * (x * x + y * y); }
          const float* z0 = noise + k * 3;
          const float* z1 = noise + (N.n_split + k) * 3;
          c0 = (R0 * (s0 * z0[0]) + R1 * (s1 * z0[1]) + R2 * (s2 * z0[2])) + v[u];
          c1 = (R0 * (s0 * z1[0]) + R1 * (s1 * z1[1]) + R2 * (s2 * z1[2])) + v[u];
        } else if (T.kind == HGS_DENSIFY_SCALING) {
          c0 = c1 = logf(expf(v[u]) / 1.6f);
        }
        const int64_t o0 = row0 * T.row_len + c, o1 = row1 * T.row_len + c;
        T.dst[o0] = c0;
        T.dst[o1] = c1;
        if (moments) {
          T.dst_exp_avg[o0] = 0.0f;
          T.dst_exp_avg_sq[o0] = 0.0f;
          T.dst_exp_avg[o1] = 0.0f;
          T.dst_exp_avg_sq[o1] = 0.0f;
        }
      }
    }
  }
}

constexpr int64_t kMaxRows = 0x7fffffff;        // 32-bit block sums and one 1-D grid of row workgroups

}  // namespace
}  // namespace hgs

using namespace hgs;

// tmp: [P] ranks and class bits of every source row, then the four workgroup-sum arrays [4][sums_stride(P)]
struct DensifyTmp { uint2* rec; uint32_t* sums; };
static DensifyTmp carve_densify(Carver& c, int64_t P) {     // (a braced list is evaluated left to right)
  return {c.take<uint2>((size_t)(P > 0 ? P : 1)), c.take<uint32_t>(4 * sums_stride(P))};
}

extern "C" size_t hgs_densify_tmp_bytes(int64_t P) {
  if (P < 0 || P > kMaxRows) { set_error("densify: bad sizes (P = %lld outside [0, 2^31 - 1])", (long long)P); return 0; }
  Carver c(nullptr);
  carve_densify(c, P);
  return c.bytes(0);   // this workspace never had a slack block
}

extern "C" int hgs_densify_plan(const float* accum, const float* radii, const float* opacity, const float* scaling,
                                int64_t P, int64_t F, float max_grad, float min_opacity, float d, void* tmp,
                                int64_t* totals, int32_t wait, hgs_stream_t stream, int device) {
  if (P < 0 || P > kMaxRows) { set_error("densify: bad sizes (P = %lld outside [0, 2^31 - 1])", (long long)P); return HGS_ERR_INVALID; }
  if (F < 0 || F > P) { set_error("densify: %lld protected rows of %lld", (long long)F, (long long)P); return HGS_ERR_INVALID; }
  if (!(max_grad > 0.0f) || !(max_grad <= 3.402823466e38f)) { set_error("densify: max_grad must be positive and finite"); return HGS_ERR_INVALID; }
  if (min_opacity != min_opacity || d != d) { set_error("densify: min_opacity / d is NaN"); return HGS_ERR_INVALID; }
  if (!tmp || !totals || (P > 0 && (!accum || !radii || !opacity || !scaling))) { set_error("densify: null argument"); return HGS_ERR_INVALID; }
  HGS_HIP(hipSetDevice(device));
  hipStream_t s = static_cast<hipStream_t>(stream);
  const uint32_t nblk = (uint32_t)plan_blocks(P), stride = (uint32_t)sums_stride(P);
  Carver c(tmp);
  const DensifyTmp t = carve_densify(c, P);
  if (nblk) {
    hipLaunchKernelGGL(densify_plan_kernel, dim3(nblk), dim3(kRows), 0, s, accum, radii, opacity, scaling, P, F, max_grad,
                       min_opacity, d, t.rec, t.sums, stride);
    HGS_LAUNCH_CHECK("densify_plan", s, false);
  }
  hipLaunchKernelGGL(densify_scan_kernel, dim3(4), dim3(1024), 0, s, t.sums, stride, nblk, totals);
  HGS_LAUNCH_CHECK("densify_scan", s, false);
  if (wait) HGS_HIP(wait_stream(s));
  return HGS_OK;
}

extern "C" int hgs_densify_apply(const hgs_densify_tensor* tensors, int32_t n_tensors, int64_t P, const int64_t* totals,
                                 const float* scaling, const float* rotation, const float* noise, const void* tmp,
                                 hgs_stream_t stream, int device) {
  if (n_tensors <= 0) return HGS_OK;
  if (!tensors || n_tensors > kMaxTensors) { set_error("densify: 1..%d tensors per call", kMaxTensors); return HGS_ERR_INVALID; }
  if (P < 0 || P > kMaxRows) { set_error("densify: bad sizes (P = %lld outside [0, 2^31 - 1])", (long long)P); return HGS_ERR_INVALID; }
  if (!totals || !tmp) { set_error("densify: null argument"); return HGS_ERR_INVALID; }
  DensifyCounts N{totals[0], totals[1], totals[2], totals[3], 0};
  if (N.n_orig < 0 || N.n_orig > P || N.n_clone < 0 || N.n_clone > P || N.n_split < 0 || N.n_split > P ||
      N.n_kept_split < 0 || N.n_kept_split > N.n_split || N.n_orig + N.n_split > P) {
    set_error("densify: totals (%lld, %lld, %lld, %lld) are not those of a plan over %lld rows", (long long)N.n_orig,
              (long long)N.n_clone, (long long)N.n_split, (long long)N.n_kept_split, (long long)P);
    return HGS_ERR_INVALID;
  }
  N.n_out = N.n_orig + N.n_clone + 2 * N.n_kept_split;
  if (P == 0 || N.n_out == 0) return HGS_OK;
  DensifyLaunch L;
  uint64_t nb = 0;
  bool wide = false, geometry = false;
  const int64_t rows_max = N.n_out > P ? N.n_out : P;
  for (int k = 0; k < n_tensors; ++k) {
    const hgs_densify_tensor& t = tensors[k];
    if (!t.src || !t.dst || t.row_len <= 0 || (t.exp_avg != nullptr) != (t.exp_avg_sq != nullptr) ||
        (t.exp_avg && (!t.dst_exp_avg || !t.dst_exp_avg_sq))) {
      set_error("densify: tensor %d has a null pointer, half a pair of moments or row_len <= 0", k);
      return HGS_ERR_INVALID;
    }
    if (t.kind != HGS_DENSIFY_COPY && t.kind != HGS_DENSIFY_XYZ && t.kind != HGS_DENSIFY_SCALING) {
      set_error("densify: tensor %d has kind %d", k, t.kind);
      return HGS_ERR_INVALID;
    }
    if ((t.kind == HGS_DENSIFY_XYZ || t.kind == HGS_DENSIFY_SCALING) && t.row_len != 3) {
      set_error("densify: tensor %d: xyz and scaling rows have 3 floats, not %d", k, t.row_len);
      return HGS_ERR_INVALID;
    }
    if (rows_max > (int64_t)(0x7fffffffffffffffll / 4) / t.row_len) {
      set_error("densify: tensor %d: %lld rows of %d floats overflow", k, (long long)rows_max, t.row_len);
      return HGS_ERR_INVALID;
    }
    geometry = geometry || t.kind == HGS_DENSIFY_XYZ;
    wide = wide || (rows_max * (int64_t)t.row_len >= (int64_t)0x7fffff00);
    L.t[k] = t;
    L.first_block[k] = (uint32_t)nb;
    nb += (uint64_t)((P * t.row_len + 256 * kPerThread - 1) / (256 * kPerThread));
    if (nb > 0x7fffffffull) { set_error("densify: too many elements for one launch"); return HGS_ERR_INVALID; }
  }
  if (geometry && N.n_kept_split > 0 && (!scaling || !rotation || !noise)) {
    set_error("densify: split children need scaling, rotation and noise");
    return HGS_ERR_INVALID;
  }
  for (int k = n_tensors; k <= kMaxTensors; ++k) L.first_block[k] = (uint32_t)nb;
  HGS_HIP(hipSetDevice(device));
  hipStream_t s = static_cast<hipStream_t>(stream);
  void (*kern)(DensifyLaunch, int, int64_t, DensifyCounts, const uint2*, const uint32_t*, uint32_t, const float*,
               const float*, const float*) = wide ? densify_apply_kernel<int64_t> : densify_apply_kernel<uint32_t>;
  Carver c(const_cast<void*>(tmp));
  const DensifyTmp dt = carve_densify(c, P);
  hipLaunchKernelGGL(kern, dim3((uint32_t)nb), dim3(256), 0, s, L, n_tensors, P, N, dt.rec, dt.sums,
                     (uint32_t)sums_stride(P), scaling, rotation, noise);
  HGS_LAUNCH_CHECK("densify_apply", s, false);
  return HGS_OK;
}
