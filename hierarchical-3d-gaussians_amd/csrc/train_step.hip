// The bookkeeping between loss.backward() and the next render.  Replaces the
// ~twenty torch launches and four device-to-host waits of train_single.py:144-186, train_post.py:164-192 and
// train_coarse.py:110-145 -- densification statistics, gradient locking, `relevant = (opacity.grad != 0).nonzero()`,
// the optimizer step and the big-Gaussian scale clamp -- by a SELECT (statistics; one class byte per model row; one
// "some row was selected" word) and an APPLY (Adam on the selected rows of every tensor with the effective gradient,
// the clamp on the freshly updated scaling row while it is in registers).  include/hgs.h states the rule.
//
// Nothing comes back to the host: the empty-`relevant` case (scene/OurAdam.py:214 takes the dense path) is decided
// inside the apply kernel from the word.  The Adam update is adam.hip's (adam_update.h holds it once): selected rows are bit
// for bit what hgs_adam_step gives on a gradient whose locked rows were zeroed.
//
// select: 4 B (opacity gradient) read and 1 B written per model row, + 4 B (radius) per rendered row and, per visible
// row, 8 B of means2D gradient and three 4 B read-modify-writes.  apply: 16 B read + 12 B written per updated element
// (adam.hip's 28 B) + the class byte of its row; with the clamp, every scaling row is read.
#include "adam_update.h"

namespace hgs {
namespace {

constexpr int kMaxTensors = HGS_ADAM_MAX_TENSORS;
constexpr uint8_t kSelected = 1, kLocked = 2, kClampCandidate = 4;
constexpr int64_t kMaxRows = 0x7fffffff;
constexpr int kPerThread = 4;      // elements per apply thread, 256 apart: four rounds of loads in flight

// tmp: [the word, one kAlign block][P class bytes]
struct StepTmp { uint32_t* word; uint8_t* cls; };
inline StepTmp carve_step(Carver& c, int64_t P) {     // (a braced list is evaluated left to right)
  return {c.take<uint32_t>(1), c.take<uint8_t>((size_t)(P > 0 ? P : 1))};
}

// torch.maximum: a NaN operand gives NaN
__device__ __forceinline__ float nan_max(float a, float b) { return (a != a) ? a : ((b != b) ? b : fmaxf(a, b)); }

constexpr int kSelectRounds = 8;   // rows per select thread, 256 apart: one word access per wave and 2 048 rows

__global__ __launch_bounds__(256) void step_select_kernel(hgs_step_args A, uint32_t* __restrict__ word,
                                                          uint8_t* __restrict__ cls) {
  const int64_t base = (int64_t)blockIdx.x * (256 * kSelectRounds) + threadIdx.x;
  bool any = false;
#pragma unroll
  for (int u = 0; u < kSelectRounds; ++u) {
    const int64_t i = base + u * 256;
    // part 1: one thread per rendered (a) or listed (b) row
    if (i < A.n) {
      const int32_t rad = A.radii[i];
      int64_t r = i;
      bool vis = true;
      if (A.visible) r = A.visible[i];
      else {
        vis = rad > 0;
        if (A.indices) r = (int64_t)A.indices[i];
      }
      if (vis && r >= 0 && r < A.P) {
        A.max_radii2D[r] = nan_max(A.max_radii2D[r], (float)rad);
        if (A.accum) {
          const float gx = A.means2D_grad[3 * r], gy = A.means2D_grad[3 * r + 1];
          A.accum[r] = nan_max(sqrtf(fmaf(gx, gx, gy * gy)), A.accum[r]);
          A.denom[r] += 1.0f;
        }
      }
    }
    // part 2's selection: one thread per model row
    if (i < A.P) {
      const bool locked = i < A.lock_head || i >= A.P - A.lock_tail || (A.lock_mask && A.lock_mask[i] != 0);
      bool sel = false;
      if (A.select_all) sel = true;
      else if (A.opacity_grad && !(A.lock_opacity && locked)) sel = A.opacity_grad[i] != 0.0f;
      uint8_t c = 0;
      if (sel) c |= kSelected;
      if (locked) c |= kLocked;
      if (A.clamp && i >= A.protect_head) c |= kClampCandidate;
      cls[i] = c;
      any = any || sel;
    }
  }
  // one store per wave that selected something and does not yet see the word set (any such store writes the same 1)
  const uint64_t b = __ballot(any);
  if (b != 0 && (threadIdx.x & 63) == (unsigned)__builtin_ctzll(b)) {
    if (__hip_atomic_load(word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0u)
      __hip_atomic_store(word, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

struct StepLaunch {
  hgs_step_tensor t[kMaxTensors];
  uint32_t first_block[kMaxTensors + 1];   // block range of every tensor
};

template <typename IDX>   // element index type
__global__ __launch_bounds__(256) void step_apply_kernel(StepLaunch L, int n_tensors, int64_t P, int select_all, int clamp,
                                                         float threshold, const uint32_t* __restrict__ word,
                                                         const uint8_t* __restrict__ cls) {
  int ti = 0;
#pragma unroll
  for (int k = 1; k < kMaxTensors; ++k)
    if (k < n_tensors && blockIdx.x >= L.first_block[k]) ti = k;
  const hgs_adam_tensor& T = L.t[ti].adam;
  const int flags = L.t[ti].flags;
  const bool update = T.grad != nullptr;
  const bool dense = select_all || *word == 0u;   // no row selected: every row is (scene/OurAdam.py:214)
  const bool lockable = (flags & HGS_STEP_LOCKABLE) != 0;

  if (flags & HGS_STEP_SCALING) {
    // a row (3 floats) per thread: the clamp sees the updated row in registers
    const int64_t r = (int64_t)(blockIdx.x - L.first_block[ti]) * 256 + threadIdx.x;
    if (r >= P) return;
    const uint8_t c = cls[r];
    const bool upd = update && (dense || (c & kSelected));
    const bool cand = clamp && (c & kClampCandidate);
    if (!upd && !cand) return;
    const int64_t o = r * 3;
    float p[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) p[k] = T.param[o + k];
    if (upd) {
      const bool zero = lockable && (c & kLocked);
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        float m = T.exp_avg[o + k], v = T.exp_avg_sq[o + k];
        const float g = zero ? 0.0f : T.grad[o + k];
        adam_update(T, g, p[k], m, v);
        T.exp_avg[o + k] = m;
        T.exp_avg_sq[o + k] = v;
      }
    }
    bool big = false;
    if (cand) {
      const float e0 = expf(p[0]), e1 = expf(p[1]), e2 = expf(p[2]);
      big = fmaxf(fmaxf(e0, e1), e2) > threshold;
      if (big) {
        p[0] = logf(e0 * 0.8f);
        p[1] = logf(e1 * 0.8f);
        p[2] = logf(e2 * 0.8f);
      }
    }
    if (upd || big) {
#pragma unroll
      for (int k = 0; k < 3; ++k) T.param[o + k] = p[k];
    }
    return;
  }

  if (!update) return;
  const IDX len = (IDX)T.row_len;
  const IDX total = (IDX)P * len;
  const IDX e0 = (IDX)(blockIdx.x - L.first_block[ti]) * (256 * kPerThread) + threadIdx.x;
  // the stores could alias the loads as far as the compiler knows, so the phases are written out: class bytes, then the
  // four values of every live element, then the arithmetic and the stores
  IDX e[kPerThread];
  bool live[kPerThread], zero[kPerThread];
  float g[kPerThread], p[kPerThread], m[kPerThread], v[kPerThread];
#pragma unroll
  for (int u = 0; u < kPerThread; ++u) {
    e[u] = e0 + (IDX)(u * 256);
    live[u] = e[u] < total;
    uint8_t c = 0;
    if (live[u]) c = cls[e[u] / len];
    live[u] = live[u] && (dense || (c & kSelected));
    zero[u] = lockable && (c & kLocked);
  }
#pragma unroll
  for (int u = 0; u < kPerThread; ++u) {
    g[u] = p[u] = m[u] = v[u] = 0.0f;
    if (live[u]) {
      if (!zero[u]) g[u] = T.grad[e[u]];
      p[u] = T.param[e[u]];
      m[u] = T.exp_avg[e[u]];
      v[u] = T.exp_avg_sq[e[u]];
    }
  }
#pragma unroll
  for (int u = 0; u < kPerThread; ++u) {
    if (live[u]) {
      adam_update(T, g[u], p[u], m[u], v[u]);
      T.exp_avg[e[u]] = m[u];
      T.exp_avg_sq[e[u]] = v[u];
      T.param[e[u]] = p[u];
    }
  }
}

bool check_common(const hgs_step_args* a) {
  if (!a) { set_error("step: null args"); return false; }
  if (a->P < 0 || a->P > kMaxRows) { set_error("step: bad sizes (P = %lld outside [0, 2^31 - 1])", (long long)a->P); return false; }
  if (a->n < 0 || a->n > kMaxRows) { set_error("step: bad sizes (n = %lld outside [0, 2^31 - 1])", (long long)a->n); return false; }
  if (a->lock_head < 0 || a->lock_tail < 0 || a->lock_head > a->P || a->lock_tail > a->P - a->lock_head) {
    set_error("step: lock_head %lld + lock_tail %lld exceed %lld rows", (long long)a->lock_head, (long long)a->lock_tail,
              (long long)a->P);
    return false;
  }
  if (a->protect_head < 0 || a->protect_head > a->P) {
    set_error("step: %lld protected rows of %lld", (long long)a->protect_head, (long long)a->P);
    return false;
  }
  if (a->clamp && (!(a->clamp_threshold > 0.0f) || !(a->clamp_threshold <= 3.402823466e38f))) {
    set_error("step: the clamp threshold must be positive and finite");
    return false;
  }
  return true;
}

}  // namespace
}  // namespace hgs

using namespace hgs;

extern "C" size_t hgs_step_tmp_bytes(int64_t P) {
  if (P < 0 || P > kMaxRows) { set_error("step: bad sizes (P = %lld outside [0, 2^31 - 1])", (long long)P); return 0; }
  Carver c(nullptr);
  carve_step(c, P);
  return c.bytes(0);   // this workspace never had a slack block
}

extern "C" int hgs_step_select(const hgs_step_args* a, void* tmp, hgs_stream_t stream, int device) {
  if (!check_common(a)) return HGS_ERR_INVALID;
  if (a->n > 0) {
    if (!a->radii || !a->max_radii2D) { set_error("step: statistics need radii and max_radii2D"); return HGS_ERR_INVALID; }
    if (a->indices && a->visible) { set_error("step: pass indices (raw radii) or visible (compacted radii), not both"); return HGS_ERR_INVALID; }
    if (!a->indices && !a->visible && a->n > a->P) {
      set_error("step: %lld raw radii for %lld rows and no indices", (long long)a->n, (long long)a->P);
      return HGS_ERR_INVALID;
    }
    if ((a->accum != nullptr) != (a->denom != nullptr)) { set_error("step: accum and denom come together"); return HGS_ERR_INVALID; }
    if (a->accum && !a->means2D_grad) { set_error("step: accum needs means2D_grad"); return HGS_ERR_INVALID; }
  }
  if (!tmp) { set_error("step: null tmp"); return HGS_ERR_INVALID; }
  if (a->P == 0) return HGS_OK;
  hgs_step_args A = *a;
  if (A.n == 0) A.radii = nullptr;
  const int64_t threads = A.n > A.P ? A.n : A.P;
  HGS_HIP(hipSetDevice(device));
  hipStream_t s = static_cast<hipStream_t>(stream);
  Carver c(tmp);
  const StepTmp t = carve_step(c, A.P);
  HGS_HIP(hipMemsetAsync(t.word, 0, sizeof(uint32_t), s));
  hipLaunchKernelGGL(step_select_kernel, dim3((uint32_t)((threads + 256 * kSelectRounds - 1) / (256 * kSelectRounds))), dim3(256), 0, s, A, t.word, t.cls);
  HGS_LAUNCH_CHECK("step_select", s, false);
  return HGS_OK;
}

extern "C" int hgs_step_apply(const hgs_step_args* a, const hgs_step_tensor* tensors, int32_t n_tensors, const void* tmp,
                              hgs_stream_t stream, int device) {
  if (!check_common(a)) return HGS_ERR_INVALID;
  if (n_tensors <= 0) return HGS_OK;
  if (!tensors || n_tensors > kMaxTensors) { set_error("step: 1..%d tensors per call", kMaxTensors); return HGS_ERR_INVALID; }
  if (!tmp) { set_error("step: null tmp"); return HGS_ERR_INVALID; }
  const int64_t P = a->P;
  StepLaunch L;
  uint64_t nb = 0;
  bool wide = false, work = false;
  int n_scaling = 0;
  for (int k = 0; k < n_tensors; ++k) {
    const hgs_step_tensor& t = tensors[k];
    const hgs_adam_tensor& ad = t.adam;
    const bool scaling = (t.flags & HGS_STEP_SCALING) != 0;
    if (t.flags & ~(HGS_STEP_LOCKABLE | HGS_STEP_SCALING)) { set_error("step: tensor %d has flags %d", k, t.flags); return HGS_ERR_INVALID; }
    if (ad.row_len <= 0 || (P > 0 && (!ad.param || (ad.grad && (!ad.exp_avg || !ad.exp_avg_sq))))) {
      set_error("step: tensor %d has a null pointer or row_len <= 0", k);
      return HGS_ERR_INVALID;
    }
    if (scaling && ad.row_len != 3) { set_error("step: tensor %d: scaling rows have 3 floats, not %d", k, ad.row_len); return HGS_ERR_INVALID; }
    if (P > (int64_t)(0x7fffffffffffffffll / 4) / ad.row_len) {
      set_error("step: tensor %d: %lld rows of %d floats overflow", k, (long long)P, ad.row_len);
      return HGS_ERR_INVALID;
    }
    n_scaling += scaling ? 1 : 0;
    work = work || ad.grad != nullptr || (scaling && a->clamp);
    wide = wide || (P * (int64_t)ad.row_len >= (int64_t)0x7fffff00);
    L.t[k] = t;
    L.first_block[k] = (uint32_t)nb;
    if (scaling && (ad.grad || a->clamp)) nb += (uint64_t)((P + 255) / 256);
    else if (ad.grad) nb += (uint64_t)((P * ad.row_len + 256 * kPerThread - 1) / (256 * kPerThread));
    if (nb > 0x7fffffffull) { set_error("step: too many elements for one launch"); return HGS_ERR_INVALID; }
  }
  if (n_scaling > 1 || (a->clamp && n_scaling != 1)) {
    set_error("step: %d tensors flagged as scaling; the clamp needs exactly one", n_scaling);
    return HGS_ERR_INVALID;
  }
  if (P == 0 || !work || nb == 0) return HGS_OK;
  for (int k = n_tensors; k <= kMaxTensors; ++k) L.first_block[k] = (uint32_t)nb;
  HGS_HIP(hipSetDevice(device));
  hipStream_t s = static_cast<hipStream_t>(stream);
  Carver c(const_cast<void*>(tmp));
  const StepTmp st = carve_step(c, P);
  void (*kern)(StepLaunch, int, int64_t, int, int, float, const uint32_t*, const uint8_t*) =
      wide ? step_apply_kernel<int64_t> : step_apply_kernel<uint32_t>;
  hipLaunchKernelGGL(kern, dim3((uint32_t)nb), dim3(256), 0, s, L, n_tensors, P, a->select_all, a->clamp,
                     a->clamp_threshold, st.word, st.cls);
  HGS_LAUNCH_CHECK("step_apply", s, false);
  return HGS_OK;
}
